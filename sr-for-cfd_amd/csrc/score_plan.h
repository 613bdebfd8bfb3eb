// The summation order of the device scorer (score.hip), decided on the host: numpy's float32 `np.sum` / `np.mean` of a contiguous
// array, restated as tables.  numpy cuts the flattened array into consecutive chunks of 8192 elements (np.getbufsize(); the last
// chunk is shorter), sums every chunk with `pairwise_sum` (numpy/_core/src/umath/loops_utils.h.src) and chains the chunk sums
// from 0.f in order.  pairwise_sum of n elements:
//   n < 8          serial sum from 0.f
//   8 <= n <= 128  eight accumulators r[j] = a[j]; r[j] += a[i + j] for i = 8, 16, ... < n - n % 8;
//                  res = ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)); res += a[i] for the last n % 8 elements
//   n > 128        n2 = n / 2; n2 -= n2 % 8; pairwise(a, n2) + pairwise(a + n2, n - n2)
// A chunk is therefore a binary tree whose leaves are runs of <= 128 elements; the tree is not balanced in general (257 -> 128 +
// 129 -> 128 + (64 + 65)).  score_table(n) is that tree for one chunk length, flat: no HIP runtime calls, no kernel code.
// tools/score_plan_check.cpp links this unit alone under the sanitizers; tests/test_score_plan.py evaluates the JSON form in numpy
// float32 against np.sum.
#pragma once
#include <cstdint>
#include <string>

namespace srcfd {

constexpr int SCORE_CHUNK = 8192;        // elements numpy reduces per buffer
constexpr int SCORE_LEAF = 128;          // numpy's PW_BLOCKSIZE
constexpr int SCORE_MAX_LEAVES = 128;    // a chunk splits only above 128, so a leaf of a split chunk has >= 64 elements: <= 127 leaves
constexpr int SCORE_MAX_NODES = 256;     // leaves + inner nodes (one fewer than the leaves)
constexpr int SCORE_MAX_LEVELS = 15;     // heights 0 .. 14 fit level_start; a chunk of 8192 has 7
constexpr int64_t SCORE_MAX_ELEMS = 2560000;   // 1600 x 1600: 313 chunks

// One chunk length's tree, as the kernel reads it (plain ints: uploaded as it stands).  Node indices: [0, n_leaves) are the leaves
// in offset order (height 0); the inner nodes follow, sorted by height, so a node comes after its children and the nodes of one
// height are the range [level_start[h], level_start[h + 1]).  The root is node n_nodes - 1.
struct ScoreTable {
  int n = 0;              // chunk length
  int n_leaves = 0;
  int n_nodes = 0;
  int n_levels = 0;       // height of the root + 1
  int level_start[SCORE_MAX_LEVELS + 1] = {};
  int leaf_off[SCORE_MAX_LEAVES] = {};
  int leaf_len[SCORE_MAX_LEAVES] = {};
  int left[SCORE_MAX_NODES] = {};      // children of inner node i (unused for leaves)
  int right[SCORE_MAX_NODES] = {};
};

// Throws std::invalid_argument for n outside 1 .. SCORE_CHUNK.
ScoreTable score_table(int n);

// A field of `elems` elements: n_full chunks of SCORE_CHUNK under `full`, then one of elems % SCORE_CHUNK under `last` (n == 0: none).
struct ScorePlan {
  int64_t elems = 0;
  int n_chunks = 0;
  ScoreTable full, last;   // full.n == 0 when elems < SCORE_CHUNK; last.n == 0 when elems is a multiple of it
};
// Throws std::invalid_argument, with the bounds in the message, for elems outside 1 .. SCORE_MAX_ELEMS.
ScorePlan score_plan(int64_t elems);

// {"elems":E,"chunk":8192,"n_chunks":..,"full":{"leaves":[[off,len],..],"nodes":[[left,right,height],..]}|null,"last":{..}|null}
// "nodes" lists the inner nodes only; a child index below the number of leaves names a leaf, any other the inner node
// index - len(leaves).
std::string score_plan_json(const ScorePlan& p);

}  // namespace srcfd
