// Host-only walk over the scorer's summation plan (sr-for-cfd_amd/csrc/score_plan.cpp), built with AddressSanitizer + UBSan by
// `make -C sr-for-cfd_amd/csrc score_plan_check`.  For every chunk length 1 .. 8192, every field size 1 .. 20 000 and the
// family's field sizes up to 1600 x 1600 it checks what the kernel relies on: the leaves tile [0, n) in order, no leaf is longer
// than 128, every child precedes its parent and lies one or more levels below it, every node but the root has exactly one
// parent, the levels are contiguous ranges and the root is the last node.  Prints the number of plans checked; exit status 1 and
// a message on the first violation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sr-for-cfd_amd/csrc/score_plan.h"

using namespace srcfd;

static void fail(int n, const std::string& what) {
  std::fprintf(stderr, "score_plan_check: chunk length %d: %s\n", n, what.c_str());
  std::exit(1);
}

static void check_table(const ScoreTable& t, int n) {
  if (t.n != n) fail(n, "table is for another length");
  if (t.n_leaves < 1 || t.n_leaves > SCORE_MAX_LEAVES - 1) fail(n, "leaf count " + std::to_string(t.n_leaves));
  if (t.n_nodes != 2 * t.n_leaves - 1 || t.n_nodes > SCORE_MAX_NODES) fail(n, "node count");
  int at = 0;
  for (int i = 0; i < t.n_leaves; ++i) {
    if (t.leaf_off[i] != at) fail(n, "leaves do not tile [0, n) in order");
    if (t.leaf_len[i] < 1 || t.leaf_len[i] > SCORE_LEAF) fail(n, "leaf length " + std::to_string(t.leaf_len[i]));
    at += t.leaf_len[i];
  }
  if (at != n) fail(n, "leaves end at " + std::to_string(at));
  if (t.n_levels < 1 || t.n_levels > SCORE_MAX_LEVELS) fail(n, "level count");
  if (t.level_start[0] != 0 || t.level_start[1] != t.n_leaves || t.level_start[t.n_levels] != t.n_nodes) fail(n, "level ranges");
  std::vector<int> height(t.n_nodes, 0), parents(t.n_nodes, 0);
  for (int h = 1; h < t.n_levels; ++h) {
    if (t.level_start[h + 1] <= t.level_start[h]) fail(n, "empty level");
    for (int i = t.level_start[h]; i < t.level_start[h + 1]; ++i) {
      const int l = t.left[i], r = t.right[i];
      if (l < 0 || r < 0 || l >= i || r >= i || l == r) fail(n, "a child does not precede its parent");
      if (height[l] >= h || height[r] >= h || (height[l] != h - 1 && height[r] != h - 1)) fail(n, "heights");
      height[i] = h;
      ++parents[l];
      ++parents[r];
    }
  }
  for (int i = 0; i < t.n_nodes; ++i)
    if (parents[i] != (i == t.n_nodes - 1 ? 0 : 1)) fail(n, "not a single tree rooted at the last node");
}

int main() {
  long checked = 0;
  for (int n = 1; n <= SCORE_CHUNK; ++n, ++checked) check_table(score_table(n), n);
  std::vector<int64_t> sizes;
  for (int64_t e = 1; e <= 20000; ++e) sizes.push_back(e);
  for (int64_t side : {10, 20, 50, 80, 100, 400, 800, 1600}) sizes.push_back(side * side);
  sizes.push_back(SCORE_MAX_ELEMS);
  for (int64_t e : sizes) {
    const ScorePlan p = score_plan(e);
    const int n_full = (int)(e / SCORE_CHUNK), rem = (int)(e % SCORE_CHUNK);
    if (p.elems != e || p.n_chunks != n_full + (rem ? 1 : 0)) fail(rem, "chunk count of " + std::to_string(e) + " elements");
    if ((p.full.n != 0) != (n_full != 0) || (p.last.n != 0) != (rem != 0)) fail(rem, "tables present for " + std::to_string(e) + " elements");
    if (n_full) check_table(p.full, SCORE_CHUNK);
    if (rem) check_table(p.last, rem);
    if (score_plan_json(p).empty()) fail(rem, "empty JSON");
    ++checked;
  }
  for (int64_t bad : {(int64_t)0, (int64_t)-1, SCORE_MAX_ELEMS + 1}) {
    try {
      score_plan(bad);
      fail(0, "score_plan accepted " + std::to_string(bad) + " elements");
    } catch (const std::invalid_argument&) {
    }
  }
  std::printf("%ld\n", checked);
  return 0;
}
