// numpy's float32 summation order as tables (score_plan.h).  Host only.
#include "score_plan.h"

#include <algorithm>
#include <stdexcept>
#include <vector>

namespace srcfd {

namespace {

struct Node {
  int left, right, height;
};

// pairwise_sum's recursion on [off, off + n): returns the index of the subtree's root in `leaves` (height 0) or, offset by
// 1 << 20, in `inner`
constexpr int INNER = 1 << 20;
int split(int off, int n, std::vector<std::pair<int, int>>& leaves, std::vector<Node>& inner) {
  if (n <= SCORE_LEAF) {
    leaves.push_back({off, n});
    return (int)leaves.size() - 1;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  const int l = split(off, n2, leaves, inner);
  const int r = split(off + n2, n - n2, leaves, inner);
  auto height = [&](int i) { return i >= INNER ? inner[i - INNER].height : 0; };
  inner.push_back({l, r, std::max(height(l), height(r)) + 1});
  return INNER + (int)inner.size() - 1;
}

}  // namespace

ScoreTable score_table(int n) {
  if (n < 1 || n > SCORE_CHUNK) throw std::invalid_argument("score_table: chunk length " + std::to_string(n) + " outside 1 .. " + std::to_string(SCORE_CHUNK));
  std::vector<std::pair<int, int>> leaves;
  std::vector<Node> inner;
  split(0, n, leaves, inner);
  const int nl = (int)leaves.size(), ni = (int)inner.size();
  if (nl > SCORE_MAX_LEAVES || nl + ni > SCORE_MAX_NODES) throw std::logic_error("score_table: more leaves than the table holds");
  // inner nodes by height (stable: recursion order inside one height), so that every height is one contiguous range
  std::vector<int> order(ni);
  for (int i = 0; i < ni; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return inner[a].height < inner[b].height; });
  std::vector<int> where(ni);
  for (int k = 0; k < ni; ++k) where[order[k]] = nl + k;
  auto index = [&](int i) { return i >= INNER ? where[i - INNER] : i; };
  ScoreTable t;
  t.n = n;
  t.n_leaves = nl;
  t.n_nodes = nl + ni;
  for (int i = 0; i < nl; ++i) { t.leaf_off[i] = leaves[i].first; t.leaf_len[i] = leaves[i].second; }
  const int top = ni ? inner[order[ni - 1]].height : 0;
  if (top + 1 > SCORE_MAX_LEVELS) throw std::logic_error("score_table: tree higher than the table holds");
  t.n_levels = top + 1;
  t.level_start[0] = 0;
  t.level_start[1] = nl;
  int h = 1;
  for (int k = 0; k < ni; ++k) {
    const Node& nd = inner[order[k]];
    while (h < nd.height) t.level_start[++h] = nl + k;
    t.left[nl + k] = index(nd.left);
    t.right[nl + k] = index(nd.right);
  }
  for (int g = h + 1; g <= SCORE_MAX_LEVELS; ++g) t.level_start[g] = nl + ni;
  if (!ni) for (int g = 1; g <= SCORE_MAX_LEVELS; ++g) t.level_start[g] = nl;
  return t;
}

ScorePlan score_plan(int64_t elems) {
  if (elems < 1 || elems > SCORE_MAX_ELEMS)
    throw std::invalid_argument("score: " + std::to_string(elems) + " elements per field; supported: 1 .. " + std::to_string(SCORE_MAX_ELEMS) + " (1600 x 1600)");
  ScorePlan p;
  p.elems = elems;
  const int n_full = (int)(elems / SCORE_CHUNK), rem = (int)(elems % SCORE_CHUNK);
  p.n_chunks = n_full + (rem ? 1 : 0);
  if (n_full) p.full = score_table(SCORE_CHUNK);
  if (rem) p.last = score_table(rem);
  return p;
}

static void table_json(const ScoreTable& t, std::string& s) {
  if (!t.n) { s += "null"; return; }
  s += "{\"leaves\":[";
  for (int i = 0; i < t.n_leaves; ++i) {
    if (i) s += ',';
    s += '[' + std::to_string(t.leaf_off[i]) + ',' + std::to_string(t.leaf_len[i]) + ']';
  }
  s += "],\"nodes\":[";
  int h = 1;
  for (int i = t.n_leaves; i < t.n_nodes; ++i) {
    while (i >= t.level_start[h + 1]) ++h;
    if (i > t.n_leaves) s += ',';
    s += '[' + std::to_string(t.left[i]) + ',' + std::to_string(t.right[i]) + ',' + std::to_string(h) + ']';
  }
  s += "]}";
}

std::string score_plan_json(const ScorePlan& p) {
  std::string s = "{\"elems\":" + std::to_string(p.elems) + ",\"chunk\":" + std::to_string(SCORE_CHUNK) + ",\"n_chunks\":" + std::to_string(p.n_chunks) + ",\"full\":";
  table_json(p.full, s);
  s += ",\"last\":";
  table_json(p.last, s);
  s += '}';
  return s;
}

}  // namespace srcfd
