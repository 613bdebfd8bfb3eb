// Host-only walk over the launch plan of tiled super-resolution (sr-for-cfd_amd/csrc/tile_plan.cpp), built with AddressSanitizer +
// UBSan by `make -C sr-for-cfd_amd/csrc tile_plan_check`.  Over a grid of tile sizes, tile grids, channel counts, chunk bounds and
// alignments -- the largest ones the plan accepts included, where 32-bit arithmetic would overflow -- it checks what the launch
// code relies on: the chunks are whole tiles, cover [0, n) once and in order and fit the intermediate; V divides the row and the
// stated alignment; every lane of a stitch grid maps to a tile of its chunk; the refusals refuse.
// Overlapped tiling: for every lh <= 12, overlap <= lh / 2, scale <= 4 and T <= 4 it walks the per-axis source map of tile_map.h --
// the statement the blending kernel runs -- over all output rows: every row maps to in-range tiles and rows, every (tile, row) is
// used exactly once, the blended rows are exactly the O * (T - 1) expected ones, the ramps equal the formula; and it checks the
// plan's geometry, grid and intermediate for those sizes.  Prints the number of plans and of axis walks checked; exit status 1
// and a message on the first violation.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sr-for-cfd_amd/csrc/tile_plan.h"

using namespace srcfd;

static void fail(const TilePlanIn& in, const std::string& what) {
  std::fprintf(stderr, "tile_plan_check: %dx%d -> %dx%d, %d x %d tiles, C %d, max_chunk %d, model_chunk %d, align %d: %s\n", in.lh, in.lw, in.hh,
               in.hw, in.tiles_y, in.tiles_x, in.channels, in.max_chunk, in.model_chunk, in.align_bytes, what.c_str());
  std::exit(1);
}

static void check(const TilePlanIn& in) {
  const TilePlan p = tile_plan(in);
  const int C = in.channels;
  if ((int64_t)p.n != (int64_t)in.tiles_y * in.tiles_x * C) fail(in, "n");
  if (p.chunk < C || p.chunk % C || p.chunk > p.n) fail(in, "chunk " + std::to_string(p.chunk));
  const int bound = in.max_chunk > 0 ? in.max_chunk : in.model_chunk;
  if (bound >= C && p.chunk > bound) fail(in, "chunk above its bound");
  if (bound >= C && p.chunk < p.n && p.chunk + C <= bound) fail(in, "not the largest multiple of C under the bound");
  if ((int64_t)p.n_chunks != ((int64_t)p.n + p.chunk - 1) / p.chunk) fail(in, "chunk count");
  // first, a middle and the last chunks: in order, whole tiles, the last one ends at n
  for (int i : {0, p.n_chunks / 2, p.n_chunks - 1}) {
    const int first = p.chunk_first(i), count = p.chunk_count(i);
    if ((int64_t)first != (int64_t)i * p.chunk || count < C || count % C || count > p.chunk) fail(in, "chunk " + std::to_string(i));
    if (i == p.n_chunks - 1 && (int64_t)first + count != p.n) fail(in, "the last chunk does not end at n");
    if (i < p.n_chunks - 1 && count != p.chunk) fail(in, "a short chunk that is not the last");
    const unsigned grid = tile_stitch_grid(p, count);
    if ((int64_t)grid != (int64_t)(count / C) * p.stitch_blocks_per_tile) fail(in, "stitch grid");
  }
  if (p.v != 1 && p.v != 2 && p.v != 4) fail(in, "V");
  if (in.hw % p.v || (p.v > 1 && (in.align_bytes < 4 * p.v || (in.align_bytes < 16 && in.align_bytes % (4 * p.v))))) fail(in, "V does not divide the row or the alignment");
  if (p.v < 4 && in.hw % (2 * p.v) == 0 && in.align_bytes >= 16) fail(in, "a wider V fits");
  if (p.stitch_items != in.hh * (in.hw / p.v)) fail(in, "items per tile");
  if ((int64_t)p.stitch_blocks_per_tile * TILE_BLOCK < p.stitch_items || (int64_t)(p.stitch_blocks_per_tile - 1) * TILE_BLOCK >= p.stitch_items) fail(in, "blocks per tile");
  if (p.intermediate_bytes != (size_t)p.chunk * in.hh * in.hw * 4) fail(in, "intermediate bytes");
  if (p.cut_grid < 1 || p.cut_grid > (1u << 20)) fail(in, "cut grid");
  if (tile_plan_json(p).empty()) fail(in, "empty JSON");
}

// one axis of an overlapped tiling: lh coarse cells per tile, overlap o, integer scale s, T tiles
static void check_axis(int lh, int o, int s, int T) {
  auto bad = [&](const std::string& what) {
    std::fprintf(stderr, "tile_plan_check: axis lh %d overlap %d scale %d T %d: %s\n", lh, o, s, T, what.c_str());
    std::exit(1);
  };
  TilePlanIn in;
  in.lh = lh; in.lw = lh; in.hh = lh * s; in.hw = lh * s; in.tiles_y = T; in.tiles_x = 1; in.channels = 3; in.model_chunk = 5;
  in.overlap_y = o; in.overlap_x = 0;
  const TilePlan p = tile_plan(in);
  const int S = (lh - o) * s, O = o * s, hh = lh * s, rows = T * S + O;
  if (p.stride_y != lh - o || p.stride_x != lh || p.field_h != T * (lh - o) + o || p.field_w != lh) fail(in, "coarse geometry");
  if (o > 0) {
    if (!p.blended || p.fine_stride_y != S || p.fine_overlap_y != O || p.out_h != rows || p.out_w != hh || p.fine_stride_x != hh || p.fine_overlap_x != 0) fail(in, "fine geometry");
    if (p.intermediate_bytes != (size_t)p.n * hh * hh * 4) fail(in, "the intermediate does not hold all n samples");
    if ((int64_t)p.blend_blocks_per_row * TILE_BLOCK < p.out_w || (int64_t)(p.blend_blocks_per_row - 1) * TILE_BLOCK >= p.out_w) fail(in, "blend blocks per row");
    if ((int64_t)p.blend_grid != (int64_t)p.out_h * p.blend_blocks_per_row) fail(in, "blend grid");
    if ((int)p.ramp_y.size() != O || !p.ramp_x.empty()) fail(in, "ramp lengths");
    for (int j = 0; j < O; ++j) {
      const float w = (float)((j + 0.5) / (double)O);
      if (p.ramp_y[(size_t)j] != w || !(w > 0.f && w < 1.f) || (j && !(p.ramp_y[(size_t)j] > p.ramp_y[(size_t)j - 1]))) fail(in, "ramp " + std::to_string(j));
    }
    if (tile_plan_json_overlap(p).find("\"stitch\":null") == std::string::npos) fail(in, "JSON of a blended plan");
  } else if (p.blended || p.blend_grid || !p.ramp_y.empty() || p.intermediate_bytes != (size_t)p.chunk * hh * hh * 4) {
    fail(in, "overlap 0 is not today's plan");
  }
  std::vector<int> used((size_t)T * hh, 0);
  int blended = 0;
  for (int R = 0; R < rows; ++R) {
    const TileAxisSrc a = tile_axis_src(R, T, S, O);
    if (a.t1 < 0 || a.t1 >= T || a.r1 < 0 || a.r1 >= hh) bad("row " + std::to_string(R) + ": source outside the tiles");
    ++used[(size_t)a.t1 * hh + a.r1];
    if (a.t0 >= 0) {
      if (a.t0 != a.t1 - 1 || a.r0 < 0 || a.r0 >= hh || a.j < 0 || a.j >= O) bad("row " + std::to_string(R) + ": blended source outside the tiles or the ramp");
      if (a.t0 * S + a.r0 != R || a.t1 * S + a.r1 != R) bad("row " + std::to_string(R) + ": the two sources are not this row");
      if (R < a.t1 * S || R >= a.t1 * S + O || a.j != R - a.t1 * S) bad("row " + std::to_string(R) + ": blended outside its zone");
      ++used[(size_t)a.t0 * hh + a.r0];
      ++blended;
    } else if (a.j != -1 || a.t1 * S + a.r1 != R) {
      bad("row " + std::to_string(R) + ": copied from another row");
    }
  }
  for (size_t i = 0; i < used.size(); ++i)
    if (used[i] != 1) bad("tile " + std::to_string(i / hh) + " row " + std::to_string(i % hh) + " is used " + std::to_string(used[i]) + " times");
  if (blended != O * (T - 1)) bad(std::to_string(blended) + " blended rows, expected " + std::to_string(O * (T - 1)));
}

static void must_refuse(const TilePlanIn& in, const char* what) {
  try {
    tile_plan(in);
  } catch (const std::invalid_argument&) {
    return;
  }
  fail(in, std::string("accepted: ") + what);
}

int main() {
  long checked = 0;
  const int sides[][2] = {{1, 1}, {7, 5}, {10, 10}, {6, 50}, {20, 20}, {3, 400}, {400, 400}, {1600, 1600}};
  const int grids[][2] = {{1, 1}, {2, 3}, {4, 4}, {1, 7}, {16, 16}, {160, 160}};
  for (const auto& hs : sides)
    for (const auto& g : grids)
      for (int C = 1; C <= TILE_MAX_CHANNELS; ++C)
        for (int align : {4, 8, 16, 64, 256}) {
          const int n = g[0] * g[1] * C;
          for (int max_chunk : {0, 1, C, 2 * C, 2 * C + 1, n - 1, n, n + 5}) {
            TilePlanIn in;
            in.lh = in.lw = 10; in.hh = hs[0]; in.hw = hs[1];
            in.tiles_y = g[0]; in.tiles_x = g[1]; in.channels = C; in.max_chunk = max_chunk; in.model_chunk = 1024; in.align_bytes = align;
            check(in);
            ++checked;
          }
        }
  {   // the largest sample counts: 46340^2 = 2 147 395 600 tiles of one channel, and INT_MAX / 8 rounded down with eight
    TilePlanIn in;
    in.lh = in.lw = 10; in.hh = in.hw = 10; in.model_chunk = 1024;
    in.tiles_y = in.tiles_x = 46340; in.channels = 1;
    check(in); ++checked;
    in.max_chunk = 1;
    check(in); ++checked;      // 2^31-odd chunks: nothing is materialised
    in.tiles_y = 16384; in.tiles_x = 16383; in.channels = 8; in.max_chunk = 0;
    check(in); ++checked;
    in.max_chunk = INT_MAX;      // one chunk of all 2 147 352 576 samples
    check(in); ++checked;
    in.max_chunk = 0;
    in.tiles_x = 16384;
    must_refuse(in, "2^31 samples");
    in.tiles_y = in.tiles_x = 46341; in.channels = 1;
    must_refuse(in, "more than INT_MAX samples");
    in.tiles_y = in.tiles_x = INT_MAX; in.channels = 8;
    must_refuse(in, "INT_MAX x INT_MAX tiles");
  }
  TilePlanIn ok;
  ok.lh = ok.lw = 10; ok.hh = ok.hw = 400; ok.tiles_y = ok.tiles_x = 4; ok.channels = 3; ok.model_chunk = 48;
  check(ok); ++checked;
  { TilePlanIn b = ok; b.channels = 0; must_refuse(b, "0 channels"); }
  { TilePlanIn b = ok; b.channels = 9; must_refuse(b, "9 channels"); }
  { TilePlanIn b = ok; b.tiles_y = 0; must_refuse(b, "TY 0"); }
  { TilePlanIn b = ok; b.tiles_x = -3; must_refuse(b, "TX -3"); }
  { TilePlanIn b = ok; b.in_channels = 3; must_refuse(b, "3 input channels"); }
  { TilePlanIn b = ok; b.out_channels = 2; must_refuse(b, "2 output channels"); }
  { TilePlanIn b = ok; b.hh = 0; must_refuse(b, "empty output"); }
  { TilePlanIn b = ok; b.hh = b.hw = 40000; must_refuse(b, "a tile of 1.6e9 elements"); }
  { TilePlanIn b = ok; b.model_chunk = 0; must_refuse(b, "no model chunk and no max_chunk"); }
  long axes = 0;
  for (int lh = 1; lh <= 12; ++lh)
    for (int o = 0; 2 * o <= lh; ++o)
      for (int s = 1; s <= 4; ++s)
        for (int T = 1; T <= 4; ++T) {
          check_axis(lh, o, s, T);
          ++axes;
        }
  { TilePlanIn b = ok; b.overlap_y = -1; must_refuse(b, "overlap -1"); }
  { TilePlanIn b = ok; b.overlap_x = 6; must_refuse(b, "overlap above half a tile"); }
  { TilePlanIn b = ok; b.overlap_y = INT_MAX; must_refuse(b, "overlap INT_MAX"); }
  { TilePlanIn b = ok; b.overlap_y = 2; b.hh = 405; must_refuse(b, "an output that is no multiple of the input"); }
  { TilePlanIn b = ok; b.overlap_y = 1; b.lh = 32768; b.hh = 65536; b.lw = 4; b.hw = 8; b.tiles_y = 40000; b.tiles_x = 1; must_refuse(b, "an output side above INT_MAX"); }
  { TilePlanIn b = ok; b.overlap_y = b.overlap_x = 1; b.lh = b.lw = 4; b.tiles_y = b.tiles_x = 30000; b.channels = 1; must_refuse(b, "a blending stitch above one launch"); }
  { TilePlanIn b = ok; b.overlap_y = 5; b.overlap_x = 5; check(b); ++checked; }   // half a tile; the chunk keys are today's
  std::printf("%ld %ld\n", checked, axes);
  return 0;
}
