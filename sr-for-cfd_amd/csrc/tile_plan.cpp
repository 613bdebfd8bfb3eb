// Launch plan of the tiled super-resolution kernels (tile_plan.h).  Host only.
#include "tile_plan.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <stdexcept>

namespace srcfd {

int tile_stitch_v(int hw, int align_bytes) {
  for (int v = 4; v > 1; v >>= 1)
    if (hw % v == 0 && align_bytes >= 4 * v && align_bytes % (4 * v) == 0) return v;
  return 1;
}

unsigned tile_stitch_grid(const TilePlan& p, int samples) {
  const int64_t grid = (int64_t)(samples / p.in.channels) * p.stitch_blocks_per_tile;
  if (grid > INT_MAX) throw std::invalid_argument("tiles: a stitch of " + std::to_string(samples) + " samples needs " + std::to_string(grid) + " workgroups, more than one launch takes");
  return (unsigned)grid;
}

TilePlan tile_plan(const TilePlanIn& in) {
  auto refuse = [](const std::string& why) { throw std::invalid_argument("tiles: " + why); };
  if (in.channels < 1 || in.channels > TILE_MAX_CHANNELS)
    refuse(std::to_string(in.channels) + " channels; supported: 1 .. " + std::to_string(TILE_MAX_CHANNELS));
  if (in.tiles_y < 1 || in.tiles_x < 1) refuse("a grid of " + std::to_string(in.tiles_y) + " x " + std::to_string(in.tiles_x) + " tiles; at least 1 x 1 is needed");
  if (in.in_channels != 1 || in.out_channels != 1)
    refuse("the model maps " + std::to_string(in.in_channels) + " -> " + std::to_string(in.out_channels) +
           " channels; every component of a tile is one sample of a one-channel model");
  if (in.lh < 1 || in.lw < 1 || in.hh < 1 || in.hw < 1) refuse("a tile of " + std::to_string(in.lh) + " x " + std::to_string(in.lw) + " -> " + std::to_string(in.hh) + " x " + std::to_string(in.hw));
  if ((int64_t)in.hh * in.hw > INT_MAX / 2 || (int64_t)in.lh * in.lw > INT_MAX / 2) refuse("a tile of more than 2^30 elements");
  const int64_t tiles = (int64_t)in.tiles_y * in.tiles_x;
  const int64_t n = tiles > INT_MAX ? tiles : tiles * in.channels;   // no 64-bit overflow on the way to the refusal
  if (n > INT_MAX) refuse(std::string(tiles > INT_MAX && in.channels > 1 ? "at least " : "") + std::to_string(n) + " tile samples (" + std::to_string(in.tiles_y) + " x " + std::to_string(in.tiles_x) + " x " + std::to_string(in.channels) + "); at most " + std::to_string(INT_MAX));
  if (in.max_chunk <= 0 && in.model_chunk < 1) refuse("the model reports no unchunked call size");
  const int oy = in.overlap_y, ox = in.overlap_x;
  if (oy < 0 || ox < 0) refuse("an overlap of (" + std::to_string(oy) + ", " + std::to_string(ox) + "); an overlap is 0 or more coarse cells");
  if (2 * (int64_t)oy > in.lh || 2 * (int64_t)ox > in.lw)
    refuse("an overlap of (" + std::to_string(oy) + ", " + std::to_string(ox) + ") on " + std::to_string(in.lh) + " x " + std::to_string(in.lw) +
           " tiles; at most half a tile (2 * overlap <= side), so that a point lies in at most two tiles per axis");
  const bool blended = oy > 0 || ox > 0;
  if (blended && (in.hh % in.lh || in.hw % in.lw))
    refuse("an overlap needs an output that is a whole multiple of the input on both axes; the model maps " + std::to_string(in.lh) + " x " +
           std::to_string(in.lw) + " -> " + std::to_string(in.hh) + " x " + std::to_string(in.hw));

  TilePlan p;
  p.in = in;
  p.in.align_bytes = std::min(std::max(in.align_bytes, 1), 16);
  p.n = (int)n;
  // the largest multiple of C not above the bound; a bound below C still takes one whole tile: a chunk never splits the C components
  const int bound = in.max_chunk > 0 ? in.max_chunk : in.model_chunk;
  p.chunk = (int)std::min<int64_t>(n, std::max(bound / in.channels, 1) * (int64_t)in.channels);
  p.n_chunks = (int)((n + p.chunk - 1) / p.chunk);
  p.v = tile_stitch_v(in.hw, p.in.align_bytes);
  const int64_t cut_elems = n * in.lh * in.lw;
  p.cut_grid = (unsigned)std::min<int64_t>((cut_elems + TILE_BLOCK - 1) / TILE_BLOCK, 1 << 20);
  p.stitch_items = in.hh * (in.hw / p.v);
  p.stitch_blocks_per_tile = (unsigned)((p.stitch_items + TILE_BLOCK - 1) / TILE_BLOCK);
  p.intermediate_bytes = (size_t)p.chunk * in.hh * in.hw * sizeof(float);
  (void)tile_stitch_grid(p, p.chunk);   // refuses a chunk that one launch cannot stitch
  p.stride_y = in.lh - oy; p.stride_x = in.lw - ox;
  p.fine_stride_y = in.hh; p.fine_stride_x = in.hw;
  if (!blended) {   // today's geometry; the sizes below are informative only and saturate rather than refuse
    p.field_h = (int)std::min<int64_t>((int64_t)in.tiles_y * in.lh, INT_MAX); p.field_w = (int)std::min<int64_t>((int64_t)in.tiles_x * in.lw, INT_MAX);
    p.out_h = (int)std::min<int64_t>((int64_t)in.tiles_y * in.hh, INT_MAX); p.out_w = (int)std::min<int64_t>((int64_t)in.tiles_x * in.hw, INT_MAX);
    return p;
  }
  p.blended = true;
  const int sy = in.hh / in.lh, sx = in.hw / in.lw;
  p.fine_stride_y = p.stride_y * sy; p.fine_stride_x = p.stride_x * sx;
  p.fine_overlap_y = oy * sy; p.fine_overlap_x = ox * sx;
  const int64_t out_h = (int64_t)in.tiles_y * p.fine_stride_y + p.fine_overlap_y, out_w = (int64_t)in.tiles_x * p.fine_stride_x + p.fine_overlap_x;
  if (out_h > INT_MAX || out_w > INT_MAX) refuse("an overlapped output of " + std::to_string(out_h) + " x " + std::to_string(out_w) + "; a side is at most " + std::to_string(INT_MAX));
  p.out_h = (int)out_h; p.out_w = (int)out_w;
  p.field_h = in.tiles_y * p.stride_y + oy; p.field_w = in.tiles_x * p.stride_x + ox;   // below the output's sides
  // all n samples stay resident; n <= INT_MAX and a plane <= 2^30 elements keep the product within 2^61, which this states in code
  const int64_t plane = (int64_t)in.hh * in.hw;
  if (n > (INT64_MAX / 4) / plane || out_h * out_w > (INT64_MAX / 4) / in.channels)
    refuse(std::to_string(n) + " samples of " + std::to_string(plane) + " elements; the 64-bit element offsets of the blending stitch do not hold them");
  p.intermediate_bytes = (size_t)n * (size_t)plane * sizeof(float);
  p.blend_blocks_per_row = (unsigned)((out_w + TILE_BLOCK - 1) / TILE_BLOCK);
  const int64_t blend_grid = out_h * p.blend_blocks_per_row;
  if (blend_grid > INT_MAX)
    refuse("a blending stitch of " + std::to_string(out_h) + " x " + std::to_string(out_w) + " needs " + std::to_string(blend_grid) + " workgroups, more than one launch takes");
  p.blend_grid = (unsigned)blend_grid;
  auto ramp = [](int O) {
    std::vector<float> w((size_t)O);
    for (int j = 0; j < O; ++j) w[(size_t)j] = (float)((j + 0.5) / (double)O);
    return w;
  };
  p.ramp_y = ramp(p.fine_overlap_y);
  p.ramp_x = ramp(p.fine_overlap_x);
  return p;
}

std::string tile_plan_json(const TilePlan& p) {
  std::string s = "{\"n\":" + std::to_string(p.n) + ",\"chunk\":" + std::to_string(p.chunk) + ",\"n_chunks\":" + std::to_string(p.n_chunks) + ",\"chunks\":";
  const bool list = p.n_chunks <= (1 << 16);
  std::string grids;
  if (list) {
    s += '[';
    grids = "[";
    for (int i = 0; i < p.n_chunks; ++i) {
      if (i) { s += ','; grids += ','; }
      s += '[' + std::to_string(p.chunk_first(i)) + ',' + std::to_string(p.chunk_count(i)) + ']';
      grids += std::to_string(tile_stitch_grid(p, p.chunk_count(i)));
    }
    s += ']';
    grids += ']';
  } else {
    s += "null";
    grids = "null";
  }
  s += ",\"v\":" + std::to_string(p.v) + ",\"cut\":{\"grid\":" + std::to_string(p.cut_grid) + ",\"block\":" + std::to_string(TILE_BLOCK) + "}";
  s += ",\"stitch\":{\"block\":" + std::to_string(TILE_BLOCK) + ",\"items_per_tile\":" + std::to_string(p.stitch_items) + ",\"blocks_per_tile\":" +
       std::to_string(p.stitch_blocks_per_tile) + ",\"grid\":" + grids + "}";
  s += ",\"intermediate_bytes\":" + std::to_string(p.intermediate_bytes) + "}";
  return s;
}

std::string tile_plan_json_overlap(const TilePlan& p) {
  std::string s = tile_plan_json(p);
  auto pair = [](int64_t a, int64_t b) { return '[' + std::to_string(a) + ',' + std::to_string(b) + ']'; };
  if (p.blended) {   // "stitch":{..} -> "stitch":null: the object holds no nested braces
    const size_t at = s.find("\"stitch\":{"), end = s.find('}', at);
    s.replace(at, end + 1 - at, "\"stitch\":null");
  }
  s.pop_back();
  s += ",\"overlap\":" + pair(p.in.overlap_y, p.in.overlap_x) + ",\"stride\":" + pair(p.stride_y, p.stride_x) + ",\"field\":" + pair(p.field_h, p.field_w) +
       ",\"out\":" + pair(p.out_h, p.out_w) + ",\"blend\":";
  if (p.blended)
    s += "{\"grid\":" + std::to_string(p.blend_grid) + ",\"block\":" + std::to_string(TILE_BLOCK) + ",\"blocks_per_row\":" + std::to_string(p.blend_blocks_per_row) +
         ",\"ramp\":" + pair(p.fine_overlap_y, p.fine_overlap_x) + "}";
  else
    s += "null";
  return s + "}";
}

}  // namespace srcfd
