// Launch plan of the tiled super-resolution kernels (tile_plan.h).  Host only.
#include "tile_plan.h"

#include <algorithm>
#include <climits>
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

}  // namespace srcfd
