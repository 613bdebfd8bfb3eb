// The launch plan of tiled super-resolution on the device (tiles.hip), decided on the host: a (TY*lh, TX*lw, C) coarse field is
// cut into TY x TX tiles, every component of every tile is one sample of a one-channel lh x lw -> hh x hw model, and the samples'
// planar results are stitched into the channel-interleaved (TY*hh, TX*hw, C) field (BASELINE config 5;
// pipeline.tiled_super_resolution is the host form and fixes the sample order s = (ty*TX + tx)*C + c).
// tile_plan() answers everything the launch code needs and nothing else does: the sample count, the chunks the network is run
// in, the vector width of the stitch, the grids of both kernels, the bytes of the planar intermediate.  No HIP runtime calls, no
// kernel code; tests/test_tiled_plan.py reads the JSON form.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace srcfd {

constexpr int TILE_MAX_CHANNELS = 8;
constexpr int TILE_BLOCK = 256;   // threads per workgroup of both kernels

struct TilePlanIn {
  int lh = 0, lw = 0, in_channels = 1;     // the model's input (h, w, c)
  int hh = 0, hw = 0, out_channels = 1;    // the model's output
  int tiles_y = 0, tiles_x = 0, channels = 0;
  int max_chunk = 0;      // <= 0: none given
  int model_chunk = 0;    // the model's largest unchunked call for n samples (srcfd_model_workspace's return value)
  int align_bytes = 16;   // what both base pointers of the stitch (intermediate and output) are aligned to; 16 and more count as 16
};

struct TilePlan {
  TilePlanIn in;
  int n = 0;            // samples: TY * TX * C
  int chunk = 0;        // samples per network call, a multiple of C; chunk i is [i * chunk, min(n, (i + 1) * chunk))
  int n_chunks = 0;
  int v = 1;            // x-consecutive floats per lane and source row of the stitch: 4, 2 or 1
  unsigned cut_grid = 0;          // tiles_cut: grid-stride over n * lh * lw elements
  int stitch_items = 0;           // lanes with work per tile: hh * (hw / v)
  unsigned stitch_blocks_per_tile = 0;
  size_t intermediate_bytes = 0;  // chunk * hh * hw * 4
  int chunk_first(int i) const { return i * chunk; }
  int chunk_count(int i) const { return n - i * chunk < chunk ? n - i * chunk : chunk; }
};

// The widest of 4, 2, 1 with hw % V == 0 and both base pointers 4 V-byte aligned.  A lane's output piece is V * C floats at an
// offset that is a multiple of V * C floats, so its alignment follows from the base pointer's.
int tile_stitch_v(int hw, int align_bytes);
// Workgroups of the stitch of `samples` samples (a multiple of C): one tile per blocks_per_tile workgroups.  Throws
// std::invalid_argument when the grid would pass INT_MAX.
unsigned tile_stitch_grid(const TilePlan& p, int samples);

// Throws std::invalid_argument with the reason: C outside 1 .. 8, TY or TX < 1, more than INT_MAX samples, a model whose input or
// output has more than one channel, sizes below 1, model_chunk < 1.
TilePlan tile_plan(const TilePlanIn& in);

// {"n":N,"chunk":K,"n_chunks":M,"chunks":[[first,count],..]|null,"v":V,"cut":{"grid":G,"block":256},
//  "stitch":{"block":256,"items_per_tile":I,"blocks_per_tile":B,"grid":[one per chunk]|null},"intermediate_bytes":Y}
// The two lists are null above 65536 chunks (they are regular: every chunk but the last has K samples).
std::string tile_plan_json(const TilePlan& p);

}  // namespace srcfd
