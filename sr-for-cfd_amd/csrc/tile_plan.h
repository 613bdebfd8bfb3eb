// The launch plan of tiled super-resolution on the device (tiles.hip), decided on the host: a (TY*lh, TX*lw, C) coarse field is
// cut into TY x TX tiles, every component of every tile is one sample of a one-channel lh x lw -> hh x hw model, and the samples'
// planar results are stitched into the channel-interleaved (TY*hh, TX*hw, C) field (BASELINE config 5;
// pipeline.tiled_super_resolution is the host form and fixes the sample order s = (ty*TX + tx)*C + c).
// tile_plan() answers everything the launch code needs and nothing else does: the sample count, the chunks the network is run
// in, the vector width of the stitch, the grids of both kernels, the bytes of the planar intermediate.  No HIP runtime calls, no
// kernel code; tests/test_tiled_plan.py reads the JSON form.
//
// Overlapped tiling (overlap_y, overlap_x coarse cells, at most half a tile; include/srcfd.h has the definition): the tiles start
// every lh - oy rows and lw - ox columns of a (TY*(lh-oy) + oy, TX*(lw-ox) + ox, C) field, the output has that size times the
// model's integer scale, and the overlaps are blended with a linear ramp.  The plan then also holds the strides, the output size,
// the two ramp tables (computed here, uploaded by the tiler: the device never divides) and the grid of the blending stitch, and the
// intermediate holds ALL n samples, since a blended pixel may need tiles of different chunks: the chunks predict into their own
// rows of it and one blending stitch follows the last.  tile_map.h states where an output row comes from, for both sides.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "tile_map.h"

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
  int overlap_y = 0, overlap_x = 0;   // coarse cells neighbouring tiles share; 0 <= 2 * o <= the tile's side
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
  size_t intermediate_bytes = 0;  // chunk * hh * hw * 4; with an overlap n * hh * hw * 4
  // overlapped tiling; with overlap 0 the strides are the tile sides and nothing below is used by a launch
  bool blended = false;           // overlap_y > 0 or overlap_x > 0: the blending stitch runs instead of the per-chunk one
  int stride_y = 0, stride_x = 0;             // coarse: lh - oy, lw - ox
  int fine_stride_y = 0, fine_stride_x = 0;   // Sy = stride_y * sy, Sx alike (hh, hw with overlap 0)
  int fine_overlap_y = 0, fine_overlap_x = 0; // Oy = oy * sy, Ox alike
  int field_h = 0, field_w = 0;               // TY * stride_y + oy, TX * stride_x + ox
  int out_h = 0, out_w = 0;                   // TY * Sy + Oy, TX * Sx + Ox
  std::vector<float> ramp_y, ramp_x;          // w[j] = float32((j + 0.5) / O), j < O; the division in double, rounded once
  unsigned blend_blocks_per_row = 0;          // blending stitch: one lane per output (row, column), a workgroup lies in one row
  unsigned blend_grid = 0;                    // out_h * blend_blocks_per_row
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
// output has more than one channel, sizes below 1, model_chunk < 1; an overlap below 0 or above half the tile; with an overlap, an
// output side that is no multiple of the input side, a field or output side above INT_MAX, n * hh * hw beyond what the 64-bit
// element offsets hold, a blending stitch of more workgroups than one launch takes.
TilePlan tile_plan(const TilePlanIn& in);

// {"n":N,"chunk":K,"n_chunks":M,"chunks":[[first,count],..]|null,"v":V,"cut":{"grid":G,"block":256},
//  "stitch":{"block":256,"items_per_tile":I,"blocks_per_tile":B,"grid":[one per chunk]|null},"intermediate_bytes":Y}
// The two lists are null above 65536 chunks (they are regular: every chunk but the last has K samples).
std::string tile_plan_json(const TilePlan& p);
// The same keys, then "overlap":[oy,ox],"stride":[ly,lx],"field":[H,W],"out":[H*sy,W*sx],
// "blend":{"grid":G,"block":256,"blocks_per_row":B,"ramp":[Oy,Ox]}|null.  With an overlap "stitch" is null (the per-chunk stitch does
// not run) and intermediate_bytes counts all n samples; without one "blend" is null.
std::string tile_plan_json_overlap(const TilePlan& p);

}  // namespace srcfd
