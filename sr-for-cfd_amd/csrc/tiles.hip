// Tiled super-resolution on the device (gfx950): cut a (TY*lh, TX*lw, C) coarse field into the tile samples of a one-channel
// model, and stitch the samples' planar hh x hw results into the channel-interleaved (TY*hh, TX*hw, C) field (BASELINE config 5;
// include/srcfd.h, "tiled super-resolution").  Sample order: s = (ty*TX + tx)*C + c, that of pipeline.tiled_super_resolution.
// Both kernels only move float32 values: the result has the bits of numpy's reshape / transpose of the same samples.
//
// tiles_cut     one grid-stride launch: every thread gathers one element of x (n, lh, lw); the first n threads also copy the
//               per-component (mean, std) pairs into the per-sample rows srcfd_predict_device takes (row s = row s % C).  Tile
//               (ty, tx) starts at coarse row ty * stride_y, column tx * stride_x: the tile sides, or less by the overlap.
// tiles_stitch  one lane per (tile, row, V x-consecutive columns): it loads V floats from each of the tile's C planar source
//               rows and stores the V * C contiguous output floats they interleave to, as C stores of V floats.  Consecutive
//               lanes read consecutive 4 V-byte pieces of C planes and write consecutive 4 V C-byte pieces of one output row:
//               both sides move whole cache lines per wave, with no LDS transpose.  C is a run-time argument; the body is
//               instantiated per C behind a wave-uniform switch so that the interleave is register renaming (no scratch).
//               Every element offset is 64-bit.  Plain stores.
// tiles_blend   the stitch of an overlapped tiling: one lane per output (row, column), a workgroup inside one row.  tile_map.h
//               says which one or two tiles the row and the column come from; the lane reads one, two or four planar values per
//               component, blends along x inside each contributing tile row, then along y -- a + w * (b - a), three float32
//               operations each rounded, the weights read from the uploaded ramp tables -- and stores the pixel's C contiguous
//               floats.  An axis with one source does no arithmetic: outside the overlap zones the pixel has its tile's bits.
//               A pixel with a contributing index outside y is left as it was.  C is instantiated behind the same switch.
// The vector width V, the grids and the chunks come from tile_plan.h; nothing here decides them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <string>

#include "engine.h"
#include "tile_plan.h"

namespace srcfd {

__global__ void __launch_bounds__(TILE_BLOCK) tiles_cut_kernel(const float* __restrict__ field, const float* __restrict__ in_aff,
                                                               const float* __restrict__ out_aff, float* __restrict__ x,
                                                               float* __restrict__ in_aff_n, float* __restrict__ out_aff_n, int lh, int lw,
                                                               int stride_y, int stride_x, int field_w, int tx_tiles, int C, int n) {
  const int64_t stride = (int64_t)gridDim.x * TILE_BLOCK;
  const int64_t first = (int64_t)blockIdx.x * TILE_BLOCK + threadIdx.x;
  const int tile_elems = lh * lw;
  const int64_t total = (int64_t)n * tile_elems;
  const int64_t row_floats = (int64_t)field_w * C;   // one row of the field
  for (int64_t e = first; e < total; e += stride) {
    const int s = (int)(e / tile_elems), q = (int)(e - (int64_t)s * tile_elems);
    const int r = q / lw, col = q - r * lw;
    const int t = s / C, c = s - t * C;
    const int ty = t / tx_tiles, tx = t - ty * tx_tiles;
    x[e] = field[((int64_t)ty * stride_y + r) * row_floats + ((int64_t)tx * stride_x + col) * C + c];
  }
  for (int64_t s = first; s < n; s += stride) {
    const int c = (int)(s % C);
    if (in_aff) { in_aff_n[2 * s] = in_aff[2 * c]; in_aff_n[2 * s + 1] = in_aff[2 * c + 1]; }
    if (out_aff) { out_aff_n[2 * s] = out_aff[2 * c]; out_aff_n[2 * s + 1] = out_aff[2 * c + 1]; }
  }
}

template <int V> struct TileVec;
template <> struct TileVec<4> { using type = float4; };
template <> struct TileVec<2> { using type = float2; };
template <> struct TileVec<1> { using type = float; };

// one lane's piece of tile t: row r, columns [g V, g V + V) of the C samples t C .. t C + C - 1
template <int V, int C>
__device__ __forceinline__ void tiles_stitch_piece(const float* __restrict__ y, float* __restrict__ out, const int* __restrict__ src_index,
                                                   int64_t y_rows, int hh, int hw, int tx_tiles, int s0, int t, int r, int g) {
  using Vec = typename TileVec<V>::type;
  const int64_t plane = (int64_t)hh * hw;
  const int64_t in_off = (int64_t)r * hw + (int64_t)g * V;
  float v[C][V];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int s = t * C + c;
    const int64_t row = src_index ? (int64_t)src_index[s] : (int64_t)(s - s0);
    if (row < 0 || row >= y_rows) return;   // an index outside y: the tile is left as it was (nothing has been stored yet)
    const Vec q = *reinterpret_cast<const Vec*>(y + row * plane + in_off);
    __builtin_memcpy(v[c], &q, sizeof(q));
  }
  const int ty = t / tx_tiles, tx = t - ty * tx_tiles;
  float* o = out + ((((int64_t)ty * hh + r) * tx_tiles + tx) * hw + (int64_t)g * V) * C;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    float w[V];
#pragma unroll
    for (int i = 0; i < V; ++i) w[i] = v[(k * V + i) % C][(k * V + i) / C];   // output float e of the piece: column e / C, component e % C
    Vec q;
    __builtin_memcpy(&q, w, sizeof(q));
    *reinterpret_cast<Vec*>(o + k * V) = q;
  }
}

template <int V>
__global__ void __launch_bounds__(TILE_BLOCK) tiles_stitch_kernel(const float* __restrict__ y, float* __restrict__ out,
                                                                  const int* __restrict__ src_index, int64_t y_rows, int hh, int hw,
                                                                  int tx_tiles, int C, int s0, unsigned blocks_per_tile) {
  const unsigned tile = blockIdx.x / blocks_per_tile;
  const int item = (int)((blockIdx.x - tile * blocks_per_tile) * TILE_BLOCK + threadIdx.x);
  const int G = hw / V;
  if (item >= hh * G) return;
  const int r = item / G, g = item - r * G;
  const int t = s0 / C + (int)tile;
  switch (C) {   // uniform over the launch
    case 1: tiles_stitch_piece<V, 1>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 2: tiles_stitch_piece<V, 2>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 3: tiles_stitch_piece<V, 3>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 4: tiles_stitch_piece<V, 4>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 5: tiles_stitch_piece<V, 5>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 6: tiles_stitch_piece<V, 6>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 7: tiles_stitch_piece<V, 7>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    case 8: tiles_stitch_piece<V, 8>(y, out, src_index, y_rows, hh, hw, tx_tiles, s0, t, r, g); break;
    default: break;
  }
}
static_assert(TILE_MAX_CHANNELS == 8, "tiles_stitch_kernel switches over 1 .. 8 channels");

struct TileBlendArgs {
  const float* y; float* out; const int* src_index; const float* ramp_y; const float* ramp_x;
  int64_t y_rows;
  int hh, hw, tiles_y, tiles_x, out_w;
  int stride_y, stride_x, overlap_y, overlap_x;   // fine: Sy, Sx, Oy, Ox
  unsigned blocks_per_row;
};

__device__ __forceinline__ float tiles_blend(float a, float b, float w) { return __fadd_rn(a, __fmul_rn(w, __fsub_rn(b, a))); }

// output pixel (R, X): ay / ax say where row R and column X come from
template <int C>
__device__ __forceinline__ void tiles_blend_pixel(const TileBlendArgs& k, const TileAxisSrc ay, const TileAxisSrc ax, int R, int X) {
  const int64_t plane = (int64_t)k.hh * k.hw;
  const bool by = ay.t0 >= 0, bx = ax.t0 >= 0;
  // planes of the contributing samples: [tile row: 0 = ay.t0, 1 = ay.t1][tile column: 0 = ax.t0, 1 = ax.t1][component]
  int64_t row[2][2][C];
#pragma unroll
  for (int iy = 0; iy < 2; ++iy) {
    if (iy == 0 && !by) continue;
#pragma unroll
    for (int ix = 0; ix < 2; ++ix) {
      if (ix == 0 && !bx) continue;
      const int64_t t = (int64_t)(iy ? ay.t1 : ay.t0) * k.tiles_x + (ix ? ax.t1 : ax.t0);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t s = t * C + c;
        const int64_t q = k.src_index ? (int64_t)k.src_index[s] : s;
        if (q < 0 || q >= k.y_rows) return;   // nothing has been stored yet: the pixel is left as it was
        row[iy][ix][c] = q;
      }
    }
  }
  const float wy = by ? k.ramp_y[ay.j] : 0.f, wx = bx ? k.ramp_x[ax.j] : 0.f;
  float v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    // one tile row's value at column X: blended along x where the column has two sources
    auto along_x = [&](int iy, int r) {
      const float b = k.y[row[iy][1][c] * plane + (int64_t)r * k.hw + ax.r1];
      if (!bx) return b;
      const float a = k.y[row[iy][0][c] * plane + (int64_t)r * k.hw + ax.r0];
      return tiles_blend(a, b, wx);
    };
    const float bottom = along_x(1, ay.r1);
    v[c] = by ? tiles_blend(along_x(0, ay.r0), bottom, wy) : bottom;
  }
  float* o = k.out + ((int64_t)R * k.out_w + X) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = v[c];
}

__global__ void __launch_bounds__(TILE_BLOCK) tiles_blend_kernel(const TileBlendArgs k, int C) {
  const unsigned R = blockIdx.x / k.blocks_per_row;
  const int64_t X64 = (int64_t)(blockIdx.x - R * k.blocks_per_row) * TILE_BLOCK + threadIdx.x;
  if (X64 >= k.out_w) return;
  const int X = (int)X64;
  const TileAxisSrc ay = tile_axis_src((int)R, k.tiles_y, k.stride_y, k.overlap_y);   // uniform over the workgroup
  const TileAxisSrc ax = tile_axis_src(X, k.tiles_x, k.stride_x, k.overlap_x);
  switch (C) {   // uniform over the launch
    case 1: tiles_blend_pixel<1>(k, ay, ax, (int)R, X); break;
    case 2: tiles_blend_pixel<2>(k, ay, ax, (int)R, X); break;
    case 3: tiles_blend_pixel<3>(k, ay, ax, (int)R, X); break;
    case 4: tiles_blend_pixel<4>(k, ay, ax, (int)R, X); break;
    case 5: tiles_blend_pixel<5>(k, ay, ax, (int)R, X); break;
    case 6: tiles_blend_pixel<6>(k, ay, ax, (int)R, X); break;
    case 7: tiles_blend_pixel<7>(k, ay, ax, (int)R, X); break;
    case 8: tiles_blend_pixel<8>(k, ay, ax, (int)R, X); break;
    default: break;
  }
}

// srcfd_tiler: the plan, the stream and the buffers of one (model, TY, TX, C, overlap, max_chunk)
struct Tiler {
  Model* m = nullptr;   // borrowed; not touched by the destructor
  int device = -1;
  TilePlan plan;
  hipStream_t stream = nullptr;
  DevBuf<float> d_x;            // (n, lh, lw) tile samples
  DevBuf<float> d_in_aff, d_out_aff;   // (n, 2) each
  DevBuf<float> d_y;            // (chunk, hh, hw): one chunk's planar predictions; with an overlap (n, hh, hw): all of them
  DevBuf<float> d_ramp_y, d_ramp_x;   // the plan's ramp tables (empty without an overlap on that axis)
  ~Tiler() { if (device >= 0) (void)hipSetDevice(device); }   // for the members' destructors (device_mem.h)
};

static int pointer_align(const void* a, const void* b) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | 16;
  return (int)(bits & (~bits + 1));   // lowest set bit: 1 .. 16
}

static int launch_cut(const Tiler& t, const float* field, const float* in_aff, const float* out_aff, float* x, float* in_aff_n, float* out_aff_n) {
  const TilePlanIn& in = t.plan.in;
  hipLaunchKernelGGL(tiles_cut_kernel, dim3(t.plan.cut_grid), dim3(TILE_BLOCK), 0, t.stream, field, in_aff, out_aff, x, in_aff_n, out_aff_n, in.lh, in.lw,
                     t.plan.stride_y, t.plan.stride_x, t.plan.field_w, in.tiles_x, in.channels, t.plan.n);
  HIPCHECK(hipGetLastError());
  return SRCFD_OK;
}

// samples [s0, s1) of the tiler's grid from y (y_rows planes) into out; the plan is the tiler's with V for these two pointers
static int launch_stitch(const Tiler& t, const float* y, int64_t y_rows, const int* src_index, int s0, int s1, float* out) {
  if (s1 == s0) return SRCFD_OK;
  TilePlanIn aligned = t.plan.in;
  aligned.align_bytes = pointer_align(y, out);
  const TilePlan p = tile_plan(aligned);
  const unsigned grid = tile_stitch_grid(p, s1 - s0);
  const TilePlanIn& in = p.in;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TILE_BLOCK), 0, t.stream, y, out, src_index, y_rows, in.hh, in.hw, in.tiles_x, in.channels, s0,
                       p.stitch_blocks_per_tile);
  };
  if (p.v == 4) go(tiles_stitch_kernel<4>);
  else if (p.v == 2) go(tiles_stitch_kernel<2>);
  else go(tiles_stitch_kernel<1>);
  HIPCHECK(hipGetLastError());
  return SRCFD_OK;
}

// the blending stitch of an overlapped tiler: all n samples from y (y_rows planes) into out, one launch
static int launch_blend(const Tiler& t, const float* y, int64_t y_rows, const int* src_index, float* out) {
  const TilePlan& p = t.plan;
  TileBlendArgs k;
  k.y = y; k.out = out; k.src_index = src_index; k.ramp_y = t.d_ramp_y.get(); k.ramp_x = t.d_ramp_x.get();
  k.y_rows = y_rows;
  k.hh = p.in.hh; k.hw = p.in.hw; k.tiles_y = p.in.tiles_y; k.tiles_x = p.in.tiles_x; k.out_w = p.out_w;
  k.stride_y = p.fine_stride_y; k.stride_x = p.fine_stride_x; k.overlap_y = p.fine_overlap_y; k.overlap_x = p.fine_overlap_x;
  k.blocks_per_row = p.blend_blocks_per_row;
  hipLaunchKernelGGL(tiles_blend_kernel, dim3(p.blend_grid), dim3(TILE_BLOCK), 0, t.stream, k, p.in.channels);
  HIPCHECK(hipGetLastError());
  return SRCFD_OK;
}

static void fill_plan_in(TilePlanIn& in, int lh, int lw, int in_channels, int hh, int hw, int out_channels, int tiles_y, int tiles_x, int channels,
                         int overlap_y, int overlap_x, int max_chunk, int model_chunk, int align_bytes) {
  in.lh = lh; in.lw = lw; in.in_channels = in_channels; in.hh = hh; in.hw = hw; in.out_channels = out_channels;
  in.tiles_y = tiles_y; in.tiles_x = tiles_x; in.channels = channels; in.max_chunk = max_chunk; in.model_chunk = model_chunk;
  in.align_bytes = align_bytes; in.overlap_y = overlap_y; in.overlap_x = overlap_x;
}

static int plan_to_buffer(const char* fn, const std::string& s, char* buf, size_t len) {
  if (s.size() + 1 > len) { set_error(std::string(fn) + ": buffer too small, " + std::to_string(s.size() + 1) + " bytes needed"); return SRCFD_EINVAL; }
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return SRCFD_OK;
}

static int tiler_create(const char* fn, srcfd_model* m, int tiles_y, int tiles_x, int channels, int overlap_y, int overlap_x, int max_chunk,
                        srcfd_tiler** out) {
  if (!out) { set_error(std::string(fn) + ": bad arguments"); return SRCFD_EINVAL; }
  *out = nullptr;
  if (!m) { set_error(std::string(fn) + ": null model"); return SRCFD_EINVAL; }
  Model* mm = reinterpret_cast<Model*>(m);
  if (mm->device < 0) { set_error(std::string(fn) + ": host-only model handle: the tiler runs on the model's device"); return SRCFD_ENODEV; }
  const int* os = mm->desc.out_shape();
  const int64_t n = (int64_t)tiles_y * tiles_x * channels;
  const int model_chunk = srcfd_model_workspace(m, (int)std::min<int64_t>(std::max<int64_t>(n, 1), INT_MAX), nullptr);
  if (model_chunk < 0) return model_chunk;
  TilePlanIn in;
  fill_plan_in(in, mm->desc.in_shape[0], mm->desc.in_shape[1], mm->desc.in_shape[2], os[0], os[1], os[2], tiles_y, tiles_x, channels, overlap_y, overlap_x,
               max_chunk, model_chunk, 16);
  std::unique_ptr<Tiler> t(new Tiler());
  t->plan = tile_plan(in);   // refuses what the kernels do not take
  t->m = mm;
  HIPCHECK(hipSetDevice(mm->device));
  t->device = mm->device;
  const size_t n_s = (size_t)t->plan.n;
  int rc = t->d_x.alloc(n_s * in.lh * in.lw);
  if (!rc) rc = t->d_in_aff.alloc(2 * n_s);
  if (!rc) rc = t->d_out_aff.alloc(2 * n_s);
  if (!rc) rc = t->d_y.alloc(t->plan.intermediate_bytes / sizeof(float));
  if (!rc) rc = t->d_ramp_y.upload(t->plan.ramp_y);
  if (!rc) rc = t->d_ramp_x.upload(t->plan.ramp_x);
  if (rc) return rc;
  *out = reinterpret_cast<srcfd_tiler*>(t.release());
  return SRCFD_OK;
}

}  // namespace srcfd

using srcfd::set_error;

extern "C" {

int srcfd_tiled_plan(int lh, int lw, int in_channels, int hh, int hw, int out_channels, int tiles_y, int tiles_x, int channels, int max_chunk,
                     int model_chunk, int align_bytes, char* buf, size_t len) {
  return srcfd::abi_guard("srcfd_tiled_plan", [&]() -> int {
    if (!buf || !len) { set_error("srcfd_tiled_plan: bad arguments"); return SRCFD_EINVAL; }
    srcfd::TilePlanIn in;
    srcfd::fill_plan_in(in, lh, lw, in_channels, hh, hw, out_channels, tiles_y, tiles_x, channels, 0, 0, max_chunk, model_chunk, align_bytes);
    return srcfd::plan_to_buffer("srcfd_tiled_plan", srcfd::tile_plan_json(srcfd::tile_plan(in)), buf, len);
  });
}

int srcfd_tiled_plan_overlap(int lh, int lw, int in_channels, int hh, int hw, int out_channels, int tiles_y, int tiles_x, int channels, int overlap_y,
                             int overlap_x, int max_chunk, int model_chunk, int align_bytes, char* buf, size_t len) {
  return srcfd::abi_guard("srcfd_tiled_plan_overlap", [&]() -> int {
    if (!buf || !len) { set_error("srcfd_tiled_plan_overlap: bad arguments"); return SRCFD_EINVAL; }
    srcfd::TilePlanIn in;
    srcfd::fill_plan_in(in, lh, lw, in_channels, hh, hw, out_channels, tiles_y, tiles_x, channels, overlap_y, overlap_x, max_chunk, model_chunk, align_bytes);
    return srcfd::plan_to_buffer("srcfd_tiled_plan_overlap", srcfd::tile_plan_json_overlap(srcfd::tile_plan(in)), buf, len);
  });
}

int srcfd_tiler_create(srcfd_model* m, int tiles_y, int tiles_x, int channels, int max_chunk, srcfd_tiler** out) {
  return srcfd::abi_guard("srcfd_tiler_create", [&]() -> int { return srcfd::tiler_create("srcfd_tiler_create", m, tiles_y, tiles_x, channels, 0, 0, max_chunk, out); });
}

int srcfd_tiler_create_overlap(srcfd_model* m, int tiles_y, int tiles_x, int channels, int overlap_y, int overlap_x, int max_chunk, srcfd_tiler** out) {
  return srcfd::abi_guard("srcfd_tiler_create_overlap", [&]() -> int {
    return srcfd::tiler_create("srcfd_tiler_create_overlap", m, tiles_y, tiles_x, channels, overlap_y, overlap_x, max_chunk, out);
  });
}

void srcfd_tiler_destroy(srcfd_tiler* t) { delete reinterpret_cast<srcfd::Tiler*>(t); }

int srcfd_tiler_set_stream(srcfd_tiler* t, void* stream) {
  return srcfd::abi_guard("srcfd_tiler_set_stream", [&]() -> int {
    if (!t) { set_error("srcfd_tiler_set_stream: null handle"); return SRCFD_EINVAL; }
    reinterpret_cast<srcfd::Tiler*>(t)->stream = reinterpret_cast<hipStream_t>(stream);
    return SRCFD_OK;
  });
}

int srcfd_tiles_cut_device(srcfd_tiler* t, const float* field_dev, const float* in_affine_dev, const float* out_affine_dev, float* x_dev,
                           float* in_affine_n_dev, float* out_affine_n_dev) {
  return srcfd::abi_guard("srcfd_tiles_cut_device", [&]() -> int {
    using namespace srcfd;
    if (!t || !field_dev || !x_dev || (in_affine_dev && !in_affine_n_dev) || (out_affine_dev && !out_affine_n_dev)) {
      set_error("srcfd_tiles_cut_device: bad arguments");
      return SRCFD_EINVAL;
    }
    const Tiler& tl = *reinterpret_cast<Tiler*>(t);
    HIPCHECK(hipSetDevice(tl.device));
    return launch_cut(tl, field_dev, in_affine_dev, out_affine_dev, x_dev, in_affine_n_dev, out_affine_n_dev);
  });
}

int srcfd_tiles_stitch_device(srcfd_tiler* t, const float* y_dev, int64_t y_rows, const int32_t* src_index_dev, int s0, int s1, float* out_dev) {
  return srcfd::abi_guard("srcfd_tiles_stitch_device", [&]() -> int {
    using namespace srcfd;
    if (!t || !y_dev || !out_dev || y_rows < 0) { set_error("srcfd_tiles_stitch_device: bad arguments"); return SRCFD_EINVAL; }
    const Tiler& tl = *reinterpret_cast<Tiler*>(t);
    const int C = tl.plan.in.channels;
    if (s0 < 0 || s1 < s0 || s1 > tl.plan.n || s0 % C || s1 % C) {
      set_error("srcfd_tiles_stitch_device: the sample range [" + std::to_string(s0) + ", " + std::to_string(s1) + ") must lie in [0, " +
                std::to_string(tl.plan.n) + "] and start and end at multiples of " + std::to_string(C) + " (whole tiles)");
      return SRCFD_EINVAL;
    }
    if (tl.plan.blended && (s0 != 0 || s1 != tl.plan.n)) {
      set_error("srcfd_tiles_stitch_device: a blended stitch needs every tile: on a tiler with an overlap the range is [0, " + std::to_string(tl.plan.n) +
                "), not [" + std::to_string(s0) + ", " + std::to_string(s1) + ")");
      return SRCFD_EINVAL;
    }
    if (!src_index_dev && y_rows < s1 - s0) {
      set_error("srcfd_tiles_stitch_device: y holds " + std::to_string(y_rows) + " rows, the range takes " + std::to_string(s1 - s0));
      return SRCFD_EINVAL;
    }
    HIPCHECK(hipSetDevice(tl.device));
    if (tl.plan.blended) return launch_blend(tl, y_dev, y_rows, src_index_dev, out_dev);
    return launch_stitch(tl, y_dev, y_rows, src_index_dev, s0, s1, out_dev);
  });
}

int srcfd_tiler_run(srcfd_tiler* t, const float* field_dev, const float* in_affine_dev, const float* out_affine_dev, float* out_dev, int flags,
                    int64_t* nonfinite_dev) {
  return srcfd::abi_guard("srcfd_tiler_run", [&]() -> int {
    using namespace srcfd;
    if (!t || !field_dev || !out_dev) { set_error("srcfd_tiler_run: bad arguments"); return SRCFD_EINVAL; }
    Tiler& tl = *reinterpret_cast<Tiler*>(t);
    const TilePlan& p = tl.plan;
    HIPCHECK(hipSetDevice(tl.device));
    int rc = launch_cut(tl, field_dev, in_affine_dev, out_affine_dev, tl.d_x.get(), tl.d_in_aff.get(), tl.d_out_aff.get());
    const size_t in_elems = (size_t)p.in.lh * p.in.lw, plane = (size_t)p.in.hh * p.in.hw;
    for (int i = 0; i < p.n_chunks && !rc; ++i) {
      const int first = p.chunk_first(i), count = p.chunk_count(i);
      // call_n = n: every chunk follows the kernel choice of the whole call, as the chunks of srcfd_predict do
      rc = tl.m->predict_device(tl.d_x.get() + first * in_elems, count, in_affine_dev ? tl.d_in_aff.get() + 2 * (size_t)first : nullptr,
                                out_affine_dev ? tl.d_out_aff.get() + 2 * (size_t)first : nullptr,
                                p.blended ? tl.d_y.get() + first * plane : tl.d_y.get(), SRCFD_F32, flags,
                                reinterpret_cast<unsigned long long*>(nonfinite_dev), tl.stream, p.n);
      if (!rc && !p.blended) rc = launch_stitch(tl, tl.d_y.get(), count, nullptr, first, first + count, out_dev);
    }
    if (!rc && p.blended) rc = launch_blend(tl, tl.d_y.get(), p.n, nullptr, out_dev);   // every chunk's planes are there: one stitch
    return rc;
  });
}

}  // extern "C"
