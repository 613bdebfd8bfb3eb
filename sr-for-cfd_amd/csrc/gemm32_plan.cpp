// The launch plan of the f32 implicit GEMM (gemm32_plan.h).  Plain C++: no HIP runtime calls.
#include "gemm32_plan.h"

#include <algorithm>

namespace srcfd {

Gemm32Route gemm32_route(const GemmDesc& d) {
  if (d.M <= 0 || d.N <= 0) return Gemm32Route::None;
  const bool conv3x3_8to1 = d.N == 1 && d.nphx == 1 && d.TX == 3 && d.TY == 3 && d.CI == 8 && d.ax == 1 && d.bx == 1 && d.ay == 1 && d.os == 1 &&
                            d.ox0 == 0 && d.OC == 1;
  if (conv3x3_8to1 && d.by == 1 && d.cx == -1 && d.cy == -1 && d.oy0 == 0 && d.IH == d.OH && d.IW == d.OW && d.MH == d.OH && d.MW == d.OW &&
      d.M % (d.MH * d.MW) == 0)
    return Gemm32Route::TiledN1;
  if (conv3x3_8to1 && d.MW % 4 == 0 && d.OW % 4 == 0 && d.K <= 512) return Gemm32Route::N1x4;
  if (d.N == 1 && d.K <= 512 && d.nphx == 1) return Gemm32Route::N1;
  if (d.CI == 1 && d.N <= 8 && d.K <= 64 && d.nphx == 1 && d.CO == d.N) return Gemm32Route::Ci1;
  return Gemm32Route::Mfma;
}

static int widest_nb(int Npad) { return (Npad % 128 == 0) ? 4 : ((Npad % 64 == 0) ? 2 : 1); }

// Skinny problems (few output tiles, long K: the Dense layers, and every layer at training batch
// sizes) are cut along K so that the weight matrix is streamed by >= 256 blocks instead of 1-6.
Gemm32Cut gemm32_cut(const GemmDesc& d, bool batch_invariant) {
  auto slabs = [&](int kchunk) { return Gemm32Cut{(d.K + kchunk - 1) / kchunk, kchunk}; };
  const Gemm32Cut whole{1, d.K};
  if (batch_invariant) {
    // inference: the summation order of a sample must not depend on the batch it sits in, so the cut depends on the
    // layer only: Dense layers (one row per sample) with a long K are always cut into 256-deep slabs, small conv maps into 144-deep ones
    if (d.M == 0) return whole;
    if (d.MH * d.MW == 1 && d.K >= 1024) return slabs(256);
    if (d.MH * d.MW <= 64 && d.K >= 512) return slabs(144);   // small feature maps with a long K (encoder conv2d_1: 25 pixels, K = 576): too few row tiles
    // ConvT#0's phases (144-169 pixels per sample, K up to 1024): a single field is 4 row tiles
    // -- costs ~3 % at batch 256 (slab traffic), cuts the one-field call by a third
    if (d.MH * d.MW <= 256 && d.K >= 512) return slabs(256);
    return whole;
  }
  const int64_t tiles = (int64_t)((d.M + BM - 1) / BM) * (d.Npad / (32 * widest_nb(d.Npad)));
  if (tiles >= 128 || d.K < 256 || tiles == 0) return whole;
  const int want = (int)std::min<int64_t>(std::min<int64_t>((512 + tiles - 1) / tiles, d.K / 64), 256);
  if (want <= 1) return whole;
  return slabs(((d.K + want - 1) / want + 31) / 32 * 32);
}

// Few rows (a solver-side call is 3 samples): narrower column blocks per wave until the launch covers the chip, and
// deeper K slabs.  The k order of every output element is the same for any nb / slab depth, so results stay
// bit-identical across batch sizes.  tiles: (row tile, K slab) pairs of the launch; rows x zs: its grid's x and z.
static Gemm32Launch tile_launch(const GemmDesc& d, int64_t tiles, int64_t rows, int zs) {
  Gemm32Launch l;
  l.vec = (d.K > 0 && d.CI % 4 == 0) ? 1 : 0;
  l.nb = widest_nb(d.Npad);
  while (l.nb > 1 && tiles * (d.Npad / (32 * l.nb)) < 512) l.nb >>= 1;
  l.bkt = tiles * (d.Npad / (32 * l.nb)) < 1024 ? 32 : 16;
  l.grid[0] = (unsigned)rows; l.grid[1] = (unsigned)(d.Npad / (32 * l.nb)); l.grid[2] = (unsigned)zs;
  return l;
}

static Gemm32Op plan_single(const GemmDesc& d, bool batch_invariant) {
  Gemm32Op o;
  o.route = gemm32_route(d);
  o.kchunk = d.K;
  auto blocks256 = [](int64_t n) { return (unsigned)((n + 255) / 256); };
  switch (o.route) {
    case Gemm32Route::None: break;
    case Gemm32Route::TiledN1:
      o.l.grid[0] = (unsigned)((d.OW + CT_W - 1) / CT_W); o.l.grid[1] = (unsigned)((d.OH + CT_H - 1) / CT_H); o.l.grid[2] = (unsigned)(d.M / (d.MH * d.MW));
      break;
    case Gemm32Route::N1x4: o.l.grid[0] = blocks256(d.M / 4); o.l.grid[1] = o.l.grid[2] = 1; break;
    case Gemm32Route::N1:
    case Gemm32Route::Ci1: o.l.grid[0] = blocks256(d.M); o.l.grid[1] = o.l.grid[2] = 1; break;
    case Gemm32Route::Mfma: {
      const Gemm32Cut cut = gemm32_cut(d, batch_invariant);
      o.splits = cut.splits; o.kchunk = cut.kchunk;
      const int64_t rows = (d.M + BM - 1) / BM, total = (int64_t)d.M * d.N;
      o.l = tile_launch(d, rows * o.splits, rows, o.splits);
      if (o.splits > 1) {
        o.finish_groups = (o.splits >= 32 && total < 65536) ? 8 : 1;
        const int epb = 256 / o.finish_groups;
        o.l.fin[0] = (unsigned)((total + epb - 1) / epb); o.l.fin[1] = 1;
      }
    }
  }
  return o;
}

static size_t slab_floats(const GemmDesc& d, const Gemm32Op& o) { return o.splits > 1 ? (size_t)o.splits * d.M * d.Npad : 0; }

Gemm32Plan plan_gemm32(const GemmDesc* ds, int count, bool batch_invariant) {
  Gemm32Plan p;
  if (count < 1 || count > 4) return p;   // count stays 0: the launchers refuse
  p.count = count;
  p.grouped = count >= 2;
  for (int i = 0; i < count; ++i) {
    p.op[i] = plan_single(ds[i], batch_invariant);
    p.ws_floats += slab_floats(ds[i], p.op[i]);   // a layer's allocation is the sum over its ops, grouped or not
    // one launch: generic GEMMs of one width and one gather form, none of which the single launch would finish in 8 groups
    p.grouped = p.grouped && p.op[i].route == Gemm32Route::Mfma && ds[i].K > 0 && ds[i].Npad == ds[0].Npad &&
                (ds[i].CI % 4 == 0) == (ds[0].CI % 4 == 0) && p.op[i].finish_groups == 1;
  }
  if (!p.grouped) return p;   // one launch after the other: each has the workspace to itself (slab_off 0)
  int64_t tiles = 0, max_rows = 0, max_finish = 0;
  int zs = 0;
  size_t off = 0;
  for (int i = 0; i < count; ++i) {
    const GemmDesc& d = ds[i];
    Gemm32Op& o = p.op[i];
    o.l = Gemm32Launch();
    o.slab_off = off;
    off += slab_floats(d, o);
    const int64_t rows = (d.M + BM - 1) / BM;
    tiles += rows * o.splits;
    zs += o.splits;
    max_rows = std::max(max_rows, rows);
    if (o.splits > 1) max_finish = std::max<int64_t>(max_finish, ((int64_t)d.M * d.N + 255) / 256);
  }
  p.group = tile_launch(ds[0], tiles, max_rows, zs);
  if (max_finish) { p.group.fin[0] = (unsigned)max_finish; p.group.fin[1] = (unsigned)count; }
  return p;
}

size_t gemm_splitk_ws_floats(const GemmDesc& d, bool batch_invariant) { return plan_gemm32(&d, 1, batch_invariant).ws_floats; }
size_t gemm_group_ws_floats(const GemmDesc* ds, int count, bool batch_invariant) { return plan_gemm32(ds, count, batch_invariant).ws_floats; }

// conv_n1*_f32 have no training epilogue, and the N == 1 kernels take a 1 -> 1 channel conv before conv_ci1_f32 sees it
bool gemm_supports_epi_aux(const GemmDesc& d) {
  const Gemm32Route r = gemm32_route(d);
  return d.K > 0 && (r == Gemm32Route::Mfma || r == Gemm32Route::Ci1);
}
bool gemm_fuses_finalize(const GemmDesc& d) { return gemm32_route(d) == Gemm32Route::TiledN1; }

bool gemm32_big_qualifies(const GemmDesc* ds, int count) {
  if (count < 1 || count > 4) return false;
  int64_t tiles = 0;
  for (int i = 0; i < count; ++i) {
    const GemmDesc& d = ds[i];
    if (d.M <= 0 || d.K <= 0 || d.CI % 16 != 0 || d.K % 16 != 0 || d.Npad % 128 != 0 || d.Npad != ds[0].Npad) return false;
    if (d.act != SRCFD_ACT_SWISH && d.act != SRCFD_ACT_LINEAR) return false;
    if (gemm32_cut(d, true).kchunk % GB_BK != 0) return false;   // a K slab of the batch-invariant split must be whole 16-deep tiles
    tiles += (int64_t)((d.M + GB_BM - 1) / GB_BM) * (d.Npad / GB_BN);
  }
  return tiles >= 1024;
}

}  // namespace srcfd
