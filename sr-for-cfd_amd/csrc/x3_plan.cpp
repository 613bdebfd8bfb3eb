// The split-bf16 GEMM's launch plan: see x3_plan.h.  Host arithmetic only.
#include "x3_plan.h"

#include <algorithm>

namespace srcfd {

bool gemm_x3_res_qualifies(const GemmDesc& d) {
  return d.K <= X3R_K && d.K % X3_BK == 0 && d.TY * d.TX == 1 && d.cy == 0 && d.cx == 0;
}

// Qualifies: a GEMM the generic f32 kernel would run, with whole 32-deep k-tiles inside a tap and whole 128-channel blocks,
// channel groups of 32 inside one output phase, 16-byte aligned rows on both sides, swish or linear.
bool gemm_x3_qualifies(const GemmDesc& d) {
  return d.K >= 128 && d.CI % X3_BK == 0 && d.N % X3_BN == 0 && d.CO % 32 == 0 && d.OC % 4 == 0 && (d.act == SRCFD_ACT_SWISH || d.act == SRCFD_ACT_LINEAR) &&
         (d.M <= 0 || ((int64_t)(d.M / (d.MH * d.MW) + 1) * d.IH * d.IW * d.CI < (1ll << 31) &&     // 32-bit element offsets into X ...
                       (int64_t)(d.M / (d.MH * d.MW) + 1) * d.OH * d.OW * d.OC < (1ll << 31)));     // ... and into Y
}

int gemm_x3_kpad(const GemmDesc& d) { return (d.K + X3_BK - 1) / X3_BK * X3_BK; }

// one op on its own
static X3Op plan_one(const GemmDesc& d, int num_cus) {
  X3Op o;
  o.kpad = gemm_x3_kpad(d);
  o.k = gemm_x3_res_qualifies(d) ? X3Kernel::Res : X3Kernel::Tile;
  if (d.M <= 0) return o;
  if (o.k == X3Kernel::Res) {   // short K, no taps: weights resident in LDS, one workgroup per CU and channel block walks the pixel tiles
    o.ntiles = (d.M + 31) / 32;
    const int nblk = d.N / X3_BN;
    o.grid[0] = (unsigned)std::max(1, std::min((o.ntiles + 7) / 8, std::max(1, num_cus / nblk)));
    o.grid[1] = (unsigned)nblk;
  } else {
    o.grid[0] = (unsigned)((d.M + X3_BP - 1) / X3_BP);
    o.grid[1] = (unsigned)(d.N / X3_BN);
  }
  return o;
}

// ops of one layer: one launch when every op takes the tiled kernel (gemm_x3), else one launch per op
X3Plan plan_gemm_x3(const GemmDesc* ds, int count, int num_cus) {
  X3Plan p;
  p.count = count;
  for (int i = 0; i < count; ++i) p.op[i] = plan_one(ds[i], num_cus);
  bool group = count >= 2 && count <= 4;
  for (int i = 0; group && i < count; ++i) group = ds[i].M > 0 && !gemm_x3_res_qualifies(ds[i]);
  if (!group) return p;
  p.grouped = true;
  int total = 0;
  for (int i = 0; i < count; ++i) {
    p.first[i] = total;
    total += ((ds[i].M + X3_BP - 1) / X3_BP) * (ds[i].N / X3_BN);
  }
  for (int i = count; i <= 4; ++i) p.first[i] = total;
  p.group_grid = (unsigned)total;
  return p;
}

}  // namespace srcfd
