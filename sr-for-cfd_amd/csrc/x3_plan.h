// The launch plan of the split-bf16 GEMM (kernels_x3.hip, SRCFD_PREC_FP32X3): which descriptors the kernels take, which of the two
// kernels takes each op of a layer, whether the layer's ops go out as one launch, every grid, the group's table of first workgroups
// and the resident kernel's tile count.  Decided here once, as pure functions of the descriptors and the CU count: no HIP runtime
// calls, no kernel code.  launch_gemm_x3_group only issues what the plan says.  tools/pack_digest.cpp links this unit on a CPU;
// tests/test_x3_forms.py checks it against an independent statement of the rules (tests/x3_plan_ref.py).
#pragma once
#include "kernels.h"

namespace srcfd {

constexpr int X3_BP = 128, X3_BN = 128, X3_BK = 32;   // workgroup tile of gemm_x3: pixels x channels x k
constexpr int X3R_K = 128;                             // the K whose three weight planes gemm_x3_res keeps in LDS

// gemm_x3_qualifies / gemm_x3_kpad: kernels.h.  The resident kernel takes the ops without taps whose K fits its LDS planes.
bool gemm_x3_res_qualifies(const GemmDesc& d);

enum class X3Kernel { Tile, Res };   // gemm_x3 (or a member of gemm_x3_group) / gemm_x3_res

struct X3Op {
  X3Kernel k = X3Kernel::Tile;
  int kpad = 0;                  // row length of the op's weight planes
  unsigned grid[2] = {0, 0};     // its own launch; unused where the plan is grouped; {0, 0}: nothing to launch (M <= 0)
  int ntiles = 0;                // Res: 32-pixel tiles the waves walk
};
struct X3Plan {
  bool grouped = false;          // the ops go out as one gemm_x3_group launch of `group_grid` workgroups
  int count = 0;
  X3Op op[4];
  unsigned group_grid = 0;
  int first[5] = {0, 0, 0, 0, 0};   // grouped: first linear workgroup of op i; first[count .. 4] = group_grid
};
// The GEMMs of one layer (count 2 .. 4: the output phases of a transposed convolution with kernel != stride) or a single GEMM,
// M set, every one accepted by gemm_x3_qualifies.
X3Plan plan_gemm_x3(const GemmDesc* ds, int count, int num_cus);

}  // namespace srcfd
