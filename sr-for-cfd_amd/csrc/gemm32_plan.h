// The launch plan of the f32 implicit GEMM (kernels_fp32.hip, kernels_gemm32.hip): which kernel takes a descriptor, its column
// blocking and K-tile depth, the split-K cut, whether a layer's GEMMs go out as one launch, every grid, and the slab floats the
// launch needs.  Decided here once, as pure functions of the descriptors: no HIP runtime calls, no kernel code.  The launchers
// only issue what the plan says; engine.hip and train.hip size their slab buffers from the same plan.  tools/pack_digest.cpp links
// this unit on a CPU; tests/test_gemm32_plan.py checks it against an independent statement of the rules (tests/gemm32_plan_ref.py).
#pragma once
#include <cstddef>

#include "kernels.h"

namespace srcfd {

constexpr int BM = 128;                               // rows of a block tile of gemm_mfma_f32 (columns: 32 * nb)
constexpr int CT_H = 16, CT_W = 64;                   // output pixels of a workgroup of conv_n1_tile_f32
constexpr int GB_BM = 128, GB_BN = 128, GB_BK = 16;   // block tile of gemm32_big

// The kernel that takes a descriptor, tested in this order (the first that accepts wins).
enum class Gemm32Route {
  None,      // M == 0 or N == 0: nothing to launch
  TiledN1,   // conv_n1_tile_f32: 3x3 SAME 8 -> 1 conv, LDS-tiled (the one kernel that can fuse the network's finalize)
  N1x4,      // conv_n1x4_f32: 3x3 unit-stride 8 -> 1 conv, four pixels per thread
  N1,        // conv_n1_f32: any single-output-channel conv with K <= 512
  Ci1,       // conv_ci1_f32: single input channel, <= 8 output channels
  Mfma,      // gemm_mfma_f32<NB, VEC, BKT>
};
Gemm32Route gemm32_route(const GemmDesc& d);

// Split-K of the Mfma route: `splits` slabs of `kchunk` k each (splits == 1: kchunk == K).
// batch_invariant (inference): the cut depends on the layer only, never on the batch size; false (training): on the tile count too.
struct Gemm32Cut { int splits, kchunk; };
Gemm32Cut gemm32_cut(const GemmDesc& d, bool batch_invariant);

// One launch of gemm_mfma_f32 / gemm_mfma_group_f32 (or, with nb == 0, of one of the conv kernels: grid only) and of its finish.
struct Gemm32Launch {
  int nb = 0, bkt = 0, vec = 0;      // template arguments: 32 * nb columns per block, K-tile depth 16 / 32, 16-byte gathers
  unsigned grid[3] = {0, 0, 0};
  unsigned fin[2] = {0, 0};          // grid of the split-K finish; fin[0] == 0: no finish launch
};
struct Gemm32Op {
  Gemm32Route route = Gemm32Route::None;
  int splits = 1, kchunk = 0;
  size_t slab_off = 0;               // of this op's slabs in the workspace, floats
  int finish_groups = 1;             // slab groups one finish workgroup adds side by side: 1 or 8
  Gemm32Launch l;                    // its own launch; unused where the plan is grouped
};
struct Gemm32Plan {
  bool grouped = false;              // the ops go out as one gemm_mfma_group_f32 launch (`group`) + one finish
  int count = 0;
  Gemm32Op op[4];
  Gemm32Launch group;
  size_t ws_floats = 0;              // slab floats the launch (or the launches, one after the other) must be handed
};
// The GEMMs of one layer (count 2 .. 4: the output phases of a transposed convolution with kernel != stride) or a single GEMM
// (count == 1), M set.  Does not depend on how large the caller's workspace is: a launcher handed less refuses (gemm32_ws_fits).
Gemm32Plan plan_gemm32(const GemmDesc* ds, int count, bool batch_invariant);
// A null workspace is legal exactly where the plan needs no slabs.
inline bool gemm32_ws_fits(const Gemm32Plan& p, const void* ws, size_t ws_floats) {
  return p.ws_floats == 0 || (ws != nullptr && ws_floats >= p.ws_floats);
}

// Derived answers for engine.hip / train.hip
size_t gemm_splitk_ws_floats(const GemmDesc& d, bool batch_invariant = true);
size_t gemm_group_ws_floats(const GemmDesc* ds, int count, bool batch_invariant = true);
bool gemm_supports_epi_aux(const GemmDesc& d);   // the kernel that takes d applies an EpiAux (kernels.h)
bool gemm_fuses_finalize(const GemmDesc& d);     // launch_gemm_finalize accepts d
// gemm32_big (kernels_gemm32.hip): a layer (1 GEMM) or the output phases of a transposed convolution (2-4 GEMMs) qualify when
// every GEMM is one of the wide decoder layers that kernel is written for and the launch is large enough that the generic kernel
// would take its widest tile anyway (so the choice does not depend on anything but the layer and "is the batch large").
bool gemm32_big_qualifies(const GemmDesc* ds, int count);

}  // namespace srcfd
