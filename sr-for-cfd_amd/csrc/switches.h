// The functional A/B switches of a forward as plain data: no HIP, so that the host-only planning units (lowp16_plan.h) can take them.
#pragma once

namespace srcfd {

// Functional A/B switches: every one selects a COMPLETE alternative implementation of a stage (no work is skipped), for the parity
// tests and the tools.  They are read from the environment once per srcfd_predict* call (Switches::from_env, engine.hip), are part of
// the hipGraph key (a captured forward is replayed only under the switches it was captured with) and are reported by srcfd_model_last_plan.
struct Switches {
  bool enc16 = true;     // SRCFD_ENC=0: layer-by-layer 16-bit encoder instead of the one-launch enc16
  bool mid16 = true;     // SRCFD_MID=0: generic GEMMs instead of the fused ConvT#0 -> ConvT#1 kernel
  int mid_shape = 3;     // workgroup shape of mid16 (SRCFD_MID=1, 2, 3): 1 = 8 waves x 32 pixels, two workgroups per CU (128 registers; rounds 1-2);
                         // 2 = 8 waves x 64 pixels, one per CU; 3 = 4 waves x 64 pixels, two per CU (256 registers; default)
  bool dense1_16 = true; // SRCFD_DENSE1=0: dense_1 on the generic 16-bit GEMM
  bool enc32 = true;     // SRCFD_NO_ENC32=1: layer-by-layer f32 encoder
  bool skinny32 = true;  // SRCFD_NO_DENSE_SKINNY=1: dense_1 on the generic f32 GEMM
  bool tail16s = false;  // SRCFD_TAIL=s: the software-pipelined 8-wave tail kernel (kernels_tail16s.hip) instead of the 16-wave, stage-by-stage one (measured slower)
  int mid_waves = 0;     // SRCFD_MID_WAVES: other workgroup shapes of mid16 (4, 16: waves per workgroup at 32 pixels per wave); 0 = the shape mid_shape selects
  int mid_order = 0;     // SRCFD_MID_ORDER=1: mid16's workgroups dispatched with output phases 0 / 3 and 1 / 2 alternating instead of phase by phase
  int tail_seg = 0;      // SRCFD_TAIL_SEG: segments per sample of the 16-bit tail (1, 2, 5, 10, 25); 0 = chosen per batch
  bool tail32 = true;    // SRCFD_NO_TAIL32=1: the f32 tail layer by layer (convt_triple + the output conv) instead of the streaming tail32
  bool triple = true;    // SRCFD_NO_TRIPLE=1: ConvT#2 on its own and convt_pair instead of convt_triple
  bool pair = true;      // SRCFD_NO_PAIR=1: neither convt_triple nor convt_pair: every layer materialised
  bool gemm32_big = true;   // SRCFD_NO_GEMM32_BIG=1: large launches of the wide decoder layers on the generic f32 GEMM too
  unsigned bits() const {
    return (enc16 ? 1u : 0u) | (mid16 ? 2u : 0u) | (dense1_16 ? 4u : 0u) | (enc32 ? 8u : 0u) | (skinny32 ? 16u : 0u) | (tail16s ? 32u : 0u) |
           ((unsigned)mid_shape << 6) | ((unsigned)tail_seg << 8) | ((unsigned)mid_waves << 16) | ((unsigned)mid_order << 24) |
           (tail32 ? 1u << 25 : 0u) | (triple ? 1u << 26 : 0u) | (pair ? 1u << 27 : 0u) | (gemm32_big ? 1u << 28 : 0u);
  }
  bool all_default() const {
    return enc16 && mid16 && mid_shape == Switches().mid_shape && dense1_16 && enc32 && skinny32 && !tail16s && tail_seg == 0 && mid_waves == 0 &&
           mid_order == Switches().mid_order && tail32 && triple && pair && gemm32_big;
  }
  static Switches from_env();
};

}  // namespace srcfd
