// The test of SRCFD_FLAG_NAN_GUARD, shared by every kernel that finishes an output (srcfd.h: "non-finite in y's own type").
#pragma once
#include <hip/hip_runtime.h>

namespace srcfd {

// True when the float32 value v is still finite AFTER the round-to-nearest-even cast to the caller's output type
// OUT (0 f32, 1 bf16, 2 f16).  A 16-bit type overflows to +-Inf from its largest finite value plus half an ulp on (the tie
// goes to the even neighbour, which is Inf): 65504 + 16 for f16, 0x7f7f0000 + 0x8000 for bf16.  Such a v is finite in f32, and a
// guard that only asked `fabsf(v) <= FLT_MAX` stored it as Inf, uncounted.  A NaN fails every comparison.  OUT == 0 is that
// expression unchanged.
template <int OUT>
__device__ __forceinline__ bool out_finite(float v) {
  if (OUT == 0) return fabsf(v) <= 3.402823466e38f;
  if (OUT == 1) return fabsf(v) < 3.3961775292304601e38f;
  return fabsf(v) < 65520.f;
}

}  // namespace srcfd
