// 16-bit kernels of the family graphs that the fused decoder_400 kernels do not cover (gfx950 only):
//
//   gemm16n     implicit GEMM for layers with 16 or 32 input channels (decoder_80's / decoder_100's last transposed convolution):
//               launch_gemm16's k-tile of 64 would straddle taps there.  Same GemmDesc, output phases and pixel-shuffle stores
//               included; k-step 16 = one v_mfma_f32_32x32x16_{bf16,f16}, always inside one tap (CI % 16 == 0).
//   outconv16   the network's last layer: 3x3 stride-1 SAME Conv2D, C -> 1 (C = 16 .. 64), 16-bit NHWC in, f32 accumulate,
//               y * std + mean as one fma, NaN guard, output cast.
//
// Activations carry the factor log2(e) of kernels_bf16.hip: a swish layer's GEMM produces u = log2e * x, the epilogue stores
// u * rcp(1 + exp2(-u)); the consumer's weights hold 1 / log2e (operand_pack.cpp, pack_any16).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev16.h"
#include "kernels16.h"

namespace srcfd {

// ---------------------------------------------------------------------------
// gemm16n.  D[channel][pixel] = Wt[channel][k] * X[pixel][k], one wave = 32 pixels x 32 channels, no LDS: both operands of a
// k-step are one 16-byte load per lane (A: weight row n0 + lane % 32, k = 8 (lane / 32) .. + 7; B: this lane's pixel, the same
// k).  These layers move 100 - 400 bytes per pixel for 1 - 4 k-steps of arithmetic: they are bound by the activation traffic,
// the few KB of weights stay in the caches.  Workgroup = 4 waves = 128 consecutive rows; blockIdx.y = 32-channel tile.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ void __launch_bounds__(256) gemm16n(GemmDesc d, const uint16_t* __restrict__ X, const uint16_t* __restrict__ Wt, int Kpad,
                                                const float* __restrict__ bias, uint16_t* __restrict__ Y) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const int m = blockIdx.x * 128 + wave * 32 + l31;
  const int n0 = blockIdx.y * 32;
  int img = -1, my = 0, mx = 0;
  if (m < d.M) {
    const int per = d.MH * d.MW;
    img = m / per;
    const int r = m - img * per;
    my = r / d.MW;
    mx = r - my * d.MW;
  }
  const int by0 = my * d.ay + d.cy, bx0 = mx * d.ax + d.cx;
  const uint16_t* xin = X + (int64_t)(img < 0 ? 0 : img) * d.IH * d.IW * d.CI + 8 * h;
  const uint16_t* wrow = Wt + (int64_t)(n0 + l31) * Kpad + 8 * h;   // rows up to Npad (a multiple of 32) exist, zero beyond N

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < d.K; k0 += 16) {
    const int tap = k0 / d.CI, ci0 = k0 - tap * d.CI;
    const int ty = tap / d.TX, tx = tap - ty * d.TX;
    const int iy = by0 + ty * d.by, ix = bx0 + tx * d.bx;
    uint4 b = make_uint4(0, 0, 0, 0);
    if (img >= 0 && (unsigned)iy < (unsigned)d.IH && (unsigned)ix < (unsigned)d.IW)
      b = *reinterpret_cast<const uint4*>(xin + ((int64_t)iy * d.IW + ix) * d.CI + ci0);
    const uint4 a = *reinterpret_cast<const uint4*>(wrow + k0);
    acc = mfma32<F16>(a, b, acc);
  }
  if (img < 0) return;
  // accumulator layout: this lane holds its pixel's channels n0 + 8 q + 4 h + (0 .. 3) in registers 4 q .. 4 q + 3
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + 8 * q + 4 * h;
    if (n >= d.N) continue;   // N % 4 == 0: a quad is inside N or outside
    const float4 bv = *reinterpret_cast<const float4*>(bias + n);
    const float v0 = act16(acc[4 * q] + bv.x, d.act), v1 = act16(acc[4 * q + 1] + bv.y, d.act);
    const float v2 = act16(acc[4 * q + 2] + bv.z, d.act), v3 = act16(acc[4 * q + 3] + bv.w, d.act);
    const int ph = n / d.CO, co = n - ph * d.CO, py = ph / d.nphx, px = ph - py * d.nphx;   // CO % 4 == 0: a quad stays in one phase
    const int64_t off = (((int64_t)img * d.OH + my * d.os + d.oy0 + py) * d.OW + mx * d.os + d.ox0 + px) * d.OC + co;
    *reinterpret_cast<uint2*>(Y + off) = make_uint2(pack2<F16>(v0, v1), pack2<F16>(v2, v3));
  }
}

hipError_t launch_gemm16n(bool f16, const GemmDesc& d, const uint16_t* X, const uint16_t* Wt, int Kpad, const float* bias, uint16_t* Y, const unsigned g[2],
                          hipStream_t s) {
  if (d.M == 0) return hipSuccess;
  if (d.CI % 16 != 0 || d.K % 16 != 0 || d.Npad % 32 != 0 || d.N % 4 != 0 || d.CO % 4 != 0 || d.OC % 4 != 0 || Kpad % 8 != 0) return hipErrorInvalidValue;
  const dim3 grid(g[0], g[1]);
  if (f16) hipLaunchKernelGGL(gemm16n<true>, grid, dim3(256), 0, s, d, X, Wt, Kpad, bias, Y);
  else hipLaunchKernelGGL(gemm16n<false>, grid, dim3(256), 0, s, d, X, Wt, Kpad, bias, Y);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// outconv16.  One thread per output pixel, consecutive threads along x: the nine taps of a pixel are 16-byte pieces of rows its
// neighbours read too (L1 / L2 hits); the weights (the 16-bit-rounded values as f32: every product is exact in f32) sit in LDS
// and are read as broadcasts.  f32 accumulation in (ty, tx, ci) order.  OUT: 0 f32, 1 bf16, 2 f16.
// ---------------------------------------------------------------------------
template <bool F16>
__device__ __forceinline__ void cvt2(uint32_t u, float& lo, float& hi) {
  if (F16) {
    const h16x2 v = __builtin_bit_cast(h16x2, u);
    lo = (float)v.x; hi = (float)v.y;
  } else {
    lo = __uint_as_float(u << 16); hi = __uint_as_float(u & 0xffff0000u);
  }
}

template <bool F16, int OUT>
__global__ void __launch_bounds__(256) outconv16(OutConv16Params p) {
  __shared__ float w[9 * 64];
  for (int i = threadIdx.x; i < 9 * p.C; i += 256) w[i] = p.w[i];
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)p.n * p.H * p.W;
  const bool valid = idx < total;
  bool bad = false;
  if (valid) {
    const int per = p.H * p.W;
    const int img = (int)(idx / per), r = (int)(idx - (int64_t)img * per), y = r / p.W, x = r - y * p.W;
    const uint16_t* base = p.in + (int64_t)img * per * p.C;
    float acc = 0.f;
    for (int ty = 0; ty < 3; ++ty) {
      const int iy = y + ty - 1;
      if ((unsigned)iy >= (unsigned)p.H) continue;
      for (int tx = 0; tx < 3; ++tx) {
        const int ix = x + tx - 1;
        if ((unsigned)ix >= (unsigned)p.W) continue;
        const uint4* px = reinterpret_cast<const uint4*>(base + ((int64_t)iy * p.W + ix) * p.C);
        const float* wp = w + (ty * 3 + tx) * p.C;
        for (int c8 = 0; c8 < p.C / 8; ++c8) {
          const uint4 v = px[c8];
          float a0, a1, a2, a3, a4, a5, a6, a7;
          cvt2<F16>(v.x, a0, a1); cvt2<F16>(v.y, a2, a3); cvt2<F16>(v.z, a4, a5); cvt2<F16>(v.w, a6, a7);
          const float* wq = wp + 8 * c8;
          acc = fmaf(a0, wq[0], acc); acc = fmaf(a1, wq[1], acc); acc = fmaf(a2, wq[2], acc); acc = fmaf(a3, wq[3], acc);
          acc = fmaf(a4, wq[4], acc); acc = fmaf(a5, wq[5], acc); acc = fmaf(a6, wq[6], acc); acc = fmaf(a7, wq[7], acc);
        }
      }
    }
    float v = acc + p.bias;
    if (p.aff_out) v = __builtin_fmaf(v, p.aff_out[2 * img + 1], p.aff_out[2 * img]);   // one fma (srcfd.h, the 16-bit precisions)
    if (p.nan_guard && !out_finite<OUT>(v)) { v = 0.f; bad = true; }
    if (OUT == 0) reinterpret_cast<float*>(p.out)[idx] = v;
    else reinterpret_cast<uint16_t*>(p.out)[idx] = (uint16_t)(pack2<OUT == 2>(v, 0.f) & 0xffffu);
  }
  if (p.nan_guard && p.nonfinite) {
    const unsigned long long mask = __ballot(bad);
    if (mask && (threadIdx.x & 63) == 0) atomicAdd(p.nonfinite, (unsigned long long)__popcll(mask));
  }
}

hipError_t launch_outconv16(bool f16, const OutConv16Params& p, unsigned blocks, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.C % 8 != 0 || p.C > 64 || p.C <= 0) return hipErrorInvalidValue;
  const dim3 grid(blocks);
#define GO(F, O) hipLaunchKernelGGL((outconv16<F, O>), grid, dim3(256), 0, s, p)
  if (f16) { if (p.out_dtype == SRCFD_F32) GO(true, 0); else if (p.out_dtype == SRCFD_BF16) GO(true, 1); else GO(true, 2); }
  else { if (p.out_dtype == SRCFD_F32) GO(false, 0); else if (p.out_dtype == SRCFD_BF16) GO(false, 1); else GO(false, 2); }
#undef GO
  return hipGetLastError();
}

}  // namespace srcfd
