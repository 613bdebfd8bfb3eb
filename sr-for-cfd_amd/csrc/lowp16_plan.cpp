// The launch plan of the 16-bit forward (lowp16_plan.h).  Host only.
#include "lowp16_plan.h"

#include <algorithm>

namespace srcfd {

bool dense1_16_qualifies(const GemmDesc& d, int Kpad) {
  return d.MH == 1 && d.MW == 1 && d.K == 64 && Kpad == 64 && d.N == d.Npad && d.N % DENSE1_NF == 0 && d.OC == d.N && d.CI == 64;
}

// Dense layers with few rows and a long K: split K over workgroups (f32 slabs + finish kernel).  The finish kernel stores row m at
// Y + m OC: a layer with a 1x1 OUTPUT.  One row per sample alone does not say that -- the phase ops of a transposed convolution on
// a one-pixel image have it too, and their rows go to (oy0, ox0) of a 2x2 image.
static Gemm16Cut gemm16_cut(const GemmDesc& d, int c) {
  Gemm16Cut q;
  q.bn = d.Npad % 128 == 0 ? 128 : 64;
  if (d.OH == 1 && d.OW == 1 && d.MH == 1 && d.MW == 1 && d.K >= 1024) q.splits = std::max(1, std::min(16, d.K / 256));
  if (q.splits > 1 && (size_t)q.splits * d.M * d.Npad > lowp16_slab_elems(c)) q.splits = 1;
  const bool sk = q.splits > 1;
  q.kslice = sk ? ((d.K / GEMM16_BK + q.splits - 1) / q.splits) * GEMM16_BK : d.K;
  q.nz = sk ? (d.K + q.kslice - 1) / q.kslice : 1;
  q.grid[0] = (d.M + GEMM16_BP - 1) / GEMM16_BP; q.grid[1] = d.Npad / q.bn; q.grid[2] = q.nz;
  q.fin = sk ? (d.M * (d.N / 4) + 255) / 256 : 0;
  q.slab_floats = sk ? (size_t)q.nz * d.M * d.Npad : 0;
  return q;
}

// Batches that do not fill the chip evenly (fewer samples than CUs, or a few more than a multiple of them): cut each sample into S
// segments so that the longest workgroup walks fewer strips.  Cost of a choice = strips walked by the busiest workgroup:
// ceil(n S / CUs) virtual samples of 50/S (+1 warm-up) strips, + 2 rounds of pipeline depth.
static int tail_segments(const Switches& sw, int c, int num_cus) {
  int seg = 1;
  if (sw.tail_seg) seg = sw.tail_seg;   // SRCFD_TAIL_SEG (tests, tools): read per call, reported by srcfd_model_last_plan
  else {
    long best = ((long)(c + num_cus - 1) / num_cus) * 50 + 2;
    for (int cand : {2, 5, 10, 25}) {
      long cost = ((long)((long)c * cand + num_cus - 1) / num_cus) * (50 / cand + 1) + 2;
      if (cost * 115 < best * 100) { best = cost; seg = cand; }  // warm-up strips and extra workgroups are not free: ask for 15 %
    }
  }
  if (seg != 1 && seg != 2 && seg != 5 && seg != 10 && seg != 25) seg = 1;
  return seg;
}

Chunk16Plan plan_chunk16(const Plan16& P, const Graph16& g, const Switches& sw, int c, int num_cus) {
  Chunk16Plan out;
  out.steps.reserve(P.ops.size() + 3);
  const int nops = (int)P.ops.size();
  // functional A/B switches of the tests (both implementations of the encoder, of dense_1 and of the network's middle are complete)
  const bool use_enc = g.fused ? g.enc_ok && sw.enc16 : sw.enc16;   // false: layer-by-layer encoder
  const bool use_mid = g.fused && sw.mid16;                         // false: generic GEMMs
  const bool use_d1 = g.fused && sw.dense1_16;                      // SRCFD_DENSE1=0: dense_1 on the generic GEMM
  int i = 0;     // next op
  int cur;       // the activation buffer the last step wrote
  {  // the encoder front: enc16 (conv2d .. latent_vector in one launch), or conv2d alone when the encoder runs layer by layer
    Step16 s;
    s.src = BUF_X;
    if (use_enc) {
      s.k = Kernel16::Enc;
      while (i < nops && P.ops[i].layer < 4) ++i;   // conv2d_1, dense, latent_vector run inside enc16
      s.nops = i;
      s.dst = 1;   // where the layer-by-layer chain leaves the latent vectors, too
      s.grid[0] = (c + ENC_G - 1) / ENC_G;
    } else {
      s.k = Kernel16::EncConv1;
      s.dst = 0;
      s.grid[0] = (c * 25 * 16 + 255) / 256;
    }
    cur = s.dst;
    out.steps.push_back(s);
  }
  // one GEMM op after the other; the ops of one layer (the output phases of a transposed convolution) read and write the same buffers
  while (i < nops && !(use_mid && P.ops[i].layer >= 5)) {   // ConvT#0 / ConvT#1 run in the fused mid kernel
    const int layer = P.ops[i].layer;
    for (; i < nops && P.ops[i].layer == layer; ++i) {
      const Op16& o = P.ops[i];
      Step16 s;
      s.op0 = i; s.nops = 1;
      s.src = cur; s.dst = cur ^ 1;
      s.d = o.d;
      s.d.M = c * o.d.MH * o.d.MW;
      if (use_d1 && o.layer == 4 && dense1_16_qualifies(s.d, o.Kpad)) {
        s.k = Kernel16::Dense1;
        s.grid[0] = s.d.N / DENSE1_NF;
      } else if (any16_narrow(s.d)) {   // a narrow op (CI 16 / 32) exists on the any16 graphs only: the fused graph refuses CI % 64 != 0
        s.k = Kernel16::GemmN;
        s.grid[0] = (s.d.M + 127) / 128; s.grid[1] = s.d.Npad / 32;
      } else {
        s.k = Kernel16::Gemm;
        s.cut = gemm16_cut(s.d, c);
        out.slab_floats = std::max(out.slab_floats, s.cut.slab_floats);
      }
      out.steps.push_back(s);
    }
    cur ^= 1;
  }
  if (use_mid) {
    Step16 s;
    s.k = Kernel16::Mid;
    s.op0 = i; s.nops = nops - i;
    s.src = cur; s.dst = cur ^ 1;
    s.shape = sw.mid_waves ? (sw.mid_waves == 4 ? MidShape::W4 : sw.mid_waves == 16 ? MidShape::W16 : MidShape::W8)
                           : (sw.mid_shape == 1 ? MidShape::W8 : sw.mid_shape == 2 ? MidShape::W8x2 : MidShape::W4x2);
    const int px = MID_PX[(int)s.shape];
    for (int ph = 0; ph < 4; ++ph) s.nblk[ph] = (c * MID_PHASE_PX[ph] + px - 1) / px;
    cur ^= 1;
    out.steps.push_back(s);
  }
  Step16 s;
  s.op0 = nops;
  s.src = cur; s.dst = BUF_Y;
  if (g.fused) {
    s.k = sw.tail16s ? Kernel16::TailS : Kernel16::Tail;
    s.seg = tail_segments(sw, c, num_cus);
    s.blocks = std::min(c * s.seg, num_cus);
    out.t1_buf = cur;
    out.tail_seg = s.seg;
  } else {
    s.k = Kernel16::OutConv;
    s.grid[0] = (unsigned)(((int64_t)c * g.out_H * g.out_W + 255) / 256);
  }
  out.steps.push_back(s);
  return out;
}

}  // namespace srcfd
