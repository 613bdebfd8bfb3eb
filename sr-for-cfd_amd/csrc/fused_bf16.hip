// Host side of the bf16 / f16 throughput path for the encoder_10 + decoder_400
// graph: weight repacking (16-bit, log2e folding, MFMA fragment order) and the
// four-launch pipeline  enc16 (conv2d .. latent_vector) -> dense1_16 -> mid16
// (ConvT#0 -> ConvT#1) -> tail16; the layer-by-layer launches they replaced
// stay reachable (SRCFD_ENC=0, SRCFD_DENSE1=0, SRCFD_MID=0) for the A/B tests.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "engine.h"
#include "kernels16.h"

namespace srcfd {

struct Pack16 {  // one per operand type (bf16, f16)
  DevBuf<uint16_t> d_w;
  DevBuf<uint8_t> d_consts;
  DevBuf<uint16_t> d_w2f;
  DevBuf<uint16_t> d_w1f;   // mid16: ConvT#1 operands
  DevBuf<uint16_t> d_w0t;   // mid16: ConvT#0 weights as the 16 KB LDS images of its stages, per output phase (offsets in w0t_off)
  size_t w0t_off[4] = {0, 0, 0, 0};
  DevBuf<uint16_t> d_encf;  // enc16: conv2d_1, dense, latent_vector operand fragments (one blob)
  size_t enc_wd_off = 0, enc_wl_off = 0;  // byte offsets of the dense / latent fragments in d_encf
  DevBuf<float> d_encb; // enc16: conv2d_1 bias fragments (128 floats)
  DevBuf<float> d_midb; // mid16: bias fragments (b0f 128 floats, then b1f 64 floats)
  bool built = false;
};

struct FusedState : Fused32Pack {   // host side: operand_pack.h
  DevBuf<float> d_f32;
  Pack16 packs[2];
  DevBuf<uint16_t> act[2];
  DevBuf<float> d_part;  // split-K partial-sum slabs
  int cap = 0;
  int t1_buf = 0;  // which act[] holds ConvT#1's output after the last forward
  int num_cus = 256;
  bool enc_ok = false;     // the encoder has the shape enc16 is written for
};

int fused_init(Model& m) {
  FusedState* fs = new FusedState();
  m.fused = fs;
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, m.device));
  fs->num_cus = prop.multiProcessorCount;
  // conv1's f32 weights and the GEMM ops of compute layers 1..6 (conv2d_1, dense, latent_vector, dense_1, conv2d_transpose, conv2d_transpose_1)
  pack_fused_f32(m.desc, m.ops, m.pack, *fs);
  for (const Op16& o : fs->ops)
    if (o.d.CI % 64 != 0 || o.d.K % 64 != 0 || o.d.N % 4 != 0 || o.d.CO % 4 != 0) { set_error("fused path: unsupported channel count in " + o.name); return SRCFD_EINVAL; }
  if (fs->ops.size() != 9) { set_error("fused path: unexpected plan shape"); return SRCFD_EINVAL; }
  {  // enc16 is written for encoder_10 exactly: 3x3 s1 pad-1 conv 64->128 on 5x5, dense 3200->128, latent 128->64 (padded)
    const GemmDesc& c2 = fs->ops[0].d; const GemmDesc& de = fs->ops[1].d; const GemmDesc& la = fs->ops[2].d;
    const Layer& l0 = m.desc.layers[fs->cl[0]];
    fs->enc_ok = fs->ops[0].layer == 1 && fs->ops[1].layer == 2 && fs->ops[2].layer == 3 && l0.act == SRCFD_ACT_SWISH &&
                 l0.kernel.size() == 9 * 64 && c2.act == SRCFD_ACT_SWISH &&
                 c2.TY == 3 && c2.TX == 3 && c2.CI == 64 && c2.N == 128 && c2.IH == 5 && c2.IW == 5 && c2.MH == 5 && c2.MW == 5 && c2.ay == 1 &&
                 c2.ax == 1 && c2.by == 1 && c2.bx == 1 && c2.cy == -1 && c2.cx == -1 && fs->ops[0].Kpad == 576 &&
                 de.MH == 1 && de.MW == 1 && de.K == 3200 && de.N == 128 && fs->ops[1].Kpad == 3200 &&
                 la.MH == 1 && la.MW == 1 && la.K == 128 && la.N == 64 && fs->ops[2].Kpad == 128;
  }
  return fs->d_f32.upload(fs->f32);
}

// the 16-bit operands of one type (operand_pack.cpp, pack_fused16), uploaded
static int build_pack(Model& m, FusedState* fs, bool f16) {
  Pack16& P = fs->packs[f16 ? 1 : 0];
  if (P.built) return SRCFD_OK;
  Pack16Host h;
  pack_fused16(m.desc, m.ops, m.pack, *fs, fs->enc_ok, f16, h);
  P.enc_wd_off = h.enc_wd_off; P.enc_wl_off = h.enc_wl_off;
  std::copy(h.w0t_off, h.w0t_off + 4, P.w0t_off);
  int rc = P.d_w.upload(h.w);
  if (!rc) rc = P.d_encf.upload(h.encf);
  if (!rc) rc = P.d_encb.upload(h.encb);
  if (!rc) rc = P.d_consts.upload(h.consts);
  if (!rc) rc = P.d_w2f.upload(h.w2f);
  if (!rc) rc = P.d_w0t.upload(h.w0t);
  if (!rc) rc = P.d_w1f.upload(h.w1f);
  if (!rc) rc = P.d_midb.upload(h.midb);
  if (rc) return rc;
  P.built = true;
  return SRCFD_OK;
}

void fused_free(Model& m) {
  delete m.fused;   // FusedState is complete only here
  m.fused = nullptr;
}

int fused_debug_read(Model& m, int index, void* dst, size_t bytes) {
  FusedState* fs = m.fused;
  if (!fs || !fs->act[index]) { set_error("no fused activations yet"); return SRCFD_EINVAL; }
  if (bytes > (size_t)fs->cap * 160000 * sizeof(uint16_t)) { set_error("read past the activation buffer"); return SRCFD_EINVAL; }
  HIPCHECK(hipSetDevice(m.device));
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(dst, fs->act[index == 0 ? fs->t1_buf : fs->t1_buf ^ 1].get(), bytes, hipMemcpyDeviceToHost));
  return SRCFD_OK;
}

static const size_t ACT_ELEMS = 160000;  // largest inter-kernel activation per sample: (50,50,64)

// Everything the 16-bit forward of an n-sample batch allocates or packs lazily: the operand packs of the current operand
// type and the two activation buffers (+ split-K slabs).  Called by the forward itself and by srcfd_model_reserve.
int fused_reserve(Model& m, int n) {
  FusedState* fs = m.fused;
  if (!fs) { set_error("fused path not initialised"); return SRCFD_EINVAL; }
  const bool f16 = m.precision == SRCFD_PREC_F16;
  int rc = build_pack(m, fs, f16);
  if (rc) return rc;
  const int want = std::min(n, 1024);
  if (want > fs->cap) {
    m.drop_graph();  // a captured forward holds the old buffers' addresses
    fs->cap = 0;
    for (auto& b : fs->act) { rc = b.alloc((size_t)want * ACT_ELEMS); if (rc) return rc; }
    rc = fs->d_part.alloc((size_t)16 * want * 128);  // dense(3200->128): up to 16 K-slice slabs of (rows x 128) f32
    if (rc) return rc;
    fs->cap = want;
  }
  return SRCFD_OK;
}

int fused_forward(Model& m, const float* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype, int flags,
                  unsigned long long* nonfinite, hipStream_t s) {
  FusedState* fs = m.fused;
  if (!fs) { set_error("fused path not initialised"); return SRCFD_EINVAL; }
  const bool f16 = m.precision == SRCFD_PREC_F16;
  int rc = fused_reserve(m, n);
  if (rc) return rc;
  const Pack16& P = fs->packs[f16 ? 1 : 0];
  const float* const d_f32 = fs->d_f32.get();
  uint16_t* const act[2] = {fs->act[0].get(), fs->act[1].get()};
  const size_t osz = out_dtype == SRCFD_F32 ? 4 : 2;
  for (int i0 = 0; i0 < n; i0 += fs->cap) {
    const int c = std::min(fs->cap, n - i0);
    const float* xin = x_dev + (size_t)i0 * 100;
    const float* ain = aff_in ? aff_in + 2 * (size_t)i0 : nullptr;
    const float* aout = aff_out ? aff_out + 2 * (size_t)i0 : nullptr;
    int cur = 0;
    // functional A/B switches of the tests (both implementations of the encoder, of dense_1 and of the network's middle are complete):
    // read once per call by Model::predict_device (Switches, engine.h), part of the hipGraph key
    const bool use_enc = fs->enc_ok && m.sw.enc16;   // false: layer-by-layer encoder
    const bool use_mid = m.sw.mid16;                 // false: generic GEMMs
    const bool use_d1 = m.sw.dense1_16;              // false: dense_1 on the generic GEMM
    if (use_enc) {
      EncParams ep;
      ep.x = xin; ep.affine = ain; ep.n = c;
      ep.w1 = d_f32 + fs->c1w_off; ep.b1 = d_f32 + fs->c1b_off;
      ep.w2f = P.d_encf.get(); ep.b2f = P.d_encb.get();
      ep.wdf = (const char*)P.d_encf.get() + P.enc_wd_off; ep.bd = d_f32 + fs->ops[1].b_off;
      ep.wlf = (const char*)P.d_encf.get() + P.enc_wl_off; ep.bl = d_f32 + fs->ops[2].b_off;
      ep.z = act[1];
      ep.act_dense = fs->ops[1].d.act; ep.act_latent = fs->ops[2].d.act;
      ep.prof = nullptr;
#ifdef SRCFD_DIAG
      static unsigned long long* d_eprof = nullptr;
      static int eprof_calls = 0;
      static const bool eprof = getenv("SRCFD_ENC_PROF") != nullptr;
      if (eprof && !d_eprof) HIPCHECK(hipMalloc(&d_eprof, 64 * sizeof(unsigned long long)));
      ep.prof = eprof ? d_eprof : nullptr;
#endif
      rc = m.launch("encoder(conv2d..latent_vector)", s, [&] { return launch_enc16(f16, ep, s); });
      if (rc) return rc;
#ifdef SRCFD_DIAG
      if (eprof && ++eprof_calls == 20) {
        unsigned long long hbuf[64];
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipMemcpy(hbuf, d_eprof, sizeof(hbuf), hipMemcpyDeviceToHost));
        fprintf(stderr, "enc16 workgroup 7, s_memtime ticks since entry: staged, conv2d, conv2d_1 MFMA, A2 ready, dense, end\n");
        for (int w = 0; w < 8; ++w)
          fprintf(stderr, "  wave %d: %6llu %6llu %6llu %6llu %6llu %6llu\n", w, hbuf[w * 8 + 1], hbuf[w * 8 + 2], hbuf[w * 8 + 3], hbuf[w * 8 + 4], hbuf[w * 8 + 5], hbuf[w * 8 + 6]);
      }
#endif
      cur = 1;   // where the layer-by-layer chain leaves the latent vectors, too
    } else {
      rc = m.launch("conv2d", s, [&] { return launch_enc_conv1_16(f16, xin, ain, d_f32 + fs->c1w_off, d_f32 + fs->c1b_off, act[0], c, s); });
      if (rc) return rc;
    }
    int prev_layer = -1;
    for (const Op16& o : fs->ops) {
      if (use_enc && o.layer < 4) continue;  // conv2d_1, dense, latent_vector ran inside enc16
      if (use_mid && o.layer >= 5) break;  // ConvT#0 / ConvT#1 run in the fused mid kernel below
      if (o.layer != prev_layer && prev_layer >= 0) cur ^= 1;
      prev_layer = o.layer;
      GemmDesc d = o.d;
      d.M = c * d.MH * d.MW;
      const uint16_t* X = act[cur];
      uint16_t* Y = act[cur ^ 1];
      // dense layers with few rows and a long K: split K over workgroups (f32 slabs + finish kernel)
      int splits = 1;
      if (d.MH == 1 && d.MW == 1 && d.K >= 1024) splits = std::max(1, std::min(16, d.K / 256));
      if (splits > 1 && (size_t)splits * d.M * d.Npad > fs->d_part.size()) splits = 1;
      if (use_d1 && o.layer == 4 && dense1_16_qualifies(d, o.Kpad))
        rc = m.launch(o.name.c_str(), s, [&] { return launch_dense1_16(f16, d, X, P.d_w.get() + o.w_off, d_f32 + o.b_off, Y, s); });
      else
        rc = m.launch(o.name.c_str(), s, [&] { return launch_gemm16(f16, d, X, P.d_w.get() + o.w_off, o.Kpad, d_f32 + o.b_off, Y, fs->d_part.get(), splits, s); });
      if (rc) return rc;
    }
    if (use_mid) {
      cur ^= 1;  // dense_1 output
      MidParams mp;
      mp.in = act[cur];
      mp.out = act[cur ^ 1];
      mp.n = c;
      int ph = 0;
      for (const Op16& o : fs->ops)
        if (o.layer == 5) { mp.w0[ph] = P.d_w.get() + o.w_off; mp.kpad[ph] = o.Kpad; mp.w0t[ph] = P.d_w0t.get() + P.w0t_off[ph]; ++ph; }
      mp.b0f = P.d_midb.get();
      mp.w1f = P.d_w1f.get();
      mp.b1f = P.d_midb.get() + 128;
      mp.ablate = 0;
      mp.order = m.sw.mid_order;
      mp.prof = nullptr;
#ifdef SRCFD_DIAG
      { static const int abl = [] { const char* e = getenv("SRCFD_MID_ABLATE"); return e ? atoi(e) : 0; }(); mp.ablate = abl; }
      static unsigned long long* d_mprof = nullptr;   // SRCFD_MID_PROF=1: section cycle sums of wave 0 of every workgroup, per output phase
      static int mprof_calls = 0;
      static const bool mprof = getenv("SRCFD_MID_PROF") != nullptr;
      if (mprof && !d_mprof) { HIPCHECK(hipMalloc(&d_mprof, 60 * sizeof(unsigned long long))); }
      if (mprof) { HIPCHECK(hipMemsetAsync(d_mprof, 0, 60 * sizeof(unsigned long long), s)); mp.prof = d_mprof; }
#endif
      const int mid_waves = m.sw.mid_waves ? m.sw.mid_waves : (m.sw.mid_shape == 1 ? 8 : m.sw.mid_shape == 2 ? 82 : 42);
      rc = m.launch("mid(convT0+convT1)", s, [&] { return launch_mid16(f16, mp, mid_waves, s); });
      if (rc) return rc;
#ifdef SRCFD_DIAG
      if (mprof && ++mprof_calls == 20) {
        unsigned long long hb[60];
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipMemcpy(hb, d_mprof, sizeof(hb), hipMemcpyDeviceToHost));
        fprintf(stderr, "mid16, wave 0 of every workgroup, mean cycles per workgroup by output phase: workgroups | entry->tables | ->first stage ready | main loop | ConvT#0 swish | ConvT#1 stage\n");
        for (int ph = 0; ph < 4; ++ph) {
          const double nwg = (double)std::max<unsigned long long>(hb[ph * 6], 1);
          fprintf(stderr, "  phase %d: %6llu | %7.0f | %7.0f | %7.0f | %7.0f | %7.0f    main loop = sync %7.0f + issue %7.0f + fragments/MFMA %7.0f\n", ph, hb[ph * 6], hb[ph * 6 + 1] / nwg, hb[ph * 6 + 2] / nwg, hb[ph * 6 + 3] / nwg,
                  hb[ph * 6 + 4] / nwg, hb[ph * 6 + 5] / nwg, hb[24 + ph * 3] / nwg, hb[24 + ph * 3 + 1] / nwg, hb[24 + ph * 3 + 2] / nwg);
        }
        fprintf(stderr, "  workgroup 3 of phase 0, per wave, main loop: sync | issue | fragments/MFMA\n");
        for (int w = 0; w < 8; ++w) fprintf(stderr, "    wave %d: %7llu | %7llu | %7llu\n", w, hb[36 + w * 3], hb[36 + w * 3 + 1], hb[36 + w * 3 + 2]);
      }
#endif
    }
    cur ^= 1;
    fs->t1_buf = cur;
    TailParams tp;
    tp.in = act[cur];
    tp.out = (char*)y_dev + (size_t)i0 * 160000 * osz;
    tp.n = c;
    tp.consts = P.d_consts.get();
    tp.w2frags = P.d_w2f.get();
    tp.aff_out = aout;
    tp.nan_guard = flags & SRCFD_FLAG_NAN_GUARD;
    tp.nonfinite = nonfinite;
    tp.out_dtype = out_dtype;
    tp.ablate = 0;
    tp.prof = nullptr;
#ifdef SRCFD_DIAG
    { static const int abl = [] { const char* e = getenv("SRCFD_TAIL_ABLATE"); return e ? atoi(e) : 0; }(); tp.ablate = abl; }
    static unsigned long long* d_prof = nullptr;   // SRCFD_TAIL_PROF=1: per-wave section timers of workgroup 0 (synchronises: never under graph capture)
    static int prof_calls = 0;
    static const bool prof = getenv("SRCFD_TAIL_PROF") != nullptr;
    if (prof && !d_prof) HIPCHECK(hipMalloc(&d_prof, 128 * sizeof(unsigned long long)));
    tp.prof = prof ? d_prof : nullptr;
#endif
    // Batches that do not fill the chip evenly (fewer samples than CUs, or a few more than a multiple of them): cut each
    // sample into S segments so that the longest workgroup walks fewer strips.  Cost of a choice = strips walked by the
    // busiest workgroup: ceil(n S / CUs) virtual samples of 50/S (+1 warm-up) strips, + 2 rounds of pipeline depth.
    int seg = 1;
    if (m.sw.tail_seg) seg = m.sw.tail_seg;   // SRCFD_TAIL_SEG (tests, tools): read per call, reported by srcfd_model_last_plan
    else {
      long best = ((long)(c + fs->num_cus - 1) / fs->num_cus) * 50 + 2;
      for (int cand : {2, 5, 10, 25}) {
        long cost = ((long)((long)c * cand + fs->num_cus - 1) / fs->num_cus) * (50 / cand + 1) + 2;
        if (cost * 115 < best * 100) { best = cost; seg = cand; }  // warm-up strips and extra workgroups are not free: ask for 15 %
      }
    }
    if (seg != 1 && seg != 2 && seg != 5 && seg != 10 && seg != 25) seg = 1;
    tp.seg = seg;
    m.plan.tail_seg = seg;
    const int blocks = std::min(c * seg, fs->num_cus);
    const bool tail_s = m.sw.tail16s;
    rc = m.launch("tail(convT2-4+out)", s, [&] { return tail_s ? launch_tail16s(f16, tp, blocks, s) : launch_tail16(f16, tp, blocks, s); });
    if (rc) return rc;
#ifdef SRCFD_DIAG
    if (prof && ++prof_calls == 20) {
      unsigned long long h[128];
      HIPCHECK(hipStreamSynchronize(s));
      HIPCHECK(hipMemcpy(h, d_prof, sizeof(h), hipMemcpyDeviceToHost));
      if (tail_s) {
        fprintf(stderr, "tail16s workgroup 0, per wave: fast rounds (work cycles, barrier wait cycles, count) | other rounds (work, wait, count)\n");
        for (int w = 0; w < 8; ++w)
          fprintf(stderr, "  wave %d: %9llu %9llu %5llu | %9llu %9llu %5llu   per fast round: work %6.0f wait %6.0f\n", w, h[w * 6], h[w * 6 + 1], h[w * 6 + 2],
                  h[w * 6 + 3], h[w * 6 + 4], h[w * 6 + 5], h[w * 6 + 2] ? (double)h[w * 6] / h[w * 6 + 2] : 0.0, h[w * 6 + 2] ? (double)h[w * 6 + 1] / h[w * 6 + 2] : 0.0);
        fprintf(stderr, "  cycles per fast round and section (top, then the blocks in issue order):\n");
        for (int w = 0; w < 8; ++w) {
          fprintf(stderr, "  wave %d:", w);
          for (int i = 0; i < 10; ++i) fprintf(stderr, " %6.0f", h[w * 6 + 2] ? (double)h[48 + w * 10 + i] / h[w * 6 + 2] : 0.0);
          fprintf(stderr, "\n");
        }
      } else {
        fprintf(stderr, "tail16 workgroup 0, cycles per wave: D, BC, A, barrier wait, total\n");
        for (int w = 0; w < 16; ++w)
          fprintf(stderr, "  wave %2d: %9llu %9llu %9llu %9llu %9llu\n", w, h[w * 5], h[w * 5 + 1], h[w * 5 + 2], h[w * 5 + 3], h[w * 5 + 4]);
      }
    }
#endif
  }
  return SRCFD_OK;
}

// ---------------------------------------------------------------------------
// any16: the 16-bit forward of encoder_10 + the other decoders of the family.  enc16 -> per layer gemm16 (CI % 64 == 0) or
// gemm16n (CI 16 / 32) -> outconv16; the layer-by-layer encoder stays reachable with SRCFD_ENC=0, like on the fused path.
// ---------------------------------------------------------------------------
struct Any16State : Any16Pack {
  struct Dev {
    DevBuf<uint16_t> d_w, d_encf;
    DevBuf<float> d_encb, d_wout;
    size_t enc_wd_off = 0, enc_wl_off = 0;
    std::vector<size_t> w_off;
    bool built = false;
  } packs[2];
  DevBuf<float> d_f32;
  DevBuf<uint16_t> act[2];
  DevBuf<float> d_part;
  int cap = 0;
};

void any16_create(Model& m) {
  Any16State* st = new Any16State();
  any16_plan(m.desc, m.ops, m.pack, *st);
  if (!st->ok) { delete st; return; }
  m.any16 = st;
}

void any16_free(Model& m) {
  delete m.any16;
  m.any16 = nullptr;
}

int any16_init(Model& m) { return m.any16->d_f32.upload(m.any16->f32); }

static int any16_build_pack(Model& m, Any16State* st, bool f16) {
  Any16State::Dev& P = st->packs[f16 ? 1 : 0];
  if (P.built) return SRCFD_OK;
  Any16Host h;
  pack_any16(m.desc, m.ops, m.pack, *st, f16, h);
  P.enc_wd_off = h.enc_wd_off; P.enc_wl_off = h.enc_wl_off;
  P.w_off.clear();
  for (const Op16& o : st->ops) P.w_off.push_back(o.w_off);
  int rc = P.d_w.upload(h.w);
  if (!rc) rc = P.d_encf.upload(h.encf);
  if (!rc) rc = P.d_encb.upload(h.encb);
  if (!rc) rc = P.d_wout.upload(h.wout);
  if (rc) return rc;
  P.built = true;
  return SRCFD_OK;
}

// two activation buffers of the graph's largest activation + the dense split-K slabs, for min(n, 1024) samples
size_t any16_workspace_bytes(const Model& m, int n) {
  const size_t want = (size_t)std::min(std::max(n, 0), 1024);
  return want ? 2 * want * m.any16->max_act * sizeof(uint16_t) + 16 * want * 128 * sizeof(float) : 0;
}

int any16_reserve(Model& m, int n) {
  Any16State* st = m.any16;
  if (!st) { set_error("any16 path not initialised"); return SRCFD_EINVAL; }
  int rc = any16_build_pack(m, st, m.precision == SRCFD_PREC_F16);
  if (rc) return rc;
  const int want = std::min(n, 1024);
  if (want > st->cap) {
    m.drop_graph();  // a captured forward holds the old buffers' addresses
    st->cap = 0;
    for (auto& b : st->act) { rc = b.alloc((size_t)want * st->max_act); if (rc) return rc; }
    rc = st->d_part.alloc((size_t)16 * want * 128);
    if (rc) return rc;
    st->cap = want;
  }
  return SRCFD_OK;
}

int any16_forward(Model& m, const float* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype, int flags,
                  unsigned long long* nonfinite, hipStream_t s) {
  Any16State* st = m.any16;
  if (!st) { set_error("any16 path not initialised"); return SRCFD_EINVAL; }
  const bool f16 = m.precision == SRCFD_PREC_F16;
  int rc = any16_reserve(m, n);
  if (rc) return rc;
  const Any16State::Dev& P = st->packs[f16 ? 1 : 0];
  const float* const d_f32 = st->d_f32.get();
  uint16_t* const act[2] = {st->act[0].get(), st->act[1].get()};
  const size_t osz = out_dtype == SRCFD_F32 ? 4 : 2;
  const size_t out_elems = (size_t)st->out_H * st->out_W;
  for (int i0 = 0; i0 < n; i0 += st->cap) {
    const int c = std::min(st->cap, n - i0);
    const float* xin = x_dev + (size_t)i0 * 100;
    const float* ain = aff_in ? aff_in + 2 * (size_t)i0 : nullptr;
    const float* aout = aff_out ? aff_out + 2 * (size_t)i0 : nullptr;
    int cur = 0;
    const bool use_enc = m.sw.enc16;   // false: layer-by-layer encoder (functional A/B switch, part of the hipGraph key)
    if (use_enc) {
      EncParams ep;
      ep.x = xin; ep.affine = ain; ep.n = c;
      ep.w1 = d_f32 + st->c1w_off; ep.b1 = d_f32 + st->c1b_off;
      ep.w2f = P.d_encf.get(); ep.b2f = P.d_encb.get();
      ep.wdf = (const char*)P.d_encf.get() + P.enc_wd_off; ep.bd = d_f32 + st->ops[1].b_off;
      ep.wlf = (const char*)P.d_encf.get() + P.enc_wl_off; ep.bl = d_f32 + st->ops[2].b_off;
      ep.z = act[1];
      ep.act_dense = st->ops[1].d.act; ep.act_latent = st->ops[2].d.act;
      ep.prof = nullptr;
      rc = m.launch("encoder(conv2d..latent_vector)", s, [&] { return launch_enc16(f16, ep, s); });
      if (rc) return rc;
      cur = 1;   // where the layer-by-layer chain leaves the latent vectors, too
    } else {
      rc = m.launch("conv2d", s, [&] { return launch_enc_conv1_16(f16, xin, ain, d_f32 + st->c1w_off, d_f32 + st->c1b_off, act[0], c, s); });
      if (rc) return rc;
    }
    int prev_layer = -1;
    for (size_t oi = 0; oi < st->ops.size(); ++oi) {
      const Op16& o = st->ops[oi];
      if (use_enc && o.layer < 4) continue;  // conv2d_1, dense, latent_vector ran inside enc16
      if (o.layer != prev_layer && prev_layer >= 0) cur ^= 1;
      prev_layer = o.layer;
      GemmDesc d = o.d;
      d.M = c * d.MH * d.MW;
      const uint16_t* X = act[cur];
      uint16_t* Y = act[cur ^ 1];
      const uint16_t* W = P.d_w.get() + P.w_off[oi];
      if (any16_narrow(d)) {
        rc = m.launch(o.name.c_str(), s, [&] { return launch_gemm16n(f16, d, X, W, o.Kpad, d_f32 + o.b_off, Y, s); });
      } else {
        int splits = 1;   // dense layers with few rows and a long K: split K over workgroups (f32 slabs + finish kernel)
        if (d.MH == 1 && d.MW == 1 && d.K >= 1024) splits = std::max(1, std::min(16, d.K / 256));
        if (splits > 1 && (size_t)splits * d.M * d.Npad > st->d_part.size()) splits = 1;
        rc = m.launch(o.name.c_str(), s, [&] { return launch_gemm16(f16, d, X, W, o.Kpad, d_f32 + o.b_off, Y, st->d_part.get(), splits, s); });
      }
      if (rc) return rc;
    }
    cur ^= 1;   // the last GEMM layer's output
    OutConv16Params op;
    op.in = act[cur];
    op.out = (char*)y_dev + (size_t)i0 * out_elems * osz;
    op.n = c; op.H = st->out_H; op.W = st->out_W; op.C = st->out_C;
    op.w = P.d_wout.get(); op.bias = st->out_bias;
    op.aff_out = aout; op.nan_guard = flags & SRCFD_FLAG_NAN_GUARD; op.nonfinite = nonfinite; op.out_dtype = out_dtype;
    rc = m.launch(m.desc.layers[st->cl.back()].name.c_str(), s, [&] { return launch_outconv16(f16, op, s); });
    if (rc) return rc;
  }
  return SRCFD_OK;
}

}  // namespace srcfd
