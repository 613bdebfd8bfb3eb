// Host side of the bf16 / f16 throughput path: the device state of both graphs, the uploads of their operands (packed by
// operand_pack.cpp), the reserve, and the loop that issues a chunk's launches.
// encoder_10 + decoder_400 (the fused graph) is the four-launch pipeline  enc16 (conv2d .. latent_vector) -> dense1_16 -> mid16
// (ConvT#0 -> ConvT#1) -> tail16; the layer-by-layer launches they replaced stay reachable (SRCFD_ENC=0, SRCFD_DENSE1=0,
// SRCFD_MID=0) for the A/B tests.  encoder_10 + the other decoders of the family (any16) run  enc16 -> per layer gemm16
// (CI % 64 == 0) or gemm16n (CI 16 / 32) -> outconv16.  Both graphs share one device state and reserve (Lowp16State).  What a
// chunk launches -- kernels, buffers, split-K cuts, grids, mid16's shape, the tail's segmentation -- is decided by plan_chunk16
// (lowp16_plan.h, host only, tested on a CPU); issue_chunk below fills the parameter structs and launches, and decides nothing.
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

struct Dev16 {  // one per operand type (bf16, f16): what both graphs upload
  DevBuf<uint16_t> d_w;     // GEMM weights, Wt[Npad][Kpad] per op
  DevBuf<uint16_t> d_encf;  // enc16: conv2d_1, dense, latent_vector operand fragments (one blob)
  size_t enc_wd_off = 0, enc_wl_off = 0;  // byte offsets of the dense / latent fragments in d_encf
  DevBuf<float> d_encb; // enc16: conv2d_1 bias fragments (128 floats)
  bool built = false;
  int upload(const std::vector<uint16_t>& w, const Enc16Host& e) {
    enc_wd_off = e.enc_wd_off; enc_wl_off = e.enc_wl_off;
    int rc = d_w.upload(w);
    if (!rc) rc = d_encf.upload(e.encf);
    if (!rc) rc = d_encb.upload(e.encb);
    return rc;
  }
};

struct Lowp16State {  // Model::lowp16: what both graphs hold; FusedState when Model::has_fused, else Any16State
  Plan16 plan;             // host side (operand_pack.h)
  DevBuf<float> d_f32;
  Dev16 dev[2];
  DevBuf<uint16_t> act[2];
  DevBuf<float> d_part;  // split-K partial-sum slabs
  int cap = 0;
  virtual ~Lowp16State() = default;
};

struct FusedState : Lowp16State {
  struct Dev {  // one per operand type
    DevBuf<uint8_t> d_consts;
    DevBuf<uint16_t> d_w2f;
    DevBuf<uint16_t> d_w1f;   // mid16: ConvT#1 operands
    DevBuf<uint16_t> d_w0t;   // mid16: ConvT#0 weights as the 16 KB LDS images of its stages, per output phase (offsets in w0t_off)
    size_t w0t_off[4] = {0, 0, 0, 0};
    DevBuf<float> d_midb; // mid16: bias fragments (b0f 128 floats, then b1f 64 floats)
  } fx[2];
  int t1_buf = 0;  // which act[] holds ConvT#1's output after the last forward
  bool enc_ok = false;     // the encoder has the shape enc16 is written for
};

struct Any16State : Lowp16State {
  Any16Pack out;            // the output convolution, the largest activation
  DevBuf<float> d_wout[2];  // per operand type
};
static FusedState& fused_of(Lowp16State& st) { return static_cast<FusedState&>(st); }
static Any16State& any16_of(Lowp16State& st) { return static_cast<Any16State&>(st); }
// largest inter-kernel activation per sample, elements: (50,50,64) on the fused graph
static size_t act_elems(const Model& m) { return m.has_fused ? 160000 : static_cast<const Any16State&>(*m.lowp16).out.max_act; }

void lowp16_free(Lowp16State* st) { delete st; }   // the states are complete only here

void lowp16_plan(Model& m) {
  if (m.has_fused) {
    m.lowp16.reset(new FusedState());
    // conv1's f32 weights and the GEMM ops of compute layers 1..6 (conv2d_1, dense, latent_vector, dense_1, conv2d_transpose, conv2d_transpose_1)
    plan16(m.desc, m.ops, m.pack, 6, false, m.lowp16->plan);
    return;
  }
  Plan16 plan;
  Any16Pack out;
  any16_plan(m.desc, m.ops, m.pack, plan, out);
  if (!out.ok) return;
  Any16State* st = new Any16State();
  m.lowp16.reset(st);
  st->plan = std::move(plan);
  st->out = std::move(out);
}

static int fused_init(Model& m, FusedState* fs) {
  for (const Op16& o : fs->plan.ops)
    if (o.d.CI % 64 != 0 || o.d.K % 64 != 0 || o.d.N % 4 != 0 || o.d.CO % 4 != 0) { set_error("fused path: unsupported channel count in " + o.name); return SRCFD_EINVAL; }
  if (fs->plan.ops.size() != 9) { set_error("fused path: unexpected plan shape"); return SRCFD_EINVAL; }
  {  // enc16 is written for encoder_10 exactly: 3x3 s1 pad-1 conv 64->128 on 5x5, dense 3200->128, latent 128->64 (padded)
    const std::vector<Op16>& ops = fs->plan.ops;
    const GemmDesc& c2 = ops[0].d; const GemmDesc& de = ops[1].d; const GemmDesc& la = ops[2].d;
    const Layer& l0 = m.desc.layers[fs->plan.cl[0]];
    fs->enc_ok = ops[0].layer == 1 && ops[1].layer == 2 && ops[2].layer == 3 && l0.act == SRCFD_ACT_SWISH &&
                 l0.kernel.size() == 9 * 64 && c2.act == SRCFD_ACT_SWISH &&
                 c2.TY == 3 && c2.TX == 3 && c2.CI == 64 && c2.N == 128 && c2.IH == 5 && c2.IW == 5 && c2.MH == 5 && c2.MW == 5 && c2.ay == 1 &&
                 c2.ax == 1 && c2.by == 1 && c2.bx == 1 && c2.cy == -1 && c2.cx == -1 && ops[0].Kpad == 576 &&
                 de.MH == 1 && de.MW == 1 && de.K == 3200 && de.N == 128 && ops[1].Kpad == 3200 &&
                 la.MH == 1 && la.MW == 1 && la.K == 128 && la.N == 64 && ops[2].Kpad == 128;
  }
  return SRCFD_OK;
}

int lowp16_init(Model& m) {
  Lowp16State& st = *m.lowp16;
  if (m.has_fused) { int rc = fused_init(m, &fused_of(st)); if (rc) return rc; }
  return st.d_f32.upload(st.plan.f32);
}

// the 16-bit operands of one type (operand_pack.cpp, pack_fused16 / pack_any16), packed and uploaded at the type's first use
static int build_pack(Model& m, Lowp16State* st, bool f16) {
  Dev16& P = st->dev[f16 ? 1 : 0];
  if (P.built) return SRCFD_OK;
  int rc;
  if (m.has_fused) {
    FusedState* fs = &fused_of(*st);
    FusedState::Dev& X = fs->fx[f16 ? 1 : 0];
    Pack16Host h;
    pack_fused16(m.desc, m.ops, m.pack, fs->plan, fs->enc_ok, f16, h);
    std::copy(h.w0t_off, h.w0t_off + 4, X.w0t_off);
    rc = P.upload(h.w, h);
    if (!rc) rc = X.d_consts.upload(h.consts);
    if (!rc) rc = X.d_w2f.upload(h.w2f);
    if (!rc) rc = X.d_w0t.upload(h.w0t);
    if (!rc) rc = X.d_w1f.upload(h.w1f);
    if (!rc) rc = X.d_midb.upload(h.midb);
  } else {
    Any16Host h;
    pack_any16(m.desc, m.ops, m.pack, st->plan, f16, h);
    rc = P.upload(h.w, h);
    if (!rc) rc = any16_of(*st).d_wout[f16 ? 1 : 0].upload(h.wout);
  }
  if (rc) return rc;
  P.built = true;
  return SRCFD_OK;
}

int fused_debug_read(Model& m, int index, void* dst, size_t bytes) {
  FusedState* fs = m.has_fused && m.lowp16 ? &fused_of(*m.lowp16) : nullptr;
  if (!fs || !fs->act[index]) { set_error("no fused activations yet"); return SRCFD_EINVAL; }
  if (bytes > (size_t)fs->cap * act_elems(m) * sizeof(uint16_t)) { set_error("read past the activation buffer"); return SRCFD_EINVAL; }
  HIPCHECK(hipSetDevice(m.device));
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(dst, fs->act[index == 0 ? fs->t1_buf : fs->t1_buf ^ 1].get(), bytes, hipMemcpyDeviceToHost));
  return SRCFD_OK;
}

// A forward runs chunks of up to 1024 samples through two activation buffers of the graph's largest activation and the split-K
// slabs (lowp16_slab_elems, lowp16_plan.h: no chunk's plan needs more).  gemm16 forms its element offsets into a chunk's
// activations in 32-bit int, so a chunk holds fewer samples where 1024 of the graph's largest activation would pass 2^31 elements
// (any16_plan refuses a single activation of that size; the fused graph's 1024 x 160000 is far below).
int lowp16_chunk_cap(const Model& m) { return (int)std::min<size_t>(1024, (((size_t)1 << 31) - 1) / act_elems(m)); }
static size_t chunk_of(const Model& m, int n) { return (size_t)std::min(std::max(n, 0), lowp16_chunk_cap(m)); }
size_t lowp16_workspace_bytes(const Model& m, int n) {
  const size_t want = chunk_of(m, n);
  return want ? 2 * want * act_elems(m) * sizeof(uint16_t) + lowp16_slab_elems(want) * sizeof(float) : 0;
}

// Everything the 16-bit forward of an n-sample batch allocates or packs lazily: the operand packs of the current operand
// type and the two activation buffers (+ split-K slabs).  Called by the forward itself and by srcfd_model_reserve.
int lowp16_reserve(Model& m, int n) {
  Lowp16State* st = m.lowp16.get();
  if (!st) { set_error(m.has_fused ? "fused path not initialised" : "any16 path not initialised"); return SRCFD_EINVAL; }
  int rc = build_pack(m, st, m.precision == SRCFD_PREC_F16);
  if (rc) return rc;
  const int want = (int)chunk_of(m, n);
  if (want > st->cap) {
    m.drop_graph();  // a captured forward holds the old buffers' addresses
    st->cap = 0;
    for (auto& b : st->act) { rc = b.alloc((size_t)want * act_elems(m)); if (rc) return rc; }
    rc = st->d_part.alloc(lowp16_slab_elems(want));
    if (rc) return rc;
    st->cap = want;
  }
  return SRCFD_OK;
}

#ifdef SRCFD_DIAG
// The diagnostic library: work-skipping switches (SRCFD_MID_ABLATE, SRCFD_TAIL_ABLATE) and the section timers of the fused graph's
// kernels (SRCFD_ENC_PROF, SRCFD_MID_PROF, SRCFD_TAIL_PROF=1).  *_arm hands a launch its counters, *_report prints them behind
// the 20th launch (it synchronises: never under graph capture).
static unsigned long long* d_eprof = nullptr;
static unsigned long long* d_mprof = nullptr;   // section cycle sums of wave 0 of every workgroup, per output phase
static unsigned long long* d_tprof = nullptr;   // per-wave section timers of workgroup 0
static int eprof_calls = 0, mprof_calls = 0, tprof_calls = 0;
static bool diag_on(const char* name) { return getenv(name) != nullptr; }
static int diag_int(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
static int diag_enc_arm(EncParams& ep) {
  static const bool eprof = diag_on("SRCFD_ENC_PROF");
  if (eprof && !d_eprof) HIPCHECK(hipMalloc(&d_eprof, 64 * sizeof(unsigned long long)));
  ep.prof = eprof ? d_eprof : nullptr;
  return SRCFD_OK;
}
static int diag_enc_report(hipStream_t s) {
  if (!d_eprof || ++eprof_calls != 20) return SRCFD_OK;
  unsigned long long hbuf[64];
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(hbuf, d_eprof, sizeof(hbuf), hipMemcpyDeviceToHost));
  fprintf(stderr, "enc16 workgroup 7, s_memtime ticks since entry: staged, conv2d, conv2d_1 MFMA, A2 ready, dense, end\n");
  for (int w = 0; w < 8; ++w)
    fprintf(stderr, "  wave %d: %6llu %6llu %6llu %6llu %6llu %6llu\n", w, hbuf[w * 8 + 1], hbuf[w * 8 + 2], hbuf[w * 8 + 3], hbuf[w * 8 + 4], hbuf[w * 8 + 5], hbuf[w * 8 + 6]);
  return SRCFD_OK;
}
static int diag_mid_arm(MidParams& mp, hipStream_t s) {
  static const int abl = diag_int("SRCFD_MID_ABLATE");
  static const bool mprof = diag_on("SRCFD_MID_PROF");
  mp.ablate = abl;
  if (mprof && !d_mprof) { HIPCHECK(hipMalloc(&d_mprof, 60 * sizeof(unsigned long long))); }
  if (mprof) { HIPCHECK(hipMemsetAsync(d_mprof, 0, 60 * sizeof(unsigned long long), s)); mp.prof = d_mprof; }
  return SRCFD_OK;
}
static int diag_mid_report(hipStream_t s) {
  if (!d_mprof || ++mprof_calls != 20) return SRCFD_OK;
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
  return SRCFD_OK;
}
static int diag_tail_arm(TailParams& tp) {
  static const int abl = diag_int("SRCFD_TAIL_ABLATE");
  static const bool prof = diag_on("SRCFD_TAIL_PROF");
  tp.ablate = abl;
  if (prof && !d_tprof) HIPCHECK(hipMalloc(&d_tprof, 128 * sizeof(unsigned long long)));
  tp.prof = prof ? d_tprof : nullptr;
  return SRCFD_OK;
}
static int diag_tail_report(bool tail_s, hipStream_t s) {
  if (!d_tprof || ++tprof_calls != 20) return SRCFD_OK;
  unsigned long long h[128];
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(h, d_tprof, sizeof(h), hipMemcpyDeviceToHost));
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
  return SRCFD_OK;
}
#else
static int diag_enc_arm(EncParams&) { return SRCFD_OK; }
static int diag_enc_report(hipStream_t) { return SRCFD_OK; }
static int diag_mid_arm(MidParams&, hipStream_t) { return SRCFD_OK; }
static int diag_mid_report(hipStream_t) { return SRCFD_OK; }
static int diag_tail_arm(TailParams&) { return SRCFD_OK; }
static int diag_tail_report(bool, hipStream_t) { return SRCFD_OK; }
#endif

// Issues the steps of one chunk's plan (lowp16_plan.h): fills each kernel's parameters from the device state and launches under the
// names the profile reports.  Every decision -- kernels, buffers, cuts, grids, shapes, segmentation -- is the plan's.
static int issue_chunk(Model& m, Lowp16State& st, const Chunk16Plan& plan, bool f16, int c, const float* xin, const float* ain, const float* aout,
                       void* y, int out_dtype, int flags, unsigned long long* nonfinite, hipStream_t s) {
  const Plan16& h = st.plan;
  const Dev16& P = st.dev[f16 ? 1 : 0];
  const float* const d_f32 = st.d_f32.get();
  for (const Step16& q : plan.steps) {
    const uint16_t* const X = q.src >= 0 ? st.act[q.src].get() : nullptr;
    uint16_t* const Y = q.dst >= 0 ? st.act[q.dst].get() : nullptr;
    const Op16* const o = q.nops ? &h.ops[q.op0] : nullptr;
    int rc = SRCFD_OK;
    switch (q.k) {
      case Kernel16::EncConv1:
        rc = m.launch("conv2d", s, [&] { return launch_enc_conv1_16(f16, xin, ain, d_f32 + h.c1w_off, d_f32 + h.c1b_off, Y, c, q.grid[0], s); });
        break;
      case Kernel16::Enc: {
        EncParams ep;
        ep.x = xin; ep.affine = ain; ep.n = c;
        ep.w1 = d_f32 + h.c1w_off; ep.b1 = d_f32 + h.c1b_off;
        ep.w2f = P.d_encf.get(); ep.b2f = P.d_encb.get();
        ep.wdf = (const char*)P.d_encf.get() + P.enc_wd_off; ep.bd = d_f32 + h.ops[1].b_off;
        ep.wlf = (const char*)P.d_encf.get() + P.enc_wl_off; ep.bl = d_f32 + h.ops[2].b_off;
        ep.z = Y;
        ep.act_dense = h.ops[1].d.act; ep.act_latent = h.ops[2].d.act;
        ep.prof = nullptr;
        rc = m.has_fused ? diag_enc_arm(ep) : SRCFD_OK;   // the section timers are the fused graph's
        if (!rc) rc = m.launch("encoder(conv2d..latent_vector)", s, [&] { return launch_enc16(f16, ep, q.grid[0], s); });
        if (!rc && m.has_fused) rc = diag_enc_report(s);
        break;
      }
      case Kernel16::Dense1:
        rc = m.launch(o->name.c_str(), s, [&] { return launch_dense1_16(f16, q.d, X, P.d_w.get() + o->w_off, d_f32 + o->b_off, Y, q.grid[0], s); });
        break;
      case Kernel16::GemmN:
        rc = m.launch(o->name.c_str(), s, [&] { return launch_gemm16n(f16, q.d, X, P.d_w.get() + o->w_off, o->Kpad, d_f32 + o->b_off, Y, q.grid, s); });
        break;
      case Kernel16::Gemm:
        rc = m.launch(o->name.c_str(), s, [&] {
          // the reserve holds every plan's slabs (tests/test_lowp16_plan.py); a buffer that did not is withheld, and the launcher refuses
          float* const part = q.cut.slab_floats <= st.d_part.size() ? st.d_part.get() : nullptr;
          return launch_gemm16(f16, q.d, X, P.d_w.get() + o->w_off, o->Kpad, d_f32 + o->b_off, Y, part, q.cut, s);
        });
        break;
      case Kernel16::Mid: {
        const FusedState::Dev& F = fused_of(st).fx[f16 ? 1 : 0];
        MidParams mp;
        mp.in = X; mp.out = Y; mp.n = c;
        int ph = 0;
        for (int i = q.op0; i < q.op0 + q.nops; ++i)
          if (h.ops[i].layer == 5) { mp.w0[ph] = P.d_w.get() + h.ops[i].w_off; mp.kpad[ph] = h.ops[i].Kpad; mp.w0t[ph] = F.d_w0t.get() + F.w0t_off[ph]; ++ph; }
        mp.b0f = F.d_midb.get();
        mp.w1f = F.d_w1f.get();
        mp.b1f = F.d_midb.get() + 128;
        std::copy(q.nblk, q.nblk + 4, mp.nblk);
        mp.ablate = 0;
        mp.order = m.sw.mid_order;
        mp.prof = nullptr;
        rc = diag_mid_arm(mp, s);
        if (!rc) rc = m.launch("mid(convT0+convT1)", s, [&] { return launch_mid16(f16, mp, q.shape, s); });
        if (!rc) rc = diag_mid_report(s);
        break;
      }
      case Kernel16::Tail:
      case Kernel16::TailS: {
        const FusedState::Dev& F = fused_of(st).fx[f16 ? 1 : 0];
        const bool tail_s = q.k == Kernel16::TailS;
        TailParams tp;
        tp.in = X; tp.out = y; tp.n = c;
        tp.consts = F.d_consts.get();
        tp.w2frags = F.d_w2f.get();
        tp.aff_out = aout;
        tp.nan_guard = flags & SRCFD_FLAG_NAN_GUARD;
        tp.nonfinite = nonfinite;
        tp.out_dtype = out_dtype;
        tp.ablate = 0;
        tp.prof = nullptr;
        tp.seg = q.seg;
        rc = diag_tail_arm(tp);
        if (!rc) rc = m.launch("tail(convT2-4+out)", s, [&] { return tail_s ? launch_tail16s(f16, tp, q.blocks, s) : launch_tail16(f16, tp, q.blocks, s); });
        if (!rc) rc = diag_tail_report(tail_s, s);
        break;
      }
      case Kernel16::OutConv: {
        const Any16State& as = any16_of(st);
        OutConv16Params op;
        op.in = X; op.out = y;
        op.n = c; op.H = as.out.out_H; op.W = as.out.out_W; op.C = as.out.out_C;
        op.w = as.d_wout[f16 ? 1 : 0].get(); op.bias = as.out.out_bias;
        op.aff_out = aout; op.nan_guard = flags & SRCFD_FLAG_NAN_GUARD; op.nonfinite = nonfinite; op.out_dtype = out_dtype;
        rc = m.launch(m.desc.layers[h.cl.back()].name.c_str(), s, [&] { return launch_outconv16(f16, op, q.grid[0], s); });
        break;
      }
    }
    if (rc) return rc;
  }
  return SRCFD_OK;
}

int lowp16_forward(Model& m, const float* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype, int flags,
                   unsigned long long* nonfinite, hipStream_t s) {
  int rc = lowp16_reserve(m, n);
  if (rc) return rc;
  Lowp16State& st = *m.lowp16;
  const bool f16 = m.precision == SRCFD_PREC_F16;
  const int* os = m.desc.out_shape();
  const size_t out_bytes = (size_t)os[0] * os[1] * os[2] * (out_dtype == SRCFD_F32 ? 4 : 2);   // per sample
  Graph16 g;
  g.fused = m.has_fused;
  if (m.has_fused) g.enc_ok = fused_of(st).enc_ok;
  else { g.out_H = any16_of(st).out.out_H; g.out_W = any16_of(st).out.out_W; }
  for (int i0 = 0; i0 < n; i0 += st.cap) {
    const int c = std::min(st.cap, n - i0);
    const Chunk16Plan plan = plan_chunk16(st.plan, g, m.sw, c, m.num_cus);
    if (m.has_fused) { fused_of(st).t1_buf = plan.t1_buf; m.plan.tail_seg = plan.tail_seg; }
    const float* xin = x_dev + (size_t)i0 * 100;
    const float* ain = aff_in ? aff_in + 2 * (size_t)i0 : nullptr;
    const float* aout = aff_out ? aff_out + 2 * (size_t)i0 : nullptr;
    void* y = (char*)y_dev + (size_t)i0 * out_bytes;
    rc = issue_chunk(m, st, plan, f16, c, xin, ain, aout, y, out_dtype, flags, nonfinite, s);
    if (rc) return rc;
  }
  return SRCFD_OK;
}

}  // namespace srcfd
