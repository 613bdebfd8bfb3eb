// srcfd engine: builds the kernel plan for a layer graph, owns device weights
// and workspaces, and exports the model part of the C ABI (include/srcfd.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"

namespace srcfd {

thread_local std::string g_last_error;
void set_error(const std::string& m) { g_last_error = m; }

// ---------------------------------------------------------------------------
// plan: which fused kernels the graph qualifies for; their operand layouts are operand_pack.cpp's
// ---------------------------------------------------------------------------
static bool is_k2s2(const Layer& L) { return L.kind == SRCFD_LAYER_CONV2D_TRANSPOSE && L.kh == 2 && L.kw == 2 && L.stride == 2; }

// Operands of the fused ConvT pair (kernels_fp32.hip, convt_pair_f32), appended to `pack`
static void plan_convt_pair(Model& m) {
  m.pair_op = -1;
  for (size_t i = 0; i + 1 < m.ops.size(); ++i) {
    const Op &a = m.ops[i], &b = m.ops[i + 1];
    const Layer &La = m.desc.layers[a.layer], &Lb = m.desc.layers[b.layer];
    if (a.layer + 1 != b.layer || !is_k2s2(La) || !is_k2s2(Lb)) continue;
    if (a.d.nphx != 2 || b.d.nphx != 2) continue;  // one op per layer (the merged-phase form)
    if (La.cin != 32 || La.cout != 16 || Lb.cin != 16 || Lb.cout != 8) continue;
    m.pair = pack_convt_pair(m.pack, La, Lb);
    m.pair_op = (int)i;
    return;
  }
}

// Operands of the three-layer chain (convt_triple_f32)
static void plan_convt_triple(Model& m) {
  m.triple_op = -1;
  for (size_t i = 0; i + 2 < m.ops.size(); ++i) {
    const Op &a = m.ops[i], &b = m.ops[i + 1], &c = m.ops[i + 2];
    if (a.layer + 1 != b.layer || b.layer + 1 != c.layer) continue;
    const Layer &L1 = m.desc.layers[a.layer], &L2 = m.desc.layers[b.layer], &L3 = m.desc.layers[c.layer];
    if (!is_k2s2(L1) || !is_k2s2(L2) || !is_k2s2(L3) || a.d.nphx != 2 || b.d.nphx != 2 || c.d.nphx != 2) continue;
    if (L1.cin != 64 || L1.cout != 32 || L2.cin != 32 || L2.cout != 16 || L3.cin != 16 || L3.cout != 8) continue;
    m.tri = pack_convt_triple(m.pack, L1, L2, L3);
    m.triple_op = (int)i;
    return;
  }
}

// Operands of the fused f32 tail (kernels_tail32.hip): the ConvT 64 -> 32 -> 16 -> 8 chain + the 3x3 SAME conv 8 -> 1 that
// ends the network
static void plan_tail32(Model& m) {
  m.tail32_op = -1;
  if (m.triple_op < 0 || (size_t)m.triple_op + 4 != m.ops.size()) return;
  const size_t i = (size_t)m.triple_op;
  const Op& last = m.ops[i + 3];
  if (last.layer != m.ops[i + 2].layer + 1) return;
  const Layer &L1 = m.desc.layers[m.ops[i].layer], &L2 = m.desc.layers[m.ops[i + 1].layer], &L3 = m.desc.layers[m.ops[i + 2].layer];
  const Layer& LO = m.desc.layers[last.layer];
  if (LO.kind != SRCFD_LAYER_CONV2D || LO.kh != 3 || LO.kw != 3 || LO.stride != 1 || !LO.same || LO.cin != 8 || LO.cout != 1) return;
  if (m.ops[i].d.MW > 50) return;  // the LDS ring holds rows of up to 400 pixels
  if (L1.act != SRCFD_ACT_SWISH || L2.act != SRCFD_ACT_SWISH || L3.act != SRCFD_ACT_SWISH || LO.act != SRCFD_ACT_LINEAR) return;
  m.t32 = pack_tail32(m.pack, L1, L2, L3, LO);
  m.tail32_op = (int)i;
}

// SRCFD_PREC_FP32X3: the ops gemm_x3 takes get their weights split into three bf16 planes (kernels_x3.hip), and the streaming
// tail's first two layers likewise (kernels_tail32.hip, X3)
static void plan_x3(Model& m) {
  m.x3_off.assign(m.ops.size(), -1);
  m.pack_x3.clear();
  for (size_t i = 0; i < m.ops.size(); ++i) {
    GemmDesc d = m.ops[i].d;
    d.M = 0;
    if (!gemm_x3_qualifies(d)) continue;
    align64(m.pack_x3);
    m.x3_off[i] = (int64_t)m.pack_x3.size();
    m.pack_x3.resize(m.pack_x3.size() + (size_t)3 * d.N * gemm_x3_kpad(d));
    gemm_x3_split_weights(d, m.pack.data() + m.ops[i].w_off, m.pack_x3.data() + m.x3_off[i]);
  }
  m.t32_w1x = m.t32_w2x = -1;
  if (m.tail32_op >= 0)
    pack_tail32_x3(m.pack_x3, m.desc.layers[m.ops[m.tail32_op].layer], m.desc.layers[m.ops[m.tail32_op + 1].layer], m.t32_w1x, m.t32_w2x);
}

// enc32 (kernels_enc32.hip): the encoder's four compute layers as one launch.  conv2d_1's weights are re-ordered into
// v_mfma_f32_16x16x4_f32 A fragments; the other three layers use their ordinary B[K][Npad] operands.
static void plan_enc32(Model& m) {
  m.enc32_ok = false;
  if (m.ops.size() < 4 || m.desc.in_shape[0] != 10 || m.desc.in_shape[1] != 10 || m.desc.in_shape[2] != 1) return;
  for (int i = 0; i < 3; ++i) if (m.ops[i + 1].layer == m.ops[i].layer) return;   // one op per layer
  if (m.ops.size() > 4 && m.ops[4].layer == m.ops[3].layer) return;
  const GemmDesc &c1 = m.ops[0].d, &c2 = m.ops[1].d, &de = m.ops[2].d, &la = m.ops[3].d;
  const Layer &L0 = m.desc.layers[m.ops[0].layer], &L1 = m.desc.layers[m.ops[1].layer];
  auto act_ok = [](int a) { return a == SRCFD_ACT_SWISH || a == SRCFD_ACT_LINEAR; };
  if (L0.kind != SRCFD_LAYER_CONV2D || L0.kh != 3 || L0.kw != 3 || L0.stride != 2 || !L0.same || L0.cin != 1 || L0.cout != 64 || c1.Npad != 64) return;
  if (L1.kind != SRCFD_LAYER_CONV2D || L1.kh != 3 || L1.kw != 3 || L1.stride != 1 || !L1.same || L1.cin != 64 || L1.cout != 128 || c2.MH != 5 || c2.MW != 5) return;
  if (de.MH != 1 || de.MW != 1 || de.K != 3200 || de.N != 128 || de.Npad != 128) return;
  if (la.MH != 1 || la.MW != 1 || la.K != 128 || la.N > 128 || la.OC != la.N) return;
  if (!act_ok(c1.act) || !act_ok(c2.act) || !act_ok(de.act) || !act_ok(la.act)) return;
  m.enc32_w2 = pack_enc32(m.pack, L1);
  m.enc32_ok = true;
}

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
Model::~Model() {
  if (device >= 0) (void)hipSetDevice(device);   // for the members' destructors (device_mem.h; lowp16's state is one of them)
}

Switches Switches::from_env() {
  auto on = [](const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; };
  Switches w;
  w.enc16 = on("SRCFD_ENC", true);
  w.mid16 = on("SRCFD_MID", true);
  { const char* e = getenv("SRCFD_MID"); const int v = e ? atoi(e) : 0; if (v >= 1 && v <= 3) w.mid_shape = v; }
  w.dense1_16 = on("SRCFD_DENSE1", true);
  w.enc32 = !on("SRCFD_NO_ENC32", false);
  w.skinny32 = !on("SRCFD_NO_DENSE_SKINNY", false);
  w.tail32 = !on("SRCFD_NO_TAIL32", false);
  w.triple = !on("SRCFD_NO_TRIPLE", false);
  w.pair = !on("SRCFD_NO_PAIR", false);
  w.gemm32_big = !on("SRCFD_NO_GEMM32_BIG", false);
  { const char* t = getenv("SRCFD_TAIL"); w.tail16s = t && t[0] == 's'; }
  { const char* e = getenv("SRCFD_MID_ORDER"); if (e) w.mid_order = atoi(e) == 1 ? 1 : 0; }
  { const char* e = getenv("SRCFD_MID_WAVES"); const int v = e ? atoi(e) : 0; w.mid_waves = (v == 4 || v == 16) ? v : 0; }
  const char* e = getenv("SRCFD_TAIL_SEG");
  const int seg = e ? atoi(e) : 0;
  w.tail_seg = (seg == 1 || seg == 2 || seg == 5 || seg == 10 || seg == 25) ? seg : 0;
  return w;
}

void Model::drop_graph() {
  graph_exec.reset();
  graph_key = GraphKey();
}

int Model::init_device() {
  if (device < 0) return SRCFD_OK;
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available (libsrcfd has no CPU fallback)");
    return SRCFD_ENODEV;
  }
  if (device >= cnt) { set_error("device index out of range"); return SRCFD_EINVAL; }
  HIPCHECK(hipSetDevice(device));
  { hipDeviceProp_t prop; HIPCHECK(hipGetDeviceProperties(&prop, device)); num_cus = prop.multiProcessorCount; }
  int rc = d_pack.upload(pack);
  return rc ? rc : d_pack_x3.upload(pack_x3);
}

// bf16 / f16 need 16-bit kernels for every layer: the fused encoder_10 + decoder_400 kernels, or any16's layer loop (fused_bf16.hip)
static const char* const LOWP_REFUSAL =
    "bf16/f16 precision needs encoder_10 in front, Dense / 2x2 or 3x3 stride-2 Conv2DTranspose layers with input channels a multiple of 16 behind it and a "
    "3x3 'same' Conv2D to one channel at the end (the encoder_10+decoder_400 layer graph is one); use SRCFD_PREC_FP32 for other graphs";

// ---------------------------------------------------------------------------
// The f32-grade forward's kernel choice.  f32_step answers "which kernel takes op i at batch n" for the launch loop
// (forward_generic) and for everything that sizes its buffers (max_act_elems, splitk_need): no HIP calls, nothing allocated.
// ---------------------------------------------------------------------------
// Descriptors of ops [i, i + count) at batch n and, with `w`, their device operands
void Model::f32_span(size_t i, int count, int n, GemmDesc ds[4], F32Operands* w) const {
  for (int q = 0; q < count; ++q) {
    const Op& op = ops[i + q];
    ds[q] = op.d;
    ds[q].M = n * ds[q].MH * ds[q].MW;
    if (!w) continue;
    w->B[q] = d_pack.get() + op.w_off;
    w->Bx[q] = x3_off[i + q] >= 0 ? d_pack_x3.get() + x3_off[i + q] : nullptr;
    w->bias[q] = d_pack.get() + op.b_off;
  }
}

// enc32: standardise + the encoder's four layers as one launch in front of the loop
size_t Model::f32_first(int precision, const Switches& sw) const { return enc32_ok && sw.enc32 && precision != SRCFD_PREC_FP32_NAIVE ? 4 : 0; }

F32Step Model::f32_step(size_t i, int n, int precision, const Switches& sw, bool x3) const {
  if (precision == SRCFD_PREC_FP32_NAIVE) return {F32Kernel::Naive, 1, false};   // the bring-up path: every op on its own
  // SRCFD_PREC_FP32X3: the split-bf16 kernels from 64 samples per call on (x3_for): below that their serial k loops lose to the generic
  // f32 kernels' split-K launches (tools/precision_sweep.py: 0.26 vs 0.13 ms at 3 samples, break-even between 48 and 96), so small
  // calls run exactly the SRCFD_PREC_FP32 path.  The caller decides once per call; a chunk of any size follows, so a sample's bits
  // do not depend on where the call was cut.
  int cnt = 1;   // the ops of one layer (ConvT output phases) are launched together
  while (i + cnt < ops.size() && ops[i + cnt].layer == ops[i].layer && cnt < 4) ++cnt;
  GemmDesc ds[4];
  f32_span(i, cnt, n, ds);
  if (i + 1 == ops.size() && gemm_fuses_finalize(ds[0])) return {F32Kernel::Finalize, 1, false};   // last layer: epilogue writes the caller's buffer directly
  if (sw.tail32 && (int)i == tail32_op) return {F32Kernel::Tail32, 4, x3 && t32_w1x >= 0 && t32_w2x >= 0};   // ConvT#2 -> #3 -> #4 -> output conv + finalize
  if (sw.pair && sw.triple && (int)i == triple_op && i + 3 < ops.size()) return {F32Kernel::Triple, 3, false};   // ConvT#2 -> #3 -> #4
  if (sw.pair && (int)i == pair_op && i + 2 < ops.size()) return {F32Kernel::Pair, 2, false};   // ConvT#3 -> ConvT#4 (kernels.h, PairDesc)
  if (x3) {   // every GEMM of the layer on the split-bf16 kernel, or none
    bool all = true;
    for (int q = 0; q < cnt && all; ++q) all = x3_off[i + q] >= 0 && gemm_x3_qualifies(ds[q]);
    if (all) return {F32Kernel::X3Group, cnt, false};
  }
  if (cnt == 1 && sw.skinny32 && dense_skinny32_qualifies(ds[0])) return {F32Kernel::Skinny, 1, false};
  if (sw.gemm32_big && gemm32_big_qualifies(ds, cnt)) return {F32Kernel::Big, cnt, false};   // sums its K slabs in registers: no slab workspace
  return {cnt > 1 ? F32Kernel::Group : F32Kernel::Mfma, cnt, false};
}

// Largest activation that sits in a ping-pong buffer.  With the streaming tail (tail32) the layers from its first one on
// never materialise: the largest tensor of the f32 path is then ConvT#1's output (640 KB per sample, not 5.12 MB).
size_t Model::max_act_elems(int precision, const Switches& sw) const {
  size_t m = (size_t)desc.in_shape[0] * desc.in_shape[1] * desc.in_shape[2];
  int stop = (int)desc.layers.size();
  F32Step st;
  for (size_t i = 0; i < ops.size() && stop == (int)desc.layers.size(); i += st.count) {
    st = f32_step(i, 1, precision, sw, false);   // the streaming tail is chosen whatever x3 says
    if (st.k == F32Kernel::Tail32) stop = ops[i].layer;
  }
  for (int i = 0; i < stop; ++i) {
    const Layer& L = desc.layers[i];
    m = std::max(m, (size_t)L.out_shape[0] * L.out_shape[1] * L.out_shape[2]);
  }
  return m;
}

// Samples per pass of the layer-by-layer path: two buffers of the largest activation within 3 GB, at most 1024 samples
// (batch 256 = 768 samples runs as one pass with the streaming tail, as three without it).
int Model::chunk_cap(int precision, const Switches& sw) const {
  size_t per = 2 * max_act_elems(precision, sw) * sizeof(float);
  size_t cap = ((size_t)3 << 30) / std::max<size_t>(per, 1);
  return (int)std::max<size_t>(1, std::min<size_t>(cap, 1024));
}

// Split-K slab floats of an n-sample chunk: what the generic GEMM launches that f32_step returns FOR THAT n ask for.  Not
// monotonic in n: a layer that gemm32_big takes at a large batch needs slabs at a small one.
size_t Model::splitk_need(int n, int precision, const Switches& sw, bool x3) const {
  size_t need = 0;
  F32Step st;
  for (size_t i = f32_first(precision, sw); i < ops.size(); i += st.count) {
    st = f32_step(i, n, precision, sw, x3);
    if (st.k != F32Kernel::Group && st.k != F32Kernel::Mfma) continue;
    GemmDesc ds[4];
    f32_span(i, st.count, n, ds);
    need = std::max(need, gemm_group_ws_floats(ds, st.count));   // the plan's ws_floats: what the launcher will insist on
  }
  return need;
}

// Buffers of an n-sample forward: the two activation buffers grow to the call's chunk, the slabs to what its chunks (whole ones
// and the remainder) ask for; neither shrinks on a smaller call.
int Model::ensure_workspace(int n, const Switches& sw, bool x3) {
  const int chunk = std::min(n, chunk_cap(precision, sw));
  const size_t per = max_act_elems(precision, sw);   // depends on the precision: the bring-up path materialises every layer
  const bool grow = chunk > ws_chunk || per > ws_per_sample;
  const int step = grow ? chunk : ws_chunk;   // predict_device's chunks: min(n, step) samples, then n % step
  const size_t need = std::max(splitk_need(std::min(n, step), precision, sw, x3), n > step && n % step ? splitk_need(n % step, precision, sw, x3) : 0);
  if (!grow && need <= d_splitk.size()) return SRCFD_OK;
  drop_graph();  // a captured forward holds the old buffers' addresses
  if (need > d_splitk.size()) { int rc = d_splitk.alloc(need); if (rc) return rc; }
  if (grow) {
    ws_chunk = 0;
    for (auto& b : buf) { int rc = b.alloc((size_t)chunk * per); if (rc) return rc; }
    ws_per_sample = per;
    ws_chunk = chunk;
  }
  return SRCFD_OK;
}

int Model::launch(const char* name, hipStream_t s, const std::function<hipError_t()>& fn) {
  ProfEvent* pe = nullptr;
  if (profiling) {
    if (prof_used == prof_events.size()) {
      ProfEvent e;
      HIPCHECK(hipEventCreate(e.a.out()));
      HIPCHECK(hipEventCreate(e.b.out()));
      prof_events.push_back(std::move(e));
    }
    pe = &prof_events[prof_used++];
    pe->name = name;
    HIPCHECK(hipEventRecord(pe->a, s));
  }
  hipError_t e = fn();
  if (e != hipSuccess) { set_error(std::string("launch of ") + name + " failed: " + hipGetErrorString(e)); return SRCFD_EHIP; }
  if (pe) HIPCHECK(hipEventRecord(pe->b, s));
  return SRCFD_OK;
}

// f32-grade forward of one chunk (<= ws_chunk samples): the steps of f32_step, one launch each.
int Model::forward_generic(const float* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype,
                           int flags, unsigned long long* nonfinite, hipStream_t s) {
  const int in_elems = desc.in_shape[0] * desc.in_shape[1] * desc.in_shape[2];
  const int* os = desc.out_shape();
  const int out_elems = os[0] * os[1] * os[2];
  const int guard = flags & SRCFD_FLAG_NAN_GUARD;
  const float* const d_pack = this->d_pack.get();
  float* const buf[2] = {this->buf[0].get(), this->buf[1].get()};
  int rc = SRCFD_OK;
  const size_t first = f32_first(precision, sw);
  if (first) {   // standardise + the encoder's four layers: one launch, latent vectors into buf[0]
    Enc32Params ep;
    ep.x = x_dev; ep.affine = aff_in; ep.n = n;
    ep.w1 = d_pack + ops[0].w_off; ep.b1 = d_pack + ops[0].b_off;
    ep.w2f = d_pack + enc32_w2; ep.b2 = d_pack + ops[1].b_off;
    ep.wd = d_pack + ops[2].w_off; ep.bd = d_pack + ops[2].b_off;
    ep.wl = d_pack + ops[3].w_off; ep.bl = d_pack + ops[3].b_off;
    ep.z = buf[0];
    ep.nl = ops[3].d.N; ep.nl_pad = ops[3].d.Npad;
    ep.act1 = ops[0].d.act; ep.act2 = ops[1].d.act; ep.act3 = ops[2].d.act; ep.act4 = ops[3].d.act;
    rc = launch("encoder(standardize..latent_vector)", s, [&] { return launch_enc32(ep, s); });
  } else {
    rc = launch("standardize", s, [&] { return launch_standardize(x_dev, buf[0], aff_in, in_elems, (int64_t)n * in_elems, s); });
  }
  int cur = 0;   // buf[cur]: the input of the next step
  F32Step st;
  for (size_t i = first; i < ops.size() && !rc; i += st.count) {
    st = f32_step(i, n, precision, sw, x3_call);
    const Op& op = ops[i];
    GemmDesc ds[4];
    F32Operands w;
    f32_span(i, st.count, n, ds, &w);
    const GemmDesc& d = ds[0];
    const float* X = buf[cur];
    float* Y = buf[cur ^ 1];
    const size_t next = i + st.count;
    if (next == ops.size() || ops[next].layer != ops[next - 1].layer) cur ^= 1;   // the next step starts a new layer: it reads what this one writes
    const char* name = (st.count > 1 ? desc.layers[op.layer].name : op.name).c_str();   // the output phases of one layer go by the layer's name
    std::string nm;   // of a launch that spans layers
    switch (st.k) {
      case F32Kernel::Finalize:
        return launch(name, s, [&] { return launch_gemm_finalize(d, X, w.B[0], w.bias[0], y_dev, out_dtype, aff_out, guard, nonfinite, s); });
      case F32Kernel::Tail32: {   // one streaming kernel up to the caller's buffer
        Tail32Params tp;
        tp.in = X; tp.out = y_dev; tp.n = n; tp.H = d.MH; tp.W = d.MW;
        tp.w1f = d_pack + t32.w1; tp.b1 = d_pack + t32.b1; tp.w2f = d_pack + t32.w2; tp.b2 = d_pack + t32.b2;
        tp.w3f = d_pack + t32.w3; tp.b3 = d_pack + t32.b3; tp.wc = d_pack + t32.wc;
        tp.aff_out = aff_out; tp.nan_guard = guard; tp.nonfinite = nonfinite; tp.out_dtype = out_dtype;
        tp.seg = tail32_segments(n, d.MH, num_cus);
        if (st.x3_tail) {   // SRCFD_PREC_FP32X3: the first two layers on the bf16 matrix cores
          tp.w1x = d_pack_x3.get() + t32_w1x;
          tp.w2x = d_pack_x3.get() + t32_w2x;
        }
#ifdef SRCFD_DIAG
        { static const int abl = [] { const char* e = getenv("SRCFD_TAIL32_ABLATE"); return e ? atoi(e) : 0; }(); tp.ablate = abl; }
#endif
        name = (nm = op.name + "+" + ops[i + 1].name + "+" + ops[i + 2].name + "+" + ops[i + 3].name + (st.x3_tail ? "(x3)" : "")).c_str();
        return launch(name, s, [&] { return launch_tail32(tp, num_cus, s); });
      }
      case F32Kernel::Triple: {
        TripleDesc td;
        td.n = n; td.H = d.MH; td.W = d.MW; td.act1 = d.act; td.act2 = ds[1].act; td.act3 = ds[2].act;
        name = (nm = op.name + "+" + ops[i + 1].name + "+" + ops[i + 2].name).c_str();
        rc = launch(name, s, [&] {
          return launch_convt_triple_f32(td, X, d_pack + tri.w1, d_pack + tri.b1, d_pack + tri.w2, d_pack + tri.b2, d_pack + tri.w3,
                                         d_pack + tri.b3, Y, s);
        });
        break;
      }
      case F32Kernel::Pair: {
        PairDesc pd;
        pd.n = n; pd.H = d.MH; pd.W = d.MW; pd.act_a = d.act; pd.act_b = ds[1].act;
        name = (nm = op.name + "+" + ops[i + 1].name).c_str();
        rc = launch(name, s, [&] { return launch_convt_pair_f32(pd, X, d_pack + pair.wa, d_pack + pair.ba, d_pack + pair.wb, d_pack + pair.bb, Y, s); });
        break;
      }
      case F32Kernel::X3Group:   // the layer's output phases: one launch (kernels_x3.hip, X3Group); a single-op layer: its own kernel
        nm = op.name;
        if (st.count > 1) { const size_t dot = nm.rfind(".ph"); if (dot != std::string::npos) nm.resize(dot); }
        name = (nm += "(x3)").c_str();
        rc = launch(name, s, [&] { return launch_gemm_x3_group(ds, st.count, X, w.Bx, w.bias, Y, s, num_cus); });
        break;
      case F32Kernel::Big:
        rc = launch(name, s, [&] { return launch_gemm32_big(ds, st.count, X, w.B, w.bias, Y, s); });
        break;
      case F32Kernel::Group:   // the output phases of one transposed convolution: one launch (kernels_fp32.hip, GemmGroup)
        rc = launch(name, s, [&] { return launch_gemm_mfma_group(ds, st.count, X, w.B, w.bias, Y, s, d_splitk.get(), d_splitk.size()); });
        break;
      case F32Kernel::Skinny:
        rc = launch(name, s, [&] { return launch_dense_skinny32(d, X, w.B[0], w.bias[0], Y, s); });
        break;
      case F32Kernel::Mfma:
        rc = launch(name, s, [&] { return launch_gemm_mfma(d, X, w.B[0], w.bias[0], Y, s, d_splitk.get(), d_splitk.size()); });
        break;
      case F32Kernel::Naive:
        rc = launch(name, s, [&] { return launch_gemm_naive(d, X, w.B[0], w.bias[0], Y, s); });
        break;
    }
  }
  if (rc) return rc;
  return launch("finalize", s, [&] { return launch_finalize(buf[cur], y_dev, out_dtype, aff_out, out_elems, (int64_t)n * out_elems, guard, nonfinite, s); });
}

int Model::predict_device(const void* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype, int flags,
                          unsigned long long* nonfinite, hipStream_t s, int call_n) {
  if (device < 0) { set_error("host-only handle: no device was requested at create"); return SRCFD_ENODEV; }
  if (n < 0) { set_error("negative batch"); return SRCFD_EINVAL; }
  if (out_dtype != SRCFD_F32 && out_dtype != SRCFD_BF16 && out_dtype != SRCFD_F16) { set_error("unsupported output dtype"); return SRCFD_EINVAL; }
  if (n == 0) return SRCFD_OK;
  HIPCHECK(hipSetDevice(device));
  prof_used = 0;
  sw = Switches::from_env();
  const bool use_fused = (precision == SRCFD_PREC_BF16 || precision == SRCFD_PREC_F16);
  plan = Plan();
  const bool use_any16 = use_fused && !has_fused && lowp16;
  plan.sw = sw; plan.precision = precision; plan.fused = use_fused && !use_any16; plan.any16 = use_any16;
  if (use_fused && !lowp_ok()) { set_error(LOWP_REFUSAL); return SRCFD_EINVAL; }
  x3_call = x3_for(call_n > 0 ? call_n : n, precision);   // once per call: ws_chunk's chunks below and the host entry's all follow it
  if (!use_fused) {
    int rc = ensure_workspace(n, sw, x3_call);  // (re)allocates before anything is captured; drops a stale graph when it does
    if (rc) return rc;
  }
  const int in_elems = desc.in_shape[0] * desc.in_shape[1] * desc.in_shape[2];
  const int* os = desc.out_shape();
  const size_t out_elems = (size_t)os[0] * os[1] * os[2];
  const size_t osz = out_dtype == SRCFD_F32 ? 4 : 2;
  auto run = [&](hipStream_t st) -> int {
    if (use_fused) return lowp16_forward(*this, (const float*)x_dev, n, aff_in, aff_out, y_dev, out_dtype, flags, nonfinite, st);
    for (int i = 0; i < n; i += ws_chunk) {
      int c = std::min(ws_chunk, n - i);
      int rc = forward_generic((const float*)x_dev + (size_t)i * in_elems, c, aff_in ? aff_in + 2 * (size_t)i : nullptr,
                               aff_out ? aff_out + 2 * (size_t)i : nullptr, (char*)y_dev + (size_t)i * out_elems * osz, out_dtype, flags,
                               nonfinite, st);
      if (rc) return rc;
    }
    return SRCFD_OK;
  };
  // hipGraph replay of the whole forward.  Measured on MI355X: at batch 256 replay is no faster than plain launches
  // (0.904 vs 0.894 ms: the gaps between the kernels are not host-bound), but a solver-side call of a few samples is
  // a chain of 8-16 kernels of 4-30 us each and replay takes ~20 us off it (bf16 one-field call 0.214 -> 0.195 ms).
  // Default: small batches only; SRCFD_GRAPH=0 never, SRCFD_GRAPH=1 always.
  static const int graph_env = [] { const char* e = getenv("SRCFD_GRAPH"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }();
  const bool graphs = !profiling && (graph_env == 1 || (graph_env == -1 && n <= 96));
  if (graphs) {
    GraphKey key;
    key.x = x_dev; key.y = y_dev; key.ain = aff_in; key.aout = aff_out; key.nf = nonfinite; key.n = n;
    key.out_dtype = out_dtype; key.flags = flags; key.precision = precision; key.switches = sw.bits(); key.x3 = x3_call;
    if (graph_exec && key == graph_key) {
      HIPCHECK(hipGraphLaunch(graph_exec, s));
      plan = graph_plan; plan.graph = 2;
      return SRCFD_OK;
    }
    if (key == last_key && !(key == graph_key)) {
      // second identical call: every buffer and attribute is set up, so the launches can be captured
      drop_graph();
      if (!graph_stream) HIPCHECK(hipStreamCreateWithFlags(graph_stream.out(), hipStreamNonBlocking));
      HIPCHECK(hipStreamBeginCapture(graph_stream, hipStreamCaptureModeThreadLocal));
      int rc = run(graph_stream);
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamEndCapture(graph_stream, &g);
      if (rc == SRCFD_OK && e == hipSuccess && g) {
        e = hipGraphInstantiate(graph_exec.out(), g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e == hipSuccess) {
          graph_key = key;
          graph_plan = plan;
          HIPCHECK(hipGraphLaunch(graph_exec, s));
          plan.graph = 1;
          return SRCFD_OK;
        }
        graph_exec.reset();
      } else if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError();  // capture not possible here: fall through to plain launches
    }
    last_key = key;
  }
  return run(s);
}

int Model::predict_host(const float* x, int n, const float* aff_in, const float* aff_out, float* y, int flags, int64_t* n_nonfinite,
                        const std::function<int(const float*, int, int)>& sink) {
  if (device < 0) { set_error("host-only handle: no device was requested at create"); return SRCFD_ENODEV; }
  if (n < 0 || (n > 0 && (!x || (!y && !sink)))) { set_error("bad arguments"); return SRCFD_EINVAL; }
  if (n_nonfinite) *n_nonfinite = 0;
  if (n == 0) return SRCFD_OK;
  HIPCHECK(hipSetDevice(device));
  const size_t in_elems = (size_t)desc.in_shape[0] * desc.in_shape[1] * desc.in_shape[2];
  const int* os = desc.out_shape();
  const size_t out_elems = (size_t)os[0] * os[1] * os[2];
  // Is the destination page-locked (srcfd_host_alloc, hipHostMalloc / hipHostRegister)?  Then the device-to-host copy of chunk i runs on
  // a second stream while chunk i + 1 is computed (two result buffers, events both ways) and the whole call moves at the PCIe rate;
  // into pageable memory the copy is staged by the runtime and nothing overlaps (one buffer, as before).
  // The WHOLE range [y, y + n out_elems) must be page-locked, not managed, and one allocation: its first and its last byte are asked
  // (a range that starts in a registered block and runs past its end, or managed memory, takes the staged path).
  bool pinned = false;
  if (y && !sink) {
    hipPointerAttribute_t a0, a1;
    const char* last = reinterpret_cast<const char*>(y) + (size_t)n * out_elems * sizeof(float) - 1;
    if (hipPointerGetAttributes(&a0, y) == hipSuccess && hipPointerGetAttributes(&a1, last) == hipSuccess)
      pinned = a0.type == hipMemoryTypeHost && a1.type == hipMemoryTypeHost && !a0.isManaged && !a1.isManaged &&
               reinterpret_cast<const char*>(a1.hostPointer) - reinterpret_cast<const char*>(a0.hostPointer) == last - reinterpret_cast<const char*>(y);
    else (void)hipGetLastError();
  }
  // On the overlapped path an error exit must not leave earlier chunks' copies into the caller's array in flight (the caller drops
  // the array, the pool hands the buffer to the next call): whatever way this function is left, both streams are drained first.
  struct Drain {
    bool armed; const Stream* cs;
    ~Drain() { if (armed) { if (*cs) (void)hipStreamSynchronize(*cs); (void)hipStreamSynchronize(nullptr); } }
  } drain{pinned, &copy_stream};
  int chunk = std::min(n, pinned ? 128 : STAGE_SAMPLES);
  if (chunk > stage_chunk || (pinned && !d_y_stage2)) {
    chunk = std::max(chunk, stage_chunk);
    stage_chunk = 0;
    drop_graph();   // a captured forward holds the old staging addresses
    int rc = d_x_stage.alloc(chunk * in_elems);
    if (!rc) rc = d_y_stage.alloc(chunk * out_elems);
    if (!rc) rc = pinned ? d_y_stage2.alloc(chunk * out_elems) : d_y_stage2.release();
    if (!rc) rc = d_aff.alloc((size_t)chunk * 4);
    if (rc) return rc;
    stage_chunk = chunk;
  }
  if (pinned && !copy_stream) {
    HIPCHECK(hipStreamCreateWithFlags(copy_stream.out(), hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      HIPCHECK(hipEventCreateWithFlags(ev_computed[b].out(), hipEventDisableTiming));
      HIPCHECK(hipEventCreateWithFlags(ev_copied[b].out(), hipEventDisableTiming));
    }
  }
  if (!d_nonfinite) { int rc = d_nonfinite.alloc(1); if (rc) return rc; }
  HIPCHECK(hipMemsetAsync(d_nonfinite.get(), 0, sizeof(unsigned long long), nullptr));
  const int step = pinned ? std::min(stage_chunk, 128) : stage_chunk;
  int k = 0;
  for (int i = 0; i < n; i += step, ++k) {
    int c = std::min(step, n - i);
    const int b = pinned ? (k & 1) : 0;
    float* ydev = (b ? d_y_stage2 : d_y_stage).get();
    HIPCHECK(hipMemcpyAsync(d_x_stage.get(), x + (size_t)i * in_elems, c * in_elems * sizeof(float), hipMemcpyHostToDevice, nullptr));
    float* ain = nullptr;
    float* aout = nullptr;
    if (aff_in) { ain = d_aff.get(); HIPCHECK(hipMemcpyAsync(ain, aff_in + 2 * (size_t)i, (size_t)c * 2 * sizeof(float), hipMemcpyHostToDevice, nullptr)); }
    if (aff_out) { aout = d_aff.get() + 2 * (size_t)stage_chunk; HIPCHECK(hipMemcpyAsync(aout, aff_out + 2 * (size_t)i, (size_t)c * 2 * sizeof(float), hipMemcpyHostToDevice, nullptr)); }
    if (pinned && k >= 2) HIPCHECK(hipStreamWaitEvent(nullptr, ev_copied[b], 0));   // the buffer's previous contents have left
    int rc = predict_device(d_x_stage.get(), c, ain, aout, ydev, SRCFD_F32, flags, d_nonfinite.get(), nullptr, n);
    if (rc) return rc;
    if (sink) { rc = sink(ydev, i, c); if (rc) return rc; HIPCHECK(hipStreamSynchronize(nullptr)); }
    else if (pinned) {
      HIPCHECK(hipEventRecord(ev_computed[b], nullptr));
      HIPCHECK(hipStreamWaitEvent(copy_stream, ev_computed[b], 0));
      HIPCHECK(hipMemcpyAsync(y + (size_t)i * out_elems, ydev, c * out_elems * sizeof(float), hipMemcpyDeviceToHost, copy_stream));
      HIPCHECK(hipEventRecord(ev_copied[b], copy_stream));
      // the host arrays of this chunk (x, affines) were consumed by stream-ordered copies from pageable memory: complete on return
    } else {
      HIPCHECK(hipMemcpyAsync(y + (size_t)i * out_elems, ydev, c * out_elems * sizeof(float), hipMemcpyDeviceToHost, nullptr));
      HIPCHECK(hipStreamSynchronize(nullptr));
    }
  }
  if (pinned && !sink) { HIPCHECK(hipStreamSynchronize(copy_stream)); HIPCHECK(hipStreamSynchronize(nullptr)); drain.armed = false; }
  if (n_nonfinite) {
    unsigned long long v = 0;
    HIPCHECK(hipMemcpy(&v, d_nonfinite.get(), sizeof(v), hipMemcpyDeviceToHost));
    *n_nonfinite = (int64_t)v;
  }
  return SRCFD_OK;
}

static int finish_create(std::unique_ptr<Model>& m, srcfd_model** out) {
  try {
    m->desc.infer_shapes();
    build_plan(m->desc, m->ops, m->pack);
    plan_convt_pair(*m);
    plan_convt_triple(*m);
    plan_tail32(*m);
    plan_enc32(*m);
    plan_x3(*m);
  } catch (const std::exception& e) {
    set_error(e.what());
    return SRCFD_EINVAL;
  }
  m->has_fused = m->desc.is_sr_10_400();
  lowp16_plan(*m);   // host only: which graphs run in bf16 / f16 (srcfd_model_supports_precision)
  int rc = m->init_device();
  if (rc) return rc;
  if (m->device >= 0 && m->lowp16) {
    rc = lowp16_init(*m);
    if (rc) return rc;
  }
  *out = reinterpret_cast<srcfd_model*>(m.release());
  return SRCFD_OK;
}

}  // namespace srcfd

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using srcfd::Model;
using srcfd::set_error;
static Model* M(srcfd_model* m) { return reinterpret_cast<Model*>(m); }
static const Model* M(const srcfd_model* m) { return reinterpret_cast<const Model*>(m); }

extern "C" {

const char* srcfd_last_error(void) { return srcfd::g_last_error.c_str(); }
const char* srcfd_version(void) { return "srcfd 0.1 (gfx950)"; }

int srcfd_device_count(void) {
  return srcfd::abi_guard("srcfd_device_count", [&]() -> int {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
  });
}

int srcfd_host_alloc(size_t bytes, void** out) {
  return srcfd::abi_guard("srcfd_host_alloc", [&]() -> int {
    if (!out || bytes == 0) { set_error("srcfd_host_alloc: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { (void)hipGetLastError(); set_error("no HIP device: page-locked memory needs the runtime"); return SRCFD_ENODEV; }
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; set_error(std::string("hipHostMalloc failed: ") + hipGetErrorString(e)); return SRCFD_ENOMEM; }
    return SRCFD_OK;
  });
}

void srcfd_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int srcfd_model_load_h5(const char* encoder_h5, const char* decoder_h5, int device, srcfd_model** out) {
  return srcfd::abi_guard("srcfd_model_load_h5", [&]() -> int {
    if (!out || (!encoder_h5 && !decoder_h5)) { set_error("srcfd_model_load_h5: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    std::unique_ptr<Model> m(new Model());
    m->device = device;
    try {
      if (encoder_h5) srcfd::append_h5_submodel(m->desc, encoder_h5);
      if (decoder_h5) srcfd::append_h5_submodel(m->desc, decoder_h5);
    } catch (const srcfd::FileError& e) {
      set_error(e.msg);
      return e.code;
    } catch (const std::exception& e) {
      set_error(e.what());
      return SRCFD_EIO;
    }
    return srcfd::finish_create(m, out);
  });
}

int srcfd_model_load_superres_h5(const char* superres_h5, int device, srcfd_model** out) {
  return srcfd::abi_guard("srcfd_model_load_superres_h5", [&]() -> int {
    if (!out || !superres_h5) { set_error("srcfd_model_load_superres_h5: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    std::unique_ptr<Model> m(new Model());
    m->device = device;
    try {
      srcfd::append_h5_whole(m->desc, superres_h5);
    } catch (const srcfd::FileError& e) {
      set_error(e.msg);
      return e.code;
    } catch (const std::exception& e) {
      set_error(e.what());
      return SRCFD_EIO;
    }
    return srcfd::finish_create(m, out);
  });
}

int srcfd_model_save_superres_h5(const srcfd_model* m, const char* superres_h5) {
  return srcfd::abi_guard("srcfd_model_save_superres_h5", [&]() -> int {
    if (!m || !superres_h5) { set_error("srcfd_model_save_superres_h5: bad arguments"); return SRCFD_EINVAL; }
    try {
      srcfd::save_h5_whole(M(m)->desc, superres_h5);
    } catch (const srcfd::FileError& e) {
      set_error(e.msg);
      return e.code;
    }
    return SRCFD_OK;
  });
}

int srcfd_model_create(const srcfd_layer* layers, int n_layers, const int in_shape[3], int device, srcfd_model** out) {
  return srcfd::abi_guard("srcfd_model_create", [&]() -> int {
    if (!out || !layers || n_layers <= 0 || !in_shape) { set_error("srcfd_model_create: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    std::unique_ptr<Model> m(new Model());
    m->device = device;
    for (int i = 0; i < 3; ++i) m->desc.in_shape[i] = in_shape[i];
    int cur[3] = {in_shape[0], in_shape[1], in_shape[2]};
    (void)cur;
    for (int i = 0; i < n_layers; ++i) {
      const srcfd_layer& s = layers[i];
      srcfd::Layer L;
      L.kind = s.kind; L.act = s.activation; L.kh = s.kh; L.kw = s.kw; L.stride = s.stride > 0 ? s.stride : 1; L.same = s.same_padding;
      L.cin = s.cin; L.cout = s.cout;
      for (int k = 0; k < 3; ++k) L.reshape[k] = s.reshape[k];
      L.name = (s.name && *s.name) ? std::string(s.name) : "layer_" + std::to_string(i);
      if (s.kind == SRCFD_LAYER_CONV2D || s.kind == SRCFD_LAYER_CONV2D_TRANSPOSE || s.kind == SRCFD_LAYER_DENSE) {
        if (!s.kernel || s.cin <= 0 || s.cout <= 0) { set_error("layer " + std::to_string(i) + ": missing kernel / channels"); return SRCFD_EINVAL; }
        if (s.kind == SRCFD_LAYER_DENSE) { L.kh = L.kw = 1; }
        if (L.kh <= 0 || L.kw <= 0) { set_error("layer " + std::to_string(i) + ": bad kernel size"); return SRCFD_EINVAL; }
        size_t cnt = (size_t)L.kh * L.kw * s.cin * s.cout;
        L.kernel.assign(s.kernel, s.kernel + cnt);
        if (s.bias) L.bias.assign(s.bias, s.bias + s.cout);
        else L.bias.assign(s.cout, 0.f);
      }
      m->desc.layers.push_back(std::move(L));
    }
    // A graph with a `latent_vector` layer in the middle is the encoder/decoder pair of SuperResolutionAE
    // (sr-ae-conv.ipynb:c162-169, c277-287): keep the two halves as separate sub-models so that save_h5 writes the
    // `vanilla_encoder...h5` / `vanilla_decoder...h5` pair the solvers load (PyCFD_ML_accelerated.py:831-832).
    int cut = -1;
    for (int i = 0; i + 1 < n_layers; ++i)
      if (m->desc.layers[i].name == "latent_vector") cut = i + 1;
    if (cut > 0) {
      try { m->desc.infer_shapes(); } catch (const std::exception& e) { set_error(e.what()); return SRCFD_EINVAL; }
      srcfd::SubModel enc, dec;
      enc.name = "encoder_" + std::to_string(in_shape[0]); enc.input_name = enc.name + "_input"; enc.first = 0; enc.count = cut;
      dec.name = "decoder_" + std::to_string(m->desc.out_shape()[0]); dec.input_name = dec.name + "_input"; dec.first = cut; dec.count = n_layers - cut;
      m->desc.subs.push_back(enc);
      m->desc.subs.push_back(dec);
    } else {
      srcfd::SubModel sub;
      sub.name = "model"; sub.input_name = "model_input"; sub.first = 0; sub.count = n_layers;
      m->desc.subs.push_back(sub);
    }
    return srcfd::finish_create(m, out);
  });
}

void srcfd_model_destroy(srcfd_model* m) { delete M(m); }

int srcfd_model_input_shape(const srcfd_model* m, int shape[3]) {
  return srcfd::abi_guard("srcfd_model_input_shape", [&]() -> int {
    if (!m || !shape) { set_error("bad arguments"); return SRCFD_EINVAL; }
    for (int i = 0; i < 3; ++i) shape[i] = M(m)->desc.in_shape[i];
    return SRCFD_OK;
  });
}
int srcfd_model_output_shape(const srcfd_model* m, int shape[3]) {
  return srcfd::abi_guard("srcfd_model_output_shape", [&]() -> int {
    if (!m || !shape) { set_error("bad arguments"); return SRCFD_EINVAL; }
    for (int i = 0; i < 3; ++i) shape[i] = M(m)->desc.out_shape()[i];
    return SRCFD_OK;
  });
}
int srcfd_model_num_layers(const srcfd_model* m) { return m ? (int)M(m)->desc.layers.size() : SRCFD_EINVAL; }

int srcfd_model_get_layer(const srcfd_model* m, int i, srcfd_layer* layer, char* name, size_t name_len) {
  return srcfd::abi_guard("srcfd_model_get_layer", [&]() -> int {
    if (!m || !layer || i < 0 || i >= (int)M(m)->desc.layers.size()) { set_error("bad arguments"); return SRCFD_EINVAL; }
    const srcfd::Layer& L = M(m)->desc.layers[i];
    layer->kind = L.kind; layer->activation = L.act; layer->kh = L.kh; layer->kw = L.kw; layer->stride = L.stride;
    layer->same_padding = L.same; layer->cin = L.cin; layer->cout = L.cout;
    for (int k = 0; k < 3; ++k) layer->reshape[k] = L.reshape[k];
    layer->kernel = L.kernel.empty() ? nullptr : L.kernel.data();
    layer->bias = L.bias.empty() ? nullptr : L.bias.data();
    layer->name = L.name.c_str();
    if (name && name_len) { std::snprintf(name, name_len, "%s", L.name.c_str()); }
    return SRCFD_OK;
  });
}

int64_t srcfd_model_macs_per_sample(const srcfd_model* m) { return m ? M(m)->desc.macs_per_sample() : 0; }

int srcfd_model_set_precision(srcfd_model* m, int precision) {
  return srcfd::abi_guard("srcfd_model_set_precision", [&]() -> int {
    if (!m || precision < 0 || precision > SRCFD_PREC_FP32X3) { set_error("bad precision"); return SRCFD_EINVAL; }
    if ((precision == SRCFD_PREC_BF16 || precision == SRCFD_PREC_F16) && !M(m)->lowp_ok()) {
      set_error(srcfd::LOWP_REFUSAL);
      return SRCFD_EINVAL;
    }
    M(m)->precision = precision;
    M(m)->drop_graph();
    return SRCFD_OK;
  });
}
int srcfd_model_reserve(srcfd_model* m, int n) {
  return srcfd::abi_guard("srcfd_model_reserve", [&]() -> int {
    if (!m || n < 0) { set_error("bad arguments"); return SRCFD_EINVAL; }
    srcfd::Model& mm = *M(m);
    if (mm.device < 0) { set_error("host-only handle: no device was requested at create"); return SRCFD_ENODEV; }
    if (n == 0) return SRCFD_OK;
    HIPCHECK(hipSetDevice(mm.device));
    if (mm.precision == SRCFD_PREC_BF16 || mm.precision == SRCFD_PREC_F16) {
      if (!mm.lowp_ok()) { set_error(srcfd::LOWP_REFUSAL); return SRCFD_EINVAL; }
      return srcfd::lowp16_reserve(mm, n);
    }
    return mm.ensure_workspace(n, srcfd::Switches::from_env(), mm.x3_for(n, mm.precision));
  });
}

int srcfd_model_get_precision(const srcfd_model* m) { return m ? M(m)->precision : SRCFD_EINVAL; }
int srcfd_model_has_fused_path(const srcfd_model* m) { return m ? (int)M(m)->has_fused : 0; }
int srcfd_model_supports_precision(const srcfd_model* m, int precision) { return (!m || precision < 0 || precision > SRCFD_PREC_FP32X3) ? 0 : (precision == SRCFD_PREC_BF16 || precision == SRCFD_PREC_F16) ? (int)M(m)->lowp_ok() : 1; }

int srcfd_predict(srcfd_model* m, const float* x, int n, const float* in_affine, const float* out_affine, float* y, int flags,
                  int64_t* n_nonfinite) {
  return srcfd::abi_guard("srcfd_predict", [&]() -> int {
    if (!m) { set_error("null model"); return SRCFD_EINVAL; }
    return M(m)->predict_host(x, n, in_affine, out_affine, y, flags, n_nonfinite);
  });
}

int srcfd_predict_device(srcfd_model* m, const void* x_dev, int n, const float* in_affine_dev, const float* out_affine_dev,
                         void* y_dev, int out_dtype, int flags, int64_t* nonfinite_dev, void* hip_stream) {
  return srcfd::abi_guard("srcfd_predict_device", [&]() -> int {
    if (!m || (n > 0 && (!x_dev || !y_dev))) { set_error("bad arguments"); return SRCFD_EINVAL; }
    return M(m)->predict_device(x_dev, n, in_affine_dev, out_affine_dev, y_dev, out_dtype, flags,
                                reinterpret_cast<unsigned long long*>(nonfinite_dev), reinterpret_cast<hipStream_t>(hip_stream));
  });
}

int srcfd_model_workspace(srcfd_model* m, int n, size_t* bytes) {
  return srcfd::abi_guard("srcfd_model_workspace", [&]() -> int {
    if (!m) { set_error("null model"); return SRCFD_EINVAL; }
    const Model& mm = *M(m);
    // the 16-bit path's chunks of up to 1024 samples (lowp16_chunk_cap); the fused graph answers with the f32 figures below, as it always has
    if ((mm.precision == SRCFD_PREC_BF16 || mm.precision == SRCFD_PREC_F16) && !mm.has_fused && mm.lowp16) {
      const int chunk16 = std::min(std::max(n, 1), srcfd::lowp16_chunk_cap(mm));
      if (bytes) *bytes = srcfd::lowp16_workspace_bytes(mm, chunk16);
      return chunk16;
    }
    const srcfd::Switches sw = srcfd::Switches::from_env();
    int chunk = std::min(std::max(n, 1), mm.chunk_cap(mm.precision, sw));
    if (bytes) *bytes = 2 * (size_t)chunk * mm.max_act_elems(mm.precision, sw) * sizeof(float);
    return chunk;
  });
}

int srcfd_model_footprint(const srcfd_model* m, int n, int precision, size_t bytes[4]) {
  return srcfd::abi_guard("srcfd_model_footprint", [&]() -> int {
    if (!m || !bytes || n < 0 || precision < 0 || precision > SRCFD_PREC_FP32X3) { set_error("bad arguments"); return SRCFD_EINVAL; }
    const srcfd::Model& mm = *M(m);
    const bool lowp = precision == SRCFD_PREC_BF16 || precision == SRCFD_PREC_F16;
    if (lowp && !mm.lowp_ok()) { set_error(srcfd::LOWP_REFUSAL); return SRCFD_EINVAL; }
    int shp_in[3] = {0, 0, 0}, shp_out[3] = {0, 0, 0};
    (void)srcfd_model_input_shape(m, shp_in);
    (void)srcfd_model_output_shape(m, shp_out);
    const size_t in_elems = (size_t)shp_in[0] * shp_in[1] * shp_in[2], out_elems = (size_t)shp_out[0] * shp_out[1] * shp_out[2];
    size_t params = 0;
    for (const auto& L : mm.desc.layers) params += L.kernel.size() + L.bias.size();
    if (lowp) {
      bytes[0] = srcfd::lowp16_workspace_bytes(mm, n);   // lowp16_reserve: two activation buffers + the dense split-K slabs
      bytes[1] = params * (sizeof(float) + 2 * sizeof(uint16_t));   // f32 weights + the 16-bit GEMM layout + fragment re-orderings (upper bound: every layer twice)
    } else {
      const srcfd::Switches sw = srcfd::Switches::from_env();
      const int chunk = n ? std::min(n, mm.chunk_cap(precision, sw)) : 0;
      bytes[0] = 2 * (size_t)chunk * mm.max_act_elems(precision, sw) * sizeof(float);
      bytes[1] = params * sizeof(float) * 2 + mm.pack_x3.size() * sizeof(uint16_t);   // packed weights + the per-layer operand orders of the fused f32 kernels (upper bound) + the split-bf16 planes
    }
    const size_t stage = (size_t)std::min(n, Model::STAGE_SAMPLES);
    bytes[2] = stage * (in_elems + 2 * out_elems + 4) * sizeof(float);   // predict_host: input, two result buffers, affine pairs
    bytes[3] = (size_t)n * out_elems * sizeof(float);                    // what ONE host result of the call takes (pool buffer or caller's array)
    return SRCFD_OK;
  });
}

int srcfd_model_set_profiling(srcfd_model* m, int enable) {
  return srcfd::abi_guard("srcfd_model_set_profiling", [&]() -> int {
    if (!m) { set_error("null model"); return SRCFD_EINVAL; }
    M(m)->profiling = enable != 0;
    M(m)->prof_used = 0;
    return SRCFD_OK;
  });
}

int srcfd_model_get_profile(srcfd_model* m, char* names, size_t names_len, float* ms, int* count, int max_count) {
  return srcfd::abi_guard("srcfd_model_get_profile", [&]() -> int {
    if (!m || !count) { set_error("bad arguments"); return SRCFD_EINVAL; }
    Model* mm = M(m);
    if (mm->device < 0) { set_error("host-only handle"); return SRCFD_ENODEV; }
    HIPCHECK(hipSetDevice(mm->device));
    HIPCHECK(hipDeviceSynchronize());
    std::string joined;
    int n = 0;
    for (size_t i = 0; i < mm->prof_used && n < max_count; ++i, ++n) {
      float t = 0.f;
      HIPCHECK(hipEventElapsedTime(&t, mm->prof_events[i].a, mm->prof_events[i].b));
      if (ms) ms[n] = t;
      if (n) joined += '\n';
      joined += mm->prof_events[i].name;
    }
    *count = n;
    if (names && names_len) std::snprintf(names, names_len, "%s", joined.c_str());
    return SRCFD_OK;
  });
}

int srcfd_model_last_plan(const srcfd_model* m, char* buf, size_t buf_len) {
  return srcfd::abi_guard("srcfd_model_last_plan", [&]() -> int {
    if (!m || !buf || buf_len == 0) { set_error("bad arguments"); return SRCFD_EINVAL; }
    const srcfd::Plan& p = M(m)->plan;
    const char* prec = p.precision == SRCFD_PREC_BF16 ? "bf16" : p.precision == SRCFD_PREC_F16 ? "f16" : p.precision == SRCFD_PREC_FP32 ? "fp32" : p.precision == SRCFD_PREC_FP32X3 ? "fp32x3" : "fp32_naive";
    char tmp[256];
    if (p.any16)
      snprintf(tmp, sizeof(tmp), "precision=%s encoder=%s decoder=any16 graph=%s", prec, p.sw.enc16 ? "enc16" : "layers",
               p.graph == 2 ? "replay" : p.graph == 1 ? "capture" : "eager");
    else if (p.fused)
      snprintf(tmp, sizeof(tmp), "precision=%s encoder=%s dense_1=%s middle=%s tail=%s tail_seg=%d graph=%s", prec, p.sw.enc16 ? "enc16" : "layers",
               p.sw.dense1_16 ? "dense1_16" : "gemm16", p.sw.mid16 ? (p.sw.mid_waves == 4 ? "mid16_4x32" : p.sw.mid_waves == 16 ? "mid16_16x32" : p.sw.mid_shape == 1 ? "mid16_8x32" : p.sw.mid_shape == 2 ? "mid16_8x64" : "mid16_4x64") : "gemm16", p.sw.tail16s ? "tail16s" : "tail16", p.tail_seg,
               p.graph == 2 ? "replay" : p.graph == 1 ? "capture" : "eager");
    else
      snprintf(tmp, sizeof(tmp), "precision=%s encoder=%s dense_1=%s graph=%s", prec, p.sw.enc32 ? "enc32" : "layers",
               p.sw.skinny32 ? "dense_skinny32" : "gemm32", p.graph == 2 ? "replay" : p.graph == 1 ? "capture" : "eager");
    snprintf(buf, buf_len, "%s", tmp);
    return SRCFD_OK;
  });
}

int srcfd_model_f32_steps(const srcfd_model* m, int n, char* buf, size_t buf_len) {
  return srcfd::abi_guard("srcfd_model_f32_steps", [&]() -> int {
    if (!m || !buf || buf_len == 0 || n < 1) { set_error("bad arguments"); return SRCFD_EINVAL; }
    const Model& mm = *M(m);
    if (mm.precision == SRCFD_PREC_BF16 || mm.precision == SRCFD_PREC_F16) { set_error("the 16-bit precisions have no f32 steps"); return SRCFD_EINVAL; }
    static const char* const kernel[] = {"tail32", "triple", "pair", "x3", "big", "group", "skinny", "finalize", "mfma", "naive"};   // F32Kernel's order
    const srcfd::Switches sw = srcfd::Switches::from_env();
    std::string out;
    const size_t first = mm.f32_first(mm.precision, sw);
    if (first) out = mm.ops[0].name + "=enc32:" + std::to_string(first);
    srcfd::F32Step st;
    for (size_t i = first; i < mm.ops.size(); i += st.count) {
      st = mm.f32_step(i, n, mm.precision, sw, mm.x3_for(n, mm.precision));   // one call of n samples
      out += (out.empty() ? "" : " ") + mm.ops[i].name + "=" + kernel[(int)st.k] + ":" + std::to_string(st.count);
    }
    if (out.size() >= buf_len) { set_error("buffer too small"); return SRCFD_EINVAL; }
    snprintf(buf, buf_len, "%s", out.c_str());
    return SRCFD_OK;
  });
}

int srcfd_model_debug_activation(srcfd_model* m, int index, void* dst, size_t bytes) {
  return srcfd::abi_guard("srcfd_model_debug_activation", [&]() -> int {
    if (!m || !dst || index < 0 || index > 1) { set_error("bad arguments"); return SRCFD_EINVAL; }
    return srcfd::fused_debug_read(*M(m), index, dst, bytes);
  });
}

int srcfd_model_save_h5(const srcfd_model* m, const char* encoder_h5, const char* decoder_h5) {
  return srcfd::abi_guard("srcfd_model_save_h5", [&]() -> int {
    if (!m) { set_error("null model"); return SRCFD_EINVAL; }
    const Model* mm = M(m);
    try {
      const char* paths[2] = {encoder_h5, decoder_h5};
      int given = (encoder_h5 ? 1 : 0) + (decoder_h5 ? 1 : 0);
      if (given == 0) { set_error("no output path"); return SRCFD_EINVAL; }
      if ((int)mm->desc.subs.size() == 1) {
        srcfd::save_h5_submodel(mm->desc, 0, encoder_h5 ? encoder_h5 : decoder_h5);
      } else {
        for (int i = 0; i < 2 && i < (int)mm->desc.subs.size(); ++i)
          if (paths[i]) srcfd::save_h5_submodel(mm->desc, i, paths[i]);
      }
    } catch (const srcfd::FileError& e) {
      set_error(e.msg);
      return e.code;
    }
    return SRCFD_OK;
  });
}

}  // extern "C"
