// Host-side operand packing (operand_pack.h).  Plain C++: no HIP runtime calls.
#include "operand_pack.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "kernels16.h"

namespace srcfd {

uint16_t to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                           // round to nearest even
  return (uint16_t)(u >> 16);
}
uint16_t to_f16(float f) {   // IEEE binary16, round to nearest even (what a cast to _Float16 gives; not every host compiler has the type)
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((u >> 13) & 0x1ffu));   // NaN stays NaN
  if (u >= 0x38800000u) {                                                         // normal: re-bias, round; carries run into the exponent
    u -= 112u << 23;
    u += 0xfffu + ((u >> 13) & 1u);
    return (uint16_t)(sign | std::min(u >> 13, 0x7c00u));
  }
  const int shift = 126 - (int)(u >> 23);                                         // subnormal: 2^-24 units
  if (shift > 24) return (uint16_t)sign;
  const uint32_t mant = (u & 0x7fffffu) | 0x800000u, rem = mant & ((1u << shift) - 1), half = 1u << (shift - 1);
  uint32_t h = mant >> shift;
  if (rem > half || (rem == half && (h & 1u))) ++h;
  return (uint16_t)(sign | h);
}

void split3(float w, uint16_t (&o)[3]) {
  uint32_t b0, b1, b2;
  std::memcpy(&b0, &w, 4); b0 &= 0xffff0000u;
  float hi; std::memcpy(&hi, &b0, 4);
  const float r1 = w - hi;
  std::memcpy(&b1, &r1, 4); b1 &= 0xffff0000u;
  float mid; std::memcpy(&mid, &b1, 4);
  const float r2 = r1 - mid;
  std::memcpy(&b2, &r2, 4);
  o[0] = (uint16_t)(b0 >> 16); o[1] = (uint16_t)(b1 >> 16); o[2] = (uint16_t)(b2 >> 16);
}

void split_planes(const float* B, int K, int N, int Npad, int Kpad, uint16_t* out) {
  const size_t plane = (size_t)N * Kpad;
  std::memset(out, 0, 3 * plane * sizeof(uint16_t));
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      uint16_t o[3];
      split3(B[(size_t)k * Npad + n], o);
      for (int pl = 0; pl < 3; ++pl) out[pl * plane + (size_t)n * Kpad + k] = o[pl];
    }
}

// f32 engine: B[K][Npad] + bias per GEMM op
static size_t put_B(std::vector<float>& pack, const GemmDesc& d, const std::vector<float>& Bmat /*[K][N]*/) {   // -> B[K][Npad]
  const size_t off = pack.size();
  pack.resize(off + (size_t)std::max(d.K, 1) * d.Npad, 0.f);
  for (int k = 0; k < d.K; ++k) std::memcpy(&pack[off + (size_t)k * d.Npad], &Bmat[(size_t)k * d.N], sizeof(float) * d.N);
  return off;
}
static void pack_B(std::vector<float>& pack, Op& op, const std::vector<float>& Bmat /*[K][N]*/, const std::vector<float>& bias_n) {
  const GemmDesc& d = op.d;
  align64(pack);  // 256-byte aligned sub-buffers
  op.w_off = put_B(pack, d, Bmat);
  align64(pack);
  op.b_off = pack.size();
  pack.resize(pack.size() + d.Npad, 0.f);
  std::memcpy(&pack[op.b_off], bias_n.data(), sizeof(float) * d.N);
}

void build_plan(const ModelDesc& desc, std::vector<Op>& ops, std::vector<float>& pack) {
  ops.clear();
  pack.clear();
  for (size_t li = 0; li < desc.layers.size(); ++li) {
    const Layer& L = desc.layers[li];
    if (L.kind == SRCFD_LAYER_FLATTEN || L.kind == SRCFD_LAYER_RESHAPE) continue;  // views of NHWC buffers
    const int IH = L.in_shape[0], IW = L.in_shape[1], OH = L.out_shape[0], OW = L.out_shape[1];
    GemmDesc d{};
    d.act = L.act;
    d.OH = OH; d.OW = OW; d.OC = L.cout; d.CO = L.cout;
    d.nphx = 1; d.os = 1;
    d.IH = IH; d.IW = IW; d.CI = L.cin;
    auto emit = [&](const GemmDesc& g, const std::string& name, const std::vector<float>& B, const std::vector<float>& bias) {
      Op op; op.d = g; op.layer = (int)li; op.name = name;
      pack_B(pack, op, B, bias);
      ops.push_back(op);
    };
    if (L.kind == SRCFD_LAYER_DENSE) {
      d.IH = d.IW = 1; d.CI = L.cin; d.OH = d.OW = 1;
      d.MH = d.MW = 1; d.TY = d.TX = 1;
      d.K = L.cin; d.N = L.cout; d.Npad = round_up(d.N, 32);
      emit(d, L.name, L.kernel, L.bias);
    } else if (L.kind == SRCFD_LAYER_CONV2D) {
      int pt = 0, pl = 0;
      if (L.same) {
        int th = std::max((OH - 1) * L.stride + L.kh - IH, 0), tw = std::max((OW - 1) * L.stride + L.kw - IW, 0);
        pt = th / 2; pl = tw / 2;  // TF SAME: the extra pixel goes after
      }
      d.MH = OH; d.MW = OW; d.TY = L.kh; d.TX = L.kw;
      d.ay = d.ax = L.stride; d.by = d.bx = 1; d.cy = -pt; d.cx = -pl;
      d.K = L.kh * L.kw * L.cin; d.N = L.cout; d.Npad = round_up(d.N, 32);
      emit(d, L.name, L.kernel, L.bias);  // (kh,kw,Cin,Cout) is already [K][N]
    } else {  // Conv2DTranspose, kernel (kh,kw,Cout,Cin).  VALID: full[s i + a] += x[i] W[a]; SAME: out[o] = full[o + pb], pb = (k - s) / 2
      const int s = L.stride;
      const int pby = L.same ? (L.kh - s) / 2 : 0, pbx = L.same ? (L.kw - s) / 2 : 0;
      auto W = [&](int a, int b, int co, int ci) { return L.kernel[(((size_t)a * L.kw + b) * L.cout + co) * L.cin + ci]; };
      if (L.kh == s && L.kw == s) {
        d.MH = IH; d.MW = IW; d.TY = d.TX = 1;
        d.ay = d.ax = 1; d.by = d.bx = 0; d.cy = d.cx = 0;
        d.K = L.cin; d.N = s * s * L.cout; d.Npad = round_up(d.N, 32);
        d.nphx = s; d.os = s;
        std::vector<float> B((size_t)d.K * d.N), bn(d.N);
        for (int ci = 0; ci < L.cin; ++ci)
          for (int py = 0; py < s; ++py)
            for (int px = 0; px < s; ++px)
              for (int co = 0; co < L.cout; ++co) B[(size_t)ci * d.N + (py * s + px) * L.cout + co] = W(py, px, co, ci);
        for (int n = 0; n < d.N; ++n) bn[n] = L.bias[n % L.cout];
        emit(d, L.name, B, bn);
      } else {
        for (int py = 0; py < s; ++py)
          for (int px = 0; px < s; ++px) {
            GemmDesc p = d;
            p.TY = py < L.kh ? (L.kh - py + s - 1) / s : 0;
            p.TX = px < L.kw ? (L.kw - px + s - 1) / s : 0;
            // phase (py, px) of the VALID result: its position s m' + py is output row s my + ry, m' = my + shy (pb = 0: ry = py, shy = 0)
            const int ry = ((py - pby) % s + s) % s, rx = ((px - pbx) % s + s) % s;
            const int shy = (ry + pby - py) / s, shx = (rx + pbx - px) / s;
            p.MH = ry < OH ? (OH - ry + s - 1) / s : 0;
            p.MW = rx < OW ? (OW - rx + s - 1) / s : 0;
            if (p.MH == 0 || p.MW == 0) continue;
            p.ay = p.ax = 1; p.by = p.bx = -1; p.cy = shy; p.cx = shx;
            p.K = p.TY * p.TX * L.cin; p.N = L.cout; p.Npad = round_up(p.N, 32);
            p.os = s; p.oy0 = ry; p.ox0 = rx;
            std::vector<float> B((size_t)std::max(p.K, 1) * p.N, 0.f);
            for (int ty = 0; ty < p.TY; ++ty)
              for (int tx = 0; tx < p.TX; ++tx)
                for (int ci = 0; ci < L.cin; ++ci)
                  for (int co = 0; co < L.cout; ++co)
                    B[((size_t)(ty * p.TX + tx) * L.cin + ci) * p.N + co] = W(py + s * ty, px + s * tx, co, ci);
            emit(p, L.name + ".ph" + std::to_string(py) + std::to_string(px), B, L.bias);
          }
      }
    }
  }
}

// fused f32 ConvT chains (kernels_fp32.hip).  Conv2DTranspose kernels are (kh, kw, Cout, Cin).
static size_t put_section(std::vector<float>& pk, const std::vector<float>& v) {
  align64(pk);
  const size_t off = pk.size();
  pk.insert(pk.end(), v.begin(), v.end());
  return off;
}
// A operands of v_mfma_f32_32x32x2f32 from a ConvT kernel read as [row = (tap, co)][ci], tiles of 32 rows, KS = ci / 2 k-steps:
//   v[(T*KS + s)*64 + lane] = K[32 T + lane % 32][k],  k = KS (lane / 32) + s             (K_HALVES: the input comes from memory)
//                                                   k = (s & 3) + 8 (s >> 2) + 4 (lane / 32) (K_ACC: the input is the previous layer's accumulators)
// pair: wa = K_HALVES, wb = K_ACC; triple: w1 = K_HALVES, w2 = w3 = K_ACC.  The 32 -> 16 layer is packed both ways: wa != w2.
enum KOrder { K_HALVES, K_ACC };
static std::vector<float> frag32(const Layer& L, KOrder order) {
  const int KS = L.cin / 2, tiles = 4 * L.cout / 32;
  std::vector<float> v((size_t)tiles * KS * 64);
  for (int T = 0; T < tiles; ++T)
    for (int s = 0; s < KS; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5, k = order == K_ACC ? (s & 3) + 8 * (s >> 2) + 4 * h : KS * h + s;
        v[(size_t)(T * KS + s) * 64 + lane] = L.kernel[((size_t)32 * T + (lane & 31)) * L.cin + k];
      }
  return v;
}

PairPack pack_convt_pair(std::vector<float>& pk, const Layer& La, const Layer& Lb) {
  PairPack p;
  p.wa = put_section(pk, frag32(La, K_HALVES)); p.ba = put_section(pk, La.bias);
  p.wb = put_section(pk, frag32(Lb, K_ACC)); p.bb = put_section(pk, Lb.bias);
  align64(pk);
  return p;
}

TriplePack pack_convt_triple(std::vector<float>& pk, const Layer& L1, const Layer& L2, const Layer& L3) {
  TriplePack p;
  p.w1 = put_section(pk, frag32(L1, K_HALVES)); p.b1 = put_section(pk, L1.bias);
  p.w2 = put_section(pk, frag32(L2, K_ACC)); p.b2 = put_section(pk, L2.bias);
  p.w3 = put_section(pk, frag32(L3, K_ACC)); p.b3 = put_section(pk, L3.bias);
  align64(pk);
  return p;
}

// the streaming f32 tail (kernels_tail32.hip) and its backward pass (train_tail.hip), as slots.  The ConvT 64 -> 32 -> 16 -> 8
// chain + the 3x3 SAME conv 8 -> 1; parameters in flat order (train_tail.h, TT_O_*): ConvT kernels (tap, co, ci), the Conv2D
// kernel (3, 3, 8, 1) = (ty, tx, ci).  v_mfma_f32_16x16x4_f32 fragments, lane = (m = lane & 15, kg = lane >> 4).
static int W1(int tap, int co, int ci) { return TT_O_W1 + (tap * 32 + co) * 64 + ci; }
static int W2(int tap, int co, int ci) { return TT_O_W2 + (tap * 16 + co) * 32 + ci; }
static int W3(int tap, int co, int ci) { return TT_O_W3 + (tap * 8 + co) * 16 + ci; }
static void pad_slots(std::vector<Slot>& s) { while (s.size() % 64) s.push_back({-1, SC_ONE}); }
static void run_slots(std::vector<Slot>& s, int first, int count, Scale sc) { for (int i = 0; i < count; ++i) s.push_back({first + i, sc}); }
// w1[((tap1*2 + t)*16 + s)*64 + lane] = W1[tap1][co 16t + m][ci 16kg + s]
static void frag_t32_w1(std::vector<Slot>& s, Scale sc) {
  for (int tap = 0; tap < 4; ++tap)
    for (int t = 0; t < 2; ++t)
      for (int k = 0; k < 16; ++k)
        for (int lane = 0; lane < 64; ++lane) s.push_back({W1(tap, 16 * t + (lane & 15), 16 * (lane >> 4) + k), sc});
}
// w2[(tap2*8 + 4t + i)*64 + lane] = W2[tap2][co m][ci 16t + 4kg + i]      (k order = the first layer's accumulator order)
static void frag_t32_w2(std::vector<Slot>& s) {
  for (int tap = 0; tap < 4; ++tap)
    for (int t = 0; t < 2; ++t)
      for (int i = 0; i < 4; ++i)
        for (int lane = 0; lane < 64; ++lane) s.push_back({W2(tap, lane & 15, 16 * t + 4 * (lane >> 4) + i), SC_ONE});
}
// w3[(u*4 + i)*64 + lane] = W3[tap3 2u + (m >> 3)][co m & 7][ci 4kg + i]
static void frag_t32_w3(std::vector<Slot>& s) {
  for (int u = 0; u < 2; ++u)
    for (int i = 0; i < 4; ++i)
      for (int lane = 0; lane < 64; ++lane) s.push_back({W3(2 * u + ((lane & 15) >> 3), lane & 7, 4 * (lane >> 4) + i), SC_ONE});
}

Tail32Pack tail32_slots(std::vector<Slot>& s) {
  Tail32Pack p;
  pad_slots(s); p.w1 = s.size(); frag_t32_w1(s, SC_LOG2E);
  pad_slots(s); p.b1 = s.size(); run_slots(s, TT_O_B1, 32, SC_LOG2E);
  pad_slots(s); p.w2 = s.size(); frag_t32_w2(s);
  pad_slots(s); p.b2 = s.size(); run_slots(s, TT_O_B2, 16, SC_LOG2E);
  pad_slots(s); p.w3 = s.size(); frag_t32_w3(s);
  pad_slots(s); p.b3 = s.size(); run_slots(s, TT_O_B3, 8, SC_LOG2E);
  pad_slots(s); p.wc = s.size(); run_slots(s, TT_O_WC, 72, SC_INV_LOG2E); s.push_back({TT_O_BC, SC_ONE});
  pad_slots(s);
  return p;
}

// the four layers' parameters in flat order
static std::vector<float> tail_params(const Layer& L1, const Layer& L2, const Layer& L3, const Layer& LO) {
  std::vector<float> p;
  for (const Layer* L : {&L1, &L2, &L3, &LO}) { p.insert(p.end(), L->kernel.begin(), L->kernel.end()); p.insert(p.end(), L->bias.begin(), L->bias.end()); }
  if (p.size() != (size_t)TT_PARAMS) throw std::runtime_error("pack_tail32: parameter count");
  return p;
}

Tail32Pack pack_tail32(std::vector<float>& pk, const Layer& L1, const Layer& L2, const Layer& L3, const Layer& LO) {
  const std::vector<float> p = tail_params(L1, L2, L3, LO);
  align64(pk);
  const size_t base = pk.size();
  std::vector<Slot> s;
  Tail32Pack t = tail32_slots(s);
  for (const Slot& q : s)   // 1 / log2(e) is applied as a division
    pk.push_back(q.src < 0 ? 0.f : q.sc == SC_LOG2E ? (float)(p[q.src] * LOG2E) : q.sc == SC_INV_LOG2E ? (float)(p[q.src] / LOG2E) : p[q.src]);
  for (size_t* o : {&t.w1, &t.b1, &t.w2, &t.b2, &t.w3, &t.b3, &t.wc}) *o += base;
  return t;
}

void train_tail_slots(size_t param_off, TrainTailPlan& plan) {
  std::vector<Slot> s;
  const Tail32Pack t = tail32_slots(s);
  plan.t32_w1 = t.w1; plan.t32_b1 = t.b1; plan.t32_w2 = t.w2; plan.t32_b2 = t.b2; plan.t32_w3 = t.w3; plan.t32_b3 = t.b3; plan.t32_wc = t.wc;
  // ---- tail_bwd32: unscaled forward fragments, data-gradient fragments, biases ----
  plan.wf = s.size(); frag_t32_w1(s, SC_ONE); frag_t32_w2(s); frag_t32_w3(s);
  pad_slots(s); plan.wb = s.size();
  for (int tap = 0; tap < 4; ++tap)      // a1b[tap][t][c][i][lane] = W1[tap][co 16c + 4kg + i][ci 16t + m]
    for (int t4 = 0; t4 < 4; ++t4)
      for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 4; ++i)
          for (int lane = 0; lane < 64; ++lane) s.push_back({W1(tap, 16 * c + 4 * (lane >> 4) + i, 16 * t4 + (lane & 15)), SC_ONE});
  for (int tap = 0; tap < 4; ++tap)      // a2b[tap][t][i][lane] = W2[tap][co 4kg + i][ci 16t + m]
    for (int t2 = 0; t2 < 2; ++t2)
      for (int i = 0; i < 4; ++i)
        for (int lane = 0; lane < 64; ++lane) s.push_back({W2(tap, 4 * (lane >> 4) + i, 16 * t2 + (lane & 15)), SC_ONE});
  for (int u = 0; u < 2; ++u)            // a3b[u][i][lane] = W3[tap3 = 2u + (r >> 3)][co r & 7][ci m], r = 4kg + i
    for (int i = 0; i < 4; ++i)
      for (int lane = 0; lane < 64; ++lane) {
        const int r = 4 * (lane >> 4) + i;
        s.push_back({W3(2 * u + (r >> 3), r & 7, lane & 15), SC_ONE});
      }
  pad_slots(s); plan.wt = s.size();
  for (int s3 = 0; s3 < 3; ++s3)         // wt[s][lane] = Wc[2 - s][2 - (b' - tx3)][co] for 0 <= b' - tx3 <= 2, else 0; m = 8 tx3 + co, b' = kg
    for (int lane = 0; lane < 64; ++lane) {
      const int m = lane & 15, tx3 = m >> 3, co = m & 7, d = (lane >> 4) - tx3;
      s.push_back({d >= 0 && d <= 2 ? TT_O_WC + ((2 - s3) * 3 + (2 - d)) * 8 + co : -1, SC_ONE});
    }
  pad_slots(s); plan.bias = s.size();
  run_slots(s, TT_O_B1, 32, SC_ONE); run_slots(s, TT_O_B2, 16, SC_ONE); run_slots(s, TT_O_B3, 8, SC_ONE); run_slots(s, TT_O_WC, 73, SC_ONE);
  pad_slots(s);
  if (s.size() - plan.wf < (size_t)TT_WF || plan.wt - plan.wb != (size_t)TT_WB || plan.bias - plan.wt != (size_t)TT_WT) throw std::runtime_error("train_tail_plan: pack sizes");
  const double factor[3] = {1.0, LOG2E, 1.0 / LOG2E};
  for (const Slot& q : s) {   // maps hold flat index + 1 (0: padding)
    plan.map.push_back(q.src < 0 ? 0 : (int)(param_off + q.src + 1));
    plan.scale.push_back(q.src < 0 ? 0.f : (float)factor[q.sc]);
  }
}

// tail32<X3> (kernels_tail32.hip): lane = (m, kg), 8 elements j per lane
//   w2x[((tap*3 + plane)*64 + lane)*8 + j] = plane(W2[tap][co m][ci j < 4 ? 4 kg + j : 16 + 4 kg + j - 4])
//   w1x[((((ty1*2 + tx1)*2 + t)*2 + c)*3 + plane)*64 + lane][j] = plane(f32(W1[2 ty1 + tx1][co 16t + m][ci 32c + 8 kg + j] x log2(e)))
void pack_tail32_x3(std::vector<uint16_t>& px, const Layer& L1, const Layer& L2, int64_t& w1x, int64_t& w2x) {
  uint16_t o[3];
  align64(px);
  w2x = (int64_t)px.size();
  px.resize(px.size() + (size_t)4 * 3 * 64 * 8);
  for (int tap = 0; tap < 4; ++tap)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int mm = lane & 15, kg = lane >> 4, ci = j < 4 ? 4 * kg + j : 16 + 4 * kg + (j - 4);
        split3(L2.kernel[((size_t)tap * 16 + mm) * 32 + ci], o);
        for (int pl = 0; pl < 3; ++pl) px[w2x + ((size_t)(tap * 3 + pl) * 64 + lane) * 8 + j] = o[pl];
      }
  align64(px);
  w1x = (int64_t)px.size();
  px.resize(px.size() + (size_t)2 * 2 * 2 * 2 * 3 * 64 * 8);
  for (int tap = 0; tap < 4; ++tap)
    for (int t = 0; t < 2; ++t)
      for (int c = 0; c < 2; ++c)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int mm = lane & 15, kg = lane >> 4;
            split3((float)(L1.kernel[((size_t)tap * 32 + 16 * t + mm) * 64 + 32 * c + 8 * kg + j] * LOG2E), o);
            for (int pl = 0; pl < 3; ++pl) px[w1x + ((size_t)(((tap * 2 + t) * 2 + c) * 3 + pl) * 64 + lane) * 8 + j] = o[pl];
          }
}

// enc32 (kernels_enc32.hip): conv2d_1's weights as v_mfma_f32_16x16x4_f32 A fragments:
// frag[((w*36 + tap*4 + q)*64 + lane)*4 + j] = W[tap][ci = 16 q + 4 (lane / 16) + j][co = 16 w + lane % 16]   (Keras Conv2D kernel (kh, kw, cin, cout))
size_t pack_enc32(std::vector<float>& pk, const Layer& L1) {
  align64(pk);
  const size_t off = pk.size();
  pk.resize(pk.size() + (size_t)8 * 36 * 64 * 4);
  for (int w = 0; w < 8; ++w)
    for (int tap = 0; tap < 9; ++tap)
      for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int ci = 16 * q + 4 * (lane >> 4) + j, co = 16 * w + (lane & 15);
            pk[off + ((size_t)((w * 36 + tap * 4 + q) * 64 + lane)) * 4 + j] = L1.kernel[((size_t)tap * 64 + ci) * 128 + co];
          }
  align64(pk);
  return off;
}

// bf16 / f16 path: 16-bit weights, log2(e) folding, MFMA fragment order
static double scale_in(const ModelDesc& md, const std::vector<int>& cl, int i) { return (i > 0 && md.layers[cl[i - 1]].act == SRCFD_ACT_SWISH) ? 1.0 / LOG2E : 1.0; }
static double scale_out(const ModelDesc& md, const std::vector<int>& cl, int i) { return md.layers[cl[i]].act == SRCFD_ACT_SWISH ? LOG2E : 1.0; }
static double scale_w(const ModelDesc& md, const std::vector<int>& cl, int i) {
  double si = scale_in(md, cl, i), so = scale_out(md, cl, i);
  return (si != 1.0 && so != 1.0) ? 1.0 : si * so;  // swish -> swish: the factors cancel exactly
}
static std::vector<int> compute_layers(const ModelDesc& md) {
  std::vector<int> cl;
  for (size_t i = 0; i < md.layers.size(); ++i)
    if (md.layers[i].kind != SRCFD_LAYER_FLATTEN && md.layers[i].kind != SRCFD_LAYER_RESHAPE) cl.push_back((int)i);
  return cl;
}

// A operands of v_mfma 32x32x16 (R = 32) / 16x16x32 (R = 16), one 16-byte load per lane, from W(row, k):
//   out[((tile*KS + ks)*64 + l)*8 + j] = W(R tile + l % R, (512 / R) ks + 8 (l / R) + j)
template <class F> static void a_frags(uint16_t* out, int R, int tiles, int KS, F W) {
  for (int t = 0; t < tiles; ++t)
    for (int ks = 0; ks < KS; ++ks)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) *out++ = W(t * R + l % R, 512 / R * ks + 8 * (l / R) + j);
}
// k order of a 32x32 accumulator used as the next B operand: registers 4..7 hold rows 8..11, i.e. bits 2 and 3 of k swapped
static int acc_k(int k) { return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1); }
// bias as 32x32 accumulator init: out[(tile*2 + lane half)*16 + r] = b(32 tile + rowof(r, half))
template <class F> static void acc_bias(float* out, int tiles, F b) {
  for (int t = 0; t < tiles; ++t)
    for (int hh = 0; hh < 2; ++hh)
      for (int r = 0; r < 16; ++r) out[(t * 2 + hh) * 16 + r] = b(32 * t + rowof(r, hh));
}

void plan16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, int last, bool narrow_ok, Plan16& P) {
  P.cl = compute_layers(md);
  {  // conv1 (VALU kernel): f32 weights, scaled
    const Layer& L = md.layers[P.cl[0]];
    const double sw = scale_w(md, P.cl, 0), so = scale_out(md, P.cl, 0);
    P.c1w_off = P.f32.size();
    for (float v : L.kernel) P.f32.push_back((float)(v * sw));
    P.c1b_off = P.f32.size();
    for (float v : L.bias) P.f32.push_back((float)(v * so));
  }
  for (size_t i = 0; i < ops.size(); ++i) {
    const Op& op = ops[i];
    int ci = -1;
    for (size_t k = 0; k < P.cl.size(); ++k) if (P.cl[k] == op.layer) ci = (int)k;
    if (ci < 1 || ci > last) continue;
    Op16 o;
    o.d = op.d; o.name = op.name; o.layer = ci; o.src = (int)i;
    if (ci == 3) { o.d.N = 64; o.d.CO = 64; o.d.OC = 64; }   // latent -> 64 zero-padded channels
    if (ci == 4) { o.d.CI = 64; o.d.K = 64; }                // the dense layer behind it reads the padded latent
    const bool narrow = narrow_ok && any16_narrow(o.d);
    o.d.Npad = round_up(o.d.N, narrow ? 32 : 64);
    o.Kpad = narrow ? o.d.K : round_up(o.d.K, 64);
    const double so = scale_out(md, P.cl, ci);
    while (P.f32.size() % 4) P.f32.push_back(0.f);
    o.b_off = P.f32.size();
    for (int n = 0; n < o.d.Npad; ++n) P.f32.push_back(n < op.d.N ? (float)(pack[op.b_off + n] * so) : 0.f);
    P.ops.push_back(o);
  }
}

void pack_wt16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& P, bool f16, std::vector<uint16_t>& w) {
  for (Op16& o : P.ops) {
    const Op& op = ops[o.src];
    const double sw = scale_w(md, P.cl, o.layer);
    while (w.size() % 8) w.push_back(0);
    o.w_off = w.size();
    w.resize(w.size() + (size_t)o.d.Npad * o.Kpad, 0);
    for (int n = 0; n < op.d.N; ++n)
      for (int k = 0; k < op.d.K; ++k) w[o.w_off + (size_t)n * o.Kpad + k] = to16((float)(pack[op.w_off + (size_t)k * op.d.Npad + n] * sw), f16);
  }
}

// the same 16-bit values as Wt, re-ordered so that one lane's MFMA A operand is one 16-byte load
void pack_enc16(const Plan16& P, const std::vector<uint16_t>& w, Enc16Host& E) {
  const uint16_t* W2 = w.data() + P.ops[0].w_off;   // [128][576]
  const uint16_t* WD = w.data() + P.ops[1].w_off;   // [128][3200]
  const uint16_t* WL = w.data() + P.ops[2].w_off;   // [64][128]
  E.enc_wd_off = (size_t)4 * 36 * 1024; E.enc_wl_off = E.enc_wd_off + (size_t)8 * 100 * 1024;
  E.encf.resize((size_t)(4 * 36 + 8 * 100 + 4 * 4) * 512);
  a_frags(E.encf.data(), 32, 4, 36, [&](int r, int k) { return W2[(size_t)r * 576 + k]; });
  a_frags(E.encf.data() + E.enc_wd_off / 2, 16, 8, 100, [&](int r, int k) { return WD[(size_t)r * 3200 + k]; });
  a_frags(E.encf.data() + E.enc_wl_off / 2, 16, 4, 4, [&](int r, int k) { return WL[(size_t)r * 128 + k]; });
  E.encb.resize(128);
  acc_bias(E.encb.data(), 4, [&](int row) { return P.f32[P.ops[0].b_off + row]; });
}

void pack_fused16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& fs, bool enc, bool f16, Pack16Host& P) {
  std::vector<uint16_t>& w = P.w;
  pack_wt16(md, ops, pack, fs, f16, w);
  if (enc) pack_enc16(fs, w, P);

  // ---- tail constants ----
  const Layer& L2 = md.layers[fs.cl[7]];   // ConvT 64->32, kernel (2,2,32,64)
  const Layer& L3 = md.layers[fs.cl[8]];   // ConvT 32->16, kernel (2,2,16,32)
  const Layer& L4 = md.layers[fs.cl[9]];   // ConvT 16->8,  kernel (2,2,8,16)
  const Layer& LO = md.layers[fs.cl[10]];  // Conv 8->1,    kernel (3,3,8,1)
  std::vector<uint8_t>& cst = P.consts;
  cst.assign(TAIL_CONST_BYTES, 0);
  uint16_t* wc = reinterpret_cast<uint16_t*>(cst.data() + TC_OFF_WC);
  for (int kk = 0; kk < 10; ++kk)
    for (int l = 0; l < 64; ++l) {
      int n = l & 15, kg = l >> 4, oy = n >> 3, ox = n & 7;
      int wy = 2 * (kk / 5) + (kg & 1), wx = 2 * (kk % 5) + (kg >> 1);
      int ky = wy - oy, kx = wx - ox;
      for (int c = 0; c < 8; ++c) {
        float v = 0.f;
        if (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) v = (float)(LO.kernel[(size_t)(ky * 3 + kx) * 8 + c] / LOG2E);
        wc[((size_t)kk * 64 + l) * 8 + c] = to16(v, f16);
      }
    }
  // ConvT kernels (2, 2, Cout, Cin) are [row = (tap, co)][ci]: ConvT#3 [m-tile 2][k-step 2], ConvT#4 one fragment, k in accumulator order
  a_frags(reinterpret_cast<uint16_t*>(cst.data() + TC_OFF_W3), 32, 2, 2, [&](int r, int k) { return to16(L3.kernel[(size_t)r * 32 + k], f16); });
  a_frags(reinterpret_cast<uint16_t*>(cst.data() + TC_OFF_W4), 32, 1, 1, [&](int r, int k) { return to16(L4.kernel[(size_t)r * 16 + acc_k(k)], f16); });
  acc_bias(reinterpret_cast<float*>(cst.data() + TC_OFF_B2), 1, [&](int row) { return (float)(L2.bias[row] * LOG2E); });
  acc_bias(reinterpret_cast<float*>(cst.data() + TC_OFF_B3), 1, [&](int row) { return (float)(L3.bias[row & 15] * LOG2E); });
  acc_bias(reinterpret_cast<float*>(cst.data() + TC_OFF_B4), 1, [&](int row) { return (float)(L4.bias[row & 7] * LOG2E); });
  *reinterpret_cast<float*>(cst.data() + TC_OFF_BC) = LO.bias[0];
  P.w2f.resize((size_t)4 * 4 * 64 * 8);   // ConvT#2 [m-tile 4][k-step 4]
  a_frags(P.w2f.data(), 32, 4, 4, [&](int r, int k) { return to16(L2.kernel[(size_t)r * 64 + k], f16); });
  // ---- mid16 (ConvT#0 -> ConvT#1) operands ----
  const Layer& L0 = md.layers[fs.cl[5]];  // ConvT 256->128 (bias only; weights reuse the per-phase GEMM packing)
  const Layer& L1 = md.layers[fs.cl[6]];  // ConvT 128->64, kernel (2,2,64,128)
  P.w1f.resize((size_t)8 * 8 * 64 * 8);   // ConvT#1 [m-tile 8][k-step 8]: k-step st consumes accumulator tile st >> 1, registers 8 (st & 1) + j
  a_frags(P.w1f.data(), 32, 8, 8, [&](int r, int k) { return to16(L1.kernel[(size_t)r * 128 + acc_k(k)], f16); });
  // ConvT#0 weights, stage by stage, in the order the kernel's LDS tile holds them: stage (chunk c, tap t) of a phase = [128 rows][64 k]
  // = 1024 sixteen-byte pieces, piece row * 8 + slot holding k-piece slot ^ ((row >> 1) & 7) (the bank swizzle of the fragment reads).
  // A tile is then 16 KB of CONSECUTIVE memory.  Read from the GEMM layout Wt[128][Kpad] instead, its 128 row segments lie Kpad * 2 =
  // 512 / 1024 / 2048 bytes apart -- powers of two: every workgroup of a phase asks the same one or two L2 channels for the same tile
  // at the same time (round 3: the tile loads' cost did not hide behind anything, whatever the prefetch depth).
  int ph = 0;
  for (const Op16& o : fs.ops) {
    if (o.layer != 5 || ph >= 4) continue;
    const int NT = o.d.K / 256;
    P.w0t_off[ph++] = P.w0t.size();
    const uint16_t* W = w.data() + o.w_off;
    for (int st = 0; st < 4 * NT; ++st) {
      const int c = st / NT, t = st - c * NT;
      for (int i = 0; i < 1024; ++i) {
        const int row = i >> 3, kc = (i & 7) ^ ((row >> 1) & 7);
        for (int j = 0; j < 8; ++j) P.w0t.push_back(W[(size_t)row * o.Kpad + t * 256 + c * 64 + kc * 8 + j]);
      }
    }
  }
  P.midb.resize(128 + 64);
  acc_bias(P.midb.data(), 4, [&](int row) { return (float)(L0.bias[row] * LOG2E); });
  acc_bias(P.midb.data() + 128, 2, [&](int row) { return (float)(L1.bias[row] * LOG2E); });
}

// the generic 16-bit path: which graphs it takes, and their operands
static float from16(uint16_t v, bool f16) {
  uint32_t u;
  if (!f16) u = (uint32_t)v << 16;
  else {
    const uint32_t sign = (uint32_t)(v & 0x8000u) << 16, e = (v >> 10) & 31u, m = v & 0x3ffu;
    if (e == 0) {
      if (m == 0) u = sign;
      else { int sh = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++sh; } u = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13); }
    } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
    else u = sign | ((e + 112u) << 23) | (m << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

void any16_plan(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& P, Any16Pack& A) {
  P = Plan16();
  A = Any16Pack();
  auto no = [&](const std::string& w) { P = Plan16(); A = Any16Pack(); A.why = w; };   // a refused graph has no plan
  const std::vector<int> cl = compute_layers(md);
  const int n = (int)cl.size();
  if (n < 6) return no("fewer layers than encoder_10 + a dense layer + an output convolution");
  auto L = [&](int i) -> const Layer& { return md.layers[cl[i]]; };
  auto act_ok = [](int a) { return a == SRCFD_ACT_SWISH || a == SRCFD_ACT_LINEAR; };
  // 1. the first four compute layers are encoder_10's (enc16 is written for exactly these)
  if (md.in_shape[0] != 10 || md.in_shape[1] != 10 || md.in_shape[2] != 1) return no("input is not (10, 10, 1)");
  const Layer &c1 = L(0), &c2 = L(1), &de = L(2), &la = L(3);
  if (c1.kind != SRCFD_LAYER_CONV2D || c1.kh != 3 || c1.kw != 3 || c1.stride != 2 || !c1.same || c1.cin != 1 || c1.cout != 64 || c1.act != SRCFD_ACT_SWISH ||
      c2.kind != SRCFD_LAYER_CONV2D || c2.kh != 3 || c2.kw != 3 || c2.stride != 1 || !c2.same || c2.cin != 64 || c2.cout != 128 || c2.act != SRCFD_ACT_SWISH ||
      de.kind != SRCFD_LAYER_DENSE || de.cin != 3200 || de.cout != 128 || !act_ok(de.act) || la.kind != SRCFD_LAYER_DENSE || la.cin != 128 || la.cout > 64 ||
      !act_ok(la.act))
    return no("the first four layers are not encoder_10's");
  // 2. the last layer: 3x3 stride-1 SAME Conv2D to one channel, linear
  const Layer& lo = L(n - 1);
  if (lo.kind != SRCFD_LAYER_CONV2D || lo.kh != 3 || lo.kw != 3 || lo.stride != 1 || !lo.same || lo.cout != 1 || lo.act != SRCFD_ACT_LINEAR || lo.cin % 16 != 0 ||
      lo.cin > 64)
    return no("the last layer is not a 3x3 stride-1 'same' Conv2D from 16 / 32 / 48 / 64 channels to one, linear");
  // 3. everything in between has a 16-bit kernel
  for (int i = 4; i < n - 1; ++i) {
    const Layer& l = L(i);
    if (!act_ok(l.act)) return no("layer '" + l.name + "': activation");
    if (l.kind == SRCFD_LAYER_DENSE) {
      if (!(i == 4 ? l.cin <= 64 : l.cin % 64 == 0) || l.cout % 64 != 0) return no("layer '" + l.name + "': dense width");
    } else if (l.kind == SRCFD_LAYER_CONV2D_TRANSPOSE) {
      const bool k2 = l.kh == 2 && l.kw == 2 && l.stride == 2, k3 = l.kh == 3 && l.kw == 3 && l.stride == 2;
      if (!k2 && !k3) return no("layer '" + l.name + "': only 2x2 and 3x3 stride-2 transposed convolutions");
      if (l.cin % 16 != 0 || l.cout % 4 != 0) return no("layer '" + l.name + "': channel counts");
    } else return no("layer '" + l.name + "': no 16-bit kernel for this layer kind");
  }
  if (L(4).kind != SRCFD_LAYER_DENSE) return no("the layer behind latent_vector is not Dense");
  plan16(md, ops, pack, n - 2, true, P);
  A.max_act = 3200;   // conv2d_1's output when the encoder runs layer by layer
  for (const Op16& o : P.ops) {
    const Layer& l = md.layers[cl[o.layer]];
    if (o.d.K <= 0 || o.d.N % 4 != 0 || o.d.CO % 4 != 0 || o.d.OC % 4 != 0 || o.d.CI % 16 != 0 || (!any16_narrow(o.d) && o.d.K % 64 != 0))
      return no("layer '" + l.name + "': GEMM shape");
    A.max_act = std::max(A.max_act, (size_t)l.out_shape[0] * l.out_shape[1] * (o.layer == 3 ? 64 : l.out_shape[2]));
  }
  // gemm16 addresses a chunk's activations with 32-bit element offsets: the chunk shrinks with the largest activation
  // (lowp16_chunk_cap, fused_bf16.hip) and one sample has to fit
  if (A.max_act >= ((size_t)1 << 31)) return no("an activation of 2^31 elements or more per sample");
  if (P.ops.size() < 4 || P.ops[0].layer != 1 || P.ops[1].layer != 2 || P.ops[2].layer != 3) return no("unexpected plan shape");
  A.out_C = lo.cin; A.out_H = lo.in_shape[0]; A.out_W = lo.in_shape[1]; A.out_bias = lo.bias[0];
  A.ok = true;
}

void pack_any16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& A, bool f16, Any16Host& P) {
  const int n = (int)A.cl.size();
  pack_wt16(md, ops, pack, A, f16, P.w);
  pack_enc16(A, P.w, P);
  // output convolution: Keras kernel (3, 3, C, 1) = (ty, tx, ci)
  const Layer& lo = md.layers[A.cl[n - 1]];
  const double si = scale_in(md, A.cl, n - 1);
  P.wout.resize(lo.kernel.size());
  for (size_t i = 0; i < lo.kernel.size(); ++i) P.wout[i] = from16(to16((float)(lo.kernel[i] * si), f16), f16);
}

// trainer
ModelDesc index_model(const ModelDesc& src, std::vector<LayerInfo>& layers, int64_t& n_params, std::vector<float>& init) {
  ModelDesc im = src;
  int64_t off = 0;
  layers.clear();
  init.clear();
  for (size_t li = 0; li < im.layers.size(); ++li) {
    Layer& L = im.layers[li];
    if (L.kernel.empty()) continue;
    LayerInfo info;
    info.desc_index = (int)li;
    info.in_elems = (size_t)L.in_shape[0] * L.in_shape[1] * L.in_shape[2];
    info.out_elems = (size_t)L.out_shape[0] * L.out_shape[1] * L.out_shape[2];
    info.swish = L.act == SRCFD_ACT_SWISH;
    info.kernel_off = (size_t)off;
    init.insert(init.end(), L.kernel.begin(), L.kernel.end());
    for (size_t i = 0; i < L.kernel.size(); ++i) L.kernel[i] = (float)(off + (int64_t)i + 1);
    off += (int64_t)L.kernel.size();
    info.bias_off = (size_t)off;
    init.insert(init.end(), L.bias.begin(), L.bias.end());
    for (size_t i = 0; i < L.bias.size(); ++i) L.bias[i] = (float)(off + (int64_t)i + 1);
    off += (int64_t)L.bias.size();
    layers.push_back(info);
  }
  n_params = off;
  return im;
}

void build_dgrad(const ModelDesc& md, const std::vector<LayerInfo>& layers, std::vector<DgradOp>& dops, std::vector<float>& pack) {
  dops.clear();
  pack.clear();
  for (size_t ci = 1; ci < layers.size(); ++ci) {  // the first layer's input needs no gradient
    const Layer& L = md.layers[layers[ci].desc_index];
    const int IH = L.in_shape[0], IW = L.in_shape[1], OH = L.out_shape[0], OW = L.out_shape[1];
    GemmDesc d{};
    d.act = SRCFD_ACT_LINEAR;
    d.nphx = 1; d.os = 1;
    d.N = L.cin; d.Npad = round_up(d.N, 32); d.CO = L.cin; d.OC = L.cin;
    std::vector<float> B;
    if (L.kind == SRCFD_LAYER_DENSE) {
      d.MH = d.MW = 1; d.TY = d.TX = 1; d.CI = L.cout; d.IH = d.IW = 1; d.OH = d.OW = 1;
      d.K = L.cout;
      B.resize((size_t)d.K * d.N);
      for (int co = 0; co < L.cout; ++co)
        for (int c = 0; c < L.cin; ++c) B[(size_t)co * d.N + c] = L.kernel[(size_t)c * L.cout + co];
    } else if (L.kind == SRCFD_LAYER_CONV2D) {
      if (L.stride != 1) throw std::runtime_error("training: strided Conv2D is only supported as the first layer");
      int pt = 0, pl = 0;
      if (L.same) { pt = std::max((OH - 1) + L.kh - IH, 0) / 2; pl = std::max((OW - 1) + L.kw - IW, 0) / 2; }
      d.MH = IH; d.MW = IW; d.TY = L.kh; d.TX = L.kw; d.CI = L.cout; d.IH = OH; d.IW = OW; d.OH = IH; d.OW = IW;
      d.ay = d.ax = 1; d.by = d.bx = -1; d.cy = pt; d.cx = pl;
      d.K = L.kh * L.kw * L.cout;
      B.resize((size_t)d.K * d.N);
      for (int ky = 0; ky < L.kh; ++ky)
        for (int kx = 0; kx < L.kw; ++kx)
          for (int co = 0; co < L.cout; ++co)
            for (int c = 0; c < L.cin; ++c)
              B[((size_t)(ky * L.kw + kx) * L.cout + co) * d.N + c] = L.kernel[(((size_t)ky * L.kw + kx) * L.cin + c) * L.cout + co];
    } else {  // Conv2DTranspose, kernel (kh,kw,Cout,Cin): dX[i,j,ci] = sum dZ[s i + a - pb, s j + b - pb, co] W[a,b,co,ci] (0 outside; VALID: pb = 0)
      d.MH = IH; d.MW = IW; d.TY = L.kh; d.TX = L.kw; d.CI = L.cout; d.IH = OH; d.IW = OW; d.OH = IH; d.OW = IW;
      d.ay = d.ax = L.stride; d.by = d.bx = 1;
      d.cy = L.same ? -((L.kh - L.stride) / 2) : 0; d.cx = L.same ? -((L.kw - L.stride) / 2) : 0;
      d.K = L.kh * L.kw * L.cout;
      B = L.kernel;  // already [(a,b,co)][ci]
    }
    align64(pack);
    dops.push_back(DgradOp{d, put_B(pack, d, B), (int)ci});
  }
}

std::vector<int> wgrad_gmap(const Op& op, const std::vector<float>& ipack) {
  const GemmDesc& d = op.d;
  std::vector<int> gmap((size_t)(d.K + 1) * d.Npad, 0);
  for (int k = 0; k < d.K; ++k)
    for (int n = 0; n < d.N; ++n) gmap[(size_t)k * d.Npad + n] = (int)ipack[op.w_off + (size_t)k * d.Npad + n];
  for (int n = 0; n < d.N; ++n) gmap[(size_t)d.K * d.Npad + n] = (int)ipack[op.b_off + n];
  return gmap;
}

GatherMap gather_map(const std::vector<float>& ipack, const std::vector<float>& dpack, const std::vector<int>* tail_map) {
  GatherMap g;
  for (float v : ipack) g.map.push_back((int)v);
  align64(g.map);
  g.dpack_off = g.map.size();
  for (float v : dpack) g.map.push_back((int)v);
  align64(g.map);
  g.dpack_elems = g.map.size() - g.dpack_off;
  g.tail_off = g.map.size();            // the scaled slots come last (gather_pack_f32: one scale region)
  if (tail_map) g.map.insert(g.map.end(), tail_map->begin(), tail_map->end());
  align64(g.map);
  return g;
}

std::vector<TrainOp> train_ops(const std::vector<Op>& iops, const std::vector<LayerInfo>& layers) {
  std::vector<TrainOp> ops;
  for (const Op& op : iops) {
    TrainOp to{op.d, op.w_off, op.b_off, -1};
    to.fwd.act = SRCFD_ACT_LINEAR;
    for (size_t k = 0; k < layers.size(); ++k) if (layers[k].desc_index == op.layer) to.layer = (int)k;
    ops.push_back(to);
  }
  return ops;
}

bool wgrad_is_n1_k72(const GemmDesc& d) { return d.N == 1 && d.TY == 3 && d.TX == 3 && d.CI == 8 && d.nphx == 1; }

WgradPlan wgrad_plan(const GemmDesc& d) {
  WgradPlan p;
  if (wgrad_is_n1_k72(d)) {
    p = WgradPlan{0, 0, 1, 1, 3, 1, 0, 0};
    p.nslices = (int)std::max<int64_t>(1, std::min<int64_t>(256, ((int64_t)d.M + 1023) / 1024));
    p.rps = (d.M + p.nslices - 1) / p.nslices;
    p.nslices = std::max(1, (d.M + p.rps - 1) / p.rps);
    return p;
  }
  p.ktiles = (d.K + 1 + 31) / 32;
  p.ntiles = d.Npad / 32;
  p.KG = p.ktiles >= 2 ? 2 : 1;
  p.NG = p.ntiles >= 3 ? 4 : (p.ntiles == 2 ? 2 : 1);
  p.kblocks = (p.ktiles + p.KG - 1) / p.KG;
  p.nblocks = (p.ntiles + p.NG - 1) / p.NG;
  const int64_t blocks = (int64_t)p.kblocks * p.nblocks, chunks = std::max<int64_t>(1, ((int64_t)d.M + WG_RC - 1) / WG_RC);
  int64_t want = std::max<int64_t>(1, std::min<int64_t>(chunks, 512 / blocks));
  p.rps = (int)(((chunks + want - 1) / want) * WG_RC);
  p.nslices = (int)std::max<int64_t>(1, ((int64_t)d.M + p.rps - 1) / p.rps);
  return p;
}

StepPlan plan_step(const std::vector<TrainOp>& ops, int Lg, int n, int tail_slabs) {
  StepPlan P;
  P.part_floats.assign(ops.size(), 0);
  auto add = [&P](int op, const WgradPlan& wp, int64_t elems, int nslices) {
    SlabSum e{};
    e.op = op; e.wp = wp; e.elems = elems; e.nslices = nslices;
    e.groups = finish_groups(nslices);
    e.block0 = P.blocks;
    const int epb = 256 / e.groups;   // consecutive elements per workgroup
    P.blocks += (int)((elems + epb - 1) / epb);
    P.sums.push_back(e);
  };
  if (tail_slabs > 0) add(-1, WgradPlan{}, TT_PARAMS, tail_slabs);
  for (int li = Lg - 1; li >= 0; --li) {
    int first = -1;
    for (size_t i = 0; i < ops.size(); ++i) {
      if (ops[i].layer != li) continue;
      GemmDesc d = ops[i].fwd;
      d.M = n * d.MH * d.MW;
      const WgradPlan wp = wgrad_plan(d);
      const int64_t elems = (int64_t)(d.K + 1) * d.Npad;
      const int me = (int)P.sums.size();
      add((int)i, wp, elems, wp.nslices);
      P.part_floats[i] = (size_t)wp.nslices * (size_t)elems;
      if (first < 0) first = me;
      else {
        SlabSum& f0 = P.sums[first];
        f0.extra[f0.nextra++] = me;
        P.sums[me].bias_skip = 1;
      }
    }
  }
  return P;
}

SlabSpace plan_slab_space(const std::vector<TrainOp>& ops, int Lg, int max_batch) {
  SlabSpace S;
  S.cap.assign(ops.size(), 0);
  for (int b = 1; b <= max_batch; ++b) {
    const StepPlan P = plan_step(ops, Lg, b, 0);
    for (size_t i = 0; i < ops.size(); ++i) S.cap[i] = std::max(S.cap[i], P.part_floats[i]);
  }
  for (size_t i = 0; i < ops.size(); ++i) {   // space of its own: the sum of one op never has to finish before the next op's slabs are written
    S.off.push_back(S.total);
    S.total += (S.cap[i] + 63) / 64 * 64;
  }
  return S;
}

}  // namespace srcfd
