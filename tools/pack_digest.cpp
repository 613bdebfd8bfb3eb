// Host-only harness for the operand packers (sr-for-cfd_amd/csrc/operand_pack.cpp): packs a whole-model .h5 (loaded through
// model.cpp) the way the engine, the 16-bit path and the trainer do, plus three small graphs built here from a seeded generator,
// and prints JSON: per named section its offset, length (elements) and sha256.  Built by `make -C sr-for-cfd_amd/csrc pack_digest`
// with -fsanitize=address,undefined; tests/test_operand_pack.py compares the output with tests/golden/operand_pack_digests.json.
//   pack_digest <superres.h5> [dump-dir [family.h5]]     dump-dir: raw arrays for the test's property checks, and the training step's
//   weight-gradient plan as text (dump_train_plan, tests/test_train_plan.py), and the f32 GEMM's launch plan of every graph as text
//   (PlanDump, tests/test_gemm32_plan.py)
//   pack_digest --forms <forms.txt> <dump-dir>           only the f32 GEMM launch plan of the layer graphs listed in forms.txt, each at
//   its own batch size (tests/gemm32_forms.py writes the list, tests/test_gemm32_forms.py reads `forms.gemm32.plan.txt`) and, in a file of its own, `forms.x3.plan.txt`, the split-bf16 GEMM's plan
//   (x3_plan.cpp) of every layer of those graphs that it takes, on 256 CUs (tests/x3_forms.py, tests/test_x3_forms.py); prints nothing
//   pack_digest --lowp16 <graphs.txt> <dump-dir>         only the 16-bit forward's chunk plan (lowp16_plan.cpp) of the graphs listed in
//   graphs.txt, at every batch, CU count and switch set of tests/test_lowp16_plan.py, as `lowp16.plan.txt`; prints nothing
//   family.h5: a whole-model file of another member of the notebook's family (family.py, e.g. encoder_10 + decoder_100, with
//   padding='same' transposed convolutions); adds `family.*` sections: its f32 plan and the trainer's maps without the fused tail.
// Which fused kernels a graph qualifies for is decided in engine.hip / fused_bf16.hip / train_tail.hip (HIP translation units this
// harness does not link); find_chain() and the shape tests below restate those decisions for the graphs at hand, and the recorded
// `plan` / `fused.c1_off` / `train.tail_plan` sections pin them.
#include <cstdio>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include "../sr-for-cfd_amd/csrc/gemm32_plan.h"
#include "../sr-for-cfd_amd/csrc/lowp16_plan.h"
#include "../sr-for-cfd_amd/csrc/x3_plan.h"
#include "../sr-for-cfd_amd/csrc/operand_pack.h"
#include "sha256.h"

namespace srcfd {
thread_local std::string g_last_error;
void set_error(const std::string& m) { g_last_error = m; }
}  // namespace srcfd
using namespace srcfd;

static bool g_first = true;
static std::string g_dump;
template <class T> static void section(const std::string& name, const T* p, size_t len, size_t off = 0) {
  std::printf("%s\n  {\"name\": \"%s\", \"off\": %zu, \"len\": %zu, \"sha256\": \"%s\"}", g_first ? "" : ",", name.c_str(), off, len,
              sha256_hex(p, len * sizeof(T)).c_str());
  g_first = false;
}
template <class T> static void whole(const std::string& name, const std::vector<T>& v, bool dump = false) {
  section(name, v.data(), v.size());
  if (dump && !g_dump.empty()) {
    FILE* f = std::fopen((g_dump + "/" + name + ".bin").c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); std::exit(2); }
    std::fclose(f);
  }
}
static void ints(const std::string& name, const std::vector<int64_t>& v) { section(name, v.data(), v.size()); }

// first op of a run of kernel == stride == 2 transposed convolutions on consecutive layers with these channel counts, or -1
static int find_chain(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<int>& ch) {
  const size_t n = ch.size() - 1;
  for (size_t i = 0; i + n <= ops.size(); ++i) {
    bool ok = true;
    for (size_t q = 0; q < n && ok; ++q) {
      const Layer& L = md.layers[ops[i + q].layer];
      ok = L.kind == SRCFD_LAYER_CONV2D_TRANSPOSE && L.kh == 2 && L.kw == 2 && L.stride == 2 && L.cin == ch[q] && L.cout == ch[q + 1] &&
           ops[i + q].d.nphx == 2 && ops[i + q].layer == ops[i].layer + (int)q;
    }
    if (ok) return (int)i;
  }
  return -1;
}

// the f32 engine's operands: finish_create() of engine.hip
static void f32_sections(const std::string& tag, const ModelDesc& md, std::vector<Op>& ops, std::vector<float>& pack) {
  build_plan(md, ops, pack);
  auto L = [&](int op) -> const Layer& { return md.layers[ops[op].layer]; };
  PairPack pair; TriplePack tri; Tail32Pack t32;
  const int pair_op = find_chain(md, ops, {32, 16, 8});
  if (pair_op >= 0) pair = pack_convt_pair(pack, L(pair_op), L(pair_op + 1));
  const int triple_op = find_chain(md, ops, {64, 32, 16, 8});
  if (triple_op >= 0) tri = pack_convt_triple(pack, L(triple_op), L(triple_op + 1), L(triple_op + 2));
  int tail32_op = -1;
  if (triple_op >= 0 && (size_t)triple_op + 4 == ops.size() && L(triple_op + 3).kind == SRCFD_LAYER_CONV2D && L(triple_op + 3).cin == 8 && L(triple_op + 3).cout == 1) {
    tail32_op = triple_op;
    t32 = pack_tail32(pack, L(tail32_op), L(tail32_op + 1), L(tail32_op + 2), L(tail32_op + 3));
  }
  size_t enc32_w2 = 0;
  const bool enc32_ok = ops.size() >= 4 && md.in_shape[0] == 10 && md.in_shape[2] == 1 && L(1).kind == SRCFD_LAYER_CONV2D && L(1).cin == 64 && L(1).cout == 128;
  if (enc32_ok) enc32_w2 = pack_enc32(pack, L(1));
  // SRCFD_PREC_FP32X3: gemm_x3_qualifies() / gemm_x3_kpad() of kernels_x3.hip (32-deep k tiles, 128-channel blocks)
  std::vector<int64_t> x3_off(ops.size(), -1);
  std::vector<uint16_t> px;
  for (size_t i = 0; i < ops.size(); ++i) {
    const GemmDesc& d = ops[i].d;
    if (!(d.K >= 128 && d.CI % 32 == 0 && d.N % 128 == 0 && d.CO % 32 == 0 && d.OC % 4 == 0 && (d.act == SRCFD_ACT_SWISH || d.act == SRCFD_ACT_LINEAR))) continue;
    const int Kpad = round_up(d.K, 32);
    align64(px);
    x3_off[i] = (int64_t)px.size();
    px.resize(px.size() + (size_t)3 * d.N * Kpad);
    split_planes(pack.data() + ops[i].w_off, d.K, d.N, d.Npad, Kpad, px.data() + x3_off[i]);
  }
  int64_t w1x = -1, w2x = -1;
  if (tail32_op >= 0) pack_tail32_x3(px, L(tail32_op), L(tail32_op + 1), w1x, w2x);

  whole(tag + "pack", pack, tag.empty());
  std::vector<int64_t> oo;
  for (const Op& o : ops) { oo.push_back((int64_t)o.w_off); oo.push_back((int64_t)o.b_off); }
  ints(tag + "ops_off", oo);
  ints(tag + "plan", {pair_op, triple_op, tail32_op, (int64_t)enc32_ok});
  auto sec = [&](const char* n, size_t off, size_t len) { section(tag + "pack." + n, pack.data() + off, len, off); };
  if (enc32_ok) sec("enc32_w2", enc32_w2, 73728);
  if (pair_op >= 0) { sec("pair_wa", pair.wa, 2048); sec("pair_ba", pair.ba, 16); sec("pair_wb", pair.wb, 512); sec("pair_bb", pair.bb, 8); }
  if (triple_op >= 0) { sec("tri_w1", tri.w1, 8192); sec("tri_b1", tri.b1, 32); sec("tri_w2", tri.w2, 2048); sec("tri_b2", tri.b2, 16); sec("tri_w3", tri.w3, 512); sec("tri_b3", tri.b3, 8); }
  if (tail32_op >= 0) { sec("t32_w1", t32.w1, 8192); sec("t32_b1", t32.b1, 32); sec("t32_w2", t32.w2, 2048); sec("t32_b2", t32.b2, 16); sec("t32_w3", t32.w3, 512); sec("t32_b3", t32.b3, 8); sec("t32_wc", t32.wc, 73); }
  whole(tag + "pack_x3", px);
  ints(tag + "x3_off", x3_off);
  if (w1x >= 0) section(tag + "pack_x3.t32_w1x", px.data() + w1x, 24576, (size_t)w1x);
  if (w2x >= 0) section(tag + "pack_x3.t32_w2x", px.data() + w2x, 6144, (size_t)w2x);
}

// lowp16_plan() + build_pack() of fused_bf16.hip for the fused graph, both operand types
static void fused_sections(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack) {
  Plan16 fs;
  plan16(md, ops, pack, 6, false, fs);   // compute layers 1..6: conv2d_1 .. conv2d_transpose_1
  const bool enc_ok = true;   // encoder_10: fused_init's shape test (fused_bf16.hip)
  whole("fused.f32", fs.f32);
  std::vector<int64_t> bo;
  for (const Op16& o : fs.ops) bo.push_back((int64_t)o.b_off);
  ints("fused.b_off", bo);
  ints("fused.c1_off", {(int64_t)fs.c1w_off, (int64_t)fs.c1b_off, (int64_t)enc_ok});
  for (int f16 = 0; f16 < 2; ++f16) {
    const std::string px = f16 ? "f16." : "bf16.";
    Pack16Host P;
    pack_fused16(md, ops, pack, fs, enc_ok, f16 != 0, P);
    whole(px + "Wt", P.w);
    std::vector<int64_t> wo;
    for (const Op16& o : fs.ops) wo.push_back((int64_t)o.w_off);
    ints(px + "w_off", wo);
    whole(px + "encf", P.encf);
    ints(px + "enc_off", {(int64_t)P.enc_wd_off, (int64_t)P.enc_wl_off});
    whole(px + "encb", P.encb);
    whole(px + "consts", P.consts);
    whole(px + "w2f", P.w2f);
    whole(px + "w0t", P.w0t);
    ints(px + "w0t_off", {(int64_t)P.w0t_off[0], (int64_t)P.w0t_off[1], (int64_t)P.w0t_off[2], (int64_t)P.w0t_off[3]});
    whole(px + "w1f", P.w1f);
    whole(px + "midb", P.midb);
  }
}

// The trainer's weight-gradient plan (plan_step / plan_slab_space, what trainer_build sizes from and trainer_step issues from) as a
// text file in the dump directory, for tests/test_train_plan.py; no digest section.  Lines of integers behind a letter:
//   E tail n slot op nslices rps groups block0 elems bias_skip nextra extra0 extra1 extra2   one slot of the slab-sum table (-1: no extra)
//   T tail n workgroups                                                                      the whole launch
//   S tail max_batch op capacity offset                                                      an op's slab space, floats
// tail = 1: the last four layers fused (their slabs as one slot, op -1), as many slabs as tail_bwd32_blocks (train_tail.hip) gives
// on 256 CUs -- restated here, the host unit takes the count as a number. 
static void dump_train_plan(const std::string& tag, const std::vector<Op>& iops, const std::vector<LayerInfo>& layers, int tail_first, int tail_hw) {
  if (g_dump.empty()) return;
  const std::vector<TrainOp> ops = train_ops(iops, layers);
  FILE* f = std::fopen((g_dump + "/" + tag + "train.plan.txt").c_str(), "w");
  if (!f) std::exit(2);
  for (int tail = 0; tail <= (tail_first >= 0 ? 1 : 0); ++tail) {
    const int Lg = tail ? tail_first : (int)layers.size();
    for (int n = 1; n <= 32; ++n) {   // every batch a max_batch = 32 trainer takes
      const int64_t pairs = (((int64_t)n * tail_hw + 15) / 16 + 1) / 2;
      const StepPlan P = plan_step(ops, Lg, n, tail ? (int)std::max<int64_t>(1, std::min<int64_t>(pairs, 256)) : 0);
      for (size_t q = 0; q < P.sums.size(); ++q) {
        const SlabSum& e = P.sums[q];
        std::fprintf(f, "E %d %d %zu %d %d %d %d %d %lld %d %d", tail, n, q, e.op, e.nslices, e.wp.rps, e.groups, e.block0, (long long)e.elems, e.bias_skip, e.nextra);
        for (int x = 0; x < 3; ++x) std::fprintf(f, " %d", x < e.nextra ? e.extra[x] : -1);
        std::fprintf(f, "\n");
      }
      std::fprintf(f, "T %d %d %d\n", tail, n, P.blocks);
    }
    for (int mb : {7, 8, 32}) {
      const SlabSpace S = plan_slab_space(ops, Lg, mb);
      for (size_t i = 0; i < ops.size(); ++i) std::fprintf(f, "S %d %d %zu %zu %zu\n", tail, mb, i, S.cap[i], S.off[i]);
    }
  }
  std::fclose(f);
}
// The f32 GEMM's launch plan (gemm32_plan.cpp: what launch_gemm_mfma / launch_gemm_mfma_group issue and the slab buffers are sized
// from) as text in the dump directory, for tests/test_gemm32_plan.py; no digest section.  mode 0: inference (batch-invariant cut),
// 1: the training step's forward GEMMs, 2: its data-gradient GEMMs.  Per launch (the ops of one layer, or a single op) one line
//   G mode n first count grouped nb bkt vec gx gy gz fx fy ws_floats fits(ws_floats - 1) fits(ws_floats) fits(null)      (-1: not asked)
// and per op one line
//   O mode n index route splits kchunk slab_off finish_groups nb bkt vec gx gy gz fx epi_aux fuses_finalize splitk_ws_floats  + the descriptor:
//     M N K Npad MH MW TY TX CI IH IW ay by cy ax bx cx CO nphx OH OW OC os oy0 ox0 act
struct PlanDump {
  FILE* f = nullptr;
  FILE* fx = nullptr;   // forms only: the split-bf16 GEMM's plan (x3_plan.cpp), a file of its own
  int next = 0;   // running op index of the file
  explicit PlanDump(const std::string& tag, bool x3 = false) {
    if (g_dump.empty()) return;
    f = std::fopen((g_dump + "/" + tag + "gemm32.plan.txt").c_str(), "w");
    if (!f) std::exit(2);
    if (x3 && !(fx = std::fopen((g_dump + "/" + tag + "x3.plan.txt").c_str(), "w"))) std::exit(2);
  }
  ~PlanDump() { if (f) std::fclose(f); if (fx) std::fclose(fx); }
  // The split-bf16 GEMM's answer for the ops of one layer at batch n, where every op qualifies (what the engine asks before it sends a
  // layer there), on `cus` CUs.  Per layer one line
  //   X first count layer cus grouped group_grid first0 .. first4
  // and per op one line
  //   P index kernel(0 tile, 1 resident) kpad gx gy ntiles res_qualifies  + the descriptor
  void x3(const GemmDesc* ds, int count, int layer, int cus) {
    if (!fx) return;
    for (int q = 0; q < count; ++q) if (!gemm_x3_qualifies(ds[q])) return;
    const X3Plan p = plan_gemm_x3(ds, count, cus);
    if (p.count != count) std::exit(2);
    std::fprintf(fx, "X %d %d %d %d %d %u %d %d %d %d %d\n", next, count, layer, cus, (int)p.grouped, p.group_grid, p.first[0], p.first[1], p.first[2], p.first[3], p.first[4]);
    for (int q = 0; q < count; ++q) {
      const X3Op& o = p.op[q];
      const GemmDesc& d = ds[q];
      std::fprintf(fx, "P %d %d %d %u %u %d %d", next + q, (int)o.k, o.kpad, o.grid[0], o.grid[1], o.ntiles, (int)gemm_x3_res_qualifies(d));
      for (int v : {d.M, d.N, d.K, d.Npad, d.MH, d.MW, d.TY, d.TX, d.CI, d.IH, d.IW, d.ay, d.by, d.cy, d.ax, d.bx, d.cx, d.CO, d.nphx, d.OH, d.OW, d.OC, d.os,
                    d.oy0, d.ox0, d.act})
        std::fprintf(fx, " %d", v);
      std::fprintf(fx, "\n");
    }
  }
  void launch(int mode, int n, const GemmDesc* ds0, int count) {
    if (!f) return;
    GemmDesc ds[4];
    for (int q = 0; q < count; ++q) { ds[q] = ds0[q]; ds[q].M = n * ds[q].MH * ds[q].MW; }
    const bool inv = mode == 0;
    const Gemm32Plan p = plan_gemm32(ds, count, inv);
    if (p.count != count) std::exit(2);
    float slab = 0.f;   // any non-null address: gemm32_ws_fits does not touch it
    const Gemm32Launch& g = p.group;
    std::fprintf(f, "G %d %d %d %d %d %d %d %d %u %u %u %u %u %zu %d %d %d\n", mode, n, next, count, (int)p.grouped, g.nb, g.bkt, g.vec, g.grid[0], g.grid[1],
                 g.grid[2], g.fin[0], g.fin[1], p.ws_floats, p.ws_floats ? (int)gemm32_ws_fits(p, &slab, p.ws_floats - 1) : -1,
                 (int)gemm32_ws_fits(p, &slab, p.ws_floats), (int)gemm32_ws_fits(p, nullptr, p.ws_floats));
    for (int q = 0; q < count; ++q) {
      const Gemm32Op& o = p.op[q];
      const GemmDesc& d = ds[q];
      std::fprintf(f, "O %d %d %d %d %d %d %zu %d %d %d %d %u %u %u %u %d %d %zu", mode, n, next + q, (int)o.route, o.splits, o.kchunk, o.slab_off, o.finish_groups,
                   o.l.nb, o.l.bkt, o.l.vec, o.l.grid[0], o.l.grid[1], o.l.grid[2], o.l.fin[0], (int)gemm_supports_epi_aux(d), (int)gemm_fuses_finalize(d),
                   gemm_splitk_ws_floats(d, inv));
      for (int v : {d.M, d.N, d.K, d.Npad, d.MH, d.MW, d.TY, d.TX, d.CI, d.IH, d.IW, d.ay, d.by, d.cy, d.ax, d.bx, d.cx, d.CO, d.nphx, d.OH, d.OW, d.OC, d.os,
                    d.oy0, d.ox0, d.act})
        std::fprintf(f, " %d", v);
      std::fprintf(f, "\n");
    }
  }
  // every batch of a mode over a list of (descriptor, layer): the ops of one layer go out together, at most four
  void ops(int mode, const std::vector<GemmDesc>& ds, const std::vector<int>& layer) {
    const std::vector<int> batches = mode == 0 ? std::vector<int>{1, 3, 7, 64, 216, 768} : std::vector<int>{1, 2, 3, 4, 5, 6, 7, 8, 32};
    const int first = next;
    for (int n : batches) {
      next = first;
      for (size_t i = 0, j; i < ds.size(); i = j) {
        for (j = i + 1; j < ds.size() && mode != 2 && layer[j] == layer[i] && j - i < 4; ++j) {}
        launch(mode, n, ds.data() + i, (int)(j - i));
        next += (int)(j - i);
      }
    }
    next = first + (int)ds.size();
  }
  // one case of a forms list: the inference launches of a layer graph at one batch, the ops of a layer together as the engine sends
  // them.  Behind a line `C name batch`, and behind every launch's G / O lines one line
  //   B first count layer big      layer: index among the graph's layers; big: gemm32_big_qualifies for these descriptors at that batch
  void form(const std::string& name, const ModelDesc& md, int n) {
    if (!f) return;
    std::vector<Op> ops_;
    std::vector<float> pack;
    build_plan(md, ops_, pack);
    std::fprintf(f, "C %s %d\n", name.c_str(), n);
    if (fx) std::fprintf(fx, "C %s %d\n", name.c_str(), n);
    next = 0;
    for (size_t i = 0, j; i < ops_.size(); i = j) {
      GemmDesc ds[4];
      for (j = i; j < ops_.size() && ops_[j].layer == ops_[i].layer && j - i < 4; ++j) { ds[j - i] = ops_[j].d; ds[j - i].M = n * ops_[j].d.MH * ops_[j].d.MW; }
      launch(0, n, ds, (int)(j - i));
      x3(ds, (int)(j - i), ops_[i].layer, 256);
      std::fprintf(f, "B %d %d %d %d\n", next, (int)(j - i), ops_[i].layer, (int)gemm32_big_qualifies(ds, (int)(j - i)));
      next += (int)(j - i);
    }
  }
  // a layer graph: its forward ops as the engine launches them, as the trainer does (activation left to the epilogue), and the trainer's data gradients
  void graph(const ModelDesc& md) {
    std::vector<Op> ops_;
    std::vector<float> pack;
    build_plan(md, ops_, pack);
    std::vector<GemmDesc> ds;
    std::vector<int> layer;
    for (const Op& o : ops_) { ds.push_back(o.d); layer.push_back(o.layer); }
    ops(0, ds, layer);
    std::vector<LayerInfo> layers;
    int64_t n_params = 0;
    std::vector<float> init;
    const ModelDesc im = index_model(md, layers, n_params, init);
    build_plan(im, ops_, pack);
    ds.clear(); layer.clear();
    for (const TrainOp& o : train_ops(ops_, layers)) { ds.push_back(o.fwd); layer.push_back(o.layer); }
    ops(1, ds, layer);
    std::vector<DgradOp> dops;
    std::vector<float> dpack;
    build_dgrad(im, layers, dops, dpack);
    ds.clear(); layer.clear();
    for (const DgradOp& o : dops) { ds.push_back(o.d); layer.push_back(o.layer); }
    ops(2, ds, layer);
  }
};

static void dump_ops(const std::string& name, const std::vector<Op>& iops) {   // per op: K N Npad layer-kind, for the bijection check
  if (g_dump.empty()) return;
  FILE* f = std::fopen((g_dump + "/" + name).c_str(), "w");
  if (!f) std::exit(2);
  for (const Op& o : iops) std::fprintf(f, "%d %d %d %d %d\n", o.d.K, o.d.N, o.d.Npad, o.layer, o.d.nphx);
  std::fclose(f);
}

// trainer_build() of train.hip with the fused tail (train_tail_plan accepts decoder_400's last four layers)
static void train_sections(const ModelDesc& md) {
  std::vector<LayerInfo> layers;
  int64_t n_params = 0;
  std::vector<float> init;
  const ModelDesc im = index_model(md, layers, n_params, init);
  std::vector<Op> iops;
  std::vector<float> ipack;
  build_plan(im, iops, ipack);
  TrainTailPlan tail;
  tail.first_layer = (int)layers.size() - 4;
  const Layer& L1 = md.layers[layers[tail.first_layer].desc_index];
  tail.H = L1.in_shape[0]; tail.W = L1.in_shape[1];
  tail.param_off = layers[tail.first_layer].kernel_off;
  train_tail_slots(tail.param_off, tail);
  whole("train.scale", tail.scale, true);
  whole("train.tail_map", tail.map, true);
  ints("train.tail_plan", {tail.first_layer, tail.H, tail.W, (int64_t)tail.param_off, (int64_t)tail.t32_w1, (int64_t)tail.t32_b1, (int64_t)tail.t32_w2,
                           (int64_t)tail.t32_b2, (int64_t)tail.t32_w3, (int64_t)tail.t32_b3, (int64_t)tail.t32_wc, (int64_t)tail.wf, (int64_t)tail.wb,
                           (int64_t)tail.wt, (int64_t)tail.bias});
  std::vector<int> tg(TT_PARAMS);
  std::iota(tg.begin(), tg.end(), (int)tail.param_off + 1);
  whole("train.tail_gmap", tg);
  for (size_t i = 0; i < iops.size(); ++i) whole("train.op" + std::to_string(i) + ".gmap", wgrad_gmap(iops[i], ipack), true);
  std::vector<DgradOp> dops;
  std::vector<float> dpack;
  build_dgrad(im, layers, dops, dpack);
  const GatherMap gm = gather_map(ipack, dpack, &tail.map);
  whole("train.init_params", init, true);
  ints("train.offsets", {(int64_t)gm.dpack_off, (int64_t)gm.dpack_elems, (int64_t)gm.tail_off, (int64_t)gm.map.size(), n_params});
  std::vector<int64_t> doff;
  for (const DgradOp& o : dops) doff.push_back((int64_t)o.w_off);
  ints("train.dops_off", doff);
  whole("train.map", gm.map);
  dump_ops("train.ops.txt", iops);
  dump_train_plan("", iops, layers, tail.first_layer, tail.H * tail.W);
}

// a family member: the f32 engine's operands + trainer_build() layer by layer (train_tail_plan declines every decoder but decoder_400)
static void family_sections(const ModelDesc& md) {
  std::vector<Op> ops;
  std::vector<float> pack;
  f32_sections("family.", md, ops, pack);
  std::vector<int64_t> geo;   // per op: the row grid and the origins a cropped ('same') transposed convolution moves
  for (const Op& o : ops) for (int v : {o.layer, o.d.MH, o.d.MW, o.d.TY, o.d.TX, o.d.cy, o.d.cx, o.d.oy0, o.d.ox0, o.d.os, o.d.K, o.d.N}) geo.push_back(v);
  ints("family.ops_geometry", geo);
  {  // the 16-bit path of the family graphs: lowp16_plan() + build_pack() of fused_bf16.hip for both operand types
    Plan16 P16;
    Any16Pack A;
    any16_plan(md, ops, pack, P16, A);
    ints("family.any16.plan", {(int64_t)A.ok, (int64_t)P16.ops.size(), A.out_C, A.out_H, A.out_W, (int64_t)A.max_act, (int64_t)P16.c1w_off, (int64_t)P16.c1b_off});
    if (A.ok) {
      whole("family.any16.f32", P16.f32);
      for (int f16 = 0; f16 < 2; ++f16) {
        const std::string px = f16 ? "family.any16.f16." : "family.any16.bf16.";
        Any16Host P;
        pack_any16(md, ops, pack, P16, f16 != 0, P);
        whole(px + "Wt", P.w);
        whole(px + "encf", P.encf);
        whole(px + "encb", P.encb);
        whole(px + "wout", P.wout, true);
        std::vector<int64_t> wo;
        for (const Op16& o : P16.ops) { wo.push_back((int64_t)o.w_off); wo.push_back(o.Kpad); wo.push_back(o.d.Npad); wo.push_back(any16_narrow(o.d)); }
        ints(px + "w_off", wo);
      }
    }
  }
  std::vector<LayerInfo> layers;
  int64_t n_params = 0;
  std::vector<float> init;
  const ModelDesc im = index_model(md, layers, n_params, init);
  std::vector<Op> iops;
  std::vector<float> ipack;
  build_plan(im, iops, ipack);
  for (size_t i = 0; i < iops.size(); ++i) whole("family.train.op" + std::to_string(i) + ".gmap", wgrad_gmap(iops[i], ipack), true);
  std::vector<DgradOp> dops;
  std::vector<float> dpack;
  build_dgrad(im, layers, dops, dpack);
  const GatherMap gm = gather_map(ipack, dpack, nullptr);
  ints("family.train.offsets", {(int64_t)gm.dpack_off, (int64_t)gm.dpack_elems, (int64_t)gm.tail_off, (int64_t)gm.map.size(), n_params});
  std::vector<int64_t> dgeo;
  for (const DgradOp& o : dops) for (int64_t v : {(int64_t)o.w_off, (int64_t)o.layer, (int64_t)o.d.cy, (int64_t)o.d.cx, (int64_t)o.d.ay, (int64_t)o.d.K, (int64_t)o.d.N}) dgeo.push_back(v);
  ints("family.train.dops", dgeo);
  whole("family.train.map", gm.map);
  dump_ops("family.train.ops.txt", iops);
}

// small graphs from a seeded generator (the same sequence is easy to write in any language: a 32-bit LCG, top 24 bits - 0.5)
struct Lcg {
  uint32_t s;
  std::vector<float> take(size_t n) {
    std::vector<float> v(n);
    for (float& x : v) { s = s * 1664525u + 1013904223u; x = (float)((double)(s >> 8) / 16777216.0 - 0.5); }
    return v;
  }
};
static Layer layer(Lcg& g, int kind, int act, int k, int stride, int same, int cin, int cout, const char* name) {
  Layer L;
  L.kind = kind; L.act = act; L.kh = L.kw = k; L.stride = stride; L.same = same; L.cin = cin; L.cout = cout; L.name = name;
  if (kind != SRCFD_LAYER_FLATTEN) { L.kernel = g.take((size_t)k * k * cin * cout); L.bias = g.take(cout); }
  return L;
}
static void small_graph(const std::string& tag, ModelDesc md, bool train_plan = false) {
  md.infer_shapes();
  std::vector<Op> ops;
  std::vector<float> pack;
  f32_sections(tag, md, ops, pack);
  PlanDump(tag).graph(md);
  if (train_plan) {   // trainer_build() layer by layer
    std::vector<LayerInfo> layers;
    int64_t n_params = 0;
    std::vector<float> init;
    const ModelDesc im = index_model(md, layers, n_params, init);
    build_plan(im, ops, pack);
    dump_ops(tag + "train.ops.txt", ops);
    dump_train_plan(tag, ops, layers, -1, 0);
  }
}

// The forms list: plain text, one graph after the other (the whole-model .h5 layout holds an encoder / decoder pair of the
// notebook's family only, which none of these graphs is).  Integers are the enums of include/srcfd.h:
//   case <name> <batch> <in_h> <in_w> <in_c> <layers>
//   layer <kind> <activation> <kh> <kw> <stride> <same> <cin> <cout>  x layers; the plan does not read the weights: zeros
//   a Reshape layer carries its target in the last three places: layer <kind> 0 1 1 1 <h> <w> <c>
static int read_graphs(const char* list, const std::function<void(const std::string&, const ModelDesc&, int)>& take) {
  FILE* in = std::fopen(list, "r");
  if (!in) { std::fprintf(stderr, "cannot read %s\n", list); return 2; }
  char name[128];
  int n, h, w, c, nl, cases = 0;
  while (std::fscanf(in, " case %127s %d %d %d %d %d", name, &n, &h, &w, &c, &nl) == 6) {
    ModelDesc md;
    md.in_shape[0] = h; md.in_shape[1] = w; md.in_shape[2] = c;
    for (int i = 0; i < nl; ++i) {
      Layer L;
      int same;
      if (std::fscanf(in, " layer %d %d %d %d %d %d %d %d", &L.kind, &L.act, &L.kh, &L.kw, &L.stride, &same, &L.cin, &L.cout) != 8 || L.kh < 0 || L.kw < 0 || L.cin < 0 || L.cout < 0) {
        std::fprintf(stderr, "%s: bad layer %d of case %s\n", list, i, name);
        std::fclose(in);
        return 2;
      }
      L.same = same != 0; L.name = "l" + std::to_string(i);
      if (L.kind == SRCFD_LAYER_RESHAPE) { L.reshape[0] = same; L.reshape[1] = L.cin; L.reshape[2] = L.cout; L.same = 0; L.cin = L.cout = 0; }
      else if (L.kind != SRCFD_LAYER_FLATTEN) { L.kernel.assign((size_t)L.kh * L.kw * L.cin * L.cout, 0.f); L.bias.assign(L.cout, 0.f); }
      md.layers.push_back(L);
    }
    md.infer_shapes();
    take(name, md, n);
    ++cases;
  }
  const bool whole = std::feof(in) != 0;
  std::fclose(in);
  if (!whole || !cases) { std::fprintf(stderr, "%s: not a graph list (stopped behind case %d)\n", list, cases); return 2; }
  return 0;
}
static int dump_forms(const char* list) {
  PlanDump out("forms.", true);
  return read_graphs(list, [&](const std::string& name, const ModelDesc& md, int n) { out.form(name, md, n); });
}

// The 16-bit forward's chunk plan (lowp16_plan.cpp: what fused_bf16.hip issues) of every listed graph as text, for
// tests/test_lowp16_plan.py; the graph goes through lowp16_plan() of fused_bf16.hip: plan16 for encoder_10 + decoder_400 (the fused
// graph; enc_ok as fused_init finds it for encoder_10), any16_plan for the rest.  Per graph
//   G name fused enc_ok out_H out_W ops
//   Q index layer Kpad + the descriptor (M = 0)                        one line per op of the Plan16
// then per switch set (SETS below, by index), CU count and chunk
//   C set num_cus c steps t1_buf tail_seg slab_floats lowp16_slab_elems(c)
//   S kernel op0 nops src dst bn splits kslice nz gx gy gz fin slab_floats g0 g1 shape nblk0..3 seg blocks + the descriptor   one per step
static void print_desc(FILE* f, const GemmDesc& d) {
  for (int v : {d.M, d.N, d.K, d.Npad, d.MH, d.MW, d.TY, d.TX, d.CI, d.IH, d.IW, d.ay, d.by, d.cy, d.ax, d.bx, d.cx, d.CO, d.nphx, d.OH, d.OW, d.OC, d.os, d.oy0,
                d.ox0, d.act})
    std::fprintf(f, " %d", v);
  std::fprintf(f, "\n");
}
static int dump_lowp16(const char* list) {
  FILE* f = std::fopen((g_dump + "/lowp16.plan.txt").c_str(), "w");
  if (!f) return 2;
  std::vector<Switches> sets(11);   // default, then SRCFD_ENC=0, DENSE1=0, MID=0, MID=1, MID=2, MID_WAVES=4, MID_WAVES=16, TAIL=s, TAIL_SEG=1, TAIL_SEG=5
  sets[1].enc16 = false; sets[2].dense1_16 = false; sets[3].mid16 = false; sets[4].mid_shape = 1; sets[5].mid_shape = 2; sets[6].mid_waves = 4;
  sets[7].mid_waves = 16; sets[8].tail16s = true; sets[9].tail_seg = 1; sets[10].tail_seg = 5;
  bool bad = false;
  const int rc = read_graphs(list, [&](const std::string& name, const ModelDesc& md, int) {
    std::vector<Op> ops;
    std::vector<float> pack;
    build_plan(md, ops, pack);
    Plan16 P;
    Graph16 g;
    g.fused = md.is_sr_10_400();
    if (g.fused) {
      plan16(md, ops, pack, 6, false, P);
      g.enc_ok = true;
    } else {
      Any16Pack A;
      any16_plan(md, ops, pack, P, A);
      if (!A.ok) { std::fprintf(stderr, "%s: %s\n", name.c_str(), A.why.c_str()); bad = true; return; }
      g.out_H = A.out_H; g.out_W = A.out_W;
    }
    std::fprintf(f, "G %s %d %d %d %d %zu\n", name.c_str(), (int)g.fused, (int)g.enc_ok, g.out_H, g.out_W, P.ops.size());
    for (size_t i = 0; i < P.ops.size(); ++i) {
      std::fprintf(f, "Q %zu %d %d", i, P.ops[i].layer, P.ops[i].Kpad);
      print_desc(f, P.ops[i].d);
    }
    const std::vector<int> batches = g.fused ? std::vector<int>{1, 3, 7, 64, 216, 256, 257, 768, 1024} : std::vector<int>{1, 3, 130, 67, 259};
    for (size_t q = 0; q < sets.size(); ++q)
      for (int cus : {256, 64})
        for (int c : batches) {
          const Chunk16Plan p = plan_chunk16(P, g, sets[q], c, cus);
          std::fprintf(f, "C %zu %d %d %zu %d %d %zu %zu\n", q, cus, c, p.steps.size(), p.t1_buf, p.tail_seg, p.slab_floats, lowp16_slab_elems((size_t)c));
          for (const Step16& s : p.steps) {
            std::fprintf(f, "S %d %d %d %d %d %d %d %d %d %u %u %u %u %zu %u %u %d %d %d %d %d %d %d", (int)s.k, s.op0, s.nops, s.src, s.dst, s.cut.bn, s.cut.splits,
                         s.cut.kslice, s.cut.nz, s.cut.grid[0], s.cut.grid[1], s.cut.grid[2], s.cut.fin, s.cut.slab_floats, s.grid[0], s.grid[1], (int)s.shape,
                         s.nblk[0], s.nblk[1], s.nblk[2], s.nblk[3], s.seg, s.blocks);
            print_desc(f, s.d);
          }
        }
  });
  std::fclose(f);
  return rc ? rc : (bad ? 2 : 0);
}

int main(int argc, char** argv) {
  if (argc == 4 && (std::string(argv[1]) == "--forms" || std::string(argv[1]) == "--lowp16")) {
    g_dump = argv[3];
    try {
      return std::string(argv[1]) == "--forms" ? dump_forms(argv[2]) : dump_lowp16(argv[2]);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "pack_digest: %s\n", e.what());
      return 1;
    }
  }
  if (argc < 2) { std::fprintf(stderr, "usage: pack_digest <superres.h5> [dump-dir [family.h5]] | pack_digest --forms <forms.txt> <dump-dir> | pack_digest --lowp16 <graphs.txt> <dump-dir>\n"); return 2; }
  if (argc > 2) g_dump = argv[2];
  try {
    std::printf("{\"sections\": [");
    ModelDesc md;
    append_h5_whole(md, argv[1]);
    md.infer_shapes();
    std::vector<Op> ops;
    std::vector<float> pack;
    f32_sections("", md, ops, pack);
    if (!md.is_sr_10_400()) { std::fprintf(stderr, "not the encoder_10 + decoder_400 graph\n"); return 2; }
    fused_sections(md, ops, pack);
    train_sections(md);
    const int CT = SRCFD_LAYER_CONV2D_TRANSPOSE, CV = SRCFD_LAYER_CONV2D, DE = SRCFD_LAYER_DENSE, SW = SRCFD_ACT_SWISH;
    {  // a 3x3 stride-2 ConvT: four output phases with 4 / 2 / 2 / 1 taps
      Lcg g{1};
      ModelDesc m; m.in_shape[0] = 4; m.in_shape[1] = 4; m.in_shape[2] = 8;
      m.layers = {layer(g, CT, SW, 3, 2, 0, 8, 4, "ct")};
      small_graph("convt3.", m, true);
    }
    {  // 32 -> 16 -> 8 with no 64 -> 32 in front: the pair without the triple
      Lcg g{2};
      ModelDesc m; m.in_shape[0] = 5; m.in_shape[1] = 5; m.in_shape[2] = 32;
      m.layers = {layer(g, CT, SW, 2, 2, 0, 32, 16, "a"), layer(g, CT, SW, 2, 2, 0, 16, 8, "b")};
      small_graph("pair.", m);
    }
    {  // an encoder whose second convolution has 64 channels, not 128: plan_enc32 declines
      Lcg g{3};
      ModelDesc m; m.in_shape[0] = 10; m.in_shape[1] = 10; m.in_shape[2] = 1;
      Layer fl; fl.kind = SRCFD_LAYER_FLATTEN; fl.name = "f";
      m.layers = {layer(g, CV, SW, 3, 2, 1, 1, 64, "c1"), layer(g, CV, SW, 3, 1, 1, 64, 64, "c2"), fl, layer(g, DE, SW, 1, 1, 0, 1600, 128, "d"),
                  layer(g, DE, SRCFD_ACT_LINEAR, 1, 1, 0, 128, 50, "l")};
      small_graph("noenc32.", m);
    }
    PlanDump("").graph(md);
    {  // graphs and descriptors for the branches of the f32 GEMM's plan that the graphs above do not reach (text dump only)
      PlanDump hand("hand.");
      Lcg g{4};
      ModelDesc a; a.in_shape[0] = 10; a.in_shape[1] = 10; a.in_shape[2] = 8;   // 3x3 8 -> 1, not SAME, rows 8 wide: conv_n1x4_f32
      a.layers = {layer(g, CV, SW, 3, 1, 0, 8, 1, "n1x4")};
      a.infer_shapes();
      hand.graph(a);
      // 3 -> 1 channels (conv_n1_f32, CI % 4 != 0), 1 -> 4 SAME (conv_ci1_f32), then a ConvT with one output channel: a layer
      // whose phases are no generic GEMMs
      ModelDesc b; b.in_shape[0] = 6; b.in_shape[1] = 6; b.in_shape[2] = 3;
      b.layers = {layer(g, CV, SW, 3, 1, 0, 3, 1, "n1"), layer(g, CV, SW, 3, 1, 1, 1, 4, "ci1"), layer(g, CT, SW, 3, 2, 0, 4, 1, "ct_n1")};
      b.infer_shapes();
      hand.graph(b);
      // a ConvT with K = 4096 in its first phase: the training cut reaches 32 slabs and more, which a single launch finishes in 8 groups
      ModelDesc c; c.in_shape[0] = 4; c.in_shape[1] = 4; c.in_shape[2] = 1024;
      c.layers = {layer(g, CT, SW, 3, 2, 0, 1024, 4, "ct_deep")};
      c.infer_shapes();
      hand.graph(c);
      // no real layer has phases of different widths or gather forms: the convt3 phases with one of them altered
      ModelDesc m; m.in_shape[0] = 4; m.in_shape[1] = 4; m.in_shape[2] = 8;
      m.layers = {layer(g, CT, SW, 3, 2, 0, 8, 4, "ct")};
      m.infer_shapes();
      std::vector<Op> o4;
      std::vector<float> pk;
      build_plan(m, o4, pk);
      std::vector<GemmDesc> wide, odd;
      for (const Op& o : o4) { wide.push_back(o.d); odd.push_back(o.d); }
      wide[1].N = wide[1].CO = wide[1].OC = 40; wide[1].Npad = 64;
      odd[2].CI = 6; odd[2].K = odd[2].TY * odd[2].TX * 6;
      for (int mode = 0; mode < 2; ++mode) { hand.ops(mode, wide, {0, 0, 0, 0}); hand.ops(mode, odd, {0, 0, 0, 0}); }
    }
    if (argc > 3) {
      ModelDesc fm;
      append_h5_whole(fm, argv[3]);
      fm.infer_shapes();
      family_sections(fm);
      PlanDump("family.").graph(fm);
    }
    std::printf("\n]}\n");
  } catch (const FileError& e) {
    std::fprintf(stderr, "pack_digest: %s\n", e.msg.c_str());
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pack_digest: %s\n", e.what());
    return 1;
  }
  return 0;
}
