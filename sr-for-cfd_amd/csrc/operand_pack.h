// Host-side operand packing: every layout a kernel reads its weights in, as pure functions from the layer graph to host vectors
// and offsets.  These layouts are the contract between host and kernel.  No HIP runtime calls in this unit: engine.hip (plan_*),
// fused_bf16.hip (lowp16_plan, build_pack: both 16-bit graphs through plan16 / pack_wt16 / pack_enc16; what a chunk of either
// launches is the sister unit lowp16_plan.h's, from the Plan16 made here), train_tail.hip
// (train_tail_plan) and train.hip (trainer_build) decide what qualifies and upload what these functions return.  The trainer's
// launch arithmetic lives here too: the grid of every weight-gradient launch, the table of the step's one slab-sum launch and the
// slab space it needs (plan_step, plan_slab_space); trainer_build sizes from it, trainer_step issues from it.
// tools/pack_digest.cpp links the same functions on a CPU; tests/test_operand_pack.py pins the packs' bytes, tests/test_train_plan.py
// checks the step plan against an independent statement of it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "train_tail.h"

namespace srcfd {

constexpr double LOG2E = 1.4426950408889634;   // swish layers produce log2(e) x (kernels_tail32.hip, swish_l2e)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
template <class T> void align64(std::vector<T>& v) { v.resize((v.size() + 63) / 64 * 64, T(0)); }   // 64-element aligned sections
inline int rowof(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // 32x32 accumulator row of register r in lane half h
uint16_t to_bf16(float f);   // round to nearest even, NaN stays NaN
uint16_t to_f16(float f);
inline uint16_t to16(float f, bool f16) { return f16 ? to_f16(f) : to_bf16(f); }
// f32 -> three bf16 terms (hi, mid, lo) by truncation; the two subtractions are exact
void split3(float w, uint16_t (&o)[3]);
// B[K][Npad] f32 -> Wt[plane 3][N][Kpad] bf16 (kernels_x3.hip, gemm_x3_split_weights)
void split_planes(const float* B, int K, int N, int Npad, int Kpad, uint16_t* out);

// ---- f32 engine: Model::pack ----
struct Op {
  GemmDesc d;                   // M filled per call (rows per image * batch)
  size_t w_off = 0, b_off = 0;  // into the packed float buffer: B[K][Npad], bias[Npad]
  int layer = 0;                // index into ModelDesc::layers
  std::string name;
};
void build_plan(const ModelDesc& desc, std::vector<Op>& ops, std::vector<float>& pack);

// Offsets of the fused f32 kernels' operands, appended to the pack in 64-float aligned sections (layouts: operand_pack.cpp)
struct PairPack { size_t wa = 0, ba = 0, wb = 0, bb = 0; };
struct TriplePack { size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0, w3 = 0, b3 = 0; };
struct Tail32Pack { size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0, w3 = 0, b3 = 0, wc = 0; };
PairPack pack_convt_pair(std::vector<float>& pk, const Layer& La, const Layer& Lb);
TriplePack pack_convt_triple(std::vector<float>& pk, const Layer& L1, const Layer& L2, const Layer& L3);
Tail32Pack pack_tail32(std::vector<float>& pk, const Layer& L1, const Layer& L2, const Layer& L3, const Layer& LO);
size_t pack_enc32(std::vector<float>& pk, const Layer& conv2d_1);
// tail32<X3>: the first two layers' fragments as three bf16 planes, appended to pack_x3
void pack_tail32_x3(std::vector<uint16_t>& px, const Layer& L1, const Layer& L2, int64_t& w1x, int64_t& w2x);

// One slot of the streaming tail's operands: which parameter of its four layers (flat order, TT_O_*; -1: padding, value 0) times
// which factor.  Inference materialises the slots from the weights, the trainer turns the same slots into its gather map + scale.
enum Scale : uint8_t { SC_ONE, SC_LOG2E, SC_INV_LOG2E };
struct Slot { int src; Scale sc; };
Tail32Pack tail32_slots(std::vector<Slot>& s);
// map / scale / offsets of TrainTailPlan for a tail whose first parameter has flat index param_off
void train_tail_slots(size_t param_off, TrainTailPlan& plan);

// ---- bf16 / f16 path (fused_bf16.hip): two graphs, one front end, one chunk plan (lowp16_plan.h) ----
// fused: encoder_10 + decoder_400 (enc16 -> dense1_16 -> mid16 -> tail16).  any16: encoder_10 + the other family decoders
// (enc16 -> per layer gemm16, or the narrow-channel GEMM of kernels_any16.hip for CI 16 / 32 -> outconv16).  Both store swish
// outputs scaled by log2e and fold 1 / log2e into the consumer's weights; both share plan16 / pack_wt16 / pack_enc16 below.
struct Op16 {
  GemmDesc d;
  size_t w_off = 0, b_off = 0;  // elements into the Wt vector of pack_wt16, floats into Plan16::f32
  int Kpad = 0;                 // row pitch of Wt
  int layer = 0, src = 0;       // compute-layer ordinal; index of the f32 op it was made from
  std::string name;
};
struct Plan16 {             // what both graphs plan once, for both operand types (plan16)
  std::vector<int> cl;      // indices of the compute layers in ModelDesc::layers
  std::vector<Op16> ops;    // GEMM ops of compute layers 1 .. last
  std::vector<float> f32;   // conv1 weights [9][64] + bias [64] (scaled), per-op biases [Npad] (scaled)
  size_t c1w_off = 0, c1b_off = 0;
};
struct Enc16Host {          // enc16's operands of one type (pack_enc16)
  std::vector<uint16_t> encf;               // conv2d_1, dense, latent_vector fragments (one blob)
  size_t enc_wd_off = 0, enc_wl_off = 0;    // byte offsets of the dense / latent fragments in encf
  std::vector<float> encb;                  // conv2d_1 bias fragments [128]
};
// cl, the scaled conv1 and the Op16 list of compute layers 1 .. last: latent padded to 64 channels, biases scaled and 4-float
// aligned, Npad / Kpad = multiples of 64, or 32 / K for a narrow op (any16_narrow) where `narrow_ok`
void plan16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, int last, bool narrow_ok, Plan16& P);
// GEMM weights of every op, transposed and scaled: Wt[Npad][Kpad], 8-element aligned; sets P.ops[].w_off (the same for both types)
void pack_wt16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& P, bool f16, std::vector<uint16_t>& w);
// ops 0..2 of w (conv2d_1, dense, latent_vector) in MFMA fragment order + conv2d_1's bias as accumulator init
void pack_enc16(const Plan16& P, const std::vector<uint16_t>& w, Enc16Host& E);
inline bool any16_narrow(const GemmDesc& d) { return d.CI % 64 != 0; }

// the fused graph (plan16 with last = 6, no narrow ops), one per operand type; the device copies are fused_bf16.hip's Dev16 (w and
// the enc16 part) and FusedState::Dev (the rest)
struct Pack16Host : Enc16Host {
  std::vector<uint16_t> w;              // pack_wt16
  std::vector<uint16_t> w2f, w0t, w1f;  // tail ConvT#2; mid16 ConvT#0 LDS images per phase, ConvT#1
  size_t w0t_off[4] = {0, 0, 0, 0};
  std::vector<uint8_t> consts;          // tail constants (kernels16.h, TC_OFF_*)
  std::vector<float> midb;              // mid16 bias fragments b0f [128] | b1f [64]
};
// the enc16 fragments only when `enc` (FusedState::enc_ok)
void pack_fused16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& fs, bool enc, bool f16, Pack16Host& P);

struct Any16Pack {           // what any16_plan finds besides the Plan16
  bool ok = false;           // the graph is eligible; `why` says what is not (the Plan16 is then empty)
  std::string why;
  int out_C = 0, out_H = 0, out_W = 0;   // the output convolution: 3x3 SAME, C -> 1
  float out_bias = 0.f;
  size_t max_act = 0;        // largest 16-bit activation per sample, elements
};
struct Any16Host : Enc16Host {   // one per operand type
  std::vector<uint16_t> w;       // pack_wt16
  std::vector<float> wout;       // output convolution (ty, tx, ci): the 16-bit-rounded weights (x 1 / log2e behind a swish) as f32
};
void any16_plan(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& P, Any16Pack& A);
void pack_any16(const ModelDesc& md, const std::vector<Op>& ops, const std::vector<float>& pack, Plan16& A, bool f16, Any16Host& P);

// ---- trainer (train.hip) ----
// a compute layer: its index in ModelDesc::layers, elements per sample, flat parameter offsets
struct LayerInfo { int desc_index; size_t in_elems, out_elems; bool swish; size_t kernel_off, bias_off; };
struct DgradOp { GemmDesc d; size_t w_off; int layer; };   // w_off into the packed dgrad buffer; layer: compute layer whose INPUT gradient this produces
// Replaces every weight by (its flat index + 1) as a float: running the ordinary packers on this
// "index model" yields, for each packed slot, which parameter lands there (0 = padding).
ModelDesc index_model(const ModelDesc& src, std::vector<LayerInfo>& layers, int64_t& n_params, std::vector<float>& init);
// dgrad descriptors + packed operands (values taken from `md`, which may be the index model)
void build_dgrad(const ModelDesc& md, const std::vector<LayerInfo>& layers, std::vector<DgradOp>& dops, std::vector<float>& pack);
// weight-gradient map of one forward op: rows 0..K-1 = operand rows, row K = bias; flat param index + 1 (0: padding)
std::vector<int> wgrad_gmap(const Op& op, const std::vector<float>& ipack);
// The trainer's gather map [forward operands | data-gradient operands | the fused tail's slots], every part 64-aligned
struct GatherMap { std::vector<int> map; size_t dpack_off = 0, dpack_elems = 0, tail_off = 0; };
GatherMap gather_map(const std::vector<float>& ipack, const std::vector<float>& dpack, const std::vector<int>* tail_map);

// ---- trainer: a step's weight-gradient launches and slab sums (kernels: train.hip wgrad_f32, wgrad_n1_k72_f32, wgrad_finish_all_f32) ----
// a forward GEMM of the step: descriptor (act forced linear, M filled per call), offsets into the packed forward buffer, compute-layer ordinal
struct TrainOp { GemmDesc fwd; size_t w_off, b_off; int layer; };
std::vector<TrainOp> train_ops(const std::vector<Op>& iops, const std::vector<LayerInfo>& layers);
// end of the run of ops that share ops[i].layer: the output phases of a strided transposed convolution, at most four (trainer_build)
template <class T> size_t layer_end(const std::vector<T>& ops, size_t i) {
  size_t j = i;
  while (j < ops.size() && ops[j].layer == ops[i].layer) ++j;
  return j;
}
constexpr int WG_RC = 64;   // rows of one chunk of wgrad_f32
// grid of one weight-gradient launch; KG == 0: wgrad_n1_k72_f32, one slab per workgroup.  rps: rows per slice (slab)
struct WgradPlan { int KG, NG, kblocks, nblocks, ktiles, ntiles, nslices, rps; };
bool wgrad_is_n1_k72(const GemmDesc& d);
WgradPlan wgrad_plan(const GemmDesc& d);   // d.M set
// slab groups one workgroup of wgrad_finish_all_f32 adds side by side, from the slab count
inline int finish_groups(int nslices) { return nslices >= 256 ? 32 : (nslices >= 64 ? 8 : (nslices >= 8 ? 4 : 1)); }
constexpr int MAX_FINISH_OPS = 24;   // slots of the slab-sum table, a kernel argument
// One slot of the table.  The first op of a layer sums the bias rows of the others (`extra`: their slots, op order), which skip theirs.
struct SlabSum {
  int op;            // index into the ops; -1: the fused tail's slabs (one column of TT_PARAMS slots, no bias row)
  WgradPlan wp;      // of that op at this batch
  int64_t elems;     // floats of one slab: (K + 1) x Npad
  int nslices, groups, block0;   // block0: first workgroup of this slot in the one launch
  int bias_skip, nextra, extra[3];
};
// The slab sums of a step on n samples, in table order: the fused tail's `tail_slabs` slabs if any (0: no fused tail), then the
// layers Lg - 1 .. 0 that run layer by layer, each layer's ops in op order.  block0 ascends: the kernel finds its slot by it.
// Which stream launches a layer's weight gradients (SRCFD_TRAIN_AUX_FROM) does not enter: either way the layers are visited from
// the last down.  trainer_build refuses graphs with more than four ops in a layer or more slots than MAX_FINISH_OPS.
struct StepPlan { std::vector<SlabSum> sums; int blocks = 0; std::vector<size_t> part_floats; };   // workgroups in all; per op, the floats of its slabs
StepPlan plan_step(const std::vector<TrainOp>& ops, int Lg, int n, int tail_slabs);
// Every op's own slab space (64-float aligned offsets): the most it needs at any batch 1 .. max_batch -- the slab count is not
// monotonic in the batch (ConvT#4 of decoder_400: 313, 417, 469, 500, 447, 469, 487, 500 slabs at 1 .. 8 samples)
struct SlabSpace { std::vector<size_t> off, cap; size_t total = 0; };
SlabSpace plan_slab_space(const std::vector<TrainOp>& ops, int Lg, int max_batch);

}  // namespace srcfd
