// The launch plan of the 16-bit forward (fused_bf16.hip): what a chunk of c samples of a graph launches -- every kernel in order, the
// ops it covers, the activation buffer it reads and the one it writes, and every batch-dependent number of the launch (M, the split-K
// cut and slab floats of gemm16, the grids, mid16's workgroup shape and per-phase workgroup counts, the tail's segmentation and
// workgroup count).  A pure function of the graph, the switches, c and the CU count: no HIP runtime calls, no kernel code, and no
// dependence on how large the caller's slab buffer is or on what the handle ran before (a launcher handed a split cut without slabs
// refuses).  fused_bf16.hip issues the steps and decides nothing; lowp16_reserve's slab buffer (lowp16_slab_elems) holds every plan.
// tools/pack_digest.cpp links this unit on a CPU; tests/test_lowp16_plan.py checks it against an independent statement of the rules
// (tests/lowp16_plan_ref.py).
#pragma once
#include <cstddef>
#include <vector>

#include "kernels.h"
#include "operand_pack.h"
#include "switches.h"

namespace srcfd {

// What the plan has to know about the kernels; each kernel file asserts its own constant against these.
constexpr int ENC_G = 5;                          // samples per workgroup of enc16
constexpr int DENSE1_NF = 144;                    // output features per workgroup of dense1_16
constexpr int GEMM16_BP = 128, GEMM16_BK = 64;    // rows of a block tile of gemm16, depth of its k tile
enum class MidShape { W4, W8, W16, W4x2, W8x2 };  // mid16's workgroup: waves [x 32-pixel tiles per wave]
constexpr int MID_PX[5] = {128, 256, 512, 256, 512};   // output pixels per workgroup: 32 x waves x tiles
constexpr int MID_PHASE_PX[4] = {169, 156, 156, 144};  // pixels per sample and output phase of ConvT#0 (13x13, 13x12, 12x13, 12x12)

// Dense with one 64-deep k tile and N a multiple of 144 (dense_1: 64 -> 36 864): one workgroup per 144 features, all samples
bool dense1_16_qualifies(const GemmDesc& d, int Kpad);

enum class Kernel16 { EncConv1, Enc, Dense1, Gemm, GemmN, Mid, Tail, TailS, OutConv };
constexpr int BUF_X = -1, BUF_Y = -2;   // Step16::src / dst: the call's input / output instead of activation buffer 0 / 1

// gemm16's launch.  splits > 1: the split-K kernel, nz slabs (M x Npad f32) of kslice k each, summed in slab order by the finish.
struct Gemm16Cut {
  int bn = 0, splits = 1, kslice = 0, nz = 1;
  unsigned grid[3] = {0, 0, 0};
  unsigned fin = 0;          // grid of the finish kernel; 0: none
  size_t slab_floats = 0;    // nz * M * Npad where split, else 0
};

struct Step16 {
  Kernel16 k;
  int op0 = 0, nops = 0;     // the ops [op0, op0 + nops) of Plan16::ops it covers (EncConv1, Tail, TailS, OutConv: layers outside the op list)
  int src = 0, dst = 0;
  GemmDesc d{};              // Dense1, Gemm, GemmN: the op's descriptor with M set
  Gemm16Cut cut;             // Gemm
  unsigned grid[2] = {0, 0}; // EncConv1, Enc, Dense1, GemmN, OutConv
  MidShape shape = MidShape::W4x2;   // Mid
  int nblk[4] = {0, 0, 0, 0};        // Mid: workgroups per output phase
  int seg = 0, blocks = 0;   // Tail, TailS
};

struct Graph16 {
  bool fused = false;        // encoder_10 + decoder_400 (enc16 -> dense1_16 -> mid16 -> tail16); else any16 (layer by layer -> outconv16)
  bool enc_ok = false;       // fused: the encoder has the shape enc16 is written for (any16_plan accepts no other)
  int out_H = 0, out_W = 0;  // any16: the output convolution's image
};

struct Chunk16Plan {
  std::vector<Step16> steps;
  int t1_buf = 0;            // fused: the activation buffer the tail reads (ConvT#1's output)
  int tail_seg = 0;          // fused: segments per sample the tail runs with
  size_t slab_floats = 0;    // the most any step needs
};
Chunk16Plan plan_chunk16(const Plan16& P, const Graph16& g, const Switches& sw, int c, int num_cus);

// The slab buffer a handle reserves for chunks of up to `chunk` samples: 16 K-slice slabs of dense's (chunk x 128) f32.  A split is
// planned only where its slabs fit the buffer reserved for the chunk itself (splits * M * Npad <= lowp16_slab_elems(c)), so the plan
// of a chunk never depends on a larger chunk the handle saw before.
inline size_t lowp16_slab_elems(size_t chunk) { return 16 * chunk * 128; }

}  // namespace srcfd
