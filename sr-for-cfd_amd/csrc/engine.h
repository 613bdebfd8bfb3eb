// Internal engine types (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "gemm32_plan.h"
#include "kernels.h"
#include "model.h"
#include "operand_pack.h"
#include "switches.h"

namespace srcfd {

extern thread_local std::string g_last_error;
void set_error(const std::string& m);

// a failed HIP call of a function that returns a status: message into the thread's last error, SRCFD_EHIP out
#define HIPCHECK(expr)                                                               \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      srcfd::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));    \
      return SRCFD_EHIP;                                                             \
    }                                                                                \
  } while (0)

}  // namespace srcfd
#include "device_mem.h"
namespace srcfd {

struct ProfEvent {
  Event a, b;
  std::string name;
};

struct Lowp16State;  // bf16/f16 path of this handle's graph: the fused encoder_10 + decoder_400 kernels or any16 (fused_bf16.hip)
void lowp16_free(Lowp16State* st);

// What the last forward of a handle ran (srcfd_model_last_plan): the switches it saw, the tail segmentation that was launched and how
// the launches were issued.
struct Plan {
  Switches sw;
  int precision = 0;
  int tail_seg = 0;   // 16-bit tail: segments per sample actually launched (last chunk)
  int graph = 0;      // 0 plain launches, 1 captured now and launched as a graph, 2 replay of an earlier capture
  bool fused = false;
  bool any16 = false;  // the 16-bit forward ran the any16 graph (decoder=any16)
};

// One step of the f32-grade forward (Model::f32_step): the kernel that takes ops [i, i + count) at a given batch, precision and switches.
enum class F32Kernel { Tail32, Triple, Pair, X3Group, Big, Group, Skinny, Finalize, Mfma, Naive };
struct F32Step {
  F32Kernel k;
  int count;
  bool x3_tail;   // Tail32: its first two layers on the split-bf16 MFMAs
};
// Device operands of up to four ops (the output phases of one layer): f32 weights, split-bf16 planes (or null), biases
struct F32Operands {
  const float* B[4];
  const uint16_t* Bx[4];
  const float* bias[4];
};

struct Model {
  ModelDesc desc;
  int device = -1;
  int precision = SRCFD_PREC_FP32;
  bool has_fused = false;

  std::vector<Op> ops;
  std::vector<float> pack;  // host copy of packed weights
  // ops[pair_op], ops[pair_op + 1]: two kernel == stride == 2 transposed convolutions (32 -> 16 -> 8 channels) that run as
  // one kernel (kernels.h, PairDesc); -1: none.  Offsets into `pack`.
  int pair_op = -1;
  PairPack pair;
  // ops[triple_op .. +2]: the same with a 64 -> 32 layer in front (kernels.h, TripleDesc); takes precedence over the pair
  int triple_op = -1;
  TriplePack tri;
  // ops[tail32_op .. +3]: that chain followed by the network's last layer, a 3x3 SAME conv 8 -> 1 (kernels.h, Tail32Params):
  // one streaming kernel; takes precedence over the triple
  int tail32_op = -1;
  // ops[0..3] = conv2d (1->64, s2) -> conv2d_1 (64->128 on 5x5) -> dense (3200->128) -> latent (128->nl) run as one launch (kernels.h, Enc32Params)
  bool enc32_ok = false;
  size_t enc32_w2 = 0;     // conv2d_1 A fragments in `pack`
  Tail32Pack t32;
  int num_cus = 256;
  DevBuf<float> d_pack;
  // SRCFD_PREC_FP32X3: ops the split-bf16 GEMM takes (kernels_x3.hip): x3_off[i] = offset of op i's three weight planes in pack_x3
  // (elements), or -1.  Built at create, uploaded with the f32 pack.
  std::vector<int64_t> x3_off;
  int64_t t32_w1x = -1, t32_w2x = -1;   // the streaming tail's first- and second-layer fragments in pack_x3 (kernels.h, Tail32Params::w1x / w2x), or -1
  std::vector<uint16_t> pack_x3;
  DevBuf<uint16_t> d_pack_x3;

  DevBuf<float> buf[2];
  int ws_chunk = 0;
  size_t ws_per_sample = 0;   // elements per sample the two buffers were sized for (depends on the precision)
  DevBuf<float> d_splitk;  // split-K slabs of the skinny f32 GEMMs
  DevBuf<double> d_solver_state;  // (3, nx+2, ny+2) + row profiles of the solver hand-off
  DevBuf<float> d_x_stage;
  DevBuf<float> d_y_stage;    // host-buffer entry: result of the chunk being computed ...
  DevBuf<float> d_y_stage2;   // ... and of the chunk being copied out (page-locked destinations: copy and compute overlap)
  DevBuf<float> d_aff;
  int stage_chunk = 0;
  Event ev_computed[2], ev_copied[2];
  Stream copy_stream;
  DevBuf<unsigned long long> d_nonfinite;

  bool profiling = false;
  std::vector<ProfEvent> prof_events;
  size_t prof_used = 0;

  std::unique_ptr<Lowp16State, void (*)(Lowp16State*)> lowp16{nullptr, lowp16_free};   // non-null: the graph runs in bf16 / f16 (host-only handles included)
  bool lowp_ok() const { return lowp16 != nullptr; }

  // hipGraph replay of the fused 16-bit pipeline: a call whose arguments equal the previous call's is
  // captured once on a private stream and replayed afterwards (removes ~8 launch gaps per batch)
  struct GraphKey {
    const void* x = nullptr; const void* y = nullptr; const float* ain = nullptr; const float* aout = nullptr;
    unsigned long long* nf = nullptr; int n = -1, out_dtype = 0, flags = 0, precision = 0;
    unsigned switches = 0;   // Switches::bits(): the A/B switches select different kernels, so they belong to the key
    bool x3 = false;         // Model::x3_call: a remainder chunk of a large call and a small call of its own run different kernels at the same n
    bool operator==(const GraphKey& o) const {
      return x == o.x && y == o.y && ain == o.ain && aout == o.aout && nf == o.nf && n == o.n && out_dtype == o.out_dtype &&
             flags == o.flags && precision == o.precision && switches == o.switches && x3 == o.x3;
    }
  };
  GraphKey graph_key, last_key;
  Switches sw;            // of the call in progress
  bool x3_call = false;   // of the call in progress: x3_for(the n the caller passed); every chunk of the call follows it
  Plan plan, graph_plan;  // of the last forward / of the captured graph
  Stream graph_stream;
  GraphExec graph_exec;
  void drop_graph();

  ~Model();
  int init_device();
  // The f32-grade forward's kernel choice (engine.hip): the loop of forward_generic and the sizes of its buffers all ask f32_step
  size_t f32_first(int precision, const Switches& sw) const;   // 4: enc32 takes ops [0, 4) in front of the loop; else 0
  // SRCFD_PREC_FP32X3 runs the split-bf16 kernels from 64 samples PER CALL on: decided once from the n the caller passed
  // (srcfd_predict's, srcfd_predict_device's), never from a chunk's
  static constexpr int X3_MIN_CALL = 64;
  bool x3_for(int call_n, int precision) const { return precision == SRCFD_PREC_FP32X3 && !pack_x3.empty() && call_n >= X3_MIN_CALL; }
  F32Step f32_step(size_t i, int n, int precision, const Switches& sw, bool x3) const;   // n: the chunk's samples; x3: the call's x3_for
  void f32_span(size_t i, int count, int n, GemmDesc ds[4], F32Operands* w = nullptr) const;
  size_t max_act_elems(int precision, const Switches& sw) const;
  int chunk_cap(int precision, const Switches& sw) const;
  size_t splitk_need(int n, int precision, const Switches& sw, bool x3) const;
  int ensure_workspace(int n, const Switches& sw, bool x3);
  int launch(const char* name, hipStream_t s, const std::function<hipError_t()>& fn);
  int forward_generic(const float* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype, int flags,
                      unsigned long long* nonfinite, hipStream_t s);
  // call_n: the samples of the caller's whole call where these n are one chunk of it (predict_host, the scorer); 0: n is the call
  int predict_device(const void* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype, int flags,
                     unsigned long long* nonfinite, hipStream_t s, int call_n = 0);
  // sink (optional): consumes each chunk's device result [first, first+count) on the default stream instead of the copy into y;
  // a chunk is up to STAGE_SAMPLES samples then, as for a pageable y
  static constexpr int STAGE_SAMPLES = 256;
  int predict_host(const float* x, int n, const float* aff_in, const float* aff_out, float* y, int flags, int64_t* n_nonfinite,
                   const std::function<int(const float* y_dev, int first, int count)>& sink = nullptr);
};

// The bf16 / f16 path of a handle (fused_bf16.hip): the fused kernels of the encoder_10 + decoder_400 graph (Model::has_fused), or
// encoder_10 + any decoder of supported layers that ends in a 3x3 C -> 1 convolution (operand_pack.h, Any16Pack).
void lowp16_plan(Model& m);   // host only: plans the graph; leaves m.lowp16 null when no 16-bit path takes it
int lowp16_init(Model& m);    // device side of a planned graph
int lowp16_reserve(Model& m, int n);
size_t lowp16_workspace_bytes(const Model& m, int n);   // what lowp16_reserve(n) allocates for activations and split-K slabs
int lowp16_chunk_cap(const Model& m);                   // samples per chunk of the 16-bit forward: 1024, fewer where gemm16's 32-bit offsets ask for it
int lowp16_forward(Model& m, const float* x_dev, int n, const float* aff_in, const float* aff_out, void* y_dev, int out_dtype,
                   int flags, unsigned long long* nonfinite, hipStream_t s);
int fused_debug_read(Model& m, int index, void* dst, size_t bytes);   // the fused graph only

// The prediction behind the hand-offs into a solver state (resample.hip): `write` takes the n_samples predicted [and
// resampled] planes (ny, nx) on the device, float or double, on the default stream.
using SolverFieldSink = std::function<int(const void* fields, bool f64, int ny, int nx)>;
int predict_solver_fields(Model* mm, srcfd_resampler* r, const float* x, int n_samples, const float* in_affine, const float* out_affine,
                          const std::string& who, const char* owner, int want_nx, int want_ny, int flags, int64_t* n_nonfinite,
                          const SolverFieldSink& write);

// A resampler as the fine solver's hand-off from device fields sees it (resample.hip): input (in_h, in_w) -> output (out_h, out_w)
// on `device`, and n planes of float or double resampled on `s` into the handle's own scratch, *out (n, out_h, out_w) float64.
struct ResamplerGeometry {
  int device, in_h, in_w, out_h, out_w;
};
ResamplerGeometry resampler_geometry(const srcfd_resampler* r);
int resample_into_scratch(srcfd_resampler* r, const void* in_dev, bool f64, int n, hipStream_t s, const double** out);

}  // namespace srcfd
