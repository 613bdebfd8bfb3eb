// Scoring of predictions against targets on the device (gfx950): per sample MAE, MSE, max |error|, the ranges of truth and
// prediction and the count of non-finite errors, every one with the bits numpy gives for the notebook's expressions
// (`evaluate_for_re`, sr-ae-conv.ipynb:c323-369; include/srcfd.h, "scoring").
//
// The two means are float32 sums in numpy's order: chunks of 8192 elements, each a pairwise tree over leaves of <= 128 elements
// that eight accumulators sum, the chunk sums chained from 0.f.  The order is built on the host (score_plan.h) and read here as a
// table; nothing in this file decides an order of additions except the eight-accumulator leaf.
//
// One workgroup of 1024 threads per sample, one launch, no scratch memory.  Per chunk:
//   A  all threads: coalesced loads of prediction and truth (16 bytes per lane where the field allows it), inverse standardise
//      (two roundings each: multiply, then add), d = t - p into LDS; min / max / non-finite bookkeeping in registers
//   B  eight lanes per leaf hold numpy's r[0..7]: lanes 0..511 sum |d| over the chunk's leaves, lanes 512..1023 sum d * d
//      (a full chunk has 64 leaves: every lane is busy); the eight are combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) by three
//      butterfly steps, the leaf's last len % 8 elements are added in order; leaf sums into LDS
//   C  one wave per sum walks the tree level by level in LDS and stores the chunk's sum; the other waves are already loading the
//      next chunk (two workgroup barriers per chunk)
// then one lane per sum chains the chunk sums from 0.f and divides by (float)elems.
// LDS: d of one chunk (8192 floats, every 128 shifted by 8 banks so that the eight-lane groups of a wave read distinct banks),
// the two tables, the tree nodes and the chunk sums: 46 KB, two workgroups per CU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "score_plan.h"

namespace srcfd {

constexpr int SCORE_THREADS = 1024;
constexpr int SCORE_STAGE = SCORE_CHUNK + SCORE_CHUNK / 128 * 8;                   // padded floats of one staged chunk
constexpr int SCORE_MAX_CHUNKS = (int)((SCORE_MAX_ELEMS + SCORE_CHUNK - 1) / SCORE_CHUNK);   // 313
constexpr int SCORE_TABLE_INTS = (int)(sizeof(ScoreTable) / sizeof(int));
static_assert(sizeof(ScoreTable) % sizeof(int) == 0, "the table is copied to LDS as ints");
static_assert(SCORE_MAX_CHUNKS <= 320, "chunk sums in LDS");

__device__ __forceinline__ int score_pad(int i) { return i + ((i >> 7) << 3); }

// LDS traffic of ONE wave is executed in order; this only keeps the compiler from moving accesses across the point
__device__ __forceinline__ void score_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what a thread keeps of the elements it has seen; min / max ignore NaN (v_min_f32 / v_max_f32) and the flags bring it back at the
// end, as np.min / np.max return NaN whenever one is present
struct ScoreRange {
  float tmin, tmax, pmin, pmax, amax;
  unsigned nonfinite;
  unsigned nan;   // bit 0: a NaN in d, bit 1: in t, bit 2: in p
};

__device__ __forceinline__ float score_element(float pv, float tv, bool has_pa, float pm, float ps, bool has_ta, float tm, float ts,
                                               ScoreRange& r) {
  // inverse_standardize: arr * std + mean in float32, two roundings, never an fma
  const float p = has_pa ? __fadd_rn(__fmul_rn(pv, ps), pm) : pv;
  const float t = has_ta ? __fadd_rn(__fmul_rn(tv, ts), tm) : tv;
  const float d = __fsub_rn(t, p);
  r.nonfinite += (__float_as_uint(d) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
  r.nan |= (d != d ? 1u : 0u) | (t != t ? 2u : 0u) | (p != p ? 4u : 0u);
  r.amax = fmaxf(r.amax, fabsf(d));
  r.tmin = fminf(r.tmin, t);
  r.tmax = fmaxf(r.tmax, t);
  r.pmin = fminf(r.pmin, p);
  r.pmax = fmaxf(r.pmax, p);
  return d;
}

__global__ void __launch_bounds__(SCORE_THREADS) score_fields_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                                      int64_t elems, const float* __restrict__ pred_affine,
                                                                      const float* __restrict__ truth_affine,
                                                                      const ScoreTable* __restrict__ tables, float* __restrict__ metrics) {
  __shared__ __attribute__((aligned(16))) float stage[SCORE_STAGE];
  __shared__ int tab_raw[2][SCORE_TABLE_INTS];
  __shared__ float node[2][SCORE_MAX_NODES];
  __shared__ float chunk_sum[2][320];
  __shared__ float red[5][SCORE_THREADS / 64];
  __shared__ unsigned s_nonfinite, s_nan;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t sample = blockIdx.x;
  const float* P = pred + sample * elems;
  const float* T = truth + sample * elems;
  const bool has_pa = pred_affine != nullptr, has_ta = truth_affine != nullptr;
  const float pm = has_pa ? pred_affine[2 * sample] : 0.f, ps = has_pa ? pred_affine[2 * sample + 1] : 1.f;
  const float tm = has_ta ? truth_affine[2 * sample] : 0.f, ts = has_ta ? truth_affine[2 * sample + 1] : 1.f;

  {
    const int* src = reinterpret_cast<const int*>(tables);
    int* dst = &tab_raw[0][0];
    for (int i = tid; i < 2 * SCORE_TABLE_INTS; i += SCORE_THREADS) dst[i] = src[i];
    if (tid == 0) { s_nonfinite = 0; s_nan = 0; }
  }
  __syncthreads();
  const ScoreTable* tab = reinterpret_cast<const ScoreTable*>(&tab_raw[0][0]);   // [0]: a chunk of 8192, [1]: the last, shorter one

  const float inf = __uint_as_float(0x7f800000u);
  ScoreRange rg{inf, -inf, inf, -inf, -inf, 0u, 0u};
  const bool vec = (elems & 3) == 0 && ((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(T)) & 15) == 0;
  const int n_chunks = (int)((elems + SCORE_CHUNK - 1) / SCORE_CHUNK);
  const int group = tid >> 3, j = tid & 7;     // eight lanes per leaf
  const int which = group >> 6;                // 0: sum of |d| (lanes 0..511), 1: sum of d * d (lanes 512..1023)

  for (int c = 0; c < n_chunks; ++c) {
    const int64_t base = (int64_t)c * SCORE_CHUNK;
    const int len = elems - base < SCORE_CHUNK ? (int)(elems - base) : SCORE_CHUNK;
    const ScoreTable& tb = tab[len == SCORE_CHUNK ? 0 : 1];

    // A: d = t - p of the chunk into LDS
    if (vec) {
      const float4* P4 = reinterpret_cast<const float4*>(P + base);
      const float4* T4 = reinterpret_cast<const float4*>(T + base);
      for (int k = tid; k < (len >> 2); k += SCORE_THREADS) {
        const float4 pv = P4[k], tv = T4[k];
        float4 d;
        d.x = score_element(pv.x, tv.x, has_pa, pm, ps, has_ta, tm, ts, rg);
        d.y = score_element(pv.y, tv.y, has_pa, pm, ps, has_ta, tm, ts, rg);
        d.z = score_element(pv.z, tv.z, has_pa, pm, ps, has_ta, tm, ts, rg);
        d.w = score_element(pv.w, tv.w, has_pa, pm, ps, has_ta, tm, ts, rg);
        *reinterpret_cast<float4*>(&stage[score_pad(4 * k)]) = d;   // 4k .. 4k + 3 lie in one run of 128
      }
    } else {
      for (int k = tid; k < len; k += SCORE_THREADS)
        stage[score_pad(k)] = score_element(P[base + k], T[base + k], has_pa, pm, ps, has_ta, tm, ts, rg);
    }
    __syncthreads();

    // B: leaf sums.  Every lane runs every round (the butterfly reads its seven neighbours); a group without a leaf adds zeros.
    for (int first = 0; first < tb.n_leaves; first += 64) {
      const int leaf = first + (group & 63);
      const bool live = leaf < tb.n_leaves;
      const int off = live ? tb.leaf_off[leaf] : 0, ln = live ? tb.leaf_len[leaf] : 0;
      auto value = [&](int i) {
        const float d = stage[score_pad(off + i)];
        return which ? __fmul_rn(d, d) : fabsf(d);
      };
      const int body = ln - (ln & 7);      // numpy: the accumulators take [0, n - n % 8)
      float r = 0.f;
      if (ln >= 8) {
        r = value(j);
        for (int i = 8; i < body; i += 8) r = __fadd_rn(r, value(i + j));
      }
      r = __fadd_rn(r, __shfl_xor(r, 1));  // lane 0 of the group: r0 + r1
      r = __fadd_rn(r, __shfl_xor(r, 2));  //   (r0 + r1) + (r2 + r3)
      r = __fadd_rn(r, __shfl_xor(r, 4));  //   ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
      if (live && j == 0) {
        float res = r;
        int i = body;
        if (ln < 8) { res = 0.f; i = 0; }  // numpy: a serial sum from 0.f
        for (; i < ln; ++i) res = __fadd_rn(res, value(i));
        node[which][leaf] = res;
      }
    }
    __syncthreads();

    // C: the tree, one wave per sum
    if (wave == 0 || wave == SCORE_THREADS / 128) {
      const int w = wave ? 1 : 0;
      volatile float* nd = node[w];
      for (int h = 1; h < tb.n_levels; ++h) {
        for (int i = tb.level_start[h] + lane; i < tb.level_start[h + 1]; i += 64) nd[i] = __fadd_rn(nd[tb.left[i]], nd[tb.right[i]]);
        score_wave_sync();
      }
      if (lane == 0) chunk_sum[w][c] = nd[tb.n_nodes - 1];
    }
    // no barrier: the next chunk's barrier A -> B orders this wave's tree before the next leaf sums, and every wave has left B
    // before any wave overwrites `stage`
  }

  // the ranges: butterfly over the wave, then over the waves through LDS
  for (int m = 1; m < 64; m <<= 1) {
    rg.tmin = fminf(rg.tmin, __shfl_xor(rg.tmin, m));
    rg.tmax = fmaxf(rg.tmax, __shfl_xor(rg.tmax, m));
    rg.pmin = fminf(rg.pmin, __shfl_xor(rg.pmin, m));
    rg.pmax = fmaxf(rg.pmax, __shfl_xor(rg.pmax, m));
    rg.amax = fmaxf(rg.amax, __shfl_xor(rg.amax, m));
  }
  if (lane == 0) { red[0][wave] = rg.tmin; red[1][wave] = rg.tmax; red[2][wave] = rg.pmin; red[3][wave] = rg.pmax; red[4][wave] = rg.amax; }
  if (rg.nonfinite) atomicAdd(&s_nonfinite, rg.nonfinite);
  if (rg.nan) atomicOr(&s_nan, rg.nan);
  __syncthreads();

  float* out = metrics + sample * SRCFD_SCORE_FIELDS;
  const float qnan = __uint_as_float(0x7fc00000u);
  if (tid == 0 || tid == 64) {
    // step 3 and 4 of numpy's mean: res = 0.f; res += chunk sums in order; res / (float)elems
    const int w = tid ? 1 : 0;
    float res = 0.f;
    for (int c = 0; c < n_chunks; ++c) res = __fadd_rn(res, chunk_sum[w][c]);
    out[w ? SRCFD_SCORE_MSE : SRCFD_SCORE_MAE] = __fdiv_rn(res, (float)elems);
  }
  if (tid == 128) {
    float v[5];
    for (int k = 0; k < 5; ++k) v[k] = red[k][0];
    for (int i = 1; i < SCORE_THREADS / 64; ++i) {
      v[0] = fminf(v[0], red[0][i]); v[1] = fmaxf(v[1], red[1][i]); v[2] = fminf(v[2], red[2][i]);
      v[3] = fmaxf(v[3], red[3][i]); v[4] = fmaxf(v[4], red[4][i]);
    }
    const unsigned nan = s_nan;
    out[SRCFD_SCORE_MAX_ABS] = (nan & 1u) ? qnan : v[4];
    out[SRCFD_SCORE_TRUTH_MIN] = (nan & 2u) ? qnan : v[0];
    out[SRCFD_SCORE_TRUTH_MAX] = (nan & 2u) ? qnan : v[1];
    out[SRCFD_SCORE_PRED_MIN] = (nan & 4u) ? qnan : v[2];
    out[SRCFD_SCORE_PRED_MAX] = (nan & 4u) ? qnan : v[3];
    out[SRCFD_SCORE_NONFINITE] = (float)s_nonfinite;   // exact: elems <= 2^24
  }
}

// pred_dev / truth_dev (n, elems), affines (n, 2) or null, tables = {full, last} of score_plan(elems), metrics_dev (n, 8): all on the device
static int launch_score(const float* pred_dev, const float* truth_dev, int n, int64_t elems, const float* pred_aff, const float* truth_aff,
                        const ScoreTable* tables, float* metrics_dev, hipStream_t s) {
  if (n <= 0) return SRCFD_OK;
  hipLaunchKernelGGL(score_fields_kernel, dim3((unsigned)n), dim3(SCORE_THREADS), 0, s, pred_dev, truth_dev, elems, pred_aff, truth_aff, tables,
                     metrics_dev);
  HIPCHECK(hipGetLastError());
  return SRCFD_OK;
}

static int upload_tables(const ScorePlan& p, DevBuf<ScoreTable>& d_tab) {
  const ScoreTable both[2] = {p.full, p.last};
  return d_tab.upload(both, 2);
}

// srcfd_evalset: inputs, targets and affines of a held-out set, resident on one device
struct EvalSet {
  int device = 0;
  int n = 0;
  int64_t in_elems = 0, out_elems = 0;
  DevBuf<float> d_x, d_truth, d_in_aff, d_pred_aff, d_truth_aff;
  DevBuf<float> d_y;          // one chunk's predictions: min(n, Model::STAGE_SAMPLES) fields
  DevBuf<float> d_metrics;    // (n, SRCFD_SCORE_FIELDS)
  DevBuf<ScoreTable> d_tab;
  ~EvalSet() { (void)hipSetDevice(device); }   // for the members' destructors (device_mem.h)
};

}  // namespace srcfd

using srcfd::set_error;

extern "C" {

int srcfd_score_plan(int64_t elems, char* buf, size_t len) {
  return srcfd::abi_guard("srcfd_score_plan", [&]() -> int {
    if (!buf || !len) { set_error("srcfd_score_plan: bad arguments"); return SRCFD_EINVAL; }
    const std::string s = srcfd::score_plan_json(srcfd::score_plan(elems));
    if (s.size() + 1 > len) { set_error("srcfd_score_plan: buffer too small, " + std::to_string(s.size() + 1) + " bytes needed"); return SRCFD_EINVAL; }
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return SRCFD_OK;
  });
}

int srcfd_score_fields(int device, const float* pred, const float* truth, int n, int64_t elems, const float* pred_affine,
                       const float* truth_affine, float* metrics) {
  return srcfd::abi_guard("srcfd_score_fields", [&]() -> int {
    using namespace srcfd;
    if (n < 0 || (n > 0 && (!pred || !truth || !metrics))) { set_error("srcfd_score_fields: bad arguments"); return SRCFD_EINVAL; }
    const ScorePlan plan = score_plan(elems);   // refuses elems outside 1 .. SCORE_MAX_ELEMS
    if (n == 0) return SRCFD_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
      (void)hipGetLastError();
      set_error("srcfd_score_fields: no such HIP device");
      return SRCFD_ENODEV;
    }
    HIPCHECK(hipSetDevice(device));
    // staged like srcfd_predict: up to 2^25 floats (128 MiB) of each array per chunk
    const int chunk = (int)std::min<int64_t>(n, std::max<int64_t>(1, (int64_t(1) << 25) / elems));
    DevBuf<float> d_p, d_t, d_pa, d_ta, d_m;
    DevBuf<ScoreTable> d_tab;
    int rc = d_p.alloc((size_t)chunk * elems);
    if (!rc) rc = d_t.alloc((size_t)chunk * elems);
    if (!rc) rc = d_m.alloc((size_t)chunk * SRCFD_SCORE_FIELDS);
    if (!rc && pred_affine) rc = d_pa.alloc((size_t)chunk * 2);
    if (!rc && truth_affine) rc = d_ta.alloc((size_t)chunk * 2);
    if (!rc) rc = upload_tables(plan, d_tab);
    if (rc) return rc;
    for (int i = 0; i < n; i += chunk) {
      const int c = std::min(chunk, n - i);
      const size_t bytes = (size_t)c * elems * sizeof(float);
      HIPCHECK(hipMemcpyAsync(d_p.get(), pred + (size_t)i * elems, bytes, hipMemcpyHostToDevice, nullptr));
      HIPCHECK(hipMemcpyAsync(d_t.get(), truth + (size_t)i * elems, bytes, hipMemcpyHostToDevice, nullptr));
      if (pred_affine) HIPCHECK(hipMemcpyAsync(d_pa.get(), pred_affine + 2 * (size_t)i, (size_t)c * 2 * sizeof(float), hipMemcpyHostToDevice, nullptr));
      if (truth_affine) HIPCHECK(hipMemcpyAsync(d_ta.get(), truth_affine + 2 * (size_t)i, (size_t)c * 2 * sizeof(float), hipMemcpyHostToDevice, nullptr));
      rc = launch_score(d_p.get(), d_t.get(), c, elems, d_pa.get(), d_ta.get(), d_tab.get(), d_m.get(), nullptr);
      if (rc) return rc;
      HIPCHECK(hipMemcpyAsync(metrics + (size_t)i * SRCFD_SCORE_FIELDS, d_m.get(), (size_t)c * SRCFD_SCORE_FIELDS * sizeof(float), hipMemcpyDeviceToHost, nullptr));
      HIPCHECK(hipStreamSynchronize(nullptr));
    }
    return SRCFD_OK;
  });
}

int srcfd_evalset_create(int device, const float* x, int64_t in_elems, const float* truth, int64_t out_elems, int n, const float* in_affine,
                         const float* pred_affine, const float* truth_affine, srcfd_evalset** out) {
  return srcfd::abi_guard("srcfd_evalset_create", [&]() -> int {
    using namespace srcfd;
    if (!out) { set_error("srcfd_evalset_create: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    if (n < 0 || in_elems <= 0 || (n > 0 && (!x || !truth))) { set_error("srcfd_evalset_create: bad arguments"); return SRCFD_EINVAL; }
    const ScorePlan plan = score_plan(out_elems);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
      (void)hipGetLastError();
      set_error("srcfd_evalset_create: no such HIP device");
      return SRCFD_ENODEV;
    }
    HIPCHECK(hipSetDevice(device));
    std::unique_ptr<EvalSet> e(new EvalSet());
    e->device = device; e->n = n; e->in_elems = in_elems; e->out_elems = out_elems;
    int rc = e->d_x.upload(x, (size_t)n * in_elems);
    if (!rc) rc = e->d_truth.upload(truth, (size_t)n * out_elems);
    if (!rc && in_affine) rc = e->d_in_aff.upload(in_affine, (size_t)n * 2);
    if (!rc && pred_affine) rc = e->d_pred_aff.upload(pred_affine, (size_t)n * 2);
    if (!rc && truth_affine) rc = e->d_truth_aff.upload(truth_affine, (size_t)n * 2);
    if (!rc && n) rc = e->d_y.alloc((size_t)std::min(n, Model::STAGE_SAMPLES) * out_elems);
    if (!rc && n) rc = e->d_metrics.alloc((size_t)n * SRCFD_SCORE_FIELDS);
    if (!rc) rc = upload_tables(plan, e->d_tab);
    if (rc) return rc;
    *out = reinterpret_cast<srcfd_evalset*>(e.release());
    return SRCFD_OK;
  });
}

int srcfd_evalset_score(srcfd_evalset* e, srcfd_model* m, float* metrics) {
  return srcfd::abi_guard("srcfd_evalset_score", [&]() -> int {
    using namespace srcfd;
    if (!e || !m) { set_error("srcfd_evalset_score: null handle"); return SRCFD_EINVAL; }
    EvalSet& es = *reinterpret_cast<EvalSet*>(e);
    Model& mm = *reinterpret_cast<Model*>(m);
    if (es.n > 0 && !metrics) { set_error("srcfd_evalset_score: bad arguments"); return SRCFD_EINVAL; }
    if (mm.device < 0) { set_error("srcfd_evalset_score: host-only model handle"); return SRCFD_ENODEV; }
    const int* os = mm.desc.out_shape();
    const int64_t m_in = (int64_t)mm.desc.in_shape[0] * mm.desc.in_shape[1] * mm.desc.in_shape[2], m_out = (int64_t)os[0] * os[1] * os[2];
    if (m_in != es.in_elems || m_out != es.out_elems) {
      set_error("srcfd_evalset_score: the model maps " + std::to_string(m_in) + " -> " + std::to_string(m_out) + " elements per sample, the set holds " +
                std::to_string(es.in_elems) + " -> " + std::to_string(es.out_elems));
      return SRCFD_EINVAL;
    }
    if (mm.device != es.device) { set_error("srcfd_evalset_score: model and set are on different devices"); return SRCFD_EINVAL; }
    if (es.n == 0) return SRCFD_OK;
    HIPCHECK(hipSetDevice(es.device));
    // the chunks of srcfd_predict into pageable memory, so that a sample has the bits `predict` of the whole set gives it; the forward
    // standardises its input and nothing else: the scorer inverse-standardises prediction and truth (two roundings each)
    for (int i = 0; i < es.n; i += Model::STAGE_SAMPLES) {
      const int c = std::min(Model::STAGE_SAMPLES, es.n - i);
      int rc = mm.predict_device(es.d_x.get() + (size_t)i * es.in_elems, c, es.d_in_aff ? es.d_in_aff.get() + 2 * (size_t)i : nullptr, nullptr,
                                 es.d_y.get(), SRCFD_F32, 0, nullptr, nullptr, es.n);
      if (!rc) rc = launch_score(es.d_y.get(), es.d_truth.get() + (size_t)i * es.out_elems, c, es.out_elems,
                                 es.d_pred_aff ? es.d_pred_aff.get() + 2 * (size_t)i : nullptr,
                                 es.d_truth_aff ? es.d_truth_aff.get() + 2 * (size_t)i : nullptr, es.d_tab.get(),
                                 es.d_metrics.get() + (size_t)i * SRCFD_SCORE_FIELDS, nullptr);
      if (rc) return rc;
    }
    HIPCHECK(hipMemcpy(metrics, es.d_metrics.get(), (size_t)es.n * SRCFD_SCORE_FIELDS * sizeof(float), hipMemcpyDeviceToHost));
    return SRCFD_OK;
  });
}

int srcfd_evalset_destroy(srcfd_evalset* e) {
  return srcfd::abi_guard("srcfd_evalset_destroy", [&]() -> int {
    delete reinterpret_cast<srcfd::EvalSet*>(e);
    return SRCFD_OK;
  });
}

}  // extern "C"
