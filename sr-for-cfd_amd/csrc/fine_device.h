// Device-side pieces that the single-case fine-mesh solver (fine_solver.hip) and the batched one (fine_batch.hip) share: the
// per-case view of the fields, the status block, the fixed-order reductions and the indexed reads.  Both solvers reduce with
// block_sum / sum_partials below and nothing else, which is what makes a case's bits the same in either.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace srcfd {
namespace {

constexpr int NT = 256;            // threads per workgroup; one workgroup per mesh row i
constexpr int SWEEP_CAP = 1000;    // inner sweeps per solve (PyCFD_ML_accelerated.py:251, 299)
constexpr double INNER_TOL = 1e-6;

struct Status {      // written by the kernels with plain stores, read by the host once per chunk
  int m_sweeps, m_stop;    // current momentum solve: sweeps executed, exit rule fired
  int p_sweeps, p_stop;    // current pressure solve
  int converged, nonfinite;
  int state;               // batched solver only (fine_batch.hip): SRCFD_CASE_*, a case that is not RUNNING is frozen
  int pad;
  double rms[3];
};

struct Dev {
  int nx, ny, sx, sy;
  double dx, dy, volp, dt, rho, nu;
  double *Var, *Old, *Ff, *Jb, *rhs, *part;
  Status* st;
};
// partials: [0, 2nx) momentum, by sweep parity; [2nx, 6nx) pressure, [parity][colour][row]; [6nx, 9nx) outer residuals [k][row]
__device__ __forceinline__ double* mom_part(const Dev& g, int parity) { return g.part + (size_t)parity * g.nx; }
__device__ __forceinline__ double* p_part(const Dev& g, int parity) { return g.part + (size_t)(2 + 2 * parity) * g.nx; }
__device__ __forceinline__ double* res_part(const Dev& g) { return g.part + (size_t)6 * g.nx; }

// Fixed-order workgroup sum: thread t's own sequential sum v, then a halving tree lds[t] += lds[t + s], s = 128 .. 1.
__device__ double block_sum(double v, double* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}
// Sum of n partials: thread t adds p[t], p[t + 256], ... in order, then block_sum.
__device__ double sum_partials(const double* p, int n, double* lds) {
  double a = 0.0;
  for (int q = threadIdx.x; q < n; q += NT) a = a + p[q];
  return block_sum(a, lds);
}
__device__ __forceinline__ int uniform_flag(const int* f, int* lds_flag) {
  if (threadIdx.x == 0) *lds_flag = *(const volatile int*)f;
  __syncthreads();
  const int v = *lds_flag;
  __syncthreads();
  return v;
}

__device__ __forceinline__ double at(const Dev& g, const double* A, int k, int i, int j) { return A[(size_t)k * g.sx + (size_t)i * g.sy + j]; }
// Grid::vw: negative indices wrap per axis, indices past the end run on in the flat (3, nx+2, ny+2) array, clamped at its end
__device__ __forceinline__ double atw(const Dev& g, const double* A, int k, int i, int j) {
  if (i < 0) i += g.nx + 2;
  if (j < 0) j += g.ny + 2;
  size_t idx = (size_t)k * g.sx + (size_t)i * g.sy + j;
  const size_t n = (size_t)3 * g.sx;
  if (idx >= n) idx = n - 1;
  return A[idx];
}

struct Bc {
  int type[4];
  double value[4];
  int bfs;
  double step_h, h, Ub;
};

}  // namespace
}  // namespace srcfd
