// Batched fine-mesh solver: B cases of one mesh, scheme and case type in one set of launches (C ABI srcfd_fine_batch_*).
//
// A Reynolds sweep of the single-case solver (fine_solver.hip) leaves the device almost empty: one workgroup per mesh row and
// about 2 000 dependent launches per outer iteration, whose cost is the launch boundary and not the cell arithmetic.  The cases
// of a sweep share the mesh and the launch sequence, so here they share the launches: blockIdx.y is the case, and within a case
// every kernel keeps fine_solver.hip's thread-to-cell mapping, its expressions in their order and its reductions (block_sum /
// sum_partials / row partials of fine_device.h, no floating-point atomics).  A case's bits therefore depend neither on B nor on
// its neighbours, and equal the single-case solver's and tests/fine_solver_spec.py's.
//
// Per-case control.  Every sweep launch covers all cases with the same sweep index m.  A case's workgroups return at once when
// that case's own stop flag is set, or when the case is frozen (converged or diverged: Status::state != 0), so each case ends
// each inner solve at its own sweep and momentum_finish picks Jb or Var by the case's own count.  The host enqueues chunks
// predicted from the largest count among the live cases, reads all B status blocks in one copy per chunk, and ends the solve
// when every live case has stopped: host synchronisations per outer iteration do not grow with B.  The live cases wait for the
// slowest inner solve of the batch -- the lock-step cost, DESIGN.md section 2c.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "fine_device.h"

namespace srcfd {

bool fine_problem_ok(const srcfd_coarse_problem* pb);   // fine_solver.hip

namespace {

constexpr int MAX_CASES = 64;   // keeps the per-chunk status read small

struct CaseP {       // what may differ between the cases of a batch
  double dx, dy, volp, dt, rho, nu;
  double tol[3], relax[3];
  Bc bc[3];
};

struct BDev {
  int nx, ny, sx, sy;
  size_t stride;     // doubles per case: Var, Old, Jb (3 planes each), Ff (4), rhs (1), partials (9 nx)
  double* base;
  const CaseP* cp;
  Status* st;
};
constexpr size_t case_doubles(int nx, int ny) { return (size_t)14 * (nx + 2) * (ny + 2) + (size_t)9 * nx; }

__device__ __forceinline__ Dev case_dev(const BDev& b, int c) {
  const CaseP& p = b.cp[c];
  Dev g;
  g.nx = b.nx; g.ny = b.ny; g.sx = b.sx; g.sy = b.sy;
  g.dx = p.dx; g.dy = p.dy; g.volp = p.volp; g.dt = p.dt; g.rho = p.rho; g.nu = p.nu;
  double* f = b.base + (size_t)c * b.stride;
  const size_t sx = (size_t)b.sx;
  g.Var = f;
  g.Old = f + 3 * sx;
  g.Jb = f + 6 * sx;
  g.Ff = f + 9 * sx;
  g.rhs = f + 13 * sx;
  g.part = f + 14 * sx;
  g.st = b.st + c;
  return g;
}
__device__ __forceinline__ bool frozen(const BDev& b) { return b.st[blockIdx.y].state != SRCFD_CASE_RUNNING; }

// ---------------------------------------------------------------- boundary conditions of plane k (fine_solver.hip bc_kernel)
__global__ void __launch_bounds__(NT) bc_batch(BDev bd, int k) {
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const Bc& b = bd.cp[blockIdx.y].bc[k];
  const int t = blockIdx.x * NT + threadIdx.x + 1;
  double* V = g.Var + (size_t)k * g.sx;
  if (t <= g.ny) {
    const int j = t;
    V[j] = b.type[0] == 0 ? 2 * b.value[0] - V[(size_t)g.sy + j] : V[(size_t)g.sy + j];
    V[(size_t)(g.nx + 1) * g.sy + j] = b.type[1] == 0 ? 2 * b.value[1] - V[(size_t)g.nx * g.sy + j] : V[(size_t)g.nx * g.sy + j];
    if (b.bfs && k <= 1) {
      const double y = (j - 0.5) * g.dy;
      double* V1 = g.Var + (size_t)g.sx;
      if (y < b.step_h) {
        V[j] = -V[(size_t)g.sy + j];
      } else if (k == 1) {
        V1[j] = -V1[(size_t)g.sy + j];
      } else {
        double yp = y - b.step_h;
        if (yp < 0.0) yp = 0.0;
        if (yp > b.h) yp = b.h;
        const double u_in = 6.0 * b.Ub * (yp / b.h) * (1.0 - (yp / b.h));
        V[j] = 2.0 * u_in - V[(size_t)g.sy + j];
        V1[j] = -V1[(size_t)g.sy + j];
      }
    }
  }
  if (t <= g.nx) {
    const int i = t;
    V[(size_t)i * g.sy + g.ny + 1] = b.type[2] == 0 ? 2 * b.value[2] - V[(size_t)i * g.sy + g.ny] : V[(size_t)i * g.sy + g.ny];
    V[(size_t)i * g.sy] = b.type[3] == 0 ? 2 * b.value[3] - V[(size_t)i * g.sy + 1] : V[(size_t)i * g.sy + 1];
  }
}

// ---------------------------------------------------------------- element-wise passes over the interior (one thread per cell)
__device__ __forceinline__ bool interior(const BDev& g, int& i, int& j) {
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c >= (int64_t)g.nx * g.ny) return false;
  i = (int)(c / g.ny) + 1;
  j = (int)(c - (int64_t)(i - 1) * g.ny) + 1;
  return true;
}

__global__ void __launch_bounds__(NT) linear_interpolation_batch(BDev bd) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const double* V = g.Var;
  double* F = g.Ff;
  const size_t c = (size_t)i * g.sy + j;
  F[c] = (at(g, V, 0, i, j) + at(g, V, 0, i + 1, j)) * g.dy * 0.5;
  F[g.sx + c] = (at(g, V, 1, i, j) + at(g, V, 1, i, j + 1)) * g.dx * 0.5;
  F[2 * (size_t)g.sx + c] = -(at(g, V, 0, i, j) + at(g, V, 0, i - 1, j)) * g.dy * 0.5;
  F[3 * (size_t)g.sx + c] = -(at(g, V, 1, i, j) + at(g, V, 1, i, j - 1)) * g.dx * 0.5;
}

// Ends a momentum solve: the result sits in Jb when the case's own sweep count is odd; BFS under-relaxes against Old.
__global__ void __launch_bounds__(NT) momentum_finish_batch(BDev bd, int k, int relax) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const size_t c = (size_t)k * g.sx + (size_t)i * g.sy + j;
  double v = (g.st->m_sweeps & 1) ? g.Jb[c] : g.Var[c];
  if (relax) {
    const double alpha = bd.cp[blockIdx.y].relax[k];
    const double o = g.Old[c];
    v = o + alpha * (v - o);
  }
  g.Var[c] = v;
}

__global__ void __launch_bounds__(NT) under_relax_batch(BDev bd, int k) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const double alpha = bd.cp[blockIdx.y].relax[k];
  const size_t c = (size_t)k * g.sx + (size_t)i * g.sy + j;
  const double o = g.Old[c];
  g.Var[c] = o + alpha * (g.Var[c] - o);
}

__global__ void __launch_bounds__(NT) pressure_rhs_batch(BDev bd) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const size_t c = (size_t)i * g.sy + j;
  g.rhs[c] = g.rho / g.dt * (g.Ff[c] + g.Ff[g.sx + c] + g.Ff[2 * (size_t)g.sx + c] + g.Ff[3 * (size_t)g.sx + c]);
}

__global__ void __launch_bounds__(NT) update_flux_batch(BDev bd) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const double* P = g.Var + 2 * (size_t)g.sx;
  double* F = g.Ff;
  const size_t c = (size_t)i * g.sy + j;
  const double p = P[c];
  F[c] += -g.dt / g.rho * (P[c + g.sy] - p) * g.dy / g.dx;
  F[g.sx + c] += -g.dt / g.rho * (P[c + 1] - p) * g.dx / g.dy;
  F[2 * (size_t)g.sx + c] += -g.dt / g.rho * (P[c - g.sy] - p) * g.dy / g.dx;
  F[3 * (size_t)g.sx + c] += -g.dt / g.rho * (P[c - 1] - p) * g.dx / g.dy;
}

// The three planes at `dst` = those at `src` (offsets in a case's block) for every case that is not frozen: the Jb copy before a
// momentum solve, and Old = Var, which a case that has just converged or diverged skips as the single-case solver does.
__global__ void __launch_bounds__(NT) copy_planes_batch(BDev bd, size_t dst, size_t src) {
  if (frozen(bd)) return;
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  double* f = bd.base + (size_t)blockIdx.y * bd.stride;
  if (c < 3 * (int64_t)bd.sx) f[dst + c] = f[src + c];
}

// Var = 0 except the interior, which comes from Jb (where init staged the host array); ghosts and corners are left 0 for the BCs.
__global__ void __launch_bounds__(NT) take_interior_batch(BDev bd) {
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c >= 3 * (int64_t)bd.sx) return;
  double* f = bd.base + (size_t)blockIdx.y * bd.stride;
  const int r = (int)(c % bd.sx), i = r / bd.sy, j = r - i * bd.sy;
  f[c] = (i >= 1 && i <= bd.nx && j >= 1 && j <= bd.ny) ? f[6 * (size_t)bd.sx + c] : 0.0;
}

// ---------------------------------------------------------------- momentum: Jacobi sweep m of plane k, row blockIdx.x + 1 of case blockIdx.y
template <bool QUICK>
__global__ void __launch_bounds__(NT) momentum_sweep_batch(BDev bd, int k, int m) {
  __shared__ double lds[NT];
  __shared__ int flag;
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  if (m > 0) {
    if (uniform_flag(&g.st->m_stop, &flag)) return;
    const double s = sum_partials(mom_part(g, (m - 1) & 1), g.nx, lds);
    if (std::sqrt(s / (g.nx * g.ny)) < INNER_TOL) {
      if (blockIdx.x == 0 && threadIdx.x == 0) g.st->m_stop = 1;
      return;
    }
  }
  const double* S = (m & 1) ? g.Jb : g.Var;
  double* D = (m & 1) ? g.Var : g.Jb;
  const int i = blockIdx.x + 1;
  double acc = 0.0;
  for (int j = 1 + threadIdx.x; j <= g.ny; j += NT) {
    const size_t c0 = (size_t)i * g.sy + j;
    const double fe = g.Ff[c0], fn = g.Ff[g.sx + c0], fw = g.Ff[2 * (size_t)g.sx + c0], fs = g.Ff[3 * (size_t)g.sx + c0];
    const double c = at(g, S, k, i, j);
    const double ve = at(g, S, k, i + 1, j), vw_ = at(g, S, k, i - 1, j), vn = at(g, S, k, i, j + 1), vs = at(g, S, k, i, j - 1);
    double ue, uw, un, us, sum = 0.0;
    if (!QUICK) {
      if (fe >= 0) { ue = c; sum += fe; } else ue = ve;
      if (fw >= 0) { uw = c; sum += fw; } else uw = vw_;
      if (fn >= 0) { un = c; sum += fn; } else un = vn;
      if (fs >= 0) { us = c; sum += fs; } else us = vs;
    } else {
      if (fe >= 0) { ue = 0.75 * c + 0.375 * ve - 0.125 * vw_; sum += 0.75 * fe; }
      else { ue = 0.75 * ve + 0.375 * c - 0.125 * atw(g, S, k, i + 2, j); sum += 0.375 * fe; }
      if (fw >= 0) { uw = 0.75 * c + 0.375 * vw_ - 0.125 * ve; sum += 0.75 * fw; }
      else { uw = 0.75 * vw_ + 0.375 * c - 0.125 * atw(g, S, k, i - 2, j); sum += 0.375 * fw; }
      if (fn >= 0) { un = 0.75 * c + 0.375 * vn - 0.125 * vs; sum += 0.75 * fn; }
      else { un = 0.75 * vn + 0.375 * c - 0.125 * atw(g, S, k, i, j + 2); sum += 0.375 * fn; }
      if (fs >= 0) { us = 0.75 * c + 0.375 * vs - 0.125 * vn; sum += 0.75 * fs; }
      else { us = 0.75 * vs + 0.375 * c - 0.125 * atw(g, S, k, i, j - 2); sum += 0.375 * fs; }
    }
    const double Fc = ue * fe + uw * fw + un * fn + us * fs;
    const double ap_c = sum * g.volp;
    const double Fd = g.volp * ((ve - 2.0 * c + vw_) / (g.dx * g.dx) + (vn - 2.0 * c + vs) / (g.dy * g.dy));
    const double ap_d = -g.volp * (2.0 / (g.dx * g.dx) + 2.0 / (g.dy * g.dy));
    const double R = -(g.volp / g.dt * (c - at(g, g.Old, k, i, j)) + Fc + (-g.nu) * Fd);
    const double ap = g.volp / g.dt + ap_c + (-g.nu) * ap_d;
    D[(size_t)k * g.sx + c0] = c + R / ap;
    acc = acc + R * R;
  }
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) {
    mom_part(g, m & 1)[blockIdx.x] = s;
    if (blockIdx.x == 0) {
      g.st->m_sweeps = m + 1;
      if (m == 0) g.st->m_stop = 0;
    }
  }
}

// ---------------------------------------------------------------- pressure: colour `colour` of red-black sweep m, in place
__global__ void __launch_bounds__(NT) pressure_half_sweep_batch(BDev bd, int colour, int m) {
  __shared__ double lds[NT];
  __shared__ int flag;
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  if (colour == 1 || m > 0) {
    if (uniform_flag(&g.st->p_stop, &flag)) return;
  }
  if (colour == 0 && m > 0) {
    const double s = sum_partials(p_part(g, (m - 1) & 1), 2 * g.nx, lds);
    if (std::sqrt(s / (g.nx * g.ny)) < INNER_TOL) {
      if (blockIdx.x == 0 && threadIdx.x == 0) g.st->p_stop = 1;
      return;
    }
  }
  double* P = g.Var + 2 * (size_t)g.sx;
  const int i = blockIdx.x + 1;
  const int j0 = ((i + 1) & 1) == colour ? 1 : 2;
  const double ap_d = -g.volp * (2.0 / (g.dx * g.dx) + 2.0 / (g.dy * g.dy));
  double acc = 0.0;
  for (int j = j0 + 2 * threadIdx.x; j <= g.ny; j += 2 * NT) {
    const size_t c = (size_t)i * g.sy + j;
    const double p = P[c];
    const double Fd = g.volp * ((P[c + g.sy] - 2.0 * p + P[c - g.sy]) / (g.dx * g.dx) + (P[c + 1] - 2.0 * p + P[c - 1]) / (g.dy * g.dy));
    const double R = g.rhs[c] - Fd;
    P[c] = p + R / ap_d;
    acc = acc + R * R;
  }
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) {
    p_part(g, m & 1)[(size_t)colour * g.nx + blockIdx.x] = s;
    if (colour == 0 && blockIdx.x == 0) {
      g.st->p_sweeps = m + 1;
      if (m == 0) g.st->p_stop = 0;
    }
  }
}

// ---------------------------------------------------------------- correct_velocity with the residual partials (row per workgroup)
__global__ void __launch_bounds__(NT) correct_velocity_batch(BDev bd) {
  __shared__ double lds[NT];
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const int i = blockIdx.x + 1;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  const double* P = g.Var + 2 * (size_t)g.sx;
  for (int j = 1 + threadIdx.x; j <= g.ny; j += NT) {
    const size_t c = (size_t)i * g.sy + j;
    const double u = g.Var[c] - g.dt / g.rho * (P[c + g.sy] - P[c - g.sy]) / (2 * g.dx);
    const double v = g.Var[g.sx + c] - g.dt / g.rho * (P[c + 1] - P[c - 1]) / (2 * g.dy);
    g.Var[c] = u;
    g.Var[g.sx + c] = v;
    const double d0 = u - g.Old[c], d1 = v - g.Old[g.sx + c], d2 = P[c] - g.Old[2 * (size_t)g.sx + c];
    a0 = a0 + d0 * d0;
    a1 = a1 + d1 * d1;
    a2 = a2 + d2 * d2;
  }
  const double s0 = block_sum(a0, lds), s1 = block_sum(a1, lds), s2 = block_sum(a2, lds);
  if (threadIdx.x == 0) {
    double* r = res_part(g);
    r[blockIdx.x] = s0;
    r[g.nx + blockIdx.x] = s1;
    r[2 * (size_t)g.nx + blockIdx.x] = s2;
  }
}

// _convergence_check, one workgroup per case.  Non-finite residuals are tested first: `r > tol` is false for NaN, so the
// converged test alone would take a NaN for convergence.
__global__ void __launch_bounds__(NT) convergence_check_batch(BDev bd) {
  __shared__ double lds[NT];
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  double res[3];
  for (int k = 0; k < 3; ++k) res[k] = sum_partials(res_part(g) + (size_t)k * g.nx, g.nx, lds);
  if (threadIdx.x != 0) return;
  const CaseP& p = bd.cp[blockIdx.y];
  int conv = 1, bad = 0;
  for (int k = 0; k < 3; ++k) {
    const double r = std::sqrt(res[k] / (g.nx * g.ny)) / g.dt;
    g.st->rms[k] = r;
    if (!std::isfinite(r)) bad = 1;
    if (r > p.tol[k]) conv = 0;
  }
  g.st->nonfinite = bad;
  g.st->converged = bad ? 0 : conv;
  g.st->state = bad ? SRCFD_CASE_DIVERGED : conv ? SRCFD_CASE_CONVERGED : SRCFD_CASE_RUNNING;
}

}  // namespace

struct FineBatch {
  std::vector<srcfd_coarse_problem> pb;
  int n = 0, device = 0;
  BDev g{};
  hipStream_t stream = nullptr;
  Status* host_st = nullptr;   // page-locked, n blocks
  char* d_mem = nullptr;
  size_t state_bytes = 0;      // fields and status blocks: what init clears
  int count = 0;               // outer iterations of the live cases since the last init
  bool primed = false;
  std::vector<int> state, iters, last_sweeps;   // per case; last_sweeps [n][3]
  std::vector<double> rms;                      // [n][3]
  int predict[3] = {16, 16, SWEEP_CAP};         // chunk sizes: the largest count of the previous solve + margin
  int64_t n_mom = 0, n_p = 0, n_launch = 0, n_sync = 0;

  ~FineBatch() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamDestroy(stream);
    if (d_mem) (void)hipFree(d_mem);
    if (host_st) (void)hipHostFree(host_st);
  }
  bool bfs() const { return pb[0].case_type == SRCFD_CASE_BFS; }
  bool live(int c) const { return state[c] == SRCFD_CASE_RUNNING; }
  bool any_live() const {
    for (int c = 0; c < n; ++c) if (live(c)) return true;
    return false;
  }
  dim3 cells_grid() const { return dim3((unsigned)(((int64_t)g.nx * g.ny + NT - 1) / NT), (unsigned)n); }
  dim3 var_grid() const { return dim3((unsigned)((3 * (int64_t)g.sx + NT - 1) / NT), (unsigned)n); }
  dim3 rows_grid() const { return dim3((unsigned)g.nx, (unsigned)n); }

  static int hip_fail(const char* what, hipError_t e) {
    set_error(std::string("fine batch: ") + what + " failed: " + hipGetErrorString(e));
    return SRCFD_EHIP;
  }
#define HIPCHECK_FB(expr)                                   \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return hip_fail(#expr, _e);       \
  } while (0)

  int launched() {
    ++n_launch;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string("fine batch: kernel launch failed: ") + hipGetErrorString(e)); return SRCFD_EHIP; }
    return SRCFD_OK;
  }
  int sync_status() {   // all n status blocks in one copy
    ++n_sync;
    HIPCHECK_FB(hipMemcpyAsync(host_st, g.st, (size_t)n * sizeof(Status), hipMemcpyDeviceToHost, stream));
    HIPCHECK_FB(hipStreamSynchronize(stream));
    return SRCFD_OK;
  }

  int bc(int k) {
    const int m = g.nx > g.ny ? g.nx : g.ny;
    hipLaunchKernelGGL(bc_batch, dim3((m + NT - 1) / NT, n), dim3(NT), 0, stream, g, k);
    return launched();
  }
  int copy_planes(size_t dst, size_t src) {
    hipLaunchKernelGGL(copy_planes_batch, var_grid(), dim3(NT), 0, stream, g, dst, src);
    return launched();
  }
  int prime() {   // BCs, Old = Var, linear_interpolation, as FineSolver::prime
    int rc;
    for (int k = 0; k < 3; ++k) if ((rc = bc(k))) return rc;
    if ((rc = copy_planes(3 * (size_t)g.sx, 0))) return rc;
    hipLaunchKernelGGL(linear_interpolation_batch, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = sync_status())) return rc;
    count = 0;
    for (int c = 0; c < n; ++c) {
      state[c] = SRCFD_CASE_RUNNING;
      iters[c] = 0;
      for (int k = 0; k < 3; ++k) rms[3 * c + k] = 0.0;
    }
    primed = true;
    return SRCFD_OK;
  }

  // One inner solve of every live case: chunks of sweep launches until each has stopped or the cap is reached.
  int inner(int which, int k, int64_t* executed) {
    int done = 0, chunk = predict[which], rc;
    for (;;) {
      if (chunk > SWEEP_CAP - done) chunk = SWEEP_CAP - done;
      for (int m = done; m < done + chunk; ++m) {
        if (which < 2) {
          if (pb[0].scheme == SRCFD_SCHEME_QUICK) hipLaunchKernelGGL(momentum_sweep_batch<true>, rows_grid(), dim3(NT), 0, stream, g, k, m);
          else hipLaunchKernelGGL(momentum_sweep_batch<false>, rows_grid(), dim3(NT), 0, stream, g, k, m);
          if ((rc = launched())) return rc;
        } else {
          for (int colour = 0; colour < 2; ++colour) {
            hipLaunchKernelGGL(pressure_half_sweep_batch, rows_grid(), dim3(NT), 0, stream, g, colour, m);
            if ((rc = launched())) return rc;
          }
        }
      }
      done += chunk;
      if ((rc = sync_status())) return rc;
      bool all_stopped = true;
      for (int c = 0; c < n; ++c)
        if (live(c) && !(which < 2 ? host_st[c].m_stop : host_st[c].p_stop)) all_stopped = false;
      if (all_stopped || done >= SWEEP_CAP) break;
      chunk = chunk < 8 ? 8 : 2 * chunk;
    }
    int most = 0;
    for (int c = 0; c < n; ++c) {
      if (!live(c)) continue;
      const int s = which < 2 ? host_st[c].m_sweeps : host_st[c].p_sweeps;
      last_sweeps[3 * c + which] = s;
      if (s > most) most = s;
    }
    *executed += most;
    const int next = most + 2 + most / 8;
    predict[which] = next > SWEEP_CAP ? SWEEP_CAP : next;
    return SRCFD_OK;
  }

  // One outer iteration of every live case (FineSolver::outer's sequence)
  int outer() {
    int rc;
    const int relax = bfs() ? 1 : 0;
    const size_t sx = (size_t)g.sx;
    for (int k = 0; k < 2; ++k) {
      if ((rc = copy_planes(6 * sx, 0))) return rc;
      if ((rc = inner(k, k, &n_mom))) return rc;
      hipLaunchKernelGGL(momentum_finish_batch, cells_grid(), dim3(NT), 0, stream, g, k, relax);
      if ((rc = launched())) return rc;
      if ((rc = bc(k))) return rc;
    }
    hipLaunchKernelGGL(linear_interpolation_batch, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(pressure_rhs_batch, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = inner(2, 2, &n_p))) return rc;
    if (relax) {
      hipLaunchKernelGGL(under_relax_batch, cells_grid(), dim3(NT), 0, stream, g, 2);
      if ((rc = launched())) return rc;
    }
    if ((rc = bc(2))) return rc;
    hipLaunchKernelGGL(correct_velocity_batch, rows_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = bc(0))) return rc;
    if ((rc = bc(1))) return rc;
    hipLaunchKernelGGL(update_flux_batch, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(convergence_check_batch, dim3(1, n), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = copy_planes(3 * sx, 0))) return rc;   // Old = Var of the cases that go on
    return sync_status();
  }
#undef HIPCHECK_FB
};

}  // namespace srcfd

using srcfd::FineBatch;
using srcfd::set_error;

extern "C" {

int srcfd_fine_batch_footprint(int nx, int ny, int n_cases, int64_t* device_bytes) {
  return srcfd::abi_guard("srcfd_fine_batch_footprint", [&]() -> int {
    if (!device_bytes || nx < 3 || ny < 3 || nx > 4096 || ny > 4096 || n_cases < 1 || n_cases > srcfd::MAX_CASES) {
      set_error("srcfd_fine_batch_footprint: bad arguments");
      return SRCFD_EINVAL;
    }
    *device_bytes = (int64_t)n_cases * (int64_t)(srcfd::case_doubles(nx, ny) * sizeof(double) + sizeof(srcfd::Status) + sizeof(srcfd::CaseP));
    return SRCFD_OK;
  });
}

int srcfd_fine_batch_create(const srcfd_coarse_problem* problems, int n_cases, int device, srcfd_fine_batch** out) {
  return srcfd::abi_guard("srcfd_fine_batch_create", [&]() -> int {
    const std::string who = "srcfd_fine_batch_create: ";
    if (!out) { set_error(who + "bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    if (n_cases < 1 || n_cases > srcfd::MAX_CASES) {
      set_error(who + "n_cases " + std::to_string(n_cases) + " is outside 1.." + std::to_string(srcfd::MAX_CASES));
      return SRCFD_EINVAL;
    }
    if (!problems) { set_error(who + "bad arguments"); return SRCFD_EINVAL; }
    for (int c = 0; c < n_cases; ++c) {
      const srcfd_coarse_problem& p = problems[c];
      if (!srcfd::fine_problem_ok(&p)) { set_error(who + "case " + std::to_string(c) + ": bad problem description"); return SRCFD_EINVAL; }
      const char* field = p.nx != problems[0].nx ? "nx" : p.ny != problems[0].ny ? "ny" : p.scheme != problems[0].scheme ? "scheme" :
                          p.case_type != problems[0].case_type ? "case_type" : nullptr;
      if (field) {
        set_error(who + "case " + std::to_string(c) + ": " + field + " differs from case 0 (one batch has one mesh, scheme and case type)");
        return SRCFD_EINVAL;
      }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error(who + "no HIP device"); return SRCFD_ENODEV; }
    if (device < 0 || device >= ndev) { set_error(who + "bad device index"); return SRCFD_EINVAL; }
    std::unique_ptr<FineBatch> s(new FineBatch());
    s->pb.assign(problems, problems + n_cases);
    s->n = n_cases;
    s->device = device;
    s->state.assign(n_cases, SRCFD_CASE_RUNNING);
    s->iters.assign(n_cases, 0);
    s->last_sweeps.assign((size_t)3 * n_cases, 0);
    s->rms.assign((size_t)3 * n_cases, 0.0);
    HIPCHECK(hipSetDevice(device));
    srcfd::BDev& g = s->g;
    g.nx = problems[0].nx; g.ny = problems[0].ny; g.sy = g.ny + 2; g.sx = (g.nx + 2) * (g.ny + 2);
    g.stride = srcfd::case_doubles(g.nx, g.ny);
    std::vector<srcfd::CaseP> cp((size_t)n_cases);
    for (int c = 0; c < n_cases; ++c) {
      const srcfd_coarse_problem& p = problems[c];
      srcfd::CaseP& q = cp[c];
      std::memset(&q, 0, sizeof(q));
      q.dx = p.lx / g.nx; q.dy = p.ly / g.ny; q.volp = q.dx * q.dy;
      q.dt = p.dt; q.rho = p.rho; q.nu = 1.0 / p.reynolds;
      for (int k = 0; k < 3; ++k) {
        q.tol[k] = p.tolerance[k];
        q.relax[k] = p.relax[k];
        for (int side = 0; side < 4; ++side) { q.bc[k].type[side] = p.bc_type[k][side]; q.bc[k].value[side] = p.bc_value[k][side]; }
        q.bc[k].bfs = p.case_type == SRCFD_CASE_BFS;
        q.bc[k].step_h = p.step_height; q.bc[k].h = p.channel_height; q.bc[k].Ub = p.bulk_velocity;
      }
    }
    const size_t field_bytes = (size_t)n_cases * g.stride * sizeof(double);
    s->state_bytes = field_bytes + (size_t)n_cases * sizeof(srcfd::Status);
    const size_t total = s->state_bytes + (size_t)n_cases * sizeof(srcfd::CaseP);
    HIPCHECK(hipMalloc(&s->d_mem, total));
    g.base = reinterpret_cast<double*>(s->d_mem);
    g.st = reinterpret_cast<srcfd::Status*>(s->d_mem + field_bytes);
    g.cp = reinterpret_cast<const srcfd::CaseP*>(s->d_mem + s->state_bytes);
    HIPCHECK(hipMemset(s->d_mem, 0, s->state_bytes));
    HIPCHECK(hipMemcpy(s->d_mem + s->state_bytes, cp.data(), cp.size() * sizeof(srcfd::CaseP), hipMemcpyHostToDevice));
    HIPCHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&s->host_st), (size_t)n_cases * sizeof(srcfd::Status), hipHostMallocDefault));
    std::memset(s->host_st, 0, (size_t)n_cases * sizeof(srcfd::Status));
    *out = reinterpret_cast<srcfd_fine_batch*>(s.release());
    return SRCFD_OK;
  });
}

void srcfd_fine_batch_destroy(srcfd_fine_batch* b) { delete reinterpret_cast<FineBatch*>(b); }

int srcfd_fine_batch_init(srcfd_fine_batch* b, const double* var) {
  return srcfd::abi_guard("srcfd_fine_batch_init", [&]() -> int {
    if (!b) { set_error("srcfd_fine_batch_init: bad arguments"); return SRCFD_EINVAL; }
    FineBatch* f = reinterpret_cast<FineBatch*>(b);
    srcfd::BDev& g = f->g;
    HIPCHECK(hipSetDevice(f->device));
    f->primed = false;
    HIPCHECK(hipMemsetAsync(f->d_mem, 0, f->state_bytes, f->stream));   // fields, fluxes and every case's status: all cases live
    ++f->n_launch;
    if (var) {   // staged through each case's Jb, which every momentum solve overwrites
      const size_t planes = 3 * (size_t)g.sx;
      for (int c = 0; c < f->n; ++c)
        HIPCHECK(hipMemcpyAsync(g.base + (size_t)c * g.stride + 2 * planes, var + (size_t)c * planes, planes * sizeof(double),
                                hipMemcpyHostToDevice, f->stream));
      hipLaunchKernelGGL(srcfd::take_interior_batch, f->var_grid(), dim3(srcfd::NT), 0, f->stream, g);
      int rc = f->launched();
      if (rc) return rc;
    }
    return f->prime();
  });
}

int srcfd_fine_batch_run(srcfd_fine_batch* b, int max_iterations, int* iterations, int* status, double* rms, double* history,
                         int history_len) {
  return srcfd::abi_guard("srcfd_fine_batch_run", [&]() -> int {
    if (!b || max_iterations < 0 || history_len < 0 || (history_len > 0 && !history)) {
      set_error("srcfd_fine_batch_run: bad arguments");
      return SRCFD_EINVAL;
    }
    FineBatch* f = reinterpret_cast<FineBatch*>(b);
    if (!f->primed) { set_error("srcfd_fine_batch_run: call srcfd_fine_batch_init first"); return SRCFD_EINVAL; }
    HIPCHECK(hipSetDevice(f->device));
    std::vector<int> n_hist((size_t)f->n, 0);
    for (int it = 0; it < max_iterations && f->any_live(); ++it) {
      ++f->count;
      int rc = f->outer();
      if (rc) { f->primed = false; return rc; }
      for (int c = 0; c < f->n; ++c) {
        if (!f->live(c)) continue;
        const srcfd::Status& st = f->host_st[c];
        f->iters[c] = f->count;
        f->state[c] = st.state;   // a diverged case is frozen on the device already; the others go on
        for (int k = 0; k < 3; ++k) f->rms[3 * c + k] = st.rms[k];
        if (f->count % 100 == 0 && n_hist[c] < history_len) {   // residual_history, at the case's own iterations 100, 200, ...
          for (int k = 0; k < 3; ++k) history[((size_t)c * history_len + n_hist[c]) * 3 + k] = st.rms[k];
          ++n_hist[c];
        }
      }
    }
    for (int c = 0; c < f->n; ++c) {
      if (iterations) iterations[c] = f->iters[c];
      if (status) status[c] = f->state[c];
      if (rms) for (int k = 0; k < 3; ++k) rms[3 * c + k] = f->rms[3 * c + k];
    }
    return SRCFD_OK;
  });
}

int srcfd_fine_batch_get_state(srcfd_fine_batch* b, int case_index, double* var) {
  return srcfd::abi_guard("srcfd_fine_batch_get_state", [&]() -> int {
    FineBatch* f = reinterpret_cast<FineBatch*>(b);
    if (!b || !var || case_index < -1 || case_index >= f->n) { set_error("srcfd_fine_batch_get_state: bad arguments"); return SRCFD_EINVAL; }
    const srcfd::BDev& g = f->g;
    HIPCHECK(hipSetDevice(f->device));
    const size_t planes = 3 * (size_t)g.sx;
    const int first = case_index < 0 ? 0 : case_index, last = case_index < 0 ? f->n : case_index + 1;
    for (int c = first; c < last; ++c)
      HIPCHECK(hipMemcpyAsync(var + (size_t)(c - first) * planes, g.base + (size_t)c * g.stride, planes * sizeof(double),
                              hipMemcpyDeviceToHost, f->stream));
    HIPCHECK(hipStreamSynchronize(f->stream));
    return SRCFD_OK;
  });
}

int srcfd_fine_batch_counters(const srcfd_fine_batch* b, int64_t counters[4], int* last_sweeps) {
  return srcfd::abi_guard("srcfd_fine_batch_counters", [&]() -> int {
    if (!b) { set_error("srcfd_fine_batch_counters: bad arguments"); return SRCFD_EINVAL; }
    const FineBatch* f = reinterpret_cast<const FineBatch*>(b);
    if (counters) {
      counters[0] = f->n_mom;
      counters[1] = f->n_p;
      counters[2] = f->n_launch;
      counters[3] = f->n_sync;
    }
    if (last_sweeps) for (int q = 0; q < 3 * f->n; ++q) last_sweeps[q] = f->last_sweeps[q];
    return SRCFD_OK;
  });
}

}  // extern "C"
