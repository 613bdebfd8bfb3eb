// Fine-mesh incompressible solver on the device (float64): the solve the SR warm start is for.
//
// The same outer loop as srcfd_coarse_solve (coarse_solver.cpp; PyCFD_ML_accelerated.py:433-505, bfs_ml_accelerated.py:626-707)
// with the same expressions in the same operation order, so that with -ffp-contract=off every cell update rounds as the host's
// does.  The one deliberate change is the order of the inner sweeps, which must be race-free on the device (the reference's
// numba `prange` sweeps are a benign race, the host port is serial):
//   momentum  Jacobi: sweep m reads buffer m & 1 and writes buffer (m + 1) & 1 (buffer 0 = Var, buffer 1 = Jb, a full copy of
//             Var taken before the solve, so the run-on reads that cross planes see the same values in both);
//   pressure  red-black in place, colour (i + j) & 1, colour 0 first; the 5-point stencil never reads its own colour.
// The inner exit rule is the host's: at least one sweep, stop when sqrt(sum R^2 / (nx ny)) < 1e-6, at most 1000 sweeps.  sum R^2
// is reduced in a fixed order without floating-point atomics (block_sum / sum_partials below); tests/fine_solver_spec.py restates
// all of it in numpy and the GPU tests require the same bits.
//
// Loop control: one launch per sweep (pressure: per colour).  Each sweep launch first reduces the previous sweep's partials and
// returns at once when the inner solve has stopped, so the host enqueues sweeps in chunks sized from the previous solve's count and
// reads one small status block per chunk -- never per sweep.  See DESIGN.md, "Fine-mesh solve on the device".
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "fine_device.h"

namespace srcfd {

int predict_solver_state(Model* mm, srcfd_resampler* r, const float* x, const float* in_affine, const float* out_affine,
                         const srcfd_solver_bc bc[3], int want_nx, int want_ny, double* d_var, double* host_var, int flags,
                         int64_t* n_nonfinite);   // resample.hip

namespace {

// ---------------------------------------------------------------- boundary conditions, apply_bc + apply_bfs_inlet of plane k
__global__ void __launch_bounds__(NT) bc_kernel(Dev g, int k, Bc b) {
  const int t = blockIdx.x * NT + threadIdx.x + 1;
  double* V = g.Var + (size_t)k * g.sx;
  if (t <= g.ny) {
    const int j = t;
    V[j] = b.type[0] == 0 ? 2 * b.value[0] - V[(size_t)g.sy + j] : V[(size_t)g.sy + j];
    V[(size_t)(g.nx + 1) * g.sy + j] = b.type[1] == 0 ? 2 * b.value[1] - V[(size_t)g.nx * g.sy + j] : V[(size_t)g.nx * g.sy + j];
    if (b.bfs && k <= 1) {   // CFDSolver._apply_bfs_inlet (bfs_ml_accelerated.py:523-562), as coarse_solver.cpp apply_bfs_inlet
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
__device__ __forceinline__ bool interior(const Dev& g, int& i, int& j) {
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c >= (int64_t)g.nx * g.ny) return false;
  i = (int)(c / g.ny) + 1;
  j = (int)(c - (int64_t)(i - 1) * g.ny) + 1;
  return true;
}

__global__ void __launch_bounds__(NT) linear_interpolation(Dev g) {   // PyCFD_ML_accelerated.py:148-155
  int i, j;
  if (!interior(g, i, j)) return;
  const double* V = g.Var;
  double* F = g.Ff;
  const size_t c = (size_t)i * g.sy + j;
  F[c] = (at(g, V, 0, i, j) + at(g, V, 0, i + 1, j)) * g.dy * 0.5;
  F[g.sx + c] = (at(g, V, 1, i, j) + at(g, V, 1, i, j + 1)) * g.dx * 0.5;
  F[2 * (size_t)g.sx + c] = -(at(g, V, 0, i, j) + at(g, V, 0, i - 1, j)) * g.dy * 0.5;
  F[3 * (size_t)g.sx + c] = -(at(g, V, 1, i, j) + at(g, V, 1, i, j - 1)) * g.dx * 0.5;
}

// Ends a momentum solve: the result sits in Jb when the sweep count is odd; BFS under-relaxes against Old (bfs...:371-375).
__global__ void __launch_bounds__(NT) momentum_finish(Dev g, int k, int relax, double alpha) {
  int i, j;
  if (!interior(g, i, j)) return;
  const size_t c = (size_t)k * g.sx + (size_t)i * g.sy + j;
  double v = (g.st->m_sweeps & 1) ? g.Jb[c] : g.Var[c];
  if (relax) {
    const double o = g.Old[c];
    v = o + alpha * (v - o);
  }
  g.Var[c] = v;
}

__global__ void __launch_bounds__(NT) under_relax(Dev g, int k, double alpha) {
  int i, j;
  if (!interior(g, i, j)) return;
  const size_t c = (size_t)k * g.sx + (size_t)i * g.sy + j;
  const double o = g.Old[c];
  g.Var[c] = o + alpha * (g.Var[c] - o);
}

__global__ void __launch_bounds__(NT) pressure_rhs(Dev g) {   // the RHS of solve_pressure: Ff is constant inside the solve
  int i, j;
  if (!interior(g, i, j)) return;
  const size_t c = (size_t)i * g.sy + j;
  g.rhs[c] = g.rho / g.dt * (g.Ff[c] + g.Ff[g.sx + c] + g.Ff[2 * (size_t)g.sx + c] + g.Ff[3 * (size_t)g.sx + c]);
}

__global__ void __launch_bounds__(NT) update_flux(Dev g) {   // PyCFD_ML_accelerated.py:242-249
  int i, j;
  if (!interior(g, i, j)) return;
  const double* P = g.Var + 2 * (size_t)g.sx;
  double* F = g.Ff;
  const size_t c = (size_t)i * g.sy + j;
  const double p = P[c];
  F[c] += -g.dt / g.rho * (P[c + g.sy] - p) * g.dy / g.dx;
  F[g.sx + c] += -g.dt / g.rho * (P[c + 1] - p) * g.dx / g.dy;
  F[2 * (size_t)g.sx + c] += -g.dt / g.rho * (P[c - g.sy] - p) * g.dy / g.dx;
  F[3 * (size_t)g.sx + c] += -g.dt / g.rho * (P[c - 1] - p) * g.dx / g.dy;
}

__global__ void __launch_bounds__(NT) copy_f64(double* __restrict__ dst, const double* __restrict__ src, int64_t n, const int* skip_if) {
  if (skip_if && *skip_if) return;
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c < n) dst[c] = src[c];
}

// Var = 0 except the interior, which comes from `src` (same layout); corners and ghosts are left 0 for the BC pass.
__global__ void __launch_bounds__(NT) take_interior(Dev g, const double* __restrict__ src) {
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c >= 3 * (int64_t)g.sx) return;
  const int r = (int)(c % g.sx), i = r / g.sy, j = r - i * g.sy;
  g.Var[c] = (i >= 1 && i <= g.nx && j >= 1 && j <= g.ny) ? src[c] : 0.0;
}

// ---------------------------------------------------------------- momentum: one Jacobi sweep m of plane k (row i = blockIdx.x + 1)
template <bool QUICK>
__global__ void __launch_bounds__(NT) momentum_sweep(Dev g, int k, int m) {
  __shared__ double lds[NT];
  __shared__ int flag;
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
    if (!QUICK) {   // simple_upwind, PyCFD_ML_accelerated.py:157-189
      if (fe >= 0) { ue = c; sum += fe; } else ue = ve;
      if (fw >= 0) { uw = c; sum += fw; } else uw = vw_;
      if (fn >= 0) { un = c; sum += fn; } else un = vn;
      if (fs >= 0) { us = c; sum += fs; } else us = vs;
    } else {        // quick_scheme, :191-231
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
__global__ void __launch_bounds__(NT) pressure_half_sweep(Dev g, int colour, int m) {
  __shared__ double lds[NT];
  __shared__ int flag;
  if (colour == 1 || m > 0) {
    if (uniform_flag(&g.st->p_stop, &flag)) return;
  }
  if (colour == 0 && m > 0) {
    const double s = sum_partials(p_part(g, (m - 1) & 1), 2 * g.nx, lds);   // colour 0's rows, then colour 1's
    if (std::sqrt(s / (g.nx * g.ny)) < INNER_TOL) {
      if (blockIdx.x == 0 && threadIdx.x == 0) g.st->p_stop = 1;
      return;
    }
  }
  double* P = g.Var + 2 * (size_t)g.sx;
  const int i = blockIdx.x + 1;
  const int j0 = ((i + 1) & 1) == colour ? 1 : 2;   // first j of this colour in row i
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
__global__ void __launch_bounds__(NT) correct_velocity(Dev g) {   // PyCFD_ML_accelerated.py:323-335
  __shared__ double lds[NT];
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

// _convergence_check (PyCFD_ML_accelerated.py:472-505): one workgroup
__global__ void __launch_bounds__(NT) convergence_check(Dev g, double tol0, double tol1, double tol2) {
  __shared__ double lds[NT];
  double res[3];
  for (int k = 0; k < 3; ++k) res[k] = sum_partials(res_part(g) + (size_t)k * g.nx, g.nx, lds);
  if (threadIdx.x != 0) return;
  const double tol[3] = {tol0, tol1, tol2};
  int conv = 1, bad = 0;
  for (int k = 0; k < 3; ++k) {
    const double r = std::sqrt(res[k] / (g.nx * g.ny)) / g.dt;
    g.st->rms[k] = r;
    if (!std::isfinite(r)) bad = 1;
    if (r > tol[k]) conv = 0;
  }
  g.st->converged = conv;
  g.st->nonfinite = bad;
}

}  // namespace

#define HIPCHECK_FS(expr)                                   \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return hip_fail(#expr, _e);       \
  } while (0)

struct FineSolver {
  srcfd_coarse_problem pb{};
  int device = 0;
  Dev g{};
  hipStream_t stream = nullptr;
  Status* host_st = nullptr;   // page-locked
  double* d_mem = nullptr;
  int count = 0;               // outer iterations since the last init
  bool converged = false;
  bool primed = false;
  int predict[3] = {16, 16, SWEEP_CAP};   // chunk sizes: the previous solve's count + margin
  int last_sweeps[3] = {0, 0, 0};
  int64_t n_mom = 0, n_p = 0, n_launch = 0, n_sync = 0;

  ~FineSolver() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamDestroy(stream);
    if (d_mem) (void)hipFree(d_mem);
    if (host_st) (void)hipHostFree(host_st);
  }
  bool bfs() const { return pb.case_type == SRCFD_CASE_BFS; }
  unsigned cells_blocks() const { return (unsigned)(((int64_t)g.nx * g.ny + NT - 1) / NT); }
  unsigned var_blocks() const { return (unsigned)((3 * (int64_t)g.sx + NT - 1) / NT); }

  int launched() {
    ++n_launch;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string("fine solver: kernel launch failed: ") + hipGetErrorString(e)); return SRCFD_EHIP; }
    return SRCFD_OK;
  }
  int sync_status() {
    ++n_sync;
    HIPCHECK_FS(hipMemcpyAsync(host_st, g.st, sizeof(Status), hipMemcpyDeviceToHost, stream));
    HIPCHECK_FS(hipStreamSynchronize(stream));
    return SRCFD_OK;
  }
  static int hip_fail(const char* what, hipError_t e) {
    set_error(std::string("fine solver: ") + what + " failed: " + hipGetErrorString(e));
    return SRCFD_EHIP;
  }

  int bc(int k) {
    Bc b{};
    for (int s = 0; s < 4; ++s) { b.type[s] = pb.bc_type[k][s]; b.value[s] = pb.bc_value[k][s]; }
    b.bfs = bfs();
    b.step_h = pb.step_height; b.h = pb.channel_height; b.Ub = pb.bulk_velocity;
    const int n = g.nx > g.ny ? g.nx : g.ny;
    hipLaunchKernelGGL(bc_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, stream, g, k, b);
    return launched();
  }
  int prime() {   // BCs (with the BFS inlet), Old = Var, linear_interpolation: _initialize_fields / PyCFD_ML_accelerated.py:940-953
    int rc;
    for (int k = 0; k < 3; ++k) if ((rc = bc(k))) return rc;
    hipLaunchKernelGGL(copy_f64, dim3(var_blocks()), dim3(NT), 0, stream, g.Old, g.Var, 3 * (int64_t)g.sx, (const int*)nullptr);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(linear_interpolation, dim3(cells_blocks()), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = sync_status())) return rc;
    count = 0;
    converged = false;
    primed = true;
    return SRCFD_OK;
  }

  // One inner solve: chunks of sweep launches until the exit rule has fired or the cap is reached.  Returns the sweep count.
  int inner(int which, int k, int* sweeps) {
    int done = 0, chunk = predict[which], rc;
    for (;;) {
      if (chunk > SWEEP_CAP - done) chunk = SWEEP_CAP - done;
      for (int m = done; m < done + chunk; ++m) {
        if (which < 2) {
          if (pb.scheme == SRCFD_SCHEME_QUICK) hipLaunchKernelGGL(momentum_sweep<true>, dim3(g.nx), dim3(NT), 0, stream, g, k, m);
          else hipLaunchKernelGGL(momentum_sweep<false>, dim3(g.nx), dim3(NT), 0, stream, g, k, m);
          if ((rc = launched())) return rc;
        } else {
          for (int colour = 0; colour < 2; ++colour) {
            hipLaunchKernelGGL(pressure_half_sweep, dim3(g.nx), dim3(NT), 0, stream, g, colour, m);
            if ((rc = launched())) return rc;
          }
        }
      }
      done += chunk;
      if ((rc = sync_status())) return rc;
      const int stop = which < 2 ? host_st->m_stop : host_st->p_stop;
      if (stop || done >= SWEEP_CAP) break;
      chunk = chunk < 8 ? 8 : 2 * chunk;
    }
    const int n = which < 2 ? host_st->m_sweeps : host_st->p_sweeps;
    *sweeps = n;
    const int next = n + 2 + n / 8;
    predict[which] = next > SWEEP_CAP ? SWEEP_CAP : next;
    return SRCFD_OK;
  }

  // One outer iteration: _implicit_solve + _convergence_check (the order of srcfd_coarse_solve)
  int outer() {
    int rc, sw = 0;
    const bool relax = bfs();
    for (int k = 0; k < 2; ++k) {
      hipLaunchKernelGGL(copy_f64, dim3(var_blocks()), dim3(NT), 0, stream, g.Jb, g.Var, 3 * (int64_t)g.sx, (const int*)nullptr);
      if ((rc = launched())) return rc;
      if ((rc = inner(k, k, &sw))) return rc;
      last_sweeps[k] = sw;
      n_mom += sw;
      hipLaunchKernelGGL(momentum_finish, dim3(cells_blocks()), dim3(NT), 0, stream, g, k, relax ? 1 : 0, pb.relax[k]);
      if ((rc = launched())) return rc;
      if ((rc = bc(k))) return rc;
    }
    hipLaunchKernelGGL(linear_interpolation, dim3(cells_blocks()), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(pressure_rhs, dim3(cells_blocks()), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = inner(2, 2, &sw))) return rc;
    last_sweeps[2] = sw;
    n_p += sw;
    if (relax) {
      hipLaunchKernelGGL(under_relax, dim3(cells_blocks()), dim3(NT), 0, stream, g, 2, pb.relax[2]);
      if ((rc = launched())) return rc;
    }
    if ((rc = bc(2))) return rc;
    hipLaunchKernelGGL(correct_velocity, dim3(g.nx), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = bc(0))) return rc;
    if ((rc = bc(1))) return rc;
    hipLaunchKernelGGL(update_flux, dim3(cells_blocks()), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(convergence_check, dim3(1), dim3(NT), 0, stream, g, pb.tolerance[0], pb.tolerance[1], pb.tolerance[2]);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(copy_f64, dim3(var_blocks()), dim3(NT), 0, stream, g.Old, g.Var, 3 * (int64_t)g.sx, (const int*)&g.st->converged);
    if ((rc = launched())) return rc;
    return sync_status();
  }
#undef HIPCHECK_FS
};

bool fine_problem_ok(const srcfd_coarse_problem* pb);

}  // namespace srcfd

using srcfd::FineSolver;
using srcfd::set_error;

namespace srcfd {
// srcfd_coarse_solve's validation rules (coarse_solver.cpp)
bool fine_problem_ok(const srcfd_coarse_problem* pb) {
  return !(pb->nx < 3 || pb->ny < 3 || pb->nx > 4096 || pb->ny > 4096 || !(pb->lx > 0) || !(pb->ly > 0) || !(pb->reynolds > 0) ||
           !(pb->rho > 0) || !(pb->dt > 0) || pb->max_iterations < 0 || (pb->scheme != SRCFD_SCHEME_QUICK && pb->scheme != SRCFD_SCHEME_UPWIND) ||
           (pb->case_type != SRCFD_CASE_LDC && pb->case_type != SRCFD_CASE_BFS) || (pb->case_type == SRCFD_CASE_BFS && !(pb->channel_height > 0)));
}
}  // namespace srcfd

extern "C" {

int srcfd_fine_solver_create(const srcfd_coarse_problem* problem, int device, srcfd_fine_solver** out) {
  return srcfd::abi_guard("srcfd_fine_solver_create", [&]() -> int {
    if (!problem || !out) { set_error("srcfd_fine_solver_create: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    if (!srcfd::fine_problem_ok(problem)) { set_error("srcfd_fine_solver_create: bad problem description"); return SRCFD_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("srcfd_fine_solver_create: no HIP device"); return SRCFD_ENODEV; }
    if (device < 0 || device >= ndev) { set_error("srcfd_fine_solver_create: bad device index"); return SRCFD_EINVAL; }
    std::unique_ptr<FineSolver> s(new FineSolver());
    s->pb = *problem;
    s->device = device;
    HIPCHECK(hipSetDevice(device));
    srcfd::Dev& g = s->g;
    g.nx = problem->nx; g.ny = problem->ny; g.sy = g.ny + 2; g.sx = (g.nx + 2) * (g.ny + 2);
    g.dx = problem->lx / g.nx; g.dy = problem->ly / g.ny; g.volp = g.dx * g.dy;
    g.dt = problem->dt; g.rho = problem->rho; g.nu = 1.0 / problem->reynolds;
    const size_t sx = (size_t)g.sx;
    // Var, Old, Jb (3 planes each), Ff (4), rhs (1), partials (9 nx), status
    const size_t n_f64 = 3 * sx + 3 * sx + 3 * sx + 4 * sx + sx + 9 * (size_t)g.nx;
    const size_t st_off = (n_f64 * sizeof(double) + 255) / 256 * 256;
    char* base = nullptr;
    HIPCHECK(hipMalloc(&base, st_off + sizeof(srcfd::Status)));
    s->d_mem = reinterpret_cast<double*>(base);
    double* p = s->d_mem;
    g.Var = p; p += 3 * sx;
    g.Old = p; p += 3 * sx;
    g.Jb = p; p += 3 * sx;
    g.Ff = p; p += 4 * sx;
    g.rhs = p; p += sx;
    g.part = p;
    g.st = reinterpret_cast<srcfd::Status*>(base + st_off);
    HIPCHECK(hipMemset(base, 0, st_off + sizeof(srcfd::Status)));
    HIPCHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&s->host_st), sizeof(srcfd::Status), hipHostMallocDefault));
    std::memset(s->host_st, 0, sizeof(srcfd::Status));
    *out = reinterpret_cast<srcfd_fine_solver*>(s.release());
    return SRCFD_OK;
  });
}

void srcfd_fine_solver_destroy(srcfd_fine_solver* s) { delete reinterpret_cast<FineSolver*>(s); }

int srcfd_fine_solver_init(srcfd_fine_solver* s, const double* var) {
  return srcfd::abi_guard("srcfd_fine_solver_init", [&]() -> int {
    if (!s) { set_error("srcfd_fine_solver_init: bad arguments"); return SRCFD_EINVAL; }
    FineSolver* f = reinterpret_cast<FineSolver*>(s);
    srcfd::Dev& g = f->g;
    HIPCHECK(hipSetDevice(f->device));
    const size_t bytes = 3 * (size_t)g.sx * sizeof(double);
    HIPCHECK(hipMemsetAsync(g.Ff, 0, 4 * (size_t)g.sx * sizeof(double), f->stream));
    ++f->n_launch;
    if (var) {   // staged through Jb, which every momentum solve overwrites
      HIPCHECK(hipMemcpyAsync(g.Jb, var, bytes, hipMemcpyHostToDevice, f->stream));
      hipLaunchKernelGGL(srcfd::take_interior, dim3(f->var_blocks()), dim3(srcfd::NT), 0, f->stream, g, (const double*)g.Jb);
      int rc = f->launched();
      if (rc) return rc;
    } else {
      HIPCHECK(hipMemsetAsync(g.Var, 0, bytes, f->stream));
      ++f->n_launch;
    }
    return f->prime();
  });
}

int srcfd_fine_solver_init_from_prediction(srcfd_fine_solver* s, srcfd_model* m, srcfd_resampler* r, const float* x, const float* in_affine,
                                           const float* out_affine, int flags, int64_t* n_nonfinite) {
  return srcfd::abi_guard("srcfd_fine_solver_init_from_prediction", [&]() -> int {
    if (!s || !m || !x) { set_error("srcfd_fine_solver_init_from_prediction: bad arguments"); return SRCFD_EINVAL; }
    FineSolver* f = reinterpret_cast<FineSolver*>(s);
    srcfd::Model* mm = reinterpret_cast<srcfd::Model*>(m);
    if (mm->device != f->device) { set_error("srcfd_fine_solver_init_from_prediction: model and solver are on different devices"); return SRCFD_EINVAL; }
    const srcfd::Dev& g = f->g;
    // the solver's own boundary conditions; BFS: the inlet / wall rows of u and v as left-boundary profiles (pipeline.bfs_inlet_profiles)
    srcfd_solver_bc bc[3];
    std::vector<double> prof((size_t)2 * g.ny, 0.0);
    for (int k = 0; k < 3; ++k) {
      for (int q = 0; q < 4; ++q) { bc[k].type[q] = f->pb.bc_type[k][q]; bc[k].value[q] = f->pb.bc_value[k][q]; }
      bc[k].left_profile = nullptr;
    }
    if (f->bfs()) {
      const double sh = f->pb.step_height, h = f->pb.channel_height, Ub = f->pb.bulk_velocity;
      for (int j = 1; j <= g.ny; ++j) {
        const double y = (j - 0.5) * g.dy;
        double yp = y - sh;
        if (yp < 0.0) yp = 0.0;
        if (yp > h) yp = h;
        prof[j - 1] = y < sh ? 0.0 : 6.0 * Ub * (yp / h) * (1.0 - (yp / h));
      }
      bc[0].left_profile = prof.data();
      bc[1].left_profile = prof.data() + g.ny;
    }
    HIPCHECK(hipSetDevice(f->device));
    HIPCHECK(hipStreamSynchronize(f->stream));   // the hand-off runs on the default stream
    int rc = srcfd::predict_solver_state(mm, r, x, in_affine, out_affine, bc, g.nx, g.ny, g.Var, nullptr, flags, n_nonfinite);
    if (rc) return rc;
    HIPCHECK(hipMemsetAsync(g.Ff, 0, 4 * (size_t)g.sx * sizeof(double), f->stream));
    ++f->n_launch;
    return f->prime();
  });
}

int srcfd_fine_solver_run(srcfd_fine_solver* s, int max_iterations, int* iterations, double rms[3], double* history, int history_len) {
  return srcfd::abi_guard("srcfd_fine_solver_run", [&]() -> int {
    if (!s || max_iterations < 0 || history_len < 0 || (history_len > 0 && !history)) {
      set_error("srcfd_fine_solver_run: bad arguments");
      return SRCFD_EINVAL;
    }
    FineSolver* f = reinterpret_cast<FineSolver*>(s);
    if (!f->primed) { set_error("srcfd_fine_solver_run: call srcfd_fine_solver_init first"); return SRCFD_EINVAL; }
    HIPCHECK(hipSetDevice(f->device));
    int n_hist = 0;
    for (int n = 0; n < max_iterations && !f->converged; ++n) {
      ++f->count;
      int rc = f->outer();
      if (rc) return rc;
      const srcfd::Status& st = *f->host_st;
      if (st.nonfinite) {
        f->primed = false;
        set_error("srcfd_fine_solver_run: NaN or Inf in the residuals (solver instability)");   // the reference raises ValueError here
        return SRCFD_EINVAL;
      }
      f->converged = st.converged != 0;
      if (f->count % 100 == 0 && n_hist < history_len) {   // residual_history (PyCFD_ML_accelerated.py:418-421)
        for (int k = 0; k < 3; ++k) history[3 * n_hist + k] = st.rms[k];
        ++n_hist;
      }
    }
    if (iterations) *iterations = f->count;
    if (rms) for (int k = 0; k < 3; ++k) rms[k] = f->host_st->rms[k];
    return SRCFD_OK;
  });
}

int srcfd_fine_solver_get_state(srcfd_fine_solver* s, double* var) {
  return srcfd::abi_guard("srcfd_fine_solver_get_state", [&]() -> int {
    if (!s || !var) { set_error("srcfd_fine_solver_get_state: bad arguments"); return SRCFD_EINVAL; }
    FineSolver* f = reinterpret_cast<FineSolver*>(s);
    HIPCHECK(hipSetDevice(f->device));
    HIPCHECK(hipMemcpyAsync(var, f->g.Var, 3 * (size_t)f->g.sx * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    HIPCHECK(hipStreamSynchronize(f->stream));
    return SRCFD_OK;
  });
}

int srcfd_fine_solver_counters(const srcfd_fine_solver* s, int64_t counters[4], int last_sweeps[3]) {
  return srcfd::abi_guard("srcfd_fine_solver_counters", [&]() -> int {
    if (!s) { set_error("srcfd_fine_solver_counters: bad arguments"); return SRCFD_EINVAL; }
    const FineSolver* f = reinterpret_cast<const FineSolver*>(s);
    if (counters) {
      counters[0] = f->n_mom;
      counters[1] = f->n_p;
      counters[2] = f->n_launch;
      counters[3] = f->n_sync;
    }
    if (last_sweeps) for (int k = 0; k < 3; ++k) last_sweeps[k] = f->last_sweeps[k];
    return SRCFD_OK;
  });
}

}  // extern "C"
