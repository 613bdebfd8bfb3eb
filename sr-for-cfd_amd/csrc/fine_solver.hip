// Fine-mesh incompressible solver on the device (float64): the solve the SR warm start is for, for one case
// (C ABI srcfd_fine_solver_*) or for B cases of one mesh, scheme and case type in one set of launches (srcfd_fine_batch_*).
// There is one solver: a single case is a batch of one.
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
// reads the status blocks once per chunk -- never per sweep.  See DESIGN.md, "Fine-mesh solve on the device".
//
// Batches.  A Reynolds sweep of single cases leaves the device almost empty: one workgroup per mesh row and about 2 000 dependent
// launches per outer iteration, whose cost is the launch boundary and not the cell arithmetic.  The cases of a sweep share the
// mesh and the launch sequence, so they share the launches: blockIdx.y is the case, and within a case the thread-to-cell mapping,
// the expressions and the reductions do not know about the batch.  A case's bits therefore depend neither on B nor on its
// neighbours.
//
// Per-case control.  Every sweep launch covers all cases with the same sweep index m.  A case's workgroups return at once when
// that case's own stop flag is set, or when the case is frozen (converged or diverged: Status::state != 0), so each case ends
// each inner solve at its own sweep and momentum_finish picks Jb or Var by the case's own count.  The host enqueues chunks
// predicted from the largest count among the live cases, reads all B status blocks in one copy per chunk, and ends the solve
// when every live case has stopped: host synchronisations per outer iteration do not grow with B.  The live cases wait for the
// slowest inner solve of the batch -- the lock-step cost, DESIGN.md section 2c.
//
// Warm starts.  srcfd_fine_batch_init_from_prediction super-resolves the coarse fields of any subset of the cases in one prediction
// and handoff_kernel writes the result into those cases' Var; the other cases start from zero ("Warm starts").
// srcfd_fine_batch_init_from_fields_device is the same hand-off fed from a caller's device fields, and
// srcfd_fine_batch_get_fields_device (fields_kernel) returns them: DESIGN.md section 2c, "Device fields in and out".
//
// The direct pressure solve (SRCFD_PRESSURE_DIRECT, set_pressure_solver).  The ghost ring is frozen during an inner pressure solve, so
// the solve is a Dirichlet Poisson problem that the sine bases diagonalise: outer() then replaces inner(2, 2, ..) by the four matrix
// products of poisson_direct.hip -- four launches, no status read -- and everything around them stays.  Launch mode only; the default,
// SRCFD_PRESSURE_SWEEPS, is the path above with its launches and bits.  DESIGN.md section 2c, "Direct pressure solve".
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "fine_dev.h"
#include "poisson_plan.h"

namespace srcfd {

namespace {

constexpr int NT = 256;            // threads per workgroup; one workgroup per mesh row i
constexpr int SWEEP_CAP = 1000;    // inner sweeps per solve (PyCFD_ML_accelerated.py:251, 299)
constexpr double INNER_TOL = 1e-6;
constexpr int MAX_CASES = 64;      // keeps the per-chunk status read small
// A warm start predicts u, v, p of up to MAX_CASES fields in one call, which must be one staged chunk of the prediction
// (predict_solver_fields refuses anything else at run time).
static_assert(3 * MAX_CASES <= Model::STAGE_SAMPLES, "the samples of a full batch must fit one staged chunk of Model::predict_host");
static_assert(MAX_CASES <= 256, "WarmMap holds case indices in bytes");

constexpr size_t case_doubles(int nx, int ny) { return (size_t)14 * (nx + 2) * (ny + 2) + (size_t)9 * nx; }

struct Dev {         // one case's view of it (case_dev)
  int nx, ny, sx, sy;
  double dx, dy, volp, dt, rho, nu;
  double *Var, *Old, *Ff, *Jb, *rhs, *part;
  Status* st;
};

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

// ---------------------------------------------------------------- cell expressions
// One copy of every expression: the launch-per-sweep kernels and the resident kernel (below) both call these, so a cell rounds the
// same way on either path.
// apply_bc + apply_bfs_inlet of plane k at edge index t (1 .. max(nx, ny))
__device__ __forceinline__ void bc_cell(const Dev& g, const Bc& b, int k, int t) {
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

__device__ __forceinline__ void interpolation_cell(const Dev& g, int i, int j) {   // PyCFD_ML_accelerated.py:148-155
  const double* V = g.Var;
  double* F = g.Ff;
  const size_t c = (size_t)i * g.sy + j;
  F[c] = (at(g, V, 0, i, j) + at(g, V, 0, i + 1, j)) * g.dy * 0.5;
  F[g.sx + c] = (at(g, V, 1, i, j) + at(g, V, 1, i, j + 1)) * g.dx * 0.5;
  F[2 * (size_t)g.sx + c] = -(at(g, V, 0, i, j) + at(g, V, 0, i - 1, j)) * g.dy * 0.5;
  F[3 * (size_t)g.sx + c] = -(at(g, V, 1, i, j) + at(g, V, 1, i, j - 1)) * g.dx * 0.5;
}

// Ends a momentum solve of `sweeps` sweeps: the result sits in Jb when the count is odd; BFS under-relaxes against Old
// (bfs...:371-375).
__device__ __forceinline__ void finish_cell(const Dev& g, int k, int i, int j, int sweeps, int relax, double alpha) {
  const size_t c = (size_t)k * g.sx + (size_t)i * g.sy + j;
  double v = (sweeps & 1) ? g.Jb[c] : g.Var[c];
  if (relax) {
    const double o = g.Old[c];
    v = o + alpha * (v - o);
  }
  g.Var[c] = v;
}

__device__ __forceinline__ void relax_cell(const Dev& g, int k, int i, int j, double alpha) {
  const size_t c = (size_t)k * g.sx + (size_t)i * g.sy + j;
  const double o = g.Old[c];
  g.Var[c] = o + alpha * (g.Var[c] - o);
}

__device__ __forceinline__ double rhs_cell(const Dev& g, size_t c) {   // the RHS of solve_pressure: Ff is constant inside the solve
  return g.rho / g.dt * (g.Ff[c] + g.Ff[g.sx + c] + g.Ff[2 * (size_t)g.sx + c] + g.Ff[3 * (size_t)g.sx + c]);
}

__device__ __forceinline__ void flux_cell(const Dev& g, int i, int j) {   // PyCFD_ML_accelerated.py:242-249
  const double* P = g.Var + 2 * (size_t)g.sx;
  double* F = g.Ff;
  const size_t c = (size_t)i * g.sy + j;
  const double p = P[c];
  F[c] += -g.dt / g.rho * (P[c + g.sy] - p) * g.dy / g.dx;
  F[g.sx + c] += -g.dt / g.rho * (P[c + 1] - p) * g.dx / g.dy;
  F[2 * (size_t)g.sx + c] += -g.dt / g.rho * (P[c - g.sy] - p) * g.dy / g.dx;
  F[3 * (size_t)g.sx + c] += -g.dt / g.rho * (P[c - 1] - p) * g.dx / g.dy;
}

// One Jacobi update of plane k at (i, j): reads S, writes D, returns the residual R
template <bool QUICK>
__device__ __forceinline__ double momentum_cell(const Dev& g, const double* S, double* D, int k, int i, int j) {
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
  return R;
}

__device__ __forceinline__ double pressure_ap_d(const Dev& g) { return -g.volp * (2.0 / (g.dx * g.dx) + 2.0 / (g.dy * g.dy)); }
// One red-black update of the pressure plane P (global, or a copy of it in LDS) at flat index c, returns the residual R
__device__ __forceinline__ double pressure_cell(const Dev& g, double* P, const double* rhs, size_t c, double ap_d) {
  const double p = P[c];
  const double Fd = g.volp * ((P[c + g.sy] - 2.0 * p + P[c - g.sy]) / (g.dx * g.dx) + (P[c + 1] - 2.0 * p + P[c - 1]) / (g.dy * g.dy));
  const double R = rhs[c] - Fd;
  P[c] = p + R / ap_d;
  return R;
}

// correct_velocity at (i, j) (PyCFD_ML_accelerated.py:323-335); d: the changes of u, v, p against Old
__device__ __forceinline__ void correct_cell(const Dev& g, int i, int j, double d[3]) {
  const double* P = g.Var + 2 * (size_t)g.sx;
  const size_t c = (size_t)i * g.sy + j;
  const double u = g.Var[c] - g.dt / g.rho * (P[c + g.sy] - P[c - g.sy]) / (2 * g.dx);
  const double v = g.Var[g.sx + c] - g.dt / g.rho * (P[c + 1] - P[c - 1]) / (2 * g.dy);
  g.Var[c] = u;
  g.Var[g.sx + c] = v;
  d[0] = u - g.Old[c];
  d[1] = v - g.Old[g.sx + c];
  d[2] = P[c] - g.Old[2 * (size_t)g.sx + c];
}

// _convergence_check (PyCFD_ML_accelerated.py:472-505) from the three sums of squares: writes the residuals and returns the state.
// Non-finite residuals are tested first: `r > tol` is false for NaN, so the converged test alone would take a NaN for convergence.
__device__ __forceinline__ int convergence_state(const Dev& g, const CaseP& p, const double res[3], double rms[3]) {
  int conv = 1, bad = 0;
  for (int k = 0; k < 3; ++k) {
    const double r = std::sqrt(res[k] / (g.nx * g.ny)) / g.dt;
    rms[k] = r;
    if (!std::isfinite(r)) bad = 1;
    if (r > p.tol[k]) conv = 0;
  }
  return bad ? SRCFD_CASE_DIVERGED : conv ? SRCFD_CASE_CONVERGED : SRCFD_CASE_RUNNING;
}

// ---------------------------------------------------------------- boundary conditions, apply_bc + apply_bfs_inlet of plane k
__global__ void __launch_bounds__(NT) bc_kernel(BDev bd, int k) {
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  bc_cell(g, bd.cp[blockIdx.y].bc[k], k, blockIdx.x * NT + threadIdx.x + 1);
}

// ---------------------------------------------------------------- element-wise passes over the interior (one thread per cell)
__device__ __forceinline__ bool interior(const BDev& g, int& i, int& j) {
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c >= (int64_t)g.nx * g.ny) return false;
  i = (int)(c / g.ny) + 1;
  j = (int)(c - (int64_t)(i - 1) * g.ny) + 1;
  return true;
}

__global__ void __launch_bounds__(NT) linear_interpolation(BDev bd) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  interpolation_cell(case_dev(bd, blockIdx.y), i, j);
}

// Ends a momentum solve with the case's own sweep count
__global__ void __launch_bounds__(NT) momentum_finish(BDev bd, int k, int relax) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  finish_cell(g, k, i, j, g.st->m_sweeps, relax, relax ? bd.cp[blockIdx.y].relax[k] : 0.0);
}

__global__ void __launch_bounds__(NT) under_relax(BDev bd, int k) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  relax_cell(case_dev(bd, blockIdx.y), k, i, j, bd.cp[blockIdx.y].relax[k]);
}

__global__ void __launch_bounds__(NT) pressure_rhs(BDev bd) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const size_t c = (size_t)i * g.sy + j;
  g.rhs[c] = rhs_cell(g, c);
}

__global__ void __launch_bounds__(NT) update_flux(BDev bd) {
  int i, j;
  if (frozen(bd) || !interior(bd, i, j)) return;
  flux_cell(case_dev(bd, blockIdx.y), i, j);
}

// The three planes at `dst` = those at `src` (offsets in a case's block) for every case that is not frozen: the Jb copy before a
// momentum solve, and Old = Var, which a case that has just converged or diverged skips.
__global__ void __launch_bounds__(NT) copy_planes_kernel(BDev bd, size_t dst, size_t src) {
  if (frozen(bd)) return;
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  double* f = bd.base + (size_t)blockIdx.y * bd.stride;
  if (c < 3 * (int64_t)bd.sx) f[dst + c] = f[src + c];
}

// Var = 0 except the interior, which comes from Jb (where init staged the host array); ghosts and corners are left 0 for the BCs.
__global__ void __launch_bounds__(NT) take_interior(BDev bd) {
  const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (c >= 3 * (int64_t)bd.sx) return;
  double* f = bd.base + (size_t)blockIdx.y * bd.stride;
  const int r = (int)(c % bd.sx), i = r / bd.sy, j = r - i * bd.sy;
  f[c] = (i >= 1 && i <= bd.nx && j >= 1 && j <= bd.ny) ? f[6 * (size_t)bd.sx + c] : 0.0;
}

// ---------------------------------------------------------------- the SR hand-off: predicted fields into Var
// Sample s of the prediction is component s % 3 of the case map.case_of[s / 3]:  Var[k, 1+i, 1+j] = field_k[j, i]  (the reference's
// transposed injection, PyCFD_ML_accelerated.py:936-938), float64, from the network's float or the resampler's double.  One
// workgroup per 32 x 32 tile of the (nx+2) x (ny+2) plane, through LDS, so that the read runs along nx and the write along ny + 2.
// The ghost ring and the corners are written as zeros: prime() follows and sets the ring of all three planes from the interior
// and the case's own CaseP, as after take_interior.
constexpr int HT = 32;
struct WarmMap { unsigned char case_of[MAX_CASES]; };

template <typename T>
__global__ void __launch_bounds__(NT) handoff_kernel(BDev bd, const T* __restrict__ fields, WarmMap map) {
  __shared__ double tile[HT][HT + 1];   // the padding column keeps the transposed read off one bank
  const int s = blockIdx.z, k = s % 3;
  const T* f = fields + (size_t)s * bd.nx * bd.ny;
  double* V = bd.base + (size_t)map.case_of[s / 3] * bd.stride + (size_t)k * bd.sx;
  const int i0 = blockIdx.x * HT, j0 = blockIdx.y * HT;
  const int tx = threadIdx.x % HT, ty = threadIdx.x / HT;
  for (int r = ty; r < HT; r += NT / HT) {
    const int i = i0 + tx, j = j0 + r;
    if (i >= 1 && i <= bd.nx && j >= 1 && j <= bd.ny) tile[r][tx] = (double)f[(size_t)(j - 1) * bd.nx + (i - 1)];
  }
  __syncthreads();
  for (int r = ty; r < HT; r += NT / HT) {
    const int i = i0 + r, j = j0 + tx;
    if (i > bd.nx + 1 || j > bd.ny + 1) continue;
    const bool inside = i >= 1 && i <= bd.nx && j >= 1 && j <= bd.ny;
    V[(size_t)i * bd.sy + j] = inside ? tile[tx][r] : 0.0;
  }
}

// Its mirror image, Var's interior back into fields:  field_k[j, i] = Var[k, 1+i, 1+j]  for plane s = 3 q + k of the output, the
// case map.case_of[q]; float64 as it is, float32 rounded to nearest.  One workgroup per 32 x 32 tile of the nx x ny interior, through
// LDS, so that the read runs along ny and the write along nx.  The ghost ring is not read.
template <typename T>
__global__ void __launch_bounds__(NT) fields_kernel(BDev bd, T* __restrict__ fields, WarmMap map) {
  __shared__ double tile[HT][HT + 1];
  const int s = blockIdx.z, k = s % 3;
  T* f = fields + (size_t)s * bd.nx * bd.ny;
  const double* V = bd.base + (size_t)map.case_of[s / 3] * bd.stride + (size_t)k * bd.sx;
  const int i0 = blockIdx.x * HT, j0 = blockIdx.y * HT;
  const int tx = threadIdx.x % HT, ty = threadIdx.x / HT;
  for (int r = ty; r < HT; r += NT / HT) {
    const int i = i0 + r, j = j0 + tx;
    if (i < bd.nx && j < bd.ny) tile[r][tx] = V[(size_t)(i + 1) * bd.sy + (j + 1)];
  }
  __syncthreads();
  for (int r = ty; r < HT; r += NT / HT) {
    const int i = i0 + tx, j = j0 + r;
    if (i < bd.nx && j < bd.ny) f[(size_t)j * bd.nx + i] = (T)tile[tx][r];
  }
}

// ---------------------------------------------------------------- momentum: Jacobi sweep m of plane k, row blockIdx.x + 1 of case blockIdx.y
template <bool QUICK>
__global__ void __launch_bounds__(NT) momentum_sweep(BDev bd, int k, int m) {
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
    const double R = momentum_cell<QUICK>(g, S, D, k, i, j);
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
__global__ void __launch_bounds__(NT) pressure_half_sweep(BDev bd, int colour, int m) {
  __shared__ double lds[NT];
  __shared__ int flag;
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
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
  const double ap_d = pressure_ap_d(g);
  double acc = 0.0;
  for (int j = j0 + 2 * threadIdx.x; j <= g.ny; j += 2 * NT) {
    const double R = pressure_cell(g, P, g.rhs, (size_t)i * g.sy + j, ap_d);
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
__global__ void __launch_bounds__(NT) correct_velocity(BDev bd) {   // PyCFD_ML_accelerated.py:323-335
  __shared__ double lds[NT];
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  const int i = blockIdx.x + 1;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int j = 1 + threadIdx.x; j <= g.ny; j += NT) {
    double d[3];
    correct_cell(g, i, j, d);
    a0 = a0 + d[0] * d[0];
    a1 = a1 + d[1] * d[1];
    a2 = a2 + d[2] * d[2];
  }
  const double s0 = block_sum(a0, lds), s1 = block_sum(a1, lds), s2 = block_sum(a2, lds);
  if (threadIdx.x == 0) {
    double* r = res_part(g);
    r[blockIdx.x] = s0;
    r[g.nx + blockIdx.x] = s1;
    r[2 * (size_t)g.nx + blockIdx.x] = s2;
  }
}

// _convergence_check, one workgroup per case
__global__ void __launch_bounds__(NT) convergence_check(BDev bd) {
  __shared__ double lds[NT];
  if (frozen(bd)) return;
  const Dev g = case_dev(bd, blockIdx.y);
  double res[3];
  for (int k = 0; k < 3; ++k) res[k] = sum_partials(res_part(g) + (size_t)k * g.nx, g.nx, lds);
  if (threadIdx.x != 0) return;
  g.st->state = convergence_state(g, bd.cp[blockIdx.y], res, g.st->rms);
}

// ---------------------------------------------------------------- the resident path: one workgroup per case, many outer iterations per launch
// A mesh of at most RES_MAX x RES_MAX cells is small enough for one workgroup to run the whole outer loop of its case, every
// inner sweep included, with __syncthreads() where the launch boundaries of the path above are.  Workgroups never read each
// other's data, so the cases of a batch run at their own pace.  The cell expressions are the functions above; what differs is
// only how the fixed-order sums are computed ("Resident"):
//   a mesh row (pressure: a row's cells of one colour) sits in W consecutive lanes of one wave, W the power of two at or above
//   the element count, and is reduced by the halving tree v[t] += v[t + s], s = W/2 .. 1.  The spec's 256-slot tree adds only
//   zeros above W, and x + 0.0 is exact for the non-negative summands, so the bits are the spec's.  The row partials (at most
//   256) are summed by the same tree in every wave (res_sum256).  Neither depends on the number of waves.
// The momentum solves sweep the global planes.  The pressure solve holds P and rhs in LDS, which measured faster than sweeping
// the global plane at every mesh size.  RES_MAX is the largest mesh at which this path measured faster than a launch per sweep.
constexpr int RES_MAX = 64;                                   // largest nx or ny; srcfd_fine_resident_supported
constexpr int RES_NT = 512;                                   // most threads of a workgroup; the host launches fewer on small meshes
constexpr int RES_PLANE = (RES_MAX + 2) * (RES_MAX + 2);
constexpr int RES_PARTS = 4 * RES_MAX;                        // pressure [parity][colour][row]; momentum [parity][row]; residuals [k][row]
static_assert(2 * RES_MAX <= 256 && RES_MAX <= 64, "res_sum256 takes at most 256 partials, a row one element per lane");

struct ResRec {      // one per case; written by the resident kernel when it leaves a launch, read by the host with the status blocks
  int iters;               // outer iterations done in this launch
  int last[3];             // sweeps of the u, v and p solves of the last of them
  long long mom, prs;      // sweeps of this launch: momentum (u and v), pressure
};

__device__ __forceinline__ int pow2_at_least(int n) {
  int w = 1;
  while (w < n) w <<= 1;
  return w;
}
// halving tree over each aligned group of w lanes (w a power of two, at most 64): the group's lane 0 gets the sum
__device__ __forceinline__ double res_tree(double v, int w) {
  for (int s = w >> 1; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
  return v;
}
// the 256-slot tree over p[0 .. n), n <= 256; every lane of the calling wave gets the sum
__device__ __forceinline__ double res_sum256(const double* p, int n, int lane) {
  const double a0 = lane < n ? p[lane] : 0.0, a1 = lane + 64 < n ? p[lane + 64] : 0.0;
  const double a2 = lane + 128 < n ? p[lane + 128] : 0.0, a3 = lane + 192 < n ? p[lane + 192] : 0.0;
  return __shfl(res_tree((a0 + a2) + (a1 + a3), 64), 0, 64);
}

struct ResLanes {    // how a pass deals rows to waves: `rows` rows per wave, w lanes each; this lane is slot t of row `seg` of them
  int w, rows, seg, t;
};
__device__ __forceinline__ ResLanes res_lanes(int elements, int lane) {
  ResLanes m;
  m.w = elements > 32 ? 64 : pow2_at_least(elements);
  m.rows = 64 / m.w;
  m.seg = lane / m.w;
  m.t = lane - m.seg * m.w;
  return m;
}

// One pass over the mesh rows with NV sums of squares per row: cell(i, j, a) updates cell (i, j) and leaves the NV summands in a;
// part[v * nx + i - 1] receives row i's sum v.
template <int NV, class F>
__device__ __forceinline__ void res_row_pass(const Dev& g, const ResLanes& m, int wave, int nwaves, double* part, F cell) {
  for (int r0 = wave * m.rows; r0 < g.nx; r0 += nwaves * m.rows) {
    const int i = r0 + m.seg + 1;
    double a[NV];
    for (int v = 0; v < NV; ++v) a[v] = 0.0;
    if (i <= g.nx && m.t < g.ny) cell(i, m.t + 1, a);
    for (int v = 0; v < NV; ++v) {
      const double s = res_tree(a[v], m.w);
      if (m.t == 0 && i <= g.nx) part[v * g.nx + i - 1] = s;
    }
  }
}

template <bool QUICK>
__global__ void __launch_bounds__(RES_NT) resident_kernel(BDev bd, ResRec* recs, int n_it, int relax) {
  __shared__ double P[RES_PLANE], rhs[RES_PLANE], part[RES_PARTS];   // the pressure plane and its right-hand side during the pressure solve
  const int cse = blockIdx.x;
  if (bd.st[cse].state != SRCFD_CASE_RUNNING) return;
  const Dev g = case_dev(bd, cse);
  const CaseP& cp = bd.cp[cse];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthr >> 6;
  const int nx = g.nx, ny = g.ny, cells = nx * ny, edge = nx > ny ? nx : ny;
  const int plane = g.sx, planes3 = 3 * g.sx;
  const ResLanes rowmap = res_lanes(ny, lane), colmap = res_lanes((ny + 1) / 2, lane);
  double* const Pg = g.Var + 2 * (size_t)g.sx;
  const double ap_d = pressure_ap_d(g);
  int state = SRCFD_CASE_RUNNING, it = 0, sw[3] = {0, 0, 0};
  long long tot_m = 0, tot_p = 0;
  while (it < n_it && state == SRCFD_CASE_RUNNING) {
    for (int k = 0; k < 2; ++k) {
      for (int c = tid; c < planes3; c += nthr) g.Jb[c] = g.Var[c];
      __syncthreads();
      int n = 0;
      for (int m = 0; m < SWEEP_CAP; ++m) {
        if (m > 0 && std::sqrt(res_sum256(part + ((m - 1) & 1) * RES_MAX, nx, lane) / (g.nx * g.ny)) < INNER_TOL) break;
        const double* S = (m & 1) ? g.Jb : g.Var;
        double* D = (m & 1) ? g.Var : g.Jb;
        res_row_pass<1>(g, rowmap, wave, nwaves, part + (m & 1) * RES_MAX, [&](int i, int j, double* a) {
          const double R = momentum_cell<QUICK>(g, S, D, k, i, j);
          a[0] = R * R;
        });
        __syncthreads();
        n = m + 1;
      }
      sw[k] = n;
      tot_m += n;
      const double alpha = relax ? cp.relax[k] : 0.0;
      for (int c = tid; c < cells; c += nthr) finish_cell(g, k, c / ny + 1, c % ny + 1, n, relax, alpha);
      __syncthreads();
      for (int t = tid + 1; t <= edge; t += nthr) bc_cell(g, cp.bc[k], k, t);
      __syncthreads();
    }
    // linear_interpolation and pressure_rhs: a cell's rhs takes the four fluxes of that cell alone
    for (int c = tid; c < cells; c += nthr) {
      const int i = c / ny + 1, j = c % ny + 1;
      interpolation_cell(g, i, j);
      const size_t q = (size_t)i * g.sy + j;
      const double r = rhs_cell(g, q);
      g.rhs[q] = r;
      rhs[q] = r;
    }
    for (int c = tid; c < plane; c += nthr) P[c] = Pg[c];
    __syncthreads();
    {
      int n = 0;
      for (int m = 0; m < SWEEP_CAP; ++m) {
        if (m > 0 && std::sqrt(res_sum256(part + ((m - 1) & 1) * 2 * RES_MAX, 2 * nx, lane) / (g.nx * g.ny)) < INNER_TOL) break;
        for (int colour = 0; colour < 2; ++colour) {
          double* const out = part + (m & 1) * 2 * RES_MAX + colour * nx;
          for (int r0 = wave * colmap.rows; r0 < nx; r0 += nwaves * colmap.rows) {
            const int i = r0 + colmap.seg + 1;
            const int j = (((i + 1) & 1) == colour ? 1 : 2) + 2 * colmap.t;   // the t-th cell of this colour in row i
            double a = 0.0;
            if (i <= nx && j <= ny) {
              const double R = pressure_cell(g, P, rhs, (size_t)i * g.sy + j, ap_d);
              a = R * R;
            }
            a = res_tree(a, colmap.w);
            if (colmap.t == 0 && i <= nx) out[i - 1] = a;
          }
          __syncthreads();
        }
        n = m + 1;
      }
      sw[2] = n;
      tot_p += n;
    }
    for (int c = tid; c < plane; c += nthr) Pg[c] = P[c];
    __syncthreads();
    if (relax) {
      for (int c = tid; c < cells; c += nthr) relax_cell(g, 2, c / ny + 1, c % ny + 1, cp.relax[2]);
      __syncthreads();
    }
    for (int t = tid + 1; t <= edge; t += nthr) bc_cell(g, cp.bc[2], 2, t);
    __syncthreads();
    res_row_pass<3>(g, rowmap, wave, nwaves, part, [&](int i, int j, double* a) {
      double d[3];
      correct_cell(g, i, j, d);
      for (int v = 0; v < 3; ++v) a[v] = d[v] * d[v];
    });
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
      for (int t = tid + 1; t <= edge; t += nthr) bc_cell(g, cp.bc[k], k, t);
      __syncthreads();
    }
    for (int c = tid; c < cells; c += nthr) flux_cell(g, c / ny + 1, c % ny + 1);
    double res[3], rms[3];
    for (int k = 0; k < 3; ++k) res[k] = res_sum256(part + k * nx, nx, lane);
    state = convergence_state(g, cp, res, rms);
    if (tid == 0) {
      for (int k = 0; k < 3; ++k) g.st->rms[k] = rms[k];
      g.st->state = state;
    }
    ++it;
    if (state == SRCFD_CASE_RUNNING)
      for (int c = tid; c < planes3; c += nthr) g.Old[c] = g.Var[c];
    __syncthreads();
  }
  if (tid == 0) {
    ResRec& r = recs[cse];
    r.iters = it;
    for (int k = 0; k < 3; ++k) r.last[k] = sw[k];
    r.mom = tot_m;
    r.prs = tot_p;
  }
}

// The resident path's one rule, for the host and the device alike
bool resident_mesh_ok(int nx, int ny) { return nx >= 3 && ny >= 3 && nx <= RES_MAX && ny <= RES_MAX; }

// srcfd_coarse_solve's validation rules (coarse_solver.cpp)
bool fine_problem_ok(const srcfd_coarse_problem* pb) {
  return !(pb->nx < 3 || pb->ny < 3 || pb->nx > 4096 || pb->ny > 4096 || !(pb->lx > 0) || !(pb->ly > 0) || !(pb->reynolds > 0) ||
           !(pb->rho > 0) || !(pb->dt > 0) || pb->max_iterations < 0 || (pb->scheme != SRCFD_SCHEME_QUICK && pb->scheme != SRCFD_SCHEME_UPWIND) ||
           (pb->case_type != SRCFD_CASE_LDC && pb->case_type != SRCFD_CASE_BFS) || (pb->case_type == SRCFD_CASE_BFS && !(pb->channel_height > 0)));
}

}  // namespace

#define HIPCHECK_F(expr)                                    \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return hip_fail(#expr, _e);       \
  } while (0)

// The handle behind both C ABIs: srcfd_fine_batch is a FineBatch, srcfd_fine_solver a FineBatch of one case.
struct FineBatch {
  std::vector<srcfd_coarse_problem> pb;
  int n = 0, device = 0;
  BDev g{};
  PinnedBuf<char> host_mem;    // n status blocks, then n resident records: what one copy per chunk brings over
  Status* host_st = nullptr;
  const ResRec* host_rec = nullptr;
  ResRec* d_rec = nullptr;
  int mode = SRCFD_FINE_MODE_LAUNCHES;
  DevBuf<char> d_mem;
  int pressure = SRCFD_PRESSURE_SWEEPS;
  DevBuf<double> d_poisson;    // the direct pressure solve's bases, eigenvalues and workspace planes: allocated by the first switch to it
  PoissonDev pd{};
  Event arrived, written;      // a caller's stream against this handle's: its work so far (join), the fields written for it (release)
  Stream stream;               // declared last: destroyed before the memory its work uses
  size_t state_bytes = 0;      // fields and status blocks: what init clears
  int count = 0;               // outer iterations of the live cases since the last init
  bool primed = false;
  std::vector<int> state, iters, last_sweeps;   // per case; last_sweeps [n][3]
  std::vector<double> rms;                      // [n][3]
  int predict[3] = {16, 16, SWEEP_CAP};         // chunk sizes: the largest count of the previous solve + margin
  int64_t n_mom = 0, n_p = 0, n_launch = 0, n_sync = 0;

  ~FineBatch() { (void)hipSetDevice(device); }   // for the members' destructors (device_mem.h)
  bool bfs() const { return pb[0].case_type == SRCFD_CASE_BFS; }
  bool live(int c) const { return state[c] == SRCFD_CASE_RUNNING; }
  bool any_live() const {
    for (int c = 0; c < n; ++c) if (live(c)) return true;
    return false;
  }
  size_t planes() const { return 3 * (size_t)g.sx; }   // doubles in Var (or Old, or Jb) of one case
  dim3 cells_grid() const { return dim3((unsigned)(((int64_t)g.nx * g.ny + NT - 1) / NT), (unsigned)n); }
  dim3 var_grid() const { return dim3((unsigned)((3 * (int64_t)g.sx + NT - 1) / NT), (unsigned)n); }
  dim3 rows_grid() const { return dim3((unsigned)g.nx, (unsigned)n); }

  static int hip_fail(const char* what, hipError_t e) {
    set_error(std::string("fine solver: ") + what + " failed: " + hipGetErrorString(e));
    return SRCFD_EHIP;
  }

  // The problems have been validated by the caller.  One allocation: the cases' field blocks, then the status blocks, then the
  // resident records, then the parameter blocks.
  static int create(const std::string& who, const srcfd_coarse_problem* problems, int n_cases, int device, FineBatch** out) {
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
    HIPCHECK_F(hipSetDevice(device));
    BDev& g = s->g;
    g.nx = problems[0].nx; g.ny = problems[0].ny; g.sy = g.ny + 2; g.sx = (g.nx + 2) * (g.ny + 2);
    g.stride = case_doubles(g.nx, g.ny);
    std::vector<CaseP> cp((size_t)n_cases);
    for (int c = 0; c < n_cases; ++c) {
      const srcfd_coarse_problem& p = problems[c];
      CaseP& q = cp[c];
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
    s->state_bytes = field_bytes + (size_t)n_cases * (sizeof(Status) + sizeof(ResRec));
    const size_t total = s->state_bytes + (size_t)n_cases * sizeof(CaseP);
    int rc = s->d_mem.alloc(total);
    if (rc) return rc;
    char* const mem = s->d_mem.get();
    g.base = reinterpret_cast<double*>(mem);
    g.st = reinterpret_cast<Status*>(mem + field_bytes);
    s->d_rec = reinterpret_cast<ResRec*>(g.st + n_cases);
    g.cp = reinterpret_cast<const CaseP*>(mem + s->state_bytes);
    HIPCHECK_F(hipMemset(mem, 0, s->state_bytes));
    HIPCHECK_F(hipMemcpy(mem + s->state_bytes, cp.data(), cp.size() * sizeof(CaseP), hipMemcpyHostToDevice));
    HIPCHECK_F(hipStreamCreateWithFlags(s->stream.out(), hipStreamNonBlocking));
    HIPCHECK_F(hipEventCreateWithFlags(s->arrived.out(), hipEventDisableTiming));
    HIPCHECK_F(hipEventCreateWithFlags(s->written.out(), hipEventDisableTiming));
    rc = s->host_mem.alloc((size_t)n_cases * (sizeof(Status) + sizeof(ResRec)));
    if (rc) return rc;
    std::memset(s->host_mem.get(), 0, s->host_mem.size());
    s->host_st = reinterpret_cast<Status*>(s->host_mem.get());
    s->host_rec = reinterpret_cast<const ResRec*>(s->host_st + n_cases);
    *out = s.release();
    return SRCFD_OK;
  }

  int launched() {
    ++n_launch;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string("fine solver: kernel launch failed: ") + hipGetErrorString(e)); return SRCFD_EHIP; }
    return SRCFD_OK;
  }
  int sync_status(bool records = false) {   // all n status blocks (and resident records) in one copy
    ++n_sync;
    HIPCHECK_F(hipMemcpyAsync(host_st, g.st, (size_t)n * (sizeof(Status) + (records ? sizeof(ResRec) : 0)), hipMemcpyDeviceToHost, stream));
    HIPCHECK_F(hipStreamSynchronize(stream));
    return SRCFD_OK;
  }

  int bc(int k) {
    const int m = g.nx > g.ny ? g.nx : g.ny;
    hipLaunchKernelGGL(bc_kernel, dim3((m + NT - 1) / NT, n), dim3(NT), 0, stream, g, k);
    return launched();
  }
  int copy_planes(size_t dst, size_t src) {
    hipLaunchKernelGGL(copy_planes_kernel, var_grid(), dim3(NT), 0, stream, g, dst, src);
    return launched();
  }

  // Clears every case's fields, fluxes, partials and status block, so that all cases are live again -- with keep_var, all of it
  // but the Var of the cases it marks, which the caller has filled on the device.  prime() follows.
  int reset(const char* keep_var) {
    primed = false;
    if (!keep_var) {
      HIPCHECK_F(hipMemsetAsync(d_mem.get(), 0, state_bytes, stream));
      ++n_launch;
      return SRCFD_OK;
    }
    for (int c = 0; c < n; ++c) {
      const size_t kept = keep_var[c] ? planes() : 0;
      HIPCHECK_F(hipMemsetAsync(g.base + (size_t)c * g.stride + kept, 0, (g.stride - kept) * sizeof(double), stream));
      ++n_launch;
    }
    HIPCHECK_F(hipMemsetAsync(g.st, 0, (size_t)n * sizeof(Status), stream));
    ++n_launch;
    return SRCFD_OK;
  }
  int prime() {   // BCs (with the BFS inlet), Old = Var, linear_interpolation: _initialize_fields / PyCFD_ML_accelerated.py:940-953
    int rc;
    for (int k = 0; k < 3; ++k) if ((rc = bc(k))) return rc;
    if ((rc = copy_planes(planes(), 0))) return rc;
    hipLaunchKernelGGL(linear_interpolation, cells_grid(), dim3(NT), 0, stream, g);
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
  // var NULL: zero fields; otherwise the interiors of (n, 3, nx+2, ny+2), staged through each case's Jb, which every momentum
  // solve overwrites
  int init(const double* var) {
    HIPCHECK_F(hipSetDevice(device));
    int rc = reset(nullptr);
    if (rc) return rc;
    if (var) {
      for (int c = 0; c < n; ++c)
        HIPCHECK_F(hipMemcpyAsync(g.base + (size_t)c * g.stride + 2 * planes(), var + (size_t)c * planes(), planes() * sizeof(double),
                                  hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(take_interior, var_grid(), dim3(NT), 0, stream, g);
      if ((rc = launched())) return rc;
    }
    return prime();
  }

  // The case list of an entry point into map and listed[]: cases[0..count) must be distinct cases of this batch; nullptr is
  // 0, 1, .. count - 1, and with every_case_if_null only the whole batch.  `what` names the count in the message.
  int case_list(const std::string& who, const char* what, int count, const int* cases, bool every_case_if_null, WarmMap* map,
                std::vector<char>* listed) const {
    const bool must_be_all = !cases && every_case_if_null;
    if (count < 1 || count > n || (must_be_all && count != n)) {
      set_error(who + ": " + what + " " + std::to_string(count) + (must_be_all ? " without a case list is not the batch's " : " is outside 1..") + std::to_string(n));
      return SRCFD_EINVAL;
    }
    for (int w = 0; w < count; ++w) {
      const int c = cases ? cases[w] : w;
      if (c < 0 || c >= n) { set_error(who + ": cases[" + std::to_string(w) + "] = " + std::to_string(c) + " is outside 0.." + std::to_string(n - 1)); return SRCFD_EINVAL; }
      if ((*listed)[c]) { set_error(who + ": case " + std::to_string(c) + " is listed twice"); return SRCFD_EINVAL; }
      (*listed)[c] = 1;
      map->case_of[w] = (unsigned char)c;
    }
    return SRCFD_OK;
  }

  // SR of n_warm coarse fields into the Var of the cases cases[0..n_warm) (nullptr: every case, in order), zero fields for the
  // others, then prime().  The prediction runs on the default stream, so this handle's stream is drained first and the
  // prediction drains its own before the memsets and prime() follow here.
  int init_from_prediction(const std::string& who, const char* owner, Model* mm, srcfd_resampler* r, const float* x, int n_warm,
                           const int* cases, const float* in_affine, const float* out_affine, int flags, int64_t* n_nonfinite) {
    WarmMap map{};
    std::vector<char> warm((size_t)n, 0);
    int rc = case_list(who, "n_warm", n_warm, cases, true, &map, &warm);
    if (rc) return rc;
    if (mm->device != device) { set_error(who + ": model and " + owner + " are on different devices"); return SRCFD_EINVAL; }
    HIPCHECK_F(hipSetDevice(device));
    HIPCHECK_F(hipStreamSynchronize(stream));
    rc = predict_solver_fields(mm, r, x, 3 * n_warm, in_affine, out_affine, who, owner, g.nx, g.ny, flags, n_nonfinite,
                                   [&](const void* fields, bool f64, int, int) -> int {
      const dim3 grid((unsigned)((g.nx + 2 + HT - 1) / HT), (unsigned)((g.ny + 2 + HT - 1) / HT), (unsigned)(3 * n_warm));
      if (f64) hipLaunchKernelGGL(handoff_kernel<double>, grid, dim3(NT), 0, nullptr, g, static_cast<const double*>(fields), map);
      else hipLaunchKernelGGL(handoff_kernel<float>, grid, dim3(NT), 0, nullptr, g, static_cast<const float*>(fields), map);
      HIPCHECK_F(hipGetLastError());
      return SRCFD_OK;
    });
    if (rc) return rc;
    if ((rc = reset(warm.data()))) return rc;
    return prime();
  }

  // This handle's stream waits for everything enqueued on the caller's so far (join); the caller's for this handle's (release).
  int join(hipStream_t callers) {
    HIPCHECK_F(hipEventRecord(arrived, callers));
    HIPCHECK_F(hipStreamWaitEvent(stream, arrived, 0));
    return SRCFD_OK;
  }
  int release(hipStream_t callers) {
    HIPCHECK_F(hipEventRecord(written, stream));
    HIPCHECK_F(hipStreamWaitEvent(callers, written, 0));
    return SRCFD_OK;
  }

  // init_from_prediction without the network: the caller's device fields (3 n_warm planes of (h, w), float or double), through
  // r when there is one, into the Var of the listed cases; zero fields for the others; prime().  All of it on this handle's
  // stream, behind what the caller's stream holds at the call.  Everything is checked before anything is enqueued.
  int init_from_fields(const std::string& who, const char* owner, srcfd_resampler* r, const void* fields, int dtype, int n_warm,
                       const int* cases, hipStream_t callers) {
    if (dtype != SRCFD_F32 && dtype != SRCFD_F64) {
      set_error(who + ": dtype " + std::to_string(dtype) + " is neither SRCFD_F32 nor SRCFD_F64");
      return SRCFD_EINVAL;
    }
    WarmMap map{};
    std::vector<char> warm((size_t)n, 0);
    int rc = case_list(who, "n_warm", n_warm, cases, false, &map, &warm);
    if (rc) return rc;
    if (r) {
      const ResamplerGeometry q = resampler_geometry(r);
      if (q.device != device) { set_error(who + ": resampler and " + owner + " are on different devices"); return SRCFD_EINVAL; }
      if (q.out_w != g.nx || q.out_h != g.ny) {
        set_error(who + ": the resampler's output mesh (" + std::to_string(q.out_w) + " x " + std::to_string(q.out_h) + ") is not the " + owner + "'s (" +
                  std::to_string(g.nx) + " x " + std::to_string(g.ny) + ")");
        return SRCFD_EINVAL;
      }
    }
    const bool f64 = dtype == SRCFD_F64;
    HIPCHECK_F(hipSetDevice(device));
    if ((rc = join(callers))) return rc;
    if ((rc = reset(warm.data()))) return rc;
    const bool from_scratch = r != nullptr;
    if (r) {
      const double* resampled = nullptr;
      if ((rc = resample_into_scratch(r, fields, f64, 3 * n_warm, stream, &resampled))) return rc;
      fields = resampled;
    }
    const dim3 grid((unsigned)((g.nx + 2 + HT - 1) / HT), (unsigned)((g.ny + 2 + HT - 1) / HT), (unsigned)(3 * n_warm));
    if (f64 || from_scratch) hipLaunchKernelGGL(handoff_kernel<double>, grid, dim3(NT), 0, stream, g, static_cast<const double*>(fields), map);
    else hipLaunchKernelGGL(handoff_kernel<float>, grid, dim3(NT), 0, stream, g, static_cast<const float*>(fields), map);
    if ((rc = launched())) return rc;
    return prime();
  }

  // The interiors of the listed cases' Var as fields, (3 count, ny, nx) float or double on the device, behind what the caller's
  // stream holds at the call; complete at return, and the caller's stream waits for it too.
  int get_fields(const std::string& who, int count, const int* cases, void* out, int dtype, hipStream_t callers) {
    if (dtype != SRCFD_F32 && dtype != SRCFD_F64) {
      set_error(who + ": dtype " + std::to_string(dtype) + " is neither SRCFD_F32 nor SRCFD_F64");
      return SRCFD_EINVAL;
    }
    WarmMap map{};
    std::vector<char> listed((size_t)n, 0);
    int rc = case_list(who, "n", count, cases, true, &map, &listed);
    if (rc) return rc;
    HIPCHECK_F(hipSetDevice(device));
    if ((rc = join(callers))) return rc;
    const dim3 grid((unsigned)((g.nx + HT - 1) / HT), (unsigned)((g.ny + HT - 1) / HT), (unsigned)(3 * count));
    if (dtype == SRCFD_F64) hipLaunchKernelGGL(fields_kernel<double>, grid, dim3(NT), 0, stream, g, static_cast<double*>(out), map);
    else hipLaunchKernelGGL(fields_kernel<float>, grid, dim3(NT), 0, stream, g, static_cast<float*>(out), map);
    if ((rc = launched())) return rc;
    if ((rc = release(callers))) return rc;
    ++n_sync;
    HIPCHECK_F(hipStreamSynchronize(stream));
    return SRCFD_OK;
  }

  // One inner solve of every live case: chunks of sweep launches until each has stopped or the cap is reached.
  int inner(int which, int k, int64_t* executed) {
    int done = 0, chunk = predict[which], rc;
    for (;;) {
      if (chunk > SWEEP_CAP - done) chunk = SWEEP_CAP - done;
      for (int m = done; m < done + chunk; ++m) {
        if (which < 2) {
          if (pb[0].scheme == SRCFD_SCHEME_QUICK) hipLaunchKernelGGL(momentum_sweep<true>, rows_grid(), dim3(NT), 0, stream, g, k, m);
          else hipLaunchKernelGGL(momentum_sweep<false>, rows_grid(), dim3(NT), 0, stream, g, k, m);
          if ((rc = launched())) return rc;
        } else {
          for (int colour = 0; colour < 2; ++colour) {
            hipLaunchKernelGGL(pressure_half_sweep, rows_grid(), dim3(NT), 0, stream, g, colour, m);
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

  // The pressure solve of every live case as four matrix products (poisson_direct.hip): no status is read, a solve counts as one sweep.
  int direct_pressure() {
    int rc;
    for (int which = 0; which < 4; ++which) {
      poisson_direct_product(which, g, pd, n, stream);
      if ((rc = launched())) return rc;
    }
    for (int c = 0; c < n; ++c)
      if (live(c)) last_sweeps[3 * c + 2] = 1;
    n_p += 1;
    return SRCFD_OK;
  }

  // One outer iteration of every live case: _implicit_solve + _convergence_check (the order of srcfd_coarse_solve)
  int outer() {
    int rc;
    const int relax = bfs() ? 1 : 0;
    for (int k = 0; k < 2; ++k) {
      if ((rc = copy_planes(2 * planes(), 0))) return rc;
      if ((rc = inner(k, k, &n_mom))) return rc;
      hipLaunchKernelGGL(momentum_finish, cells_grid(), dim3(NT), 0, stream, g, k, relax);
      if ((rc = launched())) return rc;
      if ((rc = bc(k))) return rc;
    }
    hipLaunchKernelGGL(linear_interpolation, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(pressure_rhs, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if (pressure == SRCFD_PRESSURE_DIRECT) {
      if ((rc = direct_pressure())) return rc;
    } else if ((rc = inner(2, 2, &n_p))) {
      return rc;
    }
    if (relax) {
      hipLaunchKernelGGL(under_relax, cells_grid(), dim3(NT), 0, stream, g, 2);
      if ((rc = launched())) return rc;
    }
    if ((rc = bc(2))) return rc;
    hipLaunchKernelGGL(correct_velocity, rows_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = bc(0))) return rc;
    if ((rc = bc(1))) return rc;
    hipLaunchKernelGGL(update_flux, cells_grid(), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(convergence_check, dim3(1, n), dim3(NT), 0, stream, g);
    if ((rc = launched())) return rc;
    if ((rc = copy_planes(planes(), 0))) return rc;   // Old = Var of the cases that go on
    return sync_status();
  }

  int set_mode(const std::string& who, int m) {
    if (m != SRCFD_FINE_MODE_LAUNCHES && m != SRCFD_FINE_MODE_RESIDENT) { set_error(who + ": unknown mode " + std::to_string(m)); return SRCFD_EINVAL; }
    if (m == SRCFD_FINE_MODE_RESIDENT && !resident_mesh_ok(g.nx, g.ny)) {
      set_error(who + ": the resident mode takes meshes of at most " + std::to_string(RES_MAX) + " x " + std::to_string(RES_MAX) + " cells, not " +
                std::to_string(g.nx) + " x " + std::to_string(g.ny));
      return SRCFD_EINVAL;
    }
    if (m == SRCFD_FINE_MODE_RESIDENT && pressure == SRCFD_PRESSURE_DIRECT) {
      set_error(who + ": SRCFD_FINE_MODE_RESIDENT has no direct pressure solve, and this handle is set to SRCFD_PRESSURE_DIRECT");
      return SRCFD_EINVAL;
    }
    mode = m;
    return SRCFD_OK;
  }

  // SRCFD_PRESSURE_DIRECT: the first switch builds the bases of this mesh on the host, uploads them and allocates the two workspace
  // planes per case; a handle that never asks keeps the footprint it had.
  int set_pressure_solver(const std::string& who, int m) {
    if (m != SRCFD_PRESSURE_SWEEPS && m != SRCFD_PRESSURE_DIRECT) { set_error(who + ": unknown pressure solver " + std::to_string(m)); return SRCFD_EINVAL; }
    if (m == SRCFD_PRESSURE_DIRECT && mode == SRCFD_FINE_MODE_RESIDENT) {
      set_error(who + ": SRCFD_PRESSURE_DIRECT has no resident path, and this handle is set to SRCFD_FINE_MODE_RESIDENT");
      return SRCFD_EINVAL;
    }
    if (m == SRCFD_PRESSURE_DIRECT && !d_poisson) {
      HIPCHECK_F(hipSetDevice(device));
      const int ldx = poisson_ld(g.nx), ldy = poisson_ld(g.ny);
      const size_t n_sx = (size_t)ldx * ldx, n_sy = (size_t)ldy * ldy, n_work = (size_t)2 * n * g.nx * g.ny;
      std::vector<double> host(n_sx + n_sy + g.nx + g.ny);
      poisson_basis(g.nx, ldx, host.data(), host.data() + n_sx + n_sy);
      poisson_basis(g.ny, ldy, host.data() + n_sx, host.data() + n_sx + n_sy + g.nx);
      DevBuf<double> mem;
      int rc = mem.alloc(host.size() + n_work);
      if (rc) return rc;
      HIPCHECK_F(hipMemcpy(mem.get(), host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));   // the planes need no clearing: product 0 writes before anything reads
      d_poisson = std::move(mem);
      double* const b = d_poisson.get();
      pd.Sx = b; pd.Sy = b + n_sx; pd.lx = b + n_sx + n_sy; pd.ly = pd.lx + g.nx;
      pd.ldx = ldx; pd.ldy = ldy;
      pd.work = b + host.size();
    }
    pressure = m;
    return SRCFD_OK;
  }

  // Resident mode: up to n_it outer iterations of every live case in one launch, one workgroup per case; then one copy of the
  // status blocks and the records.  The workgroup has one wave per 128 cells: the bits do not depend on it.
  int resident_chunk(int n_it) {
    int waves = (g.nx * g.ny + 127) / 128;
    waves = waves < 1 ? 1 : waves > RES_NT / 64 ? RES_NT / 64 : waves;
    const int relax = bfs() ? 1 : 0;
    if (pb[0].scheme == SRCFD_SCHEME_QUICK) hipLaunchKernelGGL(resident_kernel<true>, dim3(n), dim3(64 * waves), 0, stream, g, d_rec, n_it, relax);
    else hipLaunchKernelGGL(resident_kernel<false>, dim3(n), dim3(64 * waves), 0, stream, g, d_rec, n_it, relax);
    int rc = launched();
    if (rc) return rc;
    return sync_status(true);
  }

  // Up to max_iterations outer iterations of the live cases; history [n][history_len][3], the other outputs per case.
  // Launch mode advances one iteration at a time; resident mode in chunks that end at the next multiple of 100 of the common
  // iteration count (where residual_history wants Status::rms) or with the budget.
  int run(int max_iterations, int* iterations, int* status, double* rms_out, double* history, int history_len) {
    HIPCHECK_F(hipSetDevice(device));
    std::vector<int> n_hist((size_t)n, 0);
    for (int left = max_iterations; left > 0 && any_live();) {
      const bool resident = mode == SRCFD_FINE_MODE_RESIDENT;
      int step = 1;
      if (resident) {
        step = 100 - count % 100;
        if (step > left) step = left;
      }
      int rc = resident ? resident_chunk(step) : outer();
      if (rc) { primed = false; return rc; }
      left -= step;
      count += step;
      int64_t most_m = 0, most_p = 0;
      for (int c = 0; c < n; ++c) {
        if (!live(c)) continue;
        const Status& st = host_st[c];
        const int did = resident ? host_rec[c].iters : step;
        if (resident) {
          for (int k = 0; k < 3; ++k) last_sweeps[3 * c + k] = host_rec[c].last[k];
          if (host_rec[c].mom > most_m) most_m = host_rec[c].mom;
          if (host_rec[c].prs > most_p) most_p = host_rec[c].prs;
        }
        iters[c] = count - step + did;
        state[c] = st.state;   // a diverged case is frozen on the device already; the others go on
        for (int k = 0; k < 3; ++k) rms[3 * c + k] = st.rms[k];
        if (did == step && count % 100 == 0 && n_hist[c] < history_len) {   // residual_history (PyCFD_ML_accelerated.py:418-421), at the case's own iterations 100, 200, ...
          for (int k = 0; k < 3; ++k) history[((size_t)c * history_len + n_hist[c]) * 3 + k] = st.rms[k];
          ++n_hist[c];
        }
      }
      n_mom += most_m;
      n_p += most_p;
    }
    for (int c = 0; c < n; ++c) {
      if (iterations) iterations[c] = iters[c];
      if (status) status[c] = state[c];
      if (rms_out) for (int k = 0; k < 3; ++k) rms_out[3 * c + k] = rms[3 * c + k];
    }
    return SRCFD_OK;
  }

  int get_state(int first, int last, double* var) {   // Var of cases [first, last)
    HIPCHECK_F(hipSetDevice(device));
    for (int c = first; c < last; ++c)
      HIPCHECK_F(hipMemcpyAsync(var + (size_t)(c - first) * planes(), g.base + (size_t)c * g.stride, planes() * sizeof(double),
                                hipMemcpyDeviceToHost, stream));
    HIPCHECK_F(hipStreamSynchronize(stream));
    return SRCFD_OK;
  }
  void counters(int64_t out[4], int* sweeps) const {
    if (out) {
      out[0] = n_mom;
      out[1] = n_p;
      out[2] = n_launch;
      out[3] = n_sync;
    }
    if (sweeps) for (int q = 0; q < 3 * n; ++q) sweeps[q] = last_sweeps[q];
  }
};
#undef HIPCHECK_F

}  // namespace srcfd

using srcfd::FineBatch;
using srcfd::set_error;

static FineBatch* batch_of(srcfd_fine_solver* s) { return reinterpret_cast<FineBatch*>(s); }
static FineBatch* batch_of(srcfd_fine_batch* b) { return reinterpret_cast<FineBatch*>(b); }

extern "C" {

// ---------------------------------------------------------------- one case: a batch of one
int srcfd_fine_solver_create(const srcfd_coarse_problem* problem, int device, srcfd_fine_solver** out) {
  return srcfd::abi_guard("srcfd_fine_solver_create", [&]() -> int {
    if (!problem || !out) { set_error("srcfd_fine_solver_create: bad arguments"); return SRCFD_EINVAL; }
    *out = nullptr;
    if (!srcfd::fine_problem_ok(problem)) { set_error("srcfd_fine_solver_create: bad problem description"); return SRCFD_EINVAL; }
    return FineBatch::create("srcfd_fine_solver_create: ", problem, 1, device, reinterpret_cast<FineBatch**>(out));
  });
}

void srcfd_fine_solver_destroy(srcfd_fine_solver* s) { delete batch_of(s); }

int srcfd_fine_solver_init(srcfd_fine_solver* s, const double* var) {
  return srcfd::abi_guard("srcfd_fine_solver_init", [&]() -> int {
    if (!s) { set_error("srcfd_fine_solver_init: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(s)->init(var);
  });
}

int srcfd_fine_solver_init_from_prediction(srcfd_fine_solver* s, srcfd_model* m, srcfd_resampler* r, const float* x, const float* in_affine,
                                           const float* out_affine, int flags, int64_t* n_nonfinite) {
  return srcfd::abi_guard("srcfd_fine_solver_init_from_prediction", [&]() -> int {
    if (!s || !m || !x) { set_error("srcfd_fine_solver_init_from_prediction: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(s)->init_from_prediction("srcfd_fine_solver_init_from_prediction", "solver", reinterpret_cast<srcfd::Model*>(m), r, x, 1,
                                             nullptr, in_affine, out_affine, flags, n_nonfinite);
  });
}

int srcfd_fine_solver_init_from_fields_device(srcfd_fine_solver* s, srcfd_resampler* r, const void* fields_dev, int dtype, void* stream) {
  return srcfd::abi_guard("srcfd_fine_solver_init_from_fields_device", [&]() -> int {
    if (!s || !fields_dev) { set_error("srcfd_fine_solver_init_from_fields_device: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(s)->init_from_fields("srcfd_fine_solver_init_from_fields_device", "solver", r, fields_dev, dtype, 1, nullptr,
                                         reinterpret_cast<hipStream_t>(stream));
  });
}

int srcfd_fine_solver_get_fields_device(srcfd_fine_solver* s, void* out_dev, int dtype, void* stream) {
  return srcfd::abi_guard("srcfd_fine_solver_get_fields_device", [&]() -> int {
    if (!s || !out_dev) { set_error("srcfd_fine_solver_get_fields_device: bad arguments"); return SRCFD_EINVAL; }
    if (!batch_of(s)->primed) { set_error("srcfd_fine_solver_get_fields_device: call srcfd_fine_solver_init first"); return SRCFD_EINVAL; }
    return batch_of(s)->get_fields("srcfd_fine_solver_get_fields_device", 1, nullptr, out_dev, dtype, reinterpret_cast<hipStream_t>(stream));
  });
}

int srcfd_fine_solver_run(srcfd_fine_solver* s, int max_iterations, int* iterations, double rms[3], double* history, int history_len) {
  return srcfd::abi_guard("srcfd_fine_solver_run", [&]() -> int {
    if (!s || max_iterations < 0 || history_len < 0 || (history_len > 0 && !history)) {
      set_error("srcfd_fine_solver_run: bad arguments");
      return SRCFD_EINVAL;
    }
    FineBatch* f = batch_of(s);
    if (!f->primed) { set_error("srcfd_fine_solver_run: call srcfd_fine_solver_init first"); return SRCFD_EINVAL; }
    int it = 0, status = SRCFD_CASE_RUNNING;
    double r[3];
    int rc = f->run(max_iterations, &it, &status, r, history, history_len);
    if (rc) return rc;
    if (status == SRCFD_CASE_DIVERGED) {
      f->primed = false;
      set_error("srcfd_fine_solver_run: NaN or Inf in the residuals (solver instability)");   // the reference raises ValueError here
      return SRCFD_EINVAL;
    }
    if (iterations) *iterations = it;
    if (rms) for (int k = 0; k < 3; ++k) rms[k] = r[k];
    return SRCFD_OK;
  });
}

int srcfd_fine_solver_get_state(srcfd_fine_solver* s, double* var) {
  return srcfd::abi_guard("srcfd_fine_solver_get_state", [&]() -> int {
    if (!s || !var) { set_error("srcfd_fine_solver_get_state: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(s)->get_state(0, 1, var);
  });
}

int srcfd_fine_solver_counters(const srcfd_fine_solver* s, int64_t counters[4], int last_sweeps[3]) {
  return srcfd::abi_guard("srcfd_fine_solver_counters", [&]() -> int {
    if (!s) { set_error("srcfd_fine_solver_counters: bad arguments"); return SRCFD_EINVAL; }
    reinterpret_cast<const FineBatch*>(s)->counters(counters, last_sweeps);
    return SRCFD_OK;
  });
}

int srcfd_fine_solver_set_mode(srcfd_fine_solver* s, int mode) {
  return srcfd::abi_guard("srcfd_fine_solver_set_mode", [&]() -> int {
    if (!s) { set_error("srcfd_fine_solver_set_mode: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(s)->set_mode("srcfd_fine_solver_set_mode", mode);
  });
}

int srcfd_fine_solver_set_pressure_solver(srcfd_fine_solver* s, int solver) {
  return srcfd::abi_guard("srcfd_fine_solver_set_pressure_solver", [&]() -> int {
    if (!s) { set_error("srcfd_fine_solver_set_pressure_solver: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(s)->set_pressure_solver("srcfd_fine_solver_set_pressure_solver", solver);
  });
}

// ---------------------------------------------------------------- the direct pressure solve's basis (host-only: poisson_plan.cpp)
int srcfd_poisson_basis(int n, double* S, double* lambda) {
  return srcfd::abi_guard("srcfd_poisson_basis", [&]() -> int {
    if (n < 1) { set_error("srcfd_poisson_basis: n " + std::to_string(n) + " is below 1"); return SRCFD_EINVAL; }
    srcfd::poisson_basis(n, n, S, lambda);
    return SRCFD_OK;
  });
}

// ---------------------------------------------------------------- batches
int srcfd_fine_resident_supported(int nx, int ny) { return srcfd::resident_mesh_ok(nx, ny) ? 1 : 0; }

int srcfd_fine_batch_set_mode(srcfd_fine_batch* b, int mode) {
  return srcfd::abi_guard("srcfd_fine_batch_set_mode", [&]() -> int {
    if (!b) { set_error("srcfd_fine_batch_set_mode: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(b)->set_mode("srcfd_fine_batch_set_mode", mode);
  });
}

int srcfd_fine_batch_set_pressure_solver(srcfd_fine_batch* b, int solver) {
  return srcfd::abi_guard("srcfd_fine_batch_set_pressure_solver", [&]() -> int {
    if (!b) { set_error("srcfd_fine_batch_set_pressure_solver: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(b)->set_pressure_solver("srcfd_fine_batch_set_pressure_solver", solver);
  });
}

int srcfd_fine_batch_footprint(int nx, int ny, int n_cases, int64_t* device_bytes) {
  return srcfd::abi_guard("srcfd_fine_batch_footprint", [&]() -> int {
    if (!device_bytes || nx < 3 || ny < 3 || nx > 4096 || ny > 4096 || n_cases < 1 || n_cases > srcfd::MAX_CASES) {
      set_error("srcfd_fine_batch_footprint: bad arguments");
      return SRCFD_EINVAL;
    }
    *device_bytes = (int64_t)n_cases * (int64_t)(srcfd::case_doubles(nx, ny) * sizeof(double) + sizeof(srcfd::Status) + sizeof(srcfd::ResRec) + sizeof(srcfd::CaseP));
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
    return FineBatch::create(who, problems, n_cases, device, reinterpret_cast<FineBatch**>(out));
  });
}

void srcfd_fine_batch_destroy(srcfd_fine_batch* b) { delete batch_of(b); }

int srcfd_fine_batch_init(srcfd_fine_batch* b, const double* var) {
  return srcfd::abi_guard("srcfd_fine_batch_init", [&]() -> int {
    if (!b) { set_error("srcfd_fine_batch_init: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(b)->init(var);
  });
}

int srcfd_fine_batch_init_from_prediction(srcfd_fine_batch* b, srcfd_model* m, srcfd_resampler* r, const float* x, int n_warm,
                                          const int* cases, const float* in_affine, const float* out_affine, int flags,
                                          int64_t* n_nonfinite) {
  return srcfd::abi_guard("srcfd_fine_batch_init_from_prediction", [&]() -> int {
    if (!b || !m || !x) { set_error("srcfd_fine_batch_init_from_prediction: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(b)->init_from_prediction("srcfd_fine_batch_init_from_prediction", "batch", reinterpret_cast<srcfd::Model*>(m), r, x, n_warm,
                                             cases, in_affine, out_affine, flags, n_nonfinite);
  });
}

int srcfd_fine_batch_init_from_fields_device(srcfd_fine_batch* b, srcfd_resampler* r, const void* fields_dev, int dtype, int n_warm,
                                             const int* cases, void* stream) {
  return srcfd::abi_guard("srcfd_fine_batch_init_from_fields_device", [&]() -> int {
    if (!b || !fields_dev) { set_error("srcfd_fine_batch_init_from_fields_device: bad arguments"); return SRCFD_EINVAL; }
    return batch_of(b)->init_from_fields("srcfd_fine_batch_init_from_fields_device", "batch", r, fields_dev, dtype, n_warm, cases,
                                         reinterpret_cast<hipStream_t>(stream));
  });
}

int srcfd_fine_batch_get_fields_device(srcfd_fine_batch* b, int n, const int* cases, void* out_dev, int dtype, void* stream) {
  return srcfd::abi_guard("srcfd_fine_batch_get_fields_device", [&]() -> int {
    if (!b || !out_dev) { set_error("srcfd_fine_batch_get_fields_device: bad arguments"); return SRCFD_EINVAL; }
    if (!batch_of(b)->primed) { set_error("srcfd_fine_batch_get_fields_device: call srcfd_fine_batch_init first"); return SRCFD_EINVAL; }
    return batch_of(b)->get_fields("srcfd_fine_batch_get_fields_device", n, cases, out_dev, dtype, reinterpret_cast<hipStream_t>(stream));
  });
}

int srcfd_fine_batch_run(srcfd_fine_batch* b, int max_iterations, int* iterations, int* status, double* rms, double* history,
                         int history_len) {
  return srcfd::abi_guard("srcfd_fine_batch_run", [&]() -> int {
    if (!b || max_iterations < 0 || history_len < 0 || (history_len > 0 && !history)) {
      set_error("srcfd_fine_batch_run: bad arguments");
      return SRCFD_EINVAL;
    }
    if (!batch_of(b)->primed) { set_error("srcfd_fine_batch_run: call srcfd_fine_batch_init first"); return SRCFD_EINVAL; }
    return batch_of(b)->run(max_iterations, iterations, status, rms, history, history_len);
  });
}

int srcfd_fine_batch_get_state(srcfd_fine_batch* b, int case_index, double* var) {
  return srcfd::abi_guard("srcfd_fine_batch_get_state", [&]() -> int {
    FineBatch* f = batch_of(b);
    if (!b || !var || case_index < -1 || case_index >= f->n) { set_error("srcfd_fine_batch_get_state: bad arguments"); return SRCFD_EINVAL; }
    return case_index < 0 ? f->get_state(0, f->n, var) : f->get_state(case_index, case_index + 1, var);
  });
}

int srcfd_fine_batch_counters(const srcfd_fine_batch* b, int64_t counters[4], int* last_sweeps) {
  return srcfd::abi_guard("srcfd_fine_batch_counters", [&]() -> int {
    if (!b) { set_error("srcfd_fine_batch_counters: bad arguments"); return SRCFD_EINVAL; }
    reinterpret_cast<const FineBatch*>(b)->counters(counters, last_sweeps);
    return SRCFD_OK;
  });
}

}  // extern "C"
