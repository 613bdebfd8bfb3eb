// What the fine-mesh solver's kernels share across translation units (fine_solver.hip, poisson_direct.hip): the per-case status
// and parameter blocks, the batch argument, and the launcher of the direct pressure solve.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace srcfd {

struct Status {      // one per case; written by the kernels with plain stores, read by the host once per chunk
  int m_sweeps, m_stop;    // current momentum solve: sweeps executed, exit rule fired
  int p_sweeps, p_stop;    // current pressure solve
  int state;               // SRCFD_CASE_*, a case that is not RUNNING is frozen
  int pad;
  double rms[3];
};

struct Bc {
  int type[4];
  double value[4];
  int bfs;
  double step_h, h, Ub;
};

struct CaseP {       // what may differ between the cases of a batch
  double dx, dy, volp, dt, rho, nu;
  double tol[3], relax[3];
  Bc bc[3];
};

struct BDev {        // the kernels' argument: the batch
  int nx, ny, sx, sy;
  size_t stride;     // doubles per case: Var, Old, Jb (3 planes each), Ff (4), rhs (1), partials (9 nx)
  double* base;
  const CaseP* cp;
  Status* st;
};
// The direct pressure solve (poisson_direct.hip): the sine bases of the batch's mesh, zero-padded to ldx and ldy (poisson_plan.h),
// their eigenvalues, and two nx x ny workspace planes per case.
struct PoissonDev {
  const double *Sx, *Sy;   // [ldx][ldx], [ldy][ldy]
  const double *lx, *ly;   // lambda of nx, of ny
  int ldx, ldy;
  double* work;            // case c's planes at work + c * 2 * nx * ny
};
// Product `which` (0 .. 3) of the solve for the n_cases cases of bd, enqueued on `stream`; a frozen case's workgroups return at once.
void poisson_direct_product(int which, const BDev& bd, const PoissonDev& pd, int n_cases, hipStream_t stream);

}  // namespace srcfd
