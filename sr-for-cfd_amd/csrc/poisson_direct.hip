// The direct pressure solve of the fine-mesh solver (fine_solver.hip, SRCFD_PRESSURE_DIRECT), float64 on the matrix cores.
//
// solve_pressure keeps the ghost ring of the pressure plane frozen for the whole inner solve, so every inner solve is a Dirichlet
// 5-point Poisson problem on the nx x ny interior,
//   volp (Dxx / dx^2 + Dyy / dy^2) p = g,     g = rhs - volp (ghost neighbours / dx^2 or dy^2),
// whatever the case type and the boundary conditions are.  The sine bases Sx, Sy (poisson_plan.h) diagonalise it:
//   p = Sx [ (Sx g Sy) / Lambda ] Sy,         Lambda[a][b] = volp (lambda_x[a] / dx^2 + lambda_y[b] / dy^2).
// That is four matrix products per case and outer iteration, evaluated left to right:
//   0:  W0 = Sx g          g is formed while the operand is staged: rhs and the frozen ghost ring are the only reads
//   1:  W1 = (W0 Sy) / Lambda    the division in the epilogue, from the case's own dx, dy, volp (the cases of a batch share nx and ny, not lx and ly)
//   2:  W0 = Sx W1
//   3:  P  = W0 Sy         stored into the interior of Var's pressure plane; ghosts, corners and the other planes are not touched;
//                          the case's p_sweeps and p_stop become 1
// W0, W1: the case's two nx x ny workspace planes.
//
// One kernel, poisson_product<MODE>.  A workgroup of four waves computes one 32 x 32 tile of the output, a wave one 16 x 16 tile on
// v_mfma_f64_16x16x4_f64.  Both operand tiles of a 32-deep chunk of the summation index go through LDS, so each element is read
// from memory once per workgroup and used by two waves; the next chunk's elements are fetched into registers while the current
// one is multiplied.  32 x 32: a single 400 x 400 case has 13 x 13 = 169 workgroups for the 256 CUs, where 64 x 64 would have 49;
// smaller tiles would halve the reuse for no more CUs than there are.  blockIdx.z is the case.
//
// Summation order.  A wave adds the index in ascending chunks of four: step s of chunk k0 contracts k = k0 + 4 s .. k0 + 4 s + 3 in
// the MFMA, accumulating into the same register.  No split, no atomics: the order depends on neither the batch size nor the tile
// position, so a case's bits do not depend on its batch.  The tail of the index is the zero padding of S (or a zero staged for an
// element outside the case's plane): adding +0.0 * +0.0 changes nothing.  Row and column tails are masked at the store.
//
// There is no numpy twin with the same bits (BLAS orders its sums otherwise); tests/test_gpu_poisson_direct.py holds this path by
// tolerance to tests/poisson_direct_ref.py.
#include <hip/hip_runtime.h>

#include "../../include/srcfd.h"
#include "fine_dev.h"
#include "poisson_plan.h"

namespace srcfd {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PT = POISSON_TILE;
constexpr int PNT = 256;
// LDS row lengths in doubles.  A is kept row-major [m][k] and read by lane (r, q) at [r][4 s + q]: 34 puts the 32 lanes of a half
// wave on 32 different bank pairs.  B is kept [k][n] and read at [4 s + q][r]: 48 shifts q = 1 by half the banks.
constexpr int LDA = PT + 2, LDB = PT + 16;
static_assert(PNT == 8 * PT && PT == 32, "the staging maps below deal 4 rows of 32 elements to each thread");

// MODE & 1 == 0: A is Sx (padded, no bounds), the summation index runs over nx.  MODE & 1 == 1: B is Sy, the index runs over ny.
template <int MODE>
__global__ void __launch_bounds__(PNT) poisson_product(BDev bd, PoissonDev pd) {
  __shared__ double As[PT * LDA], Bs[PT * LDB];
  const int cse = blockIdx.z;
  if (bd.st[cse].state != SRCFD_CASE_RUNNING) return;
  const int nx = bd.nx, ny = bd.ny, sy = bd.sy;
  const int K = (MODE & 1) ? ny : nx;
  const CaseP& cp = bd.cp[cse];
  double* const W0 = pd.work + (size_t)cse * 2 * nx * ny;
  double* const W1 = W0 + (size_t)nx * ny;
  double* const fields = bd.base + (size_t)cse * bd.stride;
  double* const P = fields + 2 * (size_t)bd.sx;           // Var's pressure plane
  const double* const rhs = fields + 13 * (size_t)bd.sx;
  const int m0 = blockIdx.y * PT, n0 = blockIdx.x * PT;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
  const int wm = (wave >> 1) * 16, wn = (wave & 1) * 16;
  const int sc = t & 31, sr = t >> 5;   // staging: this thread takes column sc of rows sr, sr + 8, sr + 16, sr + 24 of both tiles
  const double gx = cp.volp / (cp.dx * cp.dx), gy = cp.volp / (cp.dy * cp.dy);

  auto load_a = [&](int k0, double (&a)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + sr + 8 * e, k = k0 + sc;
      if (MODE == 0 || MODE == 2) {
        a[e] = pd.Sx[(size_t)m * pd.ldx + k];              // m, k < ldx: the padding is zeros
      } else {
        a[e] = (m < nx && k < ny) ? W0[(size_t)m * ny + k] : 0.0;
      }
    }
  };
  auto load_b = [&](int k0, double (&b)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + sr + 8 * e, n = n0 + sc;
      if (MODE == 1 || MODE == 3) {
        b[e] = pd.Sy[(size_t)k * pd.ldy + n];              // k, n < ldy
      } else if (MODE == 2) {
        b[e] = (k < nx && n < ny) ? W1[(size_t)k * ny + n] : 0.0;
      } else {
        // g at cell (i, j) = (k + 1, n + 1): rhs less the frozen ghost neighbours' share of the stencil
        double g = 0.0;
        if (k < nx && n < ny) {
          const int i = k + 1, j = n + 1;
          const size_t c = (size_t)i * sy + j;
          double ghost_x = 0.0, ghost_y = 0.0;
          if (i == 1) ghost_x = ghost_x + P[c - sy];
          if (i == nx) ghost_x = ghost_x + P[c + sy];
          if (j == 1) ghost_y = ghost_y + P[c - 1];
          if (j == ny) ghost_y = ghost_y + P[c + 1];
          g = rhs[c] - (gx * ghost_x + gy * ghost_y);
        }
        b[e] = g;
      }
    }
  };

  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  double ra[4], rb[4];
  load_a(0, ra);
  load_b(0, rb);
  for (int k0 = 0; k0 < K; k0 += PT) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      As[(sr + 8 * e) * LDA + sc] = ra[e];
      Bs[(sr + 8 * e) * LDB + sc] = rb[e];
    }
    __syncthreads();
    if (k0 + PT < K) {   // uniform
      load_a(k0 + PT, ra);
      load_b(k0 + PT, rb);
    }
#pragma unroll
    for (int s = 0; s < PT / 4; ++s)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(wm + r) * LDA + 4 * s + q], Bs[(4 * s + q) * LDB + wn + r], acc, 0, 0, 0);
    __syncthreads();
  }

  // D layout of v_mfma_f64_16x16x4_f64: register v of lane (r, q) is C[4 v + q][r]
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int m = m0 + wm + 4 * v + q, n = n0 + wn + r;
    if (m >= nx || n >= ny) continue;
    double c = acc[v];
    if (MODE == 1) c = c / (cp.volp * (pd.lx[m] / (cp.dx * cp.dx) + pd.ly[n] / (cp.dy * cp.dy)));
    if (MODE == 0 || MODE == 2) W0[(size_t)m * ny + n] = c;
    else if (MODE == 1) W1[(size_t)m * ny + n] = c;
    else P[(size_t)(m + 1) * sy + n + 1] = c;
  }
  if (MODE == 3 && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
    bd.st[cse].p_sweeps = 1;
    bd.st[cse].p_stop = 1;
  }
}

}  // namespace

void poisson_direct_product(int which, const BDev& bd, const PoissonDev& pd, int n_cases, hipStream_t stream) {
  const dim3 grid((unsigned)((bd.ny + PT - 1) / PT), (unsigned)((bd.nx + PT - 1) / PT), (unsigned)n_cases);
  switch (which) {
    case 0: hipLaunchKernelGGL(poisson_product<0>, grid, dim3(PNT), 0, stream, bd, pd); break;
    case 1: hipLaunchKernelGGL(poisson_product<1>, grid, dim3(PNT), 0, stream, bd, pd); break;
    case 2: hipLaunchKernelGGL(poisson_product<2>, grid, dim3(PNT), 0, stream, bd, pd); break;
    default: hipLaunchKernelGGL(poisson_product<3>, grid, dim3(PNT), 0, stream, bd, pd); break;
  }
}

}  // namespace srcfd
