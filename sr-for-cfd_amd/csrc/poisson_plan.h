// The host side of the direct pressure solve (poisson_direct.hip): the orthonormal sine basis that diagonalises the 5-point
// Dirichlet Laplacian of n interior cells along one axis, and its eigenvalues,
//   S[a][b]   = sqrt(2 / (n + 1)) sin(pi (a + 1)(b + 1) / (n + 1)),   symmetric and its own inverse (DST-I),
//   lambda[a] = -4 sin^2(pi (a + 1) / (2 (n + 1))).
// Every entry is evaluated in long double and rounded to double once; S is filled for a <= b and mirrored, so it is symmetric to the
// bit.  The kernels read S in POISSON_TILE-wide tiles without bounds checks, and take the tail of the summation index from the
// padding: S is stored [ld][ld] with ld = poisson_ld(n), every entry outside [0, n) x [0, n) a +0.0.  No HIP runtime calls, no
// kernel code; tools/poisson_plan_check.cpp walks it under the sanitizers.
#pragma once
#include <cstddef>

namespace srcfd {

constexpr int POISSON_TILE = 32;   // the tile edge of a product's output and the depth of one staged chunk of its summation index

// n rounded up to a multiple of POISSON_TILE (n >= 1)
int poisson_ld(int n);
// S [ld][ld] (ld >= n; the padding is written as zeros) and lambda [n]; either may be null.  False, with nothing written, for n < 1 or ld < n.
bool poisson_basis(int n, int ld, double* S, double* lambda);

}  // namespace srcfd
