// Host-only walk over the basis of the direct pressure solve (sr-for-cfd_amd/csrc/poisson_plan.cpp), built with AddressSanitizer +
// UBSan by `make -C sr-for-cfd_amd/csrc poisson_plan_check`.  For n = 1 .. 70 and 400 it checks what the kernels rely on: the
// leading dimension is the next multiple of the tile and at least n; S is symmetric to the bit; every entry of the padding is +0.0
// (the kernels read whole tiles without bounds checks and take the tail of the summation index from it); the unpadded form is the
// same matrix; S S = I and the eigenvalues are those of the second-difference matrix, in long double; the refusals refuse.
// Prints the number of sizes checked; exit status 1 and a message on the first violation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sr-for-cfd_amd/csrc/poisson_plan.h"

using namespace srcfd;

static void fail(int n, const std::string& what) {
  std::fprintf(stderr, "poisson_plan_check: n %d: %s\n", n, what.c_str());
  std::exit(1);
}

static bool is_plus_zero(double v) {
  const double z = 0.0;
  return std::memcmp(&v, &z, sizeof(v)) == 0;
}

static void check(int n) {
  const int ld = poisson_ld(n);
  if (ld < n || ld % POISSON_TILE || ld - n >= POISSON_TILE) fail(n, "leading dimension " + std::to_string(ld));
  // exactly the sizes the library allocates: the sanitizer sees any write past them
  std::vector<double> S((size_t)ld * ld, -1.0), lam((size_t)n, 1.0), T((size_t)n * n, -1.0), lam2((size_t)n, 1.0);
  if (!poisson_basis(n, ld, S.data(), lam.data())) fail(n, "refused");
  if (!poisson_basis(n, n, T.data(), lam2.data())) fail(n, "the unpadded form is refused");
  for (int a = 0; a < ld; ++a)
    for (int b = 0; b < ld; ++b) {
      const double v = S[(size_t)a * ld + b];
      if (a >= n || b >= n) {
        if (!is_plus_zero(v)) fail(n, "padding at (" + std::to_string(a) + ", " + std::to_string(b) + ") is not +0.0");
        continue;
      }
      if (std::memcmp(&v, &S[(size_t)b * ld + a], sizeof(v))) fail(n, "not symmetric at (" + std::to_string(a) + ", " + std::to_string(b) + ")");
      if (std::memcmp(&v, &T[(size_t)a * n + b], sizeof(v))) fail(n, "padded and unpadded forms differ");
      if (!(std::fabs(v) <= std::sqrt(2.0 / (n + 1)) * (1.0 + 1e-15))) fail(n, "an entry above sqrt(2 / (n + 1))");
    }
  const long double u = ldexpl(1.0L, -53);
  for (int a = 0; a < n; ++a) {
    if (std::memcmp(&lam[(size_t)a], &lam2[(size_t)a], sizeof(double))) fail(n, "lambda differs between the two forms");
    if (!(lam[(size_t)a] < 0.0 && lam[(size_t)a] > -4.0)) fail(n, "lambda outside (-4, 0)");
    if (a && !(lam[(size_t)a] < lam[(size_t)a - 1])) fail(n, "lambda does not decrease");
    // S is its own inverse: entries rounded once, |s|^2 <= 2 / (n + 1), n products
    for (int b = a; b < n; ++b) {
      long double dot = 0.0L;
      for (int k = 0; k < n; ++k) dot += (long double)S[(size_t)a * ld + k] * (long double)S[(size_t)k * ld + b];
      if (fabsl(dot - (a == b ? 1.0L : 0.0L)) > 16.0L * u) fail(n, "S S - I above 16 u at (" + std::to_string(a) + ", " + std::to_string(b) + ")");
    }
    // column a of S is an eigenvector of the second-difference matrix with eigenvalue lambda[a]
    for (int i = 0; i < n; ++i) {
      const long double up = i + 1 < n ? S[(size_t)(i + 1) * ld + a] : 0.0, down = i > 0 ? S[(size_t)(i - 1) * ld + a] : 0.0;
      const long double mid = S[(size_t)i * ld + a];
      if (fabsl(up - 2.0L * mid + down - (long double)lam[(size_t)a] * mid) > 16.0L * u) fail(n, "column " + std::to_string(a) + " is no eigenvector");
    }
  }
  // null outputs are skipped, not followed
  if (!poisson_basis(n, ld, nullptr, lam.data()) || !poisson_basis(n, ld, S.data(), nullptr)) fail(n, "a null output is refused");
}

int main() {
  long checked = 0;
  for (int n = 1; n <= 70; ++n) { check(n); ++checked; }
  check(400); ++checked;
  double one = 7.0;
  if (poisson_basis(0, 32, &one, &one) || poisson_basis(-3, 32, &one, &one) || poisson_basis(5, 4, &one, &one) || one != 7.0) fail(0, "a bad size is accepted or written to");
  std::printf("%ld\n", checked);
  return 0;
}
