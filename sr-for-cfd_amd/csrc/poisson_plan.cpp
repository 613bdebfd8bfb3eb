// The sine basis and eigenvalues of the direct pressure solve: see poisson_plan.h.  Host-only.
#include "poisson_plan.h"

#include <cmath>

namespace srcfd {

namespace {
const long double PI_L = 3.14159265358979323846264338327950288L;
}

int poisson_ld(int n) { return (n + POISSON_TILE - 1) / POISSON_TILE * POISSON_TILE; }

bool poisson_basis(int n, int ld, double* S, double* lambda) {
  if (n < 1 || ld < n) return false;
  if (S) {
    const long double scale = sqrtl(2.0L / (long double)(n + 1));
    for (size_t q = 0; q < (size_t)ld * ld; ++q) S[q] = 0.0;
    for (int a = 0; a < n; ++a)
      for (int b = a; b < n; ++b) {
        // the argument reduced to [0, 2 (n + 1)) in integers: sin(pi m / (n + 1)) has that period in m
        const long long m = ((long long)(a + 1) * (b + 1)) % (2LL * (n + 1));
        const double s = (double)(scale * sinl(PI_L * (long double)m / (long double)(n + 1)));
        S[(size_t)a * ld + b] = s;
        S[(size_t)b * ld + a] = s;
      }
  }
  if (lambda)
    for (int a = 0; a < n; ++a) {
      const long double h = sinl(PI_L * (long double)(a + 1) / (2.0L * (long double)(n + 1)));
      lambda[a] = (double)(-4.0L * h * h);
    }
  return true;
}

}  // namespace srcfd
