// g++ build of the credible-interval bodies (tapqir_amd/csrc/tq_quantile.h) on host memory, for the test suite.
#include "../../tapqir_amd/csrc/tq_quantile.h"

extern "C" {

// the kernel's element loop: tq_credible_intervals without the launch
void hq_intervals(int kind, const float* p0, const float* p1, double low, double high, double ci, double* ll, double* ul,
                  int64_t n) {
  tq_interval_args a;
  a.kind = kind, a.p0 = p0, a.p1 = p1, a.ll = ll, a.ul = ul, a.n = n, a.ci = ci, a.low = low, a.high = high;
  const double p = 0.5 * (1.0 - ci);
  for (int64_t i = 0; i < n; ++i) tq_body_interval(a, p, i);
}

void hq_igamma(double a, double y, double* P, double* Q) {
  double D;
  tq_igamma(a, tq_binet_d(a), y, P, Q, &D);
}

// xc = 1 - x is the caller's, so that (a, b, x, xc) and (b, a, xc, x) are the same point seen from both ends
void hq_ibeta(double a, double b, double x, double xc, double* P, double* Q) {
  double D;
  tq_ibeta(a, b, tq_binet_d(a + b) - tq_binet_d(a) - tq_binet_d(b), x, xc, P, Q, &D);
}
}
