// g++ build of the time-to-first-binding bodies (tapqir_amd/csrc/tq_kinetics.h) on host memory, for the test suite:
// per-point likelihood terms and gradients, and a replay of the sampler (same prefix bits, same Philox uniforms).
#include "../../tapqir_amd/csrc/tq_kinetics.h"

extern "C" {

void hk_ttfb_point(const float* par, float tau, float T, int control, float* out) {
  tq_ttfb_point(par, tau, T, control, out);
}

// L[n, f] in the kernel's order: left to right per AOI
void hk_ttfb_prefix(const float* p, double* L, int N, int F) {
  for (int n = 0; n < N; ++n) {
    double acc = 0.0;
    for (int f = 0; f < F; ++f) {
      acc += tq_ttfb_log_surv_term(p[(int64_t)n * F + f]);
      L[(int64_t)n * F + f] = acc;
    }
  }
}

int hk_ttfb_search(const double* L, int F, double lu) { return tq_ttfb_search(L, F, lu); }

void hk_ttfb_sample(const double* L, float* tau, int N, int F, int S, uint64_t seed) {
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n)
      tau[(int64_t)s * N + n] = (float)tq_ttfb_search(L + (int64_t)n * F, F, tq_ttfb_log_uniform(seed, s, n));
}

double hk_log1p_det(double x) { return tq_log1p_det(x); }
}
