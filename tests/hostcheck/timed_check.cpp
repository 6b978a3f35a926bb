// g++ build of the bodies of the continuous-time hidden Markov chain (tapqir_amd/csrc/tq_timed.h) on host memory, for the
// test suite: the tables with the device's work items, the E-step with the device's ownership of frames by 64 lanes and
// its scan order over an array of 64, the M-step with the device's strided sums and tree.
// With -DTIMED_CHECK_MAIN it is a program of its own (the sanitizer run of DESIGN.md section 34).
#include <vector>

#include "../../tapqir_amd/csrc/tq_timed.h"
#include "chain_host.h"

namespace {

template <int M>
void table(const double* theta, const double* d, int D, int U, uint32_t allow, double* P, double* K) {
  const TqTimedModel<M> m = tq_timed_model<M>(theta, U, 0.5, allow);
  for (int k = 0; k < D; ++k)
    for (int ij = 0; ij < M * M; ++ij) tq_timed_table_item<M>(m, d, k, ij, P, K);
}

// tq_timed_estep_kernel: estep_row of chain_host.h given the timed chain, one workgroup per row
template <int M>
void estep(const float* p, int N, int F, const double* theta, const double* P, const double* K, const int32_t* cls, int U,
           uint32_t allow, double prior, double* filt, double* gamma, double* rows) {
  const TqTimedChain<M> m = tq_timed_chain<M>(theta, U, prior, allow, P, K, cls);
  for (int64_t n = 0; n < N; ++n) {
    const TqTimedEmit<M> em{m, p + n * F};
    if (gamma)
      estep_row<M, true>(m, em, F, filt + n * F * M, gamma + n * F * M, rows + n * TQ_HMM_COLS(M));
    else
      estep_row<M, false>(m, em, F, filt + n * F * M, nullptr, rows + n * TQ_HMM_COLS(M));
  }
}

template <int M>
double mstep(const double* rows, int N, uint32_t allow, double* theta) {
  double sums[TQ_HMM_COLS(M)];
  reduce_rows<TQ_HMM_COLS(M)>(rows, N, sums);
  tq_timed_mstep_theta<M>(sums, N, allow, theta);
  return sums[TQ_HMM_COLS(M) - 1];
}

}  // namespace

extern "C" {

void hk_timed_table(const double* theta, const double* d, int D, int U, int B, uint32_t allow, double* P, double* K) {
  HK_SWITCH_M(U + B, table<MM>(theta, d, D, U, allow, P, K));
}

// gamma may be NULL
void hk_timed_estep(const float* p, int N, int F, const double* theta, const double* P, const double* K, const int32_t* cls,
                    int U, int B, uint32_t allow, double prior, double* filt, double* gamma, double* rows) {
  HK_SWITCH_M(U + B, estep<MM>(p, N, F, theta, P, K, cls, U, allow, prior, filt, gamma, rows));
}

// theta in place; returns the summed log evidence
double hk_timed_mstep(const double* rows, int N, int U, int B, uint32_t allow, double* theta) {
  double ll = 0.0;
  HK_SWITCH_M(U + B, ll = mstep<MM>(rows, N, allow, theta));
  return ll;
}
}

#ifdef TIMED_CHECK_MAIN
#include <stdio.h>

// tables, E-step (with and without gamma) and M-step at (U, B) = (2, 2), N = 6, F = 65, D = F - 1, on heap buffers of
// exactly the documented sizes
int main() {
  const int N = 6, F = 65, D = F - 1, U = 2, B = 2, M = 4;
  const uint32_t allow = 0xFFFFu & ~(1u << (0 * M + 3));
  std::vector<float> p((size_t)N * F);
  for (int i = 0; i < N * F; ++i) p[i] = (float)((i * 37 % 101) / 100.0);
  std::vector<double> theta(M * M + M), d(D);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j < M; ++j) theta[i * M + j] = i == j ? -0.3 : 0.1;
    theta[M * M + i] = 0.25;
  }
  std::vector<int32_t> cls(F - 1);
  for (int k = 0; k < D; ++k) {
    d[k] = 0.5 + 0.07 * k;
    cls[k] = (k * 5) % D;
  }
  std::vector<double> P((size_t)D * M * M), K((size_t)D * M * M * M * M);
  hk_timed_table(theta.data(), d.data(), D, U, B, allow, P.data(), K.data());
  std::vector<double> filt((size_t)N * F * M), gamma((size_t)N * F * M), rows((size_t)N * TQ_HMM_COLS(M));
  hk_timed_estep(p.data(), N, F, theta.data(), P.data(), K.data(), cls.data(), U, B, allow, 1.0 / 3.0, filt.data(), nullptr,
                 rows.data());
  const double t0 = rows[0];
  hk_timed_estep(p.data(), N, F, theta.data(), P.data(), K.data(), cls.data(), U, B, allow, 1.0 / 3.0, filt.data(),
                 gamma.data(), rows.data());
  const double ll = hk_timed_mstep(rows.data(), N, U, B, allow, theta.data());
  printf("loglik %.6f T0 %.6f %.6f q01 %.6f q03 %.6f\n", ll, t0, rows[0], theta[1], theta[3]);
  return 0;
}
#endif
