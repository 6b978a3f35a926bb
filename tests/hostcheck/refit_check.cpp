// g++ build of the bootstrap-refit bodies (tapqir_amd/csrc/tq_refit.h over tq_multistart.h and tq_hmm.h) on host memory,
// for the test suite: the weights of R resamples, the batched E-step that leaves out the pairs of weight 0 where the
// device's workgroups return, and the weighted M-step with the device's strided sums, tree and topology mask.
// With -DREFIT_CHECK_MAIN it is a program of its own (the sanitizer run of DESIGN.md section 33).
#include <vector>

#include "../../tapqir_amd/csrc/tq_refit.h"
#include "chain_host.h"

namespace {

template <int M>
void estep(const float* p, int N, int F, const double* theta, int R, int U, double prior, const int32_t* active,
           const int32_t* weights, double* filt, double* rows) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const TqHmmModel<M> m = tq_hmm_model<M>(theta + tq_multistart_theta_at<M>(r), U, prior);
    for (int n = 0; n < N; ++n) {
      if (weights[tq_refit_weight_at(r, n, N)] == 0) continue;
      estep_row<M, false>(m, TqHmmEmit<M>{m, p + (int64_t)n * F}, F, filt + tq_multistart_filt_at<M>(r, n, N, F), nullptr,
                          rows + tq_multistart_row_at<M>(r, n, N));
    }
  }
}

// one workgroup of tq_refit_mstep_kernel per replica: 256 threads' weighted sums, then the tree of tq_chain_reduce_rows
template <int M>
void mstep(const double* rows, const int32_t* weights, int N, int R, int T, int it, uint32_t allow, const int32_t* active,
           double* theta, double* trace) {
  constexpr int COLS = TQ_HMM_COLS(M);
  static double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  static int64_t wpart[TQ_SMOOTH_MSTEP_THREADS];
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    for (int t = 0; t < TQ_SMOOTH_MSTEP_THREADS; ++t) {
      double s[COLS];
      tq_refit_thread_sums<COLS>(rows + tq_multistart_row_at<M>(r, 0, N), weights + tq_refit_weight_at(r, 0, N), N, t,
                                 TQ_SMOOTH_MSTEP_THREADS, s, wpart[t]);
      for (int j = 0; j < COLS; ++j) part[j][t] = s[j];
    }
    for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1)
      for (int t = 0; t < h; ++t) {
        for (int j = 0; j < COLS; ++j) part[j][t] += part[j][t + h];
        wpart[t] += wpart[t + h];
      }
    double sums[COLS];
    for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
    trace[(int64_t)r * T + it] = tq_refit_mstep_theta<M>(sums, wpart[0], allow, theta + tq_multistart_theta_at<M>(r));
  }
}

}  // namespace

extern "C" {

// weights (R, N): zeroed here, as the kernel zeroes its row
void hk_refit_weights(uint64_t seed, int first, int R, int N, int32_t* weights) {
  for (int r = 0; r < R; ++r) {
    int32_t* w = weights + tq_refit_weight_at(r, 0, N);
    for (int n = 0; n < N; ++n) w[n] = 0;
    for (uint32_t i = 0; i < (uint32_t)N; ++i) w[tq_refit_draw(seed, first + r, i, (uint32_t)N)] += 1;
  }
}

// theta (R, M * M + M), filt (R, N, F, M) scratch, rows (R, N, COLS); active (R) or NULL; weights (R, N)
void hk_refit_estep(const float* p, int N, int F, const double* theta, int R, int U, int B, double prior, const int32_t* active,
                    const int32_t* weights, double* filt, double* rows) {
  HK_SWITCH_M(U + B, estep<MM>(p, N, F, theta, R, U, prior, active, weights, filt, rows));
}

// theta (R, M * M + M) in place, trace (R, T)
void hk_refit_mstep(const double* rows, const int32_t* weights, int N, int R, int T, int it, int U, int B, uint32_t allow,
                    const int32_t* active, double* theta, double* trace) {
  HK_SWITCH_M(U + B, mstep<MM>(rows, weights, N, R, T, it, allow, active, theta, trace));
}
}

#ifdef REFIT_CHECK_MAIN
#include <stdio.h>

// R = 4 (replica 0 all ones, three resamples), N = 6, F = 65 at (U, B) = (2, 2): three EM iterations under a mask with
// replica 1 frozen after the first, on heap buffers of exactly the documented sizes; rows of weight 0 are never written
int main() {
  const int R = 4, N = 6, F = 65, U = 2, B = 2, M = 4, T = 3;
  std::vector<float> p((size_t)N * F);
  for (int i = 0; i < N * F; ++i) p[i] = (float)((i * 37 % 101) / 100.0);
  std::vector<double> theta((size_t)R * (M * M + M));
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < M; ++i) {
      for (int j = 0; j < M; ++j) theta[r * (M * M + M) + i * M + j] = i == j ? 0.7 : 0.1;
      theta[r * (M * M + M) + M * M + i] = 0.25;
    }
  std::vector<int32_t> weights((size_t)R * N, 1), active(R, 1);
  hk_refit_weights(7, 0, R - 1, N, weights.data() + N);
  std::vector<double> filt((size_t)R * N * F * M), rows((size_t)R * N * TQ_HMM_COLS(M)), trace((size_t)R * T);
  const uint32_t allow = 0xFFFFu & ~(1u << (1 * M + 2)) & ~(1u << (2 * M + 1));
  for (int it = 0; it < T; ++it) {
    hk_refit_estep(p.data(), N, F, theta.data(), R, U, B, 1.0 / 3.0, active.data(), weights.data(), filt.data(), rows.data());
    hk_refit_mstep(rows.data(), weights.data(), N, R, T, it, U, B, allow, active.data(), theta.data(), trace.data());
    active[1] = 0;
  }
  int total = 0;
  for (int i = N; i < R * N; ++i) total += weights[i];
  printf("trace %.6f %.6f A12 %.3g weights %d\n", trace[2], trace[3 * T + 2], theta[1 * M + 2], total);
  return total == (R - 1) * N ? 0 : 1;
}
#endif
