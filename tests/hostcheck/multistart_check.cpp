// g++ build of the side-by-side EM bodies (tapqir_amd/csrc/tq_multistart.h over tq_hmm.h) on host memory, for the test
// suite: the batched E-step with the device's ownership of frames by 64 lanes, its scan order over an array of 64 and its
// replica layout, and the batched M-step with the device's strided sums, tree and topology mask.  An inactive replica is
// skipped where the device's workgroups return.
// With -DMULTISTART_CHECK_MAIN it is a program of its own (the sanitizer run of DESIGN.md section 26).
#include <vector>

#include "../../tapqir_amd/csrc/tq_multistart.h"
#include "chain_host.h"

namespace {

template <int M>
void estep(const float* p, int N, int F, const double* theta, int R, int U, double prior, const int32_t* active, double* filt,
           double* rows) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const TqHmmModel<M> m = tq_hmm_model<M>(theta + tq_multistart_theta_at<M>(r), U, prior);
    for (int n = 0; n < N; ++n)
      estep_row<M, false>(m, TqHmmEmit<M>{m, p + (int64_t)n * F}, F, filt + tq_multistart_filt_at<M>(r, n, N, F), nullptr,
                          rows + tq_multistart_row_at<M>(r, n, N));
  }
}

// one workgroup of tq_multistart_mstep_kernel per replica
template <int M>
void mstep(const double* rows, int N, int R, int T, int it, uint32_t allow, const int32_t* active, double* theta,
           double* trace) {
  constexpr int COLS = TQ_HMM_COLS(M);
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    double sums[COLS];
    reduce_rows<COLS>(rows + tq_multistart_row_at<M>(r, 0, N), N, sums);
    tq_multistart_mstep_theta<M>(sums, N, allow, theta + tq_multistart_theta_at<M>(r));
    trace[(int64_t)r * T + it] = sums[COLS - 1];
  }
}

}  // namespace

extern "C" {

// theta (R, M * M + M), filt (R, N, F, M) scratch, rows (R, N, COLS); active (R) or NULL
void hk_multistart_estep(const float* p, int N, int F, const double* theta, int R, int U, int B, double prior,
                         const int32_t* active, double* filt, double* rows) {
  HK_SWITCH_M(U + B, estep<MM>(p, N, F, theta, R, U, prior, active, filt, rows));
}

// theta (R, M * M + M) in place, trace (R, T)
void hk_multistart_mstep(const double* rows, int N, int R, int T, int it, int U, int B, uint32_t allow, const int32_t* active,
                         double* theta, double* trace) {
  HK_SWITCH_M(U + B, mstep<MM>(rows, N, R, T, it, allow, active, theta, trace));
}

int hk_multistart_allow_ok(uint32_t allow, int M) { return tq_multistart_allow_ok(allow, M) ? 1 : 0; }

// what every kernel reads theta as: A (M, M) and rho (M) of tq_hmm_model into out (M * M + M)
void hk_multistart_model(const double* theta, int U, int B, double* out) {
  HK_SWITCH_M(U + B, {
    const TqHmmModel<MM> m = tq_hmm_model<MM>(theta, U, 0.5);
    for (int i = 0; i < MM; ++i) {
      for (int j = 0; j < MM; ++j) out[i * MM + j] = m.A[i][j];
      out[MM * MM + i] = m.rho[i];
    }
  });
}
}

#ifdef MULTISTART_CHECK_MAIN
#include <stdio.h>

// R = 3, N = 6, F = 65 at (U, B) = (2, 2): three EM iterations under a mask with replica 1 frozen after the first, on heap
// buffers of exactly the documented sizes
int main() {
  const int R = 3, N = 6, F = 65, U = 2, B = 2, M = 4, T = 3;
  std::vector<float> p((size_t)N * F);
  for (int i = 0; i < N * F; ++i) p[i] = (float)((i * 37 % 101) / 100.0);
  std::vector<double> theta((size_t)R * (M * M + M));
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < M; ++i) {
      for (int j = 0; j < M; ++j) theta[r * (M * M + M) + i * M + j] = i == j ? 0.7 - 0.1 * r : 0.1 + 0.1 * r / 3.0;
      theta[r * (M * M + M) + M * M + i] = 0.25;
    }
  std::vector<double> filt((size_t)R * N * F * M), rows((size_t)R * N * TQ_HMM_COLS(M)), trace((size_t)R * T);
  std::vector<int32_t> active(R, 1);
  const uint32_t allow = 0xFFFFu & ~(1u << (1 * M + 2)) & ~(1u << (2 * M + 1));
  for (int it = 0; it < T; ++it) {
    hk_multistart_estep(p.data(), N, F, theta.data(), R, U, B, 1.0 / 3.0, active.data(), filt.data(), rows.data());
    hk_multistart_mstep(rows.data(), N, R, T, it, U, B, allow, active.data(), theta.data(), trace.data());
    active[1] = 0;
  }
  hk_multistart_estep(p.data(), N, F, theta.data(), R, U, B, 1.0 / 3.0, nullptr, filt.data(), rows.data());
  printf("trace %.6f %.6f A12 %.3g ok %d\n", trace[2], trace[2 * T + 2], theta[1 * M + 2], hk_multistart_allow_ok(allow, M));
  return 0;
}
#endif
