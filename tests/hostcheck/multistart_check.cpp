// g++ build of the side-by-side EM bodies (tapqir_amd/csrc/tq_multistart.h over tq_hmm.h) on host memory, for the test
// suite: the batched E-step with the device's ownership of frames by 64 lanes, its scan order over an array of 64 and its
// replica layout, and the batched M-step with the device's strided sums, tree and topology mask.  An inactive replica is
// skipped where the device's workgroups return.
// With -DMULTISTART_CHECK_MAIN it is a program of its own (the sanitizer run of DESIGN.md section 26).
#include "../../tapqir_amd/csrc/tq_multistart.h"

#include <vector>

namespace {

// the butterfly of tq_group_sum<64>: after the six exchanges every lane holds the sum; lane 0's is returned
double wave_sum(const double* v) {
  double a[64], b[64];
  for (int i = 0; i < 64; ++i) a[i] = v[i];
  for (int d = 1; d < 64; d <<= 1) {
    for (int i = 0; i < 64; ++i) b[i] = a[i] + a[i ^ d];
    for (int i = 0; i < 64; ++i) a[i] = b[i];
  }
  return a[0];
}

// one workgroup of tq_multistart_estep_kernel
template <int M>
void estep_row(const TqHmmModel<M>& m, const float* pr, int F, double* filt, double* row) {
  constexpr int COLS = TQ_HMM_COLS(M);
  static TqHmmMat<M> pre[64], suf[64], old[64];
  int lo[64], hi[64];
  for (int k = 0; k < 64; ++k) {
    tq_smooth_lane_range(k, F, lo[k], hi[k]);
    pre[k] = suf[k] = tq_hmm_chunk(m, pr, lo[k], hi[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {  // the kernel's Hillis-Steele steps: all lanes read, then all lanes write
    for (int k = 0; k < 64; ++k) old[k] = pre[k];
    for (int k = d; k < 64; ++k) pre[k] = tq_hmm_mul(old[k - d], old[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {
    for (int k = 0; k < 64; ++k) old[k] = suf[k];
    for (int k = 0; k + d < 64; ++k) suf[k] = tq_hmm_mul(old[k], old[k + d]);
  }
  static double acc[COLS][64];
  for (int k = 0; k < 64; ++k) {
    const TqHmmMat<M> e = k == 0 ? tq_hmm_identity<M>() : pre[k - 1];
    const TqHmmMat<M> s = k == 63 ? tq_hmm_identity<M>() : suf[k + 1];
    double v[M], b[M], a[COLS];
    tq_hmm_prefix_vector(e, v);
    tq_hmm_suffix_vector(s, b);
    tq_multistart_sweeps(m, pr, lo[k], hi[k], v, b, filt, a);
    for (int j = 0; j < COLS; ++j) acc[j][k] = a[j];
  }
  for (int j = 0; j < COLS; ++j) row[j] = wave_sum(acc[j]);
}

template <int M>
void estep(const float* p, int N, int F, const double* theta, int R, int U, double prior, const int32_t* active, double* filt,
           double* rows) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const TqHmmModel<M> m = tq_hmm_model<M>(theta + tq_multistart_theta_at<M>(r), U, prior);
    for (int n = 0; n < N; ++n)
      estep_row<M>(m, p + (int64_t)n * F, F, filt + tq_multistart_filt_at<M>(r, n, N, F), rows + tq_multistart_row_at<M>(r, n, N));
  }
}

// one workgroup of tq_multistart_mstep_kernel per replica
template <int M>
void mstep(const double* rows, int N, int R, int T, int it, uint32_t allow, const int32_t* active, double* theta,
           double* trace) {
  constexpr int COLS = TQ_HMM_COLS(M);
  static double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const double* rr = rows + tq_multistart_row_at<M>(r, 0, N);
    for (int t = 0; t < TQ_SMOOTH_MSTEP_THREADS; ++t)
      for (int j = 0; j < COLS; ++j) {
        double s = 0.0;
        for (int n = t; n < N; n += TQ_SMOOTH_MSTEP_THREADS) s += rr[(int64_t)n * COLS + j];
        part[j][t] = s;
      }
    for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1)
      for (int t = 0; t < h; ++t)
        for (int j = 0; j < COLS; ++j) part[j][t] += part[j][t + h];
    double sums[COLS];
    for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
    tq_multistart_mstep_theta<M>(sums, N, allow, theta + tq_multistart_theta_at<M>(r));
    trace[(int64_t)r * T + it] = sums[COLS - 1];
  }
}

}  // namespace

#define HK_SWITCH_M(M, ...)   \
  switch (M) {                \
    case 2: {                 \
      constexpr int MM = 2;   \
      __VA_ARGS__;            \
    } break;                  \
    case 3: {                 \
      constexpr int MM = 3;   \
      __VA_ARGS__;            \
    } break;                  \
    case 4: {                 \
      constexpr int MM = 4;   \
      __VA_ARGS__;            \
    } break;                  \
    default:                  \
      break;                  \
  }

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
