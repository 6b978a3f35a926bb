// g++ build of the hidden-Markov smoothing bodies (tapqir_amd/csrc/tq_smooth.h) on host memory, for the test suite: the
// E-step with the device's ownership of frames by 64 lanes and the device's scan order over an array of 64, the M-step
// with the device's strided sums and tree, the Viterbi row and the backward sampler.
#include "../../tapqir_amd/csrc/tq_smooth.h"

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

void estep_row(const TqSmoothModel& m, const float* pr, int F, double* filt, double* gam, double* row) {
  TqSmoothMat pre[64], suf[64], old[64];
  int lo[64], hi[64];
  for (int k = 0; k < 64; ++k) {
    tq_smooth_lane_range(k, F, lo[k], hi[k]);
    pre[k] = suf[k] = tq_smooth_chunk(m, pr, lo[k], hi[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {  // the kernel's Hillis-Steele steps: all lanes read, then all lanes write
    for (int k = 0; k < 64; ++k) old[k] = pre[k];
    for (int k = d; k < 64; ++k) pre[k] = tq_smooth_mul(old[k - d], old[k]);
    for (int k = 0; k < 64; ++k) old[k] = suf[k];
    for (int k = 0; k + d < 64; ++k) suf[k] = tq_smooth_mul(old[k], old[k + d]);
  }
  double acc[TQ_SMOOTH_COLS][64];
  for (int k = 0; k < 64; ++k) {
    const TqSmoothMat e = k == 0 ? tq_smooth_identity() : pre[k - 1];
    const TqSmoothMat s = k == 63 ? tq_smooth_identity() : suf[k + 1];
    double v0, v1, a[TQ_SMOOTH_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    tq_smooth_prefix_vector(e, v0, v1);
    a[4] = tq_smooth_forward(m, pr, lo[k], hi[k], v0, v1, filt, gam);
    tq_smooth_backward(m, pr, lo[k], hi[k], s.m00 + s.m01, s.m10 + s.m11, v0, v1, filt, gam, a);
    for (int j = 0; j < TQ_SMOOTH_COLS; ++j) acc[j][k] = a[j];
  }
  for (int j = 0; j < TQ_SMOOTH_COLS; ++j) row[j] = wave_sum(acc[j]);
}

}  // namespace

extern "C" {

void hk_smooth_estep(const float* p, int N, int F, const double* theta, double prior, double* filt, double* gamma,
                     double* rows) {
  const TqSmoothModel m = tq_smooth_model(theta, prior);
  for (int64_t n = 0; n < N; ++n) estep_row(m, p + n * F, F, filt + n * F, gamma + n * F, rows + n * TQ_SMOOTH_COLS);
}

// the M-step kernel: thread t sums rows t, t + 256, ...; the tree halves 256 partial sums; theta in place, returns loglik
double hk_smooth_mstep(const double* rows, int N, double* theta, double* sums) {
  static double part[TQ_SMOOTH_COLS][TQ_SMOOTH_MSTEP_THREADS];
  for (int t = 0; t < TQ_SMOOTH_MSTEP_THREADS; ++t)
    for (int j = 0; j < TQ_SMOOTH_COLS; ++j) {
      double s = 0.0;
      for (int n = t; n < N; n += TQ_SMOOTH_MSTEP_THREADS) s += rows[(int64_t)n * TQ_SMOOTH_COLS + j];
      part[j][t] = s;
    }
  for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1)
    for (int t = 0; t < h; ++t)
      for (int j = 0; j < TQ_SMOOTH_COLS; ++j) part[j][t] += part[j][t + h];
  for (int j = 0; j < TQ_SMOOTH_COLS; ++j) sums[j] = part[j][0];
  tq_smooth_mstep_theta(sums, N, theta);
  return sums[4];
}

// theta from given sums alone
void hk_smooth_mstep_theta(const double* sums, int N, double* theta) { tq_smooth_mstep_theta(sums, N, theta); }

// back: ((F + 15) / 16) * N words, the device's layout
void hk_smooth_viterbi(const float* p, int N, int F, const double* theta, double prior, uint32_t* back, uint8_t* path) {
  const TqSmoothModel m = tq_smooth_model(theta, prior);
  for (int64_t n = 0; n < N; ++n) tq_smooth_viterbi_row(m, p + n * F, F, back + n, N, path + n * F);
}

// the draws and the count of tq_smooth_count; raster (S, N, F) may be NULL.  Returns the smallest |u - q| of all draws.
double hk_smooth_count(const double* filt, const double* theta, int S, int N, int F, uint64_t seed, int32_t* counts,
                       uint8_t* raster) {
  const TqSmoothModel m = tq_smooth_model(theta, 0.5);
  double margin = 1.0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      TqPhilox ph, probe;
      tq_smooth_stream(&ph, seed, s, n);
      TqRatesRow r = {0, 0, 0, 0};
      for (int f = F - 1; f >= 0; --f) {
        double q0, q1;
        tq_smooth_thresholds(m, filt[(int64_t)n * F + f], f == F - 1, q0, q1);
        const double q = (f == F - 1 || r.prev == 0) ? q0 : q1;
        probe = ph;
        const double gap = fabs((double)tq_uniform(&probe) - q);
        if (gap < margin) margin = gap;
        const int z = tq_smooth_label(&ph, q);
        if (f == F - 1) tq_smooth_back_begin(r, z);
        else tq_smooth_back_step(r, z);
        if (raster) raster[((int64_t)s * N + n) * F + f] = (uint8_t)z;
      }
      tq_rates_finish(r, F, counts + ((int64_t)s * N + n) * TQ_RATES_COLS);
    }
  return margin;
}
}
