// g++ build of the multi-state hidden-Markov smoothing bodies (tapqir_amd/csrc/tq_hmm.h) on host memory, for the test
// suite: the E-step with the device's ownership of frames by 64 lanes and the device's scan order over an array of 64, the
// M-step with the device's strided sums and tree, the Viterbi row, the backward sampler and the estimate.
// With -DHMM_CHECK_MAIN it is a program of its own (the sanitizer run of DESIGN.md section 22).
#include <vector>

#include "chain_host.h"

namespace {

template <int M>
void estep(const float* p, int N, int F, const double* theta, int U, double prior, double* filt, double* gamma,
           double* rows) {
  const TqHmmModel<M> m = tq_hmm_model<M>(theta, U, prior);
  for (int64_t n = 0; n < N; ++n)
    estep_row<M, true>(m, TqHmmEmit<M>{m, p + n * F}, F, filt + n * F * M, gamma + n * F * M, rows + n * TQ_HMM_COLS(M));
}

// the M-step kernel: theta in place, returns loglik
template <int M>
double mstep(const double* rows, int N, double* theta, double* sums) {
  reduce_rows<TQ_HMM_COLS(M)>(rows, N, sums);
  tq_hmm_mstep_theta<M>(sums, N, theta);
  return sums[TQ_HMM_COLS(M) - 1];
}

template <int M>
void viterbi(const float* p, int N, int F, const double* theta, int U, double prior, uint32_t* back, uint8_t* path) {
  const TqHmmModel<M> m = tq_hmm_model<M>(theta, U, prior);
  for (int64_t n = 0; n < N; ++n) tq_hmm_viterbi_row<M>(m, p + n * F, F, back + n, N, path + n * F);
}

// the draws and the counts of tq_hmm_count; trans and raster may be NULL.  Returns the smallest |u - t| of all compares.
template <int M>
double count(const double* filt, const double* theta, int U, int S, int N, int F, uint64_t seed, int32_t* counts,
             int32_t* trans, uint8_t* raster) {
  const TqHmmModel<M> m = tq_hmm_model<M>(theta, U, 0.5);
  double margin = 1.0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      TqPhilox ph;
      tq_hmm_stream(&ph, seed, s, n);
      TqRatesRow r = {0, 0, 0, 0};
      int next = 0;
      int32_t tr[M * M] = {0};
      for (int f = F - 1; f >= 0; --f) {
        double t[M * (M - 1)];
        const bool last = f == F - 1;
        tq_hmm_thresholds(m, filt + ((int64_t)n * F + f) * M, last, t);
        const double* tj = t + (last ? 0 : next) * (M - 1);
        const double u = (double)tq_uniform(&ph);
        for (int i = 0; i < M - 1; ++i) margin = fmin(margin, fabs(u - tj[i]));
        const int z = tq_hmm_label<M>(u, tj);
        const int zc = z >= U ? 1 : 0;
        if (last) {
          tq_smooth_back_begin(r, zc);
        } else {
          tq_smooth_back_step(r, zc);
          tr[z * M + next] += 1;
        }
        next = z;
        if (raster) raster[row * F + f] = (uint8_t)z;
      }
      tq_rates_finish(r, F, counts + row * TQ_RATES_COLS);
      if (trans)
        for (int k = 0; k < M * M; ++k) trans[row * (M * M) + k] = tr[k];
    }
  return margin;
}

// the sums and quotients of tq_hmm_estimate (integer sums are exact in any order)
template <int M>
void estimate(const int32_t* trans, int S, int N, int resample, uint64_t seed, int64_t* totals, double* estimand) {
  for (int s = 0; s < S; ++s) {
    int64_t t[M * M] = {0};
    for (uint32_t i = 0; i < (uint32_t)N; ++i) {
      const uint32_t k = resample ? tq_rates_index(seed, s, i, (uint32_t)N) : i;
      for (int j = 0; j < M * M; ++j) t[j] += trans[((int64_t)s * N + k) * (M * M) + j];
    }
    for (int i = 0; i < M; ++i) {
      int64_t rs = 0;
      for (int j = 0; j < M; ++j) rs += t[i * M + j];
      for (int j = 0; j < M; ++j) {
        totals[(int64_t)s * (M * M) + i * M + j] = t[i * M + j];
        estimand[(int64_t)s * (M * M) + i * M + j] = (double)t[i * M + j] / (double)rs;
      }
    }
  }
}

}  // namespace

extern "C" {

void hk_hmm_estep(const float* p, int N, int F, const double* theta, int U, int B, double prior, double* filt, double* gamma,
                  double* rows) {
  HK_SWITCH_M(U + B, estep<MM>(p, N, F, theta, U, prior, filt, gamma, rows));
}

double hk_hmm_mstep(const double* rows, int N, int U, int B, double* theta, double* sums) {
  double ll = 0.0;
  HK_SWITCH_M(U + B, ll = mstep<MM>(rows, N, theta, sums));
  return ll;
}

// theta from given sums alone
void hk_hmm_mstep_theta(const double* sums, int N, int U, int B, double* theta) {
  HK_SWITCH_M(U + B, tq_hmm_mstep_theta<MM>(sums, N, theta));
}

// back: ((F + 3) / 4) * N words, the device's layout
void hk_hmm_viterbi(const float* p, int N, int F, const double* theta, int U, int B, double prior, uint32_t* back,
                    uint8_t* path) {
  HK_SWITCH_M(U + B, viterbi<MM>(p, N, F, theta, U, prior, back, path));
}

double hk_hmm_count(const double* filt, const double* theta, int U, int B, int S, int N, int F, uint64_t seed,
                    int32_t* counts, int32_t* trans, uint8_t* raster) {
  double margin = -1.0;
  HK_SWITCH_M(U + B, margin = count<MM>(filt, theta, U, S, N, F, seed, counts, trans, raster));
  return margin;
}

void hk_hmm_estimate(const int32_t* trans, int S, int N, int U, int B, int resample, uint64_t seed, int64_t* totals,
                     double* estimand) {
  HK_SWITCH_M(U + B, estimate<MM>(trans, S, N, resample, seed, totals, estimand));
}
}

#ifdef HMM_CHECK_MAIN
#include <stdio.h>

// N = 6, F = 65, S = 70 at (U, B) = (2, 2): every body once, on heap buffers of exactly the documented sizes
int main() {
  const int N = 6, F = 65, S = 70, U = 2, B = 2, M = 4;
  std::vector<float> p((size_t)N * F);
  for (int i = 0; i < N * F; ++i) p[i] = (float)((i * 37 % 101) / 100.0);
  std::vector<double> theta(M * M + M);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j < M; ++j) theta[i * M + j] = i == j ? 0.7 : 0.1;
    theta[M * M + i] = 0.25;
  }
  std::vector<double> filt((size_t)N * F * M), gamma((size_t)N * F * M), rows((size_t)N * TQ_HMM_COLS(M)), sums(TQ_HMM_COLS(M));
  hk_hmm_estep(p.data(), N, F, theta.data(), U, B, 1.0 / 3.0, filt.data(), gamma.data(), rows.data());
  std::vector<uint32_t> back((size_t)((F + 3) / 4) * N);
  std::vector<uint8_t> path((size_t)N * F), raster((size_t)S * N * F);
  hk_hmm_viterbi(p.data(), N, F, theta.data(), U, B, 1.0 / 3.0, back.data(), path.data());
  std::vector<int32_t> counts((size_t)S * N * TQ_RATES_COLS), trans((size_t)S * N * M * M);
  const double margin = hk_hmm_count(filt.data(), theta.data(), U, B, S, N, F, 7, counts.data(), trans.data(), raster.data());
  std::vector<int64_t> totals((size_t)S * M * M);
  std::vector<double> est((size_t)S * M * M);
  hk_hmm_estimate(trans.data(), S, N, U, B, 1, 7, totals.data(), est.data());
  const double ll = hk_hmm_mstep(rows.data(), N, U, B, theta.data(), sums.data());
  printf("loglik %.6f margin %.3g A00 %.6f est00 %.6f\n", ll, margin, theta[0], est[0]);
  return 0;
}
#endif
