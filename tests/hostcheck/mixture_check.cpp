// g++ build of the mixture-of-chains bodies (tapqir_amd/csrc/tq_mixture.h over tq_multistart.h and tq_hmm.h) on host
// memory, for the test suite: the batched E-step of multistart_check.cpp with R = P * G, the weighted M-step with the
// device's strided ownership of the AOIs, its order of populations and its tree, the sampler that draws a population with
// every raster, and the per-population estimate.  An inactive start is skipped where the device's workgroup returns.
// With -DMIXTURE_CHECK_MAIN it is a program of its own (the sanitizer run of DESIGN.md section 29).
#include <vector>

#include "../../tapqir_amd/csrc/tq_mixture.h"
#include "chain_host.h"

namespace {

template <int M>
void estep(const float* p, int N, int F, const double* theta, int R, int U, double prior, const int32_t* active, int G,
           double* filt, double* rows) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r / G] == 0) continue;
    const TqHmmModel<M> m = tq_hmm_model<M>(theta + tq_multistart_theta_at<M>(r), U, prior);
    for (int n = 0; n < N; ++n)
      estep_row<M, false>(m, TqHmmEmit<M>{m, p + (int64_t)n * F}, F, filt + tq_multistart_filt_at<M>(r, n, N, F), nullptr,
                          rows + tq_multistart_row_at<M>(r, n, N));
  }
}

// one workgroup of tq_mixture_mstep_kernel per start: thread t owns rows t, t + 256, ...; the columns are the M * M + M
// weighted sums, then sum w, then sum ev; the tree is reduce_rows' of chain_host.h on one more column
template <int M>
void mstep(const double* rows_all, int N, int P, int G, int T, int it, uint32_t allow, const int32_t* active, double* theta,
           double* phi_all, double* trace, double* resp, double* evidence) {
  constexpr int COLS = TQ_HMM_COLS(M), W = M * M + M, TH = TQ_SMOOTH_MSTEP_THREADS;
  static double part[COLS + 1][TH];
  for (int p = 0; p < P; ++p) {
    if (active && active[p] == 0) continue;
    const double* rows = rows_all + tq_multistart_row_at<M>(tq_mixture_replica(p, 0, G), 0, N);
    const int64_t stride = (int64_t)N * COLS;
    double lphi[TQ_MIXTURE_MAX_POP], wsum[TQ_MIXTURE_MAX_POP];
    tq_mixture_log_weights(phi_all + (int64_t)p * G, G, lphi);
    for (int g = 0; g < G; ++g) {
      for (int t = 0; t < TH; ++t) {
        double s[COLS + 1];
        for (int j = 0; j < COLS + 1; ++j) s[j] = 0.0;
        for (int n = t; n < N; n += TH) {
          double w[TQ_MIXTURE_MAX_POP];
          const double ev = tq_mixture_evidence(rows + (int64_t)n * COLS + COLS - 1, stride, lphi, G, w);
          const double wg = tq_mixture_pick(w, g);
          const double* row = rows + g * stride + (int64_t)n * COLS;
          for (int j = 0; j < W; ++j) s[j] += wg * row[j];
          s[W] += wg;
          s[COLS] += ev;
          if (g == 0) {
            if (evidence) evidence[(int64_t)p * N + n] = ev;
            if (resp)
              for (int k = 0; k < G; ++k) resp[((int64_t)p * G + k) * N + n] = w[k];
          }
        }
        for (int j = 0; j < COLS + 1; ++j) part[j][t] = s[j];
      }
      for (int h = TH / 2; h > 0; h >>= 1)
        for (int t = 0; t < h; ++t)
          for (int j = 0; j < COLS + 1; ++j) part[j][t] += part[j][t + h];
      double sums[W];
      for (int j = 0; j < W; ++j) sums[j] = part[j][0];
      wsum[g] = part[W][0];
      tq_mixture_mstep_theta<M>(sums, wsum[g], allow, theta + tq_multistart_theta_at<M>(tq_mixture_replica(p, g, G)));
      if (g == 0) trace[(int64_t)p * T + it] = part[COLS][0];
    }
    tq_mixture_mstep_phi(wsum, G, N, phi_all + (int64_t)p * G);
  }
}

// the draws and the counts of tq_mixture_count; trans and raster may be NULL.  margins[0]: the smallest |u - tail| of the
// population draws, margins[1]: the smallest |u - t| of the state draws.
template <int M>
void count(const double* filt, const double* theta, const double* resp, int U, int G, int S, int N, int F, uint64_t seed,
           int32_t* counts, int32_t* trans, uint8_t* pop, uint8_t* raster, double* margins) {
  TqHmmModel<M> mods[TQ_MIXTURE_MAX_POP];
  for (int g = 0; g < G; ++g) mods[g] = tq_hmm_model<M>(theta + tq_multistart_theta_at<M>(g), U, 0.5);
  margins[0] = margins[1] = 1.0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      const int g = tq_mixture_population(seed, s, n, resp + n, N, G);
      {
        TqPhilox ph;
        tq_philox_init(&ph, seed, (uint32_t)s, TQ_MIXTURE_SITE, (uint64_t)n);
        const double u = (double)tq_uniform(&ph);
        double tail = 0.0;
        for (int k = G - 1; k >= 1; --k) {
          tail += resp[(int64_t)k * N + n];
          margins[0] = fmin(margins[0], fabs(u - tail));
        }
      }
      const double* fr = filt + tq_multistart_filt_at<M>(g, n, N, F);
      TqPhilox ph;
      tq_hmm_stream(&ph, seed, s, n);
      TqRatesRow r = {0, 0, 0, 0};
      int next = 0;
      int32_t tr[M * M] = {0};
      for (int f = F - 1; f >= 0; --f) {
        double t[M * (M - 1)];
        const bool last = f == F - 1;
        tq_hmm_thresholds(mods[g], fr + (int64_t)f * M, last, t);
        const double* tj = t + (last ? 0 : next) * (M - 1);
        const double u = (double)tq_uniform(&ph);
        for (int i = 0; i < M - 1; ++i) margins[1] = fmin(margins[1], fabs(u - tj[i]));
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
      pop[row] = (uint8_t)g;
      if (trans)
        for (int k = 0; k < M * M; ++k) trans[row * (M * M) + k] = tr[k];
    }
}

// the sums and quotients of tq_mixture_estimate (integer sums are exact in any order)
template <int M>
void estimate(const int32_t* trans, const uint8_t* pop, int S, int N, int G, int resample, uint64_t seed, int64_t* totals,
              int64_t* members, double* estimand) {
  for (int s = 0; s < S; ++s)
    for (int g = 0; g < G; ++g) {
      int64_t t[M * M] = {0}, cnt = 0;
      for (uint32_t i = 0; i < (uint32_t)N; ++i) {
        const uint32_t k = resample ? tq_rates_index(seed, s, i, (uint32_t)N) : i;
        if ((int)pop[(int64_t)s * N + k] != g) continue;
        for (int j = 0; j < M * M; ++j) t[j] += trans[((int64_t)s * N + k) * (M * M) + j];
        cnt += 1;
      }
      const int64_t at = ((int64_t)s * G + g) * (M * M);
      members[(int64_t)s * G + g] = cnt;
      for (int i = 0; i < M; ++i) {
        int64_t rs = 0;
        for (int j = 0; j < M; ++j) rs += t[i * M + j];
        for (int j = 0; j < M; ++j) {
          totals[at + i * M + j] = t[i * M + j];
          estimand[at + i * M + j] = (double)t[i * M + j] / (double)rs;
        }
      }
    }
}

}  // namespace

extern "C" {

// theta (P * G, M * M + M), filt (P * G, N, F, M) scratch, rows (P * G, N, COLS); active (P) or NULL
void hk_mixture_estep(const float* p, int N, int F, const double* theta, int P, int G, int U, int B, double prior,
                      const int32_t* active, double* filt, double* rows) {
  HK_SWITCH_M(U + B, estep<MM>(p, N, F, theta, P * G, U, prior, active, G, filt, rows));
}

// theta (P, G, M * M + M) and phi (P, G) in place, trace (P, T); resp (P, G, N) and evidence (P, N) may be NULL
void hk_mixture_mstep(const double* rows, int N, int P, int G, int T, int it, int U, int B, uint32_t allow,
                      const int32_t* active, double* theta, double* phi, double* trace, double* resp, double* evidence) {
  HK_SWITCH_M(U + B, mstep<MM>(rows, N, P, G, T, it, allow, active, theta, phi, trace, resp, evidence));
}

void hk_mixture_count(const double* filt, const double* theta, const double* resp, int U, int B, int G, int S, int N, int F,
                      uint64_t seed, int32_t* counts, int32_t* trans, uint8_t* pop, uint8_t* raster, double* margins) {
  HK_SWITCH_M(U + B, count<MM>(filt, theta, resp, U, G, S, N, F, seed, counts, trans, pop, raster, margins));
}

void hk_mixture_estimate(const int32_t* trans, const uint8_t* pop, int S, int N, int G, int U, int B, int resample,
                         uint64_t seed, int64_t* totals, int64_t* members, double* estimand) {
  HK_SWITCH_M(U + B, estimate<MM>(trans, pop, S, N, G, resample, seed, totals, members, estimand));
}
}

#ifdef MIXTURE_CHECK_MAIN
#include <stdio.h>

// P = 2, G = 3, N = 6, F = 65 at (U, B) = (2, 2): three EM iterations under a mask with start 1 frozen after the first, then
// one sampler call and one estimate on the populations of start 0, on heap buffers of exactly the documented sizes
int main() {
  const int P = 2, G = 3, N = 6, F = 65, U = 2, B = 2, M = 4, T = 3, S = 70, R = P * G, W = M * M + M;
  std::vector<float> p((size_t)N * F);
  for (int i = 0; i < N * F; ++i) p[i] = (float)((i * 37 % 101) / 100.0);
  std::vector<double> theta((size_t)R * W), phi((size_t)P * G, 1.0 / G);
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < M; ++i) {
      for (int j = 0; j < M; ++j) theta[r * W + i * M + j] = i == j ? 0.85 - 0.1 * r : 0.05 + 0.1 * r / 3.0;
      theta[r * W + M * M + i] = 0.25;
    }
  std::vector<double> filt((size_t)R * N * F * M), rows((size_t)R * N * TQ_HMM_COLS(M)), trace((size_t)P * T);
  std::vector<double> resp((size_t)P * G * N), evidence((size_t)P * N);
  std::vector<int32_t> active(P, 1);
  const uint32_t allow = 0xFFFFu & ~(1u << (1 * M + 2)) & ~(1u << (2 * M + 1));
  for (int it = 0; it < T; ++it) {
    hk_mixture_estep(p.data(), N, F, theta.data(), P, G, U, B, 1.0 / 3.0, active.data(), filt.data(), rows.data());
    hk_mixture_mstep(rows.data(), N, P, G, T, it, U, B, allow, active.data(), theta.data(), phi.data(), trace.data(),
                     resp.data(), evidence.data());
    active[1] = 0;
  }
  hk_mixture_estep(p.data(), N, F, theta.data(), P, G, U, B, 1.0 / 3.0, nullptr, filt.data(), rows.data());
  std::vector<int32_t> counts((size_t)S * N * TQ_RATES_COLS), trans((size_t)S * N * M * M);
  std::vector<uint8_t> pop((size_t)S * N), raster((size_t)S * N * F);
  std::vector<double> filt0(filt.begin(), filt.begin() + (size_t)G * N * F * M), theta0(theta.begin(), theta.begin() + G * W);
  std::vector<double> resp0(resp.begin(), resp.begin() + (size_t)G * N);
  double margins[2];
  hk_mixture_count(filt0.data(), theta0.data(), resp0.data(), U, B, G, S, N, F, 7, counts.data(), trans.data(), pop.data(),
                   raster.data(), margins);
  std::vector<int64_t> totals((size_t)S * G * M * M), members((size_t)S * G);
  std::vector<double> est((size_t)S * G * M * M);
  hk_mixture_estimate(trans.data(), pop.data(), S, N, G, U, B, 1, 7, totals.data(), members.data(), est.data());
  printf("trace %.6f %.6f phi %.4f %.4f %.4f A12 %.3g margins %.3g %.3g members %lld\n", trace[2], trace[T], phi[0], phi[1],
         phi[2], theta[1 * M + 2], margins[0], margins[1], (long long)members[0]);
  return 0;
}
#endif
