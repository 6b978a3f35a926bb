// tq_mixture.h -- a mixture of G chains of tq_hmm.h over the AOIs (`smooth --populations G`),
// host+device inline bodies, templated on the number of states M = U + B in {2, 3, 4}:
//   * where population g of start p keeps its theta, its rows and its responsibilities: replica r = p * G + g of
//     tq_multistart.h, so that the E-step is tq_multistart_estep as it stands;
//   * the weights phi as they are read, the evidence and the responsibilities of one AOI from its G logliks;
//   * the M-step of one population from its weighted sums under the topology mask;
//   * the sampler's draw of an AOI's population;
//   * where the interior-run histograms of a sample's population start (tq_population_dwell).
// With G = 1 every body reduces to its single-chain counterpart bit for bit: phi reads as 1, its logarithm is 0, the
// evidence is L + 0, the responsibility exp(0) / 1, and a product with 1.0 is exact, fused or not.
// The __global__ wrappers are in tq_mixture.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "tq_multistart.h"

#define TQ_MIXTURE_SITE 0xA05u  // Philox site id of the population draw: stream (seed, step = s, site, elem = n)

// ---- layout -----------------------------------------------------------------------------------------------------------
TQ_HD int tq_mixture_replica(int p, int g, int G) { return p * G + g; }

// ---- weights, evidence, responsibilities ------------------------------------------------------------------------------
// lphi[g] = log of phi floored at TQ_SMOOTH_RMIN and renormalised, as every reader of phi takes it
TQ_HD void tq_mixture_log_weights(const double* phi, int G, double* lphi) {
  double f[TQ_MIXTURE_MAX_POP], s = 0.0;
#pragma unroll
  for (int g = 0; g < TQ_MIXTURE_MAX_POP; ++g)
    if (g < G) {
      f[g] = fmax(phi[g], TQ_SMOOTH_RMIN);
      s += f[g];
    }
#pragma unroll
  for (int g = 0; g < TQ_MIXTURE_MAX_POP; ++g) lphi[g] = g < G ? log(f[g] / s) : 0.0;
}

// ev = log sum_g phi_g e^{L_g} as max + log sum exp(. - max), g ascending, and w[g] = the share of population g in that
// sum: exp(log phi_g + L_g - ev), taken as the term over the sum so that its error does not grow with |ev| and the w of an
// AOI sum to 1 within the rounding of G quotients.  L_g = rows[g * stride]: the loglik column of the AOI's row of
// population g.
TQ_HD double tq_mixture_evidence(const double* L, int64_t stride, const double* lphi, int G, double* w) {
  double a[TQ_MIXTURE_MAX_POP], mx = 0.0, s = 0.0;
#pragma unroll
  for (int g = 0; g < TQ_MIXTURE_MAX_POP; ++g)
    if (g < G) {
      a[g] = lphi[g] + L[g * stride];
      mx = g == 0 ? a[0] : fmax(mx, a[g]);
    }
#pragma unroll
  for (int g = 0; g < TQ_MIXTURE_MAX_POP; ++g) {
    w[g] = g < G ? exp(a[g] - mx) : 0.0;
    if (g < G) s += w[g];
  }
#pragma unroll
  for (int g = 0; g < TQ_MIXTURE_MAX_POP; ++g) w[g] /= s;
  return mx + log(s);
}

// x[g] of an array of TQ_MIXTURE_MAX_POP kept in registers
TQ_HD double tq_mixture_pick(const double* x, int g) { return g == 0 ? x[0] : g == 1 ? x[1] : g == 2 ? x[2] : x[3]; }

// ---- M-step -----------------------------------------------------------------------------------------------------------
// theta of one population from its weighted sums: sums[0 .. M * M + M) = sum_n w E n_ij and sum_n w gamma_0, wsum = sum_n w.
// The forbidden sums are zeroed and A comes out of tq_hmm_mstep_theta's quotients and floor, as in
// tq_multistart_mstep_theta; rho divides by wsum where that divides by N.  wsum = 0 (no AOI has any share): theta stays.
template <int M>
TQ_HD void tq_mixture_mstep_theta(const double* sums, double wsum, uint32_t allow, double* theta) {
  if (!(wsum > 0.0)) return;
  double q[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s[M], rs = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      s[j] = ((allow >> (i * M + j)) & 1u) == 0u ? 0.0 : sums[i * M + j];
      rs += s[j];
    }
    if (rs > 0.0) {
#pragma unroll
      for (int j = 0; j < M; ++j) q[j] = s[j] / rs;
      tq_hmm_floor<M>(q, theta + i * M);
    }
  }
#pragma unroll
  for (int i = 0; i < M; ++i) q[i] = sums[M * M + i] / wsum;
  tq_hmm_floor<M>(q, theta + M * M);
}

// phi = wsum / N, floored at TQ_SMOOTH_RMIN and renormalised
TQ_HD void tq_mixture_mstep_phi(const double* wsum, int G, int N, double* phi) {
  double f[TQ_MIXTURE_MAX_POP], s = 0.0;
  for (int g = 0; g < G; ++g) {
    f[g] = fmax(wsum[g] / (double)N, TQ_SMOOTH_RMIN);
    s += f[g];
  }
  for (int g = 0; g < G; ++g) phi[g] = f[g] / s;
}

// ---- sampler ----------------------------------------------------------------------------------------------------------
// The population of row (s, n): the first uniform of its own stream against the tails of resp[., n] (stride N), the
// convention of tq_hmm_label: the largest g with u < sum_{g' >= g} resp[g'], or 0.  G = 1 compares nothing.
TQ_HD int tq_mixture_population(uint64_t seed, int s, int n, const double* resp, int64_t stride, int G) {
  TqPhilox ph;
  tq_philox_init(&ph, seed, (uint32_t)s, TQ_MIXTURE_SITE, (uint64_t)n);
  const double u = (double)tq_uniform(&ph);
  double tail = 0.0;
  int pop = 0;
  for (int g = G - 1; g >= 1; --g) {
    tail += resp[g * stride];
    if (pop == 0 && u < tail) pop = g;
  }
  return pop;
}

// ---- sampler walked into intervals (tq_population_dwell) -------------------------------------------
// The draws are tq_mixture_population and then TqHmmDraws / tq_hmm_thresholds / tq_hmm_label under theta_g, the walk is
// TqChainDwellRow / tq_chain_dwell_frame / tq_chain_dwell_finish of tq_hmm.h; only the layout is new: the F bins of sample
// s and drawn population g in histograms of shape (S, G, F).
TQ_HD int64_t tq_population_hist_at(int s, int g, int G, int F) { return ((int64_t)s * G + g) * F; }
