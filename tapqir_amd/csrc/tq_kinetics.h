// tq_kinetics.h -- time-to-first-binding kinetics (tapqir `ttfb`, tapqir/main.py:926-1147), host+device inline bodies:
//   * the first-binding sampler: tau = first frame f with z_f = 1 under the factorised posterior q(z), drawn by inverting
//     the survival function P(tau > f) = prod_{j <= f} (1 - p_j) (tapqir/utils/imscroll.py:187-196 of z_sample draws);
//   * the censored two-exponential MLE of Friedman & Gelles (2015) that tapqir/utils/mle_analysis.py:11-105 fits with
//     pyro SVI + TraceEnum_ELBO + Adam, one independent 3-parameter fit per posterior sample.
// The __global__ wrappers are in tq_kinetics.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "../../include/tapqir_hip.h"
#include "tq_fit.h"
#include "tq_math.h"

#define TQ_TTFB_SITE 0xA00u  // Philox site id of the sampler's uniforms: stream (seed, step = s, site, elem = n)

// ---- deterministic double logarithm -----------------------------------------------------------------------------------
// log1p(x), x >= -1, from correctly rounded IEEE operations only (+, *, /, fma, bit moves): a g++ build and the gfx950
// build give the same bits, so a host replay of the sampler reproduces tau exactly.  Every multiply-add is an explicit
// fma() (hipcc would contract a * b + c on its own, g++ on x86-64 would not).  Relative error ~1e-16.
TQ_HD double tq_log1p_det(double x) {
  if (x == 0.0) return x;
  if (x <= -1.0) return x == -1.0 ? -INFINITY : NAN;
  const double w = 1.0 + x;
  const double corr = (fabs(x) < 0.5) ? (x - (w - 1.0)) / w : 0.0;  // what the rounding of 1 + x lost, to first order
  union { double d; long long i; } u;
  u.d = w;
  int e = (int)((u.i >> 52) & 0x7ff) - 1023;
  u.i = (u.i & 0x000fffffffffffffLL) | 0x3ff0000000000000LL;
  double m = u.d;  // w = m 2^e, m in [1, 2)  ->  [sqrt(1/2), sqrt(2))
  if (m > 1.41421356237309504880) {
    m *= 0.5;
    e += 1;
  }
  const double s = (m - 1.0) / (m + 1.0);  // ln m = 2 atanh(s), |s| <= 0.1716
  const double s2 = s * s;
  double p = 1.0 / 25.0;
  p = fma(p, s2, 1.0 / 23.0);
  p = fma(p, s2, 1.0 / 21.0);
  p = fma(p, s2, 1.0 / 19.0);
  p = fma(p, s2, 1.0 / 17.0);
  p = fma(p, s2, 1.0 / 15.0);
  p = fma(p, s2, 1.0 / 13.0);
  p = fma(p, s2, 1.0 / 11.0);
  p = fma(p, s2, 1.0 / 9.0);
  p = fma(p, s2, 1.0 / 7.0);
  p = fma(p, s2, 1.0 / 5.0);
  p = fma(p, s2, 1.0 / 3.0);
  const double lnm = fma(2.0 * s * s2, p, 2.0 * s);
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  return fma((double)e, ln2_hi, fma((double)e, ln2_lo, lnm) + corr);
}

// ---- first-binding sampler ------------------------------------------------------------------------------------------
// L[f] = sum_{j <= f} log1p(-p_j), left to right in double: log P(tau > f) under q.  p_j = 1 gives -inf from there on.
TQ_HD double tq_ttfb_log_surv_term(float p) { return tq_log1p_det(-(double)p); }

// first f in [0, F) with L[f] < lu, or F (binary search; L is non-increasing)
TQ_HD int tq_ttfb_search(const double* L, int F, double lu) {
  int lo = 0, hi = F;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (L[mid] < lu) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// log u of the uniform of sample s, AOI n: tau = first f with P(tau > f) < u, so P(tau = f) = S_{f-1} - S_f = S_{f-1} p_f
TQ_HD double tq_ttfb_log_uniform(uint64_t seed, int s, int n) {
  TqPhilox ph;
  tq_philox_init(&ph, seed, (uint32_t)s, TQ_TTFB_SITE, (uint64_t)n);
  const float u = tq_uniform(&ph);       // in (0, 1), 24 random bits
  return tq_log1p_det((double)u - 1.0);  // u - 1 is exact in double
}

// ---- censored two-exponential MLE -----------------------------------------------------------------------------------
// Unconstrained parameters p = (log ka, log kns, logit Af) (pyro constraints.positive / unit_interval).  With
// k0 = kns, k1 = ka + kns, la = log Af, lb = log(1 - Af), the log-likelihood of one sample (mle_analysis.py:49-101) is
//   0 < tau < T : logaddexp(la + ln k1 - k1 tau, lb + ln k0 - k0 tau) = lb + ln k0 - k0 tau + softplus(d),
//                 d = c + ln(k1 / k0) - ka tau                        (la - lb = c exactly)
//   tau == T    : logaddexp(la - k1 T, lb - k0 T)                     = lb - k0 T + softplus(c - ka T)
//   tau == 0    : 0 (the enumerated Bernoulli sums to one)
//   control     : 0 < tauc < T: ln kns - kns tauc;  tauc == T: -kns T
// The gradient needs, per step, only two data sums over the uncensored points: W1 = sum w1, W1tau = sum w1 tau with
// w1 = sigmoid(d) the posterior weight of the "active" component; the other sums are constants of the data.
struct TqTtfbK {
  float ka, kns, Af;    // constrained values
  float rk1;            // 1 / (ka + kns)
  float lk0, lr10;      // ln k0, ln(k1 / k0) = softplus(log ka - log kns)
  float la, lb, c;      // ln Af, ln(1 - Af), logit Af
  float base;           // c + ln(k1 / k0): d = base - ka tau
};

TQ_HD TqTtfbK tq_ttfb_consts(float lka, float lkns, float c) {
  TqTtfbK k;
  k.ka = tq_fit_exp(lka);  // the gradient sets k sum tau against counts: see tq_fit_exp
  k.kns = tq_fit_exp(lkns);
  k.Af = tq_sigmoid(c);
  k.rk1 = 1.0f / (k.ka + k.kns);
  k.lk0 = lkns;
  k.lr10 = tq_softplus(lka - lkns);
  k.la = -tq_softplus(-c);
  k.lb = -tq_softplus(c);
  k.c = c;
  k.base = c + k.lr10;
  return k;
}

// data constants of one sample (counts and sums of the classified points)
struct TqTtfbData {
  float n_int, sum_tau;    // 0 < tau < T
  float n_cens;            // tau == T
  float nc_int, sum_tauc;  // control, 0 < tauc < T
  float nc_cens;           // control, tauc == T
  float T;
};

// per-point work of a step: accumulate w1 and w1 tau of an uncensored point (and softplus(d) for the loss)
TQ_HD void tq_ttfb_accumulate(const TqTtfbK& k, float tau, float& W1, float& W1tau) {
  const float w1 = tq_sigmoid(fmaf(-k.ka, tau, k.base));
  W1 += w1;
  W1tau = fmaf(w1, tau, W1tau);
}
TQ_HD float tq_ttfb_softplus_d(const TqTtfbK& k, float tau) { return tq_softplus(fmaf(-k.ka, tau, k.base)); }

// gradient of the LOSS (= -log-likelihood, what Adam descends) w.r.t. (log ka, log kns, logit Af)
TQ_HD void tq_ttfb_grad(const TqTtfbK& k, const TqTtfbData& d, float W1, float W1tau, float g[3]) {
  const float w1c = tq_sigmoid(fmaf(-k.ka, d.T, k.c));  // censored points: d = c - ka T
  // uncensored: d/dlog ka = ka (W1 / k1 - W1tau); d/dlog kns = kns W1 / k1 + (n - W1) - kns sum tau; d/dc = W1 - n Af
  // censored:   -ka T n w1c;                      -kns T n;                               n (w1c - Af)
  // control:                                     nc - kns (sum tauc + T ncc)
  const float ga = k.ka * (W1 * k.rk1 - W1tau) - k.ka * d.T * d.n_cens * w1c;
  const float gb = k.kns * W1 * k.rk1 + (d.n_int - W1) - k.kns * d.sum_tau - k.kns * d.T * d.n_cens + d.nc_int -
                   k.kns * (d.sum_tauc + d.T * d.nc_cens);
  const float gc = (W1 - d.n_int * k.Af) + d.n_cens * (w1c - k.Af);
  g[0] = -ga;
  g[1] = -gb;
  g[2] = -gc;
}

// loss (= -log-likelihood) of one sample; SP = sum of softplus(d) over the uncensored points
TQ_HD float tq_ttfb_loss(const TqTtfbK& k, const TqTtfbData& d, float SP) {
  const float kns = k.kns;
  const float ll = d.n_int * (k.lb + k.lk0) - kns * d.sum_tau + SP +
                   d.n_cens * (k.lb - kns * d.T + tq_softplus(fmaf(-k.ka, d.T, k.c))) + d.nc_int * k.lk0 -
                   kns * (d.sum_tauc + d.T * d.nc_cens);
  return -ll;
}

// one data point alone: log-likelihood term and its gradient (of the log-likelihood) in (log ka, log kns, logit Af),
// through the same consts / accumulate / grad / loss code as the kernel (host tests)
TQ_HD void tq_ttfb_point(const float* par, float tau, float T, int control, float* out) {
  const TqTtfbK k = tq_ttfb_consts(par[0], par[1], par[2]);
  TqTtfbData d = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, T};
  float W1 = 0.0f, W1tau = 0.0f, SP = 0.0f;
  const bool inner = tau > 0.0f && tau < T;
  if (control) {
    if (inner) {
      d.nc_int = 1.0f;
      d.sum_tauc = tau;
    } else if (tau == T) {
      d.nc_cens = 1.0f;
    }
  } else if (inner) {
    d.n_int = 1.0f;
    d.sum_tau = tau;
    tq_ttfb_accumulate(k, tau, W1, W1tau);
    SP = tq_ttfb_softplus_d(k, tau);
  } else if (tau == T) {
    d.n_cens = 1.0f;
  }
  float g[3];
  tq_ttfb_grad(k, d, W1, W1tau, g);
  out[0] = -tq_ttfb_loss(k, d, SP);
  out[1] = -g[0];
  out[2] = -g[1];
  out[3] = -g[2];
}
