// tq_censored.h -- what `dwelltime --censored` adds to the dwell-time kinetics of tq_dwell.h (host+device inline bodies,
// DESIGN.md section 31): the run that is still open at the last frame enters the K-exponential fit as a right-censored
// observation, and the product-limit (Kaplan-Meier) survival curve of a row of histograms.
//
// A run of d frames that closes inside the record sits at t = d: d - 1 stays and one leave, the density term
// log sum_j A_j k_j exp(-k_j d) of tq_dwell.h.  A run that opened inside the record and is open at frame F - 1 after d
// seen frames has made d - 1 stays and nothing else: its term is the survival log sum_j A_j exp(-k_j (d - 1)).
// The __global__ wrappers are in tq_censored.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "tq_dwell.h"

// ---- the censored term ------------------------------------------------------------------------------------------------
// Per censored pair (t, w): w log sum_j A_j exp(-k_j t) = w (M + log Z) with l_j = log A_j - k_j t -- the density term of
// tq_dwell_resp with log A_j in the place of c_j = log A_j + log k_j.  So the constants of a step are those of
// tq_dwell_consts with c_j - log k_j, and tq_dwell_resp / tq_dwell_accumulate on them give log S(t), the responsibilities
// rho_j and the sums Rc_j = sum w rho_j, RTc_j = sum w rho_j t.
template <int K>
TQ_HD TqDwellK<K> tq_censored_consts(const TqDwellK<K>& q, const float* par) {
  TqDwellK<K> qc;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    qc.k[j] = q.k[j];
    qc.A[j] = q.A[j];
    qc.c[j] = q.c[j] - par[j];
  }
  return qc;
}

// Gradient of the LOSS = -sum w log f(t) - sum wc log S(tc) in (log k_0.., a_0..) from the reduced sums:
//   d/dlog k_j = -(R_j - k_j (RT_j + RTc_j)),  d/da_j = -(R_j + Rc_j - (n + nc) A_j)
// through tq_dwell_grad, so that with Rc = RTc = nc = 0 (exact zeros) it is tq_dwell_grad's result bit for bit.
template <int K>
TQ_HD void tq_censored_grad(const TqDwellK<K>& q, const float R[K], const float RT[K], float n, const float Rc[K],
                            const float RTc[K], float nc, float g[2 * K]) {
  float Rs[K], RTs[K], gk[2 * K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    Rs[j] = R[j] + Rc[j];
    RTs[j] = RT[j] + RTc[j];
  }
  tq_dwell_grad<K>(q, R, RTs, n + nc, gk);
  tq_dwell_grad<K>(q, Rs, RTs, n + nc, g);
#pragma unroll
  for (int j = 0; j < K; ++j) g[j] = gk[j];
}

// one censored pair alone: log-likelihood term and its gradient (of the log-likelihood) through the kernel's code (host
// tests).  out = [ll, d/dlog k (K), d/da (K)]
template <int K>
TQ_HD void tq_censored_pair_k(const float* par, float t, float w, float* out) {
  const TqDwellK<K> q = tq_dwell_consts<K>(par);
  const TqDwellK<K> qc = tq_censored_consts<K>(q, par);
  float R[K], RT[K], Rc[K], RTc[K], r[K], g[2 * K];
#pragma unroll
  for (int j = 0; j < K; ++j) R[j] = RT[j] = Rc[j] = RTc[j] = 0.0f;
  tq_dwell_accumulate<K>(qc, t, w, Rc, RTc);
  tq_censored_grad<K>(q, R, RT, 0.0f, Rc, RTc, w, g);
  out[0] = w * tq_dwell_resp<K>(qc, t, r, true);
  for (int j = 0; j < 2 * K; ++j) out[1 + j] = -g[j];
}

// ---- product-limit survival -------------------------------------------------------------------------------------------
// Row of complete-run counts h_d and open-run counts c_d, d < F.  At u >= 1 the runs at risk are
//   Y_u = sum_{d >= u} h_d + sum_{d >= u + 1} c_d
// (an open run of d frames is at risk up to d - 1, the convention of the fit), and surv[t] = prod_{u = 1..t} (Y_u - h_u) /
// Y_u with a factor of 1 where Y_u = 0.  Bin 0 of h and bins 0 and 1 of c hold nothing that is at risk anywhere.
TQ_HD int64_t tq_survival_h(const int32_t* h, int f) { return f >= 1 ? (int64_t)h[f] : 0; }
TQ_HD int64_t tq_survival_c(const int32_t* c, int f) { return f >= 2 ? (int64_t)c[f] : 0; }

// one factor: one division of an integer numerator by an integer denominator (exact 1 at h = 0, exact 0 at Y = h)
TQ_HD double tq_survival_factor(int64_t Y, int64_t h) { return Y > 0 ? (double)(Y - h) / (double)Y : 1.0; }

// the whole row, serially (what tq_dwell_survival computes with one wave; host tests)
TQ_HD void tq_survival_row(const int32_t* h, const int32_t* c, int F, double* surv) {
  int64_t total = 0;
  for (int f = 0; f < F; ++f) total += tq_survival_h(h, f) + tq_survival_c(c, f);
  int64_t gone = 0;  // sum_{d < u} h_d + sum_{d <= u} c_d
  double prod = 1.0;
  for (int f = 0; f < F; ++f) {
    const int64_t hv = tq_survival_h(h, f);
    gone += tq_survival_c(c, f);
    prod *= tq_survival_factor(total - gone, hv);
    gone += hv;
    surv[f] = prod;
  }
}
