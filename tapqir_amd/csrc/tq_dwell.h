// tq_dwell.h -- dwell-time kinetics (tapqir `dwelltime`, tapqir/main.py:1150-1384), host+device inline bodies:
//   * the interval sampler: posterior z rasters drawn frame by frame from the factorised q(z) and walked into runs of equal
//     labels as they are drawn, with count_intervals' bookkeeping (tapqir/utils/imscroll.py:14-110) -- no raster is stored;
//   * the K-exponential mixture MLE that tapqir/utils/mle_analysis.py:107-130 fits with pyro SVI + TraceEnum_ELBO + Adam,
//     one independent 2K-parameter fit per posterior sample.
// The __global__ wrappers are in tq_dwell.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "../../include/tapqir_hip.h"
#include "tq_fit.h"

#define TQ_DWELL_SITE 0xA01u  // Philox site id of the raster uniforms: stream (seed, step = s, site, elem = n)

// ---- raster sampler + interval walker -------------------------------------------------------------------------------
// Frame f of (sample s, AOI n) is z = (u < p[n, f]) with u the f-th tq_uniform of the stream: p = 0 never binds, p = 1
// always does (u < 1 always).
TQ_HD void tq_dwell_stream(TqPhilox* ph, uint64_t seed, int s, int n) {
  tq_philox_init(ph, seed, (uint32_t)s, TQ_DWELL_SITE, (uint64_t)n);
}
TQ_HD int tq_dwell_label(TqPhilox* ph, float p) { return tq_uniform(ph) < p ? 1 : 0; }

// one run of equal labels: frames [start, stop], label z, and count_intervals' low_or_high code
struct TqDwellInterval {
  int start, stop, z, low_or_high;
};

// walker state of one row: the open run
struct TqDwellWalk {
  int cur, start, first;
};

// low_or_high of a run: start type -z - 2 when it opens the record (else z), stop type z + 2 when it closes it (else z);
// the larger magnitude wins and the stop type wins a tie (a run that is both first and last gets z + 2)
TQ_HD int tq_dwell_code(int z, int first, int last) {
  const int start_type = first ? -z - 2 : z;
  const int stop_type = last ? z + 2 : z;
  return (start_type < 0 ? -start_type : start_type) > stop_type ? start_type : stop_type;
}

TQ_HD void tq_dwell_begin(TqDwellWalk& w, int z) {
  w.cur = z;
  w.start = 0;
  w.first = 1;
}

// frame f >= 1 with label z: returns 1 and fills `out` when it closes the run that ended at f - 1
TQ_HD int tq_dwell_step(TqDwellWalk& w, int f, int z, TqDwellInterval& out) {
  if (z == w.cur) return 0;
  out.start = w.start;
  out.stop = f - 1;
  out.z = w.cur;
  out.low_or_high = tq_dwell_code(w.cur, w.first, 0);
  w.cur = z;
  w.start = f;
  w.first = 0;
  return 1;
}

// the run still open after the last frame F - 1
TQ_HD void tq_dwell_finish(const TqDwellWalk& w, int F, TqDwellInterval& out) {
  out.start = w.start;
  out.stop = F - 1;
  out.z = w.cur;
  out.low_or_high = tq_dwell_code(w.cur, w.first, 1);
}

// ---- K-exponential mixture MLE ----------------------------------------------------------------------------------------
// Unconstrained parameters per sample: log k_j and softmax logits a_j, j < K (pyro constraints.positive / simplex through
// transform_to: ExpTransform, SoftmaxTransform).  Per data pair (t, w) the log-likelihood is
//   w log sum_j A_j k_j exp(-k_j t) = w (M + log Z),  l_j = log A_j + log k_j - k_j t,  M = max_j l_j,  Z = sum_j e^{l_j - M}
// and with the responsibilities r_j = e^{l_j - M} / Z the gradient of the LOSS (= -log-likelihood) is
//   d/dlog k_j = -(R_j - k_j RT_j),  d/da_j = -(R_j - n A_j),   R_j = sum w r_j,  RT_j = sum w r_j t,  n = sum w.
template <int K>
struct TqDwellK {
  float k[K];   // rates
  float c[K];   // log A_j + log k_j
  float A[K];   // mixture weights
};

template <int K>
TQ_HD TqDwellK<K> tq_dwell_consts(const float* par) {
  TqDwellK<K> q;
  float amax = par[K];
#pragma unroll
  for (int j = 1; j < K; ++j) amax = fmaxf(amax, par[K + j]);
  float e[K], sum = 0.0f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    e[j] = TQ_FEXP(par[K + j] - amax);
    sum += e[j];
  }
  const float lsum = TQ_FLOG(sum), rsum = 1.0f / sum;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    q.k[j] = TQ_FEXP(par[j]);
    q.A[j] = e[j] * rsum;
    q.c[j] = (par[K + j] - amax - lsum) + par[j];
  }
  return q;
}

// responsibilities of one pair; returns M + log Z only when `want_ll` (the loss pass)
template <int K>
TQ_HD float tq_dwell_resp(const TqDwellK<K>& q, float t, float r[K], bool want_ll) {
  float l[K], m = -INFINITY;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    l[j] = fmaf(-q.k[j], t, q.c[j]);
    m = fmaxf(m, l[j]);
  }
  float z = 0.0f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    r[j] = TQ_FEXP(l[j] - m);
    z += r[j];
  }
  const float rz = 1.0f / z;
#pragma unroll
  for (int j = 0; j < K; ++j) r[j] *= rz;
  return want_ll ? m + TQ_FLOG(z) : 0.0f;
}

// per-pair work of a step: R_j += w r_j, RT_j += w r_j t
template <int K>
TQ_HD void tq_dwell_accumulate(const TqDwellK<K>& q, float t, float w, float R[K], float RT[K]) {
  float r[K];
  tq_dwell_resp<K>(q, t, r, false);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float wr = w * r[j];
    R[j] += wr;
    RT[j] = fmaf(wr, t, RT[j]);
  }
}

// gradient of the LOSS in (log k_0.., a_0..) from the reduced sums; K = 1 has no free weight: its logit gradient is 0
template <int K>
TQ_HD void tq_dwell_grad(const TqDwellK<K>& q, const float R[K], const float RT[K], float n, float g[2 * K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    g[j] = -(R[j] - q.k[j] * RT[j]);
    g[K + j] = K == 1 ? 0.0f : -(R[j] - n * q.A[j]);
  }
}

// one pair alone: log-likelihood term and its gradient (of the log-likelihood) through the kernel's code (host tests).
// out = [ll, d/dlog k (K), d/da (K)]
template <int K>
TQ_HD void tq_dwell_pair_k(const float* par, float t, float w, float* out) {
  const TqDwellK<K> q = tq_dwell_consts<K>(par);
  float R[K], RT[K], r[K], g[2 * K];
#pragma unroll
  for (int j = 0; j < K; ++j) R[j] = RT[j] = 0.0f;
  tq_dwell_accumulate<K>(q, t, w, R, RT);
  tq_dwell_grad<K>(q, R, RT, w, g);
  out[0] = w * tq_dwell_resp<K>(q, t, r, true);
  for (int j = 0; j < 2 * K; ++j) out[1 + j] = -g[j];
}
