// g++ build of the censored dwell-time bodies (tapqir_amd/csrc/tq_censored.h) on host memory, for the test suite: the term
// and gradient of one censored pair, the product-limit survival of a row, and a serial replay of one launch of
// tq_dwell_censored_fit.
#include "../../tapqir_amd/csrc/tq_censored.h"

namespace {

// balanced pairwise sum of the 64 lane partials (in place): the tree tq_group_sum<64> forms in every lane
float lane_tree_sum(float* x) {
  for (int w = 1; w < 64; w *= 2)
    for (int i = 0; i < 64; i += 2 * w) x[i] += x[i + w];
  return x[0];
}

// lane-strided partial sums of one list under the constants q, then the wave tree
template <int K>
void list_sums(const TqDwellK<K>& q, const float* vals, const float* wts, int len, float R[K], float RT[K]) {
  float Rl[K][64], RTl[K][64];
  for (int lane = 0; lane < 64; ++lane) {
    float r[K], rt[K];
    for (int j = 0; j < K; ++j) r[j] = rt[j] = 0.0f;
    for (int i = lane; i < len; i += 64) tq_dwell_accumulate<K>(q, vals[i], wts[i], r, rt);
    for (int j = 0; j < K; ++j) {
      Rl[j][lane] = r[j];
      RTl[j][lane] = rt[j];
    }
  }
  for (int j = 0; j < K; ++j) {
    R[j] = lane_tree_sum(Rl[j]);
    RT[j] = lane_tree_sum(RTl[j]);
  }
}

float list_weight(const float* wts, int len) {
  float part[64];
  for (int lane = 0; lane < 64; ++lane) {
    part[lane] = 0.0f;
    for (int i = lane; i < len; i += 64) part[lane] += wts[i];
  }
  return lane_tree_sum(part);
}

template <int K>
float list_loglik(const TqDwellK<K>& q, const float* vals, const float* wts, int len) {
  float part[64];
  for (int lane = 0; lane < 64; ++lane) {
    float ll = 0.0f, r[K];
    for (int i = lane; i < len; i += 64) ll = fmaf(wts[i], tq_dwell_resp<K>(q, vals[i], r, true), ll);
    part[lane] = ll;
  }
  return lane_tree_sum(part);
}

// serial replay of one tq_dwell_censored_fit launch.  The LDS and L2 routes of the kernel differ only in where a pair is
// read from, so one replay stands for both.
template <int K>
void fit_steps_k(const float* values, const float* weights, const int64_t* row_ptr, const float* cvalues,
                 const float* cweights, const int64_t* crow_ptr, float* state, float* loss, int S, int step0, int n_steps,
                 double lr, double beta1, double beta2, double eps) {
  constexpr int P = 2 * K;
  for (int s = 0; s < S; ++s) {
    const int len = (int)(row_ptr[s + 1] - row_ptr[s]), clen = (int)(crow_ptr[s + 1] - crow_ptr[s]);
    const float* vals = values + row_ptr[s];
    const float* wts = weights + row_ptr[s];
    const float* cvals = cvalues + crow_ptr[s];
    const float* cwts = cweights + crow_ptr[s];
    const float n = list_weight(wts, len), nc = list_weight(cwts, clen);
    float* st = state + (int64_t)s * 3 * P;
    float p[P], m[P], v[P];
    for (int j = 0; j < P; ++j) {
      p[j] = st[j];
      m[j] = st[P + j];
      v[j] = st[2 * P + j];
    }
    const TqFitAdam adam(lr, beta1, beta2, eps);
    const int last = step0 + n_steps;
    for (int t = step0 + 1; t <= last; ++t) {
      const TqDwellK<K> q = tq_dwell_consts<K>(p);
      const TqDwellK<K> qc = tq_censored_consts<K>(q, p);
      float R[K], RT[K], Rc[K], RTc[K], g[P];
      list_sums<K>(q, vals, wts, len, R, RT);
      list_sums<K>(qc, cvals, cwts, clen, Rc, RTc);
      if (t == last && loss) loss[s] = -(list_loglik<K>(q, vals, wts, len) + list_loglik<K>(qc, cvals, cwts, clen));
      tq_censored_grad<K>(q, R, RT, n, Rc, RTc, nc, g);
      const float step_size = adam.step_size(t), bc2s = adam.bc2s(t);
      for (int j = 0; j < P; ++j) tq_fit_adam(p[j], m[j], v[j], g[j], adam.w1, adam.b2, adam.w2, step_size, bc2s, adam.eps);
    }
    for (int j = 0; j < P; ++j) {
      st[j] = p[j];
      st[P + j] = m[j];
      st[2 * P + j] = v[j];
    }
  }
}

}  // namespace

extern "C" {

// one censored pair: out = [ll, d ll / d log k (K), d ll / d a (K)]; returns 0, or 1 for K outside 1 .. TQ_DWELL_KMAX
int hk_censored_pair(const float* par, int K, float t, float w, float* out) {
#define TQ_PAIR_CASE(k) \
  case k: tq_censored_pair_k<k>(par, t, w, out); return 0;
  switch (K) {
    TQ_PAIR_CASE(1)
    TQ_PAIR_CASE(2)
    TQ_PAIR_CASE(3)
    TQ_PAIR_CASE(4)
    TQ_PAIR_CASE(5)
    TQ_PAIR_CASE(6)
    TQ_PAIR_CASE(7)
    TQ_PAIR_CASE(8)
    default: return 1;
  }
#undef TQ_PAIR_CASE
}

// product-limit survival of R rows of F bins
void hk_survival(const int32_t* hist, const int32_t* cens, int R, int F, double* surv) {
  for (int r = 0; r < R; ++r) tq_survival_row(hist + (int64_t)r * F, cens + (int64_t)r * F, F, surv + (int64_t)r * F);
}

// one launch of tq_dwell_censored_fit on host memory (state (S, 6K) in place, loss (S) or NULL); returns 0, or 1 for K
// outside 1 .. TQ_DWELL_KMAX
int hk_censored_fit_steps(int K, const float* values, const float* weights, const int64_t* row_ptr, const float* cvalues,
                          const float* cweights, const int64_t* crow_ptr, float* state, float* loss, int S, int step0,
                          int n_steps, double lr, double beta1, double beta2, double eps) {
#define TQ_FIT_CASE(k)                                                                                                  \
  case k:                                                                                                               \
    fit_steps_k<k>(values, weights, row_ptr, cvalues, cweights, crow_ptr, state, loss, S, step0, n_steps, lr, beta1, beta2, \
                   eps);                                                                                                \
    return 0;
  switch (K) {
    TQ_FIT_CASE(1)
    TQ_FIT_CASE(2)
    TQ_FIT_CASE(3)
    TQ_FIT_CASE(4)
    TQ_FIT_CASE(5)
    TQ_FIT_CASE(6)
    TQ_FIT_CASE(7)
    TQ_FIT_CASE(8)
    default: return 1;
  }
#undef TQ_FIT_CASE
}
}
