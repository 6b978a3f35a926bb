// g++ build of the time-to-first-binding bodies (tapqir_amd/csrc/tq_kinetics.h) on host memory, for the test suite:
// per-point likelihood terms and gradients, and a replay of the sampler (same prefix bits, same Philox uniforms).
#include <vector>

#include "../../tapqir_amd/csrc/tq_fit.h"
#include "../../tapqir_amd/csrc/tq_kinetics.h"

namespace {

// balanced pairwise sum of the 64 lane partials (in place): the tree tq_group_sum<64> forms in every lane
float lane_tree_sum(float* x) {
  for (int w = 1; w < 64; w *= 2)
    for (int i = 0; i < 64; i += 2 * w) x[i] += x[i + w];
  return x[0];
}

}  // namespace

extern "C" {

void hk_ttfb_point(const float* par, float tau, float T, int control, float* out) {
  tq_ttfb_point(par, tau, T, control, out);
}

// L[n, f] in the kernel's order: left to right per AOI
void hk_ttfb_prefix(const float* p, double* L, int N, int F) {
  for (int n = 0; n < N; ++n) {
    double acc = 0.0;
    for (int f = 0; f < F; ++f) {
      acc += tq_ttfb_log_surv_term(p[(int64_t)n * F + f]);
      L[(int64_t)n * F + f] = acc;
    }
  }
}

int hk_ttfb_search(const double* L, int F, double lu) { return tq_ttfb_search(L, F, lu); }

void hk_ttfb_sample(const double* L, float* tau, int N, int F, int S, uint64_t seed) {
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n)
      tau[(int64_t)s * N + n] = (float)tq_ttfb_search(L + (int64_t)n * F, F, tq_ttfb_log_uniform(seed, s, n));
}

double hk_log1p_det(double x) { return tq_log1p_det(x); }

// serial replay of one tq_ttfb_fit launch on host memory (state (S, 9) in place, loss (S) or NULL, tauc NULL without a
// control): lane-strided partial sums, the wave tree, the kernel's bodies and its Adam.  `staged` != 0 replays the LDS
// route (N <= TQ_TTFB_LDS_POINTS): the uncensored points compacted in row order, point j of them summed by lane j % 64;
// otherwise point i of the row is summed by lane i % 64.
void hk_ttfb_fit_steps(const float* tau, const float* tauc, float* state, float* loss, int S, int N, int Nc, int step0,
                       int n_steps, int staged, float T, double lr, double beta1, double beta2, double eps) {
  std::vector<float> pts((size_t)N);
  std::vector<int> owner((size_t)N);
  for (int s = 0; s < S; ++s) {
    const float* row = tau + (int64_t)s * N;
    double n_int = 0.0, sum_tau = 0.0, n_cens = 0.0, nc_int = 0.0, sum_tauc = 0.0, nc_cens = 0.0;  // exact: integer data
    int n_pts = 0;
    for (int i = 0; i < N; ++i) {
      const float t = row[i];
      if (t > 0.0f && t < T) {
        n_int += 1.0;
        sum_tau += (double)t;
        owner[n_pts] = (staged ? n_pts : i) % 64;
        pts[n_pts++] = t;
      }
      n_cens += t == T ? 1.0 : 0.0;
    }
    for (int i = 0; tauc && i < Nc; ++i) {
      const float t = tauc[(int64_t)s * Nc + i];
      const bool inner = t > 0.0f && t < T;
      nc_int += inner ? 1.0 : 0.0;
      sum_tauc += inner ? (double)t : 0.0;
      nc_cens += t == T ? 1.0 : 0.0;
    }
    const TqTtfbData d = {(float)n_int, (float)sum_tau, (float)n_cens, (float)nc_int, (float)sum_tauc, (float)nc_cens, T};
    float* st = state + (int64_t)s * TQ_TTFB_STATE;
    float p[3] = {st[0], st[1], st[2]}, m[3] = {st[3], st[4], st[5]}, v[3] = {st[6], st[7], st[8]};
    const TqFitAdam adam(lr, beta1, beta2, eps);
    const int last = step0 + n_steps;
    for (int t = step0 + 1; t <= last; ++t) {
      const TqTtfbK k = tq_ttfb_consts(p[0], p[1], p[2]);
      float W1l[64], W1taul[64], SPl[64];
      for (int lane = 0; lane < 64; ++lane) W1l[lane] = W1taul[lane] = SPl[lane] = 0.0f;
      for (int j = 0; j < n_pts; ++j) tq_ttfb_accumulate(k, pts[j], W1l[owner[j]], W1taul[owner[j]]);
      const float W1 = lane_tree_sum(W1l), W1tau = lane_tree_sum(W1taul);
      if (t == last && loss) {
        for (int j = 0; j < n_pts; ++j) SPl[owner[j]] += tq_ttfb_softplus_d(k, pts[j]);
        loss[s] = tq_ttfb_loss(k, d, lane_tree_sum(SPl));
      }
      float g[3];
      tq_ttfb_grad(k, d, W1, W1tau, g);
      const float step_size = adam.step_size(t), bc2s = adam.bc2s(t);
      for (int j = 0; j < 3; ++j) tq_fit_adam(p[j], m[j], v[j], g[j], adam.w1, adam.b2, adam.w2, step_size, bc2s, adam.eps);
    }
    for (int j = 0; j < 3; ++j) {
      st[j] = p[j];
      st[3 + j] = m[j];
      st[6 + j] = v[j];
    }
  }
}
}
