// g++ build of the dwell-time bodies (tapqir_amd/csrc/tq_dwell.h) on host memory, for the test suite: the interval walker
// on given rasters, a replay of the sampler (same Philox uniforms, same walk), per-pair likelihood terms and gradients.
#include "../../tapqir_amd/csrc/tq_dwell.h"

namespace {

// walk rows (s, n) of labels produced by `label(s, n, f)`; count mode fills counts / histograms, emit mode the columns
template <class Label>
void walk_rows(Label label, int S, int N, int F, int32_t* counts, int32_t* hb, int32_t* hu, int32_t* cols,
               int64_t total) {
  int64_t o = 0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      int count = 0;
      auto put = [&](const TqDwellInterval& v) {
        ++count;
        const int d = v.stop + 1 - v.start;
        if (hb && (v.low_or_high == 0 || v.low_or_high == 1)) ++(v.z ? hb : hu)[(int64_t)s * F + d];
        if (cols && o < total) {
          const int32_t row[TQ_DWELL_COLS] = {s, n, v.start, v.stop, d, v.low_or_high, v.z};
          for (int c = 0; c < TQ_DWELL_COLS; ++c) cols[c * total + o] = row[c];
        }
        ++o;
      };
      TqDwellWalk w;
      TqDwellInterval iv;
      label.begin(s, n);
      tq_dwell_begin(w, label.next(0));
      for (int f = 1; f < F; ++f)
        if (tq_dwell_step(w, f, label.next(f), iv)) put(iv);
      tq_dwell_finish(w, F, iv);
      put(iv);
      if (counts) counts[(int64_t)s * N + n] = count;
    }
}

struct Given {
  const int32_t* z;
  int N, F;
  const int32_t* row;
  void begin(int s, int n) { row = z + ((int64_t)s * N + n) * F; }
  int next(int f) { return row[f] != 0; }
};

struct Drawn {
  const float* p;
  int N, F;
  uint64_t seed;
  TqPhilox ph;
  const float* row;
  void begin(int s, int n) {
    tq_dwell_stream(&ph, seed, s, n);
    row = p + (int64_t)n * F;
  }
  int next(int f) { return tq_dwell_label(&ph, row[f]); }
};

template <int K>
void pair_k(const float* par, float t, float w, float* out) {
  tq_dwell_pair_k<K>(par, t, w, out);
}

// balanced pairwise sum of the 64 lane partials (in place): the tree tq_group_sum<64> forms in every lane
float lane_tree_sum(float* x) {
  for (int w = 1; w < 64; w *= 2)
    for (int i = 0; i < 64; i += 2 * w) x[i] += x[i + w];
  return x[0];
}

// serial replay of one tq_dwell_fit launch: lane-strided partial sums, the wave tree, the kernel's bodies and its Adam.
// The LDS and L2 routes of the kernel differ only in where a pair is read from, so one replay stands for both.
template <int K>
void fit_steps_k(const float* values, const float* weights, const int64_t* row_ptr, float* state, float* loss, int S,
                 int step0, int n_steps, double lr, double beta1, double beta2, double eps) {
  constexpr int P = 2 * K;
  for (int s = 0; s < S; ++s) {
    const int len = (int)(row_ptr[s + 1] - row_ptr[s]);
    const float* vals = values + row_ptr[s];
    const float* wts = weights + row_ptr[s];
    float part[64];
    for (int lane = 0; lane < 64; ++lane) {
      part[lane] = 0.0f;
      for (int i = lane; i < len; i += 64) part[lane] += wts[i];
    }
    const float n = lane_tree_sum(part);
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
      float Rl[K][64], RTl[K][64], R[K], RT[K];
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
      if (t == last && loss) {
        for (int lane = 0; lane < 64; ++lane) {
          float ll = 0.0f, r[K];
          for (int i = lane; i < len; i += 64) ll = fmaf(wts[i], tq_dwell_resp<K>(q, vals[i], r, true), ll);
          part[lane] = ll;
        }
        loss[s] = -lane_tree_sum(part);
      }
      float g[P];
      tq_dwell_grad<K>(q, R, RT, n, g);
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

// the walker on a given (S, N, F) raster of 0/1 labels: counts (S, N), histograms (S, F) and/or the columns (7, total)
void hk_dwell_walk(const int32_t* z, int S, int N, int F, int32_t* counts, int32_t* hb, int32_t* hu, int32_t* cols,
                   int64_t total) {
  walk_rows(Given{z, N, F, nullptr}, S, N, F, counts, hb, hu, cols, total);
}

// the sampler's draws and walk (what tq_dwell_sample computes in both modes)
void hk_dwell_sample(const float* p, int S, int N, int F, uint64_t seed, int32_t* counts, int32_t* hb, int32_t* hu,
                     int32_t* cols, int64_t total) {
  Drawn d;
  d.p = p;
  d.N = N;
  d.F = F;
  d.seed = seed;
  walk_rows(d, S, N, F, counts, hb, hu, cols, total);
}

// the sampled raster itself (S, N, F), for count_intervals
void hk_dwell_raster(const float* p, int S, int N, int F, uint64_t seed, int32_t* z) {
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      TqPhilox ph;
      tq_dwell_stream(&ph, seed, s, n);
      for (int f = 0; f < F; ++f) z[((int64_t)s * N + n) * F + f] = tq_dwell_label(&ph, p[(int64_t)n * F + f]);
    }
}

int hk_dwell_code(int z, int first, int last) { return tq_dwell_code(z, first, last); }

// one pair: out = [ll, d ll / d log k (K), d ll / d a (K)]; returns 0, or 1 for K outside 1 .. 4
int hk_dwell_pair(const float* par, int K, float t, float w, float* out) {
  switch (K) {
    case 1: pair_k<1>(par, t, w, out); return 0;
    case 2: pair_k<2>(par, t, w, out); return 0;
    case 3: pair_k<3>(par, t, w, out); return 0;
    case 4: pair_k<4>(par, t, w, out); return 0;
    default: return 1;
  }
}

// one launch of tq_dwell_fit on host memory (state (S, 6K) in place, loss (S) or NULL); returns 0, or 1 for K outside
// 1 .. TQ_DWELL_KMAX
int hk_dwell_fit_steps(int K, const float* values, const float* weights, const int64_t* row_ptr, float* state,
                       float* loss, int S, int step0, int n_steps, double lr, double beta1, double beta2, double eps) {
#define TQ_FIT_CASE(k) \
  case k: fit_steps_k<k>(values, weights, row_ptr, state, loss, S, step0, n_steps, lr, beta1, beta2, eps); return 0;
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
