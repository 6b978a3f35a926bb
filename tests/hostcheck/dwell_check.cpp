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
}
