// g++ build of the draws and the walk of tq_chain_dwell (tapqir_amd/csrc/tq_hmm.h: TqHmmDraws, tq_chain_dwell_frame) on
// host memory, for the test suite: a replay of both modes of the entry point per row, with the kernel's order of draws
// (u_0 for frame F - 1, then downwards, four uniforms to a Philox block).  With -DHMM_DWELL_MAIN the file is a stand-alone
// program that replays one case and checks it against a forward walk of the same labels (for a sanitizer build).
#include "../../tapqir_amd/csrc/tq_hmm.h"

namespace {

// Rows (s, n) of tq_chain_dwell.  COUNT (cols == nullptr): counts (S, N), histograms (S, F), tau (S, N) or NULL; EMIT: the
// table (7, total) from `counts` and `offsets`.  `raster`, when given, receives the hidden states (S, N, F).  Returns the
// smallest |u - t| of all compares.
template <int M>
double sample(const double* filt, const double* theta, int U, int S, int N, int F, uint64_t seed, int32_t* counts,
              int32_t* hb, int32_t* hu, float* tau, const int64_t* offsets, int32_t* cols, int64_t total, uint8_t* raster) {
  const TqHmmModel<M> m = tq_hmm_model<M>(theta, U, 0.5);
  double margin = 1.0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      const int64_t o = cols ? offsets[row] : 0;
      const int count = cols ? counts[row] : 0;
      int closed = 0;
      auto put = [&](const TqDwellInterval& v) {
        if (cols) {
          const int64_t pos = tq_smooth_emit_slot(o, count, closed, total);
          if (pos >= 0) tq_smooth_emit_row(cols, total, pos, s, n, v);
        } else if (v.low_or_high == 0 || v.low_or_high == 1) {
          ++(v.z ? hb : hu)[(int64_t)s * F + v.stop + 1 - v.start];
        }
        ++closed;
      };
      TqHmmDraws draws;
      tq_hmm_draws_begin(draws, seed, s, n);
      TqChainDwellRow r;
      tq_chain_dwell_begin(r, F);
      TqDwellInterval iv;
      for (int f = F - 1; f >= 0; --f) {
        double t[M * (M - 1)];
        tq_hmm_thresholds(m, filt + ((int64_t)n * F + f) * M, f == F - 1, t);
        const double u = tq_hmm_draws_next(draws, F - 1 - f);
        const double* tj = t + (f == F - 1 ? 0 : r.next) * (M - 1);
        for (int i = 0; i < M - 1; ++i) margin = fmin(margin, fabs(u - tj[i]));
        if (tq_chain_dwell_frame<M>(r, u, t, f, F, U, iv)) put(iv);
        if (raster) raster[row * F + f] = (uint8_t)r.next;
      }
      tq_chain_dwell_finish(r, iv);
      put(iv);
      if (!cols) {
        counts[row] = closed;
        if (tau) tau[row] = (float)r.tau;
      }
    }
  return margin;
}

}  // namespace

extern "C" {

double hk_hd_sample(const double* filt, const double* theta, int U, int B, int S, int N, int F, uint64_t seed,
                    int32_t* counts, int32_t* hb, int32_t* hu, float* tau, const int64_t* offsets, int32_t* cols,
                    int64_t total, uint8_t* raster) {
  switch (U + B) {
    case 2:
      return sample<2>(filt, theta, U, S, N, F, seed, counts, hb, hu, tau, offsets, cols, total, raster);
    case 3:
      return sample<3>(filt, theta, U, S, N, F, seed, counts, hb, hu, tau, offsets, cols, total, raster);
    case 4:
      return sample<4>(filt, theta, U, S, N, F, seed, counts, hb, hu, tau, offsets, cols, total, raster);
    default:
      return -1.0;
  }
}
}

#ifdef HMM_DWELL_MAIN
#include <stdio.h>

#include <vector>

// N = 6, F = 65, S = 70 at (U, B) = (2, 2): filt from a fixed recurrence, COUNT, the scan, EMIT into a table of exactly the
// documented size, and a forward walk (tq_dwell.h) of the replayed states' classes as the cross-check.  Exit status 0 when
// the two agree.
int main() {
  const int S = 70, N = 6, F = 65, U = 2, B = 2, M = 4;
  const uint64_t seed = 0;
  std::vector<double> theta(M * M + M);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j < M; ++j) theta[i * M + j] = i == j ? 0.7 : 0.1;
    theta[M * M + i] = 0.25;
  }
  std::vector<double> filt((size_t)N * F * M);
  uint32_t x = 12345u;
  for (size_t k = 0; k < filt.size(); k += M) {
    double sum = 0.0;
    for (int i = 0; i < M; ++i) {
      x = x * 1664525u + 1013904223u;
      filt[k + i] = ((x >> 8) + 0.5) / 16777216.0;
      sum += filt[k + i];
    }
    for (int i = 0; i < M; ++i) filt[k + i] /= sum;
  }
  for (int f = 0; f < F; ++f)  // rows 0 and 1: never and always bound
    for (int i = 0; i < M; ++i) {
      filt[(size_t)f * M + i] = i == 0 ? 1.0 : 0.0;
      filt[((size_t)F + f) * M + i] = i == M - 1 ? 1.0 : 0.0;
    }
  std::vector<int32_t> counts((size_t)S * N), hb((size_t)S * F), hu((size_t)S * F);
  std::vector<float> tau((size_t)S * N);
  std::vector<uint8_t> raster((size_t)S * N * F);
  hk_hd_sample(filt.data(), theta.data(), U, B, S, N, F, seed, counts.data(), hb.data(), hu.data(), tau.data(), nullptr,
               nullptr, 0, raster.data());
  std::vector<int64_t> offsets((size_t)S * N);
  int64_t total = 0;
  for (size_t i = 0; i < counts.size(); ++i) {
    offsets[i] = total;
    total += counts[i];
  }
  std::vector<int32_t> cols((size_t)TQ_DWELL_COLS * total, -7);
  hk_hd_sample(filt.data(), theta.data(), U, B, S, N, F, seed, counts.data(), nullptr, nullptr, nullptr, offsets.data(),
               cols.data(), total, nullptr);
  std::vector<int64_t> wb((size_t)S * F), wu((size_t)S * F);
  int64_t o = 0, bad = 0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const uint8_t* zr = raster.data() + ((size_t)s * N + n) * F;
      TqDwellWalk w;
      TqDwellInterval iv;
      auto check = [&](const TqDwellInterval& v) {
        const int32_t want[TQ_DWELL_COLS] = {s, n, v.start, v.stop, v.stop + 1 - v.start, v.low_or_high, v.z};
        for (int c = 0; c < TQ_DWELL_COLS; ++c) bad += o >= total || cols[(size_t)c * total + o] != want[c];
        if (v.low_or_high == 0 || v.low_or_high == 1) ++(v.z ? wb : wu)[(size_t)s * F + v.stop + 1 - v.start];
        ++o;
      };
      tq_dwell_begin(w, zr[0] >= U);
      for (int f = 1; f < F; ++f)
        if (tq_dwell_step(w, f, zr[f] >= U, iv)) check(iv);
      tq_dwell_finish(w, F, iv);
      check(iv);
      int first = F;
      for (int f = F - 1; f >= 0; --f)
        if (zr[f] >= U) first = f;
      bad += tau[(size_t)s * N + n] != (float)first;
    }
  bad += o != total;
  for (size_t i = 0; i < wb.size(); ++i) bad += (wb[i] != hb[i]) + (wu[i] != hu[i]);
  printf("hmm_dwell_check: %lld intervals, %lld mismatches\n", (long long)total, (long long)bad);
  return bad ? 1 : 0;
}
#endif
