// g++ build of the draws and the walk of tq_pair_dwell (tapqir_amd/csrc/tq_joint.h: TqPairDwellRow, tq_pair_dwell_frame,
// tq_pair_hist_at; tapqir_amd/csrc/tq_hmm.h: TqHmmDraws, tq_hmm_thresholds, tq_hmm_label) on host memory, for the test
// suite: a replay of both modes of the entry point per row, with the kernel's order of draws (u_0 for frame F - 1, then
// downwards, four uniforms to a Philox block).  With -DPAIR_DWELL_MAIN the file is a stand-alone program that replays one
// case in both modes and for both channels and checks it against a forward walk of the same states (for a sanitizer build).
#include "../../tapqir_amd/csrc/tq_joint.h"

namespace {

// Rows (s, n) of tq_pair_dwell.  COUNT (cols == nullptr): counts (S, N), histograms (S, 2, F), tau and tau_after (S, N) or
// NULL; EMIT: the table (7, total) and the partner codes (total) from `counts` and `offsets`.  `raster`, when given,
// receives the joint states (S, N, F).  Returns the smallest |u - t| of all compares.
double sample(const double* filt, const double* theta, int which, int S, int N, int F, uint64_t seed, int32_t* counts,
              int32_t* hb, int32_t* hu, float* tau, float* tau_after, const int64_t* offsets, int32_t* cols, uint8_t* partner,
              int64_t total, uint8_t* raster) {
  constexpr int M = TQ_JOINT_M;
  const TqHmmModel<M> m = tq_hmm_model<M>(theta, 2, 0.5);
  double margin = 1.0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      const int64_t o = cols ? offsets[row] : 0;
      const int count = cols ? counts[row] : 0;
      int closed = 0;
      auto put = [&](const TqDwellInterval& v, int code) {
        if (cols) {
          const int64_t pos = tq_smooth_emit_slot(o, count, closed, total);
          if (pos >= 0) {
            tq_smooth_emit_row(cols, total, pos, s, n, v);
            partner[pos] = (uint8_t)code;
          }
        } else if (v.low_or_high == 0 || v.low_or_high == 1) {
          ++(v.z ? hb : hu)[tq_pair_hist_at(s, code & 1, F) + v.stop + 1 - v.start];
        }
        ++closed;
      };
      TqHmmDraws draws;
      tq_hmm_draws_begin(draws, seed, s, n);
      TqPairDwellRow r;
      tq_pair_dwell_begin(r, F);
      TqDwellInterval iv;
      int code = 0;
      for (int f = F - 1; f >= 0; --f) {
        double t[M * (M - 1)];
        tq_hmm_thresholds(m, filt + ((int64_t)n * F + f) * M, f == F - 1, t);
        const double u = tq_hmm_draws_next(draws, F - 1 - f);
        const double* tj = t + (f == F - 1 ? 0 : r.c.next) * (M - 1);
        for (int i = 0; i < M - 1; ++i) margin = fmin(margin, fabs(u - tj[i]));
        if (tq_pair_dwell_frame(r, u, t, f, F, which, iv, code)) put(iv, code);
        if (raster) raster[row * F + f] = (uint8_t)r.c.next;
      }
      tq_pair_dwell_finish(r, iv, code);
      put(iv, code);
      if (!cols) {
        counts[row] = closed;
        if (tau) tau[row] = (float)r.c.tau;
        if (tau_after) tau_after[row] = (float)r.tau_after;
      }
    }
  return margin;
}

}  // namespace

extern "C" {

double hk_pw_sample(const double* filt, const double* theta, int which, int S, int N, int F, uint64_t seed, int32_t* counts,
                    int32_t* hb, int32_t* hu, float* tau, float* tau_after, const int64_t* offsets, int32_t* cols,
                    uint8_t* partner, int64_t total, uint8_t* raster) {
  if (which != 0 && which != 1) return -1.0;
  return sample(filt, theta, which, S, N, F, seed, counts, hb, hu, tau, tau_after, offsets, cols, partner, total, raster);
}
}

#ifdef PAIR_DWELL_MAIN
#include <stdio.h>

#include <vector>

// N = 6, F = 65, S = 70, both channels: filt from a fixed recurrence, COUNT, the scan, EMIT into a table and a code array of
// exactly the documented sizes, and a forward walk (tq_dwell.h) of the replayed states as the cross-check of the table, the
// partner codes, the histograms by q(start), tau and tau_after.  Exit status 0 when the two agree.
int main() {
  const int S = 70, N = 6, F = 65, M = 4;
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
  for (int f = 0; f < F; ++f)  // rows 0 and 1: neither channel ever bound, both always
    for (int i = 0; i < M; ++i) {
      filt[(size_t)f * M + i] = i == 0 ? 1.0 : 0.0;
      filt[((size_t)F + f) * M + i] = i == M - 1 ? 1.0 : 0.0;
    }
  long long bad = 0, intervals = 0;
  for (int which = 0; which < 2; ++which) {
    std::vector<int32_t> counts((size_t)S * N), hb((size_t)S * 2 * F), hu((size_t)S * 2 * F);
    std::vector<float> tau((size_t)S * N), tau_after((size_t)S * N);
    std::vector<uint8_t> raster((size_t)S * N * F);
    hk_pw_sample(filt.data(), theta.data(), which, S, N, F, seed, counts.data(), hb.data(), hu.data(), tau.data(),
                 tau_after.data(), nullptr, nullptr, nullptr, 0, raster.data());
    std::vector<int64_t> offsets((size_t)S * N);
    int64_t total = 0;
    for (size_t i = 0; i < counts.size(); ++i) {
      offsets[i] = total;
      total += counts[i];
    }
    std::vector<int32_t> cols((size_t)TQ_DWELL_COLS * total, -7);
    std::vector<uint8_t> partner((size_t)total, 0xEE);
    hk_pw_sample(filt.data(), theta.data(), which, S, N, F, seed, counts.data(), nullptr, nullptr, nullptr, nullptr,
                 offsets.data(), cols.data(), partner.data(), total, nullptr);
    std::vector<int64_t> wb((size_t)S * 2 * F), wu((size_t)S * 2 * F);
    int64_t o = 0;
    for (int s = 0; s < S; ++s)
      for (int n = 0; n < N; ++n) {
        const uint8_t* sr = raster.data() + ((size_t)s * N + n) * F;
        auto z = [&](int f) { return (sr[f] >> which) & 1; };
        auto q = [&](int f) { return f < 0 || f >= F ? 0 : (sr[f] >> (which ^ 1)) & 1; };
        TqDwellWalk w;
        TqDwellInterval iv;
        auto check = [&](const TqDwellInterval& v) {
          const int32_t want[TQ_DWELL_COLS] = {s, n, v.start, v.stop, v.stop + 1 - v.start, v.low_or_high, v.z};
          for (int c = 0; c < TQ_DWELL_COLS; ++c) bad += o >= total || cols[(size_t)c * total + o] != want[c];
          const int code = q(v.start) | q(v.start - 1) << 1 | q(v.stop) << 2 | q(v.stop + 1) << 3;
          bad += o >= total || partner[o] != code;
          if (v.low_or_high == 0 || v.low_or_high == 1)
            ++(v.z ? wb : wu)[((size_t)s * 2 + q(v.start)) * F + v.stop + 1 - v.start];
          ++o;
        };
        tq_dwell_begin(w, z(0));
        for (int f = 1; f < F; ++f)
          if (tq_dwell_step(w, f, z(f), iv)) check(iv);
        tq_dwell_finish(w, F, iv);
        check(iv);
        int first = F, follow = F;
        for (int f = F - 1; f >= 0; --f)
          if (z(f)) first = f;
        for (int f = F - 1; f >= first; --f)
          if (q(f)) follow = f;
        bad += tau[(size_t)s * N + n] != (float)first;
        bad += tau_after[(size_t)s * N + n] != (float)follow;
      }
    bad += o != total;
    for (size_t i = 0; i < wb.size(); ++i) bad += (wb[i] != hb[i]) + (wu[i] != hu[i]);
    intervals += total;
  }
  printf("pair_dwell_check: %lld intervals, %lld mismatches\n", intervals, bad);
  return bad ? 1 : 0;
}
#endif
