// g++ build of the draws and the walk of tq_population_dwell (tapqir_amd/csrc/tq_mixture.h: tq_mixture_population,
// tq_population_hist_at; tapqir_amd/csrc/tq_hmm.h: TqHmmDraws, tq_chain_dwell_frame) on host memory, for the test suite: a
// replay of both modes of the entry point per row, with the kernel's order of draws (the population first, then u_0 for
// frame F - 1 and downwards, four uniforms to a Philox block).  With -DPOPULATION_DWELL_MAIN the file is a stand-alone
// program that replays one case and checks it against a forward walk of the same labels (for a sanitizer build).
#include "../../tapqir_amd/csrc/tq_mixture.h"

namespace {

// Rows (s, n) of tq_population_dwell.  COUNT (cols == nullptr): counts (S, N), pop (S, N), histograms (S, G, F), tau (S, N) or
// NULL; EMIT: the table (7, total) from `counts` and `offsets`.  `raster`, when given, receives the hidden states
// (S, N, F).  margins[0]: the smallest |u - tail| of the population draws, margins[1]: the smallest |u - t| of the state
// draws.
template <int M>
void sample(const double* filt, const double* theta, const double* resp, int U, int G, int S, int N, int F, uint64_t seed,
            int32_t* counts, uint8_t* pop, int32_t* hb, int32_t* hu, float* tau, const int64_t* offsets, int32_t* cols,
            int64_t total, uint8_t* raster, double* margins) {
  TqHmmModel<M> mods[TQ_MIXTURE_MAX_POP];
  for (int g = 0; g < G; ++g) mods[g] = tq_hmm_model<M>(theta + tq_multistart_theta_at<M>(g), U, 0.5);
  margins[0] = margins[1] = 1.0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      const int g = tq_mixture_population(seed, s, n, resp + n, N, G);
      {
        TqPhilox ph;
        tq_philox_init(&ph, seed, (uint32_t)s, TQ_MIXTURE_SITE, (uint64_t)n);
        const double u = (double)tq_uniform(&ph);
        double tail = 0.0;
        for (int k = G - 1; k >= 1; --k) {
          tail += resp[(int64_t)k * N + n];
          margins[0] = fmin(margins[0], fabs(u - tail));
        }
      }
      const double* fr = filt + tq_multistart_filt_at<M>(g, n, N, F);
      const int64_t o = cols ? offsets[row] : 0;
      const int count = cols ? counts[row] : 0;
      int closed = 0;
      auto put = [&](const TqDwellInterval& v) {
        if (cols) {
          const int64_t pos = tq_smooth_emit_slot(o, count, closed, total);
          if (pos >= 0) tq_smooth_emit_row(cols, total, pos, s, n, v);
        } else if (v.low_or_high == 0 || v.low_or_high == 1) {
          ++(v.z ? hb : hu)[tq_population_hist_at(s, g, G, F) + v.stop + 1 - v.start];
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
        tq_hmm_thresholds(mods[g], fr + (int64_t)f * M, f == F - 1, t);
        const double u = tq_hmm_draws_next(draws, F - 1 - f);
        const double* tj = t + (f == F - 1 ? 0 : r.next) * (M - 1);
        for (int i = 0; i < M - 1; ++i) margins[1] = fmin(margins[1], fabs(u - tj[i]));
        if (tq_chain_dwell_frame<M>(r, u, t, f, F, U, iv)) put(iv);
        if (raster) raster[row * F + f] = (uint8_t)r.next;
      }
      tq_chain_dwell_finish(r, iv);
      put(iv);
      if (!cols) {
        counts[row] = closed;
        pop[row] = (uint8_t)g;
        if (tau) tau[row] = (float)r.tau;
      }
    }
}

}  // namespace

extern "C" {

int hk_pd_sample(const double* filt, const double* theta, const double* resp, int U, int B, int G, int S, int N, int F,
                 uint64_t seed, int32_t* counts, uint8_t* pop, int32_t* hb, int32_t* hu, float* tau, const int64_t* offsets,
                 int32_t* cols, int64_t total, uint8_t* raster, double* margins) {
  if (G < 1 || G > TQ_MIXTURE_MAX_POP) return -1;
  switch (U + B) {
    case 2:
      sample<2>(filt, theta, resp, U, G, S, N, F, seed, counts, pop, hb, hu, tau, offsets, cols, total, raster, margins);
      return 0;
    case 3:
      sample<3>(filt, theta, resp, U, G, S, N, F, seed, counts, pop, hb, hu, tau, offsets, cols, total, raster, margins);
      return 0;
    case 4:
      sample<4>(filt, theta, resp, U, G, S, N, F, seed, counts, pop, hb, hu, tau, offsets, cols, total, raster, margins);
      return 0;
    default:
      return -1;
  }
}
}

#ifdef POPULATION_DWELL_MAIN
#include <stdio.h>

#include <vector>

// N = 6, F = 65, S = 70, G = 3 at (U, B) = (2, 2): filt and resp from a fixed recurrence, COUNT, the scan, EMIT into a table
// of exactly the documented size, and a forward walk (tq_dwell.h) of the replayed states' classes, binned by the replayed
// population, as the cross-check.  Exit status 0 when the two agree.
int main() {
  const int S = 70, N = 6, F = 65, U = 2, B = 2, M = 4, G = 3;
  const uint64_t seed = 0;
  std::vector<double> theta((size_t)G * (M * M + M));
  for (int g = 0; g < G; ++g)
    for (int i = 0; i < M; ++i) {
      for (int j = 0; j < M; ++j) theta[(size_t)g * (M * M + M) + i * M + j] = i == j ? 1.0 - 0.3 / (g + 1) : 0.1 / (g + 1);
      theta[(size_t)g * (M * M + M) + M * M + i] = 0.25;
    }
  std::vector<double> filt((size_t)G * N * F * M), resp((size_t)G * N);
  uint32_t x = 12345u;
  auto next = [&]() {
    x = x * 1664525u + 1013904223u;
    return ((x >> 8) + 0.5) / 16777216.0;
  };
  for (size_t k = 0; k < filt.size(); k += M) {
    double sum = 0.0;
    for (int i = 0; i < M; ++i) sum += filt[k + i] = next();
    for (int i = 0; i < M; ++i) filt[k + i] /= sum;
  }
  for (int g = 0; g < G; ++g)
    for (int f = 0; f < F; ++f)  // rows 0 and 1 of every population: never and always bound
      for (int i = 0; i < M; ++i) {
        filt[(((size_t)g * N + 0) * F + f) * M + i] = i == 0 ? 1.0 : 0.0;
        filt[(((size_t)g * N + 1) * F + f) * M + i] = i == M - 1 ? 1.0 : 0.0;
      }
  for (int n = 0; n < N; ++n) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += resp[(size_t)g * N + n] = next();
    for (int g = 0; g < G; ++g) resp[(size_t)g * N + n] /= sum;
  }
  std::vector<int32_t> counts((size_t)S * N), hb((size_t)S * G * F), hu((size_t)S * G * F);
  std::vector<uint8_t> pop((size_t)S * N), raster((size_t)S * N * F);
  std::vector<float> tau((size_t)S * N);
  double margins[2];
  hk_pd_sample(filt.data(), theta.data(), resp.data(), U, B, G, S, N, F, seed, counts.data(), pop.data(), hb.data(), hu.data(),
               tau.data(), nullptr, nullptr, 0, raster.data(), margins);
  std::vector<int64_t> offsets((size_t)S * N);
  int64_t total = 0;
  for (size_t i = 0; i < counts.size(); ++i) {
    offsets[i] = total;
    total += counts[i];
  }
  std::vector<int32_t> cols((size_t)TQ_DWELL_COLS * total, -7);
  hk_pd_sample(filt.data(), theta.data(), resp.data(), U, B, G, S, N, F, seed, counts.data(), nullptr, nullptr, nullptr, nullptr,
               offsets.data(), cols.data(), total, nullptr, margins);
  std::vector<int64_t> wb((size_t)S * G * F), wu((size_t)S * G * F);
  int64_t o = 0, bad = 0, members[TQ_MIXTURE_MAX_POP] = {0, 0, 0, 0};
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const uint8_t* zr = raster.data() + ((size_t)s * N + n) * F;
      const int g = pop[(size_t)s * N + n];
      if (g >= G) {
        ++bad;
        continue;
      }
      ++members[g];
      TqDwellWalk w;
      TqDwellInterval iv;
      auto check = [&](const TqDwellInterval& v) {
        const int32_t want[TQ_DWELL_COLS] = {s, n, v.start, v.stop, v.stop + 1 - v.start, v.low_or_high, v.z};
        for (int c = 0; c < TQ_DWELL_COLS; ++c) bad += o >= total || cols[(size_t)c * total + o] != want[c];
        if (v.low_or_high == 0 || v.low_or_high == 1) ++(v.z ? wb : wu)[((size_t)s * G + g) * F + v.stop + 1 - v.start];
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
  for (int g = 0; g < G; ++g) bad += members[g] == 0;  // every population is drawn: the binning is exercised
  printf("population_dwell_check: %lld intervals, members %lld %lld %lld, %lld mismatches\n", (long long)total,
         (long long)members[0], (long long)members[1], (long long)members[2], (long long)bad);
  return bad ? 1 : 0;
}
#endif
