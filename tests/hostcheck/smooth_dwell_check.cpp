// g++ build of the backward interval walker and of the draws of tq_smooth_dwell (tapqir_amd/csrc/tq_smooth.h) on host
// memory, for the test suite: the walker on given rasters, and a replay of both modes of the entry point per row, with the
// kernel's order of draws (u_0 for frame F - 1, then downwards).  With -DSMOOTH_DWELL_MAIN the file is a stand-alone
// program that replays one case and checks it against a forward walk of the replayed raster (for a sanitizer build).
#include "../../tapqir_amd/csrc/tq_smooth.h"

namespace {

// One row visited from frame F - 1 down to 0, labels from `label(f)`.  COUNT (cols == nullptr): the number of intervals is
// returned, interior runs go to the histogram rows hb / hu (when given) and *tau is the first bound frame.  EMIT: the
// k-th closed run is written at tq_smooth_emit_slot(o, count, k, total).
template <class Label>
int walk_row(Label label, int s, int n, int F, int32_t* hb, int32_t* hu, float* tau, int32_t* cols, int64_t o, int count,
             int64_t total) {
  TqSmoothWalk w = {0, 0, 0};
  TqDwellInterval iv;
  int closed = 0, first_bound = F;
  auto put = [&](const TqDwellInterval& v) {
    if (cols) {
      const int64_t pos = tq_smooth_emit_slot(o, count, closed, total);
      if (pos >= 0) tq_smooth_emit_row(cols, total, pos, s, n, v);
    } else if (hb && (v.low_or_high == 0 || v.low_or_high == 1)) {
      ++(v.z ? hb : hu)[v.stop + 1 - v.start];
    }
    ++closed;
  };
  for (int f = F - 1; f >= 0; --f) {
    const int z = label(f, w.cur);
    if (f == F - 1) tq_smooth_walk_begin(w, F, z);
    else if (tq_smooth_walk_step(w, f, z, iv)) put(iv);
    if (z) first_bound = f;
  }
  tq_smooth_walk_finish(w, iv);
  put(iv);
  if (tau) *tau = (float)first_bound;
  return closed;
}

}  // namespace

extern "C" {

// the walker on a given (S, N, F) raster of 0/1 bytes.  cols == NULL: counts (S, N), histograms (S, F), tau (S, N);
// otherwise the table (7, total) from `counts` and `offsets`.
void hk_sd_walk(const uint8_t* z, int S, int N, int F, int32_t* counts, int32_t* hb, int32_t* hu, float* tau,
                const int64_t* offsets, int32_t* cols, int64_t total) {
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      const uint8_t* zr = z + row * F;
      auto label = [&](int f, int) { return zr[f] != 0 ? 1 : 0; };
      if (cols) walk_row(label, s, n, F, nullptr, nullptr, nullptr, cols, offsets[row], counts[row], total);
      else counts[row] = walk_row(label, s, n, F, hb + (int64_t)s * F, hu + (int64_t)s * F, tau + row, nullptr, 0, 0, 0);
    }
}

// the draws and the walk of tq_smooth_dwell: COUNT (cols == NULL) or EMIT
void hk_sd_sample(const double* filt, const double* theta, int S, int N, int F, uint64_t seed, int32_t* counts, int32_t* hb,
                  int32_t* hu, float* tau, const int64_t* offsets, int32_t* cols, int64_t total) {
  const TqSmoothModel m = tq_smooth_model(theta, 0.5);
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      const int64_t row = (int64_t)s * N + n;
      const double* fr = filt + (int64_t)n * F;
      TqPhilox ph;
      tq_smooth_stream(&ph, seed, s, n);
      auto label = [&](int f, int next) {
        double q0, q1;
        tq_smooth_thresholds(m, fr[f], f == F - 1, q0, q1);
        return tq_smooth_label(&ph, (f == F - 1 || next == 0) ? q0 : q1);
      };
      if (cols) walk_row(label, s, n, F, nullptr, nullptr, nullptr, cols, offsets[row], counts[row], total);
      else counts[row] = walk_row(label, s, n, F, hb + (int64_t)s * F, hu + (int64_t)s * F, tau ? tau + row : nullptr,
                                  nullptr, 0, 0, 0);
    }
}

int64_t hk_sd_emit_slot(int64_t o, int count, int k, int64_t total) { return tq_smooth_emit_slot(o, count, k, total); }
}

#ifdef SMOOTH_DWELL_MAIN
#include <stdio.h>

#include <vector>

// N = 6, F = 65, S = 70: filt from a fixed recurrence, COUNT, the scan, EMIT into a table with a guard column behind it, and
// a forward walk (tq_dwell.h) of the same labels as the cross-check.  Exit status 0 when the two agree.
int main() {
  const int S = 70, N = 6, F = 65;
  const uint64_t seed = 0;
  const double theta[3] = {0.05, 0.10, 0.4};
  std::vector<double> filt((size_t)N * F);
  uint32_t x = 12345u;
  for (double& v : filt) {
    x = x * 1664525u + 1013904223u;
    v = ((x >> 8) + 0.5) / 16777216.0;
  }
  for (int f = 0; f < F; ++f) {  // rows 0 and 1: never and always bound
    filt[f] = 0.0;
    filt[F + f] = 1.0;
  }
  std::vector<int32_t> counts((size_t)S * N), hb((size_t)S * F), hu((size_t)S * F);
  std::vector<float> tau((size_t)S * N);
  hk_sd_sample(filt.data(), theta, S, N, F, seed, counts.data(), hb.data(), hu.data(), tau.data(), nullptr, nullptr, 0);
  std::vector<int64_t> offsets((size_t)S * N);
  int64_t total = 0;
  for (size_t i = 0; i < counts.size(); ++i) {
    offsets[i] = total;
    total += counts[i];
  }
  std::vector<int32_t> cols((size_t)TQ_DWELL_COLS * total, -7);
  hk_sd_sample(filt.data(), theta, S, N, F, seed, counts.data(), nullptr, nullptr, nullptr, offsets.data(), cols.data(),
               total);
  // the same labels once more, stored, and walked forwards
  const TqSmoothModel m = tq_smooth_model(theta, 0.5);
  std::vector<uint8_t> z(F);
  int64_t o = 0, bad = 0;
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      TqPhilox ph;
      tq_smooth_stream(&ph, seed, s, n);
      int next = 0;
      for (int f = F - 1; f >= 0; --f) {
        double q0, q1;
        tq_smooth_thresholds(m, filt[(size_t)n * F + f], f == F - 1, q0, q1);
        next = tq_smooth_label(&ph, (f == F - 1 || next == 0) ? q0 : q1);
        z[f] = (uint8_t)next;
      }
      TqDwellWalk w;
      TqDwellInterval iv;
      auto check = [&](const TqDwellInterval& v) {
        const int32_t want[TQ_DWELL_COLS] = {s, n, v.start, v.stop, v.stop + 1 - v.start, v.low_or_high, v.z};
        for (int c = 0; c < TQ_DWELL_COLS; ++c) bad += o >= total || cols[(size_t)c * total + o] != want[c];
        ++o;
      };
      tq_dwell_begin(w, z[0]);
      for (int f = 1; f < F; ++f)
        if (tq_dwell_step(w, f, z[f], iv)) check(iv);
      tq_dwell_finish(w, F, iv);
      check(iv);
      int first = F;
      for (int f = F - 1; f >= 0; --f)
        if (z[f]) first = f;
      bad += tau[(size_t)s * N + n] != (float)first;
    }
  bad += o != total;
  printf("smooth_dwell_check: %lld intervals, %lld mismatches\n", (long long)total, (long long)bad);
  return bad ? 1 : 0;
}
#endif
