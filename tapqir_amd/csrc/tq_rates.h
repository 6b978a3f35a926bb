// tq_rates.h -- two-state rate estimates (tapqir/utils/imscroll.py:199-246, 278-317), host+device inline bodies:
//   * the row counter: the four transition counts of one posterior z row, kept as it is drawn -- no raster is stored.  The
//     rows are those of the dwell-time sampler (tq_dwell.h: same stream, same site, frame f the f-th uniform), so one seed
//     gives `rates` and `dwelltime` the same rasters;
//   * the index draw of the bootstrap over AOIs and the two quotients of a sample's totals.
// The __global__ wrappers are in tq_rates.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "../../include/tapqir_hip.h"
#include "tq_dwell.h"

#define TQ_RATES_SITE 0xA02u  // Philox site id of the bootstrap indices: stream (seed, step = s, site, elem = i)

// ---- row counter ------------------------------------------------------------------------------------------------------
// Over the F - 1 frame pairs (f, f + 1) of a row:  n01 = #(0 -> 1),  n0 = #(z_f = 0),  n10 = #(1 -> 0),  n1 = #(z_f = 1).
// Three counters and the previous label; n0 = F - 1 - n1 follows at the end.
struct TqRatesRow {
  int prev, n01, n10, n1;
};

TQ_HD void tq_rates_begin(TqRatesRow& r, int z) {
  r.prev = z;
  r.n01 = r.n10 = r.n1 = 0;
}

// frame f >= 1 with label z: closes the pair (f - 1, f)
TQ_HD void tq_rates_step(TqRatesRow& r, int z) {
  r.n1 += r.prev;
  r.n01 += (1 - r.prev) & z;
  r.n10 += r.prev & (1 - z);
  r.prev = z;
}

// counts[0 .. TQ_RATES_COLS) of a row of F frames: n01, n0, n10, n1 (F = 1: four zeros)
TQ_HD void tq_rates_finish(const TqRatesRow& r, int F, int32_t* out) {
  out[0] = r.n01;
  out[1] = F - 1 - r.n1;
  out[2] = r.n10;
  out[3] = r.n1;
}

// ---- bootstrap over AOIs ------------------------------------------------------------------------------------------------
// The i-th resampled AOI of sample s: the high word of w N, w the first 32-bit word of the stream.  The 2^32 values of w
// fall into N bins whose sizes differ by at most one, so an index is over- or under-drawn by at most N / 2^32 relative to
// 1 / N (1e-7 at N = 400); no rejection loop.
TQ_HD uint32_t tq_rates_index(uint64_t seed, int s, uint32_t i, uint32_t N) {
  TqPhilox ph;
  tq_philox_init(&ph, seed, (uint32_t)s, TQ_RATES_SITE, (uint64_t)i);
  const uint32_t w = tq_philox_next(&ph);
  return (uint32_t)(((uint64_t)w * N) >> 32);
}

// kon = n01 / n0 and koff = n10 / n1 of a sample's totals: IEEE double division, so 0 / 0 is NaN and x / 0 is inf, as
// the reference's division gives
TQ_HD void tq_rates_quotients(const int64_t* totals, double* out) {
  out[0] = (double)totals[0] / (double)totals[1];
  out[1] = (double)totals[2] / (double)totals[3];
}
