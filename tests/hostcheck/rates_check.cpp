// g++ build of the two-state rate bodies (tapqir_amd/csrc/tq_rates.h) on host memory, for the test suite: the row counter
// on given rasters and on the sampler's own draws, the bootstrap index draw and the quotients.
#include "../../tapqir_amd/csrc/tq_rates.h"

extern "C" {

// the row counter on a given (S, N, F) raster of 0/1 labels: counts (S, N, TQ_RATES_COLS)
void hk_rates_count(const int32_t* z, int S, int N, int F, int32_t* counts) {
  for (int64_t row = 0; row < (int64_t)S * N; ++row) {
    const int32_t* zr = z + row * F;
    TqRatesRow r;
    tq_rates_begin(r, zr[0] != 0);
    for (int f = 1; f < F; ++f) tq_rates_step(r, zr[f] != 0);
    tq_rates_finish(r, F, counts + row * TQ_RATES_COLS);
  }
}

// the draws and the count of tq_rates_count
void hk_rates_sample(const float* p, int S, int N, int F, uint64_t seed, int32_t* counts) {
  for (int s = 0; s < S; ++s)
    for (int n = 0; n < N; ++n) {
      TqPhilox ph;
      tq_dwell_stream(&ph, seed, s, n);
      const float* pr = p + (int64_t)n * F;
      TqRatesRow r;
      tq_rates_begin(r, tq_dwell_label(&ph, pr[0]));
      for (int f = 1; f < F; ++f) tq_rates_step(r, tq_dwell_label(&ph, pr[f]));
      tq_rates_finish(r, F, counts + ((int64_t)s * N + n) * TQ_RATES_COLS);
    }
}

// the i-th resampled AOI of sample s
uint32_t hk_rates_index(uint64_t seed, int s, uint32_t i, uint32_t N) { return tq_rates_index(seed, s, i, N); }

// indices (S, N) of a whole bootstrap
void hk_rates_indices(uint64_t seed, int S, uint32_t N, int64_t* out) {
  for (int s = 0; s < S; ++s)
    for (uint32_t i = 0; i < N; ++i) out[(int64_t)s * N + i] = tq_rates_index(seed, s, i, N);
}

// out = [kon, koff] of totals[4]
void hk_rates_quotients(const int64_t* totals, double* out) { tq_rates_quotients(totals, out); }
}
