// tq_rates.hip -- two-state rate estimates on the device (bodies in tq_rates.h): the transition counts of posterior z rows
// drawn frame by frame, and the pooled or AOI-resampled totals with their quotients kon, koff.
#include <hip/hip_runtime.h>

#include "tq_host.h"
#include "tq_rates.h"

// ---- counts: one wave per (AOI n, block of 64 samples), one lane per sample ---------------------------------------------
// The geometry of tq_dwell_sample_kernel: every lane draws its own row (s, n) frame by frame, the row of p is staged 64
// frames at a time in LDS and read there as a broadcast.  A lane keeps three counters and the previous label; its four
// counts leave in one 16-byte store.  No atomics, no raster in memory.
__global__ __launch_bounds__(64) void tq_rates_count_kernel(const tq_rates_count_args a) {
  __shared__ float pbuf[64];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;

  TqPhilox ph;
  tq_dwell_stream(&ph, a.seed, s, n);
  TqRatesRow r;

  for (int f0 = 0; f0 < F; f0 += 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) pbuf[lane] = pr[f0 + lane];
    __syncthreads();
    if (active) {
      for (int j = 0; j < cnt; ++j) {
        const int z = tq_dwell_label(&ph, pbuf[j]);
        if (f0 + j == 0) tq_rates_begin(r, z);
        else tq_rates_step(r, z);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  int32_t c[TQ_RATES_COLS];
  tq_rates_finish(r, F, c);
  reinterpret_cast<int4*>(a.counts)[(int64_t)s * a.N + n] = make_int4(c[0], c[1], c[2], c[3]);
}

extern "C" int tq_rates_count(const tq_rates_count_args* a, void* stream) {
  if (!a || !a->p || !a->counts) {
    tq_set_error("tq_rates_count: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (((uintptr_t)a->counts & 15u) != 0) {
    tq_set_error("tq_rates_count: counts must be 16-byte aligned");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->F < 1 || a->S < 1) {
    tq_set_error("tq_rates_count: N, F and S must be positive");
    return TQ_ERR_ARG;
  }
  const dim3 grid((unsigned)a->N, (unsigned)((a->S + 63) / 64));
  if (grid.y > 65535u) {
    tq_set_error("tq_rates_count: S too large");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_rates_count_kernel, grid, dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_rates_count_kernel");
}

// ---- estimate: one wave (= one workgroup) per posterior sample ----------------------------------------------------------
// Lanes stride over i < N; with `resample` each draws its own AOI index.  A row is one 16-byte load; four int64 partial
// sums per lane, one wave reduction, and lane 0 writes the totals and the two quotients.
__global__ __launch_bounds__(64) void tq_rates_estimate_kernel(const tq_rates_estimate_args a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const uint32_t N = (uint32_t)a.N;
  const int4* rows = reinterpret_cast<const int4*>(a.counts) + (int64_t)s * a.N;
  int64_t t[TQ_RATES_COLS] = {0, 0, 0, 0};
  for (uint32_t i = lane; i < N; i += 64) {
    const uint32_t k = a.resample ? tq_rates_index(a.seed, s, i, N) : i;
    const int4 c = rows[k];
    t[0] += c.x;
    t[1] += c.y;
    t[2] += c.z;
    t[3] += c.w;
  }
#pragma unroll
  for (int j = 0; j < TQ_RATES_COLS; ++j) t[j] = tq_fit_wave_sum(t[j]);  // every lane is back here: the wave is whole
  if (lane == 0) {
    int64_t* out = a.totals + (int64_t)s * TQ_RATES_COLS;
#pragma unroll
    for (int j = 0; j < TQ_RATES_COLS; ++j) out[j] = t[j];
    double q[2];
    tq_rates_quotients(t, q);
    a.estimand[(int64_t)s * 2] = q[0];
    a.estimand[(int64_t)s * 2 + 1] = q[1];
  }
}

extern "C" int tq_rates_estimate(const tq_rates_estimate_args* a, void* stream) {
  if (!a || !a->counts || !a->totals || !a->estimand) {
    tq_set_error("tq_rates_estimate: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (((uintptr_t)a->counts & 15u) != 0) {
    tq_set_error("tq_rates_estimate: counts must be 16-byte aligned");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->S < 1 || (a->resample != 0 && a->resample != 1)) {
    tq_set_error("tq_rates_estimate: N and S must be positive and resample 0 or 1");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_rates_estimate_kernel, dim3((unsigned)a->S), dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_rates_estimate_kernel");
}
