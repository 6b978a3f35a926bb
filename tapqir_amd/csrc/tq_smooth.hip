// tq_smooth.hip -- two-state hidden Markov smoothing on the device (bodies in tq_smooth.h): the E-step as a chunked
// forward-backward with a wave scan of 2x2 products, the M-step of the summed rows, the Viterbi path and the backward
// sampler with its transition counts, and the same sampler walked into dwell-time intervals and
// first-binding frames.
#include <hip/hip_runtime.h>

#include "tq_dpp.h"
#include "tq_host.h"
#include "tq_smooth.h"

// ---- E-step: one wave (= one workgroup) per row, L = ceil(F / 64) consecutive frames per lane --------------------------
__device__ __forceinline__ TqSmoothMat tq_smooth_shfl_up(const TqSmoothMat& x, int d) {
  return TqSmoothMat{__shfl_up(x.m00, d, 64), __shfl_up(x.m01, d, 64), __shfl_up(x.m10, d, 64), __shfl_up(x.m11, d, 64)};
}
__device__ __forceinline__ TqSmoothMat tq_smooth_shfl_down(const TqSmoothMat& x, int d) {
  return TqSmoothMat{__shfl_down(x.m00, d, 64), __shfl_down(x.m01, d, 64), __shfl_down(x.m10, d, 64),
                     __shfl_down(x.m11, d, 64)};
}

// The chunk products C_k do not commute, so both scans keep the lane order: the prefix scan multiplies the lower lanes'
// product from the left, the suffix scan the higher lanes' from the right (Hillis-Steele, six steps each); one more
// shuffle makes them exclusive.  Every lane takes part in every shuffle.
__global__ __launch_bounds__(64) void tq_smooth_estep_kernel(const tq_smooth_estep_args a) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  double* filt = a.filt + (int64_t)n * F;
  double* gam = a.gamma + (int64_t)n * F;
  const TqSmoothModel m = tq_smooth_model(a.theta, a.prior);
  int lo, hi;
  tq_smooth_lane_range(lane, F, lo, hi);

  const TqSmoothMat c = tq_smooth_chunk(m, pr, lo, hi);
  TqSmoothMat pre = c, suf = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const TqSmoothMat left = tq_smooth_shfl_up(pre, d), right = tq_smooth_shfl_down(suf, d);
    if (lane >= d) pre = tq_smooth_mul(left, pre);
    if (lane + d < 64) suf = tq_smooth_mul(suf, right);
  }
  pre = tq_smooth_shfl_up(pre, 1);
  suf = tq_smooth_shfl_down(suf, 1);
  if (lane == 0) pre = tq_smooth_identity();
  if (lane == 63) suf = tq_smooth_identity();

  double v0, v1;
  tq_smooth_prefix_vector(pre, v0, v1);
  double acc[TQ_SMOOTH_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  acc[4] = tq_smooth_forward(m, pr, lo, hi, v0, v1, filt, gam);
  tq_smooth_backward(m, pr, lo, hi, suf.m00 + suf.m01, suf.m10 + suf.m11, v0, v1, filt, gam, acc);
#pragma unroll
  for (int j = 0; j < TQ_SMOOTH_COLS; ++j) acc[j] = tq_group_sum<64>(acc[j]);  // every lane is back here
  if (lane == 0) {
    double* out = a.rows + (int64_t)n * TQ_SMOOTH_COLS;
#pragma unroll
    for (int j = 0; j < TQ_SMOOTH_COLS; ++j) out[j] = acc[j];
  }
}

extern "C" int tq_smooth_estep(const tq_smooth_estep_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->filt || !a->gamma || !a->rows) {
    tq_set_error("tq_smooth_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->F < 1 || a->F > TQ_SMOOTH_MAX_F) {
    tq_set_error("tq_smooth_estep: N and F must be positive and F at most 65536");
    return TQ_ERR_ARG;
  }
  if (!(a->prior > 0.0 && a->prior < 1.0)) {
    tq_set_error("tq_smooth_estep: prior must lie in (0, 1)");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_smooth_estep_kernel, dim3((unsigned)a->N), dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_smooth_estep_kernel");
}

// ---- M-step: one workgroup; thread t sums rows t, t + 256, ..., then a fixed tree in LDS -------------------------------
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_smooth_mstep_kernel(const tq_smooth_mstep_args a) {
  __shared__ double part[TQ_SMOOTH_COLS][TQ_SMOOTH_MSTEP_THREADS];
  const int t = threadIdx.x;
  double s[TQ_SMOOTH_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int n = t; n < a.N; n += TQ_SMOOTH_MSTEP_THREADS) {
    const double* row = a.rows + (int64_t)n * TQ_SMOOTH_COLS;
#pragma unroll
    for (int j = 0; j < TQ_SMOOTH_COLS; ++j) s[j] += row[j];
  }
#pragma unroll
  for (int j = 0; j < TQ_SMOOTH_COLS; ++j) part[j][t] = s[j];
  __syncthreads();
  for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int j = 0; j < TQ_SMOOTH_COLS; ++j) part[j][t] += part[j][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    double sums[TQ_SMOOTH_COLS], theta[3] = {a.theta[0], a.theta[1], a.theta[2]};
#pragma unroll
    for (int j = 0; j < TQ_SMOOTH_COLS; ++j) sums[j] = part[j][0];
    tq_smooth_mstep_theta(sums, a.N, theta);
    a.theta[0] = theta[0];
    a.theta[1] = theta[1];
    a.theta[2] = theta[2];
    a.trace[a.it] = sums[4];
  }
}

extern "C" int tq_smooth_mstep(const tq_smooth_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->trace) {
    tq_set_error("tq_smooth_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->it < 0) {
    tq_set_error("tq_smooth_mstep: N must be positive and it non-negative");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_smooth_mstep_kernel, dim3(1), dim3(TQ_SMOOTH_MSTEP_THREADS), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_smooth_mstep_kernel");
}

// ---- Viterbi: one lane per row, sequential in f; the back-pointer words of a wave's rows are adjacent -------------------
__global__ __launch_bounds__(64) void tq_smooth_viterbi_kernel(const tq_smooth_viterbi_args a) {
  const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (n >= a.N) return;
  const TqSmoothModel m = tq_smooth_model(a.theta, a.prior);
  tq_smooth_viterbi_row(m, a.p + n * a.F, a.F, a.back + n, a.N, a.path + n * a.F);
}

extern "C" int tq_smooth_viterbi(const tq_smooth_viterbi_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->back || !a->path) {
    tq_set_error("tq_smooth_viterbi: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->F < 1 || a->F > TQ_SMOOTH_MAX_F) {
    tq_set_error("tq_smooth_viterbi: N and F must be positive and F at most 65536");
    return TQ_ERR_ARG;
  }
  if (!(a->prior > 0.0 && a->prior < 1.0)) {
    tq_set_error("tq_smooth_viterbi: prior must lie in (0, 1)");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_smooth_viterbi_kernel, dim3((unsigned)((a->N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_smooth_viterbi_kernel");
}

// ---- backward sampler: one wave per (row n, block of 64 samples), one lane per sample ----------------------------------
// The geometry of tq_rates_count_kernel, walked from the last frame: lane j of the wave stages the two thresholds of
// frame f0 + j in LDS, then every lane draws its own row through the 64 frames, highest first, and only compares.
__global__ __launch_bounds__(64) void tq_smooth_count_kernel(const tq_smooth_count_args a) {
  __shared__ double qbuf[2][64];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F;
  const double* fr = a.filt + (int64_t)n * F;
  uint8_t* zr = a.raster ? a.raster + ((int64_t)s * a.N + n) * F : nullptr;
  const TqSmoothModel m = tq_smooth_model(a.theta, 0.5);  // the prior is already in filt

  TqPhilox ph;
  tq_smooth_stream(&ph, a.seed, s, n);
  TqRatesRow r = {0, 0, 0, 0};

  for (int f0 = (F - 1) & ~63; f0 >= 0; f0 -= 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) tq_smooth_thresholds(m, fr[f0 + lane], f0 + lane == F - 1, qbuf[0][lane], qbuf[1][lane]);
    __syncthreads();
    if (active) {
      for (int j = cnt - 1; j >= 0; --j) {
        const bool last = f0 + j == F - 1;
        const int z = tq_smooth_label(&ph, qbuf[last ? 0 : r.prev][j]);
        if (last) tq_smooth_back_begin(r, z);
        else tq_smooth_back_step(r, z);
        if (zr) zr[f0 + j] = (uint8_t)z;
      }
    }
    __syncthreads();
  }
  if (!active) return;
  int32_t c[TQ_RATES_COLS];
  tq_rates_finish(r, F, c);
  reinterpret_cast<int4*>(a.counts)[(int64_t)s * a.N + n] = make_int4(c[0], c[1], c[2], c[3]);
}

extern "C" int tq_smooth_count(const tq_smooth_count_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->counts) {
    tq_set_error("tq_smooth_count: NULL required pointer");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_counts_aligned("tq_smooth_count", a->counts) || !tq_chain_sampler_ok("tq_smooth_count", a->N, a->F, a->S) ||
      !tq_chain_sample_grid("tq_smooth_count", a->N, a->S, &grid))
    return TQ_ERR_ARG;
  hipLaunchKernelGGL(tq_smooth_count_kernel, grid, dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_smooth_count_kernel");
}

// ---- backward sampler walked into intervals: the geometry, the staging and the draws of tq_smooth_count_kernel ----------
// Row (s, n) is the raster that kernel draws; here it is walked, as it is drawn, into runs of equal labels
// (TqSmoothWalk), and no raster is stored.  EMIT = false: per-row interval counts, the interior-run histograms (integer
// atomics: order-free, so deterministic) and the first-binding frame; EMIT = true: the same draws again, the k-th run a
// row closes written at tq_smooth_emit_slot, so that the table is the one tq_dwell_sample's EMIT writes for that raster.
template <bool EMIT>
__global__ __launch_bounds__(64) void tq_smooth_dwell_kernel(const tq_smooth_dwell_args a) {
  __shared__ double qbuf[2][64];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F;
  const double* fr = a.filt + (int64_t)n * F;
  const int64_t row = (int64_t)s * a.N + n;
  const TqSmoothModel m = tq_smooth_model(a.theta, 0.5);  // the prior is already in filt
  int32_t* hb = EMIT ? nullptr : a.hist_bound + (int64_t)s * F;
  int32_t* hu = EMIT ? nullptr : a.hist_unbound + (int64_t)s * F;
  const int64_t total = a.total;
  int64_t o = 0;
  int count = 0;
  if (EMIT && active) {
    o = a.offsets[row];
    count = a.counts[row];
  }

  TqPhilox ph;
  tq_smooth_stream(&ph, a.seed, s, n);
  TqSmoothWalk w = {0, 0, 0};
  TqDwellInterval iv;
  int closed = 0;  // runs closed so far
  int tau = F;     // the last frame seen bound: the first bound frame of the row

  auto emit = [&](const TqDwellInterval& v) {
    if (EMIT) {
      const int64_t pos = tq_smooth_emit_slot(o, count, closed, total);
      if (pos >= 0) tq_smooth_emit_row(a.intervals, total, pos, s, n, v);
    } else if (v.low_or_high == 0 || v.low_or_high == 1) {
      atomicAdd((v.z ? hb : hu) + (v.stop + 1 - v.start), 1);
    }
    ++closed;
  };

  for (int f0 = (F - 1) & ~63; f0 >= 0; f0 -= 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) tq_smooth_thresholds(m, fr[f0 + lane], f0 + lane == F - 1, qbuf[0][lane], qbuf[1][lane]);
    __syncthreads();
    if (active) {
      for (int j = cnt - 1; j >= 0; --j) {
        const int f = f0 + j;
        const bool last = f == F - 1;
        const int z = tq_smooth_label(&ph, qbuf[last ? 0 : w.cur][j]);
        if (last) tq_smooth_walk_begin(w, F, z);
        else if (tq_smooth_walk_step(w, f, z, iv)) emit(iv);
        if (!EMIT && z) tau = f;
      }
    }
    __syncthreads();
  }
  if (!active) return;
  tq_smooth_walk_finish(w, iv);
  emit(iv);
  if (!EMIT) {
    a.counts[row] = closed;
    if (a.tau) a.tau[row] = (float)tau;
  }
}

extern "C" int tq_smooth_dwell(const tq_smooth_dwell_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->counts) {
    tq_set_error("tq_smooth_dwell: NULL required pointer");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_dwell_mode_ok("tq_smooth_dwell", a->mode, a->hist_bound && a->hist_unbound,
                              a->offsets && (a->total <= 0 || a->intervals)) ||
      !tq_chain_dwell_sampler_ok("tq_smooth_dwell", a->N, a->F, a->S, a->total) ||
      !tq_chain_sample_grid("tq_smooth_dwell", a->N, a->S, &grid))
    return TQ_ERR_ARG;
  if (a->mode == TQ_DWELL_COUNT) {
    hipLaunchKernelGGL(tq_smooth_dwell_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, *a);
  } else {
    if (a->total == 0) return TQ_OK;
    hipLaunchKernelGGL(tq_smooth_dwell_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, *a);
  }
  return tq_launch_status("tq_smooth_dwell_kernel");
}
