// tq_hmm.hip -- hidden Markov smoothing with M = U + B <= 4 hidden states on the device (bodies in tq_hmm.h): the E-step
// as a chunked forward-backward with two wave scans of MxM products, the M-step of the summed rows, the Viterbi path in
// hidden states, the backward sampler with its class-level and state-level counts, the same sampler walked into dwell-time
// intervals and first-binding frames, and the pooled or AOI-resampled estimate of A (DESIGN.md
// section 22).  The kernels are templates over M; the two-state kernels of tq_smooth.hip stay.  The E-step's body and the
// M-step's sum of rows are tq_chain_dev.h's, shared with tq_multistart.hip and tq_joint.hip, and so
// are the dwell kernel's walk, its staging of thresholds and its interval sink, shared with tq_mixture.hip and
// tq_joint.hip (section 35).
#include <hip/hip_runtime.h>

#include "tq_chain_dev.h"
#include "tq_host.h"

// ---- E-step: one wave (= one workgroup) per row; the scans and the sweeps are tq_chain_estep_row ------------------------
template <int M>
__global__ __launch_bounds__(64) void tq_hmm_estep_kernel(const tq_hmm_estep_args a) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  double* filt = a.filt + (int64_t)n * F * M;
  double* gam = a.gamma + (int64_t)n * F * M;
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta, a.U, a.prior);
  tq_chain_estep_row<M, true>(m, TqHmmEmit<M>{m, pr}, F, lane, filt, gam, a.rows + (int64_t)n * TQ_HMM_COLS(M));
}

extern "C" int tq_hmm_estep(const tq_hmm_estep_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->filt || !a->gamma || !a->rows) {
    tq_set_error("tq_hmm_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_hmm_estep", a->N, a->F) || !tq_chain_states_ok("tq_hmm_estep", a->U, a->B) ||
      !tq_chain_prior_ok("tq_hmm_estep", a->prior))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_hmm_estep_kernel<MM>), dim3((unsigned)a->N), dim3(64), 0,
                                                  (hipStream_t)stream, *a));
  return tq_launch_status("tq_hmm_estep_kernel");
}

// ---- M-step: one workgroup; thread t sums rows t, t + 256, ..., then a fixed tree in LDS -------------------------------
template <int M>
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_hmm_mstep_kernel(const tq_hmm_mstep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M);
  __shared__ double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  double sums[COLS];
  if (tq_chain_reduce_rows<COLS>(a.rows, a.N, part, sums)) {
    double theta[M * M + M];
#pragma unroll
    for (int j = 0; j < M * M + M; ++j) theta[j] = a.theta[j];
    tq_hmm_mstep_theta<M>(sums, a.N, theta);
#pragma unroll
    for (int j = 0; j < M * M + M; ++j) a.theta[j] = theta[j];
    a.trace[a.it] = sums[COLS - 1];
  }
}

extern "C" int tq_hmm_mstep(const tq_hmm_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->trace) {
    tq_set_error("tq_hmm_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_iteration_ok("tq_hmm_mstep", a->N, a->it)) return TQ_ERR_ARG;
  if (!tq_chain_states_ok("tq_hmm_mstep", a->U, a->B)) return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_hmm_mstep_kernel<MM>), dim3(1), dim3(TQ_SMOOTH_MSTEP_THREADS), 0,
                                                  (hipStream_t)stream, *a));
  return tq_launch_status("tq_hmm_mstep_kernel");
}

// ---- Viterbi: one lane per row, sequential in f; the back-pointer words of a wave's rows are adjacent -------------------
template <int M>
__global__ __launch_bounds__(64) void tq_hmm_viterbi_kernel(const tq_hmm_viterbi_args a) {
  const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (n >= a.N) return;
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta, a.U, a.prior);
  tq_hmm_viterbi_row(m, a.p + n * a.F, a.F, a.back + n, a.N, a.path + n * a.F);
}

extern "C" int tq_hmm_viterbi(const tq_hmm_viterbi_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->back || !a->path) {
    tq_set_error("tq_hmm_viterbi: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_hmm_viterbi", a->N, a->F) || !tq_chain_states_ok("tq_hmm_viterbi", a->U, a->B) ||
      !tq_chain_prior_ok("tq_hmm_viterbi", a->prior))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_hmm_viterbi_kernel<MM>), dim3((unsigned)((a->N + 63) / 64)),
                                                  dim3(64), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_hmm_viterbi_kernel");
}

// ---- backward sampler: one wave per (row n, block of 64 samples), one lane per sample ----------------------------------
// The geometry of tq_smooth_count_kernel: lane j of the wave stages the M (M - 1) thresholds of frame f0 + j in LDS, then
// every lane draws its own row through the 64 frames, highest first, and only compares.  The class of a state goes
// through the row counter of the two-state sampler; the state pairs are counted by M * M compare-and-adds, so that the
// counters stay in registers.  Inactive lanes reach every barrier and touch no memory but the staging.  The device text
// is kept as it was: every shared form tried for it cost a wave per SIMD or 5 to 8 % of its time.
template <int M>
__global__ __launch_bounds__(64) void tq_hmm_count_kernel(const tq_hmm_count_args a) {
  constexpr int T = M * (M - 1);
  __shared__ double qbuf[64][T];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F, U = a.U;
  const double* fr = a.filt + (int64_t)n * F * M;
  const int64_t row = (int64_t)s * a.N + n;
  uint8_t* zr = a.raster ? a.raster + row * F : nullptr;
  const bool pairs = a.trans != nullptr;
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta, U, 0.5);  // the prior is already in filt

  TqPhilox ph;
  tq_hmm_stream(&ph, a.seed, s, n);
  TqRatesRow r = {0, 0, 0, 0};
  int next = 0;  // the state of the frame after the current one
  double u4[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t tr[M * M];
#pragma unroll
  for (int k = 0; k < M * M; ++k) tr[k] = 0;

  for (int f0 = (F - 1) & ~63; f0 >= 0; f0 -= 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) {
      double af[M], t[T];
#pragma unroll
      for (int i = 0; i < M; ++i) af[i] = fr[(int64_t)(f0 + lane) * M + i];
      tq_hmm_thresholds(m, af, f0 + lane == F - 1, t);
#pragma unroll
      for (int k = 0; k < T; ++k) qbuf[lane][k] = t[k];
    }
    __syncthreads();
    if (active) {
      for (int j = cnt - 1; j >= 0; --j) {
        const int k = F - 1 - (f0 + j);  // the frame takes the k-th uniform of the stream
        if ((k & 3) == 0) {              // one Philox block is four of them: drawn together, so its words stay in registers
#pragma unroll
          for (int q = 0; q < 4; ++q) u4[q] = (double)tq_uniform(&ph);
        }
        const double u = (k & 3) == 0 ? u4[0] : (k & 3) == 1 ? u4[1] : (k & 3) == 2 ? u4[2] : u4[3];
        const bool last = k == 0;
        const int z = tq_hmm_label<M>(u, &qbuf[j][(last ? 0 : next) * (M - 1)]);
        const int zc = z >= U ? 1 : 0;
        if (last) {
          tq_smooth_back_begin(r, zc);
        } else {
          tq_smooth_back_step(r, zc);
          if (pairs) {
            const int idx = z * M + next;
#pragma unroll
            for (int k = 0; k < M * M; ++k) tr[k] += idx == k ? 1 : 0;
          }
        }
        next = z;
        if (zr) zr[f0 + j] = (uint8_t)z;
      }
    }
    __syncthreads();
  }
  if (!active) return;
  int32_t c[TQ_RATES_COLS];
  tq_rates_finish(r, F, c);
  reinterpret_cast<int4*>(a.counts)[row] = make_int4(c[0], c[1], c[2], c[3]);
  if (pairs) {
    int32_t* out = a.trans + row * (M * M);
#pragma unroll
    for (int k = 0; k < M * M; ++k) out[k] = tr[k];
  }
}

extern "C" int tq_hmm_count(const tq_hmm_count_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->counts) {
    tq_set_error("tq_hmm_count: NULL required pointer");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_counts_aligned("tq_hmm_count", a->counts) || !tq_chain_sampler_ok("tq_hmm_count", a->N, a->F, a->S) ||
      !tq_chain_states_ok("tq_hmm_count", a->U, a->B) || !tq_chain_sample_grid("tq_hmm_count", a->N, a->S, &grid))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_hmm_count_kernel<MM>), grid, dim3(64), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_hmm_count_kernel");
}

// ---- backward sampler walked into intervals -----------------------------------------------------------------------------
// Row (s, n) is the raster tq_hmm_count_kernel draws, state for state, on the walk of tq_chain_sample_row.  Here its class
// z = (state >= U) is walked, as it is drawn, into runs of equal labels (tq_chain_dwell_frame), and neither a raster nor
// the state pairs are stored.  EMIT = false: per-row interval counts, the interior-run histograms and the first-binding
// frame; EMIT = true: the same draws again, the k-th run a row closes written at tq_smooth_emit_slot, so that the table
// is the one tq_smooth_dwell writes for that class raster (tq_chain_sink_put).
template <int M, bool EMIT>
__global__ __launch_bounds__(64) void tq_chain_dwell_kernel(const tq_chain_dwell_args a) {
  constexpr int T = M * (M - 1);
  __shared__ double qbuf[64][T];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F, U = a.U;
  const double* fr = a.filt + (int64_t)n * F * M;
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta, U, 0.5);  // the prior is already in filt
  int32_t* hb = EMIT || !active ? nullptr : a.hist_bound + (int64_t)s * F;
  int32_t* hu = EMIT || !active ? nullptr : a.hist_unbound + (int64_t)s * F;
  const int64_t total = a.total;
  int64_t o = 0;
  int count = 0;
  if (EMIT && active) {
    o = a.offsets[(int64_t)s * a.N + n];
    count = a.counts[(int64_t)s * a.N + n];
  }
  int closed = 0;  // runs closed so far
  auto sink = [&](const TqDwellInterval& v) {
    tq_chain_sink_put<EMIT>(v, closed, o, count, total, a.intervals, hb, hu, s, n);
  };

  TqHmmDraws draws;
  tq_hmm_draws_begin(draws, a.seed, s, n);
  TqChainDwellRow r;
  tq_chain_dwell_begin(r, F);
  TqDwellInterval iv;
  // M = 4 writes its twelve quotients to LDS as they come (96 VGPRs in place of 126); at M = 3 the same costs 30
  // registers, so the smaller chains go through a local array
  tq_chain_sample_row(
      F, lane, active,
      [&](int f, int l, bool last) { tq_chain_stage_thresholds<M, M == 4>(m, fr + (int64_t)f * M, last, qbuf[l]); },
      [&](int f, int j) {
        if (tq_chain_dwell_frame<M>(r, tq_hmm_draws_next(draws, F - 1 - f), qbuf[j], f, F, U, iv)) sink(iv);
      });
  if (!active) return;
  tq_chain_dwell_finish(r, iv);
  sink(iv);
  if (!EMIT) {
    const int64_t row = (int64_t)s * a.N + n;
    a.counts[row] = closed;
    if (a.tau) a.tau[row] = (float)r.tau;
  }
}

extern "C" int tq_chain_dwell(const tq_chain_dwell_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->counts) {
    tq_set_error("tq_chain_dwell: NULL required pointer");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_dwell_mode_ok("tq_chain_dwell", a->mode, a->hist_bound && a->hist_unbound,
                              a->offsets && (a->total <= 0 || a->intervals)) ||
      !tq_chain_dwell_sampler_ok("tq_chain_dwell", a->N, a->F, a->S, a->total) ||
      !tq_chain_states_ok("tq_chain_dwell", a->U, a->B) || !tq_chain_sample_grid("tq_chain_dwell", a->N, a->S, &grid))
    return TQ_ERR_ARG;
  if (a->mode == TQ_DWELL_COUNT) {
    TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_chain_dwell_kernel<MM, false>), grid, dim3(64), 0,
                                                    (hipStream_t)stream, *a));
  } else {
    if (a->total == 0) return TQ_OK;
    TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_chain_dwell_kernel<MM, true>), grid, dim3(64), 0,
                                                    (hipStream_t)stream, *a));
  }
  return tq_launch_status("tq_chain_dwell_kernel");
}

// ---- estimate: one wave (= one workgroup) per posterior sample ----------------------------------------------------------
// The geometry of tq_rates_estimate_kernel and its index draw: lanes stride over k < N, M * M int64 partial sums per lane,
// one wave reduction each (exact in any order), and lane 0 writes the totals and the row quotients.
template <int M>
__global__ __launch_bounds__(64) void tq_hmm_estimate_kernel(const tq_hmm_estimate_args a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const uint32_t N = (uint32_t)a.N;
  const int32_t* rows = a.trans + (int64_t)s * a.N * (M * M);
  int64_t t[M * M];
#pragma unroll
  for (int j = 0; j < M * M; ++j) t[j] = 0;
  for (uint32_t i = lane; i < N; i += 64) {
    const uint32_t k = a.resample ? tq_rates_index(a.seed, s, i, N) : i;  // k < N
    const int32_t* c = rows + (int64_t)k * (M * M);
#pragma unroll
    for (int j = 0; j < M * M; ++j) t[j] += c[j];
  }
#pragma unroll
  for (int j = 0; j < M * M; ++j) t[j] = tq_group_sum<64>(t[j]);  // every lane is back here: the wave is whole
  if (lane == 0) {
    int64_t* tot = a.totals + (int64_t)s * (M * M);
    double* est = a.estimand + (int64_t)s * (M * M);
#pragma unroll
    for (int i = 0; i < M; ++i) {
      int64_t rs = 0;
#pragma unroll
      for (int j = 0; j < M; ++j) rs += t[i * M + j];
#pragma unroll
      for (int j = 0; j < M; ++j) {
        tot[i * M + j] = t[i * M + j];
        est[i * M + j] = (double)t[i * M + j] / (double)rs;
      }
    }
  }
}

extern "C" int tq_hmm_estimate(const tq_hmm_estimate_args* a, void* stream) {
  if (!a || !a->trans || !a->totals || !a->estimand) {
    tq_set_error("tq_hmm_estimate: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->S < 1 || (a->resample != 0 && a->resample != 1)) {
    tq_set_error("tq_hmm_estimate: N and S must be positive and resample 0 or 1");
    return TQ_ERR_ARG;
  }
  if (a->S > 65535 * 64) {
    tq_set_error("tq_hmm_estimate: S too large");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_states_ok("tq_hmm_estimate", a->U, a->B)) return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B,
                  hipLaunchKernelGGL((tq_hmm_estimate_kernel<MM>), dim3((unsigned)a->S), dim3(64), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_hmm_estimate_kernel");
}
