// tq_mixture.hip -- a mixture of G <= 4 chains of tq_hmm.h over the AOIs on the device (`smooth --populations G`,
// DESIGN.md section 29; bodies in tq_mixture.h): the M-step that weights every AOI by its responsibility, on a grid of one
// workgroup per start; the backward sampler that draws a population with every raster; the same sampler walked into
// dwell-time intervals and first-binding frames (tq_population_dwell, section 30); and the per-population estimate of A.
// The E-step is tq_multistart_estep with R = P * G.  tq_population_dwell runs on the walk and the interval sink that
// tq_chain_dev.h shares with tq_hmm.hip and tq_joint.hip.  No atomics
// but the integer histogram bins of tq_population_dwell, no workgroup waits on another, every loop bounded by N, F, S or G.
#include <hip/hip_runtime.h>

#include "tq_chain_dev.h"
#include "tq_host.h"
#include "tq_mixture.h"
#include "tq_rates.h"

static inline bool tq_mixture_pops_ok(const char* who, int G) {
  return tq_chain_require(G >= 1 && G <= TQ_MIXTURE_MAX_POP, who, "G must be at least 1 and at most " TQ_STR(TQ_MIXTURE_MAX_POP));
}

// ---- M-step: one workgroup per start ------------------------------------------------------------------------------------
// Every thread forms ev and w of its rows t, t + 256, ... from the G logliks, once per population; the columns of
// population g times w[g] go through the strided sum and the tree of tq_chain_reduce_rows -- the same order of additions,
// so the same bits at w = 1 -- in one LDS array, one population after the other.  Columns: the M * M + M weighted sums,
// then sum w, then sum ev.  Thread 0 alone writes theta, phi and trace; phi is read by every thread before the first
// barrier and written after the last.
template <int M>
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_mixture_mstep_kernel(const tq_mixture_mstep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M), W = M * M + M;
  __shared__ double part[COLS + 1][TQ_SMOOTH_MSTEP_THREADS];
  __shared__ double wsum[TQ_MIXTURE_MAX_POP];  // thread 0's alone
  const int p = blockIdx.x, t = threadIdx.x, G = a.G, N = a.N;
  if (a.active && a.active[p] == 0) return;  // the whole workgroup, before its first barrier
  const double* rows = a.rows + tq_multistart_row_at<M>(tq_mixture_replica(p, 0, G), 0, N);
  const int64_t stride = (int64_t)N * COLS;  // from population g to g + 1
  double lphi[TQ_MIXTURE_MAX_POP];
  tq_mixture_log_weights(a.phi + (int64_t)p * G, G, lphi);

  for (int g = 0; g < G; ++g) {
    double s[COLS + 1];
#pragma unroll
    for (int j = 0; j < COLS + 1; ++j) s[j] = 0.0;
    for (int n = t; n < N; n += TQ_SMOOTH_MSTEP_THREADS) {
      double w[TQ_MIXTURE_MAX_POP];
      const double ev = tq_mixture_evidence(rows + (int64_t)n * COLS + COLS - 1, stride, lphi, G, w);
      const double wg = tq_mixture_pick(w, g);
      const double* row = rows + g * stride + (int64_t)n * COLS;
#pragma unroll
      for (int j = 0; j < W; ++j) s[j] += wg * row[j];
      s[W] += wg;
      s[COLS] += ev;
      if (g == 0) {
        if (a.evidence) a.evidence[(int64_t)p * N + n] = ev;
        if (a.resp) {
#pragma unroll
          for (int k = 0; k < TQ_MIXTURE_MAX_POP; ++k)
            if (k < G) a.resp[((int64_t)p * G + k) * N + n] = w[k];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < COLS + 1; ++j) part[j][t] = s[j];
    __syncthreads();
    for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1) {
      if (t < h) {
#pragma unroll
        for (int j = 0; j < COLS + 1; ++j) part[j][t] += part[j][t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
      double sums[W], theta[W];
      double* th = a.theta + tq_multistart_theta_at<M>(tq_mixture_replica(p, g, G));
#pragma unroll
      for (int j = 0; j < W; ++j) {
        sums[j] = part[j][0];
        theta[j] = th[j];
      }
      wsum[g] = part[W][0];
      tq_mixture_mstep_theta<M>(sums, wsum[g], a.allow, theta);
#pragma unroll
      for (int j = 0; j < W; ++j) th[j] = theta[j];
      if (g == 0) a.trace[(int64_t)p * a.T + a.it] = part[COLS][0];
    }
  }
  if (t == 0) {
    double phi[TQ_MIXTURE_MAX_POP];
    tq_mixture_mstep_phi(wsum, G, N, phi);
    for (int g = 0; g < G; ++g) a.phi[(int64_t)p * G + g] = phi[g];
  }
}

extern "C" int tq_mixture_mstep(const tq_mixture_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->phi || !a->trace) {
    tq_set_error("tq_mixture_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_iteration_ok("tq_mixture_mstep", a->N, a->it) ||
      !tq_chain_trace_ok("tq_mixture_mstep", a->it, a->T, "the trace of a start"))
    return TQ_ERR_ARG;
  if (!tq_chain_states_ok("tq_mixture_mstep", a->U, a->B) || !tq_mixture_pops_ok("tq_mixture_mstep", a->G)) return TQ_ERR_ARG;
  if (a->P < 1 || a->P > TQ_MULTISTART_MAX / a->G) {
    tq_set_error("tq_mixture_mstep: P must be at least 1 and P * G at most " TQ_STR(TQ_MULTISTART_MAX));
    return TQ_ERR_ARG;
  }
  if (!tq_chain_allow_ok("tq_mixture_mstep", tq_multistart_allow_ok(a->allow, a->U + a->B)))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_mixture_mstep_kernel<MM>), dim3((unsigned)a->P),
                                                  dim3(TQ_SMOOTH_MSTEP_THREADS), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_mixture_mstep_kernel");
}

// ---- backward sampler: one wave per (row n, block of 64 samples), one lane per sample ----------------------------------
// tq_hmm_count_kernel with a population drawn first.  The lanes of a wave may then hold different ones, so lane j stages
// the thresholds of frame f0 + j for all G populations and the draw reads qbuf[g][j]: addresses diverge, control flow
// does not, and every lane reaches every barrier; inactive lanes touch no memory but the staging.
// qbuf[G][64][M (M - 1)] is the launch's dynamic LDS, so that one population takes the LDS of tq_hmm_count_kernel and four
// take 24 KB at M = 4.  The G chains as they are read (tq_hmm_model) are set up once, by lanes 0 .. G - 1, in LDS, and a
// barrier stands between that and the first block.  The device text is kept as it was, as tq_hmm_count_kernel's is
// (DESIGN.md section 35 says what the shared forms cost it).
template <int M>
__global__ __launch_bounds__(64) void tq_mixture_count_kernel(const tq_mixture_count_args a) {
  constexpr int T = M * (M - 1);
  extern __shared__ double qbuf[];  // [G][64][T]
  __shared__ TqHmmModel<M> mods[TQ_MIXTURE_MAX_POP];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F, U = a.U, G = a.G, N = a.N;
  const int64_t row = (int64_t)s * N + n;
  uint8_t* zr = a.raster ? a.raster + row * F : nullptr;
  const bool pairs = a.trans != nullptr;
  if (lane < G) mods[lane] = tq_hmm_model<M>(a.theta + tq_multistart_theta_at<M>(lane), U, 0.5);  // the prior is in filt

  const int g = active ? tq_mixture_population(a.seed, s, n, a.resp + n, N, G) : 0;
  TqPhilox ph;
  tq_hmm_stream(&ph, a.seed, s, n);
  TqRatesRow r = {0, 0, 0, 0};
  int next = 0;  // the state of the frame after the current one
  double u4[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t tr[M * M];
#pragma unroll
  for (int k = 0; k < M * M; ++k) tr[k] = 0;
  __syncthreads();

  for (int f0 = (F - 1) & ~63; f0 >= 0; f0 -= 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) {
      for (int gp = 0; gp < G; ++gp) {
        const double* fr = a.filt + tq_multistart_filt_at<M>(gp, n, N, F) + (int64_t)(f0 + lane) * M;
        double af[M], t[T];
#pragma unroll
        for (int i = 0; i < M; ++i) af[i] = fr[i];
        tq_hmm_thresholds(mods[gp], af, f0 + lane == F - 1, t);
#pragma unroll
        for (int k = 0; k < T; ++k) qbuf[(gp * 64 + lane) * T + k] = t[k];
      }
    }
    __syncthreads();
    if (active) {
      for (int j = cnt - 1; j >= 0; --j) {
        const int k = F - 1 - (f0 + j);  // the frame takes the k-th uniform of the stream
        if ((k & 3) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) u4[q] = (double)tq_uniform(&ph);
        }
        const double u = (k & 3) == 0 ? u4[0] : (k & 3) == 1 ? u4[1] : (k & 3) == 2 ? u4[2] : u4[3];
        const bool last = k == 0;
        const int z = tq_hmm_label<M>(u, &qbuf[(g * 64 + j) * T + (last ? 0 : next) * (M - 1)]);
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
  a.pop[row] = (uint8_t)g;
  if (pairs) {
    int32_t* out = a.trans + row * (M * M);
#pragma unroll
    for (int k = 0; k < M * M; ++k) out[k] = tr[k];
  }
}

extern "C" int tq_mixture_count(const tq_mixture_count_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->resp || !a->counts || !a->pop) {
    tq_set_error("tq_mixture_count: NULL required pointer");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_counts_aligned("tq_mixture_count", a->counts) || !tq_chain_sampler_ok("tq_mixture_count", a->N, a->F, a->S) ||
      !tq_chain_states_ok("tq_mixture_count", a->U, a->B) || !tq_mixture_pops_ok("tq_mixture_count", a->G) ||
      !tq_chain_sample_grid("tq_mixture_count", a->N, a->S, &grid))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_mixture_count_kernel<MM>), grid, dim3(64),
                                                  (size_t)a->G * 64 * MM * (MM - 1) * sizeof(double), (hipStream_t)stream, *a));
  return tq_launch_status("tq_mixture_count_kernel");
}

// ---- backward sampler walked into intervals -----------------------------------------------------------------------------
// Row (s, n) is the raster tq_mixture_count_kernel draws, population for population and state for state
// (tq_mixture_population, then TqHmmDraws against qbuf[g][j]), on the walk of tq_chain_sample_row.  Here its class
// z = (state >= U) is walked, as it is drawn, into runs of equal labels (tq_chain_dwell_frame), and neither a raster nor
// the state pairs are kept.  EMIT = false: per-row interval counts, the drawn population, the first-binding frame, and
// the interior-run histograms of the row's population; EMIT = true: the same draws again, the k-th run a row closes
// written at tq_smooth_emit_slot (tq_chain_sink_put).  Every loop is bounded by F or G.  M = 4 writes its quotients to LDS
// as they come, as tq_chain_dwell_kernel does, but in its own text: through tq_chain_stage_thresholds the COUNT kernels
// take 100 and 116 VGPRs at M = 3 and 4 in place of 68 and 76.
template <int M, bool EMIT>
__global__ __launch_bounds__(64) void tq_population_dwell_kernel(const tq_population_dwell_args a) {
  constexpr int T = M * (M - 1);
  extern __shared__ double qbuf[];  // [G][64][T]
  __shared__ TqHmmModel<M> mods[TQ_MIXTURE_MAX_POP];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F, U = a.U, G = a.G, N = a.N;
  const int64_t row = (int64_t)s * N + n;
  if (lane < G) mods[lane] = tq_hmm_model<M>(a.theta + tq_multistart_theta_at<M>(lane), U, 0.5);  // the prior is in filt

  const int g = active ? tq_mixture_population(a.seed, s, n, a.resp + n, N, G) : 0;  // g < G
  int32_t* hb = EMIT || !active ? nullptr : a.hist_bound + tq_population_hist_at(s, g, G, F);
  int32_t* hu = EMIT || !active ? nullptr : a.hist_unbound + tq_population_hist_at(s, g, G, F);
  const int64_t total = a.total;
  int64_t o = 0;
  int count = 0;
  if (EMIT && active) {
    o = a.offsets[row];
    count = a.counts[row];
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
  __syncthreads();
  tq_chain_sample_row(
      F, lane, active,
      [&](int f, int l, bool last) {
        for (int gp = 0; gp < G; ++gp) {
          const double* fr = a.filt + tq_multistart_filt_at<M>(gp, n, N, F) + (int64_t)f * M;
          double* q = qbuf + (gp * 64 + l) * T;
          double af[M];
#pragma unroll
          for (int i = 0; i < M; ++i) af[i] = fr[i];
          if constexpr (M == 4) {
            tq_hmm_thresholds(mods[gp], af, last, q);
          } else {
            double t[T];
            tq_hmm_thresholds(mods[gp], af, last, t);
#pragma unroll
            for (int k = 0; k < T; ++k) q[k] = t[k];
          }
        }
      },
      [&](int f, int j) {
        if (tq_chain_dwell_frame<M>(r, tq_hmm_draws_next(draws, F - 1 - f), qbuf + (g * 64 + j) * T, f, F, U, iv)) sink(iv);
      });
  if (!active) return;
  tq_chain_dwell_finish(r, iv);
  sink(iv);
  if (!EMIT) {
    a.counts[row] = closed;
    a.pop[row] = (uint8_t)g;
    if (a.tau) a.tau[row] = (float)r.tau;
  }
}

extern "C" int tq_population_dwell(const tq_population_dwell_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->resp || !a->counts) {
    tq_set_error("tq_population_dwell: NULL required pointer");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_dwell_mode_ok("tq_population_dwell", a->mode, a->pop && a->hist_bound && a->hist_unbound,
                              a->offsets && (a->total <= 0 || a->intervals)) ||
      !tq_chain_dwell_sampler_ok("tq_population_dwell", a->N, a->F, a->S, a->total) ||
      !tq_chain_states_ok("tq_population_dwell", a->U, a->B) || !tq_mixture_pops_ok("tq_population_dwell", a->G) ||
      !tq_chain_sample_grid("tq_population_dwell", a->N, a->S, &grid))
    return TQ_ERR_ARG;
  if (a->mode == TQ_DWELL_COUNT) {
    TQ_HMM_SWITCH_M(a->U + a->B,
                    hipLaunchKernelGGL((tq_population_dwell_kernel<MM, false>), grid, dim3(64),
                                       (size_t)a->G * 64 * MM * (MM - 1) * sizeof(double), (hipStream_t)stream, *a));
  } else {
    if (a->total == 0) return TQ_OK;
    TQ_HMM_SWITCH_M(a->U + a->B,
                    hipLaunchKernelGGL((tq_population_dwell_kernel<MM, true>), grid, dim3(64),
                                       (size_t)a->G * 64 * MM * (MM - 1) * sizeof(double), (hipStream_t)stream, *a));
  }
  return tq_launch_status("tq_population_dwell_kernel");
}

// ---- estimate: one wave (= one workgroup) per posterior sample ----------------------------------------------------------
// tq_hmm_estimate_kernel, one population after the other so that the M * M partial sums of a lane stay in registers: the
// index draw is repeated per population and the rows of the others are skipped.  Every lane runs every wave reduction.
template <int M>
__global__ __launch_bounds__(64) void tq_mixture_estimate_kernel(const tq_mixture_estimate_args a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const uint32_t N = (uint32_t)a.N;
  const int32_t* rows = a.trans + (int64_t)s * a.N * (M * M);
  const uint8_t* pop = a.pop + (int64_t)s * a.N;
  for (int g = 0; g < a.G; ++g) {
    int64_t t[M * M], cnt = 0;
#pragma unroll
    for (int j = 0; j < M * M; ++j) t[j] = 0;
    for (uint32_t i = lane; i < N; i += 64) {
      const uint32_t k = a.resample ? tq_rates_index(a.seed, s, i, N) : i;  // k < N
      if ((int)pop[k] != g) continue;
      const int32_t* c = rows + (int64_t)k * (M * M);
#pragma unroll
      for (int j = 0; j < M * M; ++j) t[j] += c[j];
      cnt += 1;
    }
#pragma unroll
    for (int j = 0; j < M * M; ++j) t[j] = tq_group_sum<64>(t[j]);  // every lane is back here: the wave is whole
    cnt = tq_group_sum<64>(cnt);
    if (lane == 0) {
      int64_t* tot = a.totals + ((int64_t)s * a.G + g) * (M * M);
      double* est = a.estimand + ((int64_t)s * a.G + g) * (M * M);
      a.members[(int64_t)s * a.G + g] = cnt;
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
}

extern "C" int tq_mixture_estimate(const tq_mixture_estimate_args* a, void* stream) {
  if (!a || !a->trans || !a->pop || !a->totals || !a->members || !a->estimand) {
    tq_set_error("tq_mixture_estimate: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->S < 1 || (a->resample != 0 && a->resample != 1)) {
    tq_set_error("tq_mixture_estimate: N and S must be positive and resample 0 or 1");
    return TQ_ERR_ARG;
  }
  if (a->S > 65535 * 64) {
    tq_set_error("tq_mixture_estimate: S too large");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_states_ok("tq_mixture_estimate", a->U, a->B) || !tq_mixture_pops_ok("tq_mixture_estimate", a->G))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_mixture_estimate_kernel<MM>), dim3((unsigned)a->S), dim3(64), 0,
                                                  (hipStream_t)stream, *a));
  return tq_launch_status("tq_mixture_estimate_kernel");
}
