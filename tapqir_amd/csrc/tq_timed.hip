// tq_timed.hip -- the continuous-time hidden Markov chain on the frame timestamps on the device (`smooth --timed`,
// DESIGN.md section 34; bodies in tq_timed.h and tq_hmm.h): the tables P = exp(Q d) and K of every gap class, the E-step
// -- the chunked forward-backward of tq_hmm_estep, the same text, with the transition of a frame read from its gap's class
// and the expected jumps and holding times for the pair marginals -- and the M-step of the summed rows.  No floating-point
// atomics, no workgroup waits on another, every loop bounded by F, N, TQ_TIMED_ORDER or TQ_TIMED_MAX_SQ.
#include <hip/hip_runtime.h>
#include <math.h>

#include "tq_chain_dev.h"
#include "tq_host.h"
#include "tq_timed.h"

// ---- tables: one thread per (class, i, j) ---------------------------------------------------------------------------------
// Thread (k, i * M + j) carries P and the M x M matrix K[k][.][.][i][j] through the series and the squarings in registers;
// it needs no other thread, so the grid is flat and a thread beyond D * M * M leaves at once.
template <int M>
__global__ __launch_bounds__(64) void tq_timed_table_kernel(const tq_timed_table_args a) {
  const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= (int64_t)a.D * (M * M)) return;
  const TqTimedModel<M> m = tq_timed_model<M>(a.theta, a.U, 0.5, a.allow);
  tq_timed_table_item<M>(m, a.d, (int)(t / (M * M)), (int)(t % (M * M)), a.P, a.K);
}

extern "C" int tq_timed_table(const tq_timed_table_args* a, void* stream) {
  if (!a || !a->theta || !a->d || !a->d_host || !a->P || !a->K) {
    tq_set_error("tq_timed_table: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->D < 1) {
    tq_set_error("tq_timed_table: D must be positive");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_states_ok("tq_timed_table", a->U, a->B)) return TQ_ERR_ARG;
  if (!tq_chain_allow_ok("tq_timed_table", tq_multistart_allow_ok(a->allow, a->U + a->B)))
    return TQ_ERR_ARG;
  for (int k = 0; k < a->D; ++k)
    if (!(a->d_host[k] > 0.0) || !isfinite(a->d_host[k])) {
      tq_set_error("tq_timed_table: every gap must be finite and positive");
      return TQ_ERR_ARG;
    }
  const int M = a->U + a->B;
  const int64_t items = (int64_t)a->D * M * M;
  TQ_HMM_SWITCH_M(M, hipLaunchKernelGGL((tq_timed_table_kernel<MM>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0,
                                        (hipStream_t)stream, *a));
  return tq_launch_status("tq_timed_table_kernel");
}

// ---- E-step: one wave (= one workgroup) per row ---------------------------------------------------------------------------
// tq_chain_estep_row, as tq_hmm_estep_kernel calls it, given the timed chain: its transition of a frame and its pair sums
// (tq_timed.h) are what the shared chunk product and backward sweep ask it for; the forward sweep is its overload.
template <int M, bool GAMMA>
__global__ __launch_bounds__(64) void tq_timed_estep_kernel(const tq_timed_estep_args a) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  double* filt = a.filt + (int64_t)n * F * M;
  double* gam = GAMMA ? a.gamma + (int64_t)n * F * M : nullptr;
  const TqTimedChain<M> m = tq_timed_chain<M>(a.theta, a.U, a.prior, a.allow, a.P, a.K, a.cls);
  tq_chain_estep_row<M, GAMMA>(m, TqTimedEmit<M>{m, pr}, F, lane, filt, gam, a.rows + (int64_t)n * TQ_HMM_COLS(M));
}

extern "C" int tq_timed_estep(const tq_timed_estep_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->P || !a->K || !a->filt || !a->rows) {
    tq_set_error("tq_timed_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_timed_estep", a->N, a->F) || !tq_chain_states_ok("tq_timed_estep", a->U, a->B) ||
      !tq_chain_prior_ok("tq_timed_estep", a->prior))
    return TQ_ERR_ARG;
  if (a->D < 1) {
    tq_set_error("tq_timed_estep: D must be positive");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_allow_ok("tq_timed_estep", tq_multistart_allow_ok(a->allow, a->U + a->B)))
    return TQ_ERR_ARG;
  if (a->F > 1 && (!a->cls || !a->cls_host)) {
    tq_set_error("tq_timed_estep: NULL cls or cls_host with more than one frame");
    return TQ_ERR_ARG;
  }
  for (int f = 0; f + 1 < a->F; ++f)
    if (a->cls_host[f] < 0 || a->cls_host[f] >= a->D) {
      tq_set_error("tq_timed_estep: every class index must lie in [0, D)");
      return TQ_ERR_ARG;
    }
  if (a->gamma) {
    TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_timed_estep_kernel<MM, true>), dim3((unsigned)a->N), dim3(64), 0,
                                                    (hipStream_t)stream, *a));
  } else {
    TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_timed_estep_kernel<MM, false>), dim3((unsigned)a->N), dim3(64), 0,
                                                    (hipStream_t)stream, *a));
  }
  return tq_launch_status("tq_timed_estep_kernel");
}

// ---- M-step: one workgroup; thread t sums rows t, t + 256, ..., then a fixed tree in LDS -------------------------------
template <int M>
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_timed_mstep_kernel(const tq_timed_mstep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M);
  __shared__ double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  double sums[COLS];
  if (tq_chain_reduce_rows<COLS>(a.rows, a.N, part, sums)) {
    double theta[M * M + M];
#pragma unroll
    for (int j = 0; j < M * M + M; ++j) theta[j] = a.theta[j];
    tq_timed_mstep_theta<M>(sums, a.N, a.allow, theta);
#pragma unroll
    for (int j = 0; j < M * M + M; ++j) a.theta[j] = theta[j];
    a.trace[a.it] = sums[COLS - 1];
  }
}

extern "C" int tq_timed_mstep(const tq_timed_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->trace) {
    tq_set_error("tq_timed_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_iteration_ok("tq_timed_mstep", a->N, a->it) ||
      !tq_chain_trace_ok("tq_timed_mstep", a->it, a->T, "the trace"))
    return TQ_ERR_ARG;
  if (!tq_chain_states_ok("tq_timed_mstep", a->U, a->B)) return TQ_ERR_ARG;
  if (!tq_chain_allow_ok("tq_timed_mstep", tq_multistart_allow_ok(a->allow, a->U + a->B)))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_timed_mstep_kernel<MM>), dim3(1), dim3(TQ_SMOOTH_MSTEP_THREADS), 0,
                                                  (hipStream_t)stream, *a));
  return tq_launch_status("tq_timed_mstep_kernel");
}
