// tq_refit.hip -- R bootstrap refits of the chain of tq_hmm.h over AOIs, side by side on the device (`smooth --refit`,
// DESIGN.md section 33; bodies in tq_refit.h, tq_multistart.h and tq_hmm.h): the AOI weights of R resamples, the E-step of
// tq_multistart_estep that leaves out the (replica, AOI) pairs a resample did not draw, and the M-step of
// tq_multistart_mstep with every row weighted by how often its AOI was drawn.  No floating-point atomics, no workgroup
// waits on another, every loop bounded by F, N or R.
#include <hip/hip_runtime.h>

#include "tq_chain_dev.h"
#include "tq_host.h"
#include "tq_refit.h"

#define TQ_REFIT_WEIGHT_THREADS 256

// ---- weights: one workgroup per replica -----------------------------------------------------------------------------------
// The workgroup zeroes its row of `weights`, meets at a barrier, and adds 1 at the AOI of each of its N draws.  Integer
// adds commute, so the counts do not depend on the order the hardware takes them in; no other workgroup touches the row.
__global__ __launch_bounds__(TQ_REFIT_WEIGHT_THREADS) void tq_refit_weights_kernel(const tq_refit_weights_args a) {
  const int r = blockIdx.x, t = threadIdx.x;
  const uint32_t N = (uint32_t)a.N;
  int32_t* w = a.weights + tq_refit_weight_at(r, 0, a.N);
  for (uint32_t n = t; n < N; n += TQ_REFIT_WEIGHT_THREADS) w[n] = 0;
  __syncthreads();  // with its fences: the zeroes are in place before any thread of the workgroup adds
  const int s = a.first + r;
  for (uint32_t i = t; i < N; i += TQ_REFIT_WEIGHT_THREADS) atomicAdd(&w[tq_refit_draw(a.seed, s, i, N)], 1);  // index < N
}

extern "C" int tq_refit_weights(const tq_refit_weights_args* a, void* stream) {
  if (!a || !a->weights) {
    tq_set_error("tq_refit_weights: NULL weights");
    return TQ_ERR_ARG;
  }
  if (a->N < 1) {
    tq_set_error("tq_refit_weights: N must be positive");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_replicas_ok("tq_refit_weights", a->R)) return TQ_ERR_ARG;
  if (a->first < 0 || a->first > INT32_MAX - a->R) {
    tq_set_error("tq_refit_weights: first must be non-negative and first + R at most 2^31 - 1");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_refit_weights_kernel, dim3((unsigned)a->R), dim3(TQ_REFIT_WEIGHT_THREADS), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_refit_weights_kernel");
}

// ---- E-step: one wave (= one workgroup) per (row, replica) ----------------------------------------------------------------
// tq_multistart_estep_kernel with one more test before the first shuffle: a pair (replica, AOI) of weight 0 adds nothing
// to the replica's M-step, so its wave leaves whole and writes nothing.  Both tests are uniform over the workgroup.
template <int M>
__global__ __launch_bounds__(64) void tq_refit_estep_kernel(const tq_refit_estep_args a) {
  const int n = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  if (a.active && a.active[r] == 0) return;
  if (a.weights[tq_refit_weight_at(r, n, a.N)] == 0) return;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  double* filt = a.filt + tq_multistart_filt_at<M>(r, n, a.N, F);
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta + tq_multistart_theta_at<M>(r), a.U, a.prior);
  tq_chain_estep_row<M, false>(m, TqHmmEmit<M>{m, pr}, F, lane, filt, nullptr, a.rows + tq_multistart_row_at<M>(r, n, a.N));
}

extern "C" int tq_refit_estep(const tq_refit_estep_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->filt || !a->rows || !a->weights) {
    tq_set_error("tq_refit_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_refit_estep", a->N, a->F) || !tq_chain_states_ok("tq_refit_estep", a->U, a->B) ||
      !tq_chain_replicas_ok("tq_refit_estep", a->R) || !tq_chain_prior_ok("tq_refit_estep", a->prior))
    return TQ_ERR_ARG;
  const dim3 grid((unsigned)a->N, (unsigned)a->R);
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_refit_estep_kernel<MM>), grid, dim3(64), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_refit_estep_kernel");
}

// ---- M-step: one workgroup per replica ------------------------------------------------------------------------------------
// tq_chain_reduce_rows with every row times its weight: thread t sums rows t, t + 256, ..., then the same fixed tree in
// LDS, the integer sum of the weights next to it; thread 0 applies the mask.
template <int M>
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_refit_mstep_kernel(const tq_refit_mstep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M);
  __shared__ double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  __shared__ int64_t wpart[TQ_SMOOTH_MSTEP_THREADS];
  const int r = blockIdx.x, t = threadIdx.x;
  if (a.active && a.active[r] == 0) return;  // the whole workgroup, before its first barrier
  double s[COLS];
  int64_t ws;
  tq_refit_thread_sums<COLS>(a.rows + tq_multistart_row_at<M>(r, 0, a.N), a.weights + tq_refit_weight_at(r, 0, a.N), a.N, t,
                             TQ_SMOOTH_MSTEP_THREADS, s, ws);
#pragma unroll
  for (int j = 0; j < COLS; ++j) part[j][t] = s[j];
  wpart[t] = ws;
  __syncthreads();
  for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int j = 0; j < COLS; ++j) part[j][t] += part[j][t + h];
      wpart[t] += wpart[t + h];
    }
    __syncthreads();
  }
  if (t != 0) return;
  double sums[COLS], theta[M * M + M];
#pragma unroll
  for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
  double* th = a.theta + tq_multistart_theta_at<M>(r);
#pragma unroll
  for (int j = 0; j < M * M + M; ++j) theta[j] = th[j];
  const double ll = tq_refit_mstep_theta<M>(sums, wpart[0], a.allow, theta);
#pragma unroll
  for (int j = 0; j < M * M + M; ++j) th[j] = theta[j];
  a.trace[(int64_t)r * a.T + a.it] = ll;
}

extern "C" int tq_refit_mstep(const tq_refit_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->trace || !a->weights) {
    tq_set_error("tq_refit_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_iteration_ok("tq_refit_mstep", a->N, a->it) ||
      !tq_chain_trace_ok("tq_refit_mstep", a->it, a->T, "the trace of a replica"))
    return TQ_ERR_ARG;
  if (!tq_chain_states_ok("tq_refit_mstep", a->U, a->B) || !tq_chain_replicas_ok("tq_refit_mstep", a->R)) return TQ_ERR_ARG;
  if (!tq_chain_allow_ok("tq_refit_mstep", tq_multistart_allow_ok(a->allow, a->U + a->B)))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_refit_mstep_kernel<MM>), dim3((unsigned)a->R),
                                                  dim3(TQ_SMOOTH_MSTEP_THREADS), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_refit_mstep_kernel");
}
