// tq_multistart.hip -- R EM fits of the chain of tq_hmm.h side by side on the device (`smooth --restarts`, DESIGN.md
// section 26; bodies in tq_multistart.h and tq_hmm.h): the E-step on a grid (N, R) that stores only the summed rows of
// every replica, and the M-step on a grid of R workgroups under a topology mask.  A replica marked inactive costs a
// workgroup that returns at once.  No atomics, no workgroup waits on another, every loop bounded by F, N or R.
#include <hip/hip_runtime.h>

#include "tq_chain_dev.h"
#include "tq_host.h"
#include "tq_multistart.h"

// ---- E-step: one wave (= one workgroup) per (row, replica) ----------------------------------------------------------------
// tq_chain_estep_row, as tq_hmm_estep_kernel calls it, with blockIdx.y = the replica: its theta, its slice of the scratch
// for a_f and its slice of rows; p is shared and no gamma is stored.  The test of `active` is uniform over the workgroup
// and comes before the first shuffle, so an inactive replica's waves leave whole and write nothing.
template <int M>
__global__ __launch_bounds__(64) void tq_multistart_estep_kernel(const tq_multistart_estep_args a) {
  const int n = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  if (a.active && a.active[r] == 0) return;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  double* filt = a.filt + tq_multistart_filt_at<M>(r, n, a.N, F);
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta + tq_multistart_theta_at<M>(r), a.U, a.prior);
  tq_chain_estep_row<M, false>(m, TqHmmEmit<M>{m, pr}, F, lane, filt, nullptr, a.rows + tq_multistart_row_at<M>(r, n, a.N));
}

extern "C" int tq_multistart_estep(const tq_multistart_estep_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->filt || !a->rows) {
    tq_set_error("tq_multistart_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_multistart_estep", a->N, a->F) || !tq_chain_states_ok("tq_multistart_estep", a->U, a->B) ||
      !tq_chain_replicas_ok("tq_multistart_estep", a->R) || !tq_chain_prior_ok("tq_multistart_estep", a->prior))
    return TQ_ERR_ARG;
  const dim3 grid((unsigned)a->N, (unsigned)a->R);
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_multistart_estep_kernel<MM>), grid, dim3(64), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_multistart_estep_kernel");
}

// ---- M-step: one workgroup per replica; tq_chain_reduce_rows, then thread 0 applies the mask ------------------------------
template <int M>
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_multistart_mstep_kernel(const tq_multistart_mstep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M);
  __shared__ double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  const int r = blockIdx.x;
  if (a.active && a.active[r] == 0) return;  // the whole workgroup, before its first barrier
  double sums[COLS];
  if (tq_chain_reduce_rows<COLS>(a.rows + tq_multistart_row_at<M>(r, 0, a.N), a.N, part, sums)) {
    double theta[M * M + M];
    double* th = a.theta + tq_multistart_theta_at<M>(r);
#pragma unroll
    for (int j = 0; j < M * M + M; ++j) theta[j] = th[j];
    tq_multistart_mstep_theta<M>(sums, a.N, a.allow, theta);
#pragma unroll
    for (int j = 0; j < M * M + M; ++j) th[j] = theta[j];
    a.trace[(int64_t)r * a.T + a.it] = sums[COLS - 1];
  }
}

extern "C" int tq_multistart_mstep(const tq_multistart_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->trace) {
    tq_set_error("tq_multistart_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_iteration_ok("tq_multistart_mstep", a->N, a->it) ||
      !tq_chain_trace_ok("tq_multistart_mstep", a->it, a->T, "the trace of a replica"))
    return TQ_ERR_ARG;
  if (!tq_chain_states_ok("tq_multistart_mstep", a->U, a->B) || !tq_chain_replicas_ok("tq_multistart_mstep", a->R))
    return TQ_ERR_ARG;
  if (!tq_chain_allow_ok("tq_multistart_mstep", tq_multistart_allow_ok(a->allow, a->U + a->B)))
    return TQ_ERR_ARG;
  TQ_HMM_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_multistart_mstep_kernel<MM>), dim3((unsigned)a->R),
                                                  dim3(TQ_SMOOTH_MSTEP_THREADS), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_multistart_mstep_kernel");
}
