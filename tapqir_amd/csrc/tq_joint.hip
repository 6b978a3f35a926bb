// tq_joint.hip -- two colour channels as one hidden Markov chain of four states on the device (`smooth --joint`, DESIGN.md
// section 27; bodies in tq_joint.h over tq_hmm.h): the E-step on a grid (N, R) with the geometry of tq_multistart_estep and
// an emission that reads both channels, the M-step on a grid of R workgroups that puts one of five structures on every
// replica's A, and the Viterbi path in joint states.  The backward sampler and the estimate of A are tq_hmm.hip's, run on
// the joint filt with (U, B) = (2, 2).  No atomics, no workgroup waits on another, every loop bounded by F, N or R.
#include <hip/hip_runtime.h>

#include "tq_chain_dev.h"
#include "tq_host.h"
#include "tq_joint.h"

// ---- E-step: one wave (= one workgroup) per (row, replica) ----------------------------------------------------------------
// tq_chain_estep_row at M = 4 with the addressing of tq_multistart_estep_kernel<4> and the joint emission.  The test of
// `active` is uniform over the workgroup and comes before the first shuffle, so an inactive replica's waves leave whole and
// write nothing.  GAMMA = false stores no gamma and never forms its address.
template <bool GAMMA>
__global__ __launch_bounds__(64) void tq_joint_estep_kernel(const tq_joint_estep_args a) {
  constexpr int M = TQ_JOINT_M;
  const int n = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  if (a.active && a.active[r] == 0) return;
  const int F = a.F;
  const float* pa = a.p_a + (int64_t)n * F;
  const float* pb = a.p_b + (int64_t)n * F;
  double* filt = a.filt + tq_multistart_filt_at<M>(r, n, a.N, F);
  double* gam = GAMMA ? a.gamma + tq_multistart_filt_at<M>(r, n, a.N, F) : nullptr;
  const TqJointModel m = tq_joint_model(a.theta + tq_multistart_theta_at<M>(r), a.prior_a, a.prior_b);
  tq_chain_estep_row<M, GAMMA>(m, TqJointEmit{m, pa, pb}, F, lane, filt, gam, a.rows + tq_multistart_row_at<M>(r, n, a.N));
}

extern "C" int tq_joint_estep(const tq_joint_estep_args* a, void* stream) {
  if (!a || !a->p_a || !a->p_b || !a->theta || !a->filt || !a->rows) {
    tq_set_error("tq_joint_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_joint_estep", a->N, a->F) || !tq_chain_replicas_ok("tq_joint_estep", a->R) ||
      !tq_chain_priors_ok("tq_joint_estep", a->prior_a, a->prior_b))
    return TQ_ERR_ARG;
  const dim3 grid((unsigned)a->N, (unsigned)a->R);
  if (a->gamma) {
    hipLaunchKernelGGL((tq_joint_estep_kernel<true>), grid, dim3(64), 0, (hipStream_t)stream, *a);
  } else {
    hipLaunchKernelGGL((tq_joint_estep_kernel<false>), grid, dim3(64), 0, (hipStream_t)stream, *a);
  }
  return tq_launch_status("tq_joint_estep_kernel");
}

// ---- M-step: one workgroup per replica; tq_chain_reduce_rows, then thread 0 applies the structure -------------------------
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_joint_mstep_kernel(const tq_joint_mstep_args a) {
  constexpr int M = TQ_JOINT_M, COLS = TQ_JOINT_COLS;
  __shared__ double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  const int r = blockIdx.x;
  if (a.active && a.active[r] == 0) return;  // the whole workgroup, before its first barrier
  double sums[COLS];
  if (tq_chain_reduce_rows<COLS>(a.rows + tq_multistart_row_at<M>(r, 0, a.N), a.N, part, sums)) {
    double theta[TQ_JOINT_THETA];
    double* th = a.theta + tq_multistart_theta_at<M>(r);
#pragma unroll
    for (int j = 0; j < TQ_JOINT_THETA; ++j) theta[j] = th[j];
    tq_joint_mstep_theta(sums, a.N, a.structure[r], theta);
#pragma unroll
    for (int j = 0; j < TQ_JOINT_THETA; ++j) th[j] = theta[j];
    a.trace[(int64_t)r * a.T + a.it] = sums[COLS - 1];
  }
}

extern "C" int tq_joint_mstep(const tq_joint_mstep_args* a, void* stream) {
  if (!a || !a->rows || !a->theta || !a->trace) {
    tq_set_error("tq_joint_mstep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->it < 0) {
    tq_set_error("tq_joint_mstep: N must be positive and it non-negative");
    return TQ_ERR_ARG;
  }
  if (a->T <= a->it) {
    tq_set_error("tq_joint_mstep: T must exceed it (the trace of a replica has T entries)");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_replicas_ok("tq_joint_mstep", a->R)) return TQ_ERR_ARG;
  for (int r = 0; r < a->R; ++r)
    if (!tq_joint_structure_ok(a->structure[r])) {
      tq_set_error("tq_joint_mstep: structure must be one of TQ_JOINT_INDEPENDENT .. TQ_JOINT_FULL (0 .. 4) for every replica");
      return TQ_ERR_ARG;
    }
  hipLaunchKernelGGL(tq_joint_mstep_kernel, dim3((unsigned)a->R), dim3(TQ_SMOOTH_MSTEP_THREADS), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_joint_mstep_kernel");
}

// ---- Viterbi: one lane per row, sequential in f; the back-pointer words of a wave's rows are adjacent -------------------
__global__ __launch_bounds__(64) void tq_joint_viterbi_kernel(const tq_joint_viterbi_args a) {
  const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (n >= a.N) return;
  const TqJointModel m = tq_joint_model(a.theta, a.prior_a, a.prior_b);
  tq_joint_viterbi_row(m, a.p_a + n * a.F, a.p_b + n * a.F, a.F, a.back + n, a.N, a.path + n * a.F);
}

extern "C" int tq_joint_viterbi(const tq_joint_viterbi_args* a, void* stream) {
  if (!a || !a->p_a || !a->p_b || !a->theta || !a->back || !a->path) {
    tq_set_error("tq_joint_viterbi: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_frames_ok("tq_joint_viterbi", a->N, a->F) || !tq_chain_priors_ok("tq_joint_viterbi", a->prior_a, a->prior_b))
    return TQ_ERR_ARG;
  hipLaunchKernelGGL(tq_joint_viterbi_kernel, dim3((unsigned)((a->N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_joint_viterbi_kernel");
}
