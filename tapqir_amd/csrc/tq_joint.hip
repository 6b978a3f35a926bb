// tq_joint.hip -- two colour channels as one hidden Markov chain of four states on the device (`smooth --joint`, DESIGN.md
// section 27; bodies in tq_joint.h over tq_hmm.h): the E-step on a grid (N, R) with the geometry of tq_multistart_estep and
// an emission that reads both channels, the M-step on a grid of R workgroups that puts one of five structures on every
// replica's A, and the Viterbi path in joint states.  The backward sampler and the estimate of A are tq_hmm.hip's, run on
// the joint filt with (U, B) = (2, 2); tq_pair_dwell walks that sampler's rows, as it draws them, into the runs of one
// channel with the other channel's state at their ends (section 32).  No atomics but the integer histogram bins of
// tq_pair_dwell, no workgroup waits on another, every loop bounded by F, N or R.
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
  if (!tq_chain_iteration_ok("tq_joint_mstep", a->N, a->it) ||
      !tq_chain_trace_ok("tq_joint_mstep", a->it, a->T, "the trace of a replica"))
    return TQ_ERR_ARG;
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

// ---- backward sampler walked into one channel's intervals ----------------------------------------------------------------
// Row (s, n) is the raster tq_hmm_count_kernel<4> draws at (U, B) = (2, 2), state for state: the walk of
// tq_chain_sample_row, the twelve thresholds of 64 frames staged in LDS (6144 B, written as they come), TqHmmDraws against
// qbuf[j].  Here the class z = (state >> which) & 1 is walked into runs (tq_pair_dwell_frame) and every run carries the
// partner's state at its ends; neither a raster nor the state pairs are stored.  EMIT = false: per-row interval counts, the
// first-binding frame, the partner's first bound frame from there on, and the interior-run histograms by the partner's state
// at the run's start; EMIT = true: the same draws again, the k-th run a row closes written at tq_smooth_emit_slot with its
// partner code beside it (tq_chain_sink_put with PARTNER).
template <bool EMIT>
__global__ __launch_bounds__(64) void tq_pair_dwell_kernel(const tq_pair_dwell_args a) {
  constexpr int M = TQ_JOINT_M, T = M * (M - 1);
  __shared__ double qbuf[64][T];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F, which = a.which;
  const double* fr = a.filt + (int64_t)n * F * M;
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta, 2, 0.5);  // the priors are already in filt
  int32_t* hb = EMIT || !active ? nullptr : a.hist_bound + tq_pair_hist_at(s, 0, F);
  int32_t* hu = EMIT || !active ? nullptr : a.hist_unbound + tq_pair_hist_at(s, 0, F);
  const int64_t total = a.total;
  int64_t o = 0;
  int count = 0;
  if (EMIT && active) {
    o = a.offsets[(int64_t)s * a.N + n];
    count = a.counts[(int64_t)s * a.N + n];
  }
  int closed = 0;  // runs closed so far
  auto sink = [&](const TqDwellInterval& v, int pc) {  // the histograms by the partner's state at the run's start
    tq_chain_sink_put<EMIT, true>(v, closed, o, count, total, a.intervals, hb, hu, s, n, (pc & 1) * F, a.partner, pc);
  };

  TqHmmDraws draws;
  tq_hmm_draws_begin(draws, a.seed, s, n);
  TqPairDwellRow r;
  tq_pair_dwell_begin(r, F);
  TqDwellInterval iv;
  int code = 0;
  tq_chain_sample_row(
      F, lane, active,
      [&](int f, int l, bool last) { tq_chain_stage_thresholds<M, true>(m, fr + (int64_t)f * M, last, qbuf[l]); },
      [&](int f, int j) {
        if (tq_pair_dwell_frame(r, tq_hmm_draws_next(draws, F - 1 - f), qbuf[j], f, F, which, iv, code)) sink(iv, code);
      });
  if (!active) return;
  tq_pair_dwell_finish(r, iv, code);
  sink(iv, code);
  if (!EMIT) {
    const int64_t row = (int64_t)s * a.N + n;
    a.counts[row] = closed;
    if (a.tau) a.tau[row] = (float)r.c.tau;
    if (a.tau_after) a.tau_after[row] = (float)r.tau_after;
  }
}

extern "C" int tq_pair_dwell(const tq_pair_dwell_args* a, void* stream) {
  if (!a || !a->filt || !a->theta || !a->counts) {
    tq_set_error("tq_pair_dwell: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (!tq_chain_dwell_mode_ok("tq_pair_dwell", a->mode, a->hist_bound && a->hist_unbound,
                              a->offsets && (a->total <= 0 || (a->intervals && a->partner))) ||
      !tq_chain_dwell_sampler_ok("tq_pair_dwell", a->N, a->F, a->S, a->total))
    return TQ_ERR_ARG;
  if (a->which != 0 && a->which != 1) {
    tq_set_error("tq_pair_dwell: which must be 0 (channel a) or 1 (channel b)");
    return TQ_ERR_ARG;
  }
  dim3 grid;
  if (!tq_chain_sample_grid("tq_pair_dwell", a->N, a->S, &grid)) return TQ_ERR_ARG;
  if (a->mode == TQ_DWELL_COUNT) {
    hipLaunchKernelGGL((tq_pair_dwell_kernel<false>), grid, dim3(64), 0, (hipStream_t)stream, *a);
  } else {
    if (a->total == 0) return TQ_OK;
    hipLaunchKernelGGL((tq_pair_dwell_kernel<true>), grid, dim3(64), 0, (hipStream_t)stream, *a);
  }
  return tq_launch_status("tq_pair_dwell_kernel");
}
