// tq_multistart.hip -- R EM fits of the chain of tq_hmm.h side by side on the device (`smooth --restarts`, DESIGN.md
// section 26; bodies in tq_multistart.h and tq_hmm.h): the E-step on a grid (N, R) that stores only the summed rows of
// every replica, and the M-step on a grid of R workgroups under a topology mask.  A replica marked inactive costs a
// workgroup that returns at once.  No atomics, no workgroup waits on another, every loop bounded by F, N or R.
#include <hip/hip_runtime.h>

#include "tq_dpp.h"
#include "tq_host.h"
#include "tq_multistart.h"

// runs `...` with the compile-time constant MM = M, which tq_multistart_states has checked to be 2, 3 or 4
#define TQ_MULTISTART_SWITCH_M(M, ...) \
  switch (M) {                         \
    case 2: {                          \
      constexpr int MM = 2;            \
      __VA_ARGS__;                     \
    } break;                           \
    case 3: {                          \
      constexpr int MM = 3;            \
      __VA_ARGS__;                     \
    } break;                           \
    default: {                         \
      constexpr int MM = 4;            \
      __VA_ARGS__;                     \
    } break;                           \
  }

static bool tq_multistart_states(const char* who, int U, int B, int R) {
  char buf[160];
  if (U < 1 || B < 1 || U + B > TQ_HMM_MAX_STATES) {
    snprintf(buf, sizeof(buf), "%s: U and B must be at least 1 and U + B at most %d", who, TQ_HMM_MAX_STATES);
    tq_set_error(buf);
    return false;
  }
  if (R < 1 || R > TQ_MULTISTART_MAX) {
    snprintf(buf, sizeof(buf), "%s: R must be at least 1 and at most %d", who, TQ_MULTISTART_MAX);
    tq_set_error(buf);
    return false;
  }
  return true;
}

// ---- E-step: one wave (= one workgroup) per (row, replica), L = ceil(F / 64) consecutive frames per lane ----------------
// the shuffles of tq_hmm.hip (device only)
template <int M>
__device__ __forceinline__ TqHmmMat<M> tq_multistart_shfl_up(const TqHmmMat<M>& x, int d) {
  TqHmmMat<M> r;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) r.m[i][j] = __shfl_up(x.m[i][j], d, 64);
  return r;
}
template <int M>
__device__ __forceinline__ TqHmmMat<M> tq_multistart_shfl_down(const TqHmmMat<M>& x, int d) {
  TqHmmMat<M> r;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) r.m[i][j] = __shfl_down(x.m[i][j], d, 64);
  return r;
}

// The geometry, the scans and the sweeps of tq_hmm_estep_kernel with blockIdx.y = the replica: its theta, its slice of the
// scratch for a_f and its slice of rows; p is shared.  The test of `active` is uniform over the workgroup and comes before
// the first shuffle, so an inactive replica's waves leave whole and write nothing.
template <int M>
__global__ __launch_bounds__(64) void tq_multistart_estep_kernel(const tq_multistart_estep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M);
  const int n = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  if (a.active && a.active[r] == 0) return;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  double* filt = a.filt + tq_multistart_filt_at<M>(r, n, a.N, F);
  const TqHmmModel<M> m = tq_hmm_model<M>(a.theta + tq_multistart_theta_at<M>(r), a.U, a.prior);
  int lo, hi;
  tq_smooth_lane_range(lane, F, lo, hi);

  const TqHmmMat<M> c = tq_hmm_chunk(m, pr, lo, hi);
  double v[M], b[M];
  {
    TqHmmMat<M> pre = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const TqHmmMat<M> left = tq_multistart_shfl_up(pre, d);
      if (lane >= d) pre = tq_hmm_mul(left, pre);
    }
    pre = tq_multistart_shfl_up(pre, 1);
    if (lane == 0) pre = tq_hmm_identity<M>();
    tq_hmm_prefix_vector(pre, v);
  }
  {
    TqHmmMat<M> suf = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const TqHmmMat<M> right = tq_multistart_shfl_down(suf, d);
      if (lane + d < 64) suf = tq_hmm_mul(suf, right);
    }
    suf = tq_multistart_shfl_down(suf, 1);
    if (lane == 63) suf = tq_hmm_identity<M>();
    tq_hmm_suffix_vector(suf, b);
  }

  double acc[COLS];
  tq_multistart_sweeps(m, pr, lo, hi, v, b, filt, acc);
#pragma unroll
  for (int j = 0; j < COLS; ++j) acc[j] = tq_group_sum<64>(acc[j]);  // every lane is back here
  if (lane == 0) {
    double* out = a.rows + tq_multistart_row_at<M>(r, n, a.N);
#pragma unroll
    for (int j = 0; j < COLS; ++j) out[j] = acc[j];
  }
}

extern "C" int tq_multistart_estep(const tq_multistart_estep_args* a, void* stream) {
  if (!a || !a->p || !a->theta || !a->filt || !a->rows) {
    tq_set_error("tq_multistart_estep: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->F < 1 || a->F > TQ_SMOOTH_MAX_F) {
    tq_set_error("tq_multistart_estep: N and F must be positive and F at most 65536");
    return TQ_ERR_ARG;
  }
  if (!tq_multistart_states("tq_multistart_estep", a->U, a->B, a->R)) return TQ_ERR_ARG;
  if (!(a->prior > 0.0 && a->prior < 1.0)) {
    tq_set_error("tq_multistart_estep: prior must lie in (0, 1)");
    return TQ_ERR_ARG;
  }
  const dim3 grid((unsigned)a->N, (unsigned)a->R);
  TQ_MULTISTART_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_multistart_estep_kernel<MM>), grid, dim3(64), 0,
                                                         (hipStream_t)stream, *a));
  return tq_launch_status("tq_multistart_estep_kernel");
}

// ---- M-step: one workgroup per replica; thread t sums rows t, t + 256, ..., then a fixed tree in LDS --------------------
template <int M>
__global__ __launch_bounds__(TQ_SMOOTH_MSTEP_THREADS) void tq_multistart_mstep_kernel(const tq_multistart_mstep_args a) {
  constexpr int COLS = TQ_HMM_COLS(M);
  __shared__ double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  const int t = threadIdx.x, r = blockIdx.x;
  if (a.active && a.active[r] == 0) return;  // the whole workgroup, before its first barrier
  const double* rows = a.rows + tq_multistart_row_at<M>(r, 0, a.N);
  double s[COLS];
#pragma unroll
  for (int j = 0; j < COLS; ++j) s[j] = 0.0;
  for (int n = t; n < a.N; n += TQ_SMOOTH_MSTEP_THREADS) {
    const double* row = rows + (int64_t)n * COLS;
#pragma unroll
    for (int j = 0; j < COLS; ++j) s[j] += row[j];
  }
#pragma unroll
  for (int j = 0; j < COLS; ++j) part[j][t] = s[j];
  __syncthreads();
  for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int j = 0; j < COLS; ++j) part[j][t] += part[j][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    double sums[COLS], theta[M * M + M];
    double* th = a.theta + tq_multistart_theta_at<M>(r);
#pragma unroll
    for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
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
  if (a->N < 1 || a->it < 0) {
    tq_set_error("tq_multistart_mstep: N must be positive and it non-negative");
    return TQ_ERR_ARG;
  }
  if (a->T <= a->it) {
    tq_set_error("tq_multistart_mstep: T must exceed it (the trace of a replica has T entries)");
    return TQ_ERR_ARG;
  }
  if (!tq_multistart_states("tq_multistart_mstep", a->U, a->B, a->R)) return TQ_ERR_ARG;
  if (!tq_multistart_allow_ok(a->allow, a->U + a->B)) {
    tq_set_error("tq_multistart_mstep: allow must have no bit beyond M * M and a free entry in every row");
    return TQ_ERR_ARG;
  }
  TQ_MULTISTART_SWITCH_M(a->U + a->B, hipLaunchKernelGGL((tq_multistart_mstep_kernel<MM>), dim3((unsigned)a->R),
                                                         dim3(TQ_SMOOTH_MSTEP_THREADS), 0, (hipStream_t)stream, *a));
  return tq_launch_status("tq_multistart_mstep_kernel");
}
