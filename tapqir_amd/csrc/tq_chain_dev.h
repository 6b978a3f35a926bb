// tq_chain_dev.h -- device-only halves of the hidden-Markov kernels over MxM products, shared by tq_hmm.hip,
// tq_multistart.hip, tq_joint.hip, tq_refit.hip and tq_timed.hip (bodies in tq_hmm.h): the wave shuffles of a product, the
// two exclusive scans, the E-step of one row by one wave -- whatever the chain: it reaches the bodies as `m`, with what it
// overloads of tq_chain_step and tq_chain_pair -- and the M-step's sum of rows.  Only .hip units include it: no header
// that the g++ host build reads may, and tests/hostcheck/chain_host.h is its mirror on arrays.
#pragma once
#include <hip/hip_runtime.h>

#include "tq_dpp.h"
#include "tq_hmm.h"

template <int M>
__device__ __forceinline__ TqHmmMat<M> tq_chain_shfl_up(const TqHmmMat<M>& x, int d) {
  TqHmmMat<M> r;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) r.m[i][j] = __shfl_up(x.m[i][j], d, 64);
  return r;
}
template <int M>
__device__ __forceinline__ TqHmmMat<M> tq_chain_shfl_down(const TqHmmMat<M>& x, int d) {
  TqHmmMat<M> r;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) r.m[i][j] = __shfl_down(x.m[i][j], d, 64);
  return r;
}

// The scans of tq_smooth_estep_kernel over a lane's chunk product c, one after the other so that only one running product
// is live at a time: the prefix scan multiplies the lower lanes' product from the left and leaves v = a_{lo-1}, the suffix
// scan the higher lanes' from the right and leaves b = beta_{hi-1} (Hillis-Steele, six steps each, one more shuffle makes
// them exclusive).  Every lane takes part in every shuffle.
template <int M>
__device__ __forceinline__ void tq_chain_prefix_scan(const TqHmmMat<M>& c, int lane, double* v) {
  TqHmmMat<M> pre = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const TqHmmMat<M> left = tq_chain_shfl_up(pre, d);
    if (lane >= d) pre = tq_hmm_mul(left, pre);
  }
  pre = tq_chain_shfl_up(pre, 1);
  if (lane == 0) pre = tq_hmm_identity<M>();
  tq_hmm_prefix_vector(pre, v);
}
template <int M>
__device__ __forceinline__ void tq_chain_suffix_scan(const TqHmmMat<M>& c, int lane, double* b) {
  TqHmmMat<M> suf = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const TqHmmMat<M> right = tq_chain_shfl_down(suf, d);
    if (lane + d < 64) suf = tq_hmm_mul(suf, right);
  }
  suf = tq_chain_shfl_down(suf, 1);
  if (lane == 63) suf = tq_hmm_identity<M>();
  tq_hmm_suffix_vector(suf, b);
}

// E-step of one row by one wave, L = ceil(F / 64) consecutive frames per lane: the chunk product, the two scans, the two
// sweeps into filt (and gam, GAMMA = true), TQ_HMM_COLS(M) wave sums, and lane 0's write of `out`.  The whole wave must
// arrive: a kernel leaves, if it leaves, before the call.
template <int M, bool GAMMA, class Chain, class Emit>
__device__ __forceinline__ void tq_chain_estep_row(const Chain& m, const Emit& em, int F, int lane, double* filt, double* gam,
                                                   double* out) {
  constexpr int COLS = TQ_HMM_COLS(M);
  int lo, hi;
  tq_smooth_lane_range(lane, F, lo, hi);

  const TqHmmMat<M> c = tq_chain_chunk<M>(m, em, lo, hi);
  double v[M], b[M];
  tq_chain_prefix_scan(c, lane, v);
  tq_chain_suffix_scan(c, lane, b);

  double acc[COLS];
  tq_chain_sweeps<M, GAMMA>(m, em, lo, hi, v, b, filt, gam, acc);
#pragma unroll
  for (int j = 0; j < COLS; ++j) acc[j] = tq_group_sum<64>(acc[j]);  // every lane is back here
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < COLS; ++j) out[j] = acc[j];
  }
}

// M-step's sum of N rows of COLS doubles by one workgroup of TQ_SMOOTH_MSTEP_THREADS: thread t sums rows t, t + 256, ...,
// then a fixed tree in `part`, the kernel's LDS.  Returns true in thread 0, which alone gets the totals in `sums`; the
// order of the additions depends on N only, so every kernel that calls this gets the same bits from the same rows.
template <int COLS>
__device__ __forceinline__ bool tq_chain_reduce_rows(const double* rows, int N, double (&part)[COLS][TQ_SMOOTH_MSTEP_THREADS],
                                                     double* sums) {
  const int t = threadIdx.x;
  double s[COLS];
#pragma unroll
  for (int j = 0; j < COLS; ++j) s[j] = 0.0;
  for (int n = t; n < N; n += TQ_SMOOTH_MSTEP_THREADS) {
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
  if (t != 0) return false;
#pragma unroll
  for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
  return true;
}
