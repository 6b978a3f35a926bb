// tq_chain_dev.h -- device-only halves of the hidden-Markov kernels over MxM products, shared by tq_hmm.hip,
// tq_multistart.hip, tq_joint.hip, tq_mixture.hip, tq_refit.hip and tq_timed.hip (bodies in tq_hmm.h): the wave shuffles of
// a product, the two exclusive scans, the E-step of one row by one wave -- whatever the chain: it reaches the bodies as
// `m`, with what it overloads of tq_chain_step and tq_chain_pair -- the M-step's sum of rows, and the backward sampler's
// walk with its staging of thresholds and its interval sink.  Only .hip units include it: no header
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

// ---- backward sampler ----------------------------------------------------------------------------
// The walk of one wave (= one workgroup) over F frames, one lane per sample, in blocks of 64 frames from the highest:
// stage(f, lane, last) once per frame f = f0 + lane of the block, by the lane of that number (last: f == F - 1), a
// barrier, visit(f, j) for every frame f = f0 + j of the block, highest first, in the active lanes, and a second barrier
// before the staging is written again.  Every lane of the workgroup must arrive and reaches every barrier; an inactive lane
// (a sample beyond S) runs nothing but `stage`, so it may touch no memory but the staging.  Every loop is bounded by F.
template <class Stage, class Visit>
__device__ __forceinline__ void tq_chain_sample_row(int F, int lane, bool active, const Stage& stage, const Visit& visit) {
  for (int f0 = (F - 1) & ~63; f0 >= 0; f0 -= 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) stage(f0 + lane, lane, f0 + lane == F - 1);
    __syncthreads();
    if (active) {
      for (int j = cnt - 1; j >= 0; --j) visit(f0 + j, j);
    }
    __syncthreads();
  }
}

// The M (M - 1) thresholds of one frame, from its a_f at `af`, into the LDS row q.  DIRECT writes the quotients to LDS as
// they come, so that they do not wait in registers; otherwise they go through a local array.  Which is cheaper depends on
// the kernel around it (section 35 has the register counts), so the kernel says.
template <int M, bool DIRECT>
__device__ __forceinline__ void tq_chain_stage_thresholds(const TqHmmModel<M>& m, const double* af, bool last, double* q) {
  constexpr int T = M * (M - 1);
  double a[M];
#pragma unroll
  for (int i = 0; i < M; ++i) a[i] = af[i];
  if constexpr (DIRECT) {
    tq_hmm_thresholds(m, a, last, q);
  } else {
    double t[T];
    tq_hmm_thresholds(m, a, last, t);
#pragma unroll
    for (int k = 0; k < T; ++k) q[k] = t[k];
  }
}

// Where the runs of row (s, n) go as the walk closes them: one text for every dwell kernel.  The bookkeeping (hb, hu, o,
// count, closed) stays in the kernel's own locals, set up in the kernel's own text, and the kernel wraps this in a
// one-line lambda: gathered in a struct, or filled through references by a shared helper, it cost the COUNT kernels a
// wave per SIMD (section 35).
// EMIT = false: an interior run adds 1 to bin `length` of the row's bound or unbound histogram (integer atomics:
// order-free, so deterministic; an interior run is shorter than F), `off` bins further on where a kernel keeps several
// histograms per sample.  EMIT = true: the k-th run the row closes is written at tq_smooth_emit_slot, with the partner
// code `pc` beside it where PARTNER.  `closed` counts both.
template <bool EMIT, bool PARTNER = false>
__device__ __forceinline__ void tq_chain_sink_put(const TqDwellInterval& v, int& closed, int64_t o, int count, int64_t total,
                                                  int32_t* intervals, int32_t* hb, int32_t* hu, int s, int n, int off = 0,
                                                  uint8_t* partner = nullptr, int pc = 0) {
  if constexpr (EMIT) {
    const int64_t pos = tq_smooth_emit_slot(o, count, closed, total);
    if (pos >= 0) {
      tq_smooth_emit_row(intervals, total, pos, s, n, v);
      if constexpr (PARTNER) partner[pos] = (uint8_t)pc;
    }
  } else {
    if (v.low_or_high == 0 || v.low_or_high == 1) atomicAdd((v.z ? hb : hu) + off + (v.stop + 1 - v.start), 1);
  }
  ++closed;
}
