// Host mirror, on arrays of 64 lanes, of the device-only halves of the hidden-Markov kernels (tapqir_amd/csrc/
// tq_chain_dev.h), shared by hmm_check.cpp, multistart_check.cpp and joint_check.cpp: the wave sum, the E-step of one row
// with the device's ownership of frames and its scan order, and the M-step's strided sums and tree.
#pragma once
#include "../../tapqir_amd/csrc/tq_hmm.h"

namespace {

// the butterfly of tq_group_sum<64>: after the six exchanges every lane holds the sum; lane 0's is returned
double wave_sum(const double* v) {
  double a[64], b[64];
  for (int i = 0; i < 64; ++i) a[i] = v[i];
  for (int d = 1; d < 64; d <<= 1) {
    for (int i = 0; i < 64; ++i) b[i] = a[i] + a[i ^ d];
    for (int i = 0; i < 64; ++i) a[i] = b[i];
  }
  return a[0];
}

// tq_chain_estep_row: one workgroup of an E-step kernel; gam is not read when GAMMA = false
template <int M, bool GAMMA, class Chain, class Emit>
void estep_row(const Chain& m, const Emit& em, int F, double* filt, double* gam, double* row) {
  constexpr int COLS = TQ_HMM_COLS(M);
  static TqHmmMat<M> pre[64], suf[64], old[64];
  int lo[64], hi[64];
  for (int k = 0; k < 64; ++k) {
    tq_smooth_lane_range(k, F, lo[k], hi[k]);
    pre[k] = suf[k] = tq_chain_chunk<M>(m, em, lo[k], hi[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {  // the kernel's Hillis-Steele steps: all lanes read, then all lanes write
    for (int k = 0; k < 64; ++k) old[k] = pre[k];
    for (int k = d; k < 64; ++k) pre[k] = tq_hmm_mul(old[k - d], old[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {
    for (int k = 0; k < 64; ++k) old[k] = suf[k];
    for (int k = 0; k + d < 64; ++k) suf[k] = tq_hmm_mul(old[k], old[k + d]);
  }
  static double acc[COLS][64];
  for (int k = 0; k < 64; ++k) {
    const TqHmmMat<M> e = k == 0 ? tq_hmm_identity<M>() : pre[k - 1];
    const TqHmmMat<M> s = k == 63 ? tq_hmm_identity<M>() : suf[k + 1];
    double v[M], b[M], a[COLS];
    tq_hmm_prefix_vector(e, v);
    tq_hmm_suffix_vector(s, b);
    tq_chain_sweeps<M, GAMMA>(m, em, lo[k], hi[k], v, b, filt, gam, a);
    for (int j = 0; j < COLS; ++j) acc[j][k] = a[j];
  }
  for (int j = 0; j < COLS; ++j) row[j] = wave_sum(acc[j]);
}

// tq_chain_reduce_rows: thread t sums rows t, t + 256, ...; the tree halves 256 partial sums
template <int COLS>
void reduce_rows(const double* rows, int N, double* sums) {
  static double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  for (int t = 0; t < TQ_SMOOTH_MSTEP_THREADS; ++t)
    for (int j = 0; j < COLS; ++j) {
      double s = 0.0;
      for (int n = t; n < N; n += TQ_SMOOTH_MSTEP_THREADS) s += rows[(int64_t)n * COLS + j];
      part[j][t] = s;
    }
  for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1)
    for (int t = 0; t < h; ++t)
      for (int j = 0; j < COLS; ++j) part[j][t] += part[j][t + h];
  for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
}

}  // namespace

#define HK_SWITCH_M(M, ...)   \
  switch (M) {                \
    case 2: {                 \
      constexpr int MM = 2;   \
      __VA_ARGS__;            \
    } break;                  \
    case 3: {                 \
      constexpr int MM = 3;   \
      __VA_ARGS__;            \
    } break;                  \
    case 4: {                 \
      constexpr int MM = 4;   \
      __VA_ARGS__;            \
    } break;                  \
    default:                  \
      break;                  \
  }
