// tq_multistart.h -- R replicas of the chain of tq_hmm.h fitted side by side (`smooth --restarts`),
// host+device inline bodies, templated on the number of states M = U + B in {2, 3, 4}:
//   * where replica r keeps its theta, its rows and its scratch of a_f;
//   * the topology mask `allow` (bit i * M + j set: A_ij is free), its check, and the M-step under it.
// Everything else -- the chain, the emission, the chunk products, the sweeps (tq_chain_sweeps with no gamma stored), the
// floor -- is tq_hmm.h's, so that a replica computes what tq_hmm_estep and tq_hmm_mstep compute from the same theta.  The __global__ wrappers are in tq_multistart.hip; the
// test suite runs the same bodies from a g++ build.
#pragma once
#include "tq_hmm.h"

// ---- layout -----------------------------------------------------------------------------------------------------------
template <int M>
TQ_HD int64_t tq_multistart_theta_at(int r) {
  return (int64_t)r * (M * M + M);
}
template <int M>
TQ_HD int64_t tq_multistart_row_at(int r, int n, int N) {
  return ((int64_t)r * N + n) * TQ_HMM_COLS(M);
}
template <int M>
TQ_HD int64_t tq_multistart_filt_at(int r, int n, int N, int F) {
  return ((int64_t)r * N + n) * F * M;
}

// ---- E-step: a lane's two sweeps, tq_chain_sweeps for the class chain with no gamma stored -------------------------------
template <int M>
TQ_HD void tq_multistart_sweeps(const TqHmmModel<M>& m, const float* pr, int lo, int hi, const double* v, const double* b,
                                double* filt, double* acc) {
  tq_chain_sweeps<M, false>(m, TqHmmEmit<M>{m, pr}, lo, hi, v, b, filt, nullptr, acc);
}

// ---- topology -----------------------------------------------------------------------------------------------------------
// every bit below M * M, and at least one free entry in every row
TQ_HD bool tq_multistart_allow_ok(uint32_t allow, int M) {
  if ((allow >> (M * M)) != 0u) return false;  // M * M <= 16
  for (int i = 0; i < M; ++i)
    if (((allow >> (i * M)) & ((1u << M) - 1u)) == 0u) return false;
  return true;
}

// The M-step under `allow`: the summed E n_ij of a forbidden pair is set to 0 before the quotient, so the entry comes out
// of the floor of tq_hmm_mstep_theta at TQ_SMOOTH_RMIN over the row's sum -- pinned at 1e-9, which tq_hmm_model gives every
// reader again, not an exact zero.  A row whose free pairs have no expected occupancy keeps its old values.
template <int M>
TQ_HD void tq_multistart_mstep_theta(const double* sums, int N, uint32_t allow, double* theta) {
  constexpr int COLS = TQ_HMM_COLS(M);
  double s[COLS];
#pragma unroll
  for (int j = 0; j < COLS; ++j) s[j] = (j < M * M && ((allow >> j) & 1u) == 0u) ? 0.0 : sums[j];
  tq_hmm_mstep_theta<M>(s, N, theta);
}
