// tq_refit.h -- bootstrap refits of the chain of tq_hmm.h over AOIs (`smooth --refit`), host+device
// inline bodies, templated on the number of states M = U + B in {2, 3, 4}:
//   * the layout of the per-replica AOI weights and the weight of one AOI: how often the resample of tq_rates_index draws
//     it;
//   * what one thread of the weighted M-step sums, and what its thread 0 does with the totals.
// Everything else -- the chain, the sweeps, the replica layout, the topology mask and the floor -- is tq_multistart.h's and
// tq_hmm.h's, so that a replica with all weights 1 computes what tq_multistart_estep and tq_multistart_mstep compute.
// The __global__ wrappers are in tq_refit.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "tq_multistart.h"
#include "tq_rates.h"

// ---- layout -----------------------------------------------------------------------------------------------------------
TQ_HD int64_t tq_refit_weight_at(int r, int n, int N) { return (int64_t)r * N + n; }

// ---- weights ------------------------------------------------------------------------------------------------------------
// The AOI that draw i of sample s lands on: tq_rates_index, so that sample s resamples here the AOIs it resamples in
// tq_rates_estimate and tq_hmm_estimate at the same seed.  weights[n] = #{ i < N : tq_refit_draw(seed, s, i, N) = n }.
TQ_HD uint32_t tq_refit_draw(uint64_t seed, int s, uint32_t i, uint32_t N) { return tq_rates_index(seed, s, i, N); }

// ---- M-step -------------------------------------------------------------------------------------------------------------
// One thread's share of sum_n w[n] rows[n, .] and of sum_n w[n]: rows t, t + stride, ... in ascending n, the order of
// tq_chain_reduce_rows.  A row with w[n] == 0 is not read: the E-step never wrote it.  With w = 1 the product is exact, so
// the partial sums are those of tq_chain_reduce_rows bit for bit.
template <int COLS>
TQ_HD void tq_refit_thread_sums(const double* rows, const int32_t* w, int N, int t, int stride, double* s, int64_t& ws) {
#pragma unroll
  for (int j = 0; j < COLS; ++j) s[j] = 0.0;
  ws = 0;
  for (int n = t; n < N; n += stride) {
    const int32_t wn = w[n];
    if (wn == 0) continue;
    const double* row = rows + (int64_t)n * COLS;
    const double x = (double)wn;
#pragma unroll
    for (int j = 0; j < COLS; ++j) s[j] += x * row[j];
    ws += wn;
  }
}

// Thread 0 of the M-step: theta[r] from the weighted totals under `allow` with W = sum_n w[n] in the place of N, and the
// weighted log evidence.  W = 0 (no AOI drawn: not a resample) leaves A as it is and rho at the floor's uniform.
template <int M>
TQ_HD double tq_refit_mstep_theta(const double* sums, int64_t W, uint32_t allow, double* theta) {
  tq_multistart_mstep_theta<M>(sums, (int)W, allow, theta);
  return sums[TQ_HMM_COLS(M) - 1];
}
