// tq_joint.h -- two colour channels as one hidden Markov chain (`smooth --joint`), host+device
// inline bodies.  The hidden state is s = z_a + 2 z_b (0 neither bound, 1 only a, 2 only b, 3 both), theta = (A row-major
// (4, 4), rho (4)) with the layout, floor and renormalisation of tq_hmm_model<4>, and the emission of a state is the
// product of the two channels' evidence, l_f(s) = l^a_f(s & 1) l^b_f(s >> 1):
//   * the chain with its two priors, and the emission of a frame and its logarithm as the callables TqJointEmit and
//     TqJointLogEmit;
//   * the M-step under one of five structures of A, closed forms in the margins of the summed pair counts;
//   * a row of the backward sampler walked, as it is drawn, into the runs of one channel, each with the other channel's
//     state at its two ends (tq_pair_dwell).
// The chunk product, the two sweeps and the Viterbi row are tq_hmm.h's tq_chain_* templates at M = 4, given TqJointModel
// as the chain and these callables: the joint chain has no sweep text of its own, and tq_joint_chunk, tq_joint_sweeps and
// tq_joint_viterbi_row are one-line names for those calls.
// The __global__ wrappers are in tq_joint.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "tq_multistart.h"

#define TQ_JOINT_M 4
#define TQ_JOINT_THETA (TQ_JOINT_M * TQ_JOINT_M + TQ_JOINT_M)
#define TQ_JOINT_COLS TQ_HMM_COLS(TQ_JOINT_M)

// ---- chain and emission -----------------------------------------------------------------------------------------------
struct TqJointModel {
  double A[TQ_JOINT_M][TQ_JOINT_M];
  double rho[TQ_JOINT_M];
  TqSmoothModel eva, evb;  // inv0, inv1 only: each channel's prior, divided out of its p by tq_smooth_evidence
};

TQ_HD TqJointModel tq_joint_model(const double* theta, double prior_a, double prior_b) {
  constexpr int M = TQ_JOINT_M;
  TqJointModel m;
#pragma unroll
  for (int i = 0; i < M; ++i) tq_hmm_floor<M>(theta + i * M, m.A[i]);
  tq_hmm_floor<M>(theta + M * M, m.rho);
  m.eva = TqSmoothModel{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / (1.0 - prior_a), 1.0 / prior_a};
  m.evb = TqSmoothModel{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / (1.0 - prior_b), 1.0 / prior_b};
  return m;
}

// l[s] = l^a(s & 1) l^b(s >> 1)
TQ_HD void tq_joint_emission(const TqJointModel& m, float pa, float pb, double* l) {
  double a0, a1, b0, b1;
  tq_smooth_evidence(m.eva, pa, a0, a1);
  tq_smooth_evidence(m.evb, pb, b0, b1);
  l[0] = a0 * b0;
  l[1] = a1 * b0;
  l[2] = a0 * b1;
  l[3] = a1 * b1;
}

// the emission of frame f of one row, as the tq_chain_* bodies of tq_hmm.h take it
struct TqJointEmit {
  const TqJointModel& m;
  const float *pa, *pb;
  TQ_HD void operator()(int f, double* l) const { tq_joint_emission(m, pa[f], pb[f], l); }
};

// ll[s] = log l^a(s & 1) + log l^b(s >> 1): four logarithms per frame, for tq_chain_viterbi_row
struct TqJointLogEmit {
  const TqJointModel& m;
  const float *pa, *pb;
  TQ_HD void operator()(int f, double* ll) const {
    double a0, a1, b0, b1;
    tq_smooth_evidence(m.eva, pa[f], a0, a1);
    tq_smooth_evidence(m.evb, pb[f], b0, b1);
    const double la0 = log(a0), la1 = log(a1), lb0 = log(b0), lb1 = log(b1);
    ll[0] = la0 + lb0;
    ll[1] = la1 + lb0;
    ll[2] = la0 + lb1;
    ll[3] = la1 + lb1;
  }
};

// tq_hmm.h's bodies under their names for the joint chain on one row's p_a and p_b: one line each, nothing of their own
TQ_HD TqHmmMat<TQ_JOINT_M> tq_joint_chunk(const TqJointModel& m, const float* pa, const float* pb, int lo, int hi) {
  return tq_chain_chunk<TQ_JOINT_M>(m, TqJointEmit{m, pa, pb}, lo, hi);
}
template <bool GAMMA>
TQ_HD void tq_joint_sweeps(const TqJointModel& m, const float* pa, const float* pb, int lo, int hi, const double* v,
                           const double* b, double* filt, double* gam, double* acc) {
  tq_chain_sweeps<TQ_JOINT_M, GAMMA>(m, TqJointEmit{m, pa, pb}, lo, hi, v, b, filt, gam, acc);
}
TQ_HD void tq_joint_viterbi_row(const TqJointModel& m, const float* pa, const float* pb, int F, uint32_t* back,
                                int64_t stride, uint8_t* path) {
  tq_chain_viterbi_row<TQ_JOINT_M>(m, TqJointLogEmit{m, pa, pb}, F, back, stride, path);
}

// ---- M-step -----------------------------------------------------------------------------------------------------------
TQ_HD bool tq_joint_structure_ok(int structure) { return structure >= TQ_JOINT_INDEPENDENT && structure <= TQ_JOINT_FULL; }

// sums[0 .. 21) over the N rows -> theta under `structure`.  With n = sums[s * 4 + s'] and s = (z_a, z_b):
//   P_a(z_a' | s) = sum_{z_b'} n[s -> (z_a', z_b')] / n[s -> .], and where channel a does not see z_b (independent,
//   a-drives-b) numerator and denominator are summed over z_b first, i.e. over the rows s and s ^ 2;
//   P_b is the mirror image, pooled over the rows s and s ^ 1 where channel b does not see z_a (independent, b-drives-a);
//   A[s -> s'] = P_a P_b, then the floor of tq_hmm_floor.  A row one of whose two denominators is zero keeps its old values.
// TQ_JOINT_FULL is tq_hmm_mstep_theta<4>.  rho = mean gamma_0, floored, for every structure.
TQ_HD void tq_joint_mstep_theta(const double* sums, int N, int structure, double* theta) {
  constexpr int M = TQ_JOINT_M;
  if (structure == TQ_JOINT_FULL) {
    tq_hmm_mstep_theta<M>(sums, N, theta);
    return;
  }
  const bool pool_a = structure == TQ_JOINT_INDEPENDENT || structure == TQ_JOINT_A_DRIVES_B;
  const bool pool_b = structure == TQ_JOINT_INDEPENDENT || structure == TQ_JOINT_B_DRIVES_A;
  double na[M][2], nb[M][2];  // na[s][z_a'], nb[s][z_b']: the margins of row s
#pragma unroll
  for (int s = 0; s < M; ++s) {
    const double* n = sums + s * M;
    na[s][0] = n[0] + n[2];
    na[s][1] = n[1] + n[3];
    nb[s][0] = n[0] + n[1];
    nb[s][1] = n[2] + n[3];
  }
  double q[M];
#pragma unroll
  for (int s = 0; s < M; ++s) {
    // a + b and b + a are the same double, so the two rows of a pool get the same factor bit for bit
    const double a0 = pool_a ? na[s][0] + na[s ^ 2][0] : na[s][0], a1 = pool_a ? na[s][1] + na[s ^ 2][1] : na[s][1];
    const double b0 = pool_b ? nb[s][0] + nb[s ^ 1][0] : nb[s][0], b1 = pool_b ? nb[s][1] + nb[s ^ 1][1] : nb[s][1];
    const double da = a0 + a1, db = b0 + b1;
    if (da > 0.0 && db > 0.0) {
      const double pa0 = a0 / da, pa1 = a1 / da, pb0 = b0 / db, pb1 = b1 / db;
      q[0] = pa0 * pb0;
      q[1] = pa1 * pb0;
      q[2] = pa0 * pb1;
      q[3] = pa1 * pb1;
      tq_hmm_floor<M>(q, theta + s * M);
    }
  }
#pragma unroll
  for (int i = 0; i < M; ++i) q[i] = sums[M * M + i] / (double)N;
  tq_hmm_floor<M>(q, theta + M * M);
}

// ---- backward sampler walked into one channel's intervals (tq_pair_dwell) ---------------------------
// The draws are TqHmmDraws / tq_hmm_thresholds<4> / tq_hmm_label<4> of tq_hmm.h, so row (s, n) is the row tq_hmm_count
// draws at (U, B) = (2, 2); the walk is TqSmoothWalk on the class z = (state >> which) & 1, channel a for which = 0 and
// channel b for which = 1.  New here is the partner q = (state >> (which ^ 1)) & 1: a run over [start, stop] gets the code
//   bit 0 = q(start), bit 1 = q(start - 1) (0 when start = 0), bit 2 = q(stop), bit 3 = q(stop + 1) (0 when stop = F - 1).
// The row comes from frame F - 1 downwards: bits 2 and 3 are known when the run opens, bits 0 and 1 when it closes.
struct TqPairDwellRow {
  TqChainDwellRow c;  // the walker, the state of the frame after the current one, the lowest frame seen with z = 1
  int qnext;          // q of the frame after the current one
  int open;           // bits 2 and 3 of the open run
  int qlow;           // the lowest frame seen with q = 1, or F
  int tau_after;      // qlow as it stood when the lowest frame with z = 1 was passed: the smallest f >= tau with q = 1, or F
};

TQ_HD void tq_pair_dwell_begin(TqPairDwellRow& r, int F) {
  tq_chain_dwell_begin(r.c, F);
  r.qnext = 0;
  r.open = 0;
  r.qlow = F;
  r.tau_after = F;
}

// Frame f with its uniform u and the twelve thresholds t of tq_hmm_thresholds<4> for that frame: draws the joint state as
// the sampler of tq_hmm_count does, and returns 1 and fills `out` and `code` when the frame closes the run of channel
// `which` that began at f + 1.
TQ_HD int tq_pair_dwell_frame(TqPairDwellRow& r, double u, const double* t, int f, int F, int which, TqDwellInterval& out,
                              int& code) {
  constexpr int M = TQ_JOINT_M;
  const bool last = f == F - 1;
  const int state = tq_hmm_label<M>(u, t + (last ? 0 : r.c.next) * (M - 1));
  const int z = (state >> which) & 1, q = (state >> (which ^ 1)) & 1;
  r.c.next = state;
  if (q) r.qlow = f;
  if (z) {
    r.c.tau = f;
    r.tau_after = r.qlow;
  }
  int closed = 0;
  if (last) {
    tq_smooth_walk_begin(r.c.w, F, z);
    r.open = q << 2;
  } else if (tq_smooth_walk_step(r.c.w, f, z, out)) {
    closed = 1;
    code = r.open | r.qnext | (q << 1);  // the closed run began at f + 1
    r.open = (q << 2) | (r.qnext << 3);  // the run that opens here stops at f
  }
  r.qnext = q;
  return closed;
}

// the run still open after frame 0: it starts the record, so bit 1 is 0
TQ_HD void tq_pair_dwell_finish(const TqPairDwellRow& r, TqDwellInterval& out, int& code) {
  tq_chain_dwell_finish(r.c, out);
  code = r.open | r.qnext;
}

// the F bins of sample s and partner state q at the run's start, in histograms of shape (S, 2, F)
TQ_HD int64_t tq_pair_hist_at(int s, int q, int F) { return ((int64_t)s * 2 + q) * F; }
