// tq_joint.h -- two colour channels as one hidden Markov chain (`smooth --joint`), host+device
// inline bodies.  The hidden state is s = z_a + 2 z_b (0 neither bound, 1 only a, 2 only b, 3 both), theta = (A row-major
// (4, 4), rho (4)) with the layout, floor and renormalisation of tq_hmm_model<4>, and the emission of a state is the
// product of the two channels' evidence, l_f(s) = l^a_f(s & 1) l^b_f(s >> 1):
//   * the chain with its two priors and the emission of a frame;
//   * what one lane of the E-step does with its chunk of frames: the chunk product and the two sweeps of tq_hmm.h with
//     that emission.  These are written out beside tq_hmm.h's instead of turning its bodies into templates over the
//     emission, so that tq_hmm.h is not touched and every kernel built from it keeps its machine code; whatever does not
//     see the emission -- TqHmmMat and its products, the floor, the prefix and suffix vectors -- is tq_hmm.h's;
//   * the M-step under one of five structures of A, closed forms in the margins of the summed pair counts;
//   * the Viterbi path of a row with four emission logarithms per frame.
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

// ---- a lane's chunk product and sweeps: tq_hmm_chunk, tq_hmm_forward and tq_hmm_backward with the joint emission --------
TQ_HD TqHmmMat<TQ_JOINT_M> tq_joint_chunk(const TqJointModel& m, const float* pa, const float* pb, int lo, int hi) {
  constexpr int M = TQ_JOINT_M;
  TqHmmMat<M> c = tq_hmm_identity<M>();
  for (int f = lo; f < hi; ++f) {
    double l[M];
    tq_joint_emission(m, pa[f], pb[f], l);
    TqHmmMat<M> t;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) {
        double s = c.m[i][0] * m.A[0][j];
#pragma unroll
        for (int k = 1; k < M; ++k) s += c.m[i][k] * m.A[k][j];
        t.m[i][j] = (f == 0 ? m.rho[j] : s) * l[j];
      }
    tq_hmm_rescale(t);
    c = t;
  }
  return c;
}

// writes a_f into filt[f * 4 ..]; returns the lane's sum of log c_f
TQ_HD double tq_joint_forward(const TqJointModel& m, const float* pa, const float* pb, int lo, int hi, const double* v0,
                              double* filt) {
  constexpr int M = TQ_JOINT_M;
  double v[M], mant = 1.0;
  int expo = 0;
#pragma unroll
  for (int i = 0; i < M; ++i) v[i] = v0[i];
  for (int f = lo; f < hi; ++f) {
    double l[M], u[M], c = 0.0;
    tq_joint_emission(m, pa[f], pb[f], l);
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = v[0] * m.A[0][j];
#pragma unroll
      for (int k = 1; k < M; ++k) s += v[k] * m.A[k][j];
      u[j] = (f == 0 ? m.rho[j] : s) * l[j];
      c += u[j];
    }
    const double r = 1.0 / c;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      v[j] = u[j] * r;
      filt[(int64_t)f * M + j] = v[j];
    }
    int e;
    mant = frexp(mant * c, &e);
    expo += e;
  }
  return log(mant) + (double)expo * 0.69314718055994530942;
}

// acc[i * 4 + j] += E n_ij of the pairs (g - 1, g) with g in the lane's frames; acc[16 + i] = gamma_0(i) in the lane that
// owns frame 0.  GAMMA = false stores no gamma_g and does not read `gam`; the sums are the same.
template <bool GAMMA>
TQ_HD void tq_joint_backward(const TqJointModel& m, const float* pa, const float* pb, int lo, int hi, const double* b0,
                             const double* v, const double* filt, double* gam, double* acc) {
  constexpr int M = TQ_JOINT_M;
  double b[M];
#pragma unroll
  for (int i = 0; i < M; ++i) b[i] = b0[i];
  for (int g = hi - 1; g >= lo; --g) {
    double r[M], s = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      r[i] = filt[(int64_t)g * M + i] * b[i];
      s += r[i];
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
      r[i] /= s;
      if constexpr (GAMMA) gam[(int64_t)g * M + i] = r[i];
    }
    if (g == 0) {
#pragma unroll
      for (int i = 0; i < M; ++i) acc[M * M + i] = r[i];
      break;
    }
    double l[M], w[M], x[M][M], tot = 0.0;
    tq_joint_emission(m, pa[g], pb[g], l);
#pragma unroll
    for (int j = 0; j < M; ++j) w[j] = l[j] * b[j];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const double pi = g > lo ? filt[(int64_t)(g - 1) * M + i] : v[i];  // a_{g-1}(i)
      double rs = 0.0;
#pragma unroll
      for (int j = 0; j < M; ++j) {
        x[i][j] = pi * m.A[i][j] * w[j];
        rs += x[i][j];
      }
      tot += rs;
    }
    const double rt = 1.0 / tot;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) acc[i * M + j] += x[i][j] * rt;
    double bs = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double t = m.A[i][0] * w[0];
#pragma unroll
      for (int j = 1; j < M; ++j) t += m.A[i][j] * w[j];
      b[i] = t;
      bs += t;
    }
    int e;
    (void)frexp(bs, &e);
#pragma unroll
    for (int i = 0; i < M; ++i) b[i] = ldexp(b[i], -e);
  }
}

// acc[0 .. 21) of the lane that owns [lo, hi), in the column order of tq_hmm_estep
template <bool GAMMA>
TQ_HD void tq_joint_sweeps(const TqJointModel& m, const float* pa, const float* pb, int lo, int hi, const double* v,
                           const double* b, double* filt, double* gam, double* acc) {
#pragma unroll
  for (int j = 0; j < TQ_JOINT_COLS; ++j) acc[j] = 0.0;
  acc[TQ_JOINT_COLS - 1] = tq_joint_forward(m, pa, pb, lo, hi, v, filt);
  tq_joint_backward<GAMMA>(m, pa, pb, lo, hi, b, v, filt, gam, acc);
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

// ---- Viterbi ----------------------------------------------------------------------------------------------------------
// tq_hmm_viterbi_row<4> with the emission logarithm of state s formed as log l^a(s & 1) + log l^b(s >> 1): the same
// relative scores, back-pointer words and tie rule (lowest state).
TQ_HD void tq_joint_log_emission(const TqJointModel& m, float pa, float pb, double* ll) {
  double a0, a1, b0, b1;
  tq_smooth_evidence(m.eva, pa, a0, a1);
  tq_smooth_evidence(m.evb, pb, b0, b1);
  const double la0 = log(a0), la1 = log(a1), lb0 = log(b0), lb1 = log(b1);
  ll[0] = la0 + lb0;
  ll[1] = la1 + lb0;
  ll[2] = la0 + lb1;
  ll[3] = la1 + lb1;
}

TQ_HD void tq_joint_viterbi_row(const TqJointModel& m, const float* pa, const float* pb, int F, uint32_t* back,
                                int64_t stride, uint8_t* path) {
  constexpr int M = TQ_JOINT_M;
  double la[M][M], d[M], ll[M];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) la[i][j] = log(m.A[i][j]);
  tq_joint_log_emission(m, pa[0], pb[0], ll);
  const double s00 = log(m.rho[0]) + ll[0];
  d[0] = 0.0;
#pragma unroll
  for (int i = 1; i < M; ++i) d[i] = (log(m.rho[i]) + ll[i]) - s00;
  uint32_t word = 0;
  for (int f = 1; f < F; ++f) {
    tq_joint_log_emission(m, pa[f], pb[f], ll);
    double s[M];
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double best = la[0][j];
      uint32_t bp = 0;
#pragma unroll
      for (int i = 1; i < M; ++i) {
        const double cand = d[i] + la[i][j];
        if (cand > best) {
          best = cand;
          bp = (uint32_t)i;
        }
      }
      s[j] = best + ll[j];
      bits |= bp << (2 * j);
    }
#pragma unroll
    for (int j = 1; j < M; ++j) d[j] = s[j] - s[0];
    word |= bits << (8 * (f & 3));
    if ((f & 3) == 3 || f == F - 1) {
      back[(int64_t)(f >> 2) * stride] = word;
      word = 0;
    }
  }
  uint32_t z = 0;
  double best = 0.0;
#pragma unroll
  for (int i = 1; i < M; ++i)
    if (d[i] > best) {
      best = d[i];
      z = (uint32_t)i;
    }
  path[F - 1] = (uint8_t)z;
  for (int f = F - 1; f >= 1; --f) {
    if ((f & 3) == 3 || f == F - 1) word = back[(int64_t)(f >> 2) * stride];
    z = (word >> (8 * (f & 3) + 2 * z)) & 3u;
    path[f - 1] = (uint8_t)z;
  }
}
