// tq_timed.h -- the continuous-time hidden Markov chain on the frame timestamps (`smooth --timed`),
// host+device inline bodies, templated on the number of states M = U + B in {2, 3, 4}:
//   * the chain read from theta = (Q row-major, rho): a free off-diagonal rate floored, a forbidden one exactly 0, the
//     diagonal minus the row's sum, rho floored and renormalised as tq_hmm_floor does;
//   * the tables of one gap class, P = exp(Q d) and K[a][b][i][j] = int_0^d P_ai(s) P_jb(d - s) ds, by a Taylor series of
//     the uniformised chain at d / 2^s and s squarings of the pair (P, K).  Every term and every product is non-negative,
//     so nothing cancels; there is no eigendecomposition and no 2M x 2M matrix;
//   * the two things the tq_chain_* bodies of tq_hmm.h ask of a chain: the transition into frame f, read from
//     P[cls[f - 1]], and what the pair (g - 1, g) adds to a lane's sums, the contraction of the rank-one pair posterior with
//     K[cls[g - 1]] in the place of the pair marginals;
//   * the forward sweep, tq_chain_forward overloaded for this chain: the one sweep kept as a text of its own, for the
//     rounding of the normaliser c_f (see there);
//   * the M-step of the summed rows: q_ij = sum E N_ij / sum E T_i.
// The chunk product, the backward sweep, the products, their rescaling, the prefix and suffix vectors and the lane ranges
// are tq_hmm.h's and tq_smooth.h's.
// Nothing here divides by a transition probability, so an exact zero in Q or P is safe.
// The __global__ wrappers are in tq_timed.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include "tq_hmm.h"
#include "tq_multistart.h"

#define TQ_TIMED_ORDER 20    // Taylor terms of the tables after the zeroth; the remainder is below 1 / 21! of the sum
#define TQ_TIMED_MAX_SQ 1100  // squarings at most: the binary exponent of a finite lambda d is below 1025

// ---- chain --------------------------------------------------------------------------------------------------------------
template <int M>
struct TqTimedModel {
  double Q[M][M];  // generator per unit of the gaps; rows sum to 0
  double rho[M];
  TqSmoothModel ev;  // inv0, inv1 only: the fit's prior, divided out of p by tq_smooth_evidence
  int U;             // states 0 .. U - 1 are class 0
  uint32_t allow;    // bit i * M + j set: q_ij is free (the diagonal bits are not read)
};

template <int M>
TQ_HD bool tq_timed_free(uint32_t allow, int i, int j) {
  return ((allow >> (i * M + j)) & 1u) != 0u;
}

template <int M>
TQ_HD TqTimedModel<M> tq_timed_model(const double* theta, int U, double prior, uint32_t allow) {
  TqTimedModel<M> m;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      if (j == i) continue;
      m.Q[i][j] = tq_timed_free<M>(allow, i, j) ? fmax(theta[i * M + j], TQ_SMOOTH_RMIN) : 0.0;
      s += m.Q[i][j];
    }
    m.Q[i][i] = -s;
  }
  tq_hmm_floor<M>(theta + M * M, m.rho);
  m.ev = TqSmoothModel{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / (1.0 - prior), 1.0 / prior};
  m.U = U;
  m.allow = allow;
  return m;
}

// l[i] = l_f(class(i)), the emission of tq_hmm_emission
template <int M>
struct TqTimedEmit {
  const TqTimedModel<M>& m;
  const float* pr;
  TQ_HD void operator()(int f, double* l) const {
    double l0, l1;
    tq_smooth_evidence(m.ev, pr[f], l0, l1);
#pragma unroll
    for (int i = 0; i < M; ++i) l[i] = i < m.U ? l0 : l1;
  }
};

// ---- tables -------------------------------------------------------------------------------------------------------------
// z = x y
template <int M>
TQ_HD void tq_timed_matmul(const double (&x)[M][M], const double (&y)[M][M], double (&z)[M][M]) {
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double s = x[r][0] * y[0][c];
#pragma unroll
      for (int k = 1; k < M; ++k) s += x[r][k] * y[k][c];
      z[r][c] = s;
    }
}

// every row of a non-negative x over its sum: exp(Q h) is stochastic, and a row sum that has drifted from 1 would drift
// twice as far with every squaring
template <int M>
TQ_HD void tq_timed_stochastic(double (&x)[M][M]) {
#pragma unroll
  for (int r = 0; r < M; ++r) {
    double s = x[r][0];
#pragma unroll
    for (int c = 1; c < M; ++c) s += x[r][c];
    const double q = 1.0 / s;
#pragma unroll
    for (int c = 0; c < M; ++c) x[r][c] *= q;
  }
}

// P = exp(Q d) and, for one pair (i, j), Kij[a][b] = int_0^d P_ai(s) P_jb(d - s) ds: the upper-right block of
// exp(d [[Q, E_ij], [0, Q]]) (Van Loan), kept as the pair (P, Kij) of M x M matrices.
// With lambda = max_i -q_ii, R = Q + lambda I has no negative entry and exp(Q h) = e^(-lambda h) exp(R h), so at
// h = d / 2^s with lambda h < 1/2
//   P(h)   = e^(-lambda h) sum_t (R h)^t / t!
//   Kij(h) = e^(-lambda h) sum_t h^(t+1) / (t+1)! sum_(m+n=t) R^m E_ij R^n
// are sums of non-negative terms; term t + 1 of the second follows from term t as (Kt (R h) + h Pt' E_ij) / (t + 2), Pt'
// the new term of the first.  Then s times (P, Kij) <- (P P, P Kij + Kij P): products of non-negative matrices again, the
// rows of P brought back to a sum of 1 after the series and after every squaring (tq_timed_stochastic).
template <int M>
TQ_HD void tq_timed_table_entry(const TqTimedModel<M>& m, double d, int i, int j, double (&P)[M][M], double (&Kij)[M][M]) {
  double lam = 0.0;
#pragma unroll
  for (int r = 0; r < M; ++r) lam = fmax(lam, -m.Q[r][r]);
  double x = lam * d;
  if (!(x < 1e300)) x = 1e300;
  int e;
  (void)frexp(x, &e);  // x = 0: e = 0
  int sq = e + 1 < 0 ? 0 : e + 1;
  if (sq > TQ_TIMED_MAX_SQ) sq = TQ_TIMED_MAX_SQ;
  const double h = ldexp(d, -sq);
  // the unit vectors of i and j as numbers: a product with them picks a row or a column without an array indexed at run time
  double Rh[M][M], Pt[M][M], Kt[M][M], tmp[M][M], ei[M], ej[M];
#pragma unroll
  for (int c = 0; c < M; ++c) {
    ei[c] = c == i ? 1.0 : 0.0;
    ej[c] = c == j ? 1.0 : 0.0;
  }
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) {
      Rh[r][c] = (m.Q[r][c] + (r == c ? lam : 0.0)) * h;
      Pt[r][c] = P[r][c] = r == c ? 1.0 : 0.0;
      Kt[r][c] = Kij[r][c] = ei[r] * ej[c] * h;
    }
  for (int t = 0; t < TQ_TIMED_ORDER; ++t) {
    const double rp = 1.0 / (double)(t + 1), rk = 1.0 / (double)(t + 2);
    tq_timed_matmul<M>(Pt, Rh, tmp);
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
      for (int c = 0; c < M; ++c) {
        Pt[r][c] = tmp[r][c] * rp;
        P[r][c] += Pt[r][c];
      }
    tq_timed_matmul<M>(Kt, Rh, tmp);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      double col = Pt[r][0] * ei[0];  // (Pt E_ij)[r][c] = Pt[r][i] where c == j
#pragma unroll
      for (int c = 1; c < M; ++c) col += Pt[r][c] * ei[c];
      col *= h;
#pragma unroll
      for (int c = 0; c < M; ++c) {
        Kt[r][c] = (tmp[r][c] + ej[c] * col) * rk;
        Kij[r][c] += Kt[r][c];
      }
    }
  }
  const double decay = exp(-lam * h);
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) {
      P[r][c] *= decay;
      Kij[r][c] *= decay;
    }
  tq_timed_stochastic<M>(P);
  for (int q = 0; q < sq; ++q) {
    tq_timed_matmul<M>(P, Kij, tmp);
    tq_timed_matmul<M>(Kij, P, Kt);
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
      for (int c = 0; c < M; ++c) Kij[r][c] = tmp[r][c] + Kt[r][c];
    tq_timed_matmul<M>(P, P, tmp);
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
      for (int c = 0; c < M; ++c) P[r][c] = tmp[r][c];
    tq_timed_stochastic<M>(P);
  }
}

// Work item `ij` = i * M + j of class k: writes K[k][a][b][i][j] for every (a, b), and, where ij == 0, P[k].
template <int M>
TQ_HD void tq_timed_table_item(const TqTimedModel<M>& m, const double* d, int k, int ij, double* Pout, double* Kout) {
  double P[M][M], Kij[M][M];
  tq_timed_table_entry<M>(m, d[k], ij / M, ij % M, P, Kij);
  double* Kk = Kout + (int64_t)k * (M * M * M * M);
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int b = 0; b < M; ++b) Kk[(a * M + b) * (M * M) + ij] = Kij[a][b];
  if (ij == 0) {
    double* Pk = Pout + (int64_t)k * (M * M);
#pragma unroll
    for (int a = 0; a < M; ++a)
#pragma unroll
      for (int b = 0; b < M; ++b) Pk[a * M + b] = P[a][b];
  }
}

// ---- the chain as the tq_chain_* bodies of tq_hmm.h take it ---------------------------------------------------------------
// the model with the tables of its D gap classes and the class of every gap: cls[f - 1] is that of (f - 1, f), and may be
// NULL where there is one frame
template <int M>
struct TqTimedChain : TqTimedModel<M> {
  const double* P;  // (D, M, M)
  const double* K;  // (D, M, M, M, M), K[k][a][b][i][j]
  const int32_t* cls;
};

template <int M>
TQ_HD TqTimedChain<M> tq_timed_chain(const double* theta, int U, double prior, uint32_t allow, const double* P,
                                     const double* K, const int32_t* cls) {
  return TqTimedChain<M>{tq_timed_model<M>(theta, U, prior, allow), P, K, cls};
}

// one gap class: its index and its P; only the pair sums read its K, so only they form that address
template <int M>
struct TqTimedStep {
  const double* P;
  int64_t k;
  TQ_HD double A(int i, int j) const { return P[i * M + j]; }
};

// the transition into frame f: the tables of class cls[f - 1].  Frame 0 has no gap before it and the bodies discard what
// they compute there, so it gets class 0's, which exist (D >= 1), and cls[-1] is not read.
template <int M>
TQ_HD TqTimedStep<M> tq_chain_step(const TqTimedChain<M>& m, int f) {
  const int64_t k = f > 0 ? m.cls[f - 1] : 0;
  return TqTimedStep<M>{m.P + k * (M * M), k};
}

// The forward sweep, tq_chain_forward for this chain: tq_chain_sweeps finds it by its argument.  It is a text of its own
// for the rounding of c_f alone.  tq_hmm.h's selects between rho_j and the sum, which leaves the product u_j and the sum
// c_f in one basic block, and the device build fuses them there into FMAs; here frame 0 is a branch of its own and c_f adds
// the rounded products.  These are the bits filt and the log evidence of this chain have had from the start, so they stay.
template <int M, class Emit>
TQ_HD double tq_chain_forward(const TqTimedChain<M>& m, const Emit& em, int lo, int hi, const double* v0, double* filt) {
  double v[M], mant = 1.0;
  int expo = 0;
#pragma unroll
  for (int i = 0; i < M; ++i) v[i] = v0[i];
  for (int f = lo; f < hi; ++f) {
    double l[M], u[M], c = 0.0;
    em(f, l);
    if (f == 0) {
#pragma unroll
      for (int j = 0; j < M; ++j) u[j] = m.rho[j] * l[j];
    } else {
      const double* A = m.P + (int64_t)m.cls[f - 1] * (M * M);
#pragma unroll
      for (int j = 0; j < M; ++j) {
        double s = v[0] * A[j];
#pragma unroll
        for (int k = 1; k < M; ++k) s += v[k] * A[k * M + j];
        u[j] = s * l[j];
      }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) c += u[j];
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

// The gap (g - 1, g) of class k, with a = a_{g-1}, w = l_g o beta_g and tot = sum_xy a_x P[k]_xy w_y, gives the rank-one pair
// posterior c_xy = a_x w_y / tot over P[k]_xy and
//   acc[i * M + i] += sum_xy c_xy K[k][x][y][i][i]         (E T_i, the expected time in state i)
//   acc[i * M + j] += q_ij sum_xy c_xy K[k][x][y][i][j]    (E N_ij, the expected number of jumps; free pairs only)
// summed over x and y into M * M running sums, one K row of M * M at a time.  A forbidden pair's K is loaded and not used:
// its slot stays 0 whatever the table holds there.
template <int M>
TQ_HD void tq_chain_pair(const TqTimedChain<M>& m, const TqTimedStep<M>& s, const double* a, const double* w, double* acc) {
  // t is row i of P[k] w, which tq_chain_backward's beta update forms again in the same statements: once inlined the two
  // are one computation (the kernels' register counts show it), so it is not carried from here to there by hand
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double t = s.A(i, 0) * w[0];
#pragma unroll
    for (int j = 1; j < M; ++j) t += s.A(i, j) * w[j];
    tot += a[i] * t;
  }
  const double* Kk = m.K + s.k * (M * M * M * M);
  double e[M * M];
#pragma unroll
  for (int q = 0; q < M * M; ++q) e[q] = 0.0;
#pragma unroll
  for (int x = 0; x < M; ++x)
#pragma unroll
    for (int y = 0; y < M; ++y) {
      const double c = a[x] * w[y];
      const double* row = Kk + (x * M + y) * (M * M);
#pragma unroll
      for (int q = 0; q < M * M; ++q) e[q] += c * row[q];
    }
  const double rt = 1.0 / tot;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      if (i == j)
        acc[i * M + i] += e[i * M + i] * rt;
      else
        acc[i * M + j] += tq_timed_free<M>(m.allow, i, j) ? m.Q[i][j] * (e[i * M + j] * rt) : 0.0;
    }
}

// the shared bodies under the timed chain's earlier names, for a caller that holds the model and the tables apart: one
// line each, nothing of their own (as tq_hmm_chunk and tq_multistart_sweeps).  The chunk product reads no K.
template <int M, class Emit>
TQ_HD TqHmmMat<M> tq_timed_chunk(const TqTimedModel<M>& m, const Emit& em, const double* P, const int32_t* cls, int lo,
                                 int hi) {
  return tq_chain_chunk<M>(TqTimedChain<M>{m, P, nullptr, cls}, em, lo, hi);
}
template <int M, bool GAMMA, class Emit>
TQ_HD void tq_timed_sweeps(const TqTimedModel<M>& m, const Emit& em, const double* P, const double* K, const int32_t* cls,
                           int lo, int hi, const double* v, const double* b, double* filt, double* gam, double* acc) {
  tq_chain_sweeps<M, GAMMA>(TqTimedChain<M>{m, P, K, cls}, em, lo, hi, v, b, filt, gam, acc);
}

// ---- M-step -------------------------------------------------------------------------------------------------------------
// sums[0 .. TQ_HMM_COLS(M)) over the N rows -> theta: q_ij = sum E N_ij / sum E T_i floored for a free pair, exactly 0 for a
// forbidden one, the stored diagonal minus the row's sum; a state without expected time keeps its free rates.  rho is the
// mean gamma_0, floored and renormalised.
template <int M>
TQ_HD void tq_timed_mstep_theta(const double* sums, int N, uint32_t allow, double* theta) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const double T = sums[i * M + i];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      if (j == i) continue;
      double q = 0.0;
      if (tq_timed_free<M>(allow, i, j)) q = T > 0.0 ? fmax(sums[i * M + j] / T, TQ_SMOOTH_RMIN) : theta[i * M + j];
      theta[i * M + j] = q;
      s += q;
    }
    theta[i * M + i] = -s;
  }
  double g[M];
#pragma unroll
  for (int i = 0; i < M; ++i) g[i] = sums[M * M + i] / (double)N;
  tq_hmm_floor<M>(g, theta + M * M);
}
