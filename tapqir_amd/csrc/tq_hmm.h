// tq_hmm.h -- hidden Markov smoothing with several hidden states per observable class (`smooth --bound-states`,
// DESIGN.md section 22), host+device inline bodies, templated on the number of states M = U + B in {2, 3, 4}:
//   * the chain read from theta = (A, rho), floored and renormalised, and the emission of a state: the evidence of its
//     class, tq_smooth_evidence;
//   * products of MxM matrices kept in range by powers of two, and what one lane of the E-step does with its chunk of
//     frames (tq_smooth_lane_range): the chunk product, the forward sweep from the chunk's exclusive prefix, the backward
//     sweep from its exclusive suffix with the pair marginals.  These tq_chain_* bodies see the chain as anything with
//     rho[M], a frame's emission through a callable em(f, l) -- TqHmmEmit here, TqJointEmit in tq_joint.h, TqTimedEmit in
//     tq_timed.h -- and ask the chain for two things: the transition into frame f, tq_chain_step, and what the pair
//     (g - 1, g) adds to a lane's sums, tq_chain_pair.  A chain with A[M][M] gets both from here: one A for every frame,
//     and the pair marginals.  The timed chain of tq_timed.h overloads both, and of the bodies tq_chain_forward alone,
//     for the rounding of its normaliser.  Every chain with M x M products runs this text;
//   * the M-step of the summed rows, the Viterbi path of a row in hidden states (tq_chain_viterbi_row: any chain with
//     A[M][M] and rho[M], the emission logarithms through a callable), and the backward sampler's thresholds;
//   * the sampler's uniforms in its order of draws, and a row drawn backwards and walked, as it is drawn, into runs of
//     equal class (tq_chain_dwell).
// The two-state bodies of tq_smooth.h stay apart on purpose: their layout differs (filt holds a_f(1) alone, gamma's row
// holds a_f(0), theta has three parameters), so folding them in would change what they store.  Nothing here subtracts
// nearly equal quantities: a_f is stored whole, and the sampler's thresholds are sums of tails.
// The __global__ wrappers are in tq_hmm.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include <math.h>

#include "../../include/tapqir_hip.h"
#include "tq_smooth.h"

#define TQ_HMM_SITE 0xA04u  // Philox site id of the backward sampler: stream (seed, step = s, site, elem = n)

// ---- chain and emission -----------------------------------------------------------------------------------------------
template <int M>
struct TqHmmModel {
  double A[M][M];
  double rho[M];
  TqSmoothModel ev;  // inv0, inv1 only: the fit's prior, divided out of p by tq_smooth_evidence
  int U;             // states 0 .. U - 1 are class 0
};

// out = max(in, TQ_SMOOTH_RMIN) / its sum: no zero entry and a sum of 1
template <int M>
TQ_HD void tq_hmm_floor(const double* in, double* out) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    out[i] = fmax(in[i], TQ_SMOOTH_RMIN);
    s += out[i];
  }
#pragma unroll
  for (int i = 0; i < M; ++i) out[i] /= s;
}

template <int M>
TQ_HD TqHmmModel<M> tq_hmm_model(const double* theta, int U, double prior) {
  TqHmmModel<M> m;
#pragma unroll
  for (int i = 0; i < M; ++i) tq_hmm_floor<M>(theta + i * M, m.A[i]);
  tq_hmm_floor<M>(theta + M * M, m.rho);
  m.ev = TqSmoothModel{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / (1.0 - prior), 1.0 / prior};
  m.U = U;
  return m;
}

// l[i] = l_f(class(i))
template <int M>
TQ_HD void tq_hmm_emission(const TqHmmModel<M>& m, float pf, double* l) {
  double l0, l1;
  tq_smooth_evidence(m.ev, pf, l0, l1);
#pragma unroll
  for (int i = 0; i < M; ++i) l[i] = i < m.U ? l0 : l1;
}

// the emission of frame f of one row, as the tq_chain_* bodies take it
template <int M>
struct TqHmmEmit {
  const TqHmmModel<M>& m;
  const float* pr;
  TQ_HD void operator()(int f, double* l) const { tq_hmm_emission(m, pr[f], l); }
};

// ll[i] = log l_f(class(i)): two logarithms per frame, state 0 is unbound and state M - 1 bound
template <int M>
struct TqHmmLogEmit {
  const TqHmmModel<M>& m;
  const float* pr;
  TQ_HD void operator()(int f, double* ll) const {
    double l[M];
    tq_hmm_emission(m, pr[f], l);
    const double ll0 = log(l[0]), ll1 = log(l[M - 1]);
#pragma unroll
    for (int i = 0; i < M; ++i) ll[i] = i < m.U ? ll0 : ll1;
  }
};

// ---- MxM products -----------------------------------------------------------------------------------------------------
template <int M>
struct TqHmmMat {
  double m[M][M];
};

template <int M>
TQ_HD TqHmmMat<M> tq_hmm_identity() {
  TqHmmMat<M> x;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) x.m[i][j] = i == j ? 1.0 : 0.0;
  return x;
}

// the power of two that brings the sum of the entries into [1/2, 1): exact (tq_smooth_rescale)
template <int M>
TQ_HD void tq_hmm_rescale(TqHmmMat<M>& x) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) s += x.m[i][j];
  int e;
  (void)frexp(s, &e);
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) x.m[i][j] = ldexp(x.m[i][j], -e);
}

// x y, rescaled (x is the earlier frames)
template <int M>
TQ_HD TqHmmMat<M> tq_hmm_mul(const TqHmmMat<M>& x, const TqHmmMat<M>& y) {
  TqHmmMat<M> r;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = x.m[i][0] * y.m[0][j];
#pragma unroll
      for (int k = 1; k < M; ++k) s += x.m[i][k] * y.m[k][j];
      r.m[i][j] = s;
    }
  tq_hmm_rescale(r);
  return r;
}

// ---- what the tq_chain_* bodies ask of a chain --------------------------------------------------------------------------
// tq_chain_step<M>(m, f): the transition into frame f, anything with A(i, j), fetched once per frame.  Frame 0 has none:
// the bodies ask all the same and discard what they compute from it, so a chain must return something readable there.
// tq_chain_pair<M>(m, t, a, w, acc): adds to acc[0 .. M * M) what the pair (g - 1, g) contributes, given the transition t
// into g, a = a_{g-1} and w = l_g o beta_g.
// These two are for a chain with A[M][M]: one A for every frame, and the pair marginals
// xi_{g-1}(i, j) ~ a_{g-1}(i) A[i][j] l_g(j) beta_g(j), so that acc[i * M + j] += E n_ij.  A chain of another kind
// overloads both on its own type (tq_timed.h).
template <int M>
struct TqChainStep {
  const double (&a)[M][M];
  TQ_HD double A(int i, int j) const { return a[i][j]; }
};

template <int M, class Chain>
TQ_HD TqChainStep<M> tq_chain_step(const Chain& m, int) {
  return TqChainStep<M>{m.A};
}

template <int M, class Chain, class Step>
TQ_HD void tq_chain_pair(const Chain&, const Step& t, const double* a, const double* w, double* acc) {
  double x[M][M], tot = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double rs = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      x[i][j] = a[i] * t.A(i, j) * w[j];
      rs += x[i][j];
    }
    tot += rs;
  }
  const double rt = 1.0 / tot;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) acc[i * M + j] += x[i][j] * rt;
}

// product of M_f = A_f diag(l_f) over the lane's frames, A_f the transition into f; M_0 has every row equal to rho o l_0,
// so that every prefix that holds frame 0 has rows proportional to a_f.  No frames: the identity.
template <int M, class Chain, class Emit>
TQ_HD TqHmmMat<M> tq_chain_chunk(const Chain& m, const Emit& em, int lo, int hi) {
  TqHmmMat<M> c = tq_hmm_identity<M>();
  for (int f = lo; f < hi; ++f) {
    double l[M];
    em(f, l);
    const auto a = tq_chain_step<M>(m, f);
    TqHmmMat<M> t;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) {
        double s = c.m[i][0] * a.A(0, j);
#pragma unroll
        for (int k = 1; k < M; ++k) s += c.m[i][k] * a.A(k, j);
        t.m[i][j] = (f == 0 ? m.rho[j] : s) * l[j];
      }
    tq_hmm_rescale(t);
    c = t;
  }
  return c;
}

// ---- the two sweeps of a lane -----------------------------------------------------------------------------------------
// a_{lo-1} from the lane's exclusive prefix (every row proportional to it; lane 0 has none and does not use it)
template <int M>
TQ_HD void tq_hmm_prefix_vector(const TqHmmMat<M>& e, double* v) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) s += e.m[0][j];
  const double r = 1.0 / s;
#pragma unroll
  for (int j = 0; j < M; ++j) v[j] = e.m[0][j] * r;
}

// beta_{hi-1} from the lane's exclusive suffix: its row sums (the last lane with frames has the identity: ones)
template <int M>
TQ_HD void tq_hmm_suffix_vector(const TqHmmMat<M>& e, double* b) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) s += e.m[i][j];
    b[i] = s;
  }
}

// Forward sweep over [lo, hi) from a_{lo-1} = v0: writes a_f into filt[f * M ..].  Returns the lane's sum of log c_f: the
// normalisers are multiplied up as mantissa and binary exponent, and one logarithm is taken at the end.
template <int M, class Chain, class Emit>
TQ_HD double tq_chain_forward(const Chain& m, const Emit& em, int lo, int hi, const double* v0, double* filt) {
  double v[M], mant = 1.0;
  int expo = 0;
#pragma unroll
  for (int i = 0; i < M; ++i) v[i] = v0[i];
  for (int f = lo; f < hi; ++f) {
    double l[M], u[M], c = 0.0;
    em(f, l);
    const auto a = tq_chain_step<M>(m, f);
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = v[0] * a.A(0, j);
#pragma unroll
      for (int k = 1; k < M; ++k) s += v[k] * a.A(k, j);
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

// Backward sweep over [lo, hi), g = hi - 1 .. lo, from beta_{hi-1} = b0.  Frame g gives gamma_g, and with a_{g-1} -- the
// lane's own, or v = a_{lo-1} of its prefix -- and w = l_g o beta_g what the pair (g - 1, g) adds to acc[0 .. M * M)
// (tq_chain_pair; the pair marginals unless the chain says otherwise): the pair belongs to the lane that owns g.
// acc[M * M + i] = gamma_0(i) in the lane that owns frame 0.  GAMMA = false stores no gamma_g and does not read `gam`; the
// sums are the same.
template <int M, bool GAMMA, class Chain, class Emit>
TQ_HD void tq_chain_backward(const Chain& m, const Emit& em, int lo, int hi, const double* b0, const double* v,
                             const double* filt, double* gam, double* acc) {
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
    double l[M], w[M], a[M];
    em(g, l);
    const auto t = tq_chain_step<M>(m, g);
#pragma unroll
    for (int j = 0; j < M; ++j) w[j] = l[j] * b[j];
#pragma unroll
    for (int i = 0; i < M; ++i) a[i] = g > lo ? filt[(int64_t)(g - 1) * M + i] : v[i];  // a_{g-1}(i)
    tq_chain_pair<M>(m, t, a, w, acc);
    // beta_{g-1} = A_g (l_g o beta_g), scaled by a power of two
    double bs = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double u = t.A(i, 0) * w[0];
#pragma unroll
      for (int j = 1; j < M; ++j) u += t.A(i, j) * w[j];
      b[i] = u;
      bs += u;
    }
    int e;
    (void)frexp(bs, &e);
#pragma unroll
    for (int i = 0; i < M; ++i) b[i] = ldexp(b[i], -e);
  }
}

// acc[0 .. TQ_HMM_COLS(M)) of the lane that owns [lo, hi): v = a_{lo-1} of its exclusive prefix, b = beta_{hi-1} of its
// exclusive suffix, filt the row's scratch of a_f.  The last column is the lane's sum of log c_f.
template <int M, bool GAMMA, class Chain, class Emit>
TQ_HD void tq_chain_sweeps(const Chain& m, const Emit& em, int lo, int hi, const double* v, const double* b, double* filt,
                           double* gam, double* acc) {
  constexpr int COLS = TQ_HMM_COLS(M);
#pragma unroll
  for (int j = 0; j < COLS; ++j) acc[j] = 0.0;
  acc[COLS - 1] = tq_chain_forward<M>(m, em, lo, hi, v, filt);
  tq_chain_backward<M, GAMMA>(m, em, lo, hi, b, v, filt, gam, acc);
}

// the same bodies under their names for the class chain on one row's p: one line each, nothing of their own
template <int M>
TQ_HD TqHmmMat<M> tq_hmm_chunk(const TqHmmModel<M>& m, const float* pr, int lo, int hi) {
  return tq_chain_chunk<M>(m, TqHmmEmit<M>{m, pr}, lo, hi);
}
template <int M>
TQ_HD double tq_hmm_forward(const TqHmmModel<M>& m, const float* pr, int lo, int hi, const double* v0, double* filt) {
  return tq_chain_forward<M>(m, TqHmmEmit<M>{m, pr}, lo, hi, v0, filt);
}
template <int M, bool GAMMA = true>
TQ_HD void tq_hmm_backward(const TqHmmModel<M>& m, const float* pr, int lo, int hi, const double* b0, const double* v,
                           const double* filt, double* gam, double* acc) {
  tq_chain_backward<M, GAMMA>(m, TqHmmEmit<M>{m, pr}, lo, hi, b0, v, filt, gam, acc);
}

// ---- M-step -----------------------------------------------------------------------------------------------------------
// sums[0 .. TQ_HMM_COLS(M)) over the N rows -> theta, floored and renormalised; a state without expected occupancy keeps
// its old row
template <int M>
TQ_HD void tq_hmm_mstep_theta(const double* sums, int N, double* theta) {
  double q[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double rs = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) rs += sums[i * M + j];
    if (rs > 0.0) {
#pragma unroll
      for (int j = 0; j < M; ++j) q[j] = sums[i * M + j] / rs;
      tq_hmm_floor<M>(q, theta + i * M);
    }
  }
#pragma unroll
  for (int i = 0; i < M; ++i) q[i] = sums[M * M + i] / (double)N;
  tq_hmm_floor<M>(q, theta + M * M);
}

// ---- Viterbi ----------------------------------------------------------------------------------------------------------
// One row, sequential in f.  The scores are kept relative to state 0's (d[i] = delta(i) - delta(0), d[0] = 0), so their
// size does not grow with F.  Back-pointers: the two bits at 8 (f & 3) + 2 j of word back[(f >> 2) * stride] are the best
// predecessor of state j at frame f >= 1; a tie takes the lowest state.  lem(f, ll) fills the M emission logarithms of
// frame f: TqHmmLogEmit, or TqJointLogEmit of tq_joint.h.
template <int M, class Chain, class LogEmit>
TQ_HD void tq_chain_viterbi_row(const Chain& m, const LogEmit& lem, int F, uint32_t* back, int64_t stride, uint8_t* path) {
  double la[M][M], d[M], ll[M];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) la[i][j] = log(m.A[i][j]);
  lem(0, ll);
  const double s00 = log(m.rho[0]) + ll[0];
  d[0] = 0.0;
#pragma unroll
  for (int i = 1; i < M; ++i) d[i] = (log(m.rho[i]) + ll[i]) - s00;
  uint32_t word = 0;
  for (int f = 1; f < F; ++f) {
    lem(f, ll);
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

template <int M>
TQ_HD void tq_hmm_viterbi_row(const TqHmmModel<M>& m, const float* pr, int F, uint32_t* back, int64_t stride,
                              uint8_t* path) {
  tq_chain_viterbi_row<M>(m, TqHmmLogEmit<M>{m, pr}, F, back, stride, path);
}

// ---- backward sampler -------------------------------------------------------------------------------------------------
// t[j * (M - 1) + i - 1] = t(i) given state_{f+1} = j, i = 1 .. M - 1: the mass of the states >= i under
// w(.) ~ a_f(.) A[.][j], as a sum of tails over the whole sum.  The last frame has no successor: w = a_{F-1} for every j.
template <int M>
TQ_HD void tq_hmm_thresholds(const TqHmmModel<M>& m, const double* af, bool last, double* t) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double tail[M];
    tail[M - 1] = last ? af[M - 1] : af[M - 1] * m.A[M - 1][j];
#pragma unroll
    for (int i = M - 2; i >= 0; --i) tail[i] = (last ? af[i] : af[i] * m.A[i][j]) + tail[i + 1];
#pragma unroll
    for (int i = 1; i < M; ++i) t[j * (M - 1) + i - 1] = tail[i] / tail[0];
  }
}

TQ_HD void tq_hmm_stream(TqPhilox* ph, uint64_t seed, int s, int n) {
  tq_philox_init(ph, seed, (uint32_t)s, TQ_HMM_SITE, (uint64_t)n);
}

// the largest i with u < t(i), or 0: u a uniform of the stream as a double, t the M - 1 thresholds of the successor's
// state, non-increasing in i
template <int M>
TQ_HD int tq_hmm_label(double u, const double* t) {
  int z = 0;
#pragma unroll
  for (int i = 1; i < M; ++i) z = u < t[i - 1] ? i : z;
  return z;
}

// ---- backward sampler walked into intervals (tq_chain_dwell) --------------------------------------
// The uniforms of row (s, n) in the order the sampler takes them: u_k belongs to frame F - 1 - k.  One Philox block is four
// of them, drawn together when k & 3 == 0 so that its words stay in registers; the values are those of one tq_uniform
// per frame.
struct TqHmmDraws {
  TqPhilox ph;
  double u0, u1, u2, u3;
};

TQ_HD void tq_hmm_draws_begin(TqHmmDraws& d, uint64_t seed, int s, int n) {
  tq_hmm_stream(&d.ph, seed, s, n);
  d.u0 = d.u1 = d.u2 = d.u3 = 0.0;
}

TQ_HD double tq_hmm_draws_next(TqHmmDraws& d, int k) {
  if ((k & 3) == 0) {
    d.u0 = (double)tq_uniform(&d.ph);
    d.u1 = (double)tq_uniform(&d.ph);
    d.u2 = (double)tq_uniform(&d.ph);
    d.u3 = (double)tq_uniform(&d.ph);
  }
  return (k & 3) == 0 ? d.u0 : (k & 3) == 1 ? d.u1 : (k & 3) == 2 ? d.u2 : d.u3;
}

// What a row keeps while it is drawn from frame F - 1 down to 0 and walked, as it is drawn, into runs of equal class: the
// hidden state of the frame after the current one, the walker of tq_smooth.h on the class z = (state >= U), and the
// lowest frame seen bound so far -- after frame 0 the first bound frame of the row, or F.
struct TqChainDwellRow {
  TqSmoothWalk w;
  int next;
  int tau;
};

TQ_HD void tq_chain_dwell_begin(TqChainDwellRow& r, int F) {
  r.w = TqSmoothWalk{0, 0, 0};
  r.next = 0;
  r.tau = F;
}

// Frame f with its uniform u and the M (M - 1) thresholds t of tq_hmm_thresholds for that frame: draws the state as the
// sampler of tq_hmm_count does, and returns 1 and fills `out` when the frame closes the run that began at f + 1.
template <int M>
TQ_HD int tq_chain_dwell_frame(TqChainDwellRow& r, double u, const double* t, int f, int F, int U, TqDwellInterval& out) {
  const bool last = f == F - 1;
  const int state = tq_hmm_label<M>(u, t + (last ? 0 : r.next) * (M - 1));
  const int z = state >= U ? 1 : 0;
  r.next = state;
  if (z) r.tau = f;
  if (last) {
    tq_smooth_walk_begin(r.w, F, z);
    return 0;
  }
  return tq_smooth_walk_step(r.w, f, z, out);
}

// the run still open after frame 0
TQ_HD void tq_chain_dwell_finish(const TqChainDwellRow& r, TqDwellInterval& out) { tq_smooth_walk_finish(r.w, out); }
