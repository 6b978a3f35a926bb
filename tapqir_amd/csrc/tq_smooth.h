// tq_smooth.h -- two-state hidden Markov smoothing of a fit's z posterior (`smooth`), host+device
// inline bodies:
//   * the chain and the evidence of a frame, products of 2x2 matrices kept in range by powers of two;
//   * what one lane of the E-step does with its chunk of frames: the chunk product, the forward sweep from the chunk's
//     exclusive prefix, the backward sweep from its exclusive suffix with the pair marginals;
//   * the M-step of the summed rows, the Viterbi path of a row, and the backward sampler's thresholds and row counter;
//   * the interval walker of a row drawn backwards, with the table position and the table row of a run it closes.
// Nothing here subtracts nearly equal quantities: 1 - p, 1 - kon, 1 - koff, 1 - pi and 1 - pi0 are formed once, from
// their clamped arguments, and a_f(0) is kept beside a_f(1) instead of being recovered from it.
// The __global__ wrappers are in tq_smooth.hip; the test suite runs the same bodies from a g++ build.
#pragma once
#include <math.h>

#include "../../include/tapqir_hip.h"
#include "tq_dwell.h"
#include "tq_rates.h"

#define TQ_SMOOTH_SITE 0xA03u        // Philox site id of the backward sampler: stream (seed, step = s, site, elem = n)
#define TQ_SMOOTH_MSTEP_THREADS 256  // workgroup of the M-step: fixed, so that its order of additions is

// ---- chain and evidence -----------------------------------------------------------------------------------------------
struct TqSmoothModel {
  double a00, a01, a10, a11;  // A
  double rho0, rho1;          // initial law
  double inv0, inv1;          // 1 / (1 - pi), 1 / pi: the fit's prior, divided out of p
};

TQ_HD double tq_smooth_clamp(double x, double lo) { return fmin(fmax(x, lo), 1.0 - lo); }

TQ_HD TqSmoothModel tq_smooth_model(const double* theta, double prior) {
  const double kon = tq_smooth_clamp(theta[0], TQ_SMOOTH_RMIN), koff = tq_smooth_clamp(theta[1], TQ_SMOOTH_RMIN);
  const double pi0 = tq_smooth_clamp(theta[2], TQ_SMOOTH_RMIN);
  TqSmoothModel m;
  m.a00 = 1.0 - kon;
  m.a01 = kon;
  m.a10 = koff;
  m.a11 = 1.0 - koff;
  m.rho0 = 1.0 - pi0;
  m.rho1 = pi0;
  m.inv0 = 1.0 / (1.0 - prior);
  m.inv1 = 1.0 / prior;
  return m;
}

// l_f = ((1 - p) / (1 - pi), p / pi) of the clamped p
TQ_HD void tq_smooth_evidence(const TqSmoothModel& m, float pf, double& l0, double& l1) {
  const double p = tq_smooth_clamp((double)pf, TQ_SMOOTH_PMIN);
  l0 = (1.0 - p) * m.inv0;
  l1 = p * m.inv1;
}

// ---- 2x2 products -----------------------------------------------------------------------------------------------------
struct TqSmoothMat {
  double m00, m01, m10, m11;
};

TQ_HD TqSmoothMat tq_smooth_identity() { return TqSmoothMat{1.0, 0.0, 0.0, 1.0}; }

// Entries are non-negative and only the direction of a product's rows and columns is used, so every product is scaled
// by the power of two that brings the sum of its entries into [1/2, 1): exact, and no log scale needs to be carried.
TQ_HD void tq_smooth_rescale(TqSmoothMat& x) {
  int e;
  (void)frexp(x.m00 + x.m01 + x.m10 + x.m11, &e);
  x.m00 = ldexp(x.m00, -e);
  x.m01 = ldexp(x.m01, -e);
  x.m10 = ldexp(x.m10, -e);
  x.m11 = ldexp(x.m11, -e);
}

// x y, rescaled (the products do not commute: x is the earlier frames)
TQ_HD TqSmoothMat tq_smooth_mul(const TqSmoothMat& x, const TqSmoothMat& y) {
  TqSmoothMat r{x.m00 * y.m00 + x.m01 * y.m10, x.m00 * y.m01 + x.m01 * y.m11, x.m10 * y.m00 + x.m11 * y.m10,
                x.m10 * y.m01 + x.m11 * y.m11};
  tq_smooth_rescale(r);
  return r;
}

// frames [lo, hi) of lane `lane` of 64: L = ceil(F / 64) consecutive frames each, the last lanes empty (lo = hi = F)
TQ_HD void tq_smooth_lane_range(int lane, int F, int& lo, int& hi) {
  const int L = (F + 63) / 64;
  lo = lane * L < F ? lane * L : F;
  hi = lo + L < F ? lo + L : F;
}

// product of M_f = A diag(l_f) over the lane's frames; M_0 has both rows equal to rho o l_0, so that every prefix that
// holds frame 0 has both rows proportional to a_f.  No frames: the identity.
TQ_HD TqSmoothMat tq_smooth_chunk(const TqSmoothModel& m, const float* pr, int lo, int hi) {
  TqSmoothMat c = tq_smooth_identity();
  for (int f = lo; f < hi; ++f) {
    double l0, l1;
    tq_smooth_evidence(m, pr[f], l0, l1);
    if (f == 0) {
      c = TqSmoothMat{m.rho0 * l0, m.rho1 * l1, m.rho0 * l0, m.rho1 * l1};
    } else {
      c = TqSmoothMat{(c.m00 * m.a00 + c.m01 * m.a10) * l0, (c.m00 * m.a01 + c.m01 * m.a11) * l1,
                      (c.m10 * m.a00 + c.m11 * m.a10) * l0, (c.m10 * m.a01 + c.m11 * m.a11) * l1};
    }
    tq_smooth_rescale(c);
  }
  return c;
}

// ---- the two sweeps of a lane -----------------------------------------------------------------------------------------
// a_{lo-1} from the lane's exclusive prefix (both rows proportional to it; lane 0 has none and does not use it)
TQ_HD void tq_smooth_prefix_vector(const TqSmoothMat& e, double& v0, double& v1) {
  const double r = 1.0 / (e.m00 + e.m01);
  v0 = e.m00 * r;
  v1 = e.m01 * r;
}

// Forward sweep over [lo, hi) from a_{lo-1} = (v0, v1): writes a_f(1) into filt and a_f(0) into the row of gamma, which
// the backward sweep of the same lane reads back and overwrites.  Returns the lane's sum of log c_f: the normalisers are
// multiplied up as mantissa and binary exponent, and one logarithm is taken at the end.
TQ_HD double tq_smooth_forward(const TqSmoothModel& m, const float* pr, int lo, int hi, double v0, double v1, double* filt,
                               double* gam) {
  double mant = 1.0;
  int expo = 0;
  for (int f = lo; f < hi; ++f) {
    double l0, l1;
    tq_smooth_evidence(m, pr[f], l0, l1);
    const double u0 = (f == 0 ? m.rho0 : v0 * m.a00 + v1 * m.a10) * l0;
    const double u1 = (f == 0 ? m.rho1 : v0 * m.a01 + v1 * m.a11) * l1;
    const double c = u0 + u1, r = 1.0 / c;
    v0 = u0 * r;
    v1 = u1 * r;
    gam[f] = v0;
    filt[f] = v1;
    int e;
    mant = frexp(mant * c, &e);
    expo += e;
  }
  return log(mant) + (double)expo * 0.69314718055994530942;
}

// Backward sweep over [lo, hi), g = hi - 1 .. lo, from beta_{hi-1} = (b0, b1) (the row sums of the lane's exclusive
// suffix).  Frame g gives gamma_g, and with a_{g-1} -- the lane's own, or (v0, v1) = a_{lo-1} of its prefix -- the pair
// marginals xi_{g-1}(i, j) ~ a_{g-1}(i) A[i][j] l_g(j) beta_g(j).  acc[0..3] += E n01, E n0, E n10, E n1;
// acc[5] = gamma_0(1) in the lane that owns frame 0.
TQ_HD void tq_smooth_backward(const TqSmoothModel& m, const float* pr, int lo, int hi, double b0, double b1, double v0,
                              double v1, const double* filt, double* gam, double* acc) {
  if (lo >= hi) return;
  double c0 = gam[hi - 1], c1 = filt[hi - 1];  // a_g
  for (int g = hi - 1; g >= lo; --g) {
    const double r0 = c0 * b0, r1 = c1 * b1;
    const double g1 = r1 / (r0 + r1);
    if (g == 0) {
      gam[0] = g1;
      acc[5] = g1;
      break;
    }
    const double p0 = g > lo ? gam[g - 1] : v0, p1 = g > lo ? filt[g - 1] : v1;  // a_{g-1}
    gam[g] = g1;
    double l0, l1;
    tq_smooth_evidence(m, pr[g], l0, l1);
    const double w0 = l0 * b0, w1 = l1 * b1;
    const double x00 = p0 * m.a00 * w0, x01 = p0 * m.a01 * w1, x10 = p1 * m.a10 * w0, x11 = p1 * m.a11 * w1;
    const double r = 1.0 / ((x00 + x01) + (x10 + x11));
    acc[0] += x01 * r;
    acc[1] += (x00 + x01) * r;
    acc[2] += x10 * r;
    acc[3] += (x10 + x11) * r;
    // beta_{g-1} = A (l_g o beta_g), scaled by a power of two
    b0 = m.a00 * w0 + m.a01 * w1;
    b1 = m.a10 * w0 + m.a11 * w1;
    int e;
    (void)frexp(b0 + b1, &e);
    b0 = ldexp(b0, -e);
    b1 = ldexp(b1, -e);
    c0 = p0;
    c1 = p1;
  }
}

// ---- M-step -----------------------------------------------------------------------------------------------------------
// sums[0..6) over the N rows -> theta, clamped; a 0 / 0 quotient (no expected frame in that state) keeps the old value
TQ_HD void tq_smooth_mstep_theta(const double* sums, int N, double* theta) {
  if (sums[1] > 0.0) theta[0] = tq_smooth_clamp(sums[0] / sums[1], TQ_SMOOTH_RMIN);
  if (sums[3] > 0.0) theta[1] = tq_smooth_clamp(sums[2] / sums[3], TQ_SMOOTH_RMIN);
  theta[2] = tq_smooth_clamp(sums[5] / (double)N, TQ_SMOOTH_RMIN);
}

// ---- Viterbi ----------------------------------------------------------------------------------------------------------
// One row, sequential in f.  The scores are kept relative to state 0's (d = delta(1) - delta(0)), so their size does not
// grow with F.  Back-pointers: bit 2 (f & 15) + j of word back[(f >> 4) * stride] is the best predecessor of state j at
// frame f >= 1; a tie takes state 0.
TQ_HD void tq_smooth_viterbi_row(const TqSmoothModel& m, const float* pr, int F, uint32_t* back, int64_t stride,
                                 uint8_t* path) {
  const double la00 = log(m.a00), la01 = log(m.a01), la10 = log(m.a10), la11 = log(m.a11);
  double l0, l1;
  tq_smooth_evidence(m, pr[0], l0, l1);
  double d = (log(m.rho1) + log(l1)) - (log(m.rho0) + log(l0));
  uint32_t word = 0;
  for (int f = 1; f < F; ++f) {
    tq_smooth_evidence(m, pr[f], l0, l1);
    const double to0_from1 = d + la10, to1_from1 = d + la11;
    const uint32_t bp0 = to0_from1 > la00 ? 1u : 0u, bp1 = to1_from1 > la01 ? 1u : 0u;
    const double s0 = (bp0 ? to0_from1 : la00) + log(l0), s1 = (bp1 ? to1_from1 : la01) + log(l1);
    d = s1 - s0;
    word |= (bp0 | (bp1 << 1)) << (2 * (f & 15));
    if ((f & 15) == 15 || f == F - 1) {
      back[(int64_t)(f >> 4) * stride] = word;
      word = 0;
    }
  }
  uint32_t z = d > 0.0 ? 1u : 0u;
  path[F - 1] = (uint8_t)z;
  for (int f = F - 1; f >= 1; --f) {
    if ((f & 15) == 15 || f == F - 1) word = back[(int64_t)(f >> 4) * stride];
    z = (word >> (2 * (f & 15) + z)) & 1u;
    path[f - 1] = (uint8_t)z;
  }
}

// ---- backward sampler -------------------------------------------------------------------------------------------------
// q_f(j) = p(z_f = 1 | z_{f+1} = j, frames <= f) from filt[f]; the last frame has no successor: both are filt[F-1]
TQ_HD void tq_smooth_thresholds(const TqSmoothModel& m, double f1, bool last, double& q0, double& q1) {
  if (last) {
    q0 = q1 = f1;
    return;
  }
  const double f0 = 1.0 - f1;
  q0 = f1 * m.a10 / (f1 * m.a10 + f0 * m.a00);
  q1 = f1 * m.a11 / (f1 * m.a11 + f0 * m.a01);
}

TQ_HD void tq_smooth_stream(TqPhilox* ph, uint64_t seed, int s, int n) {
  tq_philox_init(ph, seed, (uint32_t)s, TQ_SMOOTH_SITE, (uint64_t)n);
}
TQ_HD int tq_smooth_label(TqPhilox* ph, double q) { return (double)tq_uniform(ph) < q ? 1 : 0; }

// The row counter of TqRatesRow for a row that is walked from its last frame to its first: it holds the label of the
// frame after the current one.  tq_rates_finish writes its counts.
TQ_HD void tq_smooth_back_begin(TqRatesRow& r, int z) {  // z of frame F - 1
  r.prev = z;
  r.n01 = r.n10 = r.n1 = 0;
}
// frame f <= F - 2 with label z: closes the pair (f, f + 1)
TQ_HD void tq_smooth_back_step(TqRatesRow& r, int z) {
  r.n1 += z;
  r.n01 += (1 - z) & r.prev;
  r.n10 += z & (1 - r.prev);
  r.prev = z;
}

// ---- backward interval walker -----------------------------------------------------------------------------------------
// The mirror of TqDwellWalk (tq_dwell.h) for a row that is visited from frame F - 1 down to 0: the open run is known by
// its last frame.  The run open at F - 1 is the last run of the record, the one still open after frame 0 the first;
// low_or_high is tq_dwell_code's.  Runs close in descending order of start_frame.
struct TqSmoothWalk {
  int cur, stop, last;
};

TQ_HD void tq_smooth_walk_begin(TqSmoothWalk& w, int F, int z) {  // z of frame F - 1
  w.cur = z;
  w.stop = F - 1;
  w.last = 1;
}

// frame f <= F - 2 with label z: returns 1 and fills `out` when it closes the run that began at f + 1
TQ_HD int tq_smooth_walk_step(TqSmoothWalk& w, int f, int z, TqDwellInterval& out) {
  if (z == w.cur) return 0;
  out.start = f + 1;
  out.stop = w.stop;
  out.z = w.cur;
  out.low_or_high = tq_dwell_code(w.cur, 0, w.last);
  w.cur = z;
  w.stop = f;
  w.last = 0;
  return 1;
}

// the run still open after frame 0 (F = 1: the only run, first and last)
TQ_HD void tq_smooth_walk_finish(const TqSmoothWalk& w, TqDwellInterval& out) {
  out.start = 0;
  out.stop = w.stop;
  out.z = w.cur;
  out.low_or_high = tq_dwell_code(w.cur, 1, w.last);
}

// Position in the interval table of the k-th run that row (s, n) closes (k = 0 is its last run): the table is ascending in
// start_frame within a row, so the run goes to o + count - 1 - k, o the row's offset.  -1 for a position outside
// [o, min(o + count, total)): a caller whose offsets or counts disagree with the draws gets a short table, never a stray
// write.
TQ_HD int64_t tq_smooth_emit_slot(int64_t o, int count, int k, int64_t total) {
  const int64_t pos = o + count - 1 - k;
  const int64_t end = o + count < total ? o + count : total;
  return o >= 0 && pos >= o && pos < end ? pos : -1;
}

// one row of the table (TQ_DWELL_COLS, total): the columns of tq_dwell_sample's EMIT
TQ_HD void tq_smooth_emit_row(int32_t* intervals, int64_t total, int64_t pos, int s, int n, const TqDwellInterval& v) {
  int32_t* col = intervals + pos;
  col[0] = s;
  col[total] = n;
  col[2 * total] = v.start;
  col[3 * total] = v.stop;
  col[4 * total] = v.stop + 1 - v.start;
  col[5 * total] = v.low_or_high;
  col[6 * total] = v.z;
}
