// tq_quantile.h -- quantile functions of the Gamma and Beta laws in double (host+device inline bodies): the credible
// intervals of the per-unit variational posteriors (tapqir/models/cosmos.py:740-776, where the reference calls
// torch_to_scipy_dist(...).interval element by element on the host).
// The __global__ wrapper is in tq_quantile.hip; tests/hostcheck/quantile_check.cpp runs the same bodies in host loops.
//
// Layers
//   * tq_binet_d, tq_log1pmx: the two pieces that keep every prefactor free of cancellation.  With the Binet function
//     S(a) = lgamma(a) - [(a - 1/2) ln a - a + ln sqrt(2 pi)]
//       y^a e^-y / Gamma(a)        = sqrt(a / 2 pi) exp(a [ln r - (r - 1)] - S(a)),                     r = y / a
//       x^a (1-x)^b / B(a, b)      = sqrt(a b / (2 pi (a+b))) exp(a [ln r1 - (r1-1)] + b [ln r2 - (r2-1)] + S(a+b) - S(a) - S(b)),
//                                    r1 = x (a+b) / a, r2 = (1-x) (a+b) / b
//     so that no term grows with the concentration (lgamma(1e6) ~ 1e7 would cost seven digits).
//   * tq_igamma: P(a, y), Q(a, y).   a < 64: power series of P for y <= max(1, a), Lentz continued fraction of Q beyond;
//                                    a >= 64: 24-point Gauss-Legendre quadrature of the tail that y cuts off the mode.
//   * tq_ibeta:  I_x(a, b) and its complement.  min(a, b) < 64: Lentz continued fraction on the side of the mean that
//                                    holds x (symmetry I_x(a, b) = 1 - I_{1-x}(b, a)); else the same quadrature.
//     Each returns the tail it computed directly and the other one as its complement: the directly computed tail is
//     the one that x cuts off, i.e. the small one, so a small tail is never formed as 1 - (something near 1).  (The
//     one exception is stated at tq_igamma: a < 1 and y < 1, where both tails exceed 0.2 a.)
//   * tq_tail_root: safeguarded Newton on ln tail(x) against u = ln x inside a bracket that every evaluation shrinks;
//     bisection of the bracket whenever Newton leaves it or fails to halve the step.
//   * tq_gamma_quantile, tq_beta_quantile, tq_body_interval.
// Every loop has a fixed cap (TQ_Q_*_CAP) and is left on the cap whatever the input; out-of-domain parameters give NaN.
#pragma once
#include "../../include/tapqir_hip.h"
#include "tq_math.h"

#define TQ_Q_BIG 64.0         // concentration at which the quadrature takes over from series / continued fraction
#define TQ_Q_SERIES_CAP 400   // power series of P(a, y), a < 64, y <= max(1, a): at most 53 terms on the test grid
#define TQ_Q_CF_CAP 4000      // continued fractions: at most 85 (Gamma) / 58 (Beta) steps on the test grid
#define TQ_Q_ROOT_CAP 128     // root search: bisection alone empties the bracket [-745, 709] in 62 halvings
#define TQ_Q_EPS 4.5e-16      // two ulps: the convergence tests compare against 1
#define TQ_Q_FPMIN 1e-300
#define TQ_Q_ULO (-745.0)     // ln of the smallest positive double
#define TQ_Q_UHI 709.0

TQ_HD double tq_qnan() { return __builtin_nan(""); }
TQ_HD bool tq_qfinite(double v) { return v - v == 0.0; }

// Binet function S(a), a > 0: asymptotic series for a >= 12 (next term 691 / (360360 a^13) < 2e-17), below that the
// shift a -> a + n >= 12 through lgamma(a) = lgamma(a + n) - ln prod_{i<n}(a + i)
TQ_HD double tq_binet_d(double a) {
  double prod = 1.0, b = a;
  for (int it = 0; it < 12 && b < 12.0; ++it) {
    prod *= b;
    b += 1.0;
  }
  const double rb = 1.0 / b, r2 = rb * rb;
  double S = rb * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0)))));
  if (b != a) S += (b - 0.5) * log(b) - (b - a) - log(prod) - (a - 0.5) * log(a);
  return S;
}

// ln r - (r - 1) given r and u = r - 1 (the caller forms u without cancellation); alternating series below 1/16
TQ_HD double tq_log1pmx(double u, double r) {
  if (fabs(u) < 0.0625) {
    double s = -1.0 / 18.0;
#pragma unroll
    for (int k = 17; k >= 2; --k) s = ((k & 1) ? 1.0 : -1.0) / (double)k + u * s;
    return u * u * s;
  }
  return log(r) - u;
}

// 24-point Gauss-Legendre rule on [-1, 1] (positive half; the rule is symmetric)
#define TQ_GL_HALF 12
#define TQ_GL_NODES                                                                                                   \
  {0.06405689286260563, 0.19111886747361631, 0.3150426796961634, 0.43379350762604513, 0.54542147138883956,            \
   0.64809365193697555, 0.74012419157855436, 0.82000198597390295, 0.88641552700440096, 0.9382745520027328,            \
   0.97472855597130947, 0.99518721999702131}
#define TQ_GL_WEIGHTS                                                                                                 \
  {0.12793819534675221, 0.1258374563468283, 0.12167047292780342, 0.11550566805372561, 0.10744427011596561,            \
   0.097618652104114065, 0.086190161531953288, 0.073346481411080411, 0.059298584915436742, 0.044277438817419551,      \
   0.028531388628933743, 0.012341229799987091}

// ---- regularised incomplete gamma --------------------------------------------------------------------------------
// D = y^a e^-y / Gamma(a) = y * pdf(y)
TQ_HD double tq_gamma_D(double a, double Sa, double y) {
  return sqrt(a * 0.15915494309189534) * exp(a * tq_log1pmx((y - a) / a, y / a) - Sa);
}

// a >= 64: the tail on the side of the mode a1 = a - 1 that holds y, integrand t^a1 e^-t / Gamma(a) =
// exp(a1 [ln(t/a1) - (t/a1 - 1)] - S(a1)) / sqrt(2 pi a1), over [y - 5 s, y] (not below a1 - 7.5 s) or
// [y, y + 6 (s + 2)] (not short of a1 + 8 (s + 2)), s = sqrt(a1): what lies beyond is < 1e-11 of the tail.
TQ_HD double tq_gamma_tail_quad(double a, double y, bool* lower) {
  constexpr double gx[TQ_GL_HALF] = TQ_GL_NODES, gw[TQ_GL_HALF] = TQ_GL_WEIGHTS;
  const double a1 = a - 1.0, s = sqrt(a1), ra1 = 1.0 / a1;
  *lower = y < a1;
  const double end = *lower ? fmax(0.0, fmin(a1 - 7.5 * s, y - 5.0 * s)) : fmax(a1 + 8.0 * (s + 2.0), y + 6.0 * (s + 2.0));
  const double half = 0.5 * (end - y), mid = (y - a1) + half;  // t - a1 = mid + half * node
  double sum = 0.0;
  for (int j = 0; j < TQ_GL_HALF; ++j) {
    const double d0 = mid - half * gx[j], d1 = mid + half * gx[j];
    sum += gw[j] * (exp(a1 * tq_log1pmx(d0 * ra1, (d0 + a1) * ra1)) + exp(a1 * tq_log1pmx(d1 * ra1, (d1 + a1) * ra1)));
  }
  return fabs(half) * sum * exp(-tq_binet_d(a1)) * sqrt(0.15915494309189534 * ra1);
}

// P(a, y), Q(a, y) and D for a > 0 finite, y >= 0 finite; Sa = tq_binet_d(a).
// a < 64: the series is taken for y <= max(1, a).  There Q is the complement of the series; it is smallest at a -> 0,
// y = 1, where Q(a, 1) = 0.22 a and P(a, y) >= 0.78 for all y in the model's range of p -- never a tail below 2e-3
// with a >= 0.01.
TQ_HD void tq_igamma(double a, double Sa, double y, double* P, double* Q, double* D) {
  if (!(y > 0.0)) {
    *P = 0.0, *Q = 1.0, *D = 0.0;
    return;
  }
  *D = tq_gamma_D(a, Sa, y);
  double tail;
  bool lower;
  if (a >= TQ_Q_BIG) {
    tail = tq_gamma_tail_quad(a, y, &lower);
  } else if (y > 1.0 && y > a) {  // modified Lentz on Q = D / (y + 1 - a - 1 (1 - a) / (y + 3 - a - ...))
    lower = false;
    double b = y + 1.0 - a, c = 1.0 / TQ_Q_FPMIN, d = 1.0 / b, h = d;
    for (int i = 1; i <= TQ_Q_CF_CAP; ++i) {
      const double an = -(double)i * ((double)i - a);
      b += 2.0;
      d = an * d + b;
      if (fabs(d) < TQ_Q_FPMIN) d = TQ_Q_FPMIN;
      c = b + an / c;
      if (fabs(c) < TQ_Q_FPMIN) c = TQ_Q_FPMIN;
      d = 1.0 / d;
      const double del = d * c;
      h *= del;
      if (fabs(del - 1.0) <= TQ_Q_EPS) break;
    }
    tail = *D * h;
  } else {  // P = D / a * sum_n y^n / ((a + 1) ... (a + n))
    lower = true;
    double ap = a, term = 1.0, sum = 1.0;
    for (int i = 0; i < TQ_Q_SERIES_CAP; ++i) {
      ap += 1.0;
      term *= y / ap;
      sum += term;
      if (term <= sum * TQ_Q_EPS) break;
    }
    tail = *D * sum / a;
  }
  tail = fmin(fmax(tail, 0.0), 1.0);
  *P = lower ? tail : 1.0 - tail;
  *Q = lower ? 1.0 - tail : tail;
}

// ---- regularised incomplete beta ---------------------------------------------------------------------------------
// D = x^a xc^b / B(a, b) = x xc pdf(x), xc = 1 - x given by the caller; Sab = S(a + b) - S(a) - S(b)
TQ_HD double tq_beta_D(double a, double b, double Sab, double x, double xc) {
  const double n = a + b, mu = a / n, muc = b / n;
  const double d = x < xc ? x - mu : muc - xc;
  return sqrt(a * b / n * 0.15915494309189534) *
         exp(a * tq_log1pmx(d / mu, x / mu) + b * tq_log1pmx(-d / muc, xc / muc) + Sab);
}

// Lentz evaluation of the continued fraction of I_x(a, b) a B(a, b) / (x^a (1-x)^b), x < (a + 1) / (a + b + 2)
TQ_HD double tq_beta_cf(double a, double b, double x) {
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < TQ_Q_FPMIN) d = TQ_Q_FPMIN;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= TQ_Q_CF_CAP; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < TQ_Q_FPMIN) d = TQ_Q_FPMIN;
    c = 1.0 + aa / c;
    if (fabs(c) < TQ_Q_FPMIN) c = TQ_Q_FPMIN;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < TQ_Q_FPMIN) d = TQ_Q_FPMIN;
    c = 1.0 + aa / c;
    if (fabs(c) < TQ_Q_FPMIN) c = TQ_Q_FPMIN;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= TQ_Q_EPS) break;
  }
  return h;
}

// a, b >= 64: the tail on the side of the mode m = a1 / (a1 + b1) (a1 = a - 1, b1 = b - 1) that holds x, integrand
// t^a1 (1-t)^b1 / B(a, b) = (n + 1) sqrt(n / (2 pi a1 b1)) exp(a1 [..] + b1 [..] + S(n) - S(a1) - S(b1)), n = a1 + b1,
// over 6 k s from x (not short of 8 k s from the mode), s the standard deviation, k = 1 + 2 / sqrt(min(a1, b1))
TQ_HD double tq_beta_tail_quad(double a, double b, double x, double xc, bool* lower) {
  constexpr double gx[TQ_GL_HALF] = TQ_GL_NODES, gw[TQ_GL_HALF] = TQ_GL_WEIGHTS;
  const double a1 = a - 1.0, b1 = b - 1.0, n = a1 + b1, m = a1 / n, mc = b1 / n;
  const double ks = sqrt(a1 * b1 / (n * n * (n + 1.0))) * (1.0 + 2.0 / sqrt(fmin(a1, b1)));
  const double dx = x < xc ? x - m : mc - xc;  // x - m
  *lower = dx < 0.0;
  // the far end as an offset from x, kept inside [0, 1]
  const double len = *lower ? -fmin(x, fmax(dx + 8.0 * ks, 6.0 * ks)) : fmin(xc, fmax(8.0 * ks - dx, 6.0 * ks));
  const double half = 0.5 * len, rm = 1.0 / m, rmc = 1.0 / mc;
  double sum = 0.0;
  for (int j = 0; j < TQ_GL_HALF; ++j) {
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const double off = half + (double)sgn * half * gx[j];  // t - x
      const double d = dx + off;                             // t - m
      sum += gw[j] * exp(a1 * tq_log1pmx(d * rm, (x + off) * rm) + b1 * tq_log1pmx(-d * rmc, (xc - off) * rmc));
    }
  }
  return fabs(half) * sum * (n + 1.0) * sqrt(0.15915494309189534 * n / (a1 * b1)) *
         exp(tq_binet_d(n) - tq_binet_d(a1) - tq_binet_d(b1));
}

// I_x(a, b) =: P, its complement Q = I_xc(b, a), and D, for a, b > 0 finite and x + xc = 1
TQ_HD void tq_ibeta(double a, double b, double Sab, double x, double xc, double* P, double* Q, double* D) {
  if (!(x > 0.0) || !(xc > 0.0)) {
    *P = x > 0.0 ? 1.0 : 0.0, *Q = 1.0 - *P, *D = 0.0;
    return;
  }
  *D = tq_beta_D(a, b, Sab, x, xc);
  double tail;
  bool lower;
  if (a >= TQ_Q_BIG && b >= TQ_Q_BIG) {
    tail = tq_beta_tail_quad(a, b, x, xc, &lower);
  } else {
    lower = x < (a + 1.0) / (a + b + 2.0);
    tail = lower ? *D * tq_beta_cf(a, b, x) / a : *D * tq_beta_cf(b, a, xc) / b;
  }
  tail = fmin(fmax(tail, 0.0), 1.0);
  *P = lower ? tail : 1.0 - tail;
  *Q = lower ? 1.0 - tail : tail;
}

// ---- root search ---------------------------------------------------------------------------------------------------
#define TQ_Q_GAMMA 0
#define TQ_Q_BETA 1

// u = ln x in [ulo, uhi] with tail(x) = p; tail = P (increasing in x) or, with `upper`, Q (decreasing).  Newton on
// ln tail against u (a power-law tail is a straight line there); each evaluation moves one end of the bracket to u, and
// the bracket is bisected when the Newton point leaves it, is not finite, or the step is more than half the previous
// one.  Stops after a Newton step below 1e-9 (quadratic convergence: the point it lands on is good to 1e-16), when the
// bracket is empty to rounding, or on the cap.
TQ_HD double tq_tail_root(int kind, double a, double b, double S, double p, bool upper, double u, double ulo, double uhi) {
  const double lnp = log(p);
  if (!(u > ulo && u < uhi)) u = 0.5 * (ulo + uhi);
  double dprev = uhi - ulo;
  for (int it = 0; it < TQ_Q_ROOT_CAP; ++it) {
    const double x = exp(u);
    double P, Q, D;
    if (kind == TQ_Q_GAMMA) {
      tq_igamma(a, S, x, &P, &Q, &D);
    } else {
      tq_ibeta(a, b, S, x, 1.0 - x, &P, &Q, &D);
      D /= 1.0 - x;
    }
    const double t = upper ? Q : P;
    if (!(t == t)) return tq_qnan();
    if (upper ? t > p : t < p) ulo = u;
    else uhi = u;
    if (!(uhi - ulo > 4e-16 * fmax(1.0, fabs(u)))) return 0.5 * (ulo + uhi);
    const double du = (lnp - log(t)) * t / (upper ? -D : D);
    const double un = u + du;
    if (fabs(du) < 1e-9) return fmin(fmax(un, ulo), uhi);  // (a step below the spacing of u lands on the bracket's end)
    if (tq_qfinite(du) && un > ulo && un < uhi && fabs(du) <= 0.5 * fabs(dprev)) {
      u = un;
      dprev = du;
    } else {
      const double mid = 0.5 * (ulo + uhi);
      dprev = mid - u;
      u = mid;
    }
  }
  return u;
}

// standard normal quantile of p <= 1/2 (Abramowitz & Stegun 26.2.23, |error| < 4.5e-4): starting points only
TQ_HD double tq_normal_start(double p) {
  const double t = sqrt(-2.0 * log(p));
  return -(t - (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308))));
}

// y with P(a, y) = p (upper: Q(a, y) = p), 0 < p <= 1/2, a > 0 finite.  Start: Wilson-Hilferty, or the power law
// P ~ y^a / Gamma(a + 1) where that has no positive cube root (small a).
TQ_HD double tq_gamma_quantile(double a, double p, bool upper) {
  const double Sa = tq_binet_d(a);
  const double z = upper ? -tq_normal_start(p) : tq_normal_start(p);
  const double c = 1.0 - 1.0 / (9.0 * a) + z / (3.0 * sqrt(a));
  double u0;
  if (a >= 1.0 && c > 0.05) {
    u0 = log(a) + 3.0 * log(c);
  } else if (!upper) {
    // ln Gamma(a + 1) = (a + 1/2) ln a - a + ln sqrt(2 pi) + S(a)
    u0 = (log(p) + (a + 0.5) * log(a) - a + 0.91893853320467274178 + Sa) / a;
  } else {
    u0 = c > 0.05 ? log(a) + 3.0 * log(c) : 0.0;
  }
  return exp(tq_tail_root(TQ_Q_GAMMA, a, 0.0, Sa, p, upper, u0, TQ_Q_ULO, TQ_Q_UHI));
}

// t in [0, 1] with I_t(a, b) = p (upper: 1 - I_t(a, b) = p), 0 < p <= 1/2, a, b > 0 finite.  The search runs in
// ln of whichever of t, 1 - t is below 1/2 (one evaluation at 1/2 decides), so that a quantile next to either end
// keeps its relative accuracy: by symmetry 1 - t has the law Beta(b, a) with the tails exchanged.
TQ_HD double tq_beta_quantile(double a, double b, double p, bool upper) {
  const double Sab = tq_binet_d(a + b) - tq_binet_d(a) - tq_binet_d(b);
  double P, Q, D;
  tq_ibeta(a, b, Sab, 0.5, 0.5, &P, &Q, &D);
  const bool left = upper ? Q <= p : P >= p;  // the quantile is in (0, 1/2]
  // starting point for t (Abramowitz & Stegun 26.5.22 for a, b > 1; the power laws at the ends otherwise)
  const double pl = upper ? 1.0 - p : p;  // lower-tail probability of t
  double t0;
  if (a > 1.0 && b > 1.0) {
    const double z = upper ? -tq_normal_start(p) : tq_normal_start(p);
    const double al = (z * z - 3.0) / 6.0, ra = 1.0 / (2.0 * a - 1.0), rb = 1.0 / (2.0 * b - 1.0);
    const double h = 2.0 / (ra + rb);
    const double w = -z * sqrt(al + h) / h - (rb - ra) * (al + 5.0 / 6.0 - 2.0 / (3.0 * h));
    t0 = a / (a + b * exp(2.0 * w));
  } else {
    const double ta = exp(a * log(a / (a + b))) / a, tb = exp(b * log(b / (a + b))) / b, w = ta + tb;
    t0 = pl < ta / w ? exp(log(a * w * pl) / a) : 1.0 - exp(log(b * w * (1.0 - pl)) / b);
  }
  const double u0 = log(left ? t0 : 1.0 - t0);
  const double uhi = -0.69314718055994530942;
  if (left) return exp(tq_tail_root(TQ_Q_BETA, a, b, Sab, p, upper, u0, TQ_Q_ULO, uhi));
  return 1.0 - exp(tq_tail_root(TQ_Q_BETA, b, a, Sab, p, !upper, u0, TQ_Q_ULO, uhi));
}

// ---- one element of tq_credible_intervals: p = (1 - CI) / 2 -------------------------------------------------------
// Gamma: concentration = the fp32 product loc * beta (as the host helper forms it before its upcast), rate = beta.
// AffineBeta: c1 = size (mean - low) / (high - low), c0 = size (high - mean) / (high - low) in double.
TQ_HD void tq_body_interval(const tq_interval_args& A, double p, int64_t i) {
  const float f0 = A.p0[i], f1 = A.p1[i];
  double ll = tq_qnan(), ul = tq_qnan();
  if (A.kind == TQ_INTERVAL_GAMMA) {
    const float af = f0 * f1;
    const double a = (double)af, rate = (double)f1;
    if (a > 0.0 && rate > 0.0 && tq_qfinite(a) && tq_qfinite(rate)) {
      ll = tq_gamma_quantile(a, p, false) / rate;
      ul = tq_gamma_quantile(a, p, true) / rate;
    }
  } else {
    const double mean = (double)f0, size = (double)f1, span = A.high - A.low;
    const double c1 = size * (mean - A.low) / span, c0 = size * (A.high - mean) / span;
    if (c1 > 0.0 && c0 > 0.0 && tq_qfinite(c1) && tq_qfinite(c0)) {
      ll = A.low + span * tq_beta_quantile(c1, c0, p, false);
      ul = A.low + span * tq_beta_quantile(c1, c0, p, true);
    }
  }
  A.ll[i] = ll;
  A.ul[i] = ul;
}
