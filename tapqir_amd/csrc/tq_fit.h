// tq_fit.h -- what a per-sample Adam fit is made of, shared by the fit kernels of tq_kinetics.hip and tq_dwell.hip
// (host+device inline bodies): the exponential of an unconstrained rate, torch.optim.Adam on parameters held in registers
// and -- device only -- the wave sum of a step's sufficient statistics.  Each kernel keeps its own data pass and its own
// consts / accumulate / grad / loss.
#pragma once
#include "tq_math.h"
#if defined(__HIPCC__)
#include "tq_dpp.h"
#endif

// e^x of an unconstrained rate parameter.  TQ_FEXP on the device rounds x log2(e) to float before v_exp_f32: up to half an
// ulp of the exponent, |x| 2^-24 ln 2 relative in e^x (3e-7 at x = log 0.002, five float32 eps), and a gradient whose
// terms cancel (k sum tau against a count) magnifies it by the cancellation.  Here the part l of the product that the
// rounding lost goes back in as 2^h (1 + l ln 2), which leaves the instruction's own 1 ulp.  Once per step, not per point.
TQ_HD float tq_fit_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float h = x * TQ_LOG2E;
  const float l = fmaf(x, TQ_LOG2E, -h) + x * 1.92596299112661747e-08f;  // log2(e) - (float)log2(e)
  const float e = TQ_FEXP2(h);
  return fmaf(e, l * 0.69314718055994530942f, e);
#else
  return expf(x);
#endif
}

// torch.optim.Adam (betas, eps, bias correction; no weight decay / amsgrad) on one parameter, float32 as torch does it:
// m.lerp_(g, 1 - beta1); v = v beta2 + (1 - beta2) g^2; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
TQ_HD void tq_fit_adam(float& p, float& m, float& v, float g, float w1, float b2, float w2, float step_size, float bc2s,
                       float eps) {
  m = m + w1 * (g - m);
  v = v * b2 + (g * g) * w2;
  p = p - step_size * (m / (sqrtf(v) / bc2s + eps));
}

// beta^t by binary powering in double: the same bits for a given t however the steps are split over launches
TQ_HD double tq_fit_pow(double b, uint32_t t) {
  double r = 1.0;
  while (t) {
    if (t & 1u) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// the Adam settings of one launch, and the two bias-correction factors of optimiser step t (1-based, counted over all
// launches of the fit): double arithmetic, then one cast each
struct TqFitAdam {
  double lr, beta1, beta2;
  float w1, b2, w2, eps;

  TQ_HD TqFitAdam(double lr_, double beta1_, double beta2_, double eps_)
      : lr(lr_), beta1(beta1_), beta2(beta2_), w1((float)(1.0 - beta1_)), b2((float)beta2_), w2((float)(1.0 - beta2_)),
        eps((float)eps_) {}

  TQ_HD float step_size(int t) const { return (float)(lr / (1.0 - tq_fit_pow(beta1, (uint32_t)t))); }
  TQ_HD float bc2s(int t) const { return (float)sqrt(1.0 - tq_fit_pow(beta2, (uint32_t)t)); }
};

#if defined(__HIPCC__)
// sum over the wave (every lane active): an xor butterfly, so the same bits in every lane (each DPP / shuffle step adds a
// pair in either order), then made wave-uniform
__device__ __forceinline__ float tq_fit_wave_sum(float v) {
  v = tq_group_sum<64>(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// the same butterfly on 64-bit integers (exact in any order): the sum in every lane
__device__ __forceinline__ int64_t tq_fit_wave_sum(int64_t v) { return tq_group_sum<64>(v); }
#endif
