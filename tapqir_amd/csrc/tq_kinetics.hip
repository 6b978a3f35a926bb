// tq_kinetics.hip -- time-to-first-binding kinetics on the device (bodies in tq_kinetics.h): the first-binding sampler
// (prefix + search) and the batched censored-mixture MLE, one wave per posterior sample.
#include <hip/hip_runtime.h>

#include "tq_fit.h"
#include "tq_host.h"
#include "tq_kinetics.h"

// ---- sampler, launch 1: log-survival prefix, one wave per AOI ---------------------------------------------------------
// The lanes form log1p(-p) of 64 frames at a time; lane 0 adds them up in frame order (the host build's order, so the
// sums are the same bits); the lanes store the prefix back coalesced.
__global__ __launch_bounds__(64) void tq_ttfb_prefix_kernel(const float* __restrict__ p, double* __restrict__ L, int F) {
  __shared__ double buf[64];
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* pr = p + (int64_t)n * F;
  double* Lr = L + (int64_t)n * F;
  double acc = 0.0;  // lane 0's running sum
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int f = f0 + lane;
    const int cnt = min(64, F - f0);
    buf[lane] = f < F ? tq_ttfb_log_surv_term(pr[f]) : 0.0;
    __syncthreads();
    if (lane == 0) {
      for (int j = 0; j < cnt; ++j) {
        acc += buf[j];
        buf[j] = acc;
      }
    }
    __syncthreads();
    if (f < F) Lr[f] = buf[lane];
    __syncthreads();
  }
}

// ---- sampler, launch 2: one lane per (s, n) ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tq_ttfb_search_kernel(const double* __restrict__ L, float* __restrict__ tau, int N,
                                                             int F, int64_t total, uint64_t seed) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int s = (int)(t / N), n = (int)(t - (int64_t)s * N);
  const double lu = tq_ttfb_log_uniform(seed, s, n);
  tau[t] = (float)tq_ttfb_search(L + (int64_t)n * F, F, lu);
}

extern "C" int tq_ttfb_sample(const tq_ttfb_sample_args* a, void* stream) {
  if (!a || !a->p || !a->log_surv || !a->tau) {
    tq_set_error("tq_ttfb_sample: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->F < 1 || a->S < 1) {
    tq_set_error("tq_ttfb_sample: N, F and S must be positive");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_ttfb_prefix_kernel, dim3((unsigned)a->N), dim3(64), 0, (hipStream_t)stream, a->p, a->log_surv,
                     a->F);
  int rc = tq_launch_status("tq_ttfb_prefix_kernel");
  if (rc != TQ_OK) return rc;
  const int64_t total = (int64_t)a->S * a->N;
  hipLaunchKernelGGL(tq_ttfb_search_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     a->log_surv, a->tau, a->N, a->F, total, a->seed);
  return tq_launch_status("tq_ttfb_search_kernel");
}

// ---- batched MLE: one wave (= one workgroup) per posterior sample -----------------------------------------------------
// double sum of a data constant over the wave, in every lane (xor butterfly); the steps' float sums are tq_fit_wave_sum
__device__ __forceinline__ double ttfb_data_sum(double v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// STAGED: the uncensored points of the row are compacted into LDS once per launch and every step reads them there;
// otherwise every step reads the row from global memory (L2) and skips the points outside (0, T).
template <bool STAGED>
__global__ __launch_bounds__(64) void tq_ttfb_fit_kernel(const tq_ttfb_fit_args a) {
  extern __shared__ float pts[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const float T = a.Tmax;
  const float* row = a.tau + (int64_t)s * a.N;

  // data constants (double partial sums: exact for integer data below 2^53)
  double n_int = 0.0, sum_tau = 0.0, n_cens = 0.0, nc_int = 0.0, sum_tauc = 0.0, nc_cens = 0.0;
  int n_staged = 0;  // wave-uniform
  for (int i0 = 0; i0 < a.N; i0 += 64) {
    const int i = i0 + lane;
    const float t = i < a.N ? row[i] : 0.0f;
    const bool inner = t > 0.0f && t < T;
    n_int += inner ? 1.0 : 0.0;
    sum_tau += inner ? (double)t : 0.0;
    n_cens += (i < a.N && t == T) ? 1.0 : 0.0;
    if (STAGED) {
      const uint64_t mask = __ballot(inner);
      const int below = __popcll(mask & ((1ull << lane) - 1ull));
      if (inner) pts[n_staged + below] = t;
      n_staged += __popcll(mask);
    }
  }
  if (a.tauc) {
    const float* crow = a.tauc + (int64_t)s * a.Nc;
    for (int i = lane; i < a.Nc; i += 64) {
      const float t = crow[i];
      const bool inner = t > 0.0f && t < T;
      nc_int += inner ? 1.0 : 0.0;
      sum_tauc += inner ? (double)t : 0.0;
      nc_cens += t == T ? 1.0 : 0.0;
    }
  }
  TqTtfbData d;
  d.n_int = (float)ttfb_data_sum(n_int);
  d.sum_tau = (float)ttfb_data_sum(sum_tau);
  d.n_cens = (float)ttfb_data_sum(n_cens);
  d.nc_int = (float)ttfb_data_sum(nc_int);
  d.sum_tauc = (float)ttfb_data_sum(sum_tauc);
  d.nc_cens = (float)ttfb_data_sum(nc_cens);
  d.T = T;
  if (STAGED) __syncthreads();

  const float* st = a.state + (int64_t)s * TQ_TTFB_STATE;
  float p[3] = {st[0], st[1], st[2]}, m[3] = {st[3], st[4], st[5]}, v[3] = {st[6], st[7], st[8]};
  const TqFitAdam adam(a.lr, a.beta1, a.beta2, a.eps);
  const int last = a.step0 + a.n_steps;
  for (int t = a.step0 + 1; t <= last; ++t) {
    const TqTtfbK k = tq_ttfb_consts(p[0], p[1], p[2]);
    float W1 = 0.0f, W1tau = 0.0f;
    if (STAGED) {
#pragma unroll 4
      for (int i = lane; i < n_staged; i += 64) tq_ttfb_accumulate(k, pts[i], W1, W1tau);
    } else {
#pragma unroll 4
      for (int i = lane; i < a.N; i += 64) {
        const float x = row[i];
        if (x > 0.0f && x < T) tq_ttfb_accumulate(k, x, W1, W1tau);
      }
    }
    W1 = tq_fit_wave_sum(W1);
    W1tau = tq_fit_wave_sum(W1tau);
    if (t == last && a.loss) {  // loss at the parameters this step starts from (what svi.step() returns)
      float SP = 0.0f;
      if (STAGED) {
        for (int i = lane; i < n_staged; i += 64) SP += tq_ttfb_softplus_d(k, pts[i]);
      } else {
        for (int i = lane; i < a.N; i += 64) {
          const float x = row[i];
          if (x > 0.0f && x < T) SP += tq_ttfb_softplus_d(k, x);
        }
      }
      SP = tq_fit_wave_sum(SP);
      if (lane == 0) a.loss[s] = tq_ttfb_loss(k, d, SP);
    }
    float g[3];
    tq_ttfb_grad(k, d, W1, W1tau, g);
    const float step_size = adam.step_size(t), bc2s = adam.bc2s(t);
#pragma unroll
    for (int j = 0; j < 3; ++j) tq_fit_adam(p[j], m[j], v[j], g[j], adam.w1, adam.b2, adam.w2, step_size, bc2s, adam.eps);
  }
  if (lane == 0) {
    float* out = a.state + (int64_t)s * TQ_TTFB_STATE;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      out[j] = p[j];
      out[3 + j] = m[j];
      out[6 + j] = v[j];
    }
  }
}

extern "C" int tq_ttfb_fit(const tq_ttfb_fit_args* a, void* stream) {
  if (!a || !a->tau || !a->state || (a->Nc > 0 && !a->tauc)) {
    tq_set_error("tq_ttfb_fit: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->S < 1 || a->N < 1 || a->Nc < 0 || (a->tauc && a->Nc < 1) || a->step0 < 0 || a->n_steps < 1 ||
      !(a->Tmax > 0.0f) || !tq_adam_settings_ok(a->lr, a->beta1, a->beta2, a->eps)) {
    tq_set_error("tq_ttfb_fit: unsupported S/N/Nc/step0/n_steps/Tmax or Adam settings");
    return TQ_ERR_ARG;
  }
  if (a->N > TQ_TTFB_LDS_POINTS || !a->stage_lds) {
    hipLaunchKernelGGL(tq_ttfb_fit_kernel<false>, dim3((unsigned)a->S), dim3(64), 0, (hipStream_t)stream, *a);
  } else {
    hipLaunchKernelGGL(tq_ttfb_fit_kernel<true>, dim3((unsigned)a->S), dim3(64), (size_t)a->N * sizeof(float),
                       (hipStream_t)stream, *a);
  }
  return tq_launch_status("tq_ttfb_fit_kernel");
}
