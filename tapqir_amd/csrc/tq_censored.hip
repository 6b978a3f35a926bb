// tq_censored.hip -- `dwelltime --censored` on the device (bodies in tq_censored.h): the histograms
// of the open last runs from the interval table, the batched K-exponential fit with right-censored pairs, one wave per
// row, and the product-limit survival curve of every row of histograms, one wave per row.
#include <hip/hip_runtime.h>

#include "tq_censored.h"
#include "tq_host.h"

// ---- open last runs: one lane per table row ---------------------------------------------------------------------------------
// A lane reads the code column first; only a row with code 2 / 3 (the run that closes the record, z = 0 / 1) that opened
// inside the record reads the other columns and adds 1 at [s, g, dwell_time].  Integer atomics: order-free, so
// deterministic.  A row whose sample, AOI, dwell time or population is out of range adds nothing, never a stray write.
__global__ __launch_bounds__(256) void tq_dwell_censored_hist_kernel(const tq_dwell_censored_hist_args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = a.total;
  if (i >= total) return;
  const int32_t* col = a.intervals + i;
  const int code = col[5 * total];
  if (code != 2 && code != 3) return;
  if (col[2 * total] <= 0) return;  // a first run: its start was not observed
  const int s = col[0], n = col[total], d = col[4 * total];
  if (s < 0 || s >= a.S || n < 0 || n >= a.N || d < 0 || d >= a.F) return;
  const int g = a.pop ? (int)a.pop[(int64_t)s * a.N + n] : 0;
  if (g >= a.G) return;
  atomicAdd((code == 3 ? a.cens_bound : a.cens_unbound) + ((int64_t)s * a.G + g) * a.F + d, 1);
}

extern "C" int tq_dwell_censored_hist(const tq_dwell_censored_hist_args* a, void* stream) {
  if (!a || !a->cens_bound || !a->cens_unbound || (a->total > 0 && !a->intervals)) {
    tq_set_error("tq_dwell_censored_hist: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->S < 1 || a->N < 1 || a->F < 1 || a->total < 0) {
    tq_set_error("tq_dwell_censored_hist: S, N and F must be positive (and total >= 0)");
    return TQ_ERR_ARG;
  }
  if (a->G < 1 || a->G > 4 || (!a->pop && a->G != 1)) {
    tq_set_error("tq_dwell_censored_hist: G must be in 1 .. 4, and 1 without pop");
    return TQ_ERR_ARG;
  }
  const int64_t blocks = (a->total + 255) / 256;
  if (blocks > 2147483647LL) {
    tq_set_error("tq_dwell_censored_hist: total too large");
    return TQ_ERR_ARG;
  }
  if (a->total == 0) return TQ_OK;
  hipLaunchKernelGGL(tq_dwell_censored_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_dwell_censored_hist_kernel");
}

// ---- batched MLE with censored pairs: one wave (= one workgroup) per row ------------------------------------------------
// tq_dwell_fit_kernel with a second list of pairs per row.  A row whose complete and censored pairs together are at most
// TQ_DWELL_LDS_PAIRS is staged in LDS once per launch (when stage_lds), the complete pairs first; otherwise both parts are
// read from global memory (L2) every step.
template <int K>
__global__ __launch_bounds__(64) void tq_dwell_censored_fit_kernel(const tq_dwell_censored_fit_args a) {
  extern __shared__ float2 pairs[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int64_t r0 = a.row_ptr[s], c0 = a.crow_ptr[s];
  const int len = (int)(a.row_ptr[s + 1] - r0), clen = (int)(a.crow_ptr[s + 1] - c0);
  const float* vals = a.values + r0;
  const float* wts = a.weights + r0;
  const float* cvals = a.cvalues + c0;
  const float* cwts = a.cweights + c0;
  const bool staged = a.stage_lds && (int64_t)len + clen <= TQ_DWELL_LDS_PAIRS;  // wave-uniform
  float2* cpairs = pairs + len;
  float n = 0.0f, nc = 0.0f;
  for (int i = lane; i < len; i += 64) {
    const float t = vals[i], wt = wts[i];
    n += wt;
    if (staged) pairs[i] = make_float2(t, wt);
  }
  for (int i = lane; i < clen; i += 64) {
    const float t = cvals[i], wt = cwts[i];
    nc += wt;
    if (staged) cpairs[i] = make_float2(t, wt);
  }
  n = tq_fit_wave_sum(n);
  nc = tq_fit_wave_sum(nc);
  __syncthreads();

  constexpr int P = 2 * K;
  const float* st = a.state + (int64_t)s * 3 * P;
  float p[P], m[P], v[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    p[j] = st[j];
    m[j] = st[P + j];
    v[j] = st[2 * P + j];
  }
  const TqFitAdam adam(a.lr, a.beta1, a.beta2, a.eps);
  const int last = a.step0 + a.n_steps;
  for (int t = a.step0 + 1; t <= last; ++t) {
    const TqDwellK<K> q = tq_dwell_consts<K>(p);
    const TqDwellK<K> qc = tq_censored_consts<K>(q, p);
    float R[K], RT[K], Rc[K], RTc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) R[j] = RT[j] = Rc[j] = RTc[j] = 0.0f;
    if (staged) {
#pragma unroll 2
      for (int i = lane; i < len; i += 64) {
        const float2 x = pairs[i];
        tq_dwell_accumulate<K>(q, x.x, x.y, R, RT);
      }
#pragma unroll 2
      for (int i = lane; i < clen; i += 64) {
        const float2 x = cpairs[i];
        tq_dwell_accumulate<K>(qc, x.x, x.y, Rc, RTc);
      }
    } else {
#pragma unroll 2
      for (int i = lane; i < len; i += 64) tq_dwell_accumulate<K>(q, vals[i], wts[i], R, RT);
#pragma unroll 2
      for (int i = lane; i < clen; i += 64) tq_dwell_accumulate<K>(qc, cvals[i], cwts[i], Rc, RTc);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      R[j] = tq_fit_wave_sum(R[j]);
      RT[j] = tq_fit_wave_sum(RT[j]);
      Rc[j] = tq_fit_wave_sum(Rc[j]);
      RTc[j] = tq_fit_wave_sum(RTc[j]);
    }
    if (t == last && a.loss) {  // loss at the parameters this step starts from (what svi.step() returns)
      float ll = 0.0f, llc = 0.0f, r[K];
      for (int i = lane; i < len; i += 64) {
        const float2 x = staged ? pairs[i] : make_float2(vals[i], wts[i]);
        ll = fmaf(x.y, tq_dwell_resp<K>(q, x.x, r, true), ll);
      }
      for (int i = lane; i < clen; i += 64) {
        const float2 x = staged ? cpairs[i] : make_float2(cvals[i], cwts[i]);
        llc = fmaf(x.y, tq_dwell_resp<K>(qc, x.x, r, true), llc);
      }
      ll = tq_fit_wave_sum(ll);
      llc = tq_fit_wave_sum(llc);
      if (lane == 0) a.loss[s] = -(ll + llc);
    }
    float g[P];
    tq_censored_grad<K>(q, R, RT, n, Rc, RTc, nc, g);
    const float step_size = adam.step_size(t), bc2s = adam.bc2s(t);
#pragma unroll
    for (int j = 0; j < P; ++j) tq_fit_adam(p[j], m[j], v[j], g[j], adam.w1, adam.b2, adam.w2, step_size, bc2s, adam.eps);
  }
  if (lane == 0) {
    float* out = a.state + (int64_t)s * 3 * P;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      out[j] = p[j];
      out[P + j] = m[j];
      out[2 * P + j] = v[j];
    }
  }
}

template <int K>
static void censored_fit_launch(const tq_dwell_censored_fit_args* a, hipStream_t stream) {
  const size_t lds = a->stage_lds ? (size_t)TQ_DWELL_LDS_PAIRS * sizeof(float2) : 0;
  hipLaunchKernelGGL(tq_dwell_censored_fit_kernel<K>, dim3((unsigned)a->S), dim3(64), lds, stream, *a);
}

extern "C" int tq_dwell_censored_fit(const tq_dwell_censored_fit_args* a, void* stream) {
  if (!a || !a->values || !a->weights || !a->row_ptr || !a->cvalues || !a->cweights || !a->crow_ptr || !a->state) {
    tq_set_error("tq_dwell_censored_fit: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->K < 1 || a->K > TQ_DWELL_KMAX) {
    tq_set_error("tq_dwell_censored_fit: K must be in 1 .. TQ_DWELL_KMAX");
    return TQ_ERR_ARG;
  }
  if (a->S < 1 || a->step0 < 0 || a->n_steps < 1 || !tq_adam_settings_ok(a->lr, a->beta1, a->beta2, a->eps)) {
    tq_set_error("tq_dwell_censored_fit: unsupported S/step0/n_steps or Adam settings");
    return TQ_ERR_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;
  switch (a->K) {
    case 1: censored_fit_launch<1>(a, st); break;
    case 2: censored_fit_launch<2>(a, st); break;
    case 3: censored_fit_launch<3>(a, st); break;
    case 4: censored_fit_launch<4>(a, st); break;
    case 5: censored_fit_launch<5>(a, st); break;
    case 6: censored_fit_launch<6>(a, st); break;
    case 7: censored_fit_launch<7>(a, st); break;
    default: censored_fit_launch<8>(a, st); break;
  }
  return tq_launch_status("tq_dwell_censored_fit_kernel");
}

// ---- product-limit survival: one wave (= one workgroup) per row --------------------------------------------------------
// A reduction for the number of runs at risk at u = 1, then one forward pass in chunks of 64 bins, a bin per lane: the
// inclusive scan of h_d + c_d gives every lane its Y_u, the inclusive scan of the factors its product; the last lane's
// two values carry into the next chunk.  Hillis-Steele over the wave, six steps each, no scratch buffer.
__global__ __launch_bounds__(64) void tq_dwell_survival_kernel(const tq_dwell_survival_args a) {
  const int lane = threadIdx.x, F = a.F;
  const int32_t* h = a.hist + (int64_t)blockIdx.x * F;
  const int32_t* c = a.cens + (int64_t)blockIdx.x * F;
  double* surv = a.surv + (int64_t)blockIdx.x * F;
  int64_t total = 0;
  for (int f = lane; f < F; f += 64) total += tq_survival_h(h, f) + tq_survival_c(c, f);
  total = tq_fit_wave_sum(total);
  long long gone = 0;  // sum_{d < f0} h_d + c_d
  double prod = 1.0;
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int f = f0 + lane;
    const long long hv = f < F ? tq_survival_h(h, f) : 0;
    long long d = hv + (f < F ? tq_survival_c(c, f) : 0);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(d, o, 64);
      if (lane >= o) d += up;
    }
    double x = tq_survival_factor(total - (gone + d - hv), hv);  // a lane past F: h = 0, a factor of 1
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(x, o, 64);
      if (lane >= o) x *= up;
    }
    x *= prod;
    if (f < F) surv[f] = x;
    gone += __shfl(d, 63, 64);
    prod = __shfl(x, 63, 64);
  }
}

extern "C" int tq_dwell_survival(const tq_dwell_survival_args* a, void* stream) {
  if (!a || !a->hist || !a->cens || !a->surv) {
    tq_set_error("tq_dwell_survival: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->R < 1 || a->F < 1 || a->F > TQ_SMOOTH_MAX_F) {
    tq_set_error("tq_dwell_survival: R and F must be positive and F at most " TQ_STR(TQ_SMOOTH_MAX_F));
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_dwell_survival_kernel, dim3((unsigned)a->R), dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_dwell_survival_kernel");
}
