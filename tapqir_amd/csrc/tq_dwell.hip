// tq_dwell.hip -- dwell-time kinetics on the device (bodies in tq_dwell.h): the raster sampler / interval walker (count and
// emit launches) and the batched K-exponential mixture MLE, one wave per posterior sample.
#include <hip/hip_runtime.h>

#include "tq_dwell.h"
#include "tq_host.h"

// ---- sampler: one wave per (AOI n, block of 64 samples), one lane per sample ---------------------------------------------
// Every lane draws its own row (s, n) frame by frame and walks it in registers; the row of p is staged 64 frames at a time
// in LDS and read there as a broadcast.  EMIT = false: per-row interval counts and the interior-run histograms (integer
// atomics: order-free, so deterministic); EMIT = true: the same draws again, each interval written at the row's offset.
template <bool EMIT>
__global__ __launch_bounds__(64) void tq_dwell_sample_kernel(const tq_dwell_sample_args a) {
  __shared__ float pbuf[64];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s = blockIdx.y * 64 + lane;
  const bool active = s < a.S;
  const int F = a.F;
  const float* pr = a.p + (int64_t)n * F;
  const int64_t row = (int64_t)s * a.N + n;
  int32_t* hb = EMIT ? nullptr : a.hist_bound + (int64_t)s * F;
  int32_t* hu = EMIT ? nullptr : a.hist_unbound + (int64_t)s * F;
  int64_t o = 0;
  if (EMIT && active) o = a.offsets[row];
  const int64_t total = a.total;

  TqPhilox ph;
  tq_dwell_stream(&ph, a.seed, s, n);
  TqDwellWalk w;
  TqDwellInterval iv;
  int count = 0;

  auto emit = [&](const TqDwellInterval& v) {
    if (EMIT) {
      if (o < total) {  // a caller whose offsets disagree with the draws gets a short table, never a stray write
        int32_t* col = a.intervals + o;
        col[0] = s;
        col[total] = n;
        col[2 * total] = v.start;
        col[3 * total] = v.stop;
        col[4 * total] = v.stop + 1 - v.start;
        col[5 * total] = v.low_or_high;
        col[6 * total] = v.z;
      }
      ++o;
    } else {
      ++count;
      if (v.low_or_high == 0 || v.low_or_high == 1) atomicAdd((v.z ? hb : hu) + (v.stop + 1 - v.start), 1);
    }
  };

  for (int f0 = 0; f0 < F; f0 += 64) {
    const int cnt = min(64, F - f0);
    if (lane < cnt) pbuf[lane] = pr[f0 + lane];
    __syncthreads();
    if (active) {
      for (int j = 0; j < cnt; ++j) {
        const int f = f0 + j;
        const int z = tq_dwell_label(&ph, pbuf[j]);
        if (f == 0) tq_dwell_begin(w, z);
        else if (tq_dwell_step(w, f, z, iv)) emit(iv);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  tq_dwell_finish(w, F, iv);
  emit(iv);
  if (!EMIT) a.counts[row] = count;
}

extern "C" int tq_dwell_sample(const tq_dwell_sample_args* a, void* stream) {
  if (!a || !a->p) {
    tq_set_error("tq_dwell_sample: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->mode == TQ_DWELL_COUNT ? (!a->counts || !a->hist_bound || !a->hist_unbound)
                                : (a->mode != TQ_DWELL_EMIT || !a->offsets || (a->total > 0 && !a->intervals))) {
    tq_set_error(a->mode == TQ_DWELL_COUNT || a->mode == TQ_DWELL_EMIT ? "tq_dwell_sample: NULL required pointer"
                                                                       : "tq_dwell_sample: unknown mode");
    return TQ_ERR_ARG;
  }
  if (a->N < 1 || a->F < 1 || a->S < 1 || a->total < 0 || a->N > 65535 * 64) {
    tq_set_error("tq_dwell_sample: N, F and S must be positive (and total >= 0)");
    return TQ_ERR_ARG;
  }
  const dim3 grid((unsigned)a->N, (unsigned)((a->S + 63) / 64));
  if (grid.y > 65535u) {
    tq_set_error("tq_dwell_sample: S too large");
    return TQ_ERR_ARG;
  }
  if (a->mode == TQ_DWELL_COUNT) {
    hipLaunchKernelGGL(tq_dwell_sample_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, *a);
  } else {
    if (a->total == 0) return TQ_OK;
    hipLaunchKernelGGL(tq_dwell_sample_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, *a);
  }
  return tq_launch_status("tq_dwell_sample_kernel");
}

// ---- batched MLE: one wave (= one workgroup) per posterior sample -----------------------------------------------------
// A row of at most TQ_DWELL_LDS_PAIRS pairs is staged in LDS once per launch (when stage_lds) and every step reads it
// there; a longer row, or stage_lds = 0, is read from global memory (L2) every step.
template <int K>
__global__ __launch_bounds__(64) void tq_dwell_fit_kernel(const tq_dwell_fit_args a) {
  extern __shared__ float2 pairs[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int64_t r0 = a.row_ptr[s], r1 = a.row_ptr[s + 1];
  const int len = (int)(r1 - r0);
  const float* vals = a.values + r0;
  const float* wts = a.weights + r0;
  const bool staged = a.stage_lds && len <= TQ_DWELL_LDS_PAIRS;  // wave-uniform
  float n = 0.0f;
  for (int i = lane; i < len; i += 64) {
    const float t = vals[i], wt = wts[i];
    n += wt;
    if (staged) pairs[i] = make_float2(t, wt);
  }
  n = tq_fit_wave_sum(n);
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
    float R[K], RT[K];
#pragma unroll
    for (int j = 0; j < K; ++j) R[j] = RT[j] = 0.0f;
    if (staged) {
#pragma unroll 2
      for (int i = lane; i < len; i += 64) {
        const float2 x = pairs[i];
        tq_dwell_accumulate<K>(q, x.x, x.y, R, RT);
      }
    } else {
#pragma unroll 2
      for (int i = lane; i < len; i += 64) tq_dwell_accumulate<K>(q, vals[i], wts[i], R, RT);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      R[j] = tq_fit_wave_sum(R[j]);
      RT[j] = tq_fit_wave_sum(RT[j]);
    }
    if (t == last && a.loss) {  // loss at the parameters this step starts from (what svi.step() returns)
      float ll = 0.0f, r[K];
      for (int i = lane; i < len; i += 64) {
        const float2 x = staged ? pairs[i] : make_float2(vals[i], wts[i]);
        ll = fmaf(x.y, tq_dwell_resp<K>(q, x.x, r, true), ll);
      }
      ll = tq_fit_wave_sum(ll);
      if (lane == 0) a.loss[s] = -ll;
    }
    float g[P];
    tq_dwell_grad<K>(q, R, RT, n, g);
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
static void dwell_fit_launch(const tq_dwell_fit_args* a, hipStream_t stream) {
  const size_t lds = a->stage_lds ? (size_t)TQ_DWELL_LDS_PAIRS * sizeof(float2) : 0;
  hipLaunchKernelGGL(tq_dwell_fit_kernel<K>, dim3((unsigned)a->S), dim3(64), lds, stream, *a);
}

extern "C" int tq_dwell_fit(const tq_dwell_fit_args* a, void* stream) {
  if (!a || !a->values || !a->weights || !a->row_ptr || !a->state) {
    tq_set_error("tq_dwell_fit: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->K < 1 || a->K > TQ_DWELL_KMAX) {
    tq_set_error("tq_dwell_fit: K must be in 1 .. TQ_DWELL_KMAX");
    return TQ_ERR_ARG;
  }
  if (a->S < 1 || a->step0 < 0 || a->n_steps < 1 || !tq_adam_settings_ok(a->lr, a->beta1, a->beta2, a->eps)) {
    tq_set_error("tq_dwell_fit: unsupported S/step0/n_steps or Adam settings");
    return TQ_ERR_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;
  switch (a->K) {
    case 1: dwell_fit_launch<1>(a, st); break;
    case 2: dwell_fit_launch<2>(a, st); break;
    case 3: dwell_fit_launch<3>(a, st); break;
    case 4: dwell_fit_launch<4>(a, st); break;
    case 5: dwell_fit_launch<5>(a, st); break;
    case 6: dwell_fit_launch<6>(a, st); break;
    case 7: dwell_fit_launch<7>(a, st); break;
    default: dwell_fit_launch<8>(a, st); break;
  }
  return tq_launch_status("tq_dwell_fit_kernel");
}
