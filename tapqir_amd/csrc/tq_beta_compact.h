// tq_beta_compact.h -- part of the translation unit tq_cosmos.hip, included from its headers only: the draw of one local
// guide site by one workgroup (tq_sample_site_wg, what every sampling launch runs), whose AffineBeta sites go through
// the regime compaction below.
#pragma once
#include <hip/hip_runtime.h>

#include "tq_bodies.h"

// ---- regime compaction of the AffineBeta implicit gradients -------------------------------------------------------
// torch's _dirichlet_grad is piecewise (two series regimes, a saddle-point expansion, a rational fit) and a wave executes
// every regime one of its lanes needs.  At the reference's initial parameters all draws sit in the saddle-point regime;
// in a converged fit the guide concentrations of absent spots have shrunk (size 5..18) and the lanes of EVERY wave are
// spread over all of them (scripts/regime_mix.py: per lane 0.50 pair / 0.40 x-small series / 0.10 (1-x)-small series /
// 0.40 rational, per wave 1.0 each), which made the sampling launch the largest of the step (157 us against 75).
// Here the workgroup (256 draws of one site kind) first classifies its draws, writes one task per needed evaluation into
// a queue in LDS ordered by regime, and evaluates the queue with consecutive lanes on consecutive tasks: a wave then runs
// one regime (two at a boundary), and each regime runs on as many waves as its tasks fill.  Same routines on the same
// arguments as tq_affine_beta_site_terms: bit-identical results.  Workgroups whose draws are all in the common
// (saddle-point pair) class skip the queue.
#define TQ_BC_NT 256
// Task queues in LDS.  A draw needs at most two evaluations, so the five classes fit three regions filled from both ends
// (no class needs another one's count before it can write): R1 = {x-small series up, rational down}, R2 = {pair up,
// (1-x)-small series down}, R3 = {saddle point of one direction}.  One 16-byte record per task.
struct TqBetaCompactLds {
  float4 r1[2 * TQ_BC_NT], r2[2 * TQ_BC_NT], r3[TQ_BC_NT];  // {draw, its alpha, size, bits((lane << 2) | direction code)}
                                                            // ((1-x)-small series: 1 - draw, which is what it takes)
  float c0[TQ_BC_NT];                                       // class 3: the other direction's alpha (rounding fallback)
  float res[2 * TQ_BC_NT];
  int cnt[8];                                               // tasks per class
};

__device__ __forceinline__ int tq_mbcnt(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// slot of task number k of class c in its region
__device__ __forceinline__ float4* tq_bc_slot(TqBetaCompactLds& L, int c, int k) {
  switch (c) {
    case 0: return &L.r2[k];
    case 1: return &L.r1[k];
    case 2: return &L.r2[2 * TQ_BC_NT - 1 - k];
    case 3: return &L.r3[k];
    default: return &L.r1[2 * TQ_BC_NT - 1 - k];
  }
}

__device__ __forceinline__ void tq_site_beta_compact(const tq_cosmos_args& a, const int site, const int64_t i, const bool live,
                                                     TqBetaCompactLds& L) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < 8) L.cnt[tid] = 0;
  __syncthreads();  // (at the top of the kernel: every wave arrives at once)
  TqSiteDraw d;
  float t = 0.0f, omt = 1.0f, c1 = 0.0f, c0 = 0.0f, size = 0.0f;
  int r0 = -1, r1 = -1;
  bool pair = false, clamped = true;
  if (live) {
    d = tq_site_draw(a, site, i);
    const float sc = d.hi - d.lo, rsc = TQ_FRCP(sc);  // (the expressions of tq_affine_beta_site_terms)
    t = (d.val - d.lo) * rsc;
    omt = tq_affine_one_minus_t(d.val, d.hi, rsc, t);
    size = d.p1;
    c1 = size * (d.p0 - d.lo) * rsc;
    c0 = size * (d.hi - d.p0) * rsc;
    clamped = (d.val <= d.lo + a.eps * sc) || (d.val >= d.hi - a.eps * sc);
    if (!clamped) {
      pair = tq_beta_grad_pair_applies((double)t, (double)c1, (double)size - (double)c1);
      if (!pair) {
        const double total = size;
        r0 = tq_dirichlet_grad_regime((double)t, (double)c1, total - (double)c1, total);
        r1 = tq_dirichlet_grad_regime((double)omt, (double)c0, total - (double)c0, total);
      }
    }
  }
  // A wave whose draws are all in the common class (saddle-point pair: every wave at the reference's initial parameters)
  // is already uniform: it evaluates in place and only joins the barriers (and the evaluation of other waves' tasks).
  float dd[2] = {0.0f, 0.0f};
  const bool wave_mixed = __ballot(r0 >= 0) != 0;
  if (!wave_mixed) {
    if (pair) {
      double ga = t, gb = c1;
      tq_beta_grad_pair_mid((double)t, (double)c1, (double)size - (double)c1, &ga, &gb);
      dd[0] = (float)ga;
      dd[1] = (float)gb;
    }
  } else {
    // tasks per class: 0 pair (both directions of a draw), 1 x-small series, 2 (1-x)-small series, 3 saddle point of one
    // direction (the pair routine with the boundary test off), 4 rational
    int k[5], pos[5];
    k[0] = pair ? 1 : 0;
    k[1] = (r0 == 0) + (r1 == 0);
    k[2] = (r0 == 1) + (r1 == 1);
    k[3] = (r0 == 2 || r1 == 2) ? 1 : 0;
    k[4] = (r0 == 3) + (r1 == 3);
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const uint64_t m1 = __ballot(k[c] >= 1), m2 = __ballot(k[c] == 2);
      const int n = __popcll(m1) + __popcll(m2);
      int base = 0;
      if (lane == 0 && n) base = atomicAdd(&L.cnt[c], n);  // (LDS; the order of the waves does not matter: a task's result
      pos[c] = __shfl(base, 0, 64) + tq_mbcnt(m1) + tq_mbcnt(m2);  //  does not depend on its place in the queue)
    }
    auto put = [&](int c, int kk, float x, float al, int code) {
      *tq_bc_slot(L, c, kk) = make_float4(x, al, size, __int_as_float((tid << 2) | code));
    };
    if (k[0]) put(0, pos[0], t, c1, 0);
    if (k[3]) {
      put(3, pos[3], t, c1, (r0 == 2 ? 1 : 0) | (r1 == 2 ? 2 : 0));
      L.c0[tid] = c0;
    }
    {
      const float xf[2] = {t, omt}, af[2] = {c1, c0};
      const int rr[2] = {r0, r1};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = rr[j];
        if (r == 0) put(1, pos[1]++, xf[j], af[j], j);
        if (r == 1) put(2, pos[2]++, xf[1 - j], af[j], j);  // (the series takes 1 - x: the record holds that)
        if (r == 3) put(4, pos[4]++, xf[j], af[j], j);
      }
    }
    L.res[2 * tid] = 0.0f;
    L.res[2 * tid + 1] = 0.0f;
  }
  __syncthreads();
  int n_c[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) n_c[c] = L.cnt[c];
  if (n_c[0] + n_c[1] + n_c[2] + n_c[3] + n_c[4] != 0) {
    // One loop per class, so that each regime's code and registers stand alone; the classes start on successive waves
    // (class c on the wave after the last one of class c-1), which spreads the ~1.4 evaluations per draw of a converged fit
    // evenly over the four waves.
    int wave0 = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int n = n_c[c];
      const int slot = (((wave - wave0) & (TQ_BC_NT / 64 - 1)) << 6) | lane;
      for (int qc = slot; qc < n; qc += TQ_BC_NT) {
        const float4 rec = *tq_bc_slot(L, c, qc);
        const float x = rec.x, al = rec.y, sz = rec.z;
        const int dst = __float_as_int(rec.w) >> 2, code = __float_as_int(rec.w) & 3;
        const double total = sz;
        if (c == 0) {
          double ga = x, gb = al;
          tq_beta_grad_pair_mid((double)x, (double)al, total - (double)al, &ga, &gb);
          L.res[2 * dst] = (float)ga;
          L.res[2 * dst + 1] = (float)gb;
        } else if (c == 1) {
          L.res[2 * dst + code] = (float)tq_beta_grad_alpha_small((double)x, (double)al, total - (double)al);
        } else if (c == 2) {
          L.res[2 * dst + code] = -tq_beta_grad_beta_small_f(x, sz - al, al);
        } else if (c == 3) {
          double ga = 0.0, gb = 0.0;
          if (!tq_beta_grad_pair_mid<true>((double)x, (double)al, total - (double)al, &ga, &gb)) {
            // (the two directions disagree about alpha, beta > 6 within rounding: the plain evaluation, as tq_beta_grad_pair_rest)
            const float c0q = L.c0[dst];
            ga = tq_beta_grad_alpha_mid((double)x, (double)al, total - (double)al);
            gb = tq_beta_grad_alpha_mid((double)(1.0f - x), (double)c0q, total - (double)c0q);
          }
          if (code & 1) L.res[2 * dst] = (float)ga;
          if (code & 2) L.res[2 * dst + 1] = (float)gb;
        } else {
          L.res[2 * dst + code] = tq_beta_grad_rational(x, al, sz);
        }
      }
      wave0 += (n + 63) >> 6;
    }
    __syncthreads();
    if (wave_mixed) {
      dd[0] = L.res[2 * tid];
      dd[1] = L.res[2 * tid + 1];
    }
  }
  if (live) {
    float terms[TQ_NSITE_TERMS];
    tq_affine_beta_site_terms(d.val, d.p0, d.p1, d.lo, d.hi, a.eps, terms, dd);
    tq_site_store(a, site, d, terms);
  }
}

// one site of one unit per lane; workgroups are uniform in the site (grid.y), AffineBeta sites go through the compaction
__device__ __forceinline__ void tq_sample_site_wg(const tq_cosmos_args& a, const int site, const int64_t i, const int64_t B) {
  if (site > a.K) {
    __shared__ TqBetaCompactLds s_bc;
    tq_site_beta_compact(a, site, i, i < B, s_bc);
  } else if (i < B) {
    tq_body_site(a, site, i);
  }
}
