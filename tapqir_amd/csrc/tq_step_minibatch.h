// tq_step_minibatch.h -- part of the translation unit tq_cosmos.hip, included from there only (it defines a __global__
// kernel): the single-launch minibatch step, the draw of the next step's subsample and the split lazy-Adam replay it runs.
// =============================================================================================================
// Single-launch minibatch step (tq_cosmos_minibatch_step).
//
// The reference's default operating point (10 AOIs x 512 frames, main.py:1428-1431) is 5120 units: 80 waves of work for
// a chip with 4096 wave slots.  As five launches (lazy-Adam catch-up, site draws + previous tail, likelihood, per-unit,
// per-AOI) a step costs five launch latencies on the device (70 us) and about as much on the host, which becomes the
// bottleneck.  Here ONE launch runs a step; a workgroup owns U = 16 or 20 units (tq_mb_upr) through
// all phases:
//   tail workgroup: tail of the PREVIOUS step (cross-unit sums, per-AOI sites, global sites, ELBO, Adam of the per-AOI /
//                   global parameters) and the global draws of this step, the GAIN's chain first: flag 1 (device-scope
//                   release) when the gain is drawn, flag 2 when the other draws are; then the next step's subsample
//                   (tq_draw_subsample).  Ticket 0, or the block dispatched last if it claims the role (tail_last);
//   phase 1       : lazy-Adam catch-up of the U units' local parameters, then their 9 x U guide-site draws;
//   (wait 1)      : one lane polls flag 1 (the likelihood needs this step's gain);
//   phase 2       : the 16-lanes-per-unit likelihood routine of tq_ksmogn_kernel (tq_ksmogn_tile_at); of 20 units the
//                   last four with a wave each;
//   (wait 2)      : flag 2 (the per-unit terms need the tables of pi, lamda, proximity: set long before);
//   phase 3       : per-unit ELBO terms, gradients and Adam (one lane per unit), row of partial sums with the per-AOI
//                   frame sums folded in (rows of U units, tq_rows.h; tq_rows_sums_body<16>).
// Phases hand data over through the step workspace in global memory; a workgroup lives on one CU, whose L1 its waves
// share, so a workgroup barrier orders those accesses.  The tail workgroup never waits for a workgroup that may not be
// resident yet, so the waiting workgroups cannot deadlock whatever the dispatch order.  The tail of THIS step runs in the next launch (or in
// tq_cosmos_tail).
//
// Units per workgroup (= per row of partial sums) of the single-launch minibatch step: 16, one 16-lane group each -- or 20,
// the last four with a wave each, when that takes fewer rounds of pixel iterations on the chip's 256 CUs.  A workgroup
// keeps one wave per SIMD busy for 13 iterations of P = 14 (196 pixels on 16 lanes), 17 with 20 units (+ 4: 196 pixels on 64
// lanes); a CU that hosts two workgroups takes twice as long, and the default 10 x 512 minibatch is 320 workgroups of 16
// units -- 64 CUs with two, 26 iterations on the critical path -- but 256 of 20: 17.  With a single camera offset the phase is
// short, but every phase of a workgroup that shares its CU is slower: 49.5 -> 44.7 us per step with 20 (once the gain has its
// own flag; before that the tail workgroup next to a worker delayed everybody and 20 lost, 55.5 against 53.0).  A pure function
// of the batch geometry (TAPQIR_AMD_MB_UNITS = 16 / 20 overrides), which the host works out (tq_mb_upr in tq_cosmos.hip): the
// launch that runs the pending tail calls it again.
// =============================================================================================================
#pragma once
#include <hip/hip_runtime.h>

#include "tq_bodies.h"
#include "tq_ksmogn_dev.h"
#include "tq_rows.h"
#include "tq_stamps.h"
#include "tq_step_rows.h"
#include "tq_step_staged.h"

// The next step's subsample, drawn by the tail workgroup of a minibatch launch (and by tq_subsample_draw, the same routine in
// a launch of its own): `take` of `n` indices without replacement = the indices of the `take` smallest of n Philox keys
// (stream: seed, step, site, element = index; ties broken by the index).  The law of randperm(n)[:take] (pyro.plate's
// subsample, cosmos.py:194-208) up to the order of the selected indices, which no sum depends on.  256 threads,
// n <= TQ_SUBSAMPLE_MAX = 65536 (the index field of the composite below); `hist` holds 2048 + 8 int32 words of LDS whatever n.
//
// Selection by radix instead of a sort (a bitonic sort of 1024 keys in LDS is 55 barrier-separated stages, ~2.5 us of every
// step): a histogram of the top 11 bits of the 48-bit composite (key << 16 | index), a scan over its bins to the bin that
// holds the take-th smallest, and -- only if that bin is not taken whole -- the same again on the next 11 bits inside it
// (levels of 11, 11, 11, 11 and 4 bits; random keys: the boundary bin of the second level holds one or two elements, so
// two levels, seldom three).  Then the selected indices are compacted in (thread, slot) order through a second scan: thread
// tid owns the indices tid, tid + 256, ..., so the output lists them ascending by (i mod 256, i div 256) and does not depend
// on the timing of any atomic.
//
// Thread tid's composites: up to TQ_SUBSAMPLE_REG = 2048 indices, eight in registers (the default minibatches; fully unrolled).
// Beyond, the thread walks its ceil(n / 256) indices once per pass -- a pass per level, one to count, one to write -- and
// recomputes the key of an index in every pass: four interleaved Philox chains per thread measured faster than composites
// parked in global memory after the first pass and loaded back (by about 6 % at n = 65536, 20 % at 4000).
#define TQ_SUBSAMPLE_REG 2048
#define TQ_SUBSAMPLE_LDS (sizeof(int) * (2048 + 8)) /* histogram of 2048 bins + scan / boundary words: what a launch that draws must provide */
__device__ __forceinline__ int tq_block_exscan(int v, int* s_w) {  // exclusive prefix sum over the 256 threads; s_w: 4 words
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();  // (the previous use of s_w has been read)
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w < wave) base += s_w[w];
  return base + inc - v;
}
__device__ __forceinline__ uint64_t tq_subsample_composite(uint64_t seed, uint32_t step, uint32_t site, int i) {
  TqPhilox s;
  tq_philox_init(&s, seed, step, site, (uint64_t)i);
  return ((uint64_t)tq_philox_next(&s) << 16) | (uint32_t)i;
}
template <bool REG>
__device__ __forceinline__ void tq_draw_subsample_impl(int* hist, uint64_t seed, uint32_t step, uint32_t site, int n, int take,
                                                       int32_t* out) {
  constexpr int PER = TQ_SUBSAMPLE_REG / 256;
  constexpr int UNR = REG ? PER : 4;
  int* s_w = hist + 2048;      // 4 words of the scans
  int* s_bnd = hist + 2048 + 4;  // boundary bin, elements below it, elements in it
  const int tid = threadIdx.x;
  const int per = REG ? PER : (n + 255) >> 8;  // slots of this thread: index tid + 256 j in slot j
  uint64_t c[PER];
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + 256 * j;
      c[j] = i < n ? tq_subsample_composite(seed, step, site, i) : ~0ull;
    }
  }
  auto composite = [&](int j) -> uint64_t {  // of slot j, whose index is < n
    if constexpr (REG) return c[j];
    return tq_subsample_composite(seed, step, site, tid + 256 * j);
  };
  uint64_t path = 0, T = 0;
  int need = take;
  for (int level = 0; level < 5; ++level) {
    const int shift = level == 4 ? 0 : 37 - 11 * level;
    const int width = level == 4 ? 4 : 11;
    for (int b = tid; b < 2048; b += 256) hist[b] = 0;
    __syncthreads();
#pragma unroll UNR
    for (int j = 0; j < per; ++j) {
      if (tid + 256 * j < n) {
        const uint64_t v = composite(j);
        if ((v >> (shift + width)) == path) atomicAdd(&hist[(int)((v >> shift) & ((1u << width) - 1u))], 1);
      }
    }
    __syncthreads();
    int cnt[8], local = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      cnt[q] = hist[8 * tid + q];
      local += cnt[q];
    }
    int run = tq_block_exscan(local, s_w);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (run < need && run + cnt[q] >= need) {
        s_bnd[0] = 8 * tid + q;
        s_bnd[1] = run;
        s_bnd[2] = cnt[q];
      }
      run += cnt[q];
    }
    __syncthreads();
    const int b = s_bnd[0], below = s_bnd[1], inbin = s_bnd[2];
    path = (path << width) | (uint64_t)b;
    need -= below;
    if (inbin == need) {  // the boundary bin is taken whole (always at the last level: composites are distinct)
      T = (path + 1) << shift;
      break;
    }
    __syncthreads();  // (s_bnd is rewritten at the next level)
  }
  int mine = 0;
#pragma unroll UNR
  for (int j = 0; j < per; ++j)
    if (tid + 256 * j < n) mine += composite(j) < T ? 1 : 0;
  int at = tq_block_exscan(mine, s_w);
#pragma unroll UNR
  for (int j = 0; j < per; ++j)
    if (tid + 256 * j < n && composite(j) < T) out[at++] = (int32_t)(tid + 256 * j);
  __syncthreads();  // (hist is reused by the next draw)
}
// The chunked walk stays out of line: inlined (twice) into tq_minibatch_kernel its Philox chains and level loop took part in
// the register allocation of the whole launch and moved the spills of the workers' phases.  One call per drawn axis.
static __device__ __noinline__ void tq_draw_subsample_chunked(int* hist, uint64_t seed, uint32_t step, uint32_t site, int n, int take,
                                                              int32_t* out) {
  tq_draw_subsample_impl<false>(hist, seed, step, site, n, take, out);
}
__device__ __forceinline__ void tq_draw_subsample(int* hist, uint64_t seed, uint32_t step, uint32_t site, int n, int take,
                                                  int32_t* out) {
  if (n <= TQ_SUBSAMPLE_REG) tq_draw_subsample_impl<true>(hist, seed, step, site, n, take, out);
  else tq_draw_subsample_chunked(hist, seed, step, site, n, take, out);
}
#define TQ_SITE_SUBSAMPLE_N 0xA00u
#define TQ_SITE_SUBSAMPLE_F 0xA01u

// Lazy-Adam replay of ONE element by G neighbouring lanes (the last, thinly filled pass of the catch-up phase: 32 of 288
// elements at K = 2, which cost the workgroup a second full pass of ~136 dependent steps on one wave).  With zero gradient
// the increment of step s0 + k depends on (m0 beta1^k, v0 beta2^k) and the step's bias factors only, not on the parameter:
// lane `part` starts from the moments after k0 = part * ceil(n / G) steps (closed form), adds up the increments of its own
// steps, the G sums are added and the parameter moves once.  Against the step-by-step form the sum is rounded once instead
// of at every step (a few ulp of the parameter) and no increment is dropped as negligible.  Steps older than the bias
// table take the plain replay on the first lane.
template <int G>
__device__ __forceinline__ void tq_adam_replay_split(const tq_cosmos_args& a, int64_t j, int s0, int s1, const float* tab, int T0,
                                                     float p, float m, float v, int part) {
  const bool valid = j >= 0 && s0 <= s1;
  const bool direct = valid && s0 < T0;
  const int n = valid ? s1 - s0 + 1 : 0;
  float dp = 0.0f;
  if (valid && !direct) {
    const int L = (n + G - 1) / G;
    const int k0 = part * L;
    const int k1 = k0 + L < n ? k0 + L : n;
    if (k0 < k1) {
      float mm = m * (float)tq_powi((double)a.beta1, k0), vv = v * (float)tq_powi((double)a.beta2, k0);
      const float* t = tab + 2 * (s0 + k0 - T0);
#pragma unroll 4
      for (int k = k0; k < k1; ++k, t += 2) {
        mm = a.beta1 * mm;
        vv = a.beta2 * vv;
        dp += t[0] * mm * TQ_FRCP(TQ_FSQRT(vv) * t[1] + a.adam_eps);
      }
    }
  }
#pragma unroll
  for (int o = 1; o < G; o <<= 1) dp += __shfl_xor(dp, o, 64);
  if (direct) {
    if (part == 0) tq_adam_replay_tab_given(a, j, s0, s1, tab, T0, p, m, v);
  } else if (valid && part == 0) {
    a.params[j] = p - dp;
    a.exp_avg[j] = m * (float)tq_powi((double)a.beta1, n);
    a.exp_avg_sq[j] = v * (float)tq_powi((double)a.beta2, n);
  }
}

template <int K, bool ONE, int U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void tq_minibatch_kernel(
    const tq_cosmos_args a, const tq_cosmos_args prev, const int has_prev, const tq_ksmogn_args k, const int64_t B,
    const int tail_last) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_ticket, s_ok, s_role;
  __shared__ float s_part[4][TQ_ROWS_MAXCOL];
  const int tid = threadIdx.x;
  TQ_MB_STAMP_LOCALS;
  TQ_MB_STAMP(TQ_ST_START);
  if (tid == 0) s_ticket = __hip_atomic_fetch_add(&a.sync[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  TQ_MB_STAMP(TQ_ST_TICKET);
  const int ticket = s_ticket;
  const int flag_value = a.sync_value;
  // every workgroup counts itself out exactly once; the last one re-arms the ticket counter for the next launch
  auto count_out = [&]() {
    const int done = __hip_atomic_fetch_add(&a.sync[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (done == (int)gridDim.x - 1) {
      __hip_atomic_store(&a.sync[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&a.sync[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&a.sync[TQ_SYNC_CLAIM], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  if (ticket >= (int)gridDim.x) {
    // the counter did not start from zero (an earlier launch was torn down before it could re-arm it): this launch has
    // no valid work split.  Touch nothing, leave a NaN loss, and re-arm so that the next launch is whole again.
    if (tid == 0) {
      a.elbo_out[0] = __builtin_nan("");
      count_out();
    }
    return;
  }
  // Who runs the tail.  Ticket 0 by default: that workgroup is resident whatever else the chip is doing, and it waits for
  // nobody.  With `tail_last` (a grid of 256 k + 1 workgroups: every CU hosts k of them and ONE hosts k + 1) the LAST block
  // of the grid -- dispatched last, so the one that doubles up on a CU -- claims the tail if it gets there within a few
  // microseconds: the tail is short, and the workgroup it shares the CU with keeps its SIMDs to itself for the long
  // likelihood phase (two workers on one CU take twice as long there and ARE the critical path of the launch).  The
  // ticket-0 workgroup then takes over the units of the claimer.  It polls the claim for a bounded time only and
  // claims the tail itself when nothing arrives: progress never depends on a workgroup that is not resident yet.
  int work = ticket - 1;
  bool is_tail = ticket == 0;
  if (tail_last) {
    if (tid == 0) {
      int role = ticket == 0 ? -1 : ticket - 1;  // -1: the tail
      if (blockIdx.x == gridDim.x - 1 && ticket != 0) {
        int expected = 0;
        if (__hip_atomic_compare_exchange_strong(&a.sync[TQ_SYNC_CLAIM], &expected, ticket + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
          role = -1;
      } else if (ticket == 0 && blockIdx.x != gridDim.x - 1) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        int c;
        while ((c = __hip_atomic_load(&a.sync[TQ_SYNC_CLAIM], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 &&
               __builtin_amdgcn_s_memrealtime() - t0 < 600ull)  // 6 us of the 100 MHz clock
          __builtin_amdgcn_s_sleep(2);
        if (c == 0 && !__hip_atomic_compare_exchange_strong(&a.sync[TQ_SYNC_CLAIM], &c, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT)) {
          // (lost the race at the last moment: c now holds the claimer's ticket + 1)
        }
        if (c != 0) role = c - 2;  // the units the claimer would have had
      }
      s_role = role;
    }
    __syncthreads();
    work = s_role;
    is_tail = work < 0;
  }
  if (is_tail) {  // the extra workgroup of the grid: owns no units
    __shared__ double s_w[4][TQ_MAX_NGSUM];
    __shared__ double s_e[TQ_NGSITES(TQ_MAXQ)];
    TQ_MB_TAIL_STAMP(TQ_ST_TAIL_START);
    // The workers need the GAIN of this step before their likelihood phase and the other global draws (tables of pi, lamda,
    // proximity) only in the per-unit phase after it: the gain's chain -- gradient of its site, Adam of its two
    // parameters, the draw -- runs on wave 0 by itself and is published first (sync[1]); the other sites' gradients
    // (7-8 us each against 3.5) run beside it on waves 1..3, and their Adam and draws follow under a second flag
    // (sync[TQ_SYNC_FLAG2]) that is long set when a worker gets to it.
    const int lane = tid & 63, wave = tid >> 6;
    if (has_prev) {
      const int64_t Bp = tq_batch_units(prev);
      if (has_prev == TQ_PREV_ROWS) tq_rows_sums_body<TQ_UNIT_BLOCK>(prev, s_w);
      else if (has_prev == TQ_PREV_ROWS16 || has_prev == TQ_PREV_ROWS20) tq_rows_sums_body<16>(prev, s_w, tq_mb_rows_upr(has_prev));
      else tq_reduce_sums_fenced_body(prev, (Bp + TQ_UNIT_BLOCK - 1) / TQ_UNIT_BLOCK, Bp, s_w);
      // (the bodies end with gsum stored, a workgroup-scope fence and a barrier)
      if (lane == 0) {
        const int nsp = tq_num_gsites(prev);
        if (wave == 0) {
          s_e[0] = tq_body_globals_grad(prev, 0);
          const int64_t gb = tq_global_base(prev);  // [0] gain_loc [1] gain_beta (tq_globals.h)
          tq_body_adam(prev, gb);
          tq_body_adam(prev, gb + 1);
        } else {
          for (int sg = wave; sg < nsp; sg += 3) s_e[sg] = tq_body_globals_grad(prev, sg);
        }
      }
    }
    if (wave == 0) {
      if (lane == 0) {
        tq_body_sample_globals(a, 0);
        // publish: the gain once more in a sync word (what the workers read: wait_flag), then the storing lane drains,
        // releases at device scope and sets the flag
        __hip_atomic_store(&a.sync[TQ_SYNC_GAIN], __float_as_int(((const TqGlobals*)a.globals)->gain), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&a.sync[1], flag_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    TQ_MB_TAIL_STAMP(TQ_ST_TAIL_SUMS);
    if (has_prev) {
      if (tid == 0) {  // total ELBO of the previous step (as tq_globals_from_gsum_body)
        const int nsp = tq_num_gsites(prev);
        double eg = 0.0;
        for (int j = 0; j < nsp; ++j) eg += s_e[j];
        prev.elbo_out[0] = prev.gsum[TQ_GS_ELBO] + (double)prev.global_weight * eg;
      }
      const int64_t total = tq_num_params(prev), gb = tq_global_base(prev);
      for (int64_t j = tq_aoi_base(prev) + tid; j < total; j += 256)
        if (j != gb && j != gb + 1) tq_body_adam(prev, j);
      __threadfence_block();
      __syncthreads();
    }
    TQ_MB_TAIL_STAMP(TQ_ST_TAIL_ADAM);
    const int ns = tq_num_gsites(a);
    if (lane == 0)
      for (int sg = 1 + wave; sg < ns; sg += 4) tq_body_sample_globals(a, sg);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&a.sync[TQ_SYNC_FLAG2], flag_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    TQ_MB_TAIL_STAMP(TQ_ST_TAIL_DRAWN);
    // the NEXT step's subsample (nobody waits for it: the next launch reads it)
    if (a.next_ndx && a.nb < a.Nt) {
      tq_draw_subsample((int*)smem, a.seed, a.step + 1, TQ_SITE_SUBSAMPLE_N, a.Nt, a.nb, a.next_ndx);
      __syncthreads();
    }
    if (a.next_fdx && a.fb < a.F) tq_draw_subsample((int*)smem, a.seed, a.step + 1, TQ_SITE_SUBSAMPLE_F, a.F, a.fb, a.next_fdx);
    if (tid == 0) count_out();
    return;
  }
  // ---- phase 1: catch-up + site draws of this workgroup's U units (work index = ticket - 1) ----
  const int64_t wblk = work;
  const int64_t u0 = wblk * U;
  const int64_t u_end = u0 + U < B ? u0 + U : B;
  constexpr int NL = TQ_NLOCAL(K), NS = 1 + 4 * K;
  TQ_MB_STAMP(TQ_ST_PHASE1);
  if (a.last_step) {
    // per-step bias-correction factors of the last TQ_BIAS_TABLE_STEPS steps, shared by every element of the workgroup
    __shared__ float s_bias[2 * TQ_BIAS_TABLE_STEPS];
    const int s1 = (int)a.step;
    const int T0 = s1 - (TQ_BIAS_TABLE_STEPS - 1) > 1 ? s1 - (TQ_BIAS_TABLE_STEPS - 1) : 1;
    // the chain of dependent loads of every element of this thread (subsample index -> unit -> last step -> values) is
    // issued first and overlaps with the table build
    constexpr int NPASS = (NL * U + 255) / 256;
    // a thin last pass is shared out: G lanes per element (tq_adam_replay_split)
    constexpr int XLAST = NL * U - 256 * (NPASS - 1);
    constexpr int G = NPASS == 1 ? 1 : (XLAST <= 32 ? 8 : (XLAST <= 64 ? 4 : (XLAST <= 128 ? 2 : 1)));
    int64_t ej[NPASS];
    int es0[NPASS];
    float ep[NPASS], em[NPASS], ev[NPASS];
#pragma unroll
    for (int q = 0; q < NPASS; ++q) {
      const bool split = G > 1 && q == NPASS - 1;
      const int e = split ? 256 * q + tid / G : tid + 256 * q;
      const int64_t i = u0 + (e % U);
      ej[q] = -1;
      es0[q] = s1 + 1;
      ep[q] = em[q] = ev[q] = 0.0f;
      if (e < NL * U && i < B) {
        const int64_t u = tq_decode_unit(a, i).u;
        ej[q] = (int64_t)(e / U) * tq_num_units(a) + u;
        es0[q] = a.last_step[u] + 1;
        ep[q] = a.params[ej[q]];
        em[q] = a.exp_avg[ej[q]];
        ev[q] = a.exp_avg_sq[ej[q]];
      }
    }
    {
      double pw1 = tq_powi(a.beta1_d, T0 + tid), pw2 = tq_powi(a.beta2_d, T0 + tid);
      const double b1_256 = tq_powi(a.beta1_d, 256), b2_256 = tq_powi(a.beta2_d, 256);
      for (int e = tid; e < TQ_BIAS_TABLE_STEPS; e += 256) {  // same expressions as tq_adam_bias_entry
        if (T0 + e <= s1) {
          s_bias[2 * e] = a.lr * TQ_FRCP((float)(1.0 - pw1));
          s_bias[2 * e + 1] = TQ_FRCP(TQ_FSQRT((float)(1.0 - pw2)));
        }
        pw1 *= b1_256;
        pw2 *= b2_256;
      }
    }
    TQ_MB_STAMP_DETAIL(0);
    __syncthreads();
    TQ_MB_STAMP_DETAIL(1);
#pragma unroll
    for (int q = 0; q < NPASS; ++q) {
      if (G > 1 && q == NPASS - 1) tq_adam_replay_split<G>(a, ej[q], es0[q], s1, s_bias, T0, ep[q], em[q], ev[q], tid % G);
      else if (ej[q] >= 0) tq_adam_replay_tab_given(a, ej[q], es0[q], s1, s_bias, T0, ep[q], em[q], ev[q]);
      if (q == 0) { TQ_MB_STAMP_DETAIL(2); }
    }
    TQ_MB_STAMP_DETAIL(3);
    __syncthreads();
  }
  TQ_MB_STAMP(TQ_ST_CATCHUP);
  if constexpr (K <= 3 && (K + 1) * U <= 64) {
    // one KIND of site per wave -- wave 0 the K+1 Gamma sites (background, heights), waves 1..3 the width / x / y sites --
    // so that no wave runs the Gamma code and then the Beta code (with its regimes) for different lanes
    const int w = tid >> 6, l = tid & 63;
    const int nl = (w == 0 ? K + 1 : K) * U;
    const int site = (w == 0 ? 0 : K + 1 + (w - 1) * K) + (l / U);
    const int64_t i = u0 + (l % U);
    if (l < nl && i < B) tq_body_site(a, site, i);
  } else {
    for (int e = tid; e < NS * U; e += 256) {
      const int64_t i = u0 + (e % U);
      if (i < B) tq_body_site(a, e / U, i);
    }
  }
  __syncthreads();
  TQ_MB_STAMP(TQ_ST_SITES);
  // ---- wait for the gain of this step (bounded: ~2 s of the 100 MHz wall clock) ----
  __shared__ float s_gain;
  auto wait_flag = [&](int word) {
    if (tid == 0) {
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      int ok = 1;
      while (__hip_atomic_load(&a.sync[word], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != flag_value) {
        __builtin_amdgcn_s_sleep(16);
        if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
          ok = 0;
          break;
        }
      }
      // No acquire fence: at device scope it invalidates the CU's vector cache AND this XCD's L2 for every workgroup on
      // them.  What the tail workgroup publishes is read so that no stale copy can answer instead:
      //   the gain        from a sync word, with a device-scope load (here);
      //   TqGlobals       with plain (scalar) loads in the per-unit phase, after the second flag: no workgroup touches the
      //                   struct's cache lines earlier in the launch (the gain comes from the sync word for that reason), and
      //                   a launch starts with clean caches;
      //   per-AOI params  with device-scope loads in tq_body_unit (their first line also holds the end of the last
      //                   local-parameter row, which a replay may have read).
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (ok && word == 1) s_gain = __int_as_float(__hip_atomic_load(&a.sync[TQ_SYNC_GAIN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      s_ok = ok;
    }
    __syncthreads();
    return s_ok != 0;
  };
  auto step_lost = [&]() {  // never observed: leave a visible trace (NaN loss) instead of reading half-written tables
    if (tid == 0) {
      // The step is lost.  Its row of partial sums carries a NaN ELBO, so the tail of this step (run by the next launch or
      // by tq_cosmos_tail) reports a NaN loss whichever workgroup was late, and Model.run rolls back to its last
      // checkpoint (model.py:220-232); CosmosEngine.reset_adam_clock zeroes the sync words on that path.
      tq_row_sum(a, tq_row_floats(tq_num_gsum(a)), wblk, TQ_GS_ELBO) = __builtin_nanf("");
      a.elbo_out[0] = __builtin_nan("");
      __hip_atomic_fetch_add(&a.sync[TQ_SYNC_LOST], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (never reset: a soak run reads it)
      count_out();  // still counted: the ticket counter is re-armed for the launches that follow
    }
  };
  if (!wait_flag(1)) {
    step_lost();
    return;
  }
  TQ_MB_STAMP(TQ_ST_GAIN);
  // ---- phase 2: likelihood of the U units (reads the draws of phase 1 and the gain): sixteen of them with 16 lanes each,
  // and of U = 20 the last four with a wave each (tq_mb_upr: why 20)
  tq_ksmogn_args kw = k;
  kw.gain = &s_gain;  // (the copy read at the flag)
  tq_ksmogn_tile_at<K, ONE, true, 16, 16, false>(kw, B, u0, u_end, smem);
  if constexpr (U > 16) {
    static_assert(U == 20, "16 units at 16 lanes + 4 at 64");
    tq_ksmogn_tile_at<K, ONE, true, 64, 16, true>(kw, B, u0 + 16, u_end, smem);
  }
  __syncthreads();
  // ---- the other global draws (tables of the per-unit terms): set long ago, unless the tail workgroup started late ----
  if (!wait_flag(TQ_SYNC_FLAG2)) {
    step_lost();
    return;
  }
  TQ_MB_STAMP(TQ_ST_PIXEL);
  // ---- phase 3: per-unit terms + Adam, one lane per unit; row of partial sums ----
  float part[TQ_MAX_NGSUM];
  TqRowAoi aoi;
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) part[j] = 0.0f;
  tq_row_clear(aoi);
  // (units 16..19 of U = 20: the second lane of the first four 16-lane groups)
  const int64_t i = u0 + (tid >> 4) + 16 * (tid & 15);
  if ((tid & 15) < (U + 15) / 16 && i < u_end) {
    float aoi2[2];
    tq_body_unit<K, false, false, true>(a, i, part, aoi2);
    const uint32_t FC = (uint32_t)(a.fb * a.C);
    tq_row_fill(aoi, tq_row_slot(tq_row_first_aoi((uint32_t)u0, FC), (uint32_t)i / FC), (int)((uint32_t)i % (uint32_t)a.C), aoi2);
  }
  tq_row_store_wg(a, s_part, wblk, aoi, part);
  TQ_MB_STAMP(TQ_ST_UNIT);
  // the last workgroup to get here re-arms the ticket counter for the next launch (the flag holds the step number)
  if (tid == 0) count_out();
}
