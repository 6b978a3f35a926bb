// tq_step_rows.h -- part of the translation unit tq_cosmos.hip, included from there only (it defines __global__ kernels):
// the full-batch steps that leave rows of partial sums (the format: tq_rows.h) -- the two per-unit kernels that write
// rows, the group rows, the single-workgroup tail bodies, and the sampling launch that carries a pending tail.
#pragma once
#include <hip/hip_runtime.h>

#include "tq_beta_compact.h"
#include "tq_bodies.h"
#include "tq_ksmogn_dev.h"
#include "tq_ksmogn_il2.h"
#include "tq_rows.h"
#include "tq_stamps.h"
#include "tq_step_staged.h"

// Per-unit kernel of full-batch steps (tq_cosmos_step_overlapped / tq_cosmos_step): a workgroup of 256 consecutive units
// leaves one row, the per-AOI frame sums folded in.
template <int K>
__global__ __launch_bounds__(TQ_UNIT_BLOCK) void tq_unit_rows_kernel(const tq_cosmos_args a, const int64_t B) {
  __shared__ float s_part[TQ_UNIT_BLOCK / 64][TQ_ROWS_MAXCOL];
  const int64_t i = (int64_t)blockIdx.x * TQ_UNIT_BLOCK + threadIdx.x;
  const uint32_t FC = (uint32_t)(a.F * a.C);
  const uint32_t n0 = tq_row_first_aoi((uint32_t)blockIdx.x * TQ_UNIT_BLOCK, FC);
  float part[TQ_MAX_NGSUM];
  TqRowAoi aoi;
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) part[j] = 0.0f;
  tq_row_clear(aoi);
  if (i < B) {
    float aoi2[2];
    tq_body_unit<K>(a, i, part, aoi2);
    tq_row_fill(aoi, tq_row_slot(n0, (uint32_t)i / FC), (int)((uint32_t)i % (uint32_t)a.C), aoi2);
  }
  tq_row_store_wg(a, s_part, blockIdx.x, aoi, part);
}

// The pending tail: what a launch that carries the tail of the PREVIOUS step (`prev`, the kernels' `has_prev`) finds in
// prev's workspace and has to do before prev's global sites, total ELBO and Adam of the per-AOI / global parameters.  The
// host picks the code (tq_prev_code, tq_prev_code_sampling), tq_sample_locals_tail_kernel and tq_minibatch_kernel act on it.
enum TqPrevTail : int {
  TQ_PREV_NONE = 0,     // nothing pending
  TQ_PREV_FLAT = 1,     // flat partial sums of tq_unit_kernel + per-AOI terms of tq_aoi_kernel: cross-unit sums first
  TQ_PREV_REDUCED = 2,  // gsum is complete (all-reduced by the caller): global sites onwards
  TQ_PREV_ROWS = 3,     // rows of 64 / 256 units with the per-AOI sums folded in, added by the tail workgroup itself
  TQ_PREV_ROWS16 = 4,   // rows of 16 units of a single-launch minibatch step
  TQ_PREV_GROUPS = 6,   // as ROWS, the rows added per group of 4096 units by the idle workgroups of the sampling launch
  TQ_PREV_ROWS20 = 7,   // as ROWS16, rows of 20 units (tq_mb_upr)
};

// units per row of a step with rows: 16 (single-launch minibatch step; its rows hold tq_mb_rows_upr units), 64 (fused pixel
// + per-unit kernel), TQ_UNIT_BLOCK (tq_unit_rows_kernel)
__host__ __device__ __forceinline__ int tq_rows_upr(const tq_cosmos_args& a) {
  return a.tail_kind == TQ_TAIL_ROWS16 ? 16 : (a.pixel_mode == TQ_PIXEL_FUSED_UNIT ? 64 : TQ_UNIT_BLOCK);
}
__device__ __forceinline__ int tq_mb_rows_upr(int has_prev) { return has_prev == TQ_PREV_ROWS20 ? 20 : 16; }

// one wave: rows of group g of step `a` -> group row g (published); returns (lane 0) how many groups had been published before
__device__ __forceinline__ int tq_group_reduce_rows(const tq_cosmos_args& a, const int g) {
  const int lane = threadIdx.x & 63;
  const int nq = tq_num_gsum(a), ncol = tq_row_floats(nq);
  const int64_t B = tq_batch_units(a);
  const uint32_t UPR = (uint32_t)tq_rows_upr(a), RPG = tq_grp_rows(UPR);
  const int64_t nrows = (B + UPR - 1) / UPR;
  const int64_t r0 = (int64_t)g * RPG;
  const int nw = (int)((nrows - r0) < (int64_t)RPG ? (nrows - r0) : (int64_t)RPG);
  const bool have = lane < nw;
  const int64_t my = r0 + (have ? lane : 0);
  const float *my0 = tq_row_slot_pairs(tq_row(a, ncol, my), 0), *my1 = tq_row_slot_pairs(tq_row(a, ncol, my), 1);
  float s0[2 * TQ_MAXQ], s1[2 * TQ_MAXQ], col[TQ_MAX_NGSUM];
#pragma unroll
  for (int j = 0; j < 2 * TQ_MAXQ; ++j) {
    const bool used = j < 2 * a.C;
    s0[j] = (have && used) ? my0[j] : 0.0f;
    s1[j] = (have && used) ? my1[j] : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) col[j] = (have && j < nq) ? tq_row_sum(a, ncol, my, j) : 0.0f;
  float* grow = tq_grp_row(a, nrows, ncol, g);
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) {
    if (j < nq) {
      const double sum = tq_wave_sum_d_lane0((double)col[j]);
      if (lane == 0) __hip_atomic_store(&tq_grp_sums(grow)[j], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  const uint32_t FC = (uint32_t)(a.fb * a.C);
  const uint32_t u_first = tq_grp_first_unit((uint32_t)g), u_last = tq_grp_last_unit((uint32_t)g, B);
  const uint32_t n_lo = tq_row_first_aoi(u_first, FC), n_hi = u_last / FC;  // (the group row's AOI 0 is n_lo)
  const uint32_t n0 = tq_row_first_aoi(u_first + UPR * (uint32_t)lane, FC);  // this row's slot 0; slot 1 is the next AOI
  for (uint32_t n = n_lo; n <= n_hi; ++n) {
    float* out = tq_grp_aoi_pair(grow, n - n_lo, 0);
#pragma unroll
    for (int j = 0; j < 2 * TQ_MAXQ; ++j) {
      if (j < 2 * a.C) {
        const float v = (n0 == n) ? s0[j] : ((n0 + 1 == n) ? s1[j] : 0.0f);
        const float sum = tq_wave_sum_rows4(v);
        if (lane == 0) __hip_atomic_store(&out[j], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the group row has left
  int ticket = 0;
  if (lane == 0) ticket = __hip_atomic_fetch_add(a.sync + TQ_SYNC_GROUPS, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ticket;
}

// Fused pixel + per-unit kernel of full-batch steps (pixel_mode = TQ_PIXEL_FUSED_UNIT): a wave renders its tile of 64
// units (tq_il2_lane, the routine of tq_ksmogn_il2_kernel) and goes straight on to the per-unit terms + Adam of the same
// 64 units, lane for lane.  The pixel phase is bound by VALU issue (PMC: ~75 % busy) and the per-unit phase by HBM
// (4.3 TB/s of traffic at 33 % VALU busy): as two launches they run one after the other, here the waves of a SIMD are in
// different phases most of the time.  The pixel results go from one phase to the next in registers (56 B per unit
// neither written nor read), a launch boundary is gone, and the row of partial sums is per wave (rows of 64 units).
//
// Split tiles (nsplit > 0; tq_cosmos_args.pu_split).  The launch holds `slots` waves at a time (2048 on 256 CUs), so the
// ntiles mod slots tiles of the last round run on a nearly empty chip: 106 of 6250 tiles at c2.  A tile is one wave only
// because one wave walks all P rows, and everything the pixel loop leaves is a sum over pixels: the last `nsplit` tiles
// are each run by TQ_PU_PARTS waves that take a range of loop bodies each (tq_il2_lane with a TqSplitPart), in the first
// blocks of the grid so that they start with the first round.  A part wave writes its partial sums to its slab of
// pu_scratch with write-through stores, drains its store queue and takes a ticket on the tile's counter (the protocol of
// tq_group_reduce_rows); the wave that draws the tile's last ticket reads all four slabs (its own too) with device-scope
// loads, adds them as ((p0 + p1) + p2) + p3 and goes on as the wave of a whole tile does; the others leave.  Nobody waits,
// and who arrives last does not enter the result.  The counters are never reset: every launch draws TQ_PU_PARTS tickets
// per split tile, so the last one is the ticket with (ticket & 3) == 3.
#define TQ_PU_PARTS 4
#define TQ_PU_PAIRS 24 /* 8-byte values per lane of a slab: the most any instance leaves (K = 2, P = 14: 23) */
__host__ __device__ __forceinline__ int64_t tq_pu_counter_words(int64_t tiles) { return ((tiles + 63) / 64) * 64; }
__host__ __device__ __forceinline__ int64_t tq_pu_scratch_bytes(int64_t tiles) {
  return tq_pu_counter_words(tiles) * 4 + tiles * TQ_PU_PARTS * TQ_PU_PAIRS * 64 * 8;
}

struct TqSplitPart {
  static constexpr bool SPLIT = true;
  int body_begin, body_end;  // loop bodies of this part
  int part;                  // 0 .. TQ_PU_PARTS - 1
  int32_t* counter;          // tickets of the tile
  uint64_t* slabs;           // [TQ_PU_PARTS][TQ_PU_PAIRS][64] of the tile

  // lane 0 draws a ticket: was it the tile's last one?  (wave-uniform)
  __device__ __forceinline__ bool last_ticket() const {
    int ticket = 0;
    if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    asm volatile("" ::: "memory");  // the loads of the slabs stay behind the ticket
    return (ticket & (TQ_PU_PARTS - 1)) == TQ_PU_PARTS - 1;
  }
  // a tile of the scalar loop: nothing to hand over, the wave with the last ticket runs all of it
  __device__ __forceinline__ bool whole_tile() const { return last_ticket(); }

  template <int K, int P, bool COLACC>
  __device__ __forceinline__ bool combine(TqPixAcc2<K, P, COLACC>& A, float* sum_gy) const {
    static_assert(tq_acc2_pairs<K, P, COLACC>() <= TQ_PU_PAIRS, "slab too small");
    static_assert(TQ_PU_PARTS == 4, "the sum below is written out for four parts");
    uint64_t* mine = slabs + (int64_t)part * (TQ_PU_PAIRS * 64) + threadIdx.x;
    int v = 0;
    tq_acc2_each<K, P, COLACC>(A, sum_gy, [&](tq_f2& x) {
      uint64_t bits;
      __builtin_memcpy(&bits, &x, 8);
      __hip_atomic_store(mine + 64 * v, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ++v;
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slab has left
    if (!last_ticket()) return false;
    const uint64_t* all = slabs + threadIdx.x;
    v = 0;
    tq_acc2_each<K, P, COLACC>(A, sum_gy, [&](tq_f2& x) {
      tq_f2 p[TQ_PU_PARTS];
#pragma unroll
      for (int q = 0; q < TQ_PU_PARTS; ++q) {
        const uint64_t bits = __hip_atomic_load(all + (q * TQ_PU_PAIRS + v) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_memcpy(&p[q], &bits, 8);
      }
      x = ((p[0] + p[1]) + p[2]) + p[3];
      ++v;
    });
    return true;
  }
};

// loop bodies [begin, end) of part q of a tile of NB bodies: ceil(NB / 4) each, the last part what is left (P = 14: 2 2 2 1
// of 7 bodies of two rows, P = 20: 5 5 5 5 of 20 rows); every part has at least one
template <int P>
__device__ __forceinline__ void tq_pu_part_bodies(int q, int* begin, int* end) {
  constexpr int R = ((P / 2) % 2) ? 2 : 1, NB = P / R, PER = (NB + TQ_PU_PARTS - 1) / TQ_PU_PARTS;
  static_assert(PER * (TQ_PU_PARTS - 1) < NB, "a part without a loop body");
  *begin = q * PER;
  *end = (q + 1) * PER < NB ? (q + 1) * PER : NB;
}

// FMT (TqTileFmt): the format in which the packed pixel loop streams the tiles -- fp32 from images_il, or 16-bit integers
// from images_il16 where the caller has that copy (tq_il2_lane: the same bits either way, half the tile bytes).
template <int K, int P, int FMT = TQ_TILE_F32>
__global__ __launch_bounds__(64, 2) void tq_pixel_unit_kernel(const tq_ksmogn_args k, const tq_cosmos_args a, const int64_t B,
                                                              const int nsplit) {
  float pixv[TQ_PIXOUT(K)];
#pragma unroll
  for (int j = 0; j < TQ_PIXOUT(K); ++j) pixv[j] = 0.0f;
  // blocks 0 .. 4 nsplit - 1: the parts of the last nsplit tiles; then the whole tiles 0 .. ntiles - nsplit - 1
  int64_t tile = (int64_t)blockIdx.x - TQ_PU_PARTS * nsplit;
  if (tile < 0) {
    const int s = (int)blockIdx.x / TQ_PU_PARTS;
    TqSplitPart sp;
    sp.part = (int)blockIdx.x % TQ_PU_PARTS;
    tq_pu_part_bodies<P>(sp.part, &sp.body_begin, &sp.body_end);
    sp.counter = (int32_t*)a.pu_scratch + s;
    sp.slabs = (uint64_t*)((int32_t*)a.pu_scratch + tq_pu_counter_words(a.pu_scratch_tiles)) +
               (int64_t)s * (TQ_PU_PARTS * TQ_PU_PAIRS * 64);
    tile = ((B + 63) >> 6) - nsplit + s;
    if (!tq_il2_lane<K, P, true, TqSplitPart, FMT>(k, B, pixv, tile, sp)) return;
  } else {
    tq_il2_lane<K, P, true, TqWholeTile, FMT>(k, B, pixv, tile);
  }
  const int64_t i = tile * 64 + threadIdx.x;
  const uint32_t FC = (uint32_t)(a.F * a.C);
  const uint32_t n0 = tq_row_first_aoi((uint32_t)tile * 64u, FC);
  float part[TQ_MAX_NGSUM];
  TqRowAoi aoi;
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) part[j] = 0.0f;
  tq_row_clear(aoi);
  if (i < B) {
    float aoi2[2];
    tq_body_unit<K, false, true>(a, i, part, aoi2, pixv);
    tq_row_fill(aoi, tq_row_slot(n0, (uint32_t)i / FC), (int)((uint32_t)i % (uint32_t)a.C), aoi2);
  }
  tq_row_store_wave(a, tile, aoi, part);
}

// acc[j] += sum over this thread's rows (r = threadIdx.x, + 256, ...) of column j of the cross-unit sums.  Four rows are
// REQUESTED before any is added: with one row in flight at a time the 25 rows per thread of a c2-sized step with rows of
// 64 units were 25 memory latencies in sequence (~25 us, which made the tail workgroup the last one of the sampling
// launch it hides in).  Same order of additions per thread as the plain loop.
__device__ __forceinline__ void tq_rows_column_sums(const tq_cosmos_args& a, int64_t nrows, int nq, int ncol, double* acc) {
  for (int64_t r0 = threadIdx.x; r0 < nrows; r0 += 4 * 256) {
    float v[4][TQ_MAX_NGSUM];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = r0 + 256 * u;
#pragma unroll
      for (int j = 0; j < TQ_MAX_NGSUM; ++j) v[u][j] = (r < nrows && j < nq) ? tq_row_sum(a, ncol, r, j) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < TQ_MAX_NGSUM; ++j)
        if (j < nq) acc[j] += (double)v[u][j];
    }
  }
}

// Sums of a step whose per-unit kernel wrote such rows (ONE workgroup of 256 threads): per-AOI sites from the rows that
// overlap the AOI, cross-unit sums in fp64 -> gsum.  Ends with gsum stored, a workgroup-scope fence and a barrier: the
// workgroup goes on to the global sites (tq_globals_from_gsum_body) or to its own chain of them (tq_minibatch_kernel).
// UPR = units per row: TQ_UNIT_BLOCK (tq_unit_rows_kernel) or 16 (the single-launch minibatch step, whose rows hold `mb_upr`
// = 16 or 20 units: the host's tq_mb_upr)
template <int UPR_T>
__device__ __forceinline__ void tq_rows_sums_body(const tq_cosmos_args& a, double (*s_w)[TQ_MAX_NGSUM], const int mb_upr = 16) {
  const int nq = tq_num_gsum(a), ncol = tq_row_floats(nq);
  const int64_t B = tq_batch_units(a);
  const uint32_t UPR = UPR_T == 16 ? (uint32_t)mb_upr : (uint32_t)tq_rows_upr(a);  // (one instance serves rows of 64 and of 256)
  const int64_t nrows = (B + UPR - 1) / UPR;
  const uint32_t FC = (uint32_t)(a.fb * a.C);  // units of one AOI of the batch
  double acc[TQ_MAX_NGSUM];
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) acc[j] = 0.0;
  // per-AOI sites: frame sums = sums over the rows that overlap the AOI; prior terms; gradient of the AOI parameters
  const int nac = a.nb * a.C;
  if constexpr (UPR_T == 16) {
    // rows of 16 units: an AOI of the minibatch spans fb C / 16 rows (32 at the default 10 x 512) and this workgroup is
    // the critical path of the step -- 16 lanes share the rows of one (AOI, channel), so the loads of an AOI are two
    // round trips instead of 32 in sequence
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
    for (int ac0 = 0; ac0 < nac; ac0 += 16) {
      const int ac = ac0 + grp;
      const bool on = ac < nac;
      const uint32_t ai = on ? (uint32_t)ac / (uint32_t)a.C : 0u;
      const int c = on ? ac - (int)ai * a.C : 0;
      float s1 = 0.0f, s2 = 0.0f;
      if (on) {
        const uint32_t r_lo = (ai * FC) / UPR, r_hi = ((ai + 1) * FC - 1) / UPR;
        for (uint32_t r = r_lo + gl; r <= r_hi; r += 16) {
          const float* row = tq_row_aoi_pair(a, ncol, r, ai, c, UPR, FC);
          s1 += row[0];
          s2 += row[1];
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 16);
        s2 += __shfl_xor(s2, o, 16);
      }
      if (on && gl == 0) {
        float e;
        tq_body_aoi_finish(a, (int)ai, c, s1, s2, &e);
        acc[TQ_GS_ELBO] += (double)e;
      }
    }
    TQ_STAMP_AT(a, TQ_ST_AOI);
  } else {
    for (int ac = threadIdx.x; ac < nac; ac += 256) {
      const uint32_t ai = (uint32_t)ac / (uint32_t)a.C;  // position of the AOI in the batch
      const int c = ac - (int)ai * a.C;
      const uint32_t r_lo = (ai * FC) / UPR, r_hi = ((ai + 1) * FC - 1) / UPR;
      float s1 = 0.0f, s2 = 0.0f;
      for (uint32_t rb = r_lo; rb <= r_hi; rb += 4) {  // four rows requested before any is added (see tq_rows_column_sums)
        float p1[4], p2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t r = rb + u;
          const float* row = tq_row_aoi_pair(a, ncol, r, ai, c, UPR, FC);
          p1[u] = r <= r_hi ? row[0] : 0.0f;
          p2[u] = r <= r_hi ? row[1] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s1 += p1[u];
          s2 += p2[u];
        }
      }
      float e;
      tq_body_aoi_finish(a, (int)ai, c, s1, s2, &e);
      acc[TQ_GS_ELBO] += (double)e;
    }
  }
  if constexpr (UPR_T == 16) {  // a few hundred rows: the plain loop (and no extra registers in the minibatch kernel)
    for (int64_t r = threadIdx.x; r < nrows; r += 256) {
#pragma unroll
      for (int j = 0; j < TQ_MAX_NGSUM; ++j)
        if (j < nq) acc[j] += (double)tq_row_sum(a, ncol, r, j);
    }
  } else {
    tq_rows_column_sums(a, nrows, nq, ncol, acc);
  }
  tq_sums_finish(a, acc, s_w);
  __threadfence_block();
  __syncthreads();
  TQ_STAMP_AT(a, TQ_ST_GSUM);
}

// Sums of a step from the group rows that other workgroups publish (ONE workgroup of 256 threads): WAIT: polls the counter of
// published groups first (the tail workgroup inside a sampling launch; returns false after ~2 s without them: never
// observed, the caller leaves a NaN loss) -- else the caller knows they are all there (the last workgroup of
// tq_group_sums_kernel).  Then per-AOI sites from the one or two groups that overlap the AOI and the cross-unit sums -> gsum.
template <bool WAIT>
__device__ __forceinline__ bool tq_groups_sums_body(const tq_cosmos_args& a, double (*s_w)[TQ_MAX_NGSUM]) {
  const int nq = tq_num_gsum(a), ncol = tq_row_floats(nq);
  const int64_t B = tq_batch_units(a);
  const uint32_t UPR = (uint32_t)tq_rows_upr(a);
  const int64_t nrows = (B + UPR - 1) / UPR;
  const int ngroups = (int)tq_grp_count(B);
  const uint32_t FC = (uint32_t)(a.fb * a.C);
  __shared__ int s_ok;
  if (threadIdx.x == 0) {
    int ok = 1;
    if (WAIT) {
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(a.sync + TQ_SYNC_GROUPS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ngroups) {
        __builtin_amdgcn_s_sleep(8);
        if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
          ok = 0;
          break;
        }
      }
    }
    __hip_atomic_store(a.sync + TQ_SYNC_GROUPS, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok) return false;
  auto ld = [](const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto ldd = [](const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  double acc[TQ_MAX_NGSUM];
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) acc[j] = 0.0;
  const int nac = a.nb * a.C;
  for (int ac = threadIdx.x; ac < nac; ac += 256) {
    const uint32_t ai = (uint32_t)ac / (uint32_t)a.C;
    const int c = ac - (int)ai * a.C;
    const uint32_t g_lo = tq_grp_of_unit(ai * FC), g_hi = tq_grp_of_unit((ai + 1) * FC - 1);
    float s1 = 0.0f, s2 = 0.0f;
    for (uint32_t g = g_lo; g <= g_hi; ++g) {
      const float* p = tq_grp_aoi_pair(tq_grp_row(a, nrows, ncol, g), tq_grp_aoi_index(g, ai, FC), c);
      s1 += ld(p);
      s2 += ld(p + 1);
    }
    float e;
    tq_body_aoi_finish(a, (int)ai, c, s1, s2, &e);
    acc[TQ_GS_ELBO] += (double)e;
  }
  for (int g = threadIdx.x; g < ngroups; g += 256) {
    const double* p = tq_grp_sums(tq_grp_row(a, nrows, ncol, g));
#pragma unroll
    for (int j = 0; j < TQ_MAX_NGSUM; ++j)
      if (j < nq) acc[j] += ldd(p + j);
  }
  TQ_STAMP_AT(a, TQ_ST_TAIL_SUMS);
  tq_sums_finish(a, acc, s_w);
  return true;
}
// ... for the tail workgroup of a sampling launch, which waits for them and goes on to the global sites: ends as
// tq_rows_sums_body does
__device__ __forceinline__ bool tq_groups_sums_fenced_body(const tq_cosmos_args& a, double (*s_w)[TQ_MAX_NGSUM]) {
  if (!tq_groups_sums_body<true>(a, s_w)) return false;
  __threadfence_block();
  __syncthreads();
  TQ_STAMP_AT(a, TQ_ST_GSUM);
  return true;
}

// AOI-sharded full-batch steps (and tq_cosmos_tail): rows -> per-AOI sites and gsum, what the all-reduce needs.  Workgroup g
// adds the rows of group g (one wave, one round trip) and publishes the group row; the workgroup whose ticket is the last
// one finishes the per-AOI sites and the cross-unit sums from the U / 4096 group rows (one wave per AOI and a last
// workgroup that walked all 6250 rows took 38 us at c2 -- on the critical path of every sharded step).
__global__ __launch_bounds__(256) void tq_group_sums_kernel(const tq_cosmos_args a) {
  __shared__ double s_w[4][TQ_MAX_NGSUM];
  __shared__ int s_last;
  if (threadIdx.x < 64) {
    const int ticket = tq_group_reduce_rows(a, (int)blockIdx.x);
    if (threadIdx.x == 0) s_last = ticket == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  tq_groups_sums_body<false>(a, s_w);
}

__global__ __launch_bounds__(256) void tq_rows_reduce_globals_kernel(const tq_cosmos_args a, const int upr) {
  __shared__ double s_w[4][TQ_MAX_NGSUM];
  __shared__ double s_e[TQ_NGSITES(TQ_MAXQ)];
  if (upr <= 20) tq_rows_sums_body<16>(a, s_w, upr);
  else tq_rows_sums_body<TQ_UNIT_BLOCK>(a, s_w);
  tq_globals_from_gsum_body(a, s_e);
}

// Full-batch pipeline (tq_cosmos_step_overlapped): the local guide sampling of step t, with ONE extra workgroup (block (0, 0),
// dispatched first) that runs the single-workgroup tail of step t-1 -- cross-unit sums, global sites, total ELBO, Adam
// of the per-AOI / global parameters -- and then draws the global sites of step t from the updated parameters.  The
// sampling of the local sites reads local parameters only (already updated by the Adam fused into the unit kernel of
// step t-1), so the ~35 us latency chain of the tail hides behind the ~14 000 sampling workgroups of the same launch.
// Compiled for the occupancy of the SAMPLING path (five waves per SIMD, 96 registers; the fp64 code of the global sites
// spills ~800 registers to scratch at that cap, which the one tail workgroup can afford now that the other workgroups of
// its grid row add the rows for it: with the tail adding all rows itself it was the last workgroup of the launch and the
// kernel had to be built for three waves -- c2 step 0.248 -> 0.235 ms, 0.320 -> 0.288 ms in the regime of a converged fit).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void tq_sample_locals_tail_kernel(
    const tq_cosmos_args a, const tq_cosmos_args prev, const int has_prev, const int64_t B, const int site_begin) {
  // has_prev: a TqPrevTail code
  if (blockIdx.y == 0) {
    if (blockIdx.x != 0) {
      // workgroup 1 + g adds the rows of group g of `prev` for the tail workgroup (one wave; the others leave)
      if (has_prev == TQ_PREV_GROUPS && (int64_t)blockIdx.x <= tq_grp_count(tq_batch_units(prev)) && threadIdx.x < 64)
        tq_group_reduce_rows(prev, (int)blockIdx.x - 1);
      return;
    }
    __shared__ double s_w[4][TQ_MAX_NGSUM];
    __shared__ double s_e[TQ_NGSITES(TQ_MAXQ)];
    TQ_STAMP_AT(a, TQ_ST_TAIL_START);
    if (has_prev) {
      const int64_t Bp = tq_batch_units(prev);
      bool have_gsum = true;  // (TQ_PREV_REDUCED: from the start)
      if (has_prev == TQ_PREV_ROWS) tq_rows_sums_body<TQ_UNIT_BLOCK>(prev, s_w);
      else if (has_prev == TQ_PREV_GROUPS) have_gsum = tq_groups_sums_fenced_body(prev, s_w);
      else if (has_prev == TQ_PREV_FLAT) tq_reduce_sums_fenced_body(prev, (Bp + TQ_UNIT_BLOCK - 1) / TQ_UNIT_BLOCK, Bp, s_w);
      if (have_gsum) tq_globals_from_gsum_body(prev, s_e);
      else if (threadIdx.x == 0) prev.elbo_out[0] = __builtin_nan("");
      __syncthreads();
      TQ_STAMP_AT(a, TQ_ST_FB_GLOBALS);
      const int64_t total = tq_num_params(prev);
      for (int64_t j = tq_aoi_base(prev) + threadIdx.x; j < total; j += 256) tq_body_adam(prev, j);
      __threadfence();
      __syncthreads();
    }
    TQ_STAMP_AT(a, TQ_ST_AOI);
    const int ns = tq_num_gsites(a);
    if ((threadIdx.x & 63) == 0)
      for (int s = threadIdx.x >> 6; s < ns; s += 4) tq_body_sample_globals(a, s);
    TQ_STAMP_BARRIER();
    TQ_STAMP_AT(a, TQ_ST_TAIL_DRAWN);
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  tq_sample_site_wg(a, site_begin + (int)blockIdx.y - 1, i, B);
  TQ_STAMP_IF(blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1, a, TQ_ST_TAIL_ADAM);  // (about) the last sampling workgroup
}
