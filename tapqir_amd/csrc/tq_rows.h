// tq_rows.h -- part of the translation unit tq_cosmos.hip: the rows of partial sums in tq_cosmos_args.blk_part, the one data
// format through which every step with rows hands its sums from the kernels that produce them (tq_step_rows.h,
// tq_step_minibatch.h) to the tail that consumes them.  This file owns the format: its widths, the writers of a row, the
// address of everything a reader takes from a row or a group row.  Nothing else computes an offset into blk_part of such a
// step (the flat layout of tq_unit_kernel, nq floats per workgroup, is tq_step_staged.h's own).
// =============================================================================================================
// Rows.  The units (f, c) of an AOI are contiguous, so a row of UPR consecutive units touches at most TWO AOIs when an AOI
// has at least UPR units: the row carries, next to the cross-unit sums of its units, the sums of
// d/d(background_mean_loc, background_std_loc) over its units of the first AOI (slot 0) and of the second (slot 1).  The
// tail adds the few rows that overlap an AOI itself, so there is no per-AOI kernel (5 us + a launch boundary at 400 000
// units) and no aoi_part round trip (16 B per unit).  Rows start at multiples of UPR units, not at AOIs: workgroups stay
// 1 KiB-aligned in every parameter row (AOI-aligned workgroups start at n * F * C and straddle cache lines: 9 % slower,
// measured).
//   row r = [2 slots][TQ_MAXQ channels](s1, s2)  [nq cross-unit sums]          tq_row_floats(nq) floats, at r * that
// Fixed offsets, whatever C and nq are, keep every register-array index a compile-time constant; columns of channels
// >= C are written as zeros and never read.
//
// Units per row (UPR) is not stored in the format; three places know it.  The host: tq_mb_upr (tq_cosmos.hip), 16 or 20
// for the single-launch minibatch step, which reaches the device as a TqPrevTail code or a kernel argument.  The device:
// tq_rows_upr (tq_step_rows.h), 64 after the fused pixel + per-unit kernel and TQ_UNIT_BLOCK after tq_unit_rows_kernel,
// and tq_mb_rows_upr (tq_step_rows.h), which decodes the TqPrevTail code.  The functions here take it as an argument.
//
// Group rows: the tail's sums, spread over the otherwise idle workgroups of the sampling launch.
// At c2 the fused launch leaves 6250 rows (one per wave).  The single-workgroup tail that adds them is a guest of the next
// step's sampling launch, and under that launch's memory traffic each of its ~17 dependent round trips (per-AOI frame
// sums: 16 rows per AOI, two AOIs per thread; cross-unit sums: 25 rows per thread) takes ~2.5 us: the sums alone kept it
// busy for 50 of its 84 us, which made it the last workgroup of the launch.  The grid row of that launch that holds the
// tail workgroup has B / 256 workgroups of which only the first did anything: now workgroup 1 + g of that row adds the rows
// of GROUP g (4096 units: 64 rows of 64 units or 16 of 256) -- one lane per row, one round trip -- and leaves a group row:
// the cross-unit sums in double and the per-AOI frame sums of the (at most 17) AOIs the group touches, published with
// write-through (`sc1`) stores, a drained store queue and an agent-scope counter (MI355X_MICROARCH.md, inter-workgroup
// visibility).  The tail workgroup polls the counter, then reads U / 4096 group rows with `sc1` loads: one round trip for
// the cross-unit sums, one for the per-AOI sums (stamps build: sums complete 9 us after its start instead of 50).  The
// reducers never wait, so the polling workgroup cannot deadlock.
//   group row g = [16 doubles: cross-unit sums][TQ_GRP_AOIS AOIs][TQ_MAXQ channels](s1, s2)       TQ_GGROW floats
// AOI m of a group row is the m-th AOI counted from the AOI of the group's first unit.  The group rows follow the rows in
// blk_part, 16-byte aligned (tq_grp_base).
// =============================================================================================================
#pragma once
#include <hip/hip_runtime.h>

#include "tq_bodies.h"
#include "tq_step_staged.h"

#define TQ_ROWS_AOICOL (2 * TQ_MAXQ)                      /* floats of a slot */
#define TQ_ROWS_GCOL (2 * TQ_ROWS_AOICOL)                 /* where the cross-unit sums begin */
#define TQ_ROWS_MAXCOL (TQ_ROWS_GCOL + TQ_MAX_NGSUM)      /* the widest row */
#define TQ_GRP_UNITS 4096
#define TQ_GRP_AOIS (TQ_GRP_UNITS / TQ_UNIT_BLOCK + 1)    /* AOIs a group can touch (F * C >= TQ_UNIT_BLOCK) */
#define TQ_GRP_DCOL (2 * 16)                              /* floats taken by the 16 doubles of a group row */
#define TQ_GGROW (TQ_GRP_DCOL + TQ_GRP_AOIS * 2 * TQ_MAXQ) /* floats of a group row */
#define TQ_GRP_ALIGN 4                                    /* floats: the group rows start 16-byte aligned */
static_assert(TQ_MAX_NGSUM <= 16, "a group row holds 16 cross-unit sums");

// ---- widths (host and device) ----------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int tq_row_floats(int nq) { return TQ_ROWS_GCOL + nq; }
__host__ __device__ __forceinline__ int64_t tq_grp_count(int64_t B) { return (B + TQ_GRP_UNITS - 1) / TQ_GRP_UNITS; }
__host__ __device__ __forceinline__ int64_t tq_grp_base(int64_t nrows, int ncol) {
  return ((nrows * ncol + TQ_GRP_ALIGN - 1) / TQ_GRP_ALIGN) * TQ_GRP_ALIGN;
}
// what the group rows of a step of B units take behind its rows, the alignment included
__host__ __device__ __forceinline__ int64_t tq_grp_floats(int64_t B) { return TQ_GRP_ALIGN + tq_grp_count(B) * TQ_GGROW; }

// ---- which units a group holds -----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t tq_grp_rows(uint32_t upr) { return TQ_GRP_UNITS / upr; }
__device__ __forceinline__ uint32_t tq_grp_first_unit(uint32_t g) { return g * TQ_GRP_UNITS; }
__device__ __forceinline__ uint32_t tq_grp_last_unit(uint32_t g, int64_t B) {
  const uint32_t u_first = tq_grp_first_unit(g);
  return (uint32_t)(((int64_t)u_first + TQ_GRP_UNITS - 1 < B - 1) ? u_first + TQ_GRP_UNITS - 1 : B - 1);
}
__device__ __forceinline__ uint32_t tq_grp_of_unit(uint32_t u) { return u / TQ_GRP_UNITS; }

// ---- the slot rule ---------------------------------------------------------------------------------------------------
// Slot 0 of a row holds the AOI of the row's first unit, slot 1 the AOI after it (upa: units per AOI of the batch; AOIs by
// their position in the batch).  Two steps, because a writer's first AOI is uniform over the row and worked out once.
__device__ __forceinline__ uint32_t tq_row_first_aoi(uint32_t first_unit, uint32_t upa) { return first_unit / upa; }
// the slot of AOI n (of unit i: n = i / upa) in a row whose first AOI is n0; the row must overlap the AOI
__device__ __forceinline__ int tq_row_slot(uint32_t n0, uint32_t n) { return n == n0 ? 0 : 1; }

// ---- writers ---------------------------------------------------------------------------------------------------------
// What one lane adds to its row: part[TQ_MAX_NGSUM], the cross-unit sums of its unit (tq_body_unit), and a TqRowAoi: the
// unit's two per-AOI partials at (slot, channel), zeros elsewhere.  (Two arrays, not one struct: as members of one object
// they cost tq_unit_rows_kernel<4> a register.)
typedef float TqRowAoi[TQ_ROWS_GCOL];
__device__ __forceinline__ void tq_row_clear(float* aoi) {
#pragma unroll
  for (int j = 0; j < TQ_ROWS_GCOL; ++j) aoi[j] = 0.0f;
}
__device__ __forceinline__ void tq_row_fill(float* aoi, const int slot, const int c, const float* aoi2) {
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
#pragma unroll
    for (int q = 0; q < TQ_MAXQ; ++q) {
      const bool mine = sl == slot && q == c;
      aoi[sl * TQ_ROWS_AOICOL + 2 * q] = mine ? aoi2[0] : 0.0f;
      aoi[sl * TQ_ROWS_AOICOL + 2 * q + 1] = mine ? aoi2[1] : 0.0f;
    }
  }
}
// row r from the 256 threads of a workgroup (s_part: its shared scratch; every thread calls)
__device__ __forceinline__ void tq_row_store_wg(const tq_cosmos_args& a, float (*s_part)[TQ_ROWS_MAXCOL], const int64_t r,
                                                const float* aoi, const float* part) {
  const int nq = tq_num_gsum(a), ncol = tq_row_floats(nq);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < TQ_ROWS_GCOL; ++j) {
    if ((j % TQ_ROWS_AOICOL) < 2 * a.C) {
      const float sum = tq_wave_sum_rows4(aoi[j]);
      if (lane == 0) s_part[wave][j] = sum;
    }
  }
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) {
    if (j < nq) {
      const float sum = tq_wave_sum_rows4(part[j]);
      if (lane == 0) s_part[wave][TQ_ROWS_GCOL + j] = sum;
    }
  }
  __syncthreads();
  if (tid < ncol) {
    const bool used = tid >= TQ_ROWS_GCOL || (tid % TQ_ROWS_AOICOL) < 2 * a.C;
    const float sum = used ? (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]) : 0.0f;
    a.blk_part[r * ncol + tid] = sum;
  }
}
// row r from a workgroup of one wave
__device__ __forceinline__ void tq_row_store_wave(const tq_cosmos_args& a, const int64_t r, const float* aoi, const float* part) {
  const int nq = tq_num_gsum(a), ncol = tq_row_floats(nq);
  float* row = a.blk_part + r * ncol;
#pragma unroll
  for (int j = 0; j < TQ_ROWS_GCOL; ++j) {
    const bool used = (j % TQ_ROWS_AOICOL) < 2 * a.C;
    const float sum = used ? tq_wave_sum_rows4(aoi[j]) : 0.0f;
    if (threadIdx.x == 0) row[j] = sum;
  }
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) {
    if (j < nq) {
      const float sum = tq_wave_sum_rows4(part[j]);
      if (threadIdx.x == 0) row[TQ_ROWS_GCOL + j] = sum;
    }
  }
}

// ---- readers: addresses only, the caller chooses the load ----------------------------------------------------------------
// (ncol = tq_row_floats(nq) of the step)
__device__ __forceinline__ float* tq_row(const tq_cosmos_args& a, const int ncol, const int64_t r) { return a.blk_part + r * ncol; }
// the (s1, s2) pairs of the channels of a slot of a row: pair c at [2 c], [2 c + 1]
__device__ __forceinline__ float* tq_row_slot_pairs(float* row, const int slot) { return row + slot * TQ_ROWS_AOICOL; }
// the (s1, s2) pair that row r holds for (AOI ai of the batch, channel c); the row must overlap the AOI
__device__ __forceinline__ const float* tq_row_aoi_pair(const tq_cosmos_args& a, const int ncol, const uint32_t r, const uint32_t ai,
                                                        const int c, const uint32_t upr, const uint32_t upa) {
  const int slot = tq_row_slot(tq_row_first_aoi(r * upr, upa), ai);
  return a.blk_part + (int64_t)r * ncol + slot * TQ_ROWS_AOICOL + 2 * c;
}
// cross-unit sum j of row r
__device__ __forceinline__ float& tq_row_sum(const tq_cosmos_args& a, const int ncol, const int64_t r, const int j) {
  return a.blk_part[r * ncol + TQ_ROWS_GCOL + j];
}
// group row g of a step with `nrows` rows; its cross-unit sums; its (s1, s2) pair of (its AOI m, channel c)
__device__ __forceinline__ float* tq_grp_row(const tq_cosmos_args& a, const int64_t nrows, const int ncol, const int64_t g) {
  return a.blk_part + tq_grp_base(nrows, ncol) + g * TQ_GGROW;
}
__device__ __forceinline__ double* tq_grp_sums(float* grow) { return (double*)grow; }
__device__ __forceinline__ float* tq_grp_aoi_pair(float* grow, const uint32_t m, const int c) {
  return grow + TQ_GRP_DCOL + m * (2 * TQ_MAXQ) + 2 * c;
}
// which AOI of group row g the AOI ai of the batch is
__device__ __forceinline__ uint32_t tq_grp_aoi_index(const uint32_t g, const uint32_t ai, const uint32_t upa) {
  return ai - tq_row_first_aoi(tq_grp_first_unit(g), upa);
}
