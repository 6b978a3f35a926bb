// tq_stamps.h -- part of the translation unit tq_cosmos.hip, included from its headers only: the words of
// tq_cosmos_args.sync and the diagnostic stamps.  The sync words and the TQ_MB_* stamps serve the two kernels that run a
// pending tail inside another launch (tq_sample_locals_tail_kernel in tq_step_rows.h, tq_minibatch_kernel in
// tq_step_minibatch.h); the bodies those tails share (tq_step_staged.h, tq_step_rows.h) carry the TQ_STAMP_* ones.
#pragma once
#include <hip/hip_runtime.h>

// ---- words of tq_cosmos_args.sync (TQ_SYNC_WORDS int32) -------------------------------------------------------------
// [0] tickets, [1] first flag and [2] count-out of a minibatch launch; from word 4 the 64-bit stamp slots of a diagnostic
// build (below); and:
#define TQ_SYNC_LOST 63    /* workgroups that gave up waiting for a flag, ever (diagnostics; never observed) */
#define TQ_SYNC_GAIN 62    /* the gain of a minibatch launch (float bits), published with the first flag */
#define TQ_SYNC_FLAG2 61   /* second flag of a minibatch launch: the global draws after the gain */
#define TQ_SYNC_CLAIM 60   /* word that names the workgroup running the tail of a minibatch launch (tail_last) */
#define TQ_SYNC_GROUPS 40  /* counts the finished groups of the group rows */

// Diagnostic stamps (scripts/build_stamps.sh: -DTQ_MB_STAMPS=<workgroup> -DTQ_MB_STAMPS_SITES=<0|1>): thread 0 of a workgroup
// writes the 100 MHz clock into a 64-bit slot behind word 4 of `sync`.  The macros are empty in the normal build.  Slots, as
// the readers index them (scripts/mb_dev_time.py: minibatch launch; scripts/fb_tail_time.py: sampling launch of a full batch;
// scripts/mb_timeline.py reads a kernel trace, no slot):
enum TqStampSlot {
  // workgroup TQ_MB_STAMPS of tq_minibatch_kernel (mb_dev_time.py: differences of 0..5, 6 and 7 against 0)
  TQ_ST_START = 0, TQ_ST_CATCHUP = 1, TQ_ST_SITES = 2, TQ_ST_GAIN = 3, TQ_ST_PIXEL = 4, TQ_ST_UNIT = 5, TQ_ST_TICKET = 6,
  TQ_ST_PHASE1 = 7,
  // the tail workgroup.  mb_dev_time.py: start / sums + global gradients / Adam / second flag.  fb_tail_time.py: start / group
  // rows read / (about) the last sampling workgroup / global draws done
  TQ_ST_TAIL_START = 8, TQ_ST_TAIL_SUMS = 9, TQ_ST_TAIL_ADAM = 10, TQ_ST_TAIL_DRAWN = 11,
  TQ_ST_GSUM = 12,        // gsum complete (both readers)
  TQ_ST_AOI = 13,         // mb_dev_time.py: per-AOI sites of rows of 16 / 20 done; fb_tail_time.py: Adam done, global draws start
  TQ_ST_FB_GLOBALS = 7,   // fb_tail_time.py: global sites of the pending step done (the sampling launch has no TQ_ST_PHASE1)
  TQ_ST_MAXIMA = 16,      // 16..21 maxima over the grid of the phase times and the total, 22 (time << 32 | tq_where) of the slowest
  TQ_ST_TAIL_WHERE = 23,  // tq_where of the tail workgroup of a minibatch launch
  TQ_ST_DETAIL = 24,      // 24..27: inside the catch-up (mb_dev_time.py CATCHUP=1) or, with TQ_MB_STAMPS_SITES=1, gradient of
};                        // global site 0..3 done (SITES=1)
#ifdef TQ_MB_STAMPS
#define TQ_STAMP_SLOTS(a) ((uint64_t*)((a).sync + 4))
// (diagnostic) where a workgroup runs: XCC (4 bits) | SE, SH, CU of HW_ID (8 bits) | block (10 bits) | ticket (10 bits)
__device__ __forceinline__ unsigned long long tq_where(unsigned block, int ticket) {
  uint32_t hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  return ((unsigned long long)(xcc & 15) << 28) | (((hw >> 8) & 0xff) << 20) | ((block & 1023) << 10) | ((unsigned)ticket & 1023);
}
// any kernel: thread 0 stamps `slot` (if `cond`); TQ_STAMP_BARRIER: a barrier only the stamped build needs before a stamp
#define TQ_STAMP_IF(cond, a, slot) \
  do { if ((cond) && threadIdx.x == 0 && (a).sync) TQ_STAMP_SLOTS(a)[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TQ_STAMP_BARRIER() __syncthreads()
// lane 0 of a wave of the tail workgroup: gradient of global site s done
#define TQ_STAMP_SITE(a, s) \
  do { if (TQ_MB_STAMPS_SITES == 1 && (a).sync && (s) < 4) TQ_STAMP_SLOTS(a)[TQ_ST_DETAIL + (s)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// tq_minibatch_kernel (they use its `a`, `tid`, `s_ticket`): every worker keeps its own stamps, workgroup TQ_MB_STAMPS
// writes them out, and at the last one all add to the maxima over the grid
#define TQ_MB_STAMP_LOCALS uint64_t tq_tloc[8]
#define TQ_MB_STAMP(n)                                                                             \
  do { if (tid == 0) {                                                                             \
    tq_tloc[n] = __builtin_amdgcn_s_memrealtime();                                                 \
    if (blockIdx.x == TQ_MB_STAMPS) TQ_STAMP_SLOTS(a)[n] = tq_tloc[n];                             \
    if (n == TQ_ST_UNIT) {                                                                         \
      unsigned long long* mx = (unsigned long long*)TQ_STAMP_SLOTS(a) + TQ_ST_MAXIMA;              \
      for (int ph = 0; ph < 5; ++ph) atomicMax(mx + ph, (unsigned long long)(tq_tloc[ph + 1] - tq_tloc[ph])); \
      atomicMax(mx + 5, (unsigned long long)(tq_tloc[5] - tq_tloc[0]));                            \
      atomicMax(mx + 6, ((unsigned long long)(tq_tloc[5] - tq_tloc[0]) << 32) | tq_where(blockIdx.x, s_ticket)); \
    }                                                                                              \
  } } while (0)
#define TQ_MB_STAMP_DETAIL(n) \
  do { if (tid == 0 && blockIdx.x == TQ_MB_STAMPS) TQ_STAMP_SLOTS(a)[TQ_ST_DETAIL + n] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TQ_MB_TAIL_STAMP(n)                                                                        \
  do { if (tid == 0) {                                                                             \
    TQ_STAMP_SLOTS(a)[n] = __builtin_amdgcn_s_memrealtime();                                       \
    if (n == TQ_ST_TAIL_START) TQ_STAMP_SLOTS(a)[TQ_ST_TAIL_WHERE] = tq_where(blockIdx.x, s_ticket); \
  } } while (0)
#else
#define TQ_STAMP_IF(cond, a, slot) do {} while (0)
#define TQ_STAMP_BARRIER() do {} while (0)
#define TQ_STAMP_SITE(a, s) do {} while (0)
#define TQ_MB_STAMP_LOCALS do {} while (0)
#define TQ_MB_STAMP(n) do {} while (0)
#define TQ_MB_STAMP_DETAIL(n) do {} while (0)
#define TQ_MB_TAIL_STAMP(n) do {} while (0)
#endif
#define TQ_STAMP_AT(a, slot) TQ_STAMP_IF(true, a, slot)
