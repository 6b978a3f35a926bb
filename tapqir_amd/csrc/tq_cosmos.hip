// tq_cosmos.hip -- one cosmos SVI step around the pixel kernel of tq_ksmogn.hip (guide sampling, per-unit ELBO terms +
// gradients, per-AOI terms, cross-unit sums, global sites, dense Adam).  Replaces what pyro's SVI/TraceEnum_ELBO/optim.Adam
// execute for tapqir/models/model.py:212 -- see include/tapqir_hip.h.
//
// ONE translation unit.  This file is its host side: the predicates that pick a launch, the argument checks, every launch_*
// and extern "C" entry point, and the posterior read-out.  The kernels are in headers that only this file includes, one
// per launch family:
//   tq_step_staged.h     one kernel per stage of a step; the wave sums and single-workgroup bodies every tail shares
//   tq_rows.h            the rows of partial sums in blk_part, the format in which a step with rows hands its sums to its
//                        tail: widths, the writers of a row, the addresses a reader takes from a row or a group row
//   tq_step_rows.h       full-batch steps with rows: per-unit kernels that leave rows, group rows, the sampling launch that
//                        carries the pending tail of the previous step
//   tq_step_minibatch.h  the single-launch minibatch step
//   tq_beta_compact.h    one local guide site by one workgroup (all sampling launches), AffineBeta regime compaction
//   tq_stamps.h          words of tq_cosmos_args.sync, diagnostic stamps (scripts/build_stamps.sh)
// Per-item math is in tq_bodies.h (shared with the host checker); the likelihood routines in tq_ksmogn_dev.h / _il2.h.
//
// Map: what each route of CosmosEngine._route() (models/engine.py) launches, in order.  "likelihood" is launch_likelihood:
// tq_ksmogn_log_prob (tq_ksmogn.hip) or, for the crosstalk model, tq_ksmogn_crosstalk_log_prob (tq_xtalk.hip).
//
// "one_launch" -- tq_cosmos_minibatch_step: tq_minibatch_kernel (tq_step_minibatch.h) and nothing else.  It runs the pending
//   tail of the previous step, then catch-up, site draws, likelihood and per-unit terms + Adam of this one, and leaves rows
//   of 16 / 20 units.  Its own tail runs in the next such launch, or in tq_cosmos_tail: tq_rows_reduce_globals_kernel
//   (tq_step_rows.h), tq_adam_kernel (tq_step_staged.h).
//
// "overlapped" -- tq_cosmos_step_overlapped, after tq_cosmos_adam_catchup (tq_adam_catchup_kernel, tq_step_staged.h) for a
//   minibatch with the lazy Adam clock:
//     1. tq_sample_locals_tail_kernel (tq_step_rows.h): local draws of this step; one workgroup runs the pending tail of the
//        previous step (tq_prev_code_sampling says from what) and draws this step's global sites;
//     2. per-unit terms + Adam of the local parameters (elbo_grads_impl, sums not finished):
//          fused (tq_fused_pixel_unit):  tq_pixel_unit_kernel (tq_step_rows.h), rows of 64 units;
//          rows layout (tq_rows_layout):  likelihood, tq_unit_rows_kernel (tq_step_rows.h), rows of 256 units;
//          flat layout (the others):      likelihood, tq_unit_kernel, tq_aoi_kernel (tq_step_staged.h).
//   The tail stays pending for the next step's launch 1.  The last step's tail is tq_cosmos_tail: with rows,
//   tq_group_sums_kernel (tq_step_rows.h) then tq_tail_reduced_kernel (tq_step_staged.h); flat, tq_reduce_globals_kernel then
//   tq_adam_kernel (tq_step_staged.h); rows without a sync buffer, tq_rows_reduce_globals_kernel (tq_step_rows.h) then
//   tq_adam_kernel.
//
// "staged" -- tq_cosmos_step, everything in tq_step_staged.h for the minibatches with the dense Adam that take this route:
//   tq_sample_globals_kernel, tq_sample_locals_kernel, likelihood, tq_unit_kernel, tq_aoi_kernel, then tq_cosmos_tail:
//   tq_reduce_globals_kernel, tq_adam_kernel.  (A full batch passed here gets the rows kernels and the rows tail above.)
//
// "sharded" -- one entry point per stage, the caller all-reduces gsum between them:
//     1. tq_cosmos_sample_locals: tq_sample_locals_kernel, and tq_cosmos_sample_globals: tq_sample_globals_kernel
//        (tq_step_staged.h) -- or, with the previous step's all-reduce in flight, tq_cosmos_sample_locals_range:
//        tq_sample_locals_kernel for the first sites, tq_sample_locals_tail_kernel (tq_step_rows.h, TQ_PREV_REDUCED) for the
//        rest, which also runs the previous step's tail behind the all-reduce and this step's global draws;
//     2. tq_cosmos_elbo_grads: as 2. above, with the sums finished: tq_group_sums_kernel (tq_step_rows.h) after rows,
//        tq_reduce_kernel (tq_step_staged.h) after the flat layout;
//     3. (all-reduce of gsum) tq_cosmos_tail_reduced: tq_tail_reduced_kernel, then tq_adam_kernel unless the Adam of the
//        local parameters was fused (tq_step_staged.h).
//
// "streamed" -- per group of AOIs the stage entry points on a gathered batch, all in tq_step_staged.h:
//   tq_cosmos_sample_globals (first group), tq_cosmos_adam_catchup (lazy minibatches), tq_cosmos_sample_locals,
//   tq_cosmos_elbo_grads (flat layout: likelihood, tq_unit_kernel, tq_aoi_kernel, tq_reduce_kernel); the host adds the
//   groups' gsum and tq_cosmos_tail_reduced closes the step.
//
// tq_cosmos_globals_grad (tq_globals_grad_kernel, tq_elbo_finish_kernel), tq_cosmos_adam and tq_cosmos_pixel_unit expose
// single stages to tests and benchmarks; tq_cosmos_probs (the end of this file) is the posterior read-out.
#include <hip/hip_runtime.h>

#include "tq_bodies.h"
#include "tq_host.h"
#include "tq_ksmogn_dev.h"
#include "tq_rows.h"
#include "tq_step_minibatch.h"
#include "tq_step_rows.h"
#include "tq_step_staged.h"

// ---- host predicates: which layout, which launch, which pending tail ------------------------------------------------------
// Does this step leave its partial sums in the rows layout (tq_rows.h)?  Full batches with the fused Adam and at least
// TQ_UNIT_BLOCK units per AOI; the others keep the flat layout + tq_aoi_kernel.
static bool tq_rows_layout(const tq_cosmos_args& a) {
  return a.fuse_adam && !a.ndx && !a.fdx && a.nb == a.Nt && a.fb == a.F && a.F * a.C >= TQ_UNIT_BLOCK;
}

// Units per workgroup (= per row of partial sums) of the single-launch minibatch step: 16 or 20 (tq_step_minibatch.h: why).
static int tq_mb_upr(const tq_cosmos_args& a) {
  const int forced = tq_env_int("TAPQIR_AMD_MB_UNITS", 0);  // (read at every call: tests switch it inside one process)
  if ((int64_t)a.fb * a.C < 20 || forced == 16) return 16;
  if (forced == 20) return 20;
  const int64_t B = tq_batch_units(a);
  const int64_t r16 = ((B + 15) / 16 + 255) / 256, r20 = ((B + 19) / 20 + 255) / 256;
  return 17 * r20 < 13 * r16 ? 20 : 16;
}

// What the launch that carries the tail of `prev` finds in prev's workspace (enum TqPrevTail, tq_step_rows.h): rows of 16 or
// 20 units after a single-launch minibatch step, rows of 64 / 256 units after a step with the rows layout, else flat sums.
static TqPrevTail tq_prev_code(const tq_cosmos_args& prev) {
  if (prev.tail_kind == TQ_TAIL_ROWS16) return tq_mb_upr(prev) == 20 ? TQ_PREV_ROWS20 : TQ_PREV_ROWS16;
  return tq_rows_layout(prev) ? TQ_PREV_ROWS : TQ_PREV_FLAT;
}
// ... in a sampling launch whose grid rows have `grid_x` workgroups: rows of 64 / 256 units are added per group by the idle
// workgroups of the first grid row (tq_group_reduce_rows) where that row has one for every group
static TqPrevTail tq_prev_code_sampling(const tq_cosmos_args* prev, int64_t grid_x) {
  if (!prev) return TQ_PREV_NONE;
  const TqPrevTail code = tq_prev_code(*prev);
  return code == TQ_PREV_ROWS && prev->sync && tq_grp_count(tq_batch_units(*prev)) + 1 <= grid_x ? TQ_PREV_GROUPS : code;
}

// May this step run pixel + per-unit kernel as one launch (tq_pixel_unit_kernel)?  Asked for by pixel_mode; a cosmos step
// with the rows layout, K <= 2, one offset value, P of 14 or 20, the interleaved images and the pixel statistics, and enough
// units for the interleaved pixel routine.  CosmosEngine._fusable (models/engine.py) asks the same of an engine.
static bool tq_fused_pixel_unit(const tq_cosmos_args& a) {
  const int64_t B = tq_batch_units(a);
  return a.pixel_mode == TQ_PIXEL_FUSED_UNIT && tq_rows_layout(a) && !a.crosstalk && a.K <= 2 && a.O == 1 && a.pixstats &&
         a.images_il && (a.P == 14 || a.P == 20) && B >= a.il_min_units;
}

// ---------------------------------------------------------------------------------------------------------
static int check_args(const tq_cosmos_args* a) {
  if (a && a->pixel_mode != 0 && a->pixel_mode != TQ_PIXEL_FUSED_UNIT) {  // (first: refused whatever else the block holds)
    tq_set_error("tq_cosmos_*: pixel_mode must be 0 or TQ_PIXEL_FUSED_UNIT (the persistent form of the pixel kernel, pixel_mode = 1, was retired)");
    return TQ_ERR_ARG;
  }
  if (!a || !a->params || !a->globals || !a->gbase) {
    tq_set_error("tq_cosmos_*: NULL args/params/globals/gbase");
    return TQ_ERR_ARG;
  }
  if (a->K < 1 || a->K > TQ_MAX_K || a->P < 2 || a->P > TQ_MAX_P || a->C < 1 || a->C > TQ_MAXQ || a->nb < 1 ||
      a->fb < 1 || a->nb > a->Nt || a->fb > a->F || a->O < 1) {
    tq_set_error("tq_cosmos_*: unsupported K/P/C or inconsistent batch geometry");
    return TQ_ERR_ARG;
  }
  if (tq_num_units(*a) >= ((int64_t)1 << 31)) {
    tq_set_error("tq_cosmos_*: Nt*F*C must be below 2^31 (unit indices are 32-bit on the device)");
    return TQ_ERR_ARG;
  }
  if (a->images_by_slot && (a->crosstalk || !a->ndx)) {
    tq_set_error("tq_cosmos_*: images_by_slot (a streamed window of AOIs) needs the AOI list ndx of the batch; cosmos model only");
    return TQ_ERR_ARG;
  }
  if (a->crosstalk && (a->C != 2 || a->K > 2)) {
    tq_set_error("tq_cosmos_*: the crosstalk model is implemented for Q = C = 2 and K <= 2");
    return TQ_ERR_ARG;
  }
  return TQ_OK;
}

extern "C" int64_t tq_globals_size(void) { return (int64_t)sizeof(TqGlobals); }
extern "C" int64_t tq_gbase_size(void) { return (int64_t)sizeof(TqGlobalBase); }
extern "C" int64_t tq_cosmos_nblk(int64_t B) { return (B + TQ_UNIT_BLOCK - 1) / TQ_UNIT_BLOCK; }
extern "C" int64_t tq_cosmos_param_count(int32_t Nt, int32_t F, int32_t C, int32_t K) {
  return (int64_t)TQ_NLOCAL(K) * Nt * F * C + 2 * (int64_t)Nt * C + TQ_NGLOBAL(C);
}
extern "C" int64_t tq_crosstalk_param_count(int32_t Nt, int32_t F, int32_t C, int32_t K) {
  return (int64_t)TQ_NLOCAL(K) * Nt * F * C + 2 * (int64_t)Nt * C + TQ_NGLOBAL_X(C, 1);
}

extern "C" int tq_cosmos_sample_globals(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  hipLaunchKernelGGL(tq_sample_globals_kernel, dim3(tq_num_gsites(*a)), dim3(64), 0, (hipStream_t)stream, *a);
  return tq_launch_status("tq_sample_globals_kernel");
}

extern "C" int tq_cosmos_sample_locals(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (!a->lat || !a->site) {
    tq_set_error("tq_cosmos_sample_locals: lat or site is NULL");
    return TQ_ERR_ARG;
  }
  const int64_t B = tq_batch_units(*a);
  hipLaunchKernelGGL(tq_sample_locals_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)(1 + 4 * a->K)), dim3(256), 0,
                     (hipStream_t)stream, *a, B, 0);
  return tq_launch_status("tq_sample_locals_kernel");
}

// argument block of the likelihood kernel of a cosmos step: the one place that knows the row order of `lat` and `pix`
// (pix_end: the first row of `pix` behind the cosmos block, where the crosstalk model's rows follow)
static tq_ksmogn_args cosmos_ksmogn_args(const tq_cosmos_args* a, float** pix_end = nullptr) {
  const int K = a->K, M = 1 << K;
  const int64_t B = tq_batch_units(*a), U = tq_num_units(*a);
  tq_ksmogn_args k = {};
  k.images = a->images; k.images_il = a->images_il; k.xy = a->xy; k.ndx = a->ndx; k.fdx = a->fdx;
  k.images_il16 = a->images_il16;
  k.nb_full = a->Nt;
  k.pixstats = a->pixstats;
  k.stats_stride = U;
  k.il_min_units = a->il_min_units;
  k.background = a->lat;
  k.height = a->lat + (int64_t)1 * B;
  k.width = a->lat + (int64_t)(1 + K) * B;
  k.x = a->lat + (int64_t)(1 + 2 * K) * B;
  k.y = a->lat + (int64_t)(1 + 3 * K) * B;
  k.gain = &((const TqGlobals*)a->globals)->gain;
  k.offset_samples = a->offset_samples; k.offset_logits = a->offset_logits;
  k.gout = nullptr;
  k.m_logit = a->params;
  k.m_kstride = U;
  k.aoi_mask = a->aoi_mask;
  k.ll = a->pix;
  k.g_background = a->pix + (int64_t)M * B;
  k.g_gain = a->pix + (int64_t)(M + 1) * B;
  k.g_height = a->pix + (int64_t)(M + 2) * B;
  k.g_width = a->pix + (int64_t)(M + 2 + K) * B;
  k.g_x = a->pix + (int64_t)(M + 2 + 2 * K) * B;
  k.g_y = a->pix + (int64_t)(M + 2 + 3 * K) * B;
  if (pix_end) *pix_end = a->pix + (int64_t)(M + 2 + 4 * K) * B;
  k.nb = a->nb; k.fb = a->fb; k.C = a->C; k.F = a->F; k.P = a->P; k.K = K; k.O = a->O;
  k.scale = a->scale;
  k.images_by_slot = a->images_by_slot;
  return k;
}

// pixel kernel of a step: fused render + log-likelihood + pathwise gradients, Dice weights from m_probs
static int launch_likelihood(const tq_cosmos_args* a, void* stream) {
  const int64_t B = tq_batch_units(*a), U = tq_num_units(*a);
  float* pix_end;
  tq_ksmogn_args k = cosmos_ksmogn_args(a, &pix_end);
  if (a->crosstalk) {
    // one data site per AOI-frame, all dyes in every channel: per-dye marginal likelihoods go where the cosmos
    // per-unit routine expects ll, two more row groups follow the cosmos block of pix
    tq_xtalk_args x = {};
    x.images = a->images; x.xy = a->xy; x.ndx = a->ndx; x.fdx = a->fdx;
    x.images_il = a->images_il;  // crosstalk: interleaved (C, P, P) tiles per AOI-frame (tq_images_interleave_n)
    x.pixstats = a->pixstats; x.nb_full = a->Nt; x.il_min_units = a->il_min_units;
    x.background = k.background; x.height = k.height; x.width = k.width; x.x = k.x; x.y = k.y;
    x.gain = k.gain;
    x.alpha = &((const TqGlobals*)a->globals)->alpha[0][0];
    x.offset_samples = a->offset_samples; x.offset_logits = a->offset_logits;
    x.gout = nullptr; x.m_logit = a->params; x.m_kstride = U; x.aoi_mask = a->aoi_mask;
    x.ll_joint = nullptr; x.ll = a->pix;
    x.ell_excess = pix_end;  // one row, then C rows of g_alpha
    x.g_alpha = pix_end + B;
    x.g_background = k.g_background; x.g_gain = k.g_gain;
    x.g_height = k.g_height; x.g_width = k.g_width; x.g_x = k.g_x; x.g_y = k.g_y;
    x.nb = a->nb; x.fb = a->fb; x.C = a->C; x.F = a->F; x.P = a->P; x.K = a->K; x.O = a->O;
    x.scale = a->scale;
    return tq_ksmogn_crosstalk_log_prob(&x, stream);
  }
  return tq_ksmogn_log_prob(&k, stream);
}

// The (K, P, tile format) instances of tq_pixel_unit_kernel: runs `...` with the compile-time constants KK = K (1 or 2) and
// PP = P (14 or 20), which tq_fused_pixel_unit has checked (not TQ_SWITCH_K: the kernel exists for K <= 2 only), and
// FF = TQ_TILE_U16 where U16 says that the step brings the 16-bit copy of the tiles (images_il16), else TQ_TILE_F32
#define TQ_SWITCH_PU(K, P, U16, ...)                                                            \
  switch (4 * ((U16) != 0) + 2 * ((K) != 1) + ((P) != 14)) {                                    \
    case 0: { constexpr int KK = 1, PP = 14, FF = TQ_TILE_F32; __VA_ARGS__; } break;            \
    case 1: { constexpr int KK = 1, PP = 20, FF = TQ_TILE_F32; __VA_ARGS__; } break;            \
    case 2: { constexpr int KK = 2, PP = 14, FF = TQ_TILE_F32; __VA_ARGS__; } break;            \
    case 3: { constexpr int KK = 2, PP = 20, FF = TQ_TILE_F32; __VA_ARGS__; } break;            \
    case 4: { constexpr int KK = 1, PP = 14, FF = TQ_TILE_U16; __VA_ARGS__; } break;            \
    case 5: { constexpr int KK = 1, PP = 20, FF = TQ_TILE_U16; __VA_ARGS__; } break;            \
    case 6: { constexpr int KK = 2, PP = 14, FF = TQ_TILE_U16; __VA_ARGS__; } break;            \
    default: { constexpr int KK = 2, PP = 20, FF = TQ_TILE_U16; __VA_ARGS__; } break;           \
  }

// Split tiles of the fused launch (tq_step_rows.h).  Waves of the (K, P, tile format) instance that the device holds at a time:
// asked once.  The exported form answers for the fp32 tiles; the 16-bit instances are built to the same register counts
// (DESIGN.md section 4), and a launch that should find more slots than its caller sized pu_scratch for splits nothing.
static int32_t tq_pu_slots(int32_t K, int32_t P, bool u16) {
  static int cache[2][2][2] = {{{-1, -1}, {-1, -1}}, {{-1, -1}, {-1, -1}}};
  if (K < 1 || K > 2 || (P != 14 && P != 20)) return 0;
  int& slots = cache[u16][K - 1][P == 20];
  if (slots < 0) {
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e;
    TQ_SWITCH_PU(K, P, u16, e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tq_pixel_unit_kernel<KK, PP, FF>, 64, 0));
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return 0;  // (not cached: no device yet)
    }
    slots = per_cu * cus;
  }
  return slots;
}
extern "C" int32_t tq_cosmos_pu_slots(int32_t K, int32_t P) { return tq_pu_slots(K, P, false); }
// pu_split = -1: the last round of tiles, where it is at most an eighth full.  Below one full round nothing is split.
// Measured on 2048 slots: a split tile costs ~0.035 us of launch time and the round it removes ~11 us, so the
// split pays below ~320 tiles (r = 106: -7.6 us; r = 506, a quarter of the slots: +6 us); an eighth keeps a margin.
extern "C" int32_t tq_cosmos_pu_split_auto(int64_t ntiles, int32_t slots) {
  if (slots < 8 || ntiles < slots) return 0;
  const int64_t r = ntiles % slots;
  return r > 0 && r <= slots / 8 ? (int32_t)r : 0;
}
extern "C" int64_t tq_cosmos_pu_scratch_bytes(int32_t tiles) { return tiles > 0 ? tq_pu_scratch_bytes(tiles) : 0; }

// launch of the fused kernel; the caller has checked that the step qualifies (tq_fused_pixel_unit)
static int launch_pixel_unit(const tq_cosmos_args* a, void* stream) {
  const int64_t B = tq_batch_units(*a);
  const tq_ksmogn_args k = cosmos_ksmogn_args(a);
  const int64_t ntiles = (B + 63) / 64;
  const bool u16 = a->images_il16 != nullptr;  // the packed loop streams the 16-bit copy of the tiles
  int nsplit = 0;
  if (a->pu_split > 0) {
    nsplit = (int)(a->pu_split < ntiles ? a->pu_split : ntiles);
    if (!a->pu_scratch || nsplit > a->pu_scratch_tiles) {
      tq_set_error("tq_cosmos: pu_split = n needs pu_scratch with room for n tiles (tq_cosmos_pu_scratch_bytes)");
      return TQ_ERR_ARG;
    }
  } else if (a->pu_split < 0 && a->pu_scratch) {
    nsplit = tq_cosmos_pu_split_auto(ntiles, tq_pu_slots(a->K, a->P, u16));
    if (nsplit > a->pu_scratch_tiles) nsplit = 0;
  }
  const dim3 grid((unsigned)(ntiles + (TQ_PU_PARTS - 1) * (int64_t)nsplit)), block(64);
  hipStream_t st = (hipStream_t)stream;
  TQ_SWITCH_PU(a->K, a->P, u16, hipLaunchKernelGGL((tq_pixel_unit_kernel<KK, PP, FF>), grid, block, 0, st, k, *a, B, nsplit));
  return tq_launch_status("tq_pixel_unit_kernel");
}

// per-AOI sites + gsum of a step with rows, for callers that all-reduce gsum before the global sites (tq_group_sums_kernel)
static int launch_rows_sums(const tq_cosmos_args* a, hipStream_t st) {
  if (!a->sync || !a->aoi_part || !a->gsum) {
    tq_set_error("tq_cosmos_elbo_grads: the rows layout needs sync, aoi_part and gsum");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_group_sums_kernel, dim3((unsigned)tq_grp_count(tq_batch_units(*a))), dim3(256), 0, st, *a);
  return tq_launch_status("tq_group_sums_kernel");
}

// rows: AOI-aligned per-unit kernel whose tail also finishes the per-AOI sites (tq_unit_rows_kernel; full-batch steps
// that finish with tq_cosmos_tail or inside the next tq_cosmos_step_overlapped)
static int elbo_grads_impl(const tq_cosmos_args* a, void* stream, bool finish_sums, bool rows = false) {
  if (int rc = check_args(a)) return rc;
  if (!a->images || !a->xy || !a->is_ontarget || !a->offset_samples || !a->offset_logits || !a->grad || !a->lat ||
      !a->site || !a->pix || (!rows && !a->aoi_part) || !a->blk_part || !a->gsum) {
    tq_set_error("tq_cosmos_elbo_grads: NULL required pointer");
    return TQ_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = tq_batch_units(*a);
  if (a->pixel_mode == TQ_PIXEL_FUSED_UNIT) {  // pixel + per-unit kernel in one launch (rows of 64 units)
    if (!rows || !tq_fused_pixel_unit(*a)) {
      tq_set_error("tq_cosmos: pixel_mode = TQ_PIXEL_FUSED_UNIT needs a full-batch cosmos step with fused Adam, K <= 2, one "
                   "offset value, P in {14, 20}, the interleaved images and the pixel statistics");
      return TQ_ERR_ARG;
    }
    if (int rc = launch_pixel_unit(a, stream)) return rc;
    return finish_sums ? launch_rows_sums(a, st) : TQ_OK;
  }
  // 1. pixel kernel
  if (int rc = launch_likelihood(a, stream)) return rc;
  // 2. per-unit sites
  if (rows) {
    const dim3 grid((unsigned)tq_cosmos_nblk(B)), block(TQ_UNIT_BLOCK);
    TQ_SWITCH_K(a->K, hipLaunchKernelGGL((tq_unit_rows_kernel<KK>), grid, block, 0, st, *a, B));
    if (int rc = tq_launch_status("tq_unit_rows_kernel")) return rc;
    return finish_sums ? launch_rows_sums(a, st) : TQ_OK;
  }
  const int64_t nblk = tq_cosmos_nblk(B);
  const dim3 grid((unsigned)nblk), block(TQ_UNIT_BLOCK);
  TQ_SWITCH_K(a->K, hipLaunchKernelGGL((tq_unit_kernel<KK>), grid, block, 0, st, *a, B));
  if (int rc = tq_launch_status("tq_unit_kernel")) return rc;
  // 3. per-AOI sites
  hipLaunchKernelGGL(tq_aoi_kernel, dim3((unsigned)(a->nb * a->C)), dim3(256), 0, st, *a, B);
  if (int rc = tq_launch_status("tq_aoi_kernel")) return rc;
  // 4. cross-unit sums
  if (!finish_sums) return TQ_OK;
  hipLaunchKernelGGL(tq_reduce_kernel, dim3(1), dim3(256), 0, st, *a, nblk, B);
  return tq_launch_status("tq_reduce_kernel");
}

extern "C" int tq_cosmos_elbo_grads(const tq_cosmos_args* a, void* stream) {
  // full-batch steps with the Adam of the local parameters fused in take the rows layout here too (the per-AOI sites are
  // finished by tq_group_sums_kernel, which also leaves gsum ready for the caller's all-reduce)
  return elbo_grads_impl(a, stream, true, a && tq_rows_layout(*a) && a->sync && a->aoi_part);
}

extern "C" int tq_cosmos_pixel_unit(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (a->pixel_mode != TQ_PIXEL_FUSED_UNIT) {
    tq_set_error("tq_cosmos_pixel_unit: pixel_mode must be TQ_PIXEL_FUSED_UNIT");
    return TQ_ERR_ARG;
  }
  return elbo_grads_impl(a, stream, false, true);
}

extern "C" int tq_cosmos_globals_grad(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (!a->grad || !a->gsum || !a->elbo_out) {
    tq_set_error("tq_cosmos_globals_grad: NULL required pointer");
    return TQ_ERR_ARG;
  }
  // per-site ELBO parts go through the tail of the gsum buffer (gsum has 3+3Q used entries; the
  // caller allocates TQ_GSUM_LEN doubles)
  double* site_elbo = a->gsum + tq_num_gsum(*a);
  hipLaunchKernelGGL(tq_globals_grad_kernel, dim3(tq_num_gsites(*a)), dim3(64), 0, (hipStream_t)stream, *a, site_elbo);
  if (int rc = tq_launch_status("tq_globals_grad_kernel")) return rc;
  hipLaunchKernelGGL(tq_elbo_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a, (const double*)site_elbo);
  return tq_launch_status("tq_elbo_finish_kernel");
}

extern "C" int tq_cosmos_adam(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (!a->grad || !a->exp_avg || !a->exp_avg_sq) {
    tq_set_error("tq_cosmos_adam: NULL required pointer");
    return TQ_ERR_ARG;
  }
  const int64_t total = tq_num_params(*a);
  // with fuse_adam the local block was already updated by the per-unit kernel
  const int64_t first = a->fuse_adam ? tq_aoi_base(*a) : 0;
  int64_t nblk = (total - first + 255) / 256;
  if (nblk > 256 * 16) nblk = 256 * 16;  // grid-stride: 16 workgroups per CU
  hipLaunchKernelGGL(tq_adam_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, *a, first, total);
  return tq_launch_status("tq_adam_kernel");
}

extern "C" int tq_cosmos_adam_catchup(const tq_cosmos_args* a, int32_t all_units, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (!a->last_step || !a->exp_avg || !a->exp_avg_sq) {
    tq_set_error("tq_cosmos_adam_catchup: NULL required pointer (last_step, exp_avg, exp_avg_sq)");
    return TQ_ERR_ARG;
  }
  const int64_t n = all_units ? tq_num_units(*a) : tq_batch_units(*a);
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)TQ_NLOCAL(a->K));
  hipLaunchKernelGGL(tq_adam_catchup_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a, n, (int)all_units);
  return tq_launch_status("tq_adam_catchup_kernel");
}

// ---- whole steps ---------------------------------------------------------------------------------------------
static int launch_reduce_globals(const tq_cosmos_args* a, hipStream_t st) {
  if (!a->grad || !a->gsum || !a->elbo_out) {
    tq_set_error("tq_cosmos_step: NULL required pointer");
    return TQ_ERR_ARG;
  }
  // no all-reduce on this path: sums, (per-AOI sites,) global sites and the total ELBO finish in one launch
  if (a->tail_kind == TQ_TAIL_ROWS16 || tq_rows_layout(*a)) {
    hipLaunchKernelGGL(tq_rows_reduce_globals_kernel, dim3(1), dim3(256), 0, st, *a, a->tail_kind == TQ_TAIL_ROWS16 ? tq_mb_upr(*a) : TQ_UNIT_BLOCK);
    return tq_launch_status("tq_rows_reduce_globals_kernel");
  }
  const int64_t B = tq_batch_units(*a);
  hipLaunchKernelGGL(tq_reduce_globals_kernel, dim3(1), dim3(256), 0, st, *a, tq_cosmos_nblk(B), B);
  return tq_launch_status("tq_reduce_globals_kernel");
}

extern "C" int tq_cosmos_tail(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (a->tail_kind != TQ_TAIL_ROWS16 && tq_rows_layout(*a) && a->fuse_adam && a->sync && a->aoi_part) {
    // rows of 64 or 256 units: the per-AOI frame sums span up to F C / 64 rows each -- added per group of 4096 units
    // (tq_group_sums_kernel) instead of by one workgroup walking all of them, then the global sites + tail Adam
    if (int rc = launch_rows_sums(a, (hipStream_t)stream)) return rc;
    return tq_cosmos_tail_reduced(a, nullptr, stream);
  }
  if (int rc = launch_reduce_globals(a, (hipStream_t)stream)) return rc;
  return tq_cosmos_adam(a, stream);
}

extern "C" int tq_cosmos_tail_reduced(const tq_cosmos_args* a, const tq_cosmos_args* next, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (next)
    if (int rc = check_args(next)) return rc;
  if (!a->grad || !a->gsum || !a->elbo_out || !a->exp_avg || !a->exp_avg_sq) {
    tq_set_error("tq_cosmos_tail_reduced: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (next && !a->fuse_adam) {
    tq_set_error("tq_cosmos_tail_reduced: the next step's global draws need this step's Adam to be complete (fuse_adam steps only)");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_tail_reduced_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *a, next ? *next : *a, next ? 1 : 0);
  if (int rc = tq_launch_status("tq_tail_reduced_kernel")) return rc;
  return a->fuse_adam ? TQ_OK : tq_cosmos_adam(a, stream);
}

extern "C" int tq_cosmos_step(const tq_cosmos_args* a, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (int rc = tq_cosmos_sample_globals(a, stream)) return rc;
  if (int rc = tq_cosmos_sample_locals(a, stream)) return rc;
  if (int rc = elbo_grads_impl(a, stream, false, tq_rows_layout(*a))) return rc;
  return tq_cosmos_tail(a, stream);
}

extern "C" int tq_cosmos_step_overlapped(const tq_cosmos_args* a, const tq_cosmos_args* prev, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (prev)
    if (int rc = check_args(prev)) return rc;
  if (!a->fuse_adam || (prev && !prev->fuse_adam)) {
    tq_set_error("tq_cosmos_step_overlapped: full-batch steps with fuse_adam only (the next step's local sampling must not depend on the pending tail)");
    return TQ_ERR_ARG;
  }
  if (!a->lat || !a->site || !a->grad || !a->gsum || !a->elbo_out || !a->exp_avg || !a->exp_avg_sq ||
      (prev && (!prev->grad || !prev->gsum || !prev->elbo_out || !prev->exp_avg || !prev->exp_avg_sq || !prev->blk_part ||
                (!tq_rows_layout(*prev) && !prev->aoi_part)))) {
    tq_set_error("tq_cosmos_step_overlapped: NULL required pointer");
    return TQ_ERR_ARG;
  }
  const int64_t B = tq_batch_units(*a);
  if (prev && prev->tail_kind == TQ_TAIL_ROWS16) {
    // (a pending single-launch minibatch step: its rows-of-16 tail is not carried by the sampling launch, whose register
    // allocation every extra tail variant burdens)
    if (int rc = tq_cosmos_tail(prev, stream)) return rc;
    prev = nullptr;
  }
  const int64_t gx = (B + 255) / 256;
  hipLaunchKernelGGL(tq_sample_locals_tail_kernel, dim3((unsigned)gx, (unsigned)(2 + 4 * a->K)), dim3(256), 0,
                     (hipStream_t)stream, *a, prev ? *prev : *a, (int)tq_prev_code_sampling(prev, gx), B, 0);
  if (int rc = tq_launch_status("tq_sample_locals_tail_kernel")) return rc;
  return elbo_grads_impl(a, stream, false, tq_rows_layout(*a));
}

extern "C" int64_t tq_cosmos_blk_floats(int32_t Nt, int32_t F, int32_t C, int32_t crosstalk, int64_t B) {
  const int64_t ncol = tq_row_floats(TQ_NGSUM_X(C, crosstalk));
  const int64_t full = (((int64_t)Nt * F * C + 63) / 64) * ncol;                             // full-batch rows of 256 or 64 units
  const int64_t mini = ((B + TQ_UNITS_PER_BLOCK - 1) / TQ_UNITS_PER_BLOCK) * ncol;          // single-launch minibatch step: rows of 16
  const int64_t flat = tq_cosmos_nblk(B) * TQ_NGSUM_X(C, crosstalk);
  const int64_t grp = tq_grp_floats((int64_t)Nt * F * C);                                    // group rows behind the full-batch rows
  const int64_t most = full > mini ? (full > flat ? full : flat) : (mini > flat ? mini : flat);
  return most + grp;
}

extern "C" int tq_cosmos_minibatch_step(const tq_cosmos_args* a, const tq_cosmos_args* prev, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (prev)
    if (int rc = check_args(prev)) return rc;
  if (a->crosstalk || !a->fuse_adam || (prev && !prev->fuse_adam) || (int64_t)a->fb * a->C < TQ_UNITS_PER_BLOCK) {
    tq_set_error("tq_cosmos_minibatch_step: cosmos steps with fuse_adam and at least 16 units per AOI only");
    return TQ_ERR_ARG;
  }
  if (!a->images || !a->xy || !a->is_ontarget || !a->offset_samples || !a->offset_logits || !a->lat || !a->site || !a->pix ||
      !a->blk_part || !a->gsum || !a->elbo_out || !a->exp_avg || !a->exp_avg_sq || !a->grad || !a->sync ||
      (prev && (!prev->grad || !prev->gsum || !prev->elbo_out || !prev->exp_avg || !prev->exp_avg_sq || !prev->blk_part ||
                (tq_prev_code(*prev) == TQ_PREV_FLAT && !prev->aoi_part)))) {
    tq_set_error("tq_cosmos_minibatch_step: NULL required pointer");
    return TQ_ERR_ARG;
  }
  const int64_t B = tq_batch_units(*a);
  const tq_ksmogn_args k = cosmos_ksmogn_args(a);
  const bool one = a->O == 1 && a->pixstats;
  // one workgroup per 16 (or 20: tq_mb_upr) units + the one that runs the tail and the global draws
  const int upr = tq_mb_upr(*a);
  const dim3 grid((unsigned)((B + upr - 1) / upr) + 1), block(256);
  const int tail_last = tq_env_int("TAPQIR_AMD_MB_TAIL_LAST", 1) != 0 && grid.x > 1 && (grid.x - 1) % 256 == 0 && grid.x <= 513;  // (<= 2 workgroups per CU: all resident)
  size_t lds = sizeof(float) * tq_tile16_lds_floats(a->P, a->K, a->O, TQ_UNITS_PER_BLOCK, !one);
  if (a->next_ndx || a->next_fdx) {
    if ((a->next_ndx && a->Nt > TQ_SUBSAMPLE_MAX) || (a->next_fdx && a->F > TQ_SUBSAMPLE_MAX)) {
      tq_set_error("tq_cosmos_minibatch_step: next_ndx / next_fdx need Nt, F <= TQ_SUBSAMPLE_MAX");
      return TQ_ERR_ARG;
    }
    if (lds < TQ_SUBSAMPLE_LDS) lds = TQ_SUBSAMPLE_LDS;
  }
  const int code = prev ? tq_prev_code(*prev) : TQ_PREV_NONE;
  const tq_cosmos_args& pv = prev ? *prev : *a;
  hipStream_t st = (hipStream_t)stream;
  TQ_SWITCH_K(a->K,
    if (upr == 20) {
      if (one) hipLaunchKernelGGL((tq_minibatch_kernel<KK, true, 20>), grid, block, lds, st, *a, pv, code, k, B, tail_last);
      else hipLaunchKernelGGL((tq_minibatch_kernel<KK, false, 20>), grid, block, lds, st, *a, pv, code, k, B, tail_last);
    } else {
      if (one) hipLaunchKernelGGL((tq_minibatch_kernel<KK, true, 16>), grid, block, lds, st, *a, pv, code, k, B, tail_last);
      else hipLaunchKernelGGL((tq_minibatch_kernel<KK, false, 16>), grid, block, lds, st, *a, pv, code, k, B, tail_last);
    });
  return tq_launch_status("tq_minibatch_kernel");
}

// The subsample of a minibatch step by itself: the routine the tail workgroup of tq_minibatch_kernel runs, in a launch of
// one workgroup.
__global__ __launch_bounds__(256) void tq_subsample_draw_kernel(const uint64_t seed, const uint32_t step, const uint32_t site, const int n,
                                                                const int take, int32_t* out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  tq_draw_subsample((int*)smem, seed, step, site, n, take, out);
}

extern "C" int tq_subsample_draw(uint64_t seed, uint32_t step, int32_t axis, int32_t n, int32_t take, int32_t* out, void* stream) {
  if (!out) {
    tq_set_error("tq_subsample_draw: NULL out");
    return TQ_ERR_ARG;
  }
  if (axis != 0 && axis != 1) {
    tq_set_error("tq_subsample_draw: axis must be 0 (AOIs) or 1 (frames)");
    return TQ_ERR_ARG;
  }
  if (n < 1 || n > TQ_SUBSAMPLE_MAX || take < 1 || take > n) {
    tq_set_error("tq_subsample_draw: need 1 <= take <= n <= TQ_SUBSAMPLE_MAX");
    return TQ_ERR_ARG;
  }
  hipLaunchKernelGGL(tq_subsample_draw_kernel, dim3(1), dim3(256), TQ_SUBSAMPLE_LDS, (hipStream_t)stream, seed, step,
                     axis == 0 ? TQ_SITE_SUBSAMPLE_N : TQ_SITE_SUBSAMPLE_F, (int)n, (int)take, out);
  return tq_launch_status("tq_subsample_draw_kernel");
}

// AOI-sharded pipeline: the local sites [site_begin, site_begin + site_count) of `a`; with `prev` (whose gsum the caller
// has all-reduced) the launch also carries, as one extra workgroup, everything of `prev` after the all-reduce and the
// global draws of `a` (tq_cosmos_tail_reduced(prev, a)).  A sharded host samples the first sites of step t+1 while the
// all-reduce of step t is in flight, waits for it, and calls this with `prev` for the remaining sites.
extern "C" int tq_cosmos_sample_locals_range(const tq_cosmos_args* a, int32_t site_begin, int32_t site_count,
                                             const tq_cosmos_args* prev, void* stream) {
  if (int rc = check_args(a)) return rc;
  if (prev)
    if (int rc = check_args(prev)) return rc;
  if (!a->lat || !a->site || site_begin < 0 || site_count < 1 || site_begin + site_count > 1 + 4 * a->K) {
    tq_set_error("tq_cosmos_sample_locals_range: bad site range or NULL lat/site");
    return TQ_ERR_ARG;
  }
  if (prev && (!prev->fuse_adam || !prev->grad || !prev->gsum || !prev->elbo_out || !prev->exp_avg || !prev->exp_avg_sq)) {
    tq_set_error("tq_cosmos_sample_locals_range: prev must be a full-batch (fuse_adam) step with grad/gsum/elbo_out/moments");
    return TQ_ERR_ARG;
  }
  const int64_t B = tq_batch_units(*a);
  const unsigned gx = (unsigned)((B + 255) / 256);
  if (prev) {
    hipLaunchKernelGGL(tq_sample_locals_tail_kernel, dim3(gx, (unsigned)(site_count + 1)), dim3(256), 0, (hipStream_t)stream, *a,
                       *prev, (int)TQ_PREV_REDUCED, B, (int)site_begin);
    return tq_launch_status("tq_sample_locals_tail_kernel");
  }
  hipLaunchKernelGGL(tq_sample_locals_kernel, dim3(gx, (unsigned)site_count), dim3(256), 0, (hipStream_t)stream, *a, B,
                     (int)site_begin);
  return tq_launch_status("tq_sample_locals_kernel");
}

// ---- posterior read-out (cosmos.compute_probs) -------------------------------------------------------------
__global__ __launch_bounds__(64) void tq_probs_globals_kernel(const tq_probs_args a) {
  if (threadIdx.x == 0) tq_body_probs_globals(a, blockIdx.x, blockIdx.y);
}

template <int K>
__global__ __launch_bounds__(256) void tq_probs_kernel(const tq_probs_args a, const int64_t U) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u < U) tq_body_probs_unit<K>(a, u);
}

extern "C" int tq_cosmos_probs(const tq_probs_args* a, void* stream) {
  if (!a || !a->params || !a->is_ontarget || !a->globals_p || !a->gbase_p || !a->z_probs || !a->theta_probs ||
      (!a->draw && !a->xy_given)) {
    tq_set_error("tq_cosmos_probs: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->K < 1 || a->K > TQ_MAX_K || a->C < 1 || a->C > TQ_MAXQ || a->particles < 1 || a->particles > 65535) {
    tq_set_error("tq_cosmos_probs: unsupported K/C/particles");
    return TQ_ERR_ARG;
  }
  if (a->n_offset < 0) {
    tq_set_error("tq_cosmos_probs: n_offset < 0");
    return TQ_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tq_probs_globals_kernel, dim3(TQ_NGSITES(a->C), a->particles), dim3(64), 0, st, *a);
  if (int rc = tq_launch_status("tq_probs_globals_kernel")) return rc;
  const int64_t U = (int64_t)a->Nt * a->F * a->C;
  const dim3 grid((unsigned)((U + 255) / 256)), block(256);
  TQ_SWITCH_K(a->K, hipLaunchKernelGGL((tq_probs_kernel<KK>), grid, block, 0, st, *a, U));
  return tq_launch_status("tq_probs_kernel");
}
