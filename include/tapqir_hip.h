/* tapqir_hip.h -- C ABI of libtapqir_hip.so, the MI355X (gfx950) implementation of the
 * cosmos SVI hot path of Tapqir.
 *
 * The reference has no FFI for this path (it is 100 % Python): the seam is
 * the Python class contract tapqir.models.Model / tapqir.distributions.KSMOGN.  Each entry
 * point below names the reference code it replaces; the Python host (tapqir_amd/) binds them
 * through ctypes (INTEGRATION.md shows the stub a maintainer would add to the reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller, contiguous, row-major, float32
 *     unless stated; nothing is allocated, freed or synchronised inside the library
 *   - every call is asynchronous on the caller's `stream` (a hipStream_t passed as void*)
 *   - return value: 0 = launched, nonzero = TQ_ERR_*; tq_last_error() gives the text
 *   - "unit" = one (AOI n, frame f, channel c) image of P x P pixels.  Minibatch units are
 *     numbered i = (a * fb + b) * C + c with n = ndx[a], f = fdx[b] (ndx/fdx may be NULL =
 *     identity); B = nb * fb * C.  Dataset-sized arrays use u = (n * F + f) * C + c.
 *   - spot arrays are K-major: [K][B] (minibatch) or [K][Nt*F*C] (dataset), as the reference's
 *     (K, Nt, F, Q) parameters (tapqir/models/cosmos.py:481-598)
 *   - enumerated spot-presence combinations are indexed mi in [0, 2^K), bit k of mi = m_k
 */
#ifndef TAPQIR_HIP_H
#define TAPQIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TQ_OK 0
#define TQ_ERR_ARG 1     /* invalid argument (shape, NULL pointer, unsupported K/P) */
#define TQ_ERR_LAUNCH 2  /* hipLaunch failed (text in tq_last_error) */

#define TQ_MAX_K 4
#define TQ_MAX_P 32
#define TQ_GSUM_LEN 32   /* doubles in tq_cosmos_args.gsum */

int tq_version(void);
const char* tq_last_error(void);

/* ---------------------------------------------------------------------------------------
 * KSMOGN image likelihood, forward and (optionally) backward in one pass.
 * Replaces: tapqir/distributions/ksmogn.py:146-238 (gaussians -> image -> concentration ->
 * log_prob; the KeOps Genred LogSumExp of 188-216) + tapqir/distributions/util.py:15-64
 * (gaussian_spots) + their autograd backward.
 *
 *   ll[mi][i] = sum_pixels log sum_o w_o Gamma(D - delta_o; (b + sum_{k in mi} spot_k)/g, 1/g)
 *
 * If the g_* outputs are non-NULL the kernel also returns the gradient of
 *   sum_mi gout[mi][i] * ll[mi][i]
 * with respect to background, height, width, x, y (per unit) and gain (per-unit partials,
 * to be summed by the caller).  The upstream weights are either given (`gout`) or built in
 * the kernel as the Dice weights of the cosmos guide:
 *   gout[mi][i] = scale * mask[n] * prod_k (m_k ? sigmoid(u_k) : sigmoid(-u_k)),
 *   u_k = m_logit[k * m_kstride + u]   (unconstrained `m_probs`, cosmos.py:419-424).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* images;         /* (Nt, F, C, P, P) */
  const float* images_il;      /* the same images in the 64-unit interleaved layout of tq_images_interleave, or
                                  NULL.  Used for contiguous batches (ndx == fdx == NULL, nb == nb_full, fb == F) */
  const float* pixstats;       /* [3][stats_stride] per-unit data statistics of tq_image_stats (dataset-indexed), or
                                  NULL.  With O == 1 they enable the single-offset formulation (tq_pixel.h) */
  const float* xy;             /* (Nt, F, C, 2) target locations (x, y) */
  const int32_t* ndx;          /* [nb] AOI indices or NULL */
  const int32_t* fdx;          /* [fb] frame indices or NULL */
  const float* background;     /* [B]    sampled background b */
  const float* height;         /* [K][B] sampled h */
  const float* width;          /* [K][B] sampled w */
  const float* x;              /* [K][B] sampled x */
  const float* y;              /* [K][B] sampled y */
  const float* gain;           /* [1]    sampled gain g (device scalar) */
  const float* offset_samples; /* [O] */
  const float* offset_logits;  /* [O] log weights */
  const float* gout;           /* [2^K][B] upstream weights, or NULL */
  const float* m_logit;        /* (K, Nt, F, C) unconstrained m_probs, used when gout == NULL */
  const uint8_t* aoi_mask;     /* [Nt] or NULL (all ones) */
  float* ll;                   /* [2^K][B] out */
  float* g_background;         /* [B]    out or NULL (forward only) */
  float* g_height;             /* [K][B] out */
  float* g_width;              /* [K][B] out */
  float* g_x;                  /* [K][B] out */
  float* g_y;                  /* [K][B] out */
  float* g_gain;               /* [B]    out: per-unit partial of d/d gain */
  int64_t m_kstride;           /* = Nt*F*C */
  int64_t stats_stride;        /* = Nt*F*C (row stride of pixstats) */
  int32_t nb, fb, C, F;        /* minibatch and dataset geometry */
  int32_t P, K, O;
  int32_t nb_full;             /* Nt of the dataset behind images_il */
  int32_t il_min_units;        /* use the interleaved kernel only for batches of at least this many units */
  float scale;                 /* plate scale (Nt/nb)(F/fb), used with m_logit */
  int32_t pixel_mode;          /* must be 0.  (1 used to select a persistent form of the backward kernel on the interleaved
                                  layout; that form was retired and any other value is now TQ_ERR_ARG) */
  int32_t images_by_slot;      /* 1: `images` holds only the AOIs of THIS batch, AOI number ai of the batch at
                                  images[ai * F * C * P * P] (a window of a data set that does not fit the device: the host
                                  streams the AOIs of a batch in, dataset.py:140-151 does the same per minibatch); every other
                                  array stays dataset-indexed.  Gathered batches (ndx given) of the 16-lane kernel */
  const uint16_t* images_il16; /* the 16-bit interleaved copy of tq_images_interleave_u16_n, or NULL (= fp32 tiles).  Read by the
                                  fused launch of a cosmos step only (tq_cosmos_args.images_il16); tq_ksmogn_log_prob ignores it */
} tq_ksmogn_args;

int tq_ksmogn_log_prob(const tq_ksmogn_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * KSMOGN likelihood of the crosstalk model (Q = C = 2 dyes / channels).
 * Replaces: the `alpha is not None` branch of tapqir/distributions/ksmogn.py:93-105, 146-165 as used by
 * tapqir/models/crosstalk.py:262-281: one observation per AOI-frame with event shape (C, P, P),
 *   image_c = b_c + sum_q alpha_qc sum_k m_qk h_qk N(x_qk + tx_c, y_qk + ty_c; w_qk),
 * for every joint spot-presence combination (bit q*K + k of the combination index = m_qk).
 * Units follow the cosmos layout: unit g*C + c of AOI-frame g carries background b_c and the spots of dye
 * q = c.  Outputs: the joint log-likelihoods (`ll_joint`), and/or, with `m_logit`, the per-dye marginals
 *   ll[mq][g*C + q] = sum_{m_-q} q(m_-q) ll_joint(m_q, m_-q)
 * that the cosmos per-unit routine consumes, plus `ell_excess` (the part of the ELBO those marginals count
 * more than once).  Backward as in tq_ksmogn_log_prob, with the extra output g_alpha.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* images;         /* (Nt, F, C, P, P) */
  const float* images_il;      /* tq_images_interleave_n(images, ., Nt*F, C*P*P): one (C, P, P) tile per AOI-frame, or NULL.
                                  With pixstats, O == 1 and a contiguous batch of at least il_min_units AOI-frames the
                                  packed lane-per-AOI-frame kernel runs */
  const float* pixstats;       /* [3][Nt*F*C] tq_image_stats of the (n, f, c) tiles, or NULL */
  const float* xy;             /* (Nt, F, C, 2) */
  const int32_t* ndx;          /* [nb] or NULL */
  const int32_t* fdx;          /* [fb] or NULL */
  const float* background;     /* [B]    B = nb*fb*C, unit g*C + c */
  const float* height;         /* [K][B] unit g*C + q */
  const float* width;
  const float* x;
  const float* y;
  const float* gain;           /* [1] */
  const float* alpha;          /* [Q*C] crosstalk fractions alpha[q][c] */
  const float* offset_samples; /* [O] */
  const float* offset_logits;  /* [O] */
  const float* gout;           /* [2^(QK)][nb*fb] upstream weights of the joint combinations, or NULL */
  const float* m_logit;        /* (K, Nt, F, Q) unconstrained m_probs: Dice weights and per-dye marginals */
  const uint8_t* aoi_mask;     /* [Nt] or NULL */
  float* ll_joint;             /* [2^(QK)][nb*fb] out or NULL */
  float* ll;                   /* [2^K][B] out or NULL (needs m_logit) */
  float* ell_excess;           /* [B] out or NULL */
  float* g_background;         /* [B] out or NULL (forward only) */
  float* g_height;             /* [K][B] */
  float* g_width;
  float* g_x;
  float* g_y;
  float* g_gain;               /* [B] per-unit partial (whole AOI-frame in unit c = 0) */
  float* g_alpha;              /* [Q][B]: row q, unit g*C + c = d/d alpha[q][c] */
  int64_t m_kstride;           /* = Nt*F*Q */
  int32_t nb, fb, C, F;
  int32_t P, K, O;
  int32_t nb_full;             /* Nt of the dataset behind images_il */
  int32_t il_min_units;        /* AOI-frames from which the packed kernel is used */
  float scale;
} tq_xtalk_args;

int tq_ksmogn_crosstalk_log_prob(const tq_xtalk_args* a, void* stream);

/* Tile-interleaved copy of the image tensor for the contiguous-batch kernel: units in blocks of 64,
 * pixels in groups of 4, so that a wave64 reads one contiguous 1 KiB row per load:
 *   out[((u / 64) * npix4 + q) * 64 + (u % 64)] = float4{ pixels 4q..4q+3 of unit u },  npix4 = ceil(P*P/4)
 * `out` must hold tq_interleaved_floats(U, P) floats. */
int64_t tq_interleaved_floats(int64_t U, int32_t P);
int tq_images_interleave(const float* images, float* images_il, int64_t U, int32_t P, void* stream);
/* the same for tiles of `npix` floats (crosstalk: one (C, P, P) tile per AOI-frame) */
int64_t tq_interleaved_floats_n(int64_t U, int32_t npix);
int tq_images_interleave_n(const float* images, float* images_il, int64_t U, int32_t npix, void* stream);
/* The same layout with 2 bytes per pixel, for images that are integers in [0, 65535] (camera counts: glimpse files hold
 * int16 + 2^15, the simulator floors): group q of four pixels of the 64 units of a block is one contiguous 512-byte row,
 *   out[(((u / 64) * npix4 + q) * 64 + (u % 64)) * 4 + e] = (uint16_t) pixel 4q + e of unit u,
 * padded as the fp32 copy is (zeros behind the last pixel and behind the last unit of the last block).  `out` must hold
 * tq_interleaved_u16_n(U, npix) uint16_t.  *inexact (a device word that the caller has zeroed) is set to 1 if any pixel v
 * fails v == (float)(uint16_t)v -- a fraction, a negative value, one above 65535, a NaN -- and is left alone otherwise;
 * the copy is then not a copy of the images and must not be used. */
int64_t tq_interleaved_u16_n(int64_t U, int32_t npix);
int tq_images_interleave_u16_n(const float* images, uint16_t* out, int64_t U, int32_t npix, int32_t* inexact, void* stream);

/* Per-unit data statistics for a single camera offset `offset[0]` (device scalar): with v = D - offset,
 *   pixstats[0][u] = sum_pix v,  pixstats[1][u] = sum_pix ln v,  pixstats[2][u] = #pixels with v <= 0
 * (a unit with such a pixel has log-likelihood -inf, ksmogn.py:226).  pixstats holds 3*U floats. */
int tq_image_stats(const float* images, const float* offset, float* pixstats, int64_t U, int32_t P, void* stream);

/* ---------------------------------------------------------------------------------------
 * One SVI step of the cosmos model = what `self.svi.step()` does at
 * tapqir/models/model.py:212 (pyro SVI + TraceEnum_ELBO(max_plate_nesting=3) over
 * cosmos.model / cosmos.guide, tapqir/models/cosmos.py:82-462, then pyro.optim.Adam,
 * model.py:169-171), split into stages so that a data-parallel host can put ONE all-reduce
 * of `gsum` between tq_cosmos_elbo_grads and tq_cosmos_globals_grad.
 *
 * Parameter storage.  All unconstrained parameters live in one flat float32 buffer
 *   params = [ local  : (8K+2) rows x U ]   U = Nt*F*C, row order:
 *                m_probs[k], h_loc[k], h_beta[k], w_mean[k], w_size[k], x_mean[k], y_mean[k],
 *                size[k]  (each K rows, k-major = the reference's (K,Nt,F,Q) tensors), b_loc, b_beta
 *            [ per-AOI: 2 rows x Nt*C ]     background_mean_loc, background_std_loc
 *            [ global : 4 + 5Q ]            gain_loc, gain_beta, proximity_loc, proximity_size,
 *                                           lamda_loc[Q], lamda_beta[Q], pi_mean[Q][2], pi_size[Q]
 * with the torch `transform_to(constraint)` maps of cosmos.py:471-598 (exp / sigmoid-affine /
 * exp+2 / softmax).  grad, exp_avg, exp_avg_sq have the same layout; `grad` receives
 * d ELBO / d param (Adam then descends on -ELBO).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  /* dataset (device) */
  const float* images;         /* (Nt, F, C, P, P) */
  const float* images_il;      /* interleaved copy (tq_images_interleave) or NULL */
  const float* pixstats;       /* [3][Nt*F*C] data statistics (tq_image_stats) when O == 1, else NULL */
  const float* xy;             /* (Nt, F, C, 2) */
  const uint8_t* is_ontarget;  /* [Nt] */
  const uint8_t* aoi_mask;     /* [Nt] or NULL */
  const int32_t* ndx;          /* [nb] or NULL */
  const int32_t* fdx;          /* [fb] or NULL */
  const float* offset_samples; /* [O] (host merges duplicate samples) */
  const float* offset_logits;  /* [O] */
  /* parameters and optimiser state (device, flat, see above) */
  float* params;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  /* workspace (device) */
  float* lat;                  /* [1+4K][B]        latent draws: b, h[K], w[K], x[K], y[K] */
  float* site;                 /* [5][(1+4K)*B]    per-site guide terms (log q, its derivatives w.r.t. the concentrations,
                                                   implicit reparameterisation gradients), same site order as lat */
  float* pix;                  /* [2^K+2+4K][B]    ll[2^K], g_b, g_gain, g_h[K], g_w[K], g_x[K], g_y[K]
                                                   (crosstalk: 1+Q more rows: ell_excess, g_alpha[Q]) */
  float* aoi_part;             /* [3][B]           per-unit d/d(bg mean, bg std) partials; row 2 = scratch */
  float* blk_part;             /* tq_cosmos_blk_floats() floats: per-workgroup partial sums, [nblk][3+3Q] (crosstalk:
                                                   3+3Q+Q*Q), or -- full-batch steps run by tq_cosmos_step /
                                                   tq_cosmos_step_overlapped -- [nblk][16 + 3+3Q(+Q*Q)] with the
                                                   per-AOI frame sums of the (at most two) AOIs a workgroup touches in front */
  double* gsum;                /* [TQ_GSUM_LEN]    cross-unit sums: d/d gain, d/d cs, ELBO, (d/d rho, a, c)[Q] in the
                                                   first 3+3Q entries (the part a data-parallel host
                                                   all-reduces); the tail is scratch of the library */
  void* globals;               /* TqGlobals  (tq_globals_size() bytes) */
  void* gbase;                 /* TqGlobalBase (tq_gbase_size() bytes): base draws of the global sites */
  double* elbo_out;            /* [1] ELBO of the step */
  /* geometry */
  int32_t Nt, F, C, P, K, O;
  int32_t nb, fb;
  int32_t n_offset;            /* global index of local AOI 0 (AOI sharding: RNG streams use global ids) */
  int32_t draw_globals;        /* 1: draw the global base variates; 0: use the contents of gbase */
  int32_t draw_locals;         /* 1: draw b, h, w, x, y; 0: use the contents of lat (parity tests) */
  int32_t il_min_units;        /* contiguous batches of at least this many units use the interleaved pixel kernel */
  float scale_n;               /* Nt_global / nb_global */
  float scale;                 /* scale_n * F / fb */
  float global_weight;         /* weight of the global ELBO part on this rank (1 on exactly one rank for reporting) */
  /* model constants */
  float eps;                   /* finfo(model dtype).eps */
  float width_min, width_max, height_std, background_mean_std, background_std_std;
  float gain_std, lamda_rate, proximity_rate;
  /* optimiser */
  float lr, beta1, beta2, adam_eps;
  float bias_correction1, bias_correction2;  /* 1 - beta^t for this step */
  int32_t zero_grad;           /* 1: Adam clears grad after use (minibatch mode keeps grad dense-zero) */
  int32_t fuse_adam;           /* 1: tq_cosmos_elbo_grads applies Adam to the local parameters of each unit of the
                                  batch right where their gradient is formed (no gradient round trip through HBM) and
                                  tq_cosmos_adam then updates only the per-AOI and global tail.  Full batches, or
                                  minibatches with `last_step` (lazy Adam, below) */
  int32_t crosstalk;           /* 1: the crosstalk model (tapqir/models/crosstalk.py; Q = C = 2, K <= 2): one data site per
                                  AOI-frame whose channel c sees every dye's spots scaled by alpha[q][c]; the global block
                                  of the parameter buffer grows by alpha_mean[Q][2], alpha_size[Q] (4+8Q entries), gsum
                                  by d/d alpha[q][c] (3+3Q+Q*Q entries) */
  /* RNG */
  uint64_t seed;
  uint32_t step;               /* number of completed steps: Philox key of this step's draws; this step is Adam step `step + 1` */
  /* lazy Adam of minibatch steps (tq_cosmos_adam_catchup) */
  int32_t* last_step;          /* [Nt*F*C] Adam step at which the local parameters of a unit were last updated, or NULL */
  double beta1_d, beta2_d;     /* the Adam betas in double: 1 - beta^s of the replayed steps is formed like the host's */
  int32_t pixel_mode;          /* 0: pixel kernel and per-unit kernel as two launches; TQ_PIXEL_FUSED_UNIT (2): see
                                  tq_cosmos_pixel_unit.  Any other value is TQ_ERR_ARG (1, the persistent pixel kernel, was retired) */
  int32_t tail_kind;           /* how the pending tail of THIS step finds its partial sums: TQ_TAIL_AUTO (what tq_cosmos_step /
                                  _step_overlapped / _elbo_grads wrote) or TQ_TAIL_ROWS16 (the step ran as
                                  tq_cosmos_minibatch_step); the host sets it on the struct it later passes as `prev` / to
                                  tq_cosmos_tail */
  int32_t* sync;               /* [TQ_SYNC_WORDS] zero-initialised device words, or NULL: [0..2] workgroup tickets, flag and completion count of
                                  tq_cosmos_minibatch_step; [3] completion ticket of the per-AOI sums of a full-batch step with
                                  rows (tq_cosmos_elbo_grads / tq_cosmos_tail; without `sync` those take the flat layout / the
                                  single-workgroup tail); [40] count of the row groups added inside the sampling launch of
                                  tq_cosmos_step_overlapped (without `sync` its tail workgroup adds all rows itself); [60..62] of
                                  tq_cosmos_minibatch_step: which workgroup runs the tail, the second flag (global draws after the
                                  gain) and the gain of the launch.  Every launch leaves the counters re-armed. */
  int32_t sync_value;          /* value the flag takes in this launch: any value different from the previous launch's on the
                                  same `sync` words (a launch counter of the host) */
  int32_t images_by_slot;      /* 1: `images` is a window holding the AOIs of this batch in batch order (tq_ksmogn_args.images_by_slot):
                                  data sets larger than the device memory, whose AOIs the host streams in group by group */
  int32_t* next_ndx;           /* tq_cosmos_minibatch_step: [nb] or NULL, and */
  int32_t* next_fdx;           /* [fb] or NULL -- the launch also draws the NEXT step's subsample, `randperm(Nt)[:nb]` /
                                  `randperm(F)[:fb]` of pyro.plate (cosmos.py:194-208), as the nb / fb smallest of Nt / F Philox
                                  keys (stream: seed, step + 1; a radix selection, no sort) in its tail workgroup, after the flags are published: a host that
                                  passes them as ndx / fdx of the next call never draws, stages or copies an index
                                  (Nt, F <= TQ_SUBSAMPLE_MAX: the index is a 16-bit field beside the key) */
  int32_t pu_split;            /* fused launch (TQ_PIXEL_FUSED_UNIT): tiles of 64 units split BY ROWS over four waves each, which are
                                  dispatched in front of the whole tiles; the wave of a tile that finishes last adds the four
                                  partial sums in a fixed order and goes on as the wave of a whole tile does, so nobody waits and the
                                  results do not depend on who arrives when.  -1: the last `ntiles mod slots` tiles where they
                                  would be a nearly empty last round (tq_cosmos_pu_split_auto; none without pu_scratch); 0: none;
                                  n > 0: the last n tiles (needs pu_scratch for n tiles) */
  int32_t pu_scratch_tiles;    /* split tiles that pu_scratch has room for */
  void* pu_scratch;            /* tq_cosmos_pu_scratch_bytes(pu_scratch_tiles) bytes, or NULL: one ticket counter per split tile,
                                  zeroed once by the caller and never reset (four tickets per tile and launch), then the
                                  partial sums [tile][part][value][lane] */
  const uint16_t* images_il16; /* fused launch (TQ_PIXEL_FUSED_UNIT): the 16-bit interleaved copy of the images
                                  (tq_images_interleave_u16_n, its flag read back as 0), or NULL.  Given, the packed pixel loop
                                  streams it instead of images_il -- 2 instead of 4 bytes per pixel, the same bits out, since a
                                  16-bit integer converts to fp32 exactly; images_il must be given all the same (the scalar loop
                                  of a tile with a small background / gain reads it).  Every other launch ignores it */
} tq_cosmos_args;
#define TQ_SUBSAMPLE_MAX 65536

#define TQ_TAIL_AUTO 0
#define TQ_TAIL_ROWS16 1
#define TQ_SYNC_WORDS 64
#define TQ_PIXEL_FUSED_UNIT 2      /* tq_cosmos_args.pixel_mode: pixel + per-unit kernel of a full-batch step in one launch */

int64_t tq_globals_size(void);
int64_t tq_gbase_size(void);
int64_t tq_cosmos_nblk(int64_t B);              /* rows of blk_part (flat layout) */
int64_t tq_cosmos_blk_floats(int32_t Nt, int32_t F, int32_t C, int32_t crosstalk, int64_t B);  /* floats blk_part must hold */
int64_t tq_cosmos_param_count(int32_t Nt, int32_t F, int32_t C, int32_t K);
int64_t tq_crosstalk_param_count(int32_t Nt, int32_t F, int32_t C, int32_t K);  /* + alpha_mean, alpha_size */

/* guide draws: globals (gain, pi, lamda, proximity) + derived tables; then, one lane per
 * (unit, site), b, h, w, x, y (cosmos.py:342-368, 408-462; torch Gamma/Beta rsample + pyro
 * AffineBeta clamp) together with log q of the draw, its derivatives and the implicit
 * reparameterisation gradient of the draw -- everything about a guide site that depends on that
 * site alone */
int tq_cosmos_sample_globals(const tq_cosmos_args* a, void* stream);
int tq_cosmos_sample_locals(const tq_cosmos_args* a, void* stream);
/* likelihood + all per-unit / per-AOI ELBO terms and gradients; fills grad (local + AOI parts) and gsum */
int tq_cosmos_elbo_grads(const tq_cosmos_args* a, void* stream);
/* global sites: chain gsum through the tables to the unconstrained global parameters; writes elbo_out */
int tq_cosmos_globals_grad(const tq_cosmos_args* a, void* stream);
/* dense Adam over the whole flat buffer (torch.optim.Adam semantics, model.py:169-171) */
int tq_cosmos_adam(const tq_cosmos_args* a, void* stream);
/* all of the above back to back */
int tq_cosmos_step(const tq_cosmos_args* a, void* stream);
/* Lazy Adam for minibatch steps.  torch.optim.Adam updates EVERY element at every step; for the units outside the
 * minibatch the gradient is zero and the update (m *= beta1, v *= beta2, p -= lr_s m / (sqrt(v / bc2_s) + eps)) depends on
 * the element's own state and the step number only, so it can be replayed later from registers instead of streaming the
 * whole parameter / moment buffers through HBM every step (28 B per element: 35 us at config c2, 1.1 ms at c3).
 * tq_cosmos_adam_catchup replays, for every local parameter of the units of the batch (all_units = 0) or of the whole
 * dataset (all_units = 1), the zero-gradient steps last_step[u] + 1 .. a->step.  A minibatch step with fuse_adam then
 * runs it before its local sampling; tq_cosmos_elbo_grads applies step a->step + 1 and records it in last_step.  Call it
 * with all_units = 1 before anything reads the buffers (it does not write last_step: the caller re-bases the clock). */
int tq_cosmos_adam_catchup(const tq_cosmos_args* a, int32_t all_units, void* stream);
/* Full-batch pipeline (fuse_adam steps).  The single-workgroup TAIL of a step -- cross-unit sums, global sites, total
 * ELBO, Adam of the per-AOI and global parameters (~35 us of latency on one CU) -- does not have to finish before the
 * NEXT step samples its local guide sites (they read local parameters only, already updated by the fused Adam).
 * tq_cosmos_step_overlapped(a, prev) runs [local sampling of a + tail of prev + global draws of a] in ONE launch (the
 * tail occupies one extra workgroup of the ~14 000), then the likelihood, per-unit and per-AOI kernels of `a`, and
 * leaves the tail of `a` pending: pass `a` as `prev` of the next call, or finish it with tq_cosmos_tail(a) before
 * reading elbo_out / the per-AOI and global parameters.  prev == NULL: nothing pending (first step). */
int tq_cosmos_step_overlapped(const tq_cosmos_args* a, const tq_cosmos_args* prev, void* stream);
int tq_cosmos_tail(const tq_cosmos_args* a, void* stream);
/* With a->pixel_mode = TQ_PIXEL_FUSED_UNIT, tq_cosmos_step / tq_cosmos_step_overlapped run the likelihood and the
 * per-unit terms + Adam of a full-batch step as ONE launch: a wave renders its tile of 64 units and goes on to the
 * per-unit routine of the same units with the pixel results in registers (the pixel phase is bound by VALU issue, the
 * per-unit phase by HBM: waves in different phases overlap).  Full-batch cosmos steps with fuse_adam, K <= 2, one offset
 * value, P in {14, 20}, images_il and pixstats given, F * C >= 256; anything else is refused (TQ_ERR_ARG).  Same results
 * as the two-launch form up to the order of the fp32 partial sums (rows of 64 units instead of 256).
 * tq_cosmos_pixel_unit is that launch alone (a stage export like tq_cosmos_elbo_grads: draws and global tables of `a`
 * must be in place; it applies the Adam step of the local parameters and leaves the rows for the tail). */
int tq_cosmos_pixel_unit(const tq_cosmos_args* a, void* stream);
/* Split tiles of that launch (tq_cosmos_args.pu_split).  tq_cosmos_pu_slots: waves of the (K, P) instance that the current
 * device holds at a time (occupancy x compute units; 0 if it cannot be asked).  tq_cosmos_pu_split_auto: the rule of
 * pu_split = -1 for a launch of `ntiles` tiles -- with r = ntiles mod slots, the last r tiles if ntiles >= slots and
 * 0 < r <= slots / 8, else none: a batch below one full round of waves is never split.  tq_cosmos_pu_scratch_bytes: size of
 * pu_scratch for `tiles` split tiles. */
int32_t tq_cosmos_pu_slots(int32_t K, int32_t P);
int32_t tq_cosmos_pu_split_auto(int64_t ntiles, int32_t slots);
int64_t tq_cosmos_pu_scratch_bytes(int32_t tiles);
/* Minibatch steps (the reference's default operating point is 10 AOIs x 512 frames = 5120 units, main.py:1428-1431) in
 * ONE launch: every workgroup takes 16 units (20 when that saves a round of workgroups on the chip's CUs) through lazy-Adam catch-up, guide-site draws, likelihood and per-unit terms + Adam; one more workgroup runs
 * the pending tail of `prev` (or nothing) and the global draws of `a` -- the gain first, which the others wait for before
 * their likelihood phase, the rest before their per-unit phase.  Same arithmetic, same RNG streams and same results as
 * tq_cosmos_adam_catchup + tq_cosmos_step_overlapped; the tail of `a` stays pending: pass `a` (with tail_kind =
 * TQ_TAIL_ROWS16) as `prev` of the next step of either kind or to tq_cosmos_tail.  cosmos model, fuse_adam,
 * fb * C >= 16; `sync` must point to TQ_SYNC_WORDS zero-initialised int32 (zeroed again by the host after a launch that was
 * torn down). */
int tq_cosmos_minibatch_step(const tq_cosmos_args* a, const tq_cosmos_args* prev, void* stream);
/* The subsample that launch draws, by itself (one workgroup running the same device routine): out[0..take) = the indices of
 * the `take` smallest of the n Philox keys of (seed, step, axis; element = index), ties broken by the index, listed
 * ascending by (index mod 256, index div 256).  axis 0: AOIs (what the launch of step `step - 1` writes to next_ndx with
 * n = Nt, take = nb), 1: frames (next_fdx, n = F, take = fb).  Replaces pyro.plate's subsample (cosmos.py:194-208);
 * a fit's subsamples can be reproduced from (seed, step) alone.  TQ_ERR_ARG, before anything touches the device, unless
 * out != NULL, axis in {0, 1} and 1 <= take <= n <= TQ_SUBSAMPLE_MAX. */
int tq_subsample_draw(uint64_t seed, uint32_t step, int32_t axis /* 0: AOIs, 1: frames */, int32_t n, int32_t take,
                      int32_t* out /* [take], device */, void* stream);

/* AOI-sharded runs: everything that follows the all-reduce of gsum (tq_cosmos_globals_grad + tq_cosmos_adam) in one
 * single-workgroup launch, plus -- if `next` is given (full-batch steps) -- the global draws of the next step
 * (tq_cosmos_sample_globals(next)), which need the global parameters this call updates. */
int tq_cosmos_tail_reduced(const tq_cosmos_args* a, const tq_cosmos_args* next, void* stream);
/* AOI-sharded pipeline: draw the local sites [site_begin, site_begin + site_count) of `a` (site order as in `lat`).
 * With `prev` != NULL -- a full-batch step whose gsum the caller has all-reduced -- the same launch carries, as one extra
 * workgroup, tq_cosmos_tail_reduced(prev, a): a sharded host draws the first sites of step t+1 while the all-reduce of
 * step t is in flight, waits for it, and passes `prev` with the remaining sites, so that neither the collective nor the
 * single-workgroup tail is exposed. */
int tq_cosmos_sample_locals_range(const tq_cosmos_args* a, int32_t site_begin, int32_t site_count,
                                  const tq_cosmos_args* prev, void* stream);


/* ---------------------------------------------------------------------------------------
 * Posterior read-out: Monte-Carlo estimate (`particles` joint guide draws) of p(z | .) and p(theta = k | .).
 * Replaces cosmos.compute_probs (tapqir/models/cosmos.py:609-672): for every particle the
 * global latents (pi, lamda, proximity) and the spot positions x_k, y_k are drawn from the guide,
 * r(z, theta | m) = softmax_{z,theta}[log p(z) p(theta|z) prod_k p(m_k|theta) (p(x_k|theta) p(y_k|theta))^{m_k}],
 * R(z, theta) = sum_m prod_k q(m_k) r(z, theta | m);  z_probs = mean_particles sum_theta R,
 * theta_probs[k] = mean_particles R(z=1, theta=k+1).  Off-target AOIs are left at zero, as in the reference.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* params;         /* flat unconstrained parameters (layout of tq_cosmos_args) */
  const uint8_t* is_ontarget;  /* [Nt] */
  void* globals_p;             /* [particles] TqGlobals (tq_globals_size() bytes each), workspace */
  void* gbase_p;               /* [particles] TqGlobalBase (tq_gbase_size() bytes each); input when draw == 0 */
  const float* xy_given;       /* [particles][2K][U] spot positions (x_0..x_{K-1}, y_0..y_{K-1}) when draw == 0, else NULL */
  float* z_probs;              /* (Nt, F, Q, 2) out */
  float* theta_probs;          /* (K, Nt, F, Q) out */
  int32_t Nt, F, C, P, K;
  int32_t particles;
  int32_t draw;                /* 1: draw latents from the guide; 0: use gbase_p / xy_given (parity tests) */
  float eps;
  uint64_t seed;
  int32_t n_offset;            /* global index of local AOI 0 (AOI sharding: the per-unit RNG streams use global unit ids,
                                * as the step's do); >= 0, 0 for an unsharded read-out */
} tq_probs_args;

int tq_cosmos_probs(const tq_probs_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * KSMOGN.rsample (tapqir/distributions/ksmogn.py:171-185), the sampler behind tapqir/utils/simulate.py:108-122:
 *   out[i, j, ic] = max(Gamma(mu / g, 1 / g), tiny) + offset_samples[odx],  odx ~ Categorical(offset_logits) per pixel,
 *   mu = background + sum_k height_k N(ic; x_k + tx, w_k) N(j; y_k + ty, w_k).
 * `height` carries the presence indicators (m_k h_k) and, for the crosstalk image of channel c, the fractions alpha_qc
 * (then K = Q K' spots per unit).  Draws are distributionally (not bitwise) those of torch: Philox4x32-10 +
 * Marsaglia-Tsang, one stream per pixel keyed by (seed, unit, pixel).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* height;         /* [K][B] */
  const float* width;          /* [K][B] */
  const float* x;              /* [K][B] */
  const float* y;              /* [K][B] */
  const float* xy;             /* [B][2] target locations */
  const float* background;     /* [B] */
  const float* gain;           /* [1] */
  const float* offset_samples; /* [O] */
  const float* offset_logits;  /* [O] */
  float* out;                  /* [B][P][P] */
  int64_t B;
  int32_t P, K, O;
  uint64_t seed;
} tq_rsample_args;

int tq_ksmogn_rsample(const tq_rsample_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Post-fit statistics of every unit (n, f, c): signal-to-noise ratio of each spot and chi2 of the fitted image.
 * Replaces snr_and_chi2 (tapqir/utils/stats.py:29-86) and the per-AOI host loop around it (stats.py:166-182):
 *   N_k      = N(ic; x_k + tx, w_k) N(j; y_k + ty, w_k)      with the posterior MEANS of the spot parameters
 *   snr[k]   = sum_ij (D - b - offset_mean) N_k / sqrt(offset_var + b gain)
 *   chi2     = mean_ij (D - (b + sum_k h_k N_k) - offset_mean)^2 / (b + sum_k h_k N_k)
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* images;         /* (Nt, F, C, P, P) */
  const float* xy;             /* (Nt, F, C, 2) */
  const float* height;         /* [K][U] posterior means, U = Nt*F*C */
  const float* width;          /* [K][U] */
  const float* x;              /* [K][U] */
  const float* y;              /* [K][U] */
  const float* background;     /* [U] */
  float* snr;                  /* [K][U] out */
  float* chi2;                 /* [U] out */
  int64_t U;
  int32_t P, K;
  float gain, offset_mean, offset_var;
} tq_snr_args;

int tq_snr_chi2(const tq_snr_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Credible intervals of the per-unit variational posteriors: the central interval of probability `ci` of
 *   TQ_INTERVAL_GAMMA        Gamma(concentration = p0 p1, rate = p1)                     p0 = loc,  p1 = beta
 *   TQ_INTERVAL_AFFINE_BETA  low + (high - low) Beta(c1, c0),                            p0 = mean, p1 = size
 *                            c1 = p1 (p0 - low) / (high - low), c0 = p1 (high - p0) / (high - low)
 * i.e. ll = quantile((1 - ci) / 2), ul = quantile((1 + ci) / 2), element by element, in double.
 * Replaces the LL / UL of background, height, width, x, y in compute_params (tapqir/models/cosmos.py:740-776), which
 * the reference takes on the host through torch_to_scipy_dist(...).interval (scipy.stats.gamma / beta).
 * The Gamma concentration is the fp32 product p0 * p1 upcast, as the reference forms it; everything after is double.
 * Elements outside the domain (non-finite, concentration <= 0, mean outside (low, high)) give NaN.
 * ------------------------------------------------------------------------------------- */
#define TQ_INTERVAL_GAMMA 0
#define TQ_INTERVAL_AFFINE_BETA 1

typedef struct {
  int32_t kind;     /* TQ_INTERVAL_* */
  const float* p0;  /* [n] loc  | mean */
  const float* p1;  /* [n] beta | size */
  double* ll;       /* [n] out (float64) */
  double* ul;       /* [n] out (float64) */
  int64_t n;
  double ci;        /* in (0, 1) */
  double low, high; /* TQ_INTERVAL_AFFINE_BETA only: finite, low < high */
} tq_interval_args;

int tq_credible_intervals(const tq_interval_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Time-to-first-binding kinetics (`tapqir ttfb`, tapqir/main.py:926-1147).
 *
 * tq_ttfb_sample replaces time_to_first_binding(z_sample(num_samples)) (tapqir/utils/imscroll.py:187-196,
 * tapqir/models/cosmos.py:706-709) without drawing the S x N x F Bernoullis: the frames are independent under q, so
 *   L[n, f] = sum_{j <= f} log1p(-p[n, j])        (double, left to right: log P(tau > f))
 *   tau[s, n] = first f with L[n, f] < log u[s, n], or F if there is none,
 * with u[s, n] the uniform of Philox stream (seed, s, site 0xA00, n) (tq_math.h).  Two launches: the prefix (one wave
 * per AOI) and the search (one lane per (s, n)).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of each AOI-frame, in [0, 1] */
  double* log_surv;            /* (N, F) out / workspace: L */
  float* tau;                  /* (S, N) out: integer-valued first-binding frames in [0, F] */
  int32_t N, F, S;
  uint64_t seed;
} tq_ttfb_sample_args;

int tq_ttfb_sample(const tq_ttfb_sample_args* a, void* stream);

/* tq_ttfb_fit replaces train(ttfb_model, ttfb_guide, lr, n_steps) of tapqir/utils/mle_analysis.py:11-105 (pyro SVI,
 * TraceEnum_ELBO, optim.Adam): S independent maximum-likelihood fits of the censored two-exponential mixture of Friedman
 * & Gelles (2015), one per row of `tau`.  Per row the unconstrained parameters are (log ka, log kns, logit Af); with
 * k0 = kns, k1 = ka + kns the log-likelihood is the sum of
 *   0 < tau < T: logaddexp(log Af + log k1 - k1 tau, log(1 - Af) + log k0 - k0 tau)
 *   tau == T:    logaddexp(log Af - k1 T, log(1 - Af) - k0 T)
 *   control:     0 < tauc < T: log kns - kns tauc;  tauc == T: -kns T
 * (tau == 0 contributes nothing) and Adam (torch.optim.Adam semantics, float32) descends on its negative.
 * `state` carries parameters and moments between launches: a launch runs Adam steps step0 + 1 .. step0 + n_steps, so a
 * fit in chunks is bitwise equal to one launch.  The caller initialises state (torch: log 0.001, log 0.001, logit 0.9,
 * zero moments).  One wave per row: tau is staged in LDS when N <= TQ_TTFB_LDS_POINTS and stage_lds != 0, read from
 * L2 every step otherwise. */
typedef struct {
  const float* tau;            /* (S, N) integer-valued data */
  const float* tauc;           /* (S, Nc) control data, or NULL (Nc = 0) */
  float* state;                /* (S, 9) in/out: log ka, log kns, logit Af, exp_avg[3], exp_avg_sq[3] */
  float* loss;                 /* (S) out or NULL: loss (-log-likelihood) at the last step of the launch, before its update */
  int32_t S, N, Nc;
  int32_t step0;               /* Adam steps completed before this launch */
  int32_t n_steps;             /* Adam steps of this launch (>= 1) */
  int32_t stage_lds;           /* 1: stage tau in LDS when it fits; 0: always read it from L2 */
  float Tmax;                  /* observation interval T */
  double lr, beta1, beta2, eps;
} tq_ttfb_fit_args;
#define TQ_TTFB_LDS_POINTS 8192
#define TQ_TTFB_STATE 9

int tq_ttfb_fit(const tq_ttfb_fit_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dwell-time kinetics (`tapqir dwelltime`, tapqir/main.py:1150-1384).
 *
 * tq_dwell_sample replaces count_intervals(z_sample(num_samples)[:, mask, :, c]) (tapqir/utils/imscroll.py:14-110,
 * tapqir/main.py:1222-1226) and the per-sample tables of bound_dwell_times / unbound_dwell_times (imscroll.py:113-141)
 * without storing the S x N x F raster: frame f of (s, n) is z = (u < p[n, f]) with u the f-th uniform of Philox stream
 * (seed, s, site 0xA01, n) (tq_math.h), and each row is walked into runs of equal labels as it is drawn.
 *   mode TQ_DWELL_COUNT: counts[s, n] = number of intervals of the row; every interior interval (low_or_high 0 / 1) of
 *     dwell time d adds 1 to hist_unbound[s, d] / hist_bound[s, d] (the caller zeroes both histograms).
 *   mode TQ_DWELL_EMIT: the same draws again; the intervals of row (s, n) are written at offsets[s, n] (the exclusive scan
 *     of counts in row-major (s, n) order) into the columns of `intervals` (TQ_DWELL_COLS, total) int32: posterior_sample,
 *     aoi, start_frame, stop_frame, dwell_time, low_or_high, z -- count_intervals' rows in its torch.nonzero order.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of each AOI-frame, in [0, 1] */
  int32_t* counts;             /* (S, N) out (COUNT) */
  int32_t* hist_bound;         /* (S, F) in/out (COUNT): interior bound runs by dwell time */
  int32_t* hist_unbound;       /* (S, F) in/out (COUNT): interior unbound runs by dwell time */
  const int64_t* offsets;      /* (S, N) in (EMIT): exclusive scan of counts */
  int32_t* intervals;          /* (TQ_DWELL_COLS, total) out (EMIT) */
  int64_t total;               /* EMIT: number of intervals (the column stride); writes beyond it are dropped */
  int32_t N, F, S;
  int32_t mode;                /* TQ_DWELL_COUNT or TQ_DWELL_EMIT */
  uint64_t seed;
} tq_dwell_sample_args;
#define TQ_DWELL_COUNT 0
#define TQ_DWELL_EMIT 1
#define TQ_DWELL_COLS 7

int tq_dwell_sample(const tq_dwell_sample_args* a, void* stream);

/* tq_dwell_fit replaces train(exp_model, exp_guide, lr, n_steps, data, K) of tapqir/utils/mle_analysis.py:11-35, 107-130
 * (pyro SVI, TraceEnum_ELBO, optim.Adam): S independent maximum-likelihood fits of a K-exponential mixture, one per
 * posterior sample.  Row s of the data is the CSR list (values[i], weights[i]), row_ptr[s] <= i < row_ptr[s + 1], of dwell
 * times t > 0 with their multiplicities; its log-likelihood is sum_i w_i log sum_j A_j k_j exp(-k_j t_i).  Per row the
 * unconstrained parameters are log k_j and softmax logits a_j (A = softmax(a)), and Adam (torch.optim.Adam semantics,
 * float32) descends on the negative log-likelihood.  `state` carries parameters and moments between launches: a launch runs
 * Adam steps step0 + 1 .. step0 + n_steps, so a fit in chunks is bitwise equal to one launch.  The caller initialises state
 * (the reference: k = logspace(-K + 1, 0, K), A = 1 / K, zero moments).  One wave per row: a row of at most
 * TQ_DWELL_LDS_PAIRS pairs is staged in LDS when stage_lds != 0, a longer one is read from L2 every step. */
typedef struct {
  const float* values;         /* (nnz) dwell times > 0 */
  const float* weights;        /* (nnz) multiplicities */
  const int64_t* row_ptr;      /* (S + 1) */
  float* state;                /* (S, 6 K) in/out: log k[K], a[K], exp_avg[2K], exp_avg_sq[2K] */
  float* loss;                 /* (S) out or NULL: loss (-log-likelihood) at the last step of the launch, before its update */
  int32_t S, K;                /* 1 <= K <= TQ_DWELL_KMAX */
  int32_t step0;               /* Adam steps completed before this launch */
  int32_t n_steps;             /* Adam steps of this launch (>= 1) */
  int32_t stage_lds;           /* 1: stage rows in LDS when they fit; 0: always read them from L2 */
  double lr, beta1, beta2, eps;
} tq_dwell_fit_args;
#define TQ_DWELL_KMAX 8
#define TQ_DWELL_LDS_PAIRS 2048

int tq_dwell_fit(const tq_dwell_fit_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Two-state rate estimates (`tapqir_amd rates`; tapqir/utils/imscroll.py:199-246, 278-317).
 *
 * tq_rates_count replaces the sums of association_rate / dissociation_rate over Bernoulli(p).sample() rasters
 * (imscroll.py:199-246 inside posterior_estimate / sample_and_bootstrap, 278-317) without storing the S x N x F raster.
 * Row (s, n) is the row of tq_dwell_sample: frame f is z = (u < p[n, f]) with u the f-th uniform of Philox stream
 * (seed, s, site 0xA01, n), so one seed gives both entry points the same rasters.  Over its F - 1 frame pairs
 *   counts[s, n, 0] = n01 = sum (1 - z_f) z_{f+1}      counts[s, n, 1] = n0 = sum (1 - z_f)
 *   counts[s, n, 2] = n10 = sum z_f (1 - z_{f+1})      counts[s, n, 3] = n1 = sum z_f = F - 1 - n0
 * (F = 1: four zeros).  A row is 16 bytes, 16-byte aligned, written by one store.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of each AOI-frame, in [0, 1] */
  int32_t* counts;             /* (S, N, TQ_RATES_COLS) out; 16-byte aligned */
  int32_t N, F, S;
  uint64_t seed;
} tq_rates_count_args;
#define TQ_RATES_COLS 4

int tq_rates_count(const tq_rates_count_args* a, void* stream);

/* tq_rates_estimate sums the rows of every sample and divides:
 *   totals[s, j] = sum_{i < N} counts[s, a(s, i), j]   (int64)
 *   estimand[s, 0] = kon = totals[s, 0] / totals[s, 1],  estimand[s, 1] = koff = totals[s, 2] / totals[s, 3]
 * as IEEE double division: a zero denominator gives NaN or inf, as the reference's division does.
 *   resample = 0: a(s, i) = i, every AOI once -- posterior_estimate(Bernoulli(p), association_rate) (imscroll.py:278-293).
 *   resample = 1: a(s, i) = (uint32_t)(((uint64_t)w * N) >> 32), w the first 32-bit word of Philox stream
 *     (seed, s, site 0xA02, i): N rows with replacement, a fresh draw per sample -- the 2-D analogue of
 *     sample_and_bootstrap (imscroll.py:296-317).  An index is off the uniform law by at most N / 2^32.
 * One wave per sample. */
typedef struct {
  const int32_t* counts;       /* (S, N, TQ_RATES_COLS) of tq_rates_count; 16-byte aligned */
  int64_t* totals;             /* (S, TQ_RATES_COLS) out */
  double* estimand;            /* (S, 2) out: kon, koff */
  int32_t N, S;
  int32_t resample;            /* 0: pooled; 1: bootstrap over AOIs */
  uint64_t seed;               /* resample = 1 only */
} tq_rates_estimate_args;

int tq_rates_estimate(const tq_rates_estimate_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Two-state hidden Markov smoothing of a fit's z posterior (`tapqir_amd smooth`; the post-hoc counterpart of z_probs /
 * z_sample of tapqir/models/hmm.py:628-633, 658-667).  One row is one on-target AOI of one channel: p[f] = the fit's
 * p(z = 1) of frame f, clamped into [TQ_SMOOTH_PMIN, 1 - TQ_SMOOTH_PMIN], and `prior` = the fit's prior pi in (0, 1).
 *   evidence  l_f = ((1 - p_f) / (1 - pi), p_f / pi)
 *   chain     A = [[1 - kon, kon], [koff, 1 - koff]],  rho = (1 - pi0, pi0),  theta = (kon, koff, pi0): 3 doubles in
 *             device memory, each read clamped into [TQ_SMOOTH_RMIN, 1 - TQ_SMOOTH_RMIN]
 * Every entry point returns TQ_ERR_ARG, before anything touches the device, for a NULL required pointer, N, F or S < 1,
 * F > TQ_SMOOTH_MAX_F, S > 65535 * 64, prior outside (0, 1) or counts not 16-byte aligned.
 *
 * tq_smooth_estep: scaled forward-backward of every row at theta.
 *   filt[n, f]  = a_f(1),  a_0 ~ rho o l_0,  a_f ~ (a_{f-1} A) o l_f  with normalisers c_f
 *   gamma[n, f] = p(z_f = 1 | all frames)  (gamma is also the kernel's scratch for a_f(0) between its two sweeps)
 *   rows[n]     = E n01, E n0, E n10, E n1 (the sums of the pair marginals xi_f(i, j), f < F - 1, in the column order of
 *                 tq_rates_count; F = 1: four zeros), loglik = sum_f log c_f, gamma_0(1)
 * ------------------------------------------------------------------------------------- */
#define TQ_SMOOTH_COLS 6
#define TQ_SMOOTH_PMIN 1e-6
#define TQ_SMOOTH_RMIN 1e-9
#define TQ_SMOOTH_MAX_F 65536
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of the fit */
  const double* theta;         /* (3) kon, koff, pi0; device memory */
  double* filt;                /* (N, F) out */
  double* gamma;               /* (N, F) out */
  double* rows;                /* (N, TQ_SMOOTH_COLS) out */
  int32_t N, F;
  double prior;
} tq_smooth_estep_args;

int tq_smooth_estep(const tq_smooth_estep_args* a, void* stream);

/* tq_smooth_mstep: sums the N rows of an E-step in a fixed order (bit-reproducible), stores the total loglik into
 * trace[it] and overwrites theta:  kon = sum E n01 / sum E n0,  koff = sum E n10 / sum E n1,  pi0 = mean gamma_0(1),
 * each clamped into [TQ_SMOOTH_RMIN, 1 - TQ_SMOOTH_RMIN]; a 0 / 0 quotient keeps the previous value.  One workgroup.
 * An EM run of I iterations is I pairs of launches on one stream; nothing in it needs the host. */
typedef struct {
  const double* rows;          /* (N, TQ_SMOOTH_COLS) of tq_smooth_estep */
  double* theta;               /* (3) in / out; device memory */
  double* trace;               /* trace[it] out: the total loglik at the theta the rows were computed with */
  int32_t N, it;
} tq_smooth_mstep_args;

int tq_smooth_mstep(const tq_smooth_mstep_args* a, void* stream);

/* tq_smooth_viterbi: the MAP path of every row under the same l, A and rho, in the log domain; a tie takes state 0.
 * back: scratch of 2 bits per frame, ((F + 15) / 16) * N 32-bit words. */
typedef struct {
  const float* p;              /* (N, F) */
  const double* theta;         /* (3); device memory */
  uint32_t* back;              /* scratch, ((F + 15) / 16) * N words */
  uint8_t* path;               /* (N, F) out: 0 / 1 */
  int32_t N, F;
  double prior;
} tq_smooth_viterbi_args;

int tq_smooth_viterbi(const tq_smooth_viterbi_args* a, void* stream);

/* tq_smooth_count: S posterior rasters of every row by forward filtering, backward sampling, and their transition counts.
 * With u_j the j-th uniform of Philox stream (seed, step = s, site 0xA03, elem = n), compared as a double:
 *   z_{F-1} = (u_0 < filt[F-1]),   z_f = (u_{F-1-f} < q_f(z_{f+1})),
 *   q_f(j) = a_f(1) A[1][j] / (a_f(1) A[1][j] + a_f(0) A[0][j]),  a_f = (1 - filt[f], filt[f]).
 * counts has the layout of tq_rates_count, so tq_rates_estimate consumes it unchanged. */
typedef struct {
  const double* filt;          /* (N, F) of tq_smooth_estep */
  const double* theta;         /* (3); device memory */
  int32_t* counts;             /* (S, N, TQ_RATES_COLS) out; 16-byte aligned */
  uint8_t* raster;             /* (S, N, F) out: 0 / 1; or NULL */
  int32_t N, F, S;
  uint64_t seed;
} tq_smooth_count_args;

int tq_smooth_count(const tq_smooth_count_args* a, void* stream);

/* tq_smooth_dwell: the rasters of tq_smooth_count walked into dwell-time intervals and first-binding frames as they are
 * drawn (`dwelltime --smooth`, `ttfb --smooth`); no raster is stored.
 * Row (s, n) is, bit for bit, the row tq_smooth_count draws for the same filt, theta and seed: the same Philox stream
 * (seed, step = s, site 0xA03, elem = n), the same order of draws (u_0 for frame F - 1, then downwards), the same
 * thresholds q_f, clamps of theta and double compare -- so one seed gives `smooth`, `dwelltime --smooth` and
 * `ttfb --smooth` the same rasters.  The outputs are those of tq_dwell_sample for such a raster:
 *   mode TQ_DWELL_COUNT: counts[s, n] = number of intervals of the row; every interior interval (low_or_high 0 / 1) of
 *     dwell time d adds 1 to hist_unbound[s, d] / hist_bound[s, d] (the caller zeroes both histograms); and, when tau is
 *     not NULL, tau[s, n] = the smallest f with z_f = 1, or F if there is none (time_to_first_binding,
 *     tapqir/utils/imscroll.py:187-196; what tq_ttfb_sample writes).
 *   mode TQ_DWELL_EMIT: the same draws again; the table `intervals` of tq_dwell_sample's EMIT, (sample, AOI) row-major and
 *     ascending in start_frame within a row.  The row is walked from its last frame, so the k-th run it closes is written
 *     at offsets[s, n] + counts[s, n] - 1 - k; a position outside [offsets[s, n], min(offsets[s, n] + counts[s, n], total))
 *     is dropped, never written.  total = 0 launches nothing.
 * TQ_ERR_ARG, before anything touches the device, for a NULL required pointer of the mode, N, F or S < 1,
 * F > TQ_SMOOTH_MAX_F, S > 65535 * 64, total < 0 or an unknown mode. */
typedef struct {
  const double* filt;          /* (N, F) of tq_smooth_estep */
  const double* theta;         /* (3); device memory */
  int32_t* counts;             /* (S, N) out (COUNT), in (EMIT) */
  int32_t* hist_bound;         /* (S, F) in/out (COUNT): interior bound runs by dwell time */
  int32_t* hist_unbound;       /* (S, F) in/out (COUNT): interior unbound runs by dwell time */
  float* tau;                  /* (S, N) out (COUNT): integer-valued first-binding frames in [0, F]; or NULL */
  const int64_t* offsets;      /* (S, N) in (EMIT): exclusive scan of counts */
  int32_t* intervals;          /* (TQ_DWELL_COLS, total) out (EMIT) */
  int64_t total;               /* EMIT: number of intervals (the column stride) */
  int32_t N, F, S;
  int32_t mode;                /* TQ_DWELL_COUNT or TQ_DWELL_EMIT */
  uint64_t seed;
} tq_smooth_dwell_args;

int tq_smooth_dwell(const tq_smooth_dwell_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Hidden Markov smoothing with several hidden states per observable class (`tapqir_amd smooth --unbound-states U
 * --bound-states B`): an aggregated chain of M = U + B <= TQ_HMM_MAX_STATES states.  States
 * 0 .. U - 1 are unbound (class 0), states U .. M - 1 bound (class 1); state i emits l_f(class(i)) with p, `prior`, the
 * clamp and l_f of the two-state section above.
 *   theta = (A row-major (M, M), rho (M)): M * M + M doubles in device memory.  Every kernel reads it floored at
 *           TQ_SMOOTH_RMIN entry by entry and renormalised row by row (A) and as a whole (rho).
 * Every entry point returns TQ_ERR_ARG, before anything touches the device, for a NULL required pointer, N, F or S < 1,
 * F > TQ_SMOOTH_MAX_F, S > 65535 * 64, U or B < 1, U + B > TQ_HMM_MAX_STATES, prior outside (0, 1) or counts not 16-byte
 * aligned.
 *
 * tq_hmm_estep: scaled forward-backward of every row at theta.
 *   filt[n, f, i]  = a_f(i),  a_0 ~ rho o l_0,  a_f ~ (a_{f-1} A) o l_f  with normalisers c_f
 *   gamma[n, f, i] = p(state_f = i | all frames)
 *   rows[n]        = E n_ij of the M * M ordered pairs, summed over f < F - 1, row-major (F = 1: zeros); gamma_0(i) of the
 *                    M states; loglik = sum_f log c_f
 * ------------------------------------------------------------------------------------- */
#define TQ_HMM_MAX_STATES 4
#define TQ_HMM_COLS(M) ((M) * (M) + (M) + 1)
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of the fit */
  const double* theta;         /* (M * M + M) A, rho; device memory */
  double* filt;                /* (N, F, M) out */
  double* gamma;               /* (N, F, M) out */
  double* rows;                /* (N, TQ_HMM_COLS(M)) out */
  int32_t N, F;
  int32_t U, B;                /* unbound and bound states, M = U + B */
  double prior;
} tq_hmm_estep_args;

int tq_hmm_estep(const tq_hmm_estep_args* a, void* stream);

/* tq_hmm_mstep: sums the N rows of an E-step in a fixed order (bit-reproducible), stores the total loglik into trace[it]
 * and overwrites theta:  A_ij = sum E n_ij / sum_j sum E n_ij (a state without expected occupancy keeps its row),
 * rho_i = mean gamma_0(i); both floored and renormalised as above.  One workgroup. */
typedef struct {
  const double* rows;          /* (N, TQ_HMM_COLS(M)) of tq_hmm_estep */
  double* theta;               /* (M * M + M) in / out; device memory */
  double* trace;               /* trace[it] out: the total loglik at the theta the rows were computed with */
  int32_t N, it;
  int32_t U, B;
} tq_hmm_mstep_args;

int tq_hmm_mstep(const tq_hmm_mstep_args* a, void* stream);

/* tq_hmm_viterbi: the MAP path in hidden states, in the log domain, scores relative to state 0's; a tie takes the
 * lowest state.  back: scratch of 2 bits per state and frame, four frames to a word, ((F + 3) / 4) * N 32-bit words. */
typedef struct {
  const float* p;              /* (N, F) */
  const double* theta;         /* (M * M + M); device memory */
  uint32_t* back;              /* scratch, ((F + 3) / 4) * N words */
  uint8_t* path;               /* (N, F) out: hidden states 0 .. M - 1 */
  int32_t N, F;
  int32_t U, B;
  double prior;
} tq_hmm_viterbi_args;

int tq_hmm_viterbi(const tq_hmm_viterbi_args* a, void* stream);

/* tq_hmm_count: S posterior rasters of every row by forward filtering, backward sampling, with their counts.
 * u_k is the k-th uniform of Philox stream (seed, step = s, site 0xA04, elem = n), compared as a double; u_0 is for
 * frame F - 1, then downwards.  The draw is the largest i with u < t(i) (state 0 if there is none), t(i) the mass of the
 * states >= i under filt[F - 1] for the last frame and under P(state_f = . | state_{f+1} = j) ~ a_f(.) A[.][j] otherwise.
 *   counts[s, n]: the class-level counts of the row in the layout of tq_rates_count (tq_rates_estimate takes them)
 *   trans[s, n, i * M + j]: the number of frame pairs (f, f + 1) with states (i, j)
 *   raster[s, n, f]: the hidden state */
typedef struct {
  const double* filt;          /* (N, F, M) of tq_hmm_estep */
  const double* theta;         /* (M * M + M); device memory */
  int32_t* counts;             /* (S, N, TQ_RATES_COLS) out; 16-byte aligned */
  int32_t* trans;              /* (S, N, M * M) out; or NULL */
  uint8_t* raster;             /* (S, N, F) out; or NULL */
  int32_t N, F, S;
  int32_t U, B;
  uint64_t seed;
} tq_hmm_count_args;

int tq_hmm_count(const tq_hmm_count_args* a, void* stream);

/* tq_hmm_estimate: totals[s, i, j] = sum_{k < N} trans[s, a(s, k), i, j] (int64) and
 * estimand[s, i, j] = totals[s, i, j] / sum_j totals[s, i, j] as IEEE double division (a zero denominator gives NaN).
 * a(s, k) is that of tq_rates_estimate for the same `resample` and `seed` -- the same Philox site 0xA02 and formula -- so
 * one seed resamples the same AOIs for the class-level rates and for A.  One wave per sample. */
typedef struct {
  const int32_t* trans;        /* (S, N, M * M) of tq_hmm_count */
  int64_t* totals;             /* (S, M * M) out */
  double* estimand;            /* (S, M * M) out */
  int32_t N, S;
  int32_t U, B;
  int32_t resample;            /* 0: pooled; 1: bootstrap over AOIs */
  uint64_t seed;               /* resample = 1 only */
} tq_hmm_estimate_args;

int tq_hmm_estimate(const tq_hmm_estimate_args* a, void* stream);

/* tq_chain_dwell: the rasters of tq_hmm_count walked into dwell-time intervals and first-binding frames as they are drawn
 * (`dwelltime --smooth` / `ttfb --smooth` with `--unbound-states U --bound-states B`); neither a
 * raster nor the state pairs are stored.
 * Row (s, n) is, state for state, the row tq_hmm_count draws for the same filt, theta, U, B and seed: the same Philox
 * stream (seed, step = s, site 0xA04, elem = n), the same order of draws (u_0 for frame F - 1, then downwards, four
 * uniforms to a Philox block), the same floor of theta, thresholds t(i) and double compare -- so one seed gives
 * `smooth --bound-states B` and the two kinetics commands rasters of the same chain.  The class z = (state >= U) of every
 * frame goes through the walker of tq_smooth_dwell, and the outputs are tq_smooth_dwell's for that class raster:
 *   mode TQ_DWELL_COUNT: counts[s, n] = number of intervals of the row; every interior interval (low_or_high 0 / 1) of
 *     dwell time d adds 1 to hist_unbound[s, d] / hist_bound[s, d] (the caller zeroes both histograms); and, when tau is
 *     not NULL, tau[s, n] = the smallest f with a bound state, or F if there is none.
 *   mode TQ_DWELL_EMIT: the same draws again; the table `intervals` of tq_dwell_sample's EMIT, (sample, AOI) row-major and
 *     ascending in start_frame within a row.  The k-th run a row closes is written at offsets[s, n] + counts[s, n] - 1 - k; a
 *     position outside [offsets[s, n], min(offsets[s, n] + counts[s, n], total)) is dropped, never written.  total = 0
 *     launches nothing.
 * TQ_ERR_ARG, before anything touches the device, for a NULL required pointer of the mode, N, F or S < 1,
 * F > TQ_SMOOTH_MAX_F, S > 65535 * 64, total < 0, an unknown mode, U or B < 1 or U + B > TQ_HMM_MAX_STATES. */
typedef struct {
  const double* filt;          /* (N, F, M) of tq_hmm_estep */
  const double* theta;         /* (M * M + M); device memory */
  int32_t* counts;             /* (S, N) out (COUNT), in (EMIT) */
  int32_t* hist_bound;         /* (S, F) in/out (COUNT): interior bound runs by dwell time */
  int32_t* hist_unbound;       /* (S, F) in/out (COUNT): interior unbound runs by dwell time */
  float* tau;                  /* (S, N) out (COUNT): integer-valued first-binding frames in [0, F]; or NULL */
  const int64_t* offsets;      /* (S, N) in (EMIT): exclusive scan of counts */
  int32_t* intervals;          /* (TQ_DWELL_COLS, total) out (EMIT) */
  int64_t total;               /* EMIT: number of intervals (the column stride) */
  int32_t N, F, S;
  int32_t U, B;                /* unbound and bound states, M = U + B */
  int32_t mode;                /* TQ_DWELL_COUNT or TQ_DWELL_EMIT */
  uint64_t seed;
} tq_chain_dwell_args;

int tq_chain_dwell(const tq_chain_dwell_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * R EM fits of the chain above side by side (`tapqir_amd smooth --restarts R`, `--forbid i-j`).
 * Replica r has its own theta[r] (M * M + M doubles), its own rows[r] and its own slice of the scratch; p is shared.  A
 * replica computes, from the same theta, what tq_hmm_estep and tq_hmm_mstep compute: the same lane geometry, scans, sweeps,
 * strided sums and tree.  `active` (R int32 in device memory, or NULL for all active) freezes replicas: the workgroups of
 * a replica with active[r] == 0 return at once and write nothing, so its theta, rows and trace keep their values.
 * Both entry points return TQ_ERR_ARG, before anything touches the device, for what the pair above refuses, for R < 1 or
 * R > TQ_MULTISTART_MAX, and the M-step for T <= it, for an `allow` with a bit beyond M * M or a row without a free entry.
 *
 * tq_multistart_estep: grid (N, R), one wave per (row, replica).  Writes only rows[r, n] (the columns of tq_hmm_estep);
 *   gamma is not stored, and the a_f that the backward sweep needs go to the caller's scratch `filt`.
 * ------------------------------------------------------------------------------------- */
#define TQ_MULTISTART_MAX 64
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of the fit, shared by the replicas */
  const double* theta;         /* (R, M * M + M); device memory */
  double* filt;                /* (R, N, F, M) scratch */
  double* rows;                /* (R, N, TQ_HMM_COLS(M)) out */
  const int32_t* active;       /* (R); device memory; or NULL: every replica runs */
  int32_t N, F, R;
  int32_t U, B;                /* unbound and bound states, M = U + B */
  double prior;
} tq_multistart_estep_args;

int tq_multistart_estep(const tq_multistart_estep_args* a, void* stream);

/* tq_multistart_mstep: grid R, one workgroup per replica.  Sums the N rows of replica r in the fixed order of
 * tq_hmm_mstep, stores the total loglik into trace[r * T + it] and overwrites theta[r].
 *   allow: bit i * M + j set means A_ij is free.  The summed E n_ij of a cleared bit is set to 0 before the quotient, so
 *   the entry leaves the floor at TQ_SMOOTH_RMIN over the row's sum: a forbidden transition is pinned at 1e-9 -- the value
 *   every kernel reads a zero of theta as -- not at an exact zero.  All M * M bits set is the M-step of tq_hmm_mstep.
 * An inactive replica keeps theta[r] and writes no trace entry. */
typedef struct {
  const double* rows;          /* (R, N, TQ_HMM_COLS(M)) of tq_multistart_estep */
  double* theta;               /* (R, M * M + M) in / out; device memory */
  double* trace;               /* (R, T): trace[r * T + it] out */
  const int32_t* active;       /* (R); device memory; or NULL */
  int32_t N, it;
  int32_t T, R;                /* entries of a replica's trace, T > it; replicas */
  int32_t U, B;
  uint32_t allow;              /* topology mask, M * M bits */
} tq_multistart_mstep_args;

int tq_multistart_mstep(const tq_multistart_mstep_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * A mixture of G chains over the AOIs (`tapqir_amd smooth --populations G`): AOI n belongs to
 * population g with weight phi_g, and every population is a chain theta_g of the same (U, B) and topology.  P starts are
 * fitted side by side; population g of start p is replica r = p * G + g of the section above, and the E-step is
 * tq_multistart_estep with R = P * G, unchanged (the caller expands `active` from P to P * G entries).  With
 * L_g[n] = the loglik column of rows[p, g, n] and phi read floored at TQ_SMOOTH_RMIN and renormalised:
 *   ev[n]   = log sum_g phi_g e^{L_g[n]}, as max + log sum exp(. - max) with g ascending
 *   w[g, n] = exp(log phi_g + L_g[n] - ev[n]), evaluated as the g-th term of that sum over the sum
 * Every entry point returns TQ_ERR_ARG, before anything touches the device, for what the tq_hmm_* / tq_multistart_* pair
 * of the same name refuses, for G < 1 or G > TQ_MIXTURE_MAX_POP, and the M-step for P < 1, P * G > TQ_MULTISTART_MAX or
 * T <= it.
 *
 * tq_mixture_mstep: grid P, one workgroup per start.  Writes sum_n ev[n] into trace[p * T + it], and for every population
 *   A_ij = sum_n w E n_ij / sum_j sum_n w E n_ij (a state without weighted occupancy keeps its row; `allow` as in
 *   tq_multistart_mstep), rho = sum_n w gamma_0 / sum_n w (a population whose weights sum to 0 keeps theta_g), both floored
 *   as tq_hmm_mstep floors them, and phi_g = sum_n w / N floored at TQ_SMOOTH_RMIN and renormalised.  The sums run in the
 *   fixed order of tq_hmm_mstep, one population after the other: no atomics, two runs give the same bits, and G = 1 gives
 *   the theta and the trace of tq_multistart_mstep bit for bit.  An inactive start keeps everything.
 * ------------------------------------------------------------------------------------- */
#define TQ_MIXTURE_MAX_POP 4
typedef struct {
  const double* rows;          /* (P, G, N, TQ_HMM_COLS(M)) of tq_multistart_estep with R = P * G */
  double* theta;               /* (P, G, M * M + M) in / out; device memory */
  double* phi;                 /* (P, G) in / out; device memory */
  double* trace;               /* (P, T): trace[p * T + it] out, the mixture log evidence */
  double* resp;                /* (P, G, N) out: w at the theta and phi the rows were computed with; or NULL */
  double* evidence;            /* (P, N) out: ev; or NULL */
  const int32_t* active;       /* (P); device memory; or NULL */
  int32_t N, it;
  int32_t T, P;                /* entries of a start's trace, T > it; starts */
  int32_t G;                   /* populations */
  int32_t U, B;
  uint32_t allow;              /* topology mask, M * M bits, shared by the populations */
} tq_mixture_mstep_args;

int tq_mixture_mstep(const tq_mixture_mstep_args* a, void* stream);

/* tq_mixture_count: S posterior rasters of every row, each with a population of its own.  Row (s, n) first draws
 *   g = the largest g with u < sum_{g' >= g} resp[g', n], or 0, u the first uniform of Philox stream (seed, step = s, site
 *   0xA05, elem = n); then it is the row tq_hmm_count draws from filt[g, n] under theta[g] with the same seed (site 0xA04).
 *   With G = 1 the outputs are tq_hmm_count's bit for bit.  pop[s, n] = g; the other outputs as there. */
typedef struct {
  const double* filt;          /* (G, N, F, M) of tq_hmm_estep, population by population */
  const double* theta;         /* (G, M * M + M); device memory */
  const double* resp;          /* (G, N) of tq_mixture_mstep */
  int32_t* counts;             /* (S, N, TQ_RATES_COLS) out; 16-byte aligned */
  int32_t* trans;              /* (S, N, M * M) out; or NULL */
  uint8_t* pop;                /* (S, N) out */
  uint8_t* raster;             /* (S, N, F) out; or NULL */
  int32_t N, F, S;
  int32_t G;
  int32_t U, B;
  uint64_t seed;
} tq_mixture_count_args;

int tq_mixture_count(const tq_mixture_count_args* a, void* stream);

/* tq_mixture_estimate: tq_hmm_estimate per population, with its a(s, k):
 *   totals[s, g, i, j] = sum_{k < N} trans[s, a(s, k), i, j] [pop[s, a(s, k)] = g] (int64), members[s, g] = the number of
 *   drawn AOIs in g, estimand = totals over their row sums as IEEE double division (a zero denominator gives NaN). */
typedef struct {
  const int32_t* trans;        /* (S, N, M * M) of tq_mixture_count */
  const uint8_t* pop;          /* (S, N) of tq_mixture_count */
  int64_t* totals;             /* (S, G, M * M) out */
  int64_t* members;            /* (S, G) out */
  double* estimand;            /* (S, G, M * M) out */
  int32_t N, S;
  int32_t G;
  int32_t U, B;
  int32_t resample;            /* 0: pooled; 1: bootstrap over AOIs */
  uint64_t seed;               /* resample = 1 only */
} tq_mixture_estimate_args;

int tq_mixture_estimate(const tq_mixture_estimate_args* a, void* stream);

/* tq_population_dwell: the rasters of tq_mixture_count walked into dwell-time intervals and first-binding frames as they
 * are drawn (`dwelltime --smooth --populations G` / `ttfb --smooth --populations G`); neither a raster
 * nor the state pairs are stored.
 * Row (s, n) is, population for population and state for state, the row tq_mixture_count draws for the same filt, theta,
 * resp, U, B, G and seed: the same population draw (Philox stream (seed, step = s, site 0xA05, elem = n), the tails of
 * resp[., n]), then the same stream (site 0xA04), order of draws, floor of theta_g, thresholds and double compare under
 * theta[g] and filt[g, n] -- so one seed gives `smooth --populations G` and the two kinetics commands rasters of the same
 * mixture.  The class z = (state >= U) of every frame goes through the walker of tq_chain_dwell, and the outputs are
 * tq_chain_dwell's for that class raster, with the histograms kept apart by the row's drawn population:
 *   mode TQ_DWELL_COUNT: counts[s, n] = number of intervals of the row; pop[s, n] = g; every interior interval
 *     (low_or_high 0 / 1) of dwell time d adds 1 to hist_unbound[s, g, d] / hist_bound[s, g, d] (the caller zeroes both
 *     histograms); and, when tau is not NULL, tau[s, n] = the smallest f with a bound state, or F if there is none.
 *   mode TQ_DWELL_EMIT: the same draws again into the table `intervals` of tq_chain_dwell's EMIT, under its rules: the k-th
 *     run a row closes is written at offsets[s, n] + counts[s, n] - 1 - k; a position outside
 *     [offsets[s, n], min(offsets[s, n] + counts[s, n], total)) is dropped, never written; total = 0 launches nothing.  The
 *     table keeps its TQ_DWELL_COLS columns: the population of a row is pop[s, n] of the COUNT launch.
 * With G = 1 every output is tq_chain_dwell's bit for bit.
 * TQ_ERR_ARG, before anything touches the device, for what tq_chain_dwell refuses (a NULL required pointer of the mode --
 * resp always, pop in COUNT --, N, F or S < 1, F > TQ_SMOOTH_MAX_F, S > 65535 * 64, total < 0, an unknown mode, U or B < 1 or
 * U + B > TQ_HMM_MAX_STATES), and for G < 1 or G > TQ_MIXTURE_MAX_POP. */
typedef struct {
  const double* filt;          /* (G, N, F, M) of tq_hmm_estep, population by population */
  const double* theta;         /* (G, M * M + M); device memory */
  const double* resp;          /* (G, N) of tq_mixture_mstep */
  int32_t* counts;             /* (S, N) out (COUNT), in (EMIT) */
  uint8_t* pop;                /* (S, N) out (COUNT) */
  int32_t* hist_bound;         /* (S, G, F) in/out (COUNT): interior bound runs by drawn population and dwell time */
  int32_t* hist_unbound;       /* (S, G, F) in/out (COUNT): interior unbound runs by drawn population and dwell time */
  float* tau;                  /* (S, N) out (COUNT): integer-valued first-binding frames in [0, F]; or NULL */
  const int64_t* offsets;      /* (S, N) in (EMIT): exclusive scan of counts */
  int32_t* intervals;          /* (TQ_DWELL_COLS, total) out (EMIT) */
  int64_t total;               /* EMIT: number of intervals (the column stride) */
  int32_t N, F, S;
  int32_t G;
  int32_t U, B;                /* unbound and bound states, M = U + B */
  int32_t mode;                /* TQ_DWELL_COUNT or TQ_DWELL_EMIT */
  uint64_t seed;
} tq_population_dwell_args;

int tq_population_dwell(const tq_population_dwell_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dwell times with the open last run (`tapqir_amd dwelltime --censored`).  A run of a kind (bound,
 * z = 1; unbound, z = 0) is used when it opens inside the record (start_frame > 0).  If it also closes inside it
 * (low_or_high 0 / 1, what the COUNT launches put into their histograms) it is a complete dwell of d frames with the term
 * log sum_j A_j k_j exp(-k_j d).  If it is still open at frame F - 1 (low_or_high == z + 2) it is right-censored after d
 * seen frames -- d - 1 stays and nothing else -- with the term log sum_j A_j exp(-k_j (d - 1)); d = 1 carries no
 * information.  First runs (start_frame == 0, a run that spans the record included) are used by neither.
 *
 * tq_dwell_censored_hist: the histograms of the open last runs from the interval table that any of the four EMIT launches
 * wrote.  One lane per table row; every row with low_or_high 2 / 3 and start_frame > 0 adds 1 to
 * cens_unbound[s, g, dwell_time] / cens_bound[s, g, dwell_time], g = pop[s, n] (the pop of tq_population_dwell's COUNT
 * launch) or 0 without pop.  The caller zeroes both histograms.  Integer atomics: the result is deterministic.  A row whose
 * entries are out of range adds nothing.  total == 0 is TQ_OK without a launch.  TQ_ERR_ARG, before anything touches the
 * device, for a NULL histogram (or table with total > 0), S, N or F < 1, total < 0, G outside 1 .. 4, or G > 1 without pop.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const int32_t* intervals;    /* (TQ_DWELL_COLS, total): the table of an EMIT launch, on the device */
  const uint8_t* pop;          /* (S, N) drawn population of every row, or NULL (G = 1) */
  int32_t* cens_bound;         /* (S, G, F) in/out: open last bound runs by drawn population and dwell time */
  int32_t* cens_unbound;       /* (S, G, F) in/out: open last unbound runs by drawn population and dwell time */
  int64_t total;               /* number of intervals (the column stride) */
  int32_t S, N, F;
  int32_t G;                   /* populations, 1 .. 4 */
} tq_dwell_censored_hist_args;

int tq_dwell_censored_hist(const tq_dwell_censored_hist_args* a, void* stream);

/* tq_dwell_censored_fit: tq_dwell_fit with a second CSR list per row, (cvalues[i], cweights[i]), crow_ptr[s] <= i <
 * crow_ptr[s + 1], of right-censored times t >= 0 (t = d - 1) with their multiplicities.  The loss of row s is
 *   -sum_i w_i log sum_j A_j k_j exp(-k_j t_i) - sum_i wc_i log sum_j A_j exp(-k_j tc_i),
 * and everything else -- parameters, state layout (S, 6 K), step0 / n_steps chunking (bitwise equal to one launch), the
 * loss of the last step, Adam -- is tq_dwell_fit's.  At K = 1 the maximiser is k = n / (sum w t + sum wc tc).  One wave per
 * row: a row is staged in LDS when stage_lds != 0 and its complete and censored pairs together are at most
 * TQ_DWELL_LDS_PAIRS, otherwise both lists are read from L2 every step.  With every censored row empty, state and loss
 * are tq_dwell_fit's bit for bit.  TQ_ERR_ARG for what tq_dwell_fit refuses, and for a NULL censored list (an empty one
 * still needs valid pointers). */
typedef struct {
  const float* values;         /* (nnz) dwell times > 0 of the complete runs */
  const float* weights;        /* (nnz) multiplicities */
  const int64_t* row_ptr;      /* (S + 1) */
  const float* cvalues;        /* (cnnz) censored times >= 0: seen frames - 1 */
  const float* cweights;       /* (cnnz) multiplicities */
  const int64_t* crow_ptr;     /* (S + 1) */
  float* state;                /* (S, 6 K) in/out: log k[K], a[K], exp_avg[2K], exp_avg_sq[2K] */
  float* loss;                 /* (S) out or NULL: loss at the last step of the launch, before its update */
  int32_t S, K;                /* 1 <= K <= TQ_DWELL_KMAX */
  int32_t step0;               /* Adam steps completed before this launch */
  int32_t n_steps;             /* Adam steps of this launch (>= 1) */
  int32_t stage_lds;           /* 1: stage rows in LDS when they fit; 0: always read them from L2 */
  double lr, beta1, beta2, eps;
} tq_dwell_censored_fit_args;

int tq_dwell_censored_fit(const tq_dwell_censored_fit_args* a, void* stream);

/* tq_dwell_survival: the product-limit (Kaplan-Meier) estimate of every row.  hist[r, d] complete runs and cens[r, d]
 * open last runs of d frames; surv[r, 0] = 1 and surv[r, t] = prod_{u = 1 .. t} (Y_u - h_u) / Y_u, a factor of 1 where
 * Y_u = 0, with Y_u = sum_{d >= u} h_d + sum_{d >= u + 1} c_d: an open run of d frames is at risk up to d - 1, the
 * convention of the fit.  Each factor is one float64 division of two integers, so a curve that reaches 0 (Y_u = h_u) or
 * stays at 1 does so exactly.  One wave per row.  TQ_ERR_ARG for a NULL pointer, R or F < 1 or F > TQ_SMOOTH_MAX_F. */
typedef struct {
  const int32_t* hist;         /* (R, F) complete runs by dwell time */
  const int32_t* cens;         /* (R, F) open last runs by seen frames */
  double* surv;                /* (R, F) out */
  int32_t R, F;
} tq_dwell_survival_args;

int tq_dwell_survival(const tq_dwell_survival_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Two colour channels as one chain (`tapqir_amd smooth --joint A,B`).  Channels a and b of one
 * cosmos fit, hidden state s = z_a + 2 z_b: 0 neither bound, 1 only a, 2 only b, 3 both.
 *   theta = (A row-major (4, 4), rho (4)): 20 doubles in device memory, read floored at TQ_SMOOTH_RMIN and renormalised as
 *           the chain of four states above reads its theta.
 *   l_f(s) = l^a_f(s & 1) l^b_f(s >> 1), l^c the evidence of the two-state section of channel c's p under channel c's
 *           prior, with the same clamp at TQ_SMOOTH_PMIN.
 * Replicas, `active` and the layout are those of the side-by-side section: replica r has theta[r], rows[r],
 * filt[r] and gamma[r]; p_a and p_b are shared.  The workgroups of a replica with active[r] == 0 return at once and write
 * nothing.  No atomics and a fixed order of additions: two runs give the same bits.
 * Every entry point returns TQ_ERR_ARG, before anything touches the device, for a NULL required pointer, N, F or R < 1,
 * F > TQ_SMOOTH_MAX_F, R > TQ_MULTISTART_MAX, a prior outside (0, 1), it < 0, T <= it, or a structure outside 0 .. 4 among
 * the first R entries.
 *
 * tq_joint_estep: grid (N, R), one wave per (row, replica), the lane ranges, scans, sweeps and lane sums of tq_hmm_estep.
 *   filt[r, n, f, s] = a_f(s), gamma[r, n, f, s] = p(state_f = s | all frames), rows[r, n] in the column order of
 *   tq_hmm_estep: E n_ss' of the 16 ordered pairs, gamma_0 of the 4 states, loglik.  gamma == NULL stores no gamma; rows
 *   have the same bits either way.
 * ------------------------------------------------------------------------------------- */
#define TQ_JOINT_INDEPENDENT 0 /* A = P_a(z_a' | z_a) P_b(z_b' | z_b): 4 free parameters of A */
#define TQ_JOINT_A_DRIVES_B 1  /* A = P_a(z_a' | z_a) P_b(z_b' | z_a, z_b): 6 */
#define TQ_JOINT_B_DRIVES_A 2  /* A = P_a(z_a' | z_a, z_b) P_b(z_b' | z_b): 6 */
#define TQ_JOINT_COUPLED 3     /* A = P_a(z_a' | s) P_b(z_b' | s), no concerted events beyond chance: 8 */
#define TQ_JOINT_FULL 4        /* A[s][s'] = n[s -> s'] / n[s -> .]: 12 */
typedef struct {
  const float* p_a;            /* (N, F) p(z = 1) of channel a, shared by the replicas */
  const float* p_b;            /* (N, F) of channel b */
  const double* theta;         /* (R, 20); device memory */
  double* filt;                /* (R, N, F, 4) out */
  double* gamma;               /* (R, N, F, 4) out; or NULL */
  double* rows;                /* (R, N, TQ_HMM_COLS(4)) out */
  const int32_t* active;       /* (R); device memory; or NULL: every replica runs */
  int32_t N, F, R;
  double prior_a, prior_b;     /* pi of each channel */
} tq_joint_estep_args;

int tq_joint_estep(const tq_joint_estep_args* a, void* stream);

/* tq_joint_mstep: grid R, one workgroup per replica.  Sums the N rows of replica r in the fixed order of tq_hmm_mstep (the
 * same bits for the same rows), stores the total loglik into trace[r * T + it] and overwrites theta[r] under structure[r].
 * With n the summed E n_ss' and s = (z_a, z_b):
 *   P_a(z_a' | s) = sum_{z_b'} n[s -> (z_a', z_b')] / n[s -> .]; where channel a does not see z_b (independent,
 *   a-drives-b), numerator and denominator are both summed over z_b first.  P_b is the mirror image.
 *   A[s][s'] = P_a P_b, then the floor of theta; TQ_JOINT_FULL is the M-step of tq_hmm_mstep.  A row whose denominator --
 *   for a pooled factor, the pooled denominator -- is zero keeps its old values.  rho = mean gamma_0, floored.
 * An inactive replica keeps theta[r] and writes no trace entry. */
typedef struct {
  const double* rows;          /* (R, N, TQ_HMM_COLS(4)) of tq_joint_estep */
  double* theta;               /* (R, 20) in / out; device memory */
  double* trace;               /* (R, T): trace[r * T + it] out */
  const int32_t* active;       /* (R); device memory; or NULL */
  int32_t N, it;
  int32_t T, R;                /* entries of a replica's trace, T > it; replicas */
  int32_t structure[TQ_MULTISTART_MAX]; /* TQ_JOINT_* of replica r; host memory, part of this struct */
} tq_joint_mstep_args;

int tq_joint_mstep(const tq_joint_mstep_args* a, void* stream);

/* tq_joint_viterbi: the MAP path in joint states at one theta: tq_hmm_viterbi of four states with the emission logarithm
 * of state s formed as log l^a(s & 1) + log l^b(s >> 1); the same back-pointer words and tie rule (lowest state).  One
 * lane per row. */
typedef struct {
  const float* p_a;            /* (N, F) */
  const float* p_b;            /* (N, F) */
  const double* theta;         /* (20); device memory */
  uint32_t* back;              /* scratch, ((F + 3) / 4) * N words */
  uint8_t* path;               /* (N, F) out: joint states 0 .. 3 */
  int32_t N, F;
  double prior_a, prior_b;
} tq_joint_viterbi_args;

int tq_joint_viterbi(const tq_joint_viterbi_args* a, void* stream);

/* tq_pair_dwell: the rasters of tq_hmm_count at (U, B) = (2, 2) on the joint filt, walked into the dwell-time intervals and
 * first-binding frames of one channel as they are drawn, every run with the other channel's state at its two ends
 * (`dwelltime --smooth --joint A,B` / `ttfb --smooth --joint A,B`); neither a raster nor the state
 * pairs are stored.
 * Row (s, n) is, state for state, the row tq_hmm_count draws at (U, B) = (2, 2) for the same filt, theta and seed: the same
 * Philox stream (seed, step = s, site 0xA04, elem = n), the same order of draws (u_0 for frame F - 1, then downwards, four
 * uniforms to a Philox block), the same floor of theta, thresholds t(i) and double compare -- so one seed gives
 * `smooth --joint A,B` and the two kinetics commands rasters of the same chain, and both values of `which` at one seed
 * describe the same rasters.  `which` chooses the channel whose runs are walked: 0 is channel a (bit 0 of the state
 * s = z_a + 2 z_b), 1 is channel b (bit 1); the other channel is the partner.  The class z = (state >> which) & 1 goes
 * through the walker of tq_chain_dwell; with q(f) the partner's class at frame f, a run over [start, stop] has the partner
 * code  bit 0 = q(start), bit 1 = q(start - 1) (0 when start = 0), bit 2 = q(stop), bit 3 = q(stop + 1) (0 when
 * stop = F - 1).
 *   mode TQ_DWELL_COUNT: counts[s, n] = number of intervals of the row; every interior interval (low_or_high 0 / 1) of
 *     dwell time d adds 1 to hist_unbound[s, q(start), d] / hist_bound[s, q(start), d] (the caller zeroes both histograms);
 *     when tau is not NULL, tau[s, n] = the smallest f with z = 1, or F if there is none; when tau_after is not NULL,
 *     tau_after[s, n] = the smallest f >= tau[s, n] with q(f) = 1, or F if there is none or tau[s, n] = F.
 *   mode TQ_DWELL_EMIT: the same draws again into the table `intervals` of tq_chain_dwell's EMIT, under its rules: ascending
 *     in start_frame within a row, the k-th run a row closes is written at offsets[s, n] + counts[s, n] - 1 - k; a position
 *     outside [offsets[s, n], min(offsets[s, n] + counts[s, n], total)) is dropped, never written; total = 0 launches
 *     nothing.  The table keeps its TQ_DWELL_COLS columns; partner[pos] receives the partner code of the run at pos.
 * With which = 1, counts, tau, the table and the histograms summed over q are tq_chain_dwell's at (2, 2) bit for bit.
 * TQ_ERR_ARG, before anything touches the device, for what tq_chain_dwell refuses (a NULL required pointer of the mode --
 * partner in EMIT with total > 0 among them --, N, F or S < 1, F > TQ_SMOOTH_MAX_F, S > 65535 * 64, total < 0, an unknown
 * mode), and for `which` outside {0, 1}. */
typedef struct {
  const double* filt;          /* (N, F, 4) of tq_joint_estep at R = 1 */
  const double* theta;         /* (20); device memory */
  int32_t* counts;             /* (S, N) out (COUNT), in (EMIT) */
  int32_t* hist_bound;         /* (S, 2, F) in/out (COUNT): interior bound runs by q(start) and dwell time */
  int32_t* hist_unbound;       /* (S, 2, F) in/out (COUNT): interior unbound runs by q(start) and dwell time */
  float* tau;                  /* (S, N) out (COUNT): integer-valued first-binding frames in [0, F]; or NULL */
  float* tau_after;            /* (S, N) out (COUNT): the partner's first bound frame from tau on, in [0, F]; or NULL */
  const int64_t* offsets;      /* (S, N) in (EMIT): exclusive scan of counts */
  int32_t* intervals;          /* (TQ_DWELL_COLS, total) out (EMIT) */
  uint8_t* partner;            /* (total) out (EMIT): partner code of every interval */
  int64_t total;               /* EMIT: number of intervals (the column stride) */
  int32_t N, F, S;
  int32_t which;               /* 0: the runs of channel a; 1: those of channel b */
  int32_t mode;                /* TQ_DWELL_COUNT or TQ_DWELL_EMIT */
  uint64_t seed;
} tq_pair_dwell_args;

int tq_pair_dwell(const tq_pair_dwell_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Bootstrap refits of the chain over AOIs (`tapqir_amd smooth --refit R`): R replicas of the EM of
 * tq_multistart_estep / tq_multistart_mstep, each on a resample of the N AOIs with replacement.  A resample is a weight
 * per AOI -- how often it was drawn -- so p stays shared and no row is gathered: the E-step leaves out the (replica, AOI)
 * pairs of weight 0, and the M-step multiplies every row by its weight.  theta, rows, the scratch, `active`, `allow` and
 * the trace have the layouts of the tq_multistart_* section; weights is (R, N) int32 in device memory, non-negative, every
 * row's sum below 2^31.
 * Every entry point returns TQ_ERR_ARG, before anything touches the device, for what the tq_multistart_* entry point of the
 * same role refuses and for a NULL `weights`; tq_refit_weights for N < 1, R < 1 or R > TQ_MULTISTART_MAX, first < 0 or
 * first + R > 2^31 - 1.
 *
 * tq_refit_weights: weights[r, n] = #{ i < N : a(first + r, i) = n }, a(s, i) the resample of tq_rates_estimate and
 *   tq_hmm_estimate for sample s at the same seed (Philox site 0xA02, the same formula), so one seed resamples the same
 *   AOIs everywhere; `first` lets the host work in batches without changing any replica's draw.  Grid R, one workgroup
 *   per replica: it zeroes its row itself -- the caller need not -- and counts with integer atomics, whose result does
 *   not depend on their order.  Every row sums to N.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  int32_t* weights;            /* (R, N) out */
  int32_t N, R;
  int32_t first;               /* replica r is sample first + r of the stream */
  uint64_t seed;
} tq_refit_weights_args;

int tq_refit_weights(const tq_refit_weights_args* a, void* stream);

/* tq_refit_estep: tq_multistart_estep on the grid (N, R) with the weights.  The workgroup of a pair with
 * weights[r, n] == 0, like that of a replica with active[r] == 0, returns before its first shuffle and writes nothing:
 * rows[r, n] and filt[r, n] keep what they held.  Where the weight is positive it writes the bits of tq_multistart_estep. */
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of the fit, shared by the replicas */
  const double* theta;         /* (R, M * M + M); device memory */
  double* filt;                /* (R, N, F, M) scratch */
  double* rows;                /* (R, N, TQ_HMM_COLS(M)) out, where weights[r, n] > 0 */
  const int32_t* active;       /* (R); device memory; or NULL: every replica runs */
  const int32_t* weights;      /* (R, N); device memory */
  int32_t N, F, R;
  int32_t U, B;                /* unbound and bound states, M = U + B */
  double prior;
} tq_refit_estep_args;

int tq_refit_estep(const tq_refit_estep_args* a, void* stream);

/* tq_refit_mstep: grid R, one workgroup per replica.  sums_j = sum_n weights[r, n] rows[r, n, j] and
 * W = sum_n weights[r, n], thread t taking rows t, t + 256, ... and a fixed tree after it -- the order of additions of
 * tq_multistart_mstep; a row of weight 0 is skipped and never read, so it may hold anything, NaN included.  Then the
 * M-step of tq_multistart_mstep under `allow` with W in the place of N, into theta[r], and the weighted log evidence
 * sum_n weights[r, n] loglik_n into trace[r * T + it].  With every weight 1 theta and the trace are those of
 * tq_multistart_mstep bit for bit.  W = 0 leaves A[r] as it is and sets rho[r] uniform.  An inactive replica keeps
 * theta[r] and writes no trace entry. */
typedef struct {
  const double* rows;          /* (R, N, TQ_HMM_COLS(M)) of tq_refit_estep */
  double* theta;               /* (R, M * M + M) in / out; device memory */
  double* trace;               /* (R, T): trace[r * T + it] out */
  const int32_t* active;       /* (R); device memory; or NULL */
  const int32_t* weights;      /* (R, N); device memory */
  int32_t N, it;
  int32_t T, R;                /* entries of a replica's trace, T > it; replicas */
  int32_t U, B;
  uint32_t allow;              /* topology mask, M * M bits */
} tq_refit_mstep_args;

int tq_refit_mstep(const tq_refit_mstep_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * The continuous-time hidden Markov chain on the frame timestamps (`tapqir_amd smooth --timed`): the
 * chain of the tq_hmm_* section with a generator Q in the place of the per-frame matrix A.  The transition from frame f to
 * f + 1 is exp(Q d_f), d_f the gap between their stamps, so the record need not be equally spaced.
 *   theta = (Q row-major (M, M), rho (M)): M * M + M doubles in device memory, Q per unit of the gaps.  Every reader
 *           ignores the stored diagonal, takes a free off-diagonal as max(q_ij, TQ_SMOOTH_RMIN), a forbidden one (cleared
 *           bit of `allow`, the mask of tq_multistart_mstep; its diagonal bits are not read) as exactly 0, sets
 *           q_ii = -sum_j q_ij, and floors and renormalises rho as tq_hmm_estep does.
 *   d     = the D distinct gaps, positive and finite, and cls (F - 1) int32 the class of every gap: the gap between frames
 *           f and f + 1 is d[cls[f]].  The host scales the gaps so that their median is 1; the floor of a rate then means
 *           what the floor of a transition probability means per frame.
 *   P (D, M, M) and K (D, M, M, M, M): P[k] = exp(Q d[k]) and K[k][a][b][i][j] = int_0^d[k] P_ai(s) P_jb(d[k] - s) ds, so
 *           that sum_b P[k][a][b] = 1 and sum_i K[k][a][b][i][i] = d[k] P[k][a][b].
 * Every entry point returns TQ_ERR_ARG, before anything touches the device, for a NULL required pointer, U or B < 1,
 * U + B > TQ_HMM_MAX_STATES, D < 1 (tables, E-step), an `allow` with a bit beyond M * M or a row without a set bit;
 * tq_timed_table for a gap of d_host that is not finite and positive; tq_timed_estep for N or F < 1, F > TQ_SMOOTH_MAX_F, a
 * prior outside (0, 1), a NULL cls or cls_host where F > 1, or an entry of cls_host outside [0, D); tq_timed_mstep for
 * N < 1, it < 0 or T <= it.  d_host and cls_host are the host's copies of d and cls: the checks read them, the kernels the
 * device's.
 *
 * tq_timed_table: one thread per (class, i, j), which carries P and the M x M matrix K[k][.][.][i][j] through a Taylor
 *   series of the uniformised chain at d / 2^s and s squarings of the pair (P, K); no thread waits on another and there
 *   are no atomics, so two runs give the same bits.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const double* theta;         /* M * M + M; device memory */
  const double* d;             /* (D) gaps; device memory */
  const double* d_host;        /* (D) the same gaps; host memory */
  double* P;                   /* (D, M, M) out */
  double* K;                   /* (D, M, M, M, M) out */
  int32_t D;
  int32_t U, B;                /* unbound and bound states, M = U + B */
  uint32_t allow;              /* topology mask, M * M bits */
} tq_timed_table_args;

int tq_timed_table(const tq_timed_table_args* a, void* stream);

/* tq_timed_estep: tq_hmm_estep -- grid N, one wave per row, its lane ranges, scans, sweeps and lane sums -- with the
 * transition into frame f read from P[cls[f - 1]].  filt and gamma are those of tq_hmm_estep; gamma may be NULL, and the
 * rows are then the same bits.  rows[n] keeps TQ_HMM_COLS(M) columns: slot i * M + j, i != j, holds E N_ij, the expected
 * number of jumps from i to j (0 for a forbidden pair, whatever K holds there); slot i * M + i holds E T_i, the expected
 * time in state i, in the unit of d; then gamma_0 (M) and the row's log evidence.  With a = a_f, w = l_{f+1} o beta_{f+1}
 * and c_ab = a_a w_b / sum_ab a_a P_ab w_b, gap f adds sum_ab c_ab K[a][b][i][i] to E T_i and q_ij sum_ab c_ab K[a][b][i][j]
 * to E N_ij: nothing is divided by P_ab.  F = 1 has no gap and writes gamma_0 and the log evidence only. */
typedef struct {
  const float* p;              /* (N, F) p(z = 1) of the fit */
  const double* theta;         /* M * M + M; device memory */
  const double* P;             /* (D, M, M) of tq_timed_table at the same theta */
  const double* K;             /* (D, M, M, M, M) of tq_timed_table */
  const int32_t* cls;          /* (F - 1); device memory */
  const int32_t* cls_host;     /* (F - 1) the same indices; host memory */
  double* filt;                /* (N, F, M) out */
  double* gamma;               /* (N, F, M) out, or NULL */
  double* rows;                /* (N, TQ_HMM_COLS(M)) out */
  int32_t N, F, D;
  int32_t U, B;
  uint32_t allow;              /* topology mask, M * M bits */
  double prior;
} tq_timed_estep_args;

int tq_timed_estep(const tq_timed_estep_args* a, void* stream);

/* tq_timed_mstep: one workgroup, the order of additions of tq_hmm_mstep.  q_ij = sum_n E N_ij / sum_n E T_i floored at
 * TQ_SMOOTH_RMIN for a free pair, exactly 0 for a forbidden one, and the stored diagonal minus the row's sum; a state with
 * sum_n E T_i = 0 keeps its free rates.  rho = the mean gamma_0, floored and renormalised; the summed log evidence goes to
 * trace[it]. */
typedef struct {
  const double* rows;          /* (N, TQ_HMM_COLS(M)) of tq_timed_estep */
  double* theta;               /* M * M + M in / out; device memory */
  double* trace;               /* (T): trace[it] out */
  int32_t N, it;
  int32_t T;                   /* entries of the trace, T > it */
  int32_t U, B;
  uint32_t allow;              /* topology mask, M * M bits */
} tq_timed_mstep_args;

int tq_timed_mstep(const tq_timed_mstep_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Input side: AOI extraction from raw Glimpse frames.
 * Replaces the per-frame / per-AOI loop of read_glimpse (tapqir/imscroll/glimpse_reader.py:358-392), the frame
 * decode of GlimpseDataset.__getitem__ (168-186: big-endian int16 + 2^15) and the offset-region value counts
 * (362-369), for one chunk of `nf` consecutive frames of one colour channel:
 *
 *   shiftx = rint(x - 0.5 (P - 1)),  shifty = rint(y - 0.5 (P - 1))       (Python round(): half to even, 374-375)
 *   images[n, f0 + f, c, i, j]   = frame_f[shifty + i, shiftx + j] + 32768  (376-378)
 *   target_xy[n, f0 + f, c, :]   = (x - shiftx, y - shifty)                 (379-384)
 *   offset_hist[v]              += #{pixels == v in frame_f[offset_y : +offset_P, offset_x : +offset_P]}  (362-369)
 *
 * Integer work, bit-exact.  A crop that leaves the frame (the reference fails there with a numpy broadcasting
 * ValueError) is skipped and counted in status[0]; the caller raises.  status[1] receives the smallest extracted
 * pixel value (atomic min: initialise to INT32_MAX), which the offset post-processing needs (419-421).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const uint8_t* frames;   /* nf frames of H*W big-endian int16: the bytes of the .glimpse file, unmodified */
  const double* raw_xy;    /* (N, nf, 2) drift-corrected target positions (x, y) in frame pixels, float64 (347-350);
                              16-byte aligned */
  int32_t* images;         /* (N, F, C, P, P) out; only channel c of frames [f0, f0 + nf) is written */
  double* target_xy;       /* (N, F, C, 2) out */
  int64_t* offset_hist;    /* [65536] accumulated; NULL = no offset region in this call */
  int32_t* status;         /* [2]: {crops outside the frame (accumulated), min pixel (atomic min)} */
  int32_t H, W;            /* frame height, width (header.mat) */
  int32_t N, F, C, P;
  int32_t c, f0, nf;
  int32_t offset_x, offset_y, offset_P;
} tq_glimpse_args;

int tq_glimpse_extract(const tq_glimpse_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
