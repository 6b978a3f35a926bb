// tq_step_staged.h -- part of the translation unit tq_cosmos.hip, included from there only (it defines __global__
// kernels): the one-kernel-per-stage launches of a step -- guide sampling, per-unit terms, per-AOI terms, cross-unit sums,
// global sites, dense and lazy Adam -- which tq_cosmos_step and the AOI-sharded and streamed routes issue one after the
// other; and the wave sums and single-workgroup bodies (sums, global sites) that the tails carried by another launch
// (tq_step_rows.h, tq_step_minibatch.h) share with them.
//
// Launch shapes: everything except the pixel kernel is one lane per work item, SoA so that
// consecutive lanes touch consecutive addresses (the flat parameter buffer is [row][unit]).
// Cross-unit sums are deterministic: wave64 __shfl_down -> LDS -> one row per workgroup ->
// a single-workgroup fp64 finish; no float atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "tq_beta_compact.h"
#include "tq_bodies.h"
#include "tq_dpp.h"
#include "tq_stamps.h"

#define TQ_UNIT_BLOCK 256
#define TQ_MAX_NGSUM (3 + 3 * TQ_MAXQ)  // >= 3 + 3*2 + 2*2 of the crosstalk model

// sum over the wave (every lane active), in every lane: DPP adds inside the four rows of 16 lanes, then the four row sums
// read as scalars -- no LDS crossbar (six ds_bpermute per sum in the shuffle form; the fused pixel + per-unit kernel ends
// every wave with 22 such sums)
// Deliberately not tq_fit_wave_sum (tq_fit.h): that one crosses the rows with two __shfl_xor through the LDS crossbar, this
// one adds the four row sums read as scalars, (r0 + r16) + (r32 + r48); the step kernels' code is tuned around this form.
__device__ __forceinline__ float tq_wave_sum_rows4(float v) {
  v = tq_group_sum16(v);
  const int b = __builtin_bit_cast(int, v);
  return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))) +
         (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48)));
}

// ---- sampling ------------------------------------------------------------------------------------------
// one wave per global site (4 independent instruction streams instead of one serial lane)
__global__ __launch_bounds__(64) void tq_sample_globals_kernel(const tq_cosmos_args a) {
  if (threadIdx.x == 0) tq_body_sample_globals(a, blockIdx.x);
}

// grid.y = site: the site kind (Gamma / AffineBeta, which parameter rows) is uniform per workgroup
__global__ __launch_bounds__(256) void tq_sample_locals_kernel(const tq_cosmos_args a, const int64_t B, const int site_begin) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  tq_sample_site_wg(a, site_begin + (int)blockIdx.y, i, B);
}

// ---- per-unit terms ------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(TQ_UNIT_BLOCK) void tq_unit_kernel(const tq_cosmos_args a, const int64_t B) {
  __shared__ float s_part[TQ_UNIT_BLOCK / 64][TQ_MAX_NGSUM];
  const int64_t i = (int64_t)blockIdx.x * TQ_UNIT_BLOCK + threadIdx.x;
  const int nq = tq_num_gsum(a);
  float part[TQ_MAX_NGSUM];
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) part[j] = 0.0f;
  if (i < B) tq_body_unit<K>(a, i, part);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) {
    if (j < nq) {
      const float s = tq_wave_sum_rows4(part[j]);
      if (lane == 0) s_part[wave][j] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < nq) {
    float s = 0.0f;
#pragma unroll
    for (int w = 0; w < TQ_UNIT_BLOCK / 64; ++w) s += s_part[w][threadIdx.x];
    a.blk_part[(int64_t)blockIdx.x * nq + threadIdx.x] = s;
  }
}

// ---- per-AOI terms: one workgroup per (a, c), threads stride the frames ------------------------------------
__global__ __launch_bounds__(256) void tq_aoi_kernel(const tq_cosmos_args a, const int64_t B) {
  __shared__ float s_sum[4][2];
  const int ac = blockIdx.x;  // < nb * C
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = ac / a.C, c = ac % a.C;
  float s1 = 0.0f, s2 = 0.0f;
  for (int b = threadIdx.x; b < a.fb; b += 256) {
    const int64_t i = ((int64_t)ai * a.fb + b) * a.C + c;
    s1 += a.aoi_part[i];
    s2 += a.aoi_part[B + i];
  }
  s1 = tq_wave_sum_rows4(s1);
  s2 = tq_wave_sum_rows4(s2);
  if (lane == 0) {
    s_sum[wave][0] = s1;
    s_sum[wave][1] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float e;
    tq_body_aoi_finish(a, ai, c, (s_sum[0][0] + s_sum[1][0]) + (s_sum[2][0] + s_sum[3][0]),
                       (s_sum[0][1] + s_sum[1][1]) + (s_sum[2][1] + s_sum[3][1]), &e);
    a.aoi_part[2 * B + ac] = e;  // per-AOI prior part of the ELBO (row 2 is scratch, nb*C <= B)
  }
}

// one single-wave workgroup per global site: the fp64 special functions get the full register file
// (no spills, hence no scratch memory: a per-lane scratch request is sized by the runtime for the
// whole device and can push a dispatch onto the slow allocate-per-dispatch path)
__global__ __launch_bounds__(64) void tq_globals_grad_kernel(const tq_cosmos_args a, double* site_elbo) {
  const int s = blockIdx.x;
  if (threadIdx.x == 0) site_elbo[s] = tq_body_globals_grad(a, s);
}

__global__ __launch_bounds__(64) void tq_elbo_finish_kernel(const tq_cosmos_args a, const double* site_elbo) {
  if (threadIdx.x == 0) {
    double eg = 0.0;
    const int ns = tq_num_gsites(a);
    for (int j = 0; j < ns; ++j) eg += site_elbo[j];
    a.elbo_out[0] = a.gsum[TQ_GS_ELBO] + (double)a.global_weight * eg;
  }
}

__global__ __launch_bounds__(256) void tq_adam_kernel(const tq_cosmos_args a, const int64_t first, const int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) tq_body_adam(a, j);
}

// lazy Adam: grid.x over the units of the batch (or of the dataset), grid.y = local parameter row
__global__ __launch_bounds__(256) void tq_adam_catchup_kernel(const tq_cosmos_args a, const int64_t n, const int all_units) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t u = all_units ? i : tq_decode_unit(a, i).u;
  tq_adam_replay(a, (int64_t)blockIdx.y * tq_num_units(a) + u, a.last_step[u] + 1, (int)a.step);
}

// single-GPU step: finish of the cross-unit sums + all global sites + total ELBO in ONE workgroup of 4 waves
// (one wave per SIMD, so the fp64 site code keeps the full register file); sites are taken round-robin
// Deliberately not an xor butterfly like the sums of the fit kernels: a __shfl_down reduction, complete in lane 0 only.
__device__ __forceinline__ double tq_wave_sum_d_lane0(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// global sites (one lane of a wave per site, round-robin over the 4 waves) and the total ELBO from the finished sums
__device__ __forceinline__ void tq_globals_from_gsum_body(const tq_cosmos_args& a, double* s_e) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ns = tq_num_gsites(a);
  if (lane == 0)
    for (int s = wave; s < ns; s += 4) {
      s_e[s] = tq_body_globals_grad(a, s);
      TQ_STAMP_SITE(a, s);
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    double eg = 0.0;
    for (int j = 0; j < ns; ++j) eg += s_e[j];
    a.elbo_out[0] = a.gsum[TQ_GS_ELBO] + (double)a.global_weight * eg;
  }
}

// the finish of every tail's sums: the per-thread fp64 partial sums `acc` of ONE workgroup of 256 threads (s_w: its shared
// scratch) -> gsum.  Wave sums, then the four waves' in the order ((w0 + w1) + w2) + w3.
__device__ __forceinline__ void tq_sums_finish(const tq_cosmos_args& a, const double* acc, double (*s_w)[TQ_MAX_NGSUM]) {
  const int nq = tq_num_gsum(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) {
    if (j < nq) {
      const double s = tq_wave_sum_d_lane0(acc[j]);
      if (lane == 0) s_w[wave][j] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < nq) a.gsum[threadIdx.x] = s_w[0][threadIdx.x] + s_w[1][threadIdx.x] + s_w[2][threadIdx.x] + s_w[3][threadIdx.x];
}

// cross-unit sums in fp64 by ONE workgroup of 256 threads (s_w: its shared scratch): per-workgroup rows of the unit
// kernel + per-AOI ELBO parts -> gsum
__device__ __forceinline__ void tq_reduce_sums_body(const tq_cosmos_args& a, const int64_t nblk, const int64_t B,
                                                    double (*s_w)[TQ_MAX_NGSUM]) {
  const int nq = tq_num_gsum(a);
  // every thread walks the rows once, carrying all columns (nq <= 15); then shuffle + 4-way LDS sum
  double acc[TQ_MAX_NGSUM];
#pragma unroll
  for (int j = 0; j < TQ_MAX_NGSUM; ++j) acc[j] = 0.0;
  for (int64_t r = threadIdx.x; r < nblk; r += 256) {
#pragma unroll
    for (int j = 0; j < TQ_MAX_NGSUM; ++j)
      if (j < nq) acc[j] += (double)a.blk_part[r * nq + j];
  }
  const int nac = a.nb * a.C;
  for (int r = threadIdx.x; r < nac; r += 256) acc[TQ_GS_ELBO] += (double)a.aoi_part[2 * B + r];
  tq_sums_finish(a, acc, s_w);
}

// ... for a workgroup that goes on to read gsum itself (single-GPU steps: no all-reduce between the sums and the global
// sites): ends with gsum stored, a workgroup-scope fence and a barrier
__device__ __forceinline__ void tq_reduce_sums_fenced_body(const tq_cosmos_args& a, const int64_t nblk, const int64_t B,
                                                           double (*s_w)[TQ_MAX_NGSUM]) {
  tq_reduce_sums_body(a, nblk, B, s_w);
  __threadfence_block();
  __syncthreads();
}

// ---- finish the cross-unit sums in fp64 (single workgroup; sharded runs all-reduce gsum after it) ------------------
__global__ __launch_bounds__(256) void tq_reduce_kernel(const tq_cosmos_args a, const int64_t nblk, const int64_t B) {
  __shared__ double s_w[4][TQ_MAX_NGSUM];
  tq_reduce_sums_body(a, nblk, B, s_w);
}

__global__ __launch_bounds__(256) void tq_reduce_globals_kernel(const tq_cosmos_args a, const int64_t nblk, const int64_t B) {
  __shared__ double s_w[4][TQ_MAX_NGSUM];
  __shared__ double s_e[TQ_NGSITES(TQ_MAXQ)];
  tq_reduce_sums_fenced_body(a, nblk, B, s_w);
  tq_globals_from_gsum_body(a, s_e);
}

// AOI-sharded runs: everything of a step that follows the all-reduce of gsum, in one single-workgroup launch -- global
// sites, total ELBO, Adam of the per-AOI / global parameters -- and, if `has_next`, the global draws of the next step.
__global__ __launch_bounds__(256) void tq_tail_reduced_kernel(const tq_cosmos_args a, const tq_cosmos_args next,
                                                              const int has_next) {
  __shared__ double s_e[TQ_NGSITES(TQ_MAXQ)];
  tq_globals_from_gsum_body(a, s_e);
  __syncthreads();
  const int64_t total = tq_num_params(a);
  const int64_t first = a.fuse_adam ? tq_aoi_base(a) : total;  // minibatch steps: the dense Adam is its own launch
  for (int64_t j = first + threadIdx.x; j < total; j += 256) tq_body_adam(a, j);
  if (has_next) {
    __threadfence();
    __syncthreads();
    const int ns = tq_num_gsites(next);
    if ((threadIdx.x & 63) == 0)
      for (int s = threadIdx.x >> 6; s < ns; s += 4) tq_body_sample_globals(next, s);
  }
}
