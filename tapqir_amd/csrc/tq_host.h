// tq_host.h -- host-side plumbing shared by the extern "C" entry points of every translation unit: the thread's error
// text, the status of the launch just issued, the launch of a kernel template over K, and the Adam settings the per-sample fits accept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/tapqir_hip.h"

void tq_set_error(const char* msg);  // defined in tq_ksmogn.hip; tq_last_error() returns the text

// TQ_OK, or TQ_ERR_LAUNCH with the error text "<what>: <hip error string>"
static inline int tq_launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    tq_set_error(buf);
    return TQ_ERR_LAUNCH;
  }
  return TQ_OK;
}

// A launch of a kernel template over the number of spots: runs `...` with the compile-time constant KK = K (1..4 = TQ_MAX_K,
// which the entry points have checked), e.g.  TQ_SWITCH_K(a->K, hipLaunchKernelGGL((kern<KK>), grid, block, 0, st, *a));
#define TQ_SWITCH_K(K, ...)                                          \
  switch (K) {                                                       \
    case 1: { constexpr int KK = 1; __VA_ARGS__; } break;            \
    case 2: { constexpr int KK = 2; __VA_ARGS__; } break;            \
    case 3: { constexpr int KK = 3; __VA_ARGS__; } break;            \
    default: { constexpr int KK = 4; __VA_ARGS__; } break;           \
  }

// ---- the hidden-Markov entry points (tq_hmm.hip and every chain unit after it) ------------------------------------------
// runs `...` with the compile-time constant MM = M, which tq_chain_states_ok has checked to be 2, 3 or 4
#define TQ_HMM_SWITCH_M(M, ...)  \
  switch (M) {                   \
    case 2: {                    \
      constexpr int MM = 2;      \
      __VA_ARGS__;               \
    } break;                     \
    case 3: {                    \
      constexpr int MM = 3;      \
      __VA_ARGS__;               \
    } break;                     \
    default: {                   \
      constexpr int MM = 4;      \
      __VA_ARGS__;               \
    } break;                     \
  }

// Argument checks: true, or false with the error text "<who>: <what>", who = the entry point
#define TQ_STR_(x) #x
#define TQ_STR(x) TQ_STR_(x)
static inline bool tq_chain_require(bool ok, const char* who, const char* what) {
  if (ok) return true;
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  tq_set_error(buf);
  return false;
}
static inline bool tq_chain_frames_ok(const char* who, int N, int F) {
  return tq_chain_require(N >= 1 && F >= 1 && F <= TQ_SMOOTH_MAX_F, who,
                          "N and F must be positive and F at most " TQ_STR(TQ_SMOOTH_MAX_F));
}
static inline bool tq_chain_states_ok(const char* who, int U, int B) {
  return tq_chain_require(U >= 1 && B >= 1 && U + B <= TQ_HMM_MAX_STATES, who,
                          "U and B must be at least 1 and U + B at most " TQ_STR(TQ_HMM_MAX_STATES));
}
// an M-step: N rows, iteration `it` of a trace of T entries
static inline bool tq_chain_iteration_ok(const char* who, int N, int it) {
  return tq_chain_require(N >= 1 && it >= 0, who, "N must be positive and it non-negative");
}
// `whose` says whose trace it is, as the text names it: "the trace of a replica"
static inline bool tq_chain_trace_ok(const char* who, int it, int T, const char* whose) {
  char what[120];
  snprintf(what, sizeof(what), "T must exceed it (%s has T entries)", whose);
  return tq_chain_require(T > it, who, what);
}
// ok = tq_multistart_allow_ok(allow, U + B) of tq_multistart.h, which only the units that take a mask include
static inline bool tq_chain_allow_ok(const char* who, bool ok) {
  return tq_chain_require(ok, who, "allow must have no bit beyond M * M and a free entry in every row");
}
static inline bool tq_chain_replicas_ok(const char* who, int R) {
  return tq_chain_require(R >= 1 && R <= TQ_MULTISTART_MAX, who, "R must be at least 1 and at most " TQ_STR(TQ_MULTISTART_MAX));
}
// written so that a NaN fails; the joint chain has two
static inline bool tq_chain_prior_ok(const char* who, double prior) {
  return tq_chain_require(prior > 0.0 && prior < 1.0, who, "prior must lie in (0, 1)");
}
static inline bool tq_chain_priors_ok(const char* who, double prior_a, double prior_b) {
  return tq_chain_require(prior_a > 0.0 && prior_a < 1.0 && prior_b > 0.0 && prior_b < 1.0, who,
                          "prior_a and prior_b must lie in (0, 1)");
}
// the backward samplers: a grid of (N, ceil(S / 64)) waves; the dwell launches also take the table's length
static inline bool tq_chain_sampler_ok(const char* who, int N, int F, int S) {
  return tq_chain_require(N >= 1 && F >= 1 && S >= 1 && F <= TQ_SMOOTH_MAX_F, who,
                          "N, F and S must be positive and F at most " TQ_STR(TQ_SMOOTH_MAX_F));
}
static inline bool tq_chain_dwell_sampler_ok(const char* who, int N, int F, int S, int64_t total) {
  return tq_chain_require(N >= 1 && F >= 1 && S >= 1 && F <= TQ_SMOOTH_MAX_F && total >= 0, who,
                          "N, F and S must be positive, F at most " TQ_STR(TQ_SMOOTH_MAX_F) " and total non-negative");
}
static inline bool tq_chain_sample_grid(const char* who, int N, int S, dim3* grid) {
  *grid = dim3((unsigned)N, (unsigned)((S + 63) / 64));
  return tq_chain_require(grid->y <= 65535u, who, "S too large");
}
// a count kernel stores its four columns as one int4
static inline bool tq_chain_counts_aligned(const char* who, const void* counts) {
  return tq_chain_require(((uintptr_t)counts & 15u) == 0, who, "counts must be 16-byte aligned");
}
// mode is TQ_DWELL_COUNT or TQ_DWELL_EMIT, and the pointers that mode needs are there
static inline bool tq_chain_dwell_mode_ok(const char* who, int mode, bool count_ptrs_ok, bool emit_ptrs_ok) {
  const bool known = mode == TQ_DWELL_COUNT || mode == TQ_DWELL_EMIT;
  return tq_chain_require(known && (mode == TQ_DWELL_COUNT ? count_ptrs_ok : emit_ptrs_ok), who,
                          known ? "NULL required pointer" : "unknown mode");
}

// torch.optim.Adam settings a fit kernel supports (written so that a NaN fails)
static inline bool tq_adam_settings_ok(double lr, double beta1, double beta2, double eps) {
  return lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0;
}
