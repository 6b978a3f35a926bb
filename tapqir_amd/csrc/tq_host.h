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

// torch.optim.Adam settings a fit kernel supports (written so that a NaN fails)
static inline bool tq_adam_settings_ok(double lr, double beta1, double beta2, double eps) {
  return lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0;
}
