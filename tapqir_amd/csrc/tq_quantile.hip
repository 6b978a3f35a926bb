// tq_quantile.hip -- credible intervals of the per-unit variational posteriors on the device (bodies in tq_quantile.h).
// Not on the SVI step path: runs once per fit from compute_params (tapqir/models/cosmos.py:740-776, where the reference
// calls scipy's interval element by element on the host).  Bound by fp64 arithmetic, not by the 24 bytes per element.
#include <hip/hip_runtime.h>

#include "tq_host.h"
#include "tq_quantile.h"

// one lane per element, no LDS.  Lanes of a wave diverge in iteration count (series / continued-fraction length, Newton
// steps, and the regime itself where neighbouring elements differ in concentration); accepted, the kernel runs once per
// fit.  Every loop in the bodies has a fixed cap, so a wave ends whatever its inputs are.
__global__ __launch_bounds__(256) void tq_credible_intervals_kernel(const tq_interval_args a, const double p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) tq_body_interval(a, p, i);
}

extern "C" int tq_credible_intervals(const tq_interval_args* a, void* stream) {
  if (!a || !a->p0 || !a->p1 || !a->ll || !a->ul) {
    tq_set_error("tq_credible_intervals: NULL required pointer");
    return TQ_ERR_ARG;
  }
  if (a->kind != TQ_INTERVAL_GAMMA && a->kind != TQ_INTERVAL_AFFINE_BETA) {
    tq_set_error("tq_credible_intervals: unknown kind");
    return TQ_ERR_ARG;
  }
  if (a->n < 1 || !(a->ci > 0.0 && a->ci < 1.0)) {
    tq_set_error("tq_credible_intervals: n < 1 or ci outside (0, 1)");
    return TQ_ERR_ARG;
  }
  if (a->kind == TQ_INTERVAL_AFFINE_BETA && !(a->high - a->low > 0.0 && a->high - a->low < 1e300)) {
    tq_set_error("tq_credible_intervals: low / high must be finite with low < high");
    return TQ_ERR_ARG;
  }
  const double p = 0.5 * (1.0 - a->ci);
  hipLaunchKernelGGL(tq_credible_intervals_kernel, dim3((unsigned)((a->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a,
                     p);
  return tq_launch_status("tq_credible_intervals_kernel");
}
