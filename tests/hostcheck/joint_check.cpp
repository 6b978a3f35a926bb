// g++ build of the two-channel chain bodies (tapqir_amd/csrc/tq_joint.h over tq_hmm.h) on host memory, for the test
// suite: the batched E-step with the device's ownership of frames by 64 lanes, its scan order over an array of 64 and its
// replica layout, with and without gamma; the batched M-step with the device's strided sums, tree and structures; and the
// Viterbi path.  An inactive replica is skipped where the device's workgroups return.
#include "../../tapqir_amd/csrc/tq_joint.h"
#include "chain_host.h"

namespace {
constexpr int M = TQ_JOINT_M, COLS = TQ_JOINT_COLS;
}

extern "C" {

// theta (R, 20), filt and gamma (R, N, F, 4) (gamma or NULL), rows (R, N, 21); active (R) or NULL
void hk_joint_estep(const float* pa, const float* pb, int N, int F, const double* theta, int R, double prior_a,
                    double prior_b, const int32_t* active, double* filt, double* gamma, double* rows) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const TqJointModel m = tq_joint_model(theta + tq_multistart_theta_at<M>(r), prior_a, prior_b);
    for (int n = 0; n < N; ++n) {
      const int64_t at = tq_multistart_filt_at<M>(r, n, N, F);
      const TqJointEmit em{m, pa + (int64_t)n * F, pb + (int64_t)n * F};
      double* row = rows + tq_multistart_row_at<M>(r, n, N);
      if (gamma)
        estep_row<M, true>(m, em, F, filt + at, gamma + at, row);
      else
        estep_row<M, false>(m, em, F, filt + at, nullptr, row);
    }
  }
}

// one workgroup of tq_joint_mstep_kernel per replica: theta (R, 20) in place, trace (R, T), structure (R)
void hk_joint_mstep(const double* rows, int N, int R, int T, int it, const int32_t* structure, const int32_t* active,
                    double* theta, double* trace) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    double sums[COLS];
    reduce_rows<COLS>(rows + tq_multistart_row_at<M>(r, 0, N), N, sums);
    tq_joint_mstep_theta(sums, N, structure[r], theta + tq_multistart_theta_at<M>(r));
    trace[(int64_t)r * T + it] = sums[COLS - 1];
  }
}

// the structure applied to sums (21) that the caller gives: theta (20) in place
void hk_joint_mstep_theta(const double* sums, int N, int structure, double* theta) {
  tq_joint_mstep_theta(sums, N, structure, theta);
}

int hk_joint_structure_ok(int structure) { return tq_joint_structure_ok(structure) ? 1 : 0; }

// path (N, F), back ((F + 3) / 4) * N words with the device's stride N
void hk_joint_viterbi(const float* pa, const float* pb, int N, int F, const double* theta, double prior_a, double prior_b,
                      uint32_t* back, uint8_t* path) {
  const TqJointModel m = tq_joint_model(theta, prior_a, prior_b);
  for (int64_t n = 0; n < N; ++n) tq_joint_viterbi_row(m, pa + n * F, pb + n * F, F, back + n, N, path + n * F);
}
}
