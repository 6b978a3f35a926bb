// g++ build of the two-channel chain bodies (tapqir_amd/csrc/tq_joint.h over tq_hmm.h) on host memory, for the test
// suite: the batched E-step with the device's ownership of frames by 64 lanes, its scan order over an array of 64 and its
// replica layout, with and without gamma; the batched M-step with the device's strided sums, tree and structures; and the
// Viterbi path.  An inactive replica is skipped where the device's workgroups return.
#include "../../tapqir_amd/csrc/tq_joint.h"

namespace {

constexpr int M = TQ_JOINT_M, COLS = TQ_JOINT_COLS;

// the butterfly of tq_group_sum<64>: after the six exchanges every lane holds the sum; lane 0's is returned
double wave_sum(const double* v) {
  double a[64], b[64];
  for (int i = 0; i < 64; ++i) a[i] = v[i];
  for (int d = 1; d < 64; d <<= 1) {
    for (int i = 0; i < 64; ++i) b[i] = a[i] + a[i ^ d];
    for (int i = 0; i < 64; ++i) a[i] = b[i];
  }
  return a[0];
}

// one workgroup of tq_joint_estep_kernel
void estep_row(const TqJointModel& m, const float* pa, const float* pb, int F, double* filt, double* gam, double* row) {
  static TqHmmMat<M> pre[64], suf[64], old[64];
  int lo[64], hi[64];
  for (int k = 0; k < 64; ++k) {
    tq_smooth_lane_range(k, F, lo[k], hi[k]);
    pre[k] = suf[k] = tq_joint_chunk(m, pa, pb, lo[k], hi[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {  // the kernel's Hillis-Steele steps: all lanes read, then all lanes write
    for (int k = 0; k < 64; ++k) old[k] = pre[k];
    for (int k = d; k < 64; ++k) pre[k] = tq_hmm_mul(old[k - d], old[k]);
  }
  for (int d = 1; d < 64; d <<= 1) {
    for (int k = 0; k < 64; ++k) old[k] = suf[k];
    for (int k = 0; k + d < 64; ++k) suf[k] = tq_hmm_mul(old[k], old[k + d]);
  }
  static double acc[COLS][64];
  for (int k = 0; k < 64; ++k) {
    const TqHmmMat<M> e = k == 0 ? tq_hmm_identity<M>() : pre[k - 1];
    const TqHmmMat<M> s = k == 63 ? tq_hmm_identity<M>() : suf[k + 1];
    double v[M], b[M], a[COLS];
    tq_hmm_prefix_vector(e, v);
    tq_hmm_suffix_vector(s, b);
    if (gam)
      tq_joint_sweeps<true>(m, pa, pb, lo[k], hi[k], v, b, filt, gam, a);
    else
      tq_joint_sweeps<false>(m, pa, pb, lo[k], hi[k], v, b, filt, nullptr, a);
    for (int j = 0; j < COLS; ++j) acc[j][k] = a[j];
  }
  for (int j = 0; j < COLS; ++j) row[j] = wave_sum(acc[j]);
}

}  // namespace

extern "C" {

// theta (R, 20), filt and gamma (R, N, F, 4) (gamma or NULL), rows (R, N, 21); active (R) or NULL
void hk_joint_estep(const float* pa, const float* pb, int N, int F, const double* theta, int R, double prior_a,
                    double prior_b, const int32_t* active, double* filt, double* gamma, double* rows) {
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const TqJointModel m = tq_joint_model(theta + tq_multistart_theta_at<M>(r), prior_a, prior_b);
    for (int n = 0; n < N; ++n) {
      const int64_t at = tq_multistart_filt_at<M>(r, n, N, F);
      estep_row(m, pa + (int64_t)n * F, pb + (int64_t)n * F, F, filt + at, gamma ? gamma + at : nullptr,
                rows + tq_multistart_row_at<M>(r, n, N));
    }
  }
}

// one workgroup of tq_joint_mstep_kernel per replica: theta (R, 20) in place, trace (R, T), structure (R)
void hk_joint_mstep(const double* rows, int N, int R, int T, int it, const int32_t* structure, const int32_t* active,
                    double* theta, double* trace) {
  static double part[COLS][TQ_SMOOTH_MSTEP_THREADS];
  for (int r = 0; r < R; ++r) {
    if (active && active[r] == 0) continue;
    const double* rr = rows + tq_multistart_row_at<M>(r, 0, N);
    for (int t = 0; t < TQ_SMOOTH_MSTEP_THREADS; ++t)
      for (int j = 0; j < COLS; ++j) {
        double s = 0.0;
        for (int n = t; n < N; n += TQ_SMOOTH_MSTEP_THREADS) s += rr[(int64_t)n * COLS + j];
        part[j][t] = s;
      }
    for (int h = TQ_SMOOTH_MSTEP_THREADS / 2; h > 0; h >>= 1)
      for (int t = 0; t < h; ++t)
        for (int j = 0; j < COLS; ++j) part[j][t] += part[j][t + h];
    double sums[COLS];
    for (int j = 0; j < COLS; ++j) sums[j] = part[j][0];
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
