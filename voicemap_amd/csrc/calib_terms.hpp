// The per-trial arithmetic and the final sum of score calibration, shared by the pair path (calib.hip: vm_pair_calib_sums) and the
// speaker-model path (enrol_tile.hpp: vm_[plda_]speaker_trial_calib_sums), so that both reduce the same eight sums of the same terms.
//
// Per trial, in float64, every operation rounded on its own (cal_terms: no fma contraction, so numpy's float64 follows it):
//   z = a s + b + tau;  t = -z (target) or +z;  e = exp(-|t|);  loss = max(t, 0) + log1p(e);
//   p = 1 / (1 + e) if t >= 0 else e / (1 + e);  w = e / (1 + e)^2
// and per class the eight doubles  n, n_skipped, L = sum loss, P0 = sum p, P1 = sum p s, W0 = sum w, W1 = sum w s, W2 = sum (w s) s.
#pragma once
#include "common.hpp"

namespace vm {

constexpr int CAL_TERMS = 8, CAL_SUMS = 2 * CAL_TERMS;

// the per-trial terms of the file comment; s is finite
__device__ inline void cal_terms(double s, bool tgt, double a, double b, double tau, double (&x)[6]) {
#pragma clang fp contract(off)
    const double z = a * s + b + tau;
    const double t = tgt ? -z : z;
    const double e = exp(-fabs(t));
    const double d = 1.0 + e;
    const double w = e / (d * d);
    const double p = t >= 0.0 ? 1.0 / d : e / d;
    x[0] = fmax(t, 0.0) + log1p(e);
    x[1] = p;
    x[2] = p * s;
    x[3] = w;
    x[4] = w * s;
    x[5] = (w * s) * s;
}

// one workgroup of CAL_SUMS waves: wave q sums row q of part (CAL_SUMS, n_part) -- lane l the partials l, l + 64, ... ascending, then
// the shuffle tree -- and lane 0 stores sums[q].  n_part == 0 writes zeros.  (static: one copy per file that includes this.)
static __global__ __launch_bounds__(64 * CAL_SUMS) void calib_final_kernel(const double* __restrict__ part, int64_t n_part,
                                                                            double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    double v = 0.0;
    for (int64_t k = lane; k < n_part; k += 64) v += part[q * n_part + k];
    v = wave_sum_d(v);
    if (lane == 0) sums[q] = v;
}

}  // namespace vm
