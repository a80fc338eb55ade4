// The arithmetic of "a row against a speaker model" (include/voicemap_hip.h, the speaker-model contract): the helpers that enrol.hip
// (vm_speaker_sums / vm_speaker_identify / vm_speaker_trial_hist) and reseg.hip (vm_reseg) share, so that both score bit-identically.
// Everything is float64 until en_finish rounds a score to fp32 ONCE.
#pragma once
#include "common.hpp"

namespace vm {

constexpr int EN_MAX_E = 256;

template <int KIND>
__device__ inline double en_acc(double acc, double q, double p) {
    if (KIND == VM_DIST_EUCLIDEAN) {
        const double d = q - p;
        return fma(d, d, acc);
    }
    return fma(q, p, acc);
}
template <int KIND>
__device__ inline float en_finish(double acc, double qn, double pn) {
    if (KIND == VM_DIST_EUCLIDEAN) return (float)__dsqrt_rn(acc);
    if (KIND == VM_DIST_COSINE) return (float)(1.0 - acc / (qn * pn));
    return (float)(-acc);
}

__device__ inline double en_row_norm(const float* __restrict__ x, int E) {
    double s = 0.0;
    for (int e = 0; e < E; ++e) {
        const double v = (double)x[e];
        s = fma(v, v, s);
    }
    return __dsqrt_rn(s);
}

// one row's contribution to its model's sum: the row itself (euclidean) or its unit vector (cosine, dot_product)
template <int KIND>
__device__ inline double en_contrib(double v, double row_norm) {
    return KIND == VM_DIST_EUCLIDEAN ? v : v / row_norm;
}

// a model's component from its sums: Sigma / n (euclidean, cosine) | (msum / n) (Sigma / n) (dot_product)
template <int KIND>
__device__ inline double en_model(double sum, double msum, double n) {
    const double p = sum / n;
    return KIND == VM_DIST_DOT ? (msum / n) * p : p;
}

// out[r] = en_row_norm of row r of x (rows, E): one launch (defined in enrol.hip)
void launch_en_rownorm(const float* x, int64_t rows, int E, double* out, hipStream_t st);

}  // namespace vm
