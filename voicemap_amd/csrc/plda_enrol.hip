// Multi-session PLDA speaker models (voicemap_amd/enrolment.py enrol(plda=...), voicemap_amd/plda.py model_tables): every query row of
// a projected cache against every speaker MODEL of n enrolment rows, scored by minus the two-covariance log-likelihood ratio of the row
// against the n rows -- which depends on the enrolment rows only through their SUM and n (include/voicemap_hip.h states the closed form
// and the arithmetic; trial_scores_plda_numpy is the numpy twin).  The sums and counts are vm_speaker_sums' (euclidean kind) of the
// projected rows; the per-count coefficient tables A, beta, C and G come from the host.
//
// Everything is float64 until a score is rounded to fp32 ONCE.  For the trial (m, s), n = count_s and Sigma = sum_s (with leave-one-out
// and q_label[m] == s: n - 1 and Sigma_d - w_md); no trial unless 1 <= n <= n_max:
//   mu_d = beta[n][d] * Sigma_d;  t = w_md - mu_d;  u = A[n][d] * t;  acc = fma(u, t, acc), ascending d from 0.0
//   g_m  = fma(G[d], w_md * w_md, g_m), ascending d from 0.0
//   score = (float)((acc - g_m) - C[n])
// every product, sum and difference rounded on its own (the helpers below switch contraction off: hipcc would fuse w - beta * Sigma).
//
// Kernels.  pe_prep_kernel: per speaker mu_s = beta[count_s] * sum_s, A_s = A[count_s] and C_s = C[count_s] (zeros where the count is
// out of range: never a trial), so that the tile loop reads two model operands and one query operand.  pe_own_kernel: one thread per
// query row, g_m and the score against the row's OWN speaker (under leave-one-out that model differs from the shared one: the score is
// computed from the sums and the tables rather than patched).  The tile kernel is enrol_tile.hpp's model_tile_kernel<PeScore, MODE,
// NORM>, the one kernel shared with enrol.hip -- 64 query rows x 64 models, thread (tq, ts) holding 4 x 4 float64 accumulators -- with
// the score policy PeScore below: THREE float64 operands staged through LDS (w, mu, A), hence stages of 16 components.  The launchers
// are enrol_tile.hpp's too, on the call PeCall (checks, scratch layout, the two staging launches): vm_plda_speaker_identify,
// _trial_hist, _trial_hist_norm and _trial_calib_sums are model_identify / model_trial_hist / model_trial_calib on a PeCall.  One
// pe_acc / pe_finish: the four entry points score bit-identically.  No float atomics.
#include "enrol_tile.hpp"

namespace vm {

constexpr int PE_MAX_P = 256;   // the widest PLDA-space row (ST_MAX_E)

__device__ inline double pe_mu(double beta, double sigma) {
#pragma clang fp contract(off)
    return beta * sigma;
}
__device__ inline double pe_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ inline double pe_acc(double acc, double w, double mu, double a) {
#pragma clang fp contract(off)
    const double t = w - mu;
    const double u = a * t;
    return fma(u, t, acc);
}
__device__ inline double pe_g(double g, double G, double w) {
#pragma clang fp contract(off)
    const double ww = w * w;   // exact: w is an fp32 value
    return fma(G, ww, g);
}
__device__ inline float pe_finish(double acc, double g, double c) {
#pragma clang fp contract(off)
    const double a = acc - g;
    return (float)(a - c);
}

__device__ inline bool pe_count_ok(int64_t n, int n_max) { return n >= 1 && n <= (int64_t)n_max; }

// grid S, 256 threads: thread d owns component d (D < 256)
__global__ __launch_bounds__(256) void pe_prep_kernel(const double* __restrict__ sums, const int32_t* __restrict__ count, int P, int D,
                                                      const double* __restrict__ A, const double* __restrict__ beta,
                                                      const double* __restrict__ C, int n_max, double* __restrict__ mu,
                                                      double* __restrict__ As, double* __restrict__ Cs) {
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t n = count[s];
    const bool ok = pe_count_ok(n, n_max);
    if (tid < D) {
        mu[s * D + tid] = ok ? pe_mu(beta[n * D + tid], sums[s * P + tid]) : 0.0;
        As[s * D + tid] = ok ? A[n * D + tid] : 0.0;
    }
    if (tid == 0) Cs[s] = ok ? C[n] : 0.0;
}

// one thread per query row: g_m and the score against the row's own speaker (NaN if there is no such trial)
__global__ __launch_bounds__(256) void pe_own_kernel(const float* __restrict__ q, const int32_t* __restrict__ q_label, int64_t M, int P, int D,
                                                     const double* __restrict__ sums, const int32_t* __restrict__ count, int64_t S,
                                                     const double* __restrict__ A, const double* __restrict__ beta,
                                                     const double* __restrict__ C, const double* __restrict__ G, int n_max, int loo,
                                                     const double* __restrict__ mu, const double* __restrict__ As,
                                                     double* __restrict__ gq, float* __restrict__ own) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float* x = q + m * P;
    double g = 0.0;
    for (int d = 0; d < D; ++d) g = pe_g(g, G[d], (double)x[d]);
    gq[m] = g;
    const int32_t s = q_label[m];
    float out = __uint_as_float(0x7fc00000u);
    const int64_t n = (s >= 0 && s < S) ? (int64_t)count[s] - (loo ? 1 : 0) : 0;
    if (pe_count_ok(n, n_max)) {
        double acc = 0.0;
        if (!loo) {
            const double* pm = mu + (int64_t)s * D;
            const double* pa = As + (int64_t)s * D;
            for (int d = 0; d < D; ++d) acc = pe_acc(acc, (double)x[d], pm[d], pa[d]);
        } else {
            const double* sg = sums + (int64_t)s * P;
            const double* bt = beta + n * D;
            const double* at = A + n * D;
            for (int d = 0; d < D; ++d) {
                const double w = (double)x[d];
                acc = pe_acc(acc, w, pe_mu(bt[d], pe_sub(sg[d], w)), at[d]);
            }
        }
        out = pe_finish(acc, g, C[n]);
    }
    own[m] = out;
}

// The PLDA score policy of model_tile_kernel (enrol_tile.hpp): TWO float64 model operands (mu, A) beside the query operand, hence stages
// of 16 components rather than 32: 25 KB of LDS, and 58 KB with the histogram, so that two workgroups still share a compute unit.  The
// row term is g_m, the model term C_s.  Columns >= D of q (zeros and the row term h) are never used; P % 4 == 0 and q is 16-byte aligned.
struct PeScore {
    static constexpr int EC = 16, NM = 2;
    static constexpr bool PADDED = true;   // D < P, P % 4 == 0
    const double* op[NM];   // mu, As (S, D)
    const double *Cs, *gq;
    int width, pitch, n_max;   // D, P
    __device__ double row_term(int64_t m, bool ok) const { return ok ? gq[m] : 0.0; }
    __device__ double model_term(int64_t s, bool ok) const { return ok ? Cs[s] : 0.0; }
    __device__ bool count_ok(int64_t n) const { return pe_count_ok(n, n_max); }
    __device__ static double acc(double a, double w, const double (&p)[NM]) { return pe_acc(a, w, p[0], p[1]); }
    __device__ static float finish(double a, double g, double c) { return pe_finish(a, g, c); }
};

static int64_t pe_scratch_bytes(int64_t M, int D, int64_t S) { return 2 * S * D * 8 + S * 8 + M * 8 + M * 4 + 6 * 256; }

// The arguments of a multi-session PLDA call, for the launchers of enrol_tile.hpp.
struct PeCall {
    const float* q;
    const int32_t* q_label;
    int64_t M;
    int P, D;
    const double* sums;
    const int32_t* count;
    int64_t S;
    const double *A, *beta, *C, *G;
    int n_max, loo;

    int check(const char* what, const void* ws) const {
        VM_REQUIRE(q && q_label && sums && count && A && beta && C && G && ws, "%s: null pointer", what);
        VM_REQUIRE(D >= 1 && D < P && P <= PE_MAX_P && (P & 3) == 0, "%s: 1 <= D < P <= %d and P %% 4 == 0 (P = %d, D = %d)", what, PE_MAX_P, P,
                   D);
        VM_REQUIRE(M >= 0 && M < (1LL << 31) && S > 0 && S < (1LL << 31), "%s: bad sizes (M, S < 2^31, S >= 1)", what);
        VM_REQUIRE(n_max >= 1, "%s: n_max must be >= 1", what);
        VM_REQUIRE((((uintptr_t)q) & 15) == 0, "%s: q must be 16-byte aligned", what);
        VM_REQUIRE(((((uintptr_t)sums) | ((uintptr_t)A) | ((uintptr_t)beta) | ((uintptr_t)C) | ((uintptr_t)G)) & 7) == 0,
                   "%s: sums and the tables must be 8-byte aligned", what);
        return 0;
    }

    // scratch: mu, As (S, D), Cs (S), gq (M) float64, own (M) fp32.  Prepare: the per-speaker operands and every row's g and own score.
    template <class Launch>
    void stage(void* ws, hipStream_t st, Launch launch) const {
        double* mu = (double*)en_align(ws);
        double* As = (double*)en_align(mu + S * D);
        double* Cs = (double*)en_align(As + S * D);
        double* gq = (double*)en_align(Cs + S);
        float* own = (float*)en_align(gq + M);
        hipLaunchKernelGGL(pe_prep_kernel, dim3((unsigned)S), dim3(256), 0, st, sums, count, P, D, A, beta, C, n_max, mu, As, Cs);
        hipLaunchKernelGGL(pe_own_kernel, dim3((unsigned)cdiv(M, 256)), dim3(256), 0, st, q, q_label, M, P, D, sums, count, S, A, beta, C, G,
                           n_max, loo, (const double*)mu, (const double*)As, gq, own);
        launch(PeScore{{mu, As}, Cs, gq, D, P, n_max}, (const float*)own);
    }
};

}  // namespace vm

extern "C" int64_t vm_plda_speaker_identify_workspace_bytes(int64_t M, int D, int64_t S) {
    if (M < 0 || D <= 0 || S <= 0) return 0;
    return vm::pe_scratch_bytes(M, D, S);
}

extern "C" int vm_plda_speaker_identify(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                        const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                        const double* G, int n_max, int leave_one_out, float* scores, float* true_score, int32_t* rank,
                                        float* best_val, int32_t* best_idx, void* ws, void* stream) {
    return vm::model_identify("vm_plda_speaker_identify", vm::PeCall{q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out},
                              vm::EnOutputs{scores, true_score, rank, best_val, best_idx}, ws, stream);
}

extern "C" int64_t vm_plda_speaker_trial_hist_workspace_bytes(int64_t M, int D, int64_t S) {
    if (M < 0 || D <= 0 || S <= 0) return 0;
    return vm::pe_scratch_bytes(M, D, S);
}

extern "C" int vm_plda_speaker_trial_hist(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                          const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                          const double* G, int n_max, int leave_one_out, const int64_t* host_windows, int n_windows,
                                          int bins, uint64_t* hist, void* ws, void* stream) {
    return vm::model_trial_hist("vm_plda_speaker_trial_hist",
                                vm::PeCall{q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out}, host_windows, n_windows,
                                bins, hist, nullptr, ws, stream);
}

extern "C" int64_t vm_plda_speaker_trial_hist_norm_workspace_bytes(int64_t M, int D, int64_t S) {
    return vm_plda_speaker_trial_hist_workspace_bytes(M, D, S);
}

extern "C" int vm_plda_speaker_trial_hist_norm(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                               const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                               const double* G, int n_max, int leave_one_out, const int64_t* host_windows, int n_windows,
                                               int bins, const float* mu_q, const float* rsig_q, const float* mu_s, const float* rsig_s,
                                               const float* mu_own, const float* rsig_own, uint64_t* hist, void* ws, void* stream) {
    const vm::EnNorm n{mu_q, rsig_q, mu_s, rsig_s, mu_own, rsig_own};
    return vm::model_trial_hist("vm_plda_speaker_trial_hist_norm",
                                vm::PeCall{q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out}, host_windows, n_windows,
                                bins, hist, &n, ws, stream);
}

extern "C" int64_t vm_plda_speaker_trial_calib_sums_workspace_bytes(int64_t M, int D, int64_t S) {
    if (M < 0 || D <= 0 || S <= 0) return 0;
    return vm::pe_scratch_bytes(M, D, S) + vm::en_calib_part_bytes(M, S);
}

extern "C" int vm_plda_speaker_trial_calib_sums(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                                const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                                const double* G, int n_max, int leave_one_out, const float* mu_q, const float* rsig_q,
                                                const float* mu_s, const float* rsig_s, const float* mu_own, const float* rsig_own,
                                                double a, double b, double tau, double* calib, void* ws, void* stream) {
    return vm::model_trial_calib("vm_plda_speaker_trial_calib_sums",
                                 vm::PeCall{q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out},
                                 vm::EnNorm{mu_q, rsig_q, mu_s, rsig_s, mu_own, rsig_own}, a, b, tau, calib, ws, stream);
}
