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
// computed from the sums and the tables rather than patched).  pe_tile_kernel<HIST>: en_tile_kernel's (enrol.hip) tile -- 64 query rows
// x 64 models, thread (tq, ts) holding 4 x 4 float64 accumulators -- with THREE float64 operands staged through LDS (w, mu, A), hence in
// chunks of 16 components rather than 32: 25 KB, and 58 KB with the histogram, so that two workgroups still share a compute unit.  The
// epilogue -- the order of the trials, rank / best, the class histogram -- is enrol_tile.hpp's, word for word en_tile_kernel's.  One
// template, one pe_acc / pe_finish: the two entry points score bit-identically.  No float atomics.  NORM = true (HIST only;
// vm_plda_speaker_trial_hist_norm, enrol_norm.hip): the finished score is normalised with the statistics of `nrm` (EN_NORM_*,
// enrol_tile.hpp) before it is binned.  pe_trial_hist is the whole histogram call, with or without the statistics.
#include "enrol_tile.hpp"

namespace vm {

constexpr int PE_EC = 16;       // components per stage
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

// grid (query tiles of 64 rows, splits of the model tiles (HIST only)); 256 threads: ts = tid & 15 owns the models
// {2 ts, 2 ts + 1, 32 + 2 ts, 33 + 2 ts} of a tile, tq = tid >> 4 the queries 4 tq .. 4 tq + 3 (en_tile_kernel's map).
template <bool HIST, bool NORM>
__global__ __launch_bounds__(256) void pe_tile_kernel(const float* __restrict__ q, const int32_t* __restrict__ q_label, int64_t M, int P, int D,
                                                      const double* __restrict__ mu, const double* __restrict__ As,
                                                      const double* __restrict__ Cs, const int32_t* __restrict__ count, int64_t S,
                                                      int n_max, int loo, const double* __restrict__ gq, const float* __restrict__ own,
                                                      float* __restrict__ scores, float* __restrict__ true_score,
                                                      int32_t* __restrict__ rank, float* __restrict__ best_val,
                                                      int32_t* __restrict__ best_idx, EnWindows win, int n_win, int bins, int splits,
                                                      unsigned long long* __restrict__ ghist, EnNorm nrm) {
    __shared__ __attribute__((aligned(16))) double qs[PE_EC * EN_LD];
    __shared__ __attribute__((aligned(16))) double ms[PE_EC * EN_LD];
    __shared__ __attribute__((aligned(16))) double as[PE_EC * EN_LD];
    __shared__ uint32_t hist[HIST ? EN_LDS_HIST_WORDS : 1];
    const int tid = threadIdx.x, lane = tid & 63, ts = tid & 15, tq = tid >> 4;
    (void)lane;
    const int slots = bins + 3;
    const int n_words = n_win * 2 * slots;
    const int64_t mb = (int64_t)blockIdx.x * EN_TQ;
    const int n_tiles = (int)((S + EN_TS - 1) / EN_TS);
    const int tps = (n_tiles + splits - 1) / splits;
    const int t_lo = blockIdx.y * tps;
    const int t_hi = min(n_tiles, t_lo + tps);
    if (t_lo >= t_hi) return;   // workgroup-uniform
    if (HIST) {
        for (int i = tid; i < n_words; i += 256) hist[i] = 0u;
    }

    const float nanf_ = __uint_as_float(0x7fc00000u);
    int32_t ql[4];
    bool okm[4], own_ok[4];
    double gv[4];
    float ownv[4];
    uint32_t okey[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = mb + tq * 4 + i;
        okm[i] = m < M;
        int32_t l = okm[i] ? q_label[m] : -1;
        if (l < 0 || l >= S) l = -1;
        ql[i] = l;
        own_ok[i] = l >= 0 && pe_count_ok((int64_t)count[l] - (loo ? 1 : 0), n_max);
        gv[i] = okm[i] ? gq[m] : 0.0;
        ownv[i] = okm[i] ? own[m] : nanf_;
        okey[i] = score_key_nan_last(ownv[i]);
    }
    EN_TILE_STATE;
    EN_NORM_ROWS

    const int nchunk = (D + PE_EC - 1) / PE_EC;
    const int n_stage = (t_hi - t_lo) * nchunk;   // workgroup-uniform: every barrier below is reached by all 256 threads
    // a stage = 64 query rows x 16 components (fp32, one piece of 4 per thread; P % 4 == 0 and q is 16-byte aligned) and 64 models x
    // 16 components of mu and of A (fp64, 2 pieces of 2 each).  Columns >= D of q (zeros and the row term h) are never used.
    auto fetch = [&](int st, f32x4& vq, f64x2 (&vm_)[2], f64x2 (&va)[2]) {
        const int ec = (st % nchunk) * PE_EC;
        const int64_t s0 = (int64_t)(t_lo + st / nchunk) * EN_TS;
        {
            const int r = tid >> 2, c = ec + (tid & 3) * 4;
            const int64_t row = mb + r;
            const bool ok = row < M && c < D;   // c < D < P and c % 4 == 0: the 4 floats lie inside the row
            const f32x4 x = *reinterpret_cast<const f32x4*>(q + (ok ? row * P + c : 0));
#pragma unroll
            for (int u = 0; u < 4; ++u) vq[u] = (ok && c + u < D) ? x[u] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * k, r = piece >> 3, c = ec + (piece & 7) * 2;
            const int64_t row = s0 + r;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bool ok = row < S && c + u < D;
                vm_[k][u] = ok ? mu[row * D + c + u] : 0.0;
                va[k][u] = ok ? As[row * D + c + u] : 0.0;
            }
        }
    };
    auto stash = [&](const f32x4& vq, const f64x2 (&vm_)[2], const f64x2 (&va)[2]) {
        {
            const int r = tid >> 2, c = (tid & 3) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) qs[(c + u) * EN_LD + r] = (double)vq[u];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * k, r = piece >> 3, c = (piece & 7) * 2;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                ms[(c + u) * EN_LD + r] = vm_[k][u];
                as[(c + u) * EN_LD + r] = va[k][u];
            }
        }
    };
    f32x4 nq;
    f64x2 nm[2], na[2];
    fetch(0, nq, nm, na);
    double acc[4][4];
    for (int st = 0; st < n_stage; ++st) {
        const int t = t_lo + st / nchunk, ck = st % nchunk;
        const int ew = min(PE_EC, D - ck * PE_EC);
        __syncthreads();   // the previous stage's readers are done (and, at st = 0, the histogram is zero)
        stash(nq, nm, na);
        if (st + 1 < n_stage) fetch(st + 1, nq, nm, na);
        __syncthreads();
        if (ck == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        }
#pragma unroll 4
        for (int e = 0; e < ew; ++e) {
            const f64x2 qa = *reinterpret_cast<const f64x2*>(qs + e * EN_LD + tq * 4);
            const f64x2 qb = *reinterpret_cast<const f64x2*>(qs + e * EN_LD + tq * 4 + 2);
            const f64x2 ma = *reinterpret_cast<const f64x2*>(ms + e * EN_LD + ts * 2);
            const f64x2 mb2 = *reinterpret_cast<const f64x2*>(ms + e * EN_LD + 32 + ts * 2);
            const f64x2 aa = *reinterpret_cast<const f64x2*>(as + e * EN_LD + ts * 2);
            const f64x2 ab = *reinterpret_cast<const f64x2*>(as + e * EN_LD + 32 + ts * 2);
            const double qv[4] = {qa[0], qa[1], qb[0], qb[1]};
            const double mv[4] = {ma[0], ma[1], mb2[0], mb2[1]};
            const double av[4] = {aa[0], aa[1], ab[0], ab[1]};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = pe_acc(acc[i][j], qv[i], mv[j], av[j]);
        }
        if (ck != nchunk - 1) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = (int64_t)t * EN_TS + (j >> 1) * 32 + ts * 2 + (j & 1);
            const bool oks = s < S;
            const double cs = oks ? Cs[s] : 0.0;
            const bool has_model = oks && pe_count_ok((int64_t)count[oks ? s : 0], n_max);
            EN_NORM_MODEL;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t m = mb + tq * 4 + i;
                const bool is_own = oks && (int64_t)ql[i] == s;
                const bool trial = okm[i] && (is_own ? own_ok[i] : has_model);
                float d = pe_finish(acc[i][j], gv[i], cs);
                if (is_own) d = ownv[i];
                EN_NORM_CELL(d)
                EN_TILE_CELL(d)
            }
        }
    }
    EN_TILE_FINISH
}

static int pe_check(const char* what, const void* q, const void* q_label, int64_t M, int P, int D, const void* sums, const void* count,
                    int64_t S, const void* A, const void* beta, const void* C, const void* G, int n_max, const void* ws) {
    VM_REQUIRE(q && q_label && sums && count && A && beta && C && G && ws, "%s: null pointer", what);
    VM_REQUIRE(D >= 1 && D < P && P <= PE_MAX_P && (P & 3) == 0, "%s: 1 <= D < P <= %d and P %% 4 == 0 (P = %d, D = %d)", what, PE_MAX_P, P, D);
    VM_REQUIRE(M >= 0 && M < (1LL << 31) && S > 0 && S < (1LL << 31), "%s: bad sizes (M, S < 2^31, S >= 1)", what);
    VM_REQUIRE(n_max >= 1, "%s: n_max must be >= 1", what);
    VM_REQUIRE((((uintptr_t)q) & 15) == 0, "%s: q must be 16-byte aligned", what);
    VM_REQUIRE(((((uintptr_t)sums) | ((uintptr_t)A) | ((uintptr_t)beta) | ((uintptr_t)C) | ((uintptr_t)G)) & 7) == 0,
               "%s: sums and the tables must be 8-byte aligned", what);
    return 0;
}

struct PeScratch {
    double *mu, *As, *Cs, *gq;
    float* own;
};

static PeScratch pe_scratch(void* ws, int64_t M, int D, int64_t S) {
    PeScratch a;
    a.mu = (double*)en_align(ws);
    a.As = (double*)en_align(a.mu + S * D);
    a.Cs = (double*)en_align(a.As + S * D);
    a.gq = (double*)en_align(a.Cs + S);
    a.own = (float*)en_align(a.gq + M);
    return a;
}

static int64_t pe_scratch_bytes(int64_t M, int D, int64_t S) { return 2 * S * D * 8 + S * 8 + M * 8 + M * 4 + 6 * 256; }

// the per-speaker operands and every row's g and own-speaker score: what both entry points stage before the tile kernel
static void pe_prepare(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums, const int32_t* count, int64_t S,
                       const double* A, const double* beta, const double* C, const double* G, int n_max, int loo, const PeScratch& a,
                       hipStream_t st) {
    hipLaunchKernelGGL(pe_prep_kernel, dim3((unsigned)S), dim3(256), 0, st, sums, count, P, D, A, beta, C, n_max, a.mu, a.As, a.Cs);
    hipLaunchKernelGGL(pe_own_kernel, dim3((unsigned)cdiv(M, 256)), dim3(256), 0, st, q, q_label, M, P, D, sums, count, S, A, beta, C, G,
                       n_max, loo, (const double*)a.mu, (const double*)a.As, a.gq, a.own);
}

}  // namespace vm

extern "C" int64_t vm_plda_speaker_identify_workspace_bytes(int64_t M, int D, int64_t S) {
    if (M < 0 || D <= 0 || S <= 0) return 0;
    return vm::pe_scratch_bytes(M, D, S);
}

extern "C" int vm_plda_speaker_identify(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                        const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                        const double* G, int n_max, int leave_one_out, float* scores, float* true_score, int32_t* rank,
                                        float* best_val, int32_t* best_idx, void* ws, void* stream) {
    using namespace vm;
    const char* what = "vm_plda_speaker_identify";
    if (int rc = pe_check(what, q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, ws)) return rc;
    VM_REQUIRE(true_score && rank && best_val && best_idx, "%s: null pointer", what);
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const PeScratch a = pe_scratch(ws, M, D, S);
    pe_prepare(q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out, a, st);
    const dim3 grid((unsigned)cdiv(M, EN_TQ), 1);
    const EnWindows win{};
    hipLaunchKernelGGL((pe_tile_kernel<false, false>), grid, dim3(256), 0, st, q, q_label, M, P, D, (const double*)a.mu, (const double*)a.As,
                       (const double*)a.Cs, count, S, n_max, leave_one_out, (const double*)a.gq, (const float*)a.own, scores, true_score,
                       rank, best_val, best_idx, win, 0, 0, 1, (unsigned long long*)nullptr, EnNorm{});
    return check_launch(what);
}

extern "C" int64_t vm_plda_speaker_trial_hist_workspace_bytes(int64_t M, int D, int64_t S) {
    if (M < 0 || D <= 0 || S <= 0) return 0;
    return vm::pe_scratch_bytes(M, D, S);
}

extern "C" int vm_plda_speaker_trial_hist(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                          const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                          const double* G, int n_max, int leave_one_out, const int64_t* host_windows, int n_windows,
                                          int bins, uint64_t* hist, void* ws, void* stream) {
    return vm::pe_trial_hist("vm_plda_speaker_trial_hist", q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out,
                             host_windows, n_windows, bins, hist, nullptr, ws, stream);
}

int vm::pe_trial_hist(const char* what, const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                      const int32_t* count, int64_t S, const double* A, const double* beta, const double* C, const double* G, int n_max,
                      int leave_one_out, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist, const EnNorm* norm, void* ws,
                      void* stream) {
    if (int rc = pe_check(what, q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, ws)) return rc;
    EnWindows win{};
    if (int rc = en_windows(what, host_windows, n_windows, bins, hist, &win)) return rc;
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const PeScratch a = pe_scratch(ws, M, D, S);
    pe_prepare(q, q_label, M, P, D, sums, count, S, A, beta, C, G, n_max, leave_one_out, a, st);
    const int64_t qb = cdiv(M, EN_TQ), splits = en_hist_splits(M, S);
    const dim3 grid((unsigned)qb, (unsigned)splits);
#define VM_PE_H(NORM, NRM)                                                                                                                \
    hipLaunchKernelGGL((pe_tile_kernel<true, NORM>), grid, dim3(256), 0, st, q, q_label, M, P, D, (const double*)a.mu, (const double*)a.As, \
                       (const double*)a.Cs, count, S, n_max, leave_one_out, (const double*)a.gq, (const float*)a.own, (float*)nullptr,     \
                       (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, win, n_windows, bins, (int)splits,          \
                       (unsigned long long*)hist, NRM)
    if (norm == nullptr) VM_PE_H(false, EnNorm{});
    else VM_PE_H(true, *norm);
#undef VM_PE_H
    return check_launch(what);
}
