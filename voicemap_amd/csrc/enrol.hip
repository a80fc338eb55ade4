// Speaker models (voicemap_amd/enrolment.py): enrol every speaker of a cached (N, E) embedding matrix, then score every utterance against
// every speaker MODEL -- S-way identification (rank of the own speaker, best speaker) and model-trial verification (every trial (utterance,
// model) binned by class on the chip, so the M x S matrix need not exist).  The models are the reference's own prototype rules for n > 1
// shots (voicemap/utils.py:159-206: mean embedding / mean unit vector / mean magnitude x mean unit vector), taken to their exhaustive
// limit: k = every speaker, n = every (other) file.
//
// Definitions (include/voicemap_hip.h repeats them; the numpy twins of voicemap_amd/enrolment.py are held to them by the tests).
// Everything is float64 until a score is rounded to fp32 ONCE.
//   |e_u|   = sqrt(sum_e e^2), ascending e, correctly rounded square root.
//   c_u     = e_u (euclidean) | e_u / |e_u| (cosine, dot_product, which also sums the magnitude |e_u|).
//   sum_s   = sum of c_u (msum_s: of |e_u|) over the rows with label s IN ASCENDING ROW ORDER; count_s.  No float atomics anywhere.
//   model of s as seen by query row m: n = count_s, Sigma = sum_s; with leave-one-out and q_label[m] == s: n = count_s - 1,
//             Sigma = sum_s - c_m (msum likewise).  n == 0: no model, (m, s) is not a trial.
//             p = Sigma / n (euclidean, cosine) | (msum / n) (Sigma / n) (dot_product).
//   score   = sqrt(sum_e (q_e - p_e)^2) (direct form) | 1 - q.p / (|q| |p|) | -q.p, sums ascending e with fma.
//   order of the trials of one query: (uint32 key of the fp32 score, speaker index) ascending; the key is vm_pair_score_hist's (-0.0 as
//             +0.0), a NaN score takes key 0xffffffff: after every number, NaN among themselves by speaker index.
//
// Kernels.  en_sums_kernel: one workgroup per speaker walks the labels in row order, 256 at a time; the matching rows of a step are
// compacted in order (ballot + prefix) and added one after the other, thread e owning component e.  en_proto_kernel: the shared models
// P (S, E) and their norms.  en_own_kernel: one thread per query row scores the row against its OWN speaker (the leave-one-out model
// differs from the shared one, so that one score is computed from the sums rather than patched).  The tile kernel is enrol_tile.hpp's
// model_tile_kernel<EnScore<KIND>, MODE, NORM>, the one kernel of "rows against speaker models", shared with plda_enrol.hip: a tile of 64
// query rows x 64 models, both staged through LDS as float64 in chunks of 32 components, thread (tq, ts) holding 4 x 4 accumulators; the
// own-speaker cell takes en_own_kernel's score.  This file gives it the score policy EnScore<KIND> -- the operand P, the norms as row
// and model terms, "a model has n > 0 rows", en_acc / en_finish (enrol_score.hpp, shared with reseg.hip) -- and the launchers of
// enrol_tile.hpp the call EnCall: the argument checks, the scratch layout and the two staging launches.  vm_speaker_identify,
// vm_speaker_trial_hist, vm_speaker_trial_hist_norm and vm_speaker_trial_calib_sums are model_identify / model_trial_hist /
// model_trial_calib on an EnCall: one template, one en_acc / en_finish, so the four entry points score bit-identically.
#include "enrol_tile.hpp"

namespace vm {

__global__ __launch_bounds__(256) void en_rownorm_kernel(const float* __restrict__ x, int64_t rows, int E, double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < rows) out[r] = en_row_norm(x + r * E, E);
}

// grid S, 256 threads: thread e owns component e (E <= 256).  Rows are added in ascending row order.
template <int KIND>
__global__ __launch_bounds__(256) void en_sums_kernel(const float* __restrict__ emb, const int32_t* __restrict__ label, int64_t N, int E,
                                                      const double* __restrict__ norm, double* __restrict__ sums,
                                                      double* __restrict__ msum, int32_t* __restrict__ count) {
    __shared__ int32_t list[256];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int32_t s = (int32_t)blockIdx.x;
    double acc = 0.0, ms = 0.0;
    int32_t cnt = 0;
    for (int64_t base = 0; base < N; base += 256) {
        const int64_t u = base + tid;
        const bool hit = u < N && label[u] == s;
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wcnt[w] = __popcll(b);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            off += k < w ? wcnt[k] : 0;
            total += wcnt[k];
        }
        if (hit) list[off + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)(u - base);
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const int64_t r = base + list[k];
            const double nr = norm[r];
            ms += nr;
            if (tid < E) {
                const double v = (double)emb[r * E + tid];
                acc += en_contrib<KIND>(v, nr);
            }
        }
        cnt += total;
    }
    if (tid < E) sums[(int64_t)s * E + tid] = acc;
    if (tid == 0) {
        msum[s] = ms;
        count[s] = cnt;
    }
}

// grid S, 256 threads: the shared model of every speaker and its norm (count 0: zeros, never a trial).
template <int KIND>
__global__ __launch_bounds__(256) void en_proto_kernel(const double* __restrict__ sums, const double* __restrict__ msum,
                                                       const int32_t* __restrict__ count, int E, double* __restrict__ P,
                                                       double* __restrict__ pn) {
    __shared__ double row[EN_MAX_E];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int32_t n = count[s];
    if (tid < E) {
        const double p = n > 0 ? en_model<KIND>(sums[s * E + tid], msum[s], (double)n) : 0.0;
        P[s * E + tid] = p;
        row[tid] = p;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int e = 0; e < E; ++e) a = fma(row[e], row[e], a);
        pn[s] = __dsqrt_rn(a);
    }
}

// one thread per query row: |q| and the score against the row's own speaker (NaN if there is no such trial).
template <int KIND>
__global__ __launch_bounds__(256) void en_own_kernel(const float* __restrict__ q, const int32_t* __restrict__ q_label, int64_t M, int E,
                                                     const double* __restrict__ sums, const double* __restrict__ msum,
                                                     const int32_t* __restrict__ count, const double* __restrict__ P,
                                                     const double* __restrict__ pn, int64_t S, int loo, double* __restrict__ qn,
                                                     float* __restrict__ own) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float* x = q + m * E;
    const double nq = en_row_norm(x, E);
    qn[m] = nq;
    const int32_t s = q_label[m];
    float out = __uint_as_float(0x7fc00000u);
    const int32_t n = (s >= 0 && s < S) ? count[s] - (loo ? 1 : 0) : 0;
    if (n > 0) {
        double acc = 0.0, pnorm;
        if (!loo) {
            const double* p = P + (int64_t)s * E;
            for (int e = 0; e < E; ++e) acc = en_acc<KIND>(acc, (double)x[e], p[e]);
            pnorm = pn[s];
        } else {
            const double* sg = sums + (int64_t)s * E;
            const double dn = (double)n;
            const double scale = KIND == VM_DIST_DOT ? (msum[s] - nq) / dn : 1.0;
            double a2 = 0.0;
            for (int e = 0; e < E; ++e) {
                const double v = (double)x[e];
                const double c = KIND == VM_DIST_EUCLIDEAN ? v : v / nq;
                double p = (sg[e] - c) / dn;
                if (KIND == VM_DIST_DOT) p = scale * p;
                acc = en_acc<KIND>(acc, v, p);
                a2 = fma(p, p, a2);
            }
            pnorm = __dsqrt_rn(a2);
        }
        out = en_finish<KIND>(acc, nq, pnorm);
    }
    own[m] = out;
}

// The geometric kinds' score policy of model_tile_kernel (enrol_tile.hpp): one model operand P, stages of 32 components (33 KB of LDS, 66 KB
// with the histogram); the row and model terms are the norms |q| and |p|, read for the cosine kind only.
template <int KIND>
struct EnScore {
    static constexpr int EC = 32, NM = 1;
    static constexpr bool PADDED = false;
    const double* op[NM];   // P (S, E)
    const double *pn, *qn;
    int width;              // E, the rows' pitch too
    __device__ double row_term(int64_t m, bool ok) const { return (KIND == VM_DIST_COSINE && ok) ? qn[m] : 1.0; }
    __device__ double model_term(int64_t s, bool ok) const { return (KIND == VM_DIST_COSINE && ok) ? pn[s] : 1.0; }
    __device__ bool count_ok(int32_t n) const { return n > 0; }
    __device__ static double acc(double a, double q, const double (&p)[NM]) { return en_acc<KIND>(a, q, p[0]); }
    __device__ static float finish(double a, double qn, double pn) { return en_finish<KIND>(a, qn, pn); }
};

void launch_en_rownorm(const float* x, int64_t rows, int E, double* out, hipStream_t st) {
    hipLaunchKernelGGL(en_rownorm_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, st, x, rows, E, out);
}

static int64_t en_scratch_bytes(int64_t M, int E, int64_t S) {
    return S * E * 8 + S * 8 + M * 8 + M * 4 + 5 * 256;
}

// The arguments of a geometric call, for the launchers of enrol_tile.hpp.
struct EnCall {
    const float* q;
    const int32_t* q_label;
    int64_t M;
    int E;
    const double *sums, *msum;
    const int32_t* count;
    int64_t S;
    int kind, loo;

    int check(const char* what, const void* ws) const {
        VM_REQUIRE(q && q_label && sums && msum && count && ws, "%s: null pointer", what);
        VM_REQUIRE(E > 0 && E <= EN_MAX_E, "%s: E must be in [1, %d]", what, EN_MAX_E);
        VM_REQUIRE(M >= 0 && M < (1LL << 31) && S > 0 && S < (1LL << 31), "%s: bad sizes (M, S < 2^31, S >= 1)", what);
        VM_REQUIRE(kind >= VM_DIST_EUCLIDEAN && kind <= VM_DIST_DOT, "%s: unknown kind %d", what, kind);
        VM_REQUIRE((E & 3) != 0 || (((uintptr_t)q) & 15) == 0, "%s: q must be 16-byte aligned when E %% 4 == 0", what);
        return 0;
    }

    // scratch: P (S, E), pn (S), qn (M) float64, own (M) fp32.  Prepare: the shared models and every row's own-speaker score.
    template <int K, class Launch>
    void stage_kind(void* ws, hipStream_t st, Launch& launch) const {
        double* P = (double*)en_align(ws);
        double* pn = (double*)en_align(P + S * E);
        double* qn = (double*)en_align(pn + S);
        float* own = (float*)en_align(qn + M);
        hipLaunchKernelGGL((en_proto_kernel<K>), dim3((unsigned)S), dim3(256), 0, st, sums, msum, count, E, P, pn);
        hipLaunchKernelGGL((en_own_kernel<K>), dim3((unsigned)cdiv(M, 256)), dim3(256), 0, st, q, q_label, M, E, sums, msum, count, P, pn, S,
                           loo, qn, own);
        launch(EnScore<K>{{P}, pn, qn, E}, (const float*)own);
    }
    template <class Launch>
    void stage(void* ws, hipStream_t st, Launch launch) const {
        switch (kind) {
            case VM_DIST_EUCLIDEAN: stage_kind<VM_DIST_EUCLIDEAN>(ws, st, launch); break;
            case VM_DIST_COSINE: stage_kind<VM_DIST_COSINE>(ws, st, launch); break;
            default: stage_kind<VM_DIST_DOT>(ws, st, launch); break;
        }
    }
};
}  // namespace vm

extern "C" int64_t vm_speaker_sums_workspace_bytes(int64_t N, int E, int64_t S) {
    if (N <= 0 || E <= 0 || S <= 0) return 0;
    return N * 8 + 512;
}

extern "C" int vm_speaker_sums(const float* emb, const int32_t* label, int64_t N, int E, int64_t S, int kind, double* sums, double* msum,
                               int32_t* count, void* ws, void* stream) {
    using namespace vm;
    VM_REQUIRE(emb && label && sums && msum && count && ws, "vm_speaker_sums: null pointer");
    VM_REQUIRE(E > 0 && E <= EN_MAX_E, "vm_speaker_sums: E must be in [1, %d]", EN_MAX_E);
    VM_REQUIRE(N > 0 && N < (1LL << 31) && S > 0 && S < (1LL << 31), "vm_speaker_sums: bad sizes (1 <= N, S < 2^31)");
    VM_REQUIRE(kind >= VM_DIST_EUCLIDEAN && kind <= VM_DIST_DOT, "vm_speaker_sums: unknown kind %d", kind);
    hipStream_t st = (hipStream_t)stream;
    double* norm = (double*)en_align(ws);
    launch_en_rownorm(emb, N, E, norm, st);
#define VM_EN_SUMS(K) hipLaunchKernelGGL((en_sums_kernel<K>), dim3((unsigned)S), dim3(256), 0, st, emb, label, N, E, norm, sums, msum, count)
    switch (kind) {
        case VM_DIST_EUCLIDEAN: VM_EN_SUMS(VM_DIST_EUCLIDEAN); break;
        case VM_DIST_COSINE: VM_EN_SUMS(VM_DIST_COSINE); break;
        default: VM_EN_SUMS(VM_DIST_DOT); break;
    }
#undef VM_EN_SUMS
    return check_launch("vm_speaker_sums");
}

extern "C" int64_t vm_speaker_identify_workspace_bytes(int64_t M, int E, int64_t S) {
    if (M < 0 || E <= 0 || S <= 0) return 0;
    return vm::en_scratch_bytes(M, E, S);
}

extern "C" int vm_speaker_identify(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                   const int32_t* count, int64_t S, int kind, int leave_one_out, float* scores, float* true_score,
                                   int32_t* rank, float* best_val, int32_t* best_idx, void* ws, void* stream) {
    return vm::model_identify("vm_speaker_identify", vm::EnCall{q, q_label, M, E, sums, msum, count, S, kind, leave_one_out},
                              vm::EnOutputs{scores, true_score, rank, best_val, best_idx}, ws, stream);
}

extern "C" int64_t vm_speaker_trial_hist_workspace_bytes(int64_t M, int E, int64_t S) {
    if (M < 0 || E <= 0 || S <= 0) return 0;
    return vm::en_scratch_bytes(M, E, S);
}

extern "C" int vm_speaker_trial_hist(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                     const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows,
                                     int n_windows, int bins, uint64_t* hist, void* ws, void* stream) {
    return vm::model_trial_hist("vm_speaker_trial_hist", vm::EnCall{q, q_label, M, E, sums, msum, count, S, kind, leave_one_out}, host_windows,
                                n_windows, bins, hist, nullptr, ws, stream);
}

extern "C" int64_t vm_speaker_trial_hist_norm_workspace_bytes(int64_t M, int E, int64_t S) {
    return vm_speaker_trial_hist_workspace_bytes(M, E, S);
}

extern "C" int vm_speaker_trial_hist_norm(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                          const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows,
                                          int n_windows, int bins, const float* mu_q, const float* rsig_q, const float* mu_s,
                                          const float* rsig_s, const float* mu_own, const float* rsig_own, uint64_t* hist, void* ws,
                                          void* stream) {
    const vm::EnNorm n{mu_q, rsig_q, mu_s, rsig_s, mu_own, rsig_own};
    return vm::model_trial_hist("vm_speaker_trial_hist_norm", vm::EnCall{q, q_label, M, E, sums, msum, count, S, kind, leave_one_out},
                                host_windows, n_windows, bins, hist, &n, ws, stream);
}

extern "C" int64_t vm_speaker_trial_calib_sums_splits(int64_t M, int64_t S) {
    if (M <= 0 || S <= 0) return 0;
    return vm::en_hist_splits(M, S);
}

extern "C" int64_t vm_speaker_trial_calib_sums_workspace_bytes(int64_t M, int E, int64_t S) {
    if (M < 0 || E <= 0 || S <= 0) return 0;
    return vm::en_scratch_bytes(M, E, S) + vm::en_calib_part_bytes(M, S);
}

extern "C" int vm_speaker_trial_calib_sums(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                           const int32_t* count, int64_t S, int kind, int leave_one_out, const float* mu_q,
                                           const float* rsig_q, const float* mu_s, const float* rsig_s, const float* mu_own,
                                           const float* rsig_own, double a, double b, double tau, double* calib, void* ws, void* stream) {
    return vm::model_trial_calib("vm_speaker_trial_calib_sums", vm::EnCall{q, q_label, M, E, sums, msum, count, S, kind, leave_one_out},
                                 vm::EnNorm{mu_q, rsig_q, mu_s, rsig_s, mu_own, rsig_own}, a, b, tau, calib, ws, stream);
}
