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
// differs from the shared one, so that one score is computed from the sums rather than patched).  en_tile_kernel<KIND, HIST>: a tile of
// 64 query rows x 64 models, both staged through LDS as float64 in chunks of 32 components, thread (tq, ts) holding 4 x 4 accumulators;
// the own-speaker cell takes en_own_kernel's score.  HIST = false: the score matrix, and per row the number of speakers before the own
// one and the best (key, speaker) -- integer sums and minima kept in registers over all model tiles and merged over the 16 lanes of a
// row at the end.  HIST = true: the counts by class, exactly as pair_hist_kernel (verif.hip) keeps them: u32 LDS bins, per-lane
// under / over / NaN counts, one flush of 64-bit integer atomics per workgroup.  One template, one en_acc / en_finish (enrol_score.hpp,
// shared with reseg.hip): the two entry points score bit-identically.  What happens to a finished score -- EN_TILE_STATE / EN_TILE_CELL /
// EN_TILE_FINISH -- and the launchers' window parsing and splits live in enrol_tile.hpp, shared with plda_enrol.hip (multi-session PLDA
// models): as text, so that this kernel's instruction stream is what it was.  NORM = true (HIST only; vm_speaker_trial_hist_norm,
// enrol_norm.hip): the finished score is normalised with the statistics of `nrm` (EN_NORM_*, enrol_tile.hpp) before it is binned; the
// plain instantiations never read `nrm`.  en_trial_hist is the whole histogram call, with or without the statistics.
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

// grid (query tiles of 64 rows, splits of the model tiles (HIST only)); 256 threads: ts = tid & 15 owns the models
// {2 ts, 2 ts + 1, 32 + 2 ts, 33 + 2 ts} of a tile, tq = tid >> 4 the queries 4 tq .. 4 tq + 3.  NORM: with HIST only.
template <int KIND, bool HIST, bool NORM>
__global__ __launch_bounds__(256) void en_tile_kernel(const float* __restrict__ q, const int32_t* __restrict__ q_label, int64_t M, int E,
                                                      const double* __restrict__ P, const double* __restrict__ pn,
                                                      const int32_t* __restrict__ count, int64_t S, int loo,
                                                      const double* __restrict__ qn, const float* __restrict__ own,
                                                      float* __restrict__ scores, float* __restrict__ true_score,
                                                      int32_t* __restrict__ rank, float* __restrict__ best_val,
                                                      int32_t* __restrict__ best_idx, EnWindows win, int n_win, int bins, int splits,
                                                      unsigned long long* __restrict__ ghist, EnNorm nrm) {
    __shared__ __attribute__((aligned(16))) double qs[EN_EC * EN_LD];
    __shared__ __attribute__((aligned(16))) double ps[EN_EC * EN_LD];
    __shared__ uint32_t hist[HIST ? EN_LDS_HIST_WORDS : 1];
    const int tid = threadIdx.x, lane = tid & 63, ts = tid & 15, tq = tid >> 4;
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
    double qnv[4];
    float ownv[4];
    uint32_t okey[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = mb + tq * 4 + i;
        okm[i] = m < M;
        int32_t l = okm[i] ? q_label[m] : -1;
        if (l < 0 || l >= S) l = -1;
        ql[i] = l;
        own_ok[i] = l >= 0 && count[l] - (loo ? 1 : 0) > 0;
        qnv[i] = (KIND == VM_DIST_COSINE && okm[i]) ? qn[m] : 1.0;
        ownv[i] = okm[i] ? own[m] : nanf_;
        okey[i] = score_key_nan_last(ownv[i]);
    }
    EN_TILE_STATE;
    EN_NORM_ROWS

    const int nchunk = (E + EN_EC - 1) / EN_EC;
    const int n_stage = (t_hi - t_lo) * nchunk;
    const bool vec = (E & 3) == 0;
    // a stage = 64 query rows x 32 components (fp32, 2 pieces of 4 per thread) and 64 models x 32 components (fp64, 4 pieces of 2)
    auto fetch = [&](int st, f32x4 (&vq)[2], f64x2 (&vp)[4]) {
        const int ec = (st % nchunk) * EN_EC;
        const int64_t s0 = (int64_t)(t_lo + st / nchunk) * EN_TS;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * k, r = piece >> 3, c = ec + (piece & 7) * 4;
            const int64_t row = mb + r;
            if (vec) {
                const bool ok = row < M && c < E;
                const f32x4 x = *reinterpret_cast<const f32x4*>(q + (ok ? row * E + c : 0));
                vq[k] = ok ? x : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) vq[k][u] = (row < M && c + u < E) ? q[row * E + c + u] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int piece = tid + 256 * k, r = piece >> 4, c = ec + (piece & 15) * 2;
            const int64_t row = s0 + r;
#pragma unroll
            for (int u = 0; u < 2; ++u) vp[k][u] = (row < S && c + u < E) ? P[row * E + c + u] : 0.0;
        }
    };
    auto stash = [&](const f32x4 (&vq)[2], const f64x2 (&vp)[4]) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * k, r = piece >> 3, c = (piece & 7) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) qs[(c + u) * EN_LD + r] = (double)vq[k][u];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int piece = tid + 256 * k, r = piece >> 4, c = (piece & 15) * 2;
#pragma unroll
            for (int u = 0; u < 2; ++u) ps[(c + u) * EN_LD + r] = vp[k][u];
        }
    };
    f32x4 nq[2];
    f64x2 np[4];
    fetch(0, nq, np);
    double acc[4][4];
    for (int st = 0; st < n_stage; ++st) {
        const int t = t_lo + st / nchunk, ck = st % nchunk;
        const int ew = min(EN_EC, E - ck * EN_EC);
        __syncthreads();   // the previous stage's readers are done (and, at st = 0, the histogram is zero)
        stash(nq, np);
        if (st + 1 < n_stage) fetch(st + 1, nq, np);
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
            const f64x2 pa = *reinterpret_cast<const f64x2*>(ps + e * EN_LD + ts * 2);
            const f64x2 pb = *reinterpret_cast<const f64x2*>(ps + e * EN_LD + 32 + ts * 2);
            const double qv[4] = {qa[0], qa[1], qb[0], qb[1]};
            const double pv[4] = {pa[0], pa[1], pb[0], pb[1]};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = en_acc<KIND>(acc[i][j], qv[i], pv[j]);
        }
        if (ck != nchunk - 1) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = (int64_t)t * EN_TS + (j >> 1) * 32 + ts * 2 + (j & 1);
            const bool oks = s < S;
            const double pnv = (KIND == VM_DIST_COSINE && oks) ? pn[s] : 1.0;
            const bool has_model = oks && count[s] > 0;
            EN_NORM_MODEL;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t m = mb + tq * 4 + i;
                const bool is_own = oks && (int64_t)ql[i] == s;
                const bool trial = okm[i] && (is_own ? own_ok[i] : has_model);
                float d = en_finish<KIND>(acc[i][j], qnv[i], pnv);
                if (is_own) d = ownv[i];
                EN_NORM_CELL(d)
                EN_TILE_CELL(d)
            }
        }
    }
    EN_TILE_FINISH
}

void launch_en_rownorm(const float* x, int64_t rows, int E, double* out, hipStream_t st) {
    hipLaunchKernelGGL(en_rownorm_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, st, x, rows, E, out);
}

static int en_check_models(const char* what, const void* q, const void* q_label, int64_t M, int E, const void* sums, const void* msum,
                           const void* count, int64_t S, int kind, const void* ws) {
    VM_REQUIRE(q && q_label && sums && msum && count && ws, "%s: null pointer", what);
    VM_REQUIRE(E > 0 && E <= EN_MAX_E, "%s: E must be in [1, %d]", what, EN_MAX_E);
    VM_REQUIRE(M >= 0 && M < (1LL << 31) && S > 0 && S < (1LL << 31), "%s: bad sizes (M, S < 2^31, S >= 1)", what);
    VM_REQUIRE(kind >= VM_DIST_EUCLIDEAN && kind <= VM_DIST_DOT, "%s: unknown kind %d", what, kind);
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)q) & 15) == 0, "%s: q must be 16-byte aligned when E %% 4 == 0", what);
    return 0;
}

struct EnScratch {
    double *P, *pn, *qn;
    float* own;
};

static EnScratch en_scratch(void* ws, int64_t M, int E, int64_t S) {
    EnScratch a;
    a.P = (double*)en_align(ws);
    a.pn = (double*)en_align(a.P + S * E);
    a.qn = (double*)en_align(a.pn + S);
    a.own = (float*)en_align(a.qn + M);
    return a;
}

static int64_t en_scratch_bytes(int64_t M, int E, int64_t S) {
    return S * E * 8 + S * 8 + M * 8 + M * 4 + 5 * 256;
}

// the shared models and every row's own-speaker score: what both entry points stage before the tile kernel
static void en_prepare(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                       const int32_t* count, int64_t S, int kind, int loo, const EnScratch& a, hipStream_t st) {
#define VM_EN_PREP(K)                                                                                                              \
    hipLaunchKernelGGL((en_proto_kernel<K>), dim3((unsigned)S), dim3(256), 0, st, sums, msum, count, E, a.P, a.pn);                 \
    hipLaunchKernelGGL((en_own_kernel<K>), dim3((unsigned)cdiv(M, 256)), dim3(256), 0, st, q, q_label, M, E, sums, msum, count, a.P, \
                       a.pn, S, loo, a.qn, a.own)
    switch (kind) {
        case VM_DIST_EUCLIDEAN: VM_EN_PREP(VM_DIST_EUCLIDEAN); break;
        case VM_DIST_COSINE: VM_EN_PREP(VM_DIST_COSINE); break;
        default: VM_EN_PREP(VM_DIST_DOT); break;
    }
#undef VM_EN_PREP
}

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
    using namespace vm;
    if (int rc = en_check_models("vm_speaker_identify", q, q_label, M, E, sums, msum, count, S, kind, ws)) return rc;
    VM_REQUIRE(true_score && rank && best_val && best_idx, "vm_speaker_identify: null pointer");
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const EnScratch a = en_scratch(ws, M, E, S);
    en_prepare(q, q_label, M, E, sums, msum, count, S, kind, leave_one_out, a, st);
    const dim3 grid((unsigned)cdiv(M, EN_TQ), 1);
    const EnWindows win{};
#define VM_EN_ID(K)                                                                                                                  \
    hipLaunchKernelGGL((en_tile_kernel<K, false, false>), grid, dim3(256), 0, st, q, q_label, M, E, a.P, a.pn, count, S, leave_one_out, \
                       a.qn, a.own, scores, true_score, rank, best_val, best_idx, win, 0, 0, 1, (unsigned long long*)nullptr, EnNorm{})
    switch (kind) {
        case VM_DIST_EUCLIDEAN: VM_EN_ID(VM_DIST_EUCLIDEAN); break;
        case VM_DIST_COSINE: VM_EN_ID(VM_DIST_COSINE); break;
        default: VM_EN_ID(VM_DIST_DOT); break;
    }
#undef VM_EN_ID
    return check_launch("vm_speaker_identify");
}

extern "C" int64_t vm_speaker_trial_hist_workspace_bytes(int64_t M, int E, int64_t S) {
    if (M < 0 || E <= 0 || S <= 0) return 0;
    return vm::en_scratch_bytes(M, E, S);
}

extern "C" int vm_speaker_trial_hist(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                     const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows,
                                     int n_windows, int bins, uint64_t* hist, void* ws, void* stream) {
    return vm::en_trial_hist("vm_speaker_trial_hist", q, q_label, M, E, sums, msum, count, S, kind, leave_one_out, host_windows, n_windows,
                             bins, hist, nullptr, ws, stream);
}

int vm::en_trial_hist(const char* what, const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                      const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows, int n_windows, int bins,
                      uint64_t* hist, const EnNorm* norm, void* ws, void* stream) {
    if (int rc = en_check_models(what, q, q_label, M, E, sums, msum, count, S, kind, ws)) return rc;
    EnWindows win{};
    if (int rc = en_windows(what, host_windows, n_windows, bins, hist, &win)) return rc;
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const EnScratch a = en_scratch(ws, M, E, S);
    en_prepare(q, q_label, M, E, sums, msum, count, S, kind, leave_one_out, a, st);
    const int64_t qb = cdiv(M, EN_TQ), splits = en_hist_splits(M, S);
    const dim3 grid((unsigned)qb, (unsigned)splits);
#define VM_EN_H(K, NORM, NRM)                                                                                                              \
    hipLaunchKernelGGL((en_tile_kernel<K, true, NORM>), grid, dim3(256), 0, st, q, q_label, M, E, a.P, a.pn, count, S, leave_one_out, a.qn, \
                       a.own, (float*)nullptr, (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, win, n_windows,      \
                       bins, (int)splits, (unsigned long long*)hist, NRM)
    if (norm == nullptr) {
        switch (kind) {
            case VM_DIST_EUCLIDEAN: VM_EN_H(VM_DIST_EUCLIDEAN, false, EnNorm{}); break;
            case VM_DIST_COSINE: VM_EN_H(VM_DIST_COSINE, false, EnNorm{}); break;
            default: VM_EN_H(VM_DIST_DOT, false, EnNorm{}); break;
        }
    } else {
        switch (kind) {
            case VM_DIST_EUCLIDEAN: VM_EN_H(VM_DIST_EUCLIDEAN, true, *norm); break;
            case VM_DIST_COSINE: VM_EN_H(VM_DIST_COSINE, true, *norm); break;
            default: VM_EN_H(VM_DIST_DOT, true, *norm); break;
        }
    }
#undef VM_EN_H
    return check_launch(what);
}
