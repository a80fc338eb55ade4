// Score normalisation (S-norm, AS-norm) of speaker-model trials (voicemap_amd/enrolment.py model_score_norm / model_trial_metrics(norm=)):
// what cohort.hip and vm_pair_score_hist_norm are to all-pairs verification, for trials (utterance, enrolled model), geometric or
// multi-session PLDA.  include/voicemap_hip.h states the definitions; DESIGN section 8n the launch shapes.
//
//  * vm_speaker_loo_sums: the VIRTUAL model of every row -- its own speaker's sums without the row (Sigma = sum_s - c_m, msum likewise,
//    n = count_s - 1), c_m and |e_m| formed as vm_speaker_sums forms them, one float64 subtraction per component.  Scoring the cohort
//    rows against these models gives the own-side statistics of leave-one-out trials.
//  * vm_[plda_]speaker_cohort_stats: vm_cohort_topk_stats' selection and statistics over the scores of rows against MODELS, per row
//    over the models (side 0) or per model over the rows (side 1).  A chunk of lines at a time: the score tile is written by
//    vm_[plda_]speaker_identify ITSELF (labels all -1, leave_one_out 0) -- the scores are that matrix, not a copy of its arithmetic -- and
//    cohort.hip's radix select runs down the rows of the tile (side 0: a chunk of rows x all models) or down its COLUMNS (side 1: all
//    rows x a chunk of models; the keys are staged with a strided read, so no second, transposed tile exists).  The tile cap is
//    cohort.hip's.  No float atomics: bit-identical from run to run.
//  * vm_[plda_]speaker_trial_hist_norm -- the trial histograms on s' = 0.5f ((s - mu_q[m]) rsig_q[m] + (s - mu_M) rsig_M) -- are not
//    here: they are the NORM instantiation of the one tile kernel and one histogram launcher of enrol_tile.hpp and stand next to their
//    plain forms in enrol.hip / plda_enrol.hip, so trials, classes, windows, slots and the raw score are the plain histograms' by
//    construction.
#include "enrol_tile.hpp"

namespace vm {

// grid M x 256 threads: thread e owns component e of row m (E <= 256).  norm: en_row_norm of every row (launch_en_rownorm).
template <int KIND>
__global__ __launch_bounds__(256) void en_loo_sums_kernel(const float* __restrict__ q, const int32_t* __restrict__ q_label, int E,
                                                          const double* __restrict__ norm, const double* __restrict__ sums,
                                                          const double* __restrict__ msum, const int32_t* __restrict__ count, int64_t S,
                                                          double* __restrict__ out_sums, double* __restrict__ out_msum,
                                                          int32_t* __restrict__ out_count) {
    const int64_t m = blockIdx.x;
    const int e = (int)threadIdx.x;
    const int32_t s = q_label[m];
    const bool in = s >= 0 && s < S;
    const int32_t n = in ? count[s] : 0;
    const bool ok = n > 1;
    const double nq = norm[m];
    if (e < E) out_sums[m * E + e] = ok ? sums[(int64_t)s * E + e] - en_contrib<KIND>((double)q[m * E + e], nq) : 0.0;
    if (e == 0) {
        out_msum[m] = ok ? msum[s] - nq : 0.0;
        out_count[m] = ok ? n - 1 : 0;
    }
}

// the lines of a statistics call and their chunks: side 0: a line per row (its entries: the S models), side 1: a line per model (the M rows)
struct MnPlan {
    int64_t lines, entries, R, RT;   // R: lines per tile; RT: with topk_idx, half of them (the other half holds the index lists)
    int64_t rows, models;            // of one scoring call at the most
};
static MnPlan mn_plan(int64_t M, int64_t S, int side, bool topk) {
    MnPlan p;
    p.lines = side ? S : M;
    p.entries = side ? M : S;
    p.R = cs_tile_rows(p.lines, p.entries);
    p.RT = topk ? (p.R + 1) / 2 : p.R;
    p.rows = side ? M : p.R;
    p.models = side ? p.R : S;
    return p;
}
// labels (all -1) and the four per-row outputs of the scoring call that nobody reads, the tile (+ the index lists), the scoring call's own
static int64_t mn_ws_bytes(const MnPlan& p, int64_t inner) { return 5 * (p.rows * 4 + 256) + (p.R + 1) * p.entries * 4 + 256 + inner + 256; }

static int mn_check_stats(const char* what, int64_t M, int64_t S, int side, int64_t K, const void* mu, const void* sigma, const void* rsig,
                          const void* cnt) {
    VM_REQUIRE(mu && sigma && rsig && cnt, "%s: null pointer", what);
    VM_REQUIRE(side == 0 || side == 1, "%s: side must be 0 (per row) or 1 (per model), not %d", what, side);
    VM_REQUIRE(K >= 1 && K < (1LL << 31), "%s: K must be in [1, 2^31)", what);
    VM_REQUIRE(M >= 0 && M < (1LL << 31) && S > 0 && S < (1LL << 31), "%s: bad sizes (M, S < 2^31, S >= 1)", what);
    return 0;
}

// The chunk loop of both statistics entry points.  score(q rows, n rows, first model, n models, labels, scores, 4 x unread, ws) writes
// the (n rows, n models) score tile.
template <typename Score>
static int mn_stats(const char* what, int64_t M, int64_t S, int side, int64_t K, float* mu, float* sigma, float* rsig, int32_t* cnt,
                    int32_t* topk_idx, void* ws, hipStream_t st, Score score) {
    const MnPlan p = mn_plan(M, S, side, topk_idx != nullptr);
    int32_t* lab = (int32_t*)en_align(ws);
    float* u0 = (float*)en_align(lab + p.rows);
    int32_t* u1 = (int32_t*)en_align(u0 + p.rows);
    float* u2 = (float*)en_align(u1 + p.rows);
    int32_t* u3 = (int32_t*)en_align(u2 + p.rows);
    float* tile = (float*)en_align(u3 + p.rows);
    void* inner = en_align(tile + (p.R + 1) * p.entries);
    int32_t* list = (int32_t*)(tile + p.RT * p.entries);
    VM_REQUIRE(hipMemsetAsync(lab, 0xff, (size_t)p.rows * 4, st) == hipSuccess, "%s: hipMemsetAsync failed", what);   // every label -1: no own speaker
    for (int64_t l0 = 0; l0 < p.lines; l0 += p.RT) {
        const int64_t n = p.RT < p.lines - l0 ? p.RT : p.lines - l0;
        const int rc = side ? score(0, M, l0, n, lab, tile, u0, u1, u2, u3, inner) : score(l0, n, 0, S, lab, tile, u0, u1, u2, u3, inner);
        if (rc != 0) return rc;
        launch_cohort_select(tile, n, p.entries, K, l0, side ? n : 0, mu, sigma, rsig, cnt, topk_idx, list, st);
        if (const int rc2 = check_launch(what)) return rc2;
    }
    return 0;
}

}  // namespace vm

extern "C" int64_t vm_speaker_loo_sums_workspace_bytes(int64_t M, int E) {
    if (M <= 0 || E <= 0) return 0;
    return M * 8 + 512;
}

extern "C" int vm_speaker_loo_sums(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                   const int32_t* count, int64_t S, int kind, double* out_sums, double* out_msum, int32_t* out_count,
                                   void* ws, void* stream) {
    using namespace vm;
    const char* what = "vm_speaker_loo_sums";
    VM_REQUIRE(q && q_label && sums && msum && count && out_sums && out_msum && out_count && ws, "%s: null pointer", what);
    VM_REQUIRE(E > 0 && E <= EN_MAX_E, "%s: E must be in [1, %d]", what, EN_MAX_E);
    VM_REQUIRE(M >= 0 && M < (1LL << 31) && S > 0 && S < (1LL << 31), "%s: bad sizes (M, S < 2^31, S >= 1)", what);
    VM_REQUIRE(kind >= VM_DIST_EUCLIDEAN && kind <= VM_DIST_DOT, "%s: unknown kind %d", what, kind);
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    double* norm = (double*)en_align(ws);
    launch_en_rownorm(q, M, E, norm, st);
#define VM_EN_LOO(K)                                                                                                                  \
    hipLaunchKernelGGL((en_loo_sums_kernel<K>), dim3((unsigned)M), dim3(256), 0, st, q, q_label, E, (const double*)norm, sums, msum, count, \
                       S, out_sums, out_msum, out_count)
    switch (kind) {
        case VM_DIST_EUCLIDEAN: VM_EN_LOO(VM_DIST_EUCLIDEAN); break;
        case VM_DIST_COSINE: VM_EN_LOO(VM_DIST_COSINE); break;
        default: VM_EN_LOO(VM_DIST_DOT); break;
    }
#undef VM_EN_LOO
    return check_launch(what);
}

extern "C" int64_t vm_speaker_cohort_stats_workspace_bytes(int64_t M, int E, int64_t S, int side) {
    if (M <= 0 || E <= 0 || S <= 0 || side < 0 || side > 1) return 0;
    const vm::MnPlan p = vm::mn_plan(M, S, side, false);
    return vm::mn_ws_bytes(p, vm_speaker_identify_workspace_bytes(p.rows, E, p.models));
}

extern "C" int vm_speaker_cohort_stats(const float* q, int64_t M, int E, const double* sums, const double* msum, const int32_t* count,
                                       int64_t S, int kind, int side, int64_t K, float* mu, float* sigma, float* rsig, int32_t* cnt,
                                       int32_t* topk_idx, void* ws, void* stream) {
    using namespace vm;
    const char* what = "vm_speaker_cohort_stats";
    VM_REQUIRE(q && sums && msum && count && ws, "%s: null pointer", what);
    if (int rc = mn_check_stats(what, M, S, side, K, mu, sigma, rsig, cnt)) return rc;
    VM_REQUIRE(E > 0 && E <= EN_MAX_E, "%s: E must be in [1, %d]", what, EN_MAX_E);
    VM_REQUIRE(kind >= VM_DIST_EUCLIDEAN && kind <= VM_DIST_DOT, "%s: unknown kind %d", what, kind);
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)q) & 15) == 0, "%s: q must be 16-byte aligned when E %% 4 == 0", what);
    if (M == 0) return 0;
    return mn_stats(what, M, S, side, K, mu, sigma, rsig, cnt, topk_idx, ws, (hipStream_t)stream,
                    [&](int64_t r0, int64_t nr, int64_t s0, int64_t ns, int32_t* lab, float* tile, float* u0, int32_t* u1, float* u2,
                        int32_t* u3, void* inner) {
                        return vm_speaker_identify(q + r0 * E, lab, nr, E, sums + s0 * E, msum + s0, count + s0, ns, kind, 0, tile, u0, u1, u2,
                                                   u3, inner, stream);
                    });
}

extern "C" int64_t vm_plda_speaker_cohort_stats_workspace_bytes(int64_t M, int D, int64_t S, int side) {
    if (M <= 0 || D <= 0 || S <= 0 || side < 0 || side > 1) return 0;
    const vm::MnPlan p = vm::mn_plan(M, S, side, false);
    return vm::mn_ws_bytes(p, vm_plda_speaker_identify_workspace_bytes(p.rows, D, p.models));
}

extern "C" int vm_plda_speaker_cohort_stats(const float* q, int64_t M, int P, int D, const double* sums, const int32_t* count, int64_t S,
                                            const double* A, const double* beta, const double* C, const double* G, int n_max, int side,
                                            int64_t K, float* mu, float* sigma, float* rsig, int32_t* cnt, int32_t* topk_idx, void* ws,
                                            void* stream) {
    using namespace vm;
    const char* what = "vm_plda_speaker_cohort_stats";
    VM_REQUIRE(q && sums && count && A && beta && C && G && ws, "%s: null pointer", what);
    if (int rc = mn_check_stats(what, M, S, side, K, mu, sigma, rsig, cnt)) return rc;
    VM_REQUIRE(D >= 1 && D < P && P <= EN_MAX_E && (P & 3) == 0, "%s: 1 <= D < P <= %d and P %% 4 == 0 (P = %d, D = %d)", what, EN_MAX_E, P, D);
    VM_REQUIRE(n_max >= 1, "%s: n_max must be >= 1", what);
    VM_REQUIRE((((uintptr_t)q) & 15) == 0, "%s: q must be 16-byte aligned", what);
    VM_REQUIRE(((((uintptr_t)sums) | ((uintptr_t)A) | ((uintptr_t)beta) | ((uintptr_t)C) | ((uintptr_t)G)) & 7) == 0,
               "%s: sums and the tables must be 8-byte aligned", what);
    if (M == 0) return 0;
    return mn_stats(what, M, S, side, K, mu, sigma, rsig, cnt, topk_idx, ws, (hipStream_t)stream,
                    [&](int64_t r0, int64_t nr, int64_t s0, int64_t ns, int32_t* lab, float* tile, float* u0, int32_t* u1, float* u2,
                        int32_t* u3, void* inner) {
                        return vm_plda_speaker_identify(q + r0 * P, lab, nr, P, D, sums + s0 * P, count + s0, ns, A, beta, C, G, n_max, 0, tile,
                                                        u0, u1, u2, u3, inner, stream);
                    });
}
