// Score calibration for all-pairs speaker verification: the sums that one Newton iteration of prior-weighted logistic regression
// llr = a s + b needs over EVERY trial of vm_pair_score_hist, recomputed and reduced on the chip (train-clean-360: 5.4e9 pairs; the
// scores cannot be stored).  voicemap_amd/calibration.py runs the fit, Cllr and the Bayes-threshold costs on these sums.
//
// Trials, scores and the visited tiles are pair_hist_kernel's (verif.hip): unordered pairs {i, j}, row_lo <= i < row_hi, i < j < N,
// class 0 (target) iff label[i] == label[j]; the fp32 score s comes from score_tile_loop (score_tile.hpp), so it is bit-identical to
// dist[i][j] of vm_pairdist_argmin, and with mu / rsig it is replaced by vh_norm's normalised score.  Only reference tiles that hold
// some j > i are visited and the pairs j <= i are masked.
//
// Per trial, in float64, every operation rounded on its own (cal_terms, calib_terms.hpp -- shared with the speaker-model path of
// enrol_tile.hpp: no fma contraction, so numpy's float64 follows it):
//   z = a s + b + tau;  t = -z (target) or +z;  e = exp(-|t|);  loss = max(t, 0) + log1p(e);
//   p = 1 / (1 + e) if t >= 0 else e / (1 + e);  w = e / (1 + e)^2
// and per class the eight doubles  n, n_skipped, L = sum loss, P0 = sum p, P1 = sum p s, W0 = sum w, W1 = sum w s, W2 = sum (w s) s.
// A trial whose s is NaN or infinite adds to n_skipped alone.
//
// Reduction, in a fixed order throughout: per-lane double accumulators (u32 counts), a shuffle tree per wave, the eight waves of the
// workgroup in order, one partial row per workgroup in the workspace; a second launch (calib_final_kernel, calib_terms.hpp) sums the
// partials (lane l takes partials l, l + 64, ... ascending, then the shuffle tree).  No floating-point atomics: the (2, 8) result is a
// function of the inputs and the grid alone, bit-identical from run to run.
#include "calib_terms.hpp"
#include "score_tile.hpp"

namespace vm {

// grid (query blocks of 64 rows of [row_lo, row_lo + M), splits of the block's reference tiles); 512 threads.  part (CAL_SUMS,
// gridDim.x * gridDim.y) doubles: every workgroup writes its column (zeros where its split holds no tile).
template <int KIND, bool NORM>
__global__ __launch_bounds__(512) void pair_calib_kernel(const float* __restrict__ qT, const float* __restrict__ ref,
                                                         const int32_t* __restrict__ label, int64_t N, int E, int64_t row_lo, int64_t M,
                                                         const float* __restrict__ rsq, const float* __restrict__ wpad, int splits,
                                                         const float* __restrict__ mu, const float* __restrict__ rsig, double a, double b,
                                                         double tau, double* __restrict__ part) {
    constexpr int RT = ST_RT;
    __shared__ __attribute__((aligned(16))) float rs[ST_RT * ST_RP];
    __shared__ double red[8][CAL_SUMS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t mb = row_lo + (int64_t)blockIdx.x * ST_T;   // the block's first query row (global index)
    const int n_tiles = (int)((N + RT - 1) / RT);
    // reference tiles holding some j > i for a query of this block: from the tile of row mb + 1 on, split over blockIdx.y
    const int t_first = (int)((mb + 1) / RT);
    const int tps = (n_tiles - t_first + splits - 1) / splits;
    const int t_lo = t_first + blockIdx.y * tps;
    const int t_hi = min(n_tiles, t_lo + tps);   // <= t_lo: no stage runs and the workgroup's partial is zero

    const int EP = ((E + 3) / 4) * 4, E4 = EP / 4;
    const int64_t m0 = mb + 8 * w;                 // this wave's first query (global row)
    const int64_t ml0 = m0 - row_lo;                // ... as a row of qT
    const int64_t last_group = (M - 1) >> 3;        // a wave past the last query computes on the last group and counts nothing
    const float* qg = qT + ((ml0 >> 3) < last_group ? (ml0 >> 3) : last_group) * (int64_t)E4 * 32;
    const int64_t row_hi = row_lo + M;
    float qn[8];
    int32_t ql[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool ok = m0 + i < row_hi;
        qn[i] = (KIND == VM_DIST_COSINE && ok) ? sqrtf(rsq[m0 + i]) : 1.f;
        if (KIND == VM_SCORE_PLDA) qn[i] = ok ? plda_row_term(rsq[m0 + i]) : 0.f;
        ql[i] = ok ? label[m0 + i] : 0;
    }
    float qmu[8], qrs[8];
    if constexpr (NORM) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = m0 + i < row_hi;
            qmu[i] = ok ? mu[m0 + i] : 0.f;
            qrs[i] = ok ? rsig[m0 + i] : 0.f;
        }
    }
    double sum[2][6];
    uint32_t cnt[2] = {0u, 0u}, skp[2] = {0u, 0u};   // at most 16 trials per lane and tile: no overflow below 2^28 tiles
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) sum[c][k] = 0.0;

    score_tile_loop<KIND>(rs, qg, ref, N, E, wpad, t_lo, t_hi, [&](int64_t n0, const float (&acc)[8][2]) {
        float rn[2] = {1.f, 1.f};
        int32_t rl[2];
        float rmu[2] = {0.f, 0.f}, rrs[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t nn = n0 + lane + 64 * j;
            if (KIND == VM_DIST_COSINE) rn[j] = sqrtf(nn < N ? rsq[nn] : 1.f);
            if (KIND == VM_SCORE_PLDA) rn[j] = nn < N ? rsq[nn] : 0.f;
            rl[j] = nn < N ? label[nn] : 0;
            if constexpr (NORM) {
                rmu[j] = nn < N ? mu[nn] : 0.f;
                rrs[j] = nn < N ? rsig[nn] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t nn = n0 + lane + 64 * j;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t m = m0 + i;
                float d;
                if (KIND == VM_DIST_EUCLIDEAN) {
                    d = sqrtf(acc[i][j]);
                } else if (KIND == VM_SCORE_NEG_EUCLIDEAN) {
                    d = -sqrtf(acc[i][j]);
                } else if (KIND == VM_DIST_COSINE) {
                    d = 1.f - acc[i][j] / (qn[i] * rn[j]);
                } else if (KIND == VM_DIST_DOT) {
                    d = -acc[i][j];
                } else if (KIND == VM_SCORE_PLDA) {
                    d = plda_finish(qn[i], rn[j], acc[i][j]);
                } else {
                    d = acc[i][j];
                }
                if constexpr (NORM) d = vh_norm(d, qmu[i], qrs[i], rmu[j], rrs[j]);
                const bool trial = nn < N && nn > m && m < row_hi;
                const bool fin = (__float_as_uint(d) & 0x7f800000u) != 0x7f800000u;   // neither NaN nor infinite
                const bool tgt = rl[j] == ql[i];
                const bool use = trial && fin;
                cnt[0] += use && tgt;
                cnt[1] += use && !tgt;
                skp[0] += trial && !fin && tgt;
                skp[1] += trial && !fin && !tgt;
                double x[6];
                cal_terms(use ? (double)d : 0.0, tgt, a, b, tau, x);
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    sum[0][k] += (use && tgt) ? x[k] : 0.0;
                    sum[1][k] += (use && !tgt) ? x[k] : 0.0;
                }
            }
        }
    });

    // the wave's sums (a fixed shuffle tree; the counts are integers), then the waves in order
    auto wave_sum_u = [](uint32_t v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint32_t n = wave_sum_u(cnt[c]), ns = wave_sum_u(skp[c]);
        if (lane == 0) {
            red[w][c * CAL_TERMS + 0] = (double)n;
            red[w][c * CAL_TERMS + 1] = (double)ns;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double v = wave_sum_d(sum[c][k]);
            if (lane == 0) red[w][c * CAL_TERMS + 2 + k] = v;
        }
    }
    __syncthreads();
    if (tid < CAL_SUMS) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += red[q][tid];
        const int64_t n_part = (int64_t)gridDim.x * gridDim.y;
        part[tid * n_part + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
    }
}

// the workgroups before the triangle empties the late blocks' ranges: vh_splits' target (verif.hip)
static int cal_splits(int64_t M, int64_t N) { return score_splits(M, N, 4096); }

// workgroups of the largest grid of N rows: cdiv(M, 64) blocks x at most cdiv(4096, blocks) splits < 4096 + blocks
static int64_t cal_max_parts(int64_t N) { return 4096 + cdiv(N, ST_T); }

}  // namespace vm

extern "C" int64_t vm_pair_calib_sums_splits(int64_t M, int64_t N) {
    if (M <= 0 || N <= 0) return 0;
    return vm::cal_splits(M, N);
}

extern "C" int64_t vm_pair_calib_sums_workspace_bytes(int64_t N, int E) {
    if (N <= 0 || E <= 0) return 0;
    const int64_t EP = ((E + 3) / 4) * 4;
    // squared row norms, the zero-padded weights, the scalar-path copy of (up to) all rows as queries, the workgroups' partial sums
    return N * 4 + 256 + vm::ST_MAX_E * 4 + 256 + ((N + 7) / 8) * 8 * EP * 4 + 256 + vm::cal_max_parts(N) * vm::CAL_SUMS * 8 + 256;
}

extern "C" int vm_pair_calib_sums(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights,
                                  int64_t row_lo, int64_t row_hi, const float* mu, const float* rsig, double a, double b, double tau,
                                  double* sums, void* ws, void* stream) {
    using namespace vm;
    const char* what = "vm_pair_calib_sums";
    VM_REQUIRE(emb && label && sums && ws, "%s: null pointer", what);
    VM_REQUIRE((mu == nullptr) == (rsig == nullptr), "%s: mu and rsig come together (both NULL: raw scores)", what);
    VM_REQUIRE(N > 0 && N < (1LL << 31) && E > 0 && E <= ST_MAX_E, "%s: bad sizes (N < 2^31, E <= %d)", what, ST_MAX_E);
    VM_REQUIRE((score_kind >= VM_DIST_EUCLIDEAN && score_kind <= VM_SCORE_NEG_EUCLIDEAN) || score_kind == VM_SCORE_PLDA,
               "%s: unknown score_kind %d", what, score_kind);
    VM_REQUIRE(plda_width_ok(score_kind, E), "%s: VM_SCORE_PLDA needs E %% 4 == 0 and E >= 4", what);
    VM_REQUIRE(score_kind != VM_SCORE_WEIGHTED_L1 || weights, "%s: weighted_l1 needs weights", what);
    VM_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= N, "%s: bad row range", what);
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)emb) & 15) == 0, "%s: emb must be 16-byte aligned when E %% 4 == 0", what);
    VM_REQUIRE((((uintptr_t)sums) & 7) == 0 && (((uintptr_t)ws) & 3) == 0, "%s: sums must be 8-byte, ws 4-byte aligned", what);
    VM_REQUIRE(a - a == 0.0 && b - b == 0.0 && tau - tau == 0.0, "%s: a, b and tau must be finite", what);
    const int64_t M = row_hi - row_lo;
    hipStream_t st = (hipStream_t)stream;
    float* rsq = (float*)ws;
    float* wpad = (float*)(((uintptr_t)(rsq + N) + 255) & ~(uintptr_t)255);
    float* qT = (float*)(((uintptr_t)(wpad + ST_MAX_E) + 255) & ~(uintptr_t)255);
    const int64_t EP = ((E + 3) / 4) * 4;
    double* part = (double*)(((uintptr_t)(qT + ((N + 7) / 8) * 8 * EP) + 255) & ~(uintptr_t)255);
    int64_t n_part = 0;
    if (M > 0) {
        launch_row_scalars(score_kind, emb, N, E, rsq, st);
        launch_pad_weights(score_kind == VM_SCORE_WEIGHTED_L1 ? weights : nullptr, E, wpad, st);
        launch_pairdist_qt(emb + row_lo * (int64_t)E, M, E, qT, st, score_kind == VM_SCORE_PLDA ? E - 1 : -1);
        const int splits = cal_splits(M, N);
        const dim3 grid((unsigned)((M + ST_T - 1) / ST_T), (unsigned)splits);
        n_part = (int64_t)grid.x * grid.y;
        VM_REQUIRE(n_part <= cal_max_parts(N), "%s: %lld workgroups exceed the workspace's %lld partials", what, (long long)n_part,
                   (long long)cal_max_parts(N));
#define VM_CAL(K, NM) hipLaunchKernelGGL((pair_calib_kernel<K, NM>), grid, dim3(512), 0, st, qT, emb, label, N, E, row_lo, M, rsq, wpad, \
                                         splits, mu, rsig, a, b, tau, part)
#define VM_CAL_KIND(NM)                                                  \
    switch (score_kind) {                                                \
        case VM_DIST_EUCLIDEAN: VM_CAL(VM_DIST_EUCLIDEAN, NM); break;    \
        case VM_DIST_COSINE: VM_CAL(VM_DIST_COSINE, NM); break;          \
        case VM_DIST_DOT: VM_CAL(VM_DIST_DOT, NM); break;                \
        case VM_SCORE_WEIGHTED_L1: VM_CAL(VM_SCORE_WEIGHTED_L1, NM); break; \
        case VM_SCORE_PLDA: VM_CAL(VM_SCORE_PLDA, NM); break;            \
        default: VM_CAL(VM_SCORE_NEG_EUCLIDEAN, NM); break;              \
    }
        if (mu == nullptr) {
            VM_CAL_KIND(false);
        } else {
            VM_CAL_KIND(true);
        }
#undef VM_CAL_KIND
#undef VM_CAL
    }
    hipLaunchKernelGGL(calib_final_kernel, dim3(1), dim3(64 * CAL_SUMS), 0, st, part, n_part, sums);
    return check_launch(what);
}
