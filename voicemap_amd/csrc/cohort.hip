// Cohort score normalisation (S-norm, AS-norm) for all-pairs speaker verification: per query row, the mean and the standard deviation
// of its scores against the K cohort rows most like it (K = C: the whole cohort).  voicemap_amd/verification.py normalises every pair
// score with these statistics of both sides in vm_pair_score_hist_norm (verif.hip).
//
// Per tile of R query rows, two kernels:
//  * cohort_score_kernel: the R x C scores into the workspace, from score_tile_loop (score_tile.hpp) -- so every score is bit-identical
//    to vm_pair_score_hist's (and to dist[m][c] of vm_pairdist_argmin).  The excluded self pair is written as NaN: the selection skips
//    it with the NaN scores.
//  * cohort_select_kernel: one 1024-thread workgroup per row.  The row's C order-preserving uint32 keys (score_key_nan_last; NaN -> 2^32 - 1,
//    above every other key) go into LDS (C <= 32 768) or are re-read from the tile in every round (larger cohorts).  A 4 x 8-bit MSB-first
//    radix select finds the K'-th smallest key T (per-wave 256-bin sub-histograms, wave-aggregated adds for the common digit, one wave
//    scans); the ties at T are cut in index order by a ballot / popcount prefix count.  The selected scores are reduced in float64 in a
//    fixed order (per-thread ascending index, a shuffle tree, then the waves in order): no float atomics, bit-identical from run to run.
//    launch_cohort_select (score_tile.hpp) is its launcher, shared with enrol_norm.hip, which also selects down the COLUMNS of a tile.
#include "score_tile.hpp"

namespace vm {

constexpr int CS_SEL_THREADS = 1024, CS_SEL_WAVES = CS_SEL_THREADS / 64;
constexpr int CS_CAP_SMALL = 4096, CS_CAP_LARGE = 32768;   // keys held in LDS: 16 KiB / 128 KiB (+ 16 KiB of sub-histograms)
constexpr int CS_LOAD_BATCH = 16;                          // score loads per thread in flight while the keys are staged
constexpr int64_t CS_TILE_FLOATS = 48LL << 20;             // the score tile: 192 MiB
constexpr uint32_t CS_KEY_NAN = 0xffffffffu;

// grid (query blocks of 64 of the tile's R rows, splits of the cohort tiles); 512 threads.  out (R, C) fp32.
template <int KIND>
__global__ __launch_bounds__(512) void cohort_score_kernel(const float* __restrict__ qT, const float* __restrict__ cohort, int64_t R, int64_t C,
                                                           int E, int64_t self_col0, const float* __restrict__ qsq,
                                                           const float* __restrict__ rsq, const float* __restrict__ wpad, int tiles_per_split,
                                                           float* __restrict__ out) {
    constexpr int RT = ST_RT;
    __shared__ __attribute__((aligned(16))) float rs[ST_RT * ST_RP];
    const int EP = ((E + 3) / 4) * 4, E4 = EP / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * ST_T + 8 * w;   // this wave's first query (row of the tile)
    const int64_t last_group = (R - 1) >> 3;                  // a wave past the last query computes on the last group and stores nothing
    const float* qg = qT + ((m0 >> 3) < last_group ? (m0 >> 3) : last_group) * (int64_t)E4 * 32;
    float qn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        qn[i] = (KIND == VM_DIST_COSINE && m0 + i < R) ? sqrtf(qsq[m0 + i]) : 1.f;
        if (KIND == VM_SCORE_PLDA) qn[i] = m0 + i < R ? plda_row_term(qsq[m0 + i]) : 0.f;
    }
    const int n_tiles = (int)((C + RT - 1) / RT);
    const int t_lo = blockIdx.y * tiles_per_split;
    const int t_hi = min(n_tiles, t_lo + tiles_per_split);
    score_tile_loop<KIND>(rs, qg, cohort, C, E, wpad, t_lo, t_hi, [&](int64_t n0, const float (&acc)[8][2]) {
        float rn[2] = {1.f, 1.f};
        if (KIND == VM_DIST_COSINE) {
#pragma unroll
            for (int j = 0; j < 2; ++j) rn[j] = sqrtf(n0 + lane + 64 * j < C ? rsq[n0 + lane + 64 * j] : 1.f);
        }
        if (KIND == VM_SCORE_PLDA) {
#pragma unroll
            for (int j = 0; j < 2; ++j) rn[j] = n0 + lane + 64 * j < C ? rsq[n0 + lane + 64 * j] : 0.f;
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
                if (self_col0 >= 0 && nn == self_col0 + m) d = __uint_as_float(0x7fc00000u);   // the row itself: skipped like NaN
                if (m < R && nn < C) out[m * C + nn] = d;   // a wave = 256 contiguous bytes of a row
            }
        }
    });
}

// One workgroup per row r of the score tile sc (rows, C).  CAP > 0: the keys are staged in LDS (C <= CAP); CAP == 0: every pass re-reads
// the row from the tile.  Writes mu / sigma / rsig / count of row row0 + r and, if topk_idx, its K slots; list (rows, C) int32 is the
// scratch of the selected indices in index order (used only with topk_idx).  COL (the speaker-model statistics per MODEL,
// enrol_norm.hip): line r is COLUMN r of a tile (C, ld) -- entry c at sc[c * ld + r] -- staged into the keys with a strided read.
template <int CAP, bool COL>
__global__ __launch_bounds__(CS_SEL_THREADS) void cohort_select_kernel(const float* __restrict__ sc, int64_t C, int64_t K, int64_t row0,
                                                                       int64_t ld,
                                                                       float* __restrict__ mu, float* __restrict__ sigma,
                                                                       float* __restrict__ rsig, int32_t* __restrict__ count,
                                                                       int32_t* __restrict__ topk_idx, int32_t* __restrict__ list) {
    __shared__ uint32_t keys[CAP > 0 ? CAP : 1];
    __shared__ uint32_t hist[CS_SEL_WAVES][256];
    __shared__ uint32_t red_u[CS_SEL_WAVES];
    __shared__ double red_d[CS_SEL_WAVES];
    __shared__ uint32_t sh_digit, sh_k, sh_eq;
    __shared__ int64_t sh_cut;
    const int64_t r = blockIdx.x;
    const float* row = COL ? sc + r : sc + r * C;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    auto score_at = [&](int64_t c) -> float {
        if constexpr (COL) return row[c * ld];
        else return row[c];
    };
    auto key_at = [&](int64_t c) -> uint32_t {
        if constexpr (CAP > 0) return keys[c];
        else return score_key_nan_last(score_at(c));
    };
    // workgroup sums in a fixed order: a shuffle tree per wave, then the waves in order
    auto block_sum_u = [&](uint32_t x) -> uint32_t {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        __syncthreads();   // red_u's previous readers are done
        if (lane == 0) red_u[w] = x;
        __syncthreads();
        uint32_t t = 0;
#pragma unroll
        for (int q = 0; q < CS_SEL_WAVES; ++q) t += red_u[q];
        return t;
    };
    auto block_sum_d = [&](double x) -> double {
        x = wave_sum_d(x);
        __syncthreads();
        if (lane == 0) red_d[w] = x;
        __syncthreads();
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < CS_SEL_WAVES; ++q) t += red_d[q];
        return t;
    };

    // stage the keys, count the NaN (and excluded) entries
    uint32_t nnan = 0;
    for (int64_t c0 = 0; c0 < C; c0 += (int64_t)CS_SEL_THREADS * CS_LOAD_BATCH) {
        float v[CS_LOAD_BATCH];
#pragma unroll
        for (int u = 0; u < CS_LOAD_BATCH; ++u) {
            const int64_t c = c0 + (int64_t)u * CS_SEL_THREADS + tid;
            v[u] = c < C ? score_at(c) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CS_LOAD_BATCH; ++u) {
            const int64_t c = c0 + (int64_t)u * CS_SEL_THREADS + tid;
            if (c < C) {
                const uint32_t k = score_key_nan_last(v[u]);
                if constexpr (CAP > 0) keys[c] = k;
                nnan += k == CS_KEY_NAN;
            }
        }
    }
    nnan = block_sum_u(nnan);   // (its barriers also publish the staged keys)
    const int64_t kk = min(K, C - (int64_t)nnan);   // K'
    const int64_t gr = row0 + r;
    if (kk == 0) {   // workgroup-uniform
        if (tid == 0) {
            const float qnan = __uint_as_float(0x7fc00000u);
            mu[gr] = qnan;
            sigma[gr] = qnan;
            rsig[gr] = qnan;
            count[gr] = 0;
        }
        if (topk_idx != nullptr)
            for (int64_t p = tid; p < K; p += CS_SEL_THREADS) topk_idx[gr * K + p] = -1;
        return;
    }

    // radix select: T = the kk-th smallest key; need = how many keys equal to T are taken; eq = how many there are
    uint32_t prefix = 0u, mask = 0u, k = (uint32_t)kk, eq = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < CS_SEL_WAVES * 256; i += CS_SEL_THREADS) (&hist[0][0])[i] = 0u;
        __syncthreads();
        for (int64_t c0 = 0; c0 < C; c0 += CS_SEL_THREADS) {   // uniform trip count: the ballots below see whole waves
            const int64_t c = c0 + tid;
            uint32_t key = c < C ? key_at(c) : 0u;
            bool act = c < C && (key & mask) == prefix;
            const uint32_t d = (key >> shift) & 255u;
            // wave-aggregated adds for the two most common digits of the wave (in the first rounds most keys of a row share one digit,
            // and 64 lanes adding to one LDS word serialise), plain LDS adds for the rest
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const unsigned long long am = __ballot(act);
                if (am == 0ull) break;
                const int leader = __builtin_ctzll(am);
                const uint32_t ld = __shfl(d, leader, 64);
                const unsigned long long mm = __ballot(act && d == ld);
                if (lane == leader) atomicAdd(&hist[w][ld], (uint32_t)__popcll(mm));
                act = act && d != ld;
            }
            if (act) atomicAdd(&hist[w][d], 1u);
        }
        __syncthreads();
        if (w == 0) {   // one wave: lane l owns the digits 4 l .. 4 l + 3
            uint32_t cnt[4], s4 = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t t = 0u;
#pragma unroll
                for (int v = 0; v < CS_SEL_WAVES; ++v) t += hist[v][4 * lane + q];
                cnt[q] = t;
                s4 += t;
            }
            uint32_t incl = s4;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const uint32_t excl = incl - s4;
            if (excl < k && k <= incl) {   // exactly one lane
                uint32_t run = excl;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (k <= run + cnt[q]) {
                        sh_digit = 4u * lane + q;
                        sh_k = k - run;
                        sh_eq = cnt[q];
                        break;
                    }
                    run += cnt[q];
                }
            }
        }
        __syncthreads();
        prefix |= sh_digit << shift;
        mask |= 255u << shift;
        k = sh_k;
        eq = sh_eq;
    }
    const uint32_t T = prefix;
    // the ties at T: the first `k` of the `eq` keys equal to T in index order are taken; cut = the index of the last one taken
    int64_t cut = C;
    if (k < eq) {
        uint32_t base = 0u;
        if (tid == 0) sh_cut = C;
        for (int64_t c0 = 0; c0 < C; c0 += CS_SEL_THREADS) {
            const int64_t c = c0 + tid;
            const bool isT = c < C && key_at(c) == T;
            const unsigned long long b = __ballot(isT);
            const uint32_t below = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) red_u[w] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t before = base, total = 0u;
#pragma unroll
            for (int q = 0; q < CS_SEL_WAVES; ++q) {
                before += q < w ? red_u[q] : 0u;
                total += red_u[q];
            }
            if (isT && before + below + 1u == k) sh_cut = c;
            base += total;
            if (base >= k) break;   // uniform
        }
        __syncthreads();
        cut = sh_cut;
    }
    auto selected = [&](int64_t c, uint32_t key) { return key < T || (key == T && c <= cut); };

    // mean and population standard deviation in float64
    double s = 0.0;
    for (int64_t c = tid; c < C; c += CS_SEL_THREADS) {
        const uint32_t key = key_at(c);
        if (selected(c, key)) s += (double)score_value(key);
    }
    const double mean = block_sum_d(s) / (double)kk;
    double ss = 0.0;
    for (int64_t c = tid; c < C; c += CS_SEL_THREADS) {
        const uint32_t key = key_at(c);
        if (selected(c, key)) {
            const double dv = (double)score_value(key) - mean;
            ss += dv * dv;
        }
    }
    const double var = block_sum_d(ss) / (double)kk;
    if (tid == 0) {
        const float sg = (float)sqrt(var);
        mu[gr] = (float)mean;
        sigma[gr] = sg;
        rsig[gr] = (float)(1.0 / (double)sg);
        count[gr] = (int32_t)kk;
    }
    if (topk_idx == nullptr) return;

    // the selection in (key, index) order: list the selected indices in index order (ballot prefix), then each one's position is the
    // number of listed entries before it in (key, index) order
    int32_t* lr = list + r * C;
    uint32_t base = 0u;
    for (int64_t c0 = 0; c0 < C; c0 += CS_SEL_THREADS) {
        const int64_t c = c0 + tid;
        const bool sel = c < C && selected(c, key_at(c));
        const unsigned long long b = __ballot(sel);
        const uint32_t below = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) red_u[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = base, total = 0u;
#pragma unroll
        for (int q = 0; q < CS_SEL_WAVES; ++q) {
            before += q < w ? red_u[q] : 0u;
            total += red_u[q];
        }
        if (sel) lr[before + below] = (int32_t)c;
        base += total;
    }
    __syncthreads();   // the list is complete (workgroup-scope: global stores of this workgroup are visible to its waves)
    for (int64_t p = tid; p < kk; p += CS_SEL_THREADS) {
        const int32_t c = lr[p];
        const uint32_t kc = key_at(c);
        int64_t pos = 0;
        for (int64_t q = 0; q < kk; ++q) {   // the list is in index order: entries before p win ties
            const uint32_t kq = key_at(lr[q]);
            pos += (kq < kc) || (kq == kc && q < p);
        }
        topk_idx[gr * K + pos] = c;
    }
    for (int64_t p = kk + tid; p < K; p += CS_SEL_THREADS) topk_idx[gr * K + p] = -1;
}

// rows of one score tile: the tile stays within CS_TILE_FLOATS
int64_t cs_tile_rows(int64_t M, int64_t C) {
    int64_t R = (CS_TILE_FLOATS / C) / ST_T * ST_T;
    if (R < ST_T) R = ST_T;
    return R < M ? R : M;
}

// the selection of `lines` lines of C entries each: the rows of a tile (lines, C) (col_ld == 0) or the columns of a tile (C, col_ld)
void launch_cohort_select(const float* tile, int64_t lines, int64_t C, int64_t K, int64_t row0, int64_t col_ld, float* mu, float* sigma,
                          float* rsig, int32_t* count, int32_t* topk_idx, int32_t* list, hipStream_t st) {
    const dim3 sg((unsigned)lines);
#define VM_CS_SEL(CAP, COL) \
    hipLaunchKernelGGL((cohort_select_kernel<CAP, COL>), sg, dim3(CS_SEL_THREADS), 0, st, tile, C, K, row0, col_ld, mu, sigma, rsig, count, topk_idx, list)
    if (col_ld == 0) {
        if (C <= CS_CAP_SMALL) VM_CS_SEL(CS_CAP_SMALL, false);
        else if (C <= CS_CAP_LARGE) VM_CS_SEL(CS_CAP_LARGE, false);
        else VM_CS_SEL(0, false);
    } else {
        if (C <= CS_CAP_SMALL) VM_CS_SEL(CS_CAP_SMALL, true);
        else if (C <= CS_CAP_LARGE) VM_CS_SEL(CS_CAP_LARGE, true);
        else VM_CS_SEL(0, true);
    }
#undef VM_CS_SEL
}

}  // namespace vm

extern "C" int64_t vm_cohort_stats_workspace_bytes(int64_t M, int64_t C, int E) {
    if (M <= 0 || C <= 0 || E <= 0) return 0;
    const int64_t R = vm::cs_tile_rows(M, C), EP = ((E + 3) / 4) * 4;
    // query and cohort squared norms, the padded weights, the scalar-path copy of a tile's queries, the score tile (+ one row: with
    // topk_idx, half the rows per tile and the other half holds the index lists)
    return M * 4 + 256 + C * 4 + 256 + vm::ST_MAX_E * 4 + 256 + ((R + 7) / 8) * 8 * EP * 4 + 256 + (R + 1) * C * 4 + 256;
}

extern "C" int vm_cohort_topk_stats(const float* q, int64_t M, const float* cohort, int64_t C, int E, int score_kind, const float* weights,
                                    int64_t self_row0, int64_t K, float* mu, float* sigma, float* rsig, int32_t* count, int32_t* topk_idx,
                                    void* ws, void* stream) {
    using namespace vm;
    VM_REQUIRE(q && cohort && mu && sigma && rsig && count && ws, "vm_cohort_topk_stats: null pointer");
    VM_REQUIRE(M > 0 && M < (1LL << 31) && C > 0 && C < (1LL << 31) && E > 0 && E <= ST_MAX_E,
               "vm_cohort_topk_stats: bad sizes (M, C < 2^31, E <= %d)", ST_MAX_E);
    VM_REQUIRE(K >= 1 && K < (1LL << 31), "vm_cohort_topk_stats: K must be in [1, 2^31)");
    VM_REQUIRE((score_kind >= VM_DIST_EUCLIDEAN && score_kind <= VM_SCORE_NEG_EUCLIDEAN) || score_kind == VM_SCORE_PLDA,
               "vm_cohort_topk_stats: unknown score_kind %d", score_kind);
    VM_REQUIRE(plda_width_ok(score_kind, E), "vm_cohort_topk_stats: VM_SCORE_PLDA needs E %% 4 == 0 and E >= 4");
    VM_REQUIRE(score_kind != VM_SCORE_WEIGHTED_L1 || weights, "vm_cohort_topk_stats: weighted_l1 needs weights");
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)cohort) & 15) == 0, "vm_cohort_topk_stats: cohort must be 16-byte aligned when E %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    const int64_t R = cs_tile_rows(M, C);
    const int64_t RT = topk_idx != nullptr ? (R + 1) / 2 : R;   // rows per tile
    float* qsq = (float*)ws;
    float* rsq = (float*)(((uintptr_t)(qsq + M) + 255) & ~(uintptr_t)255);
    float* wpad = (float*)(((uintptr_t)(rsq + C) + 255) & ~(uintptr_t)255);
    float* qT = (float*)(((uintptr_t)(wpad + ST_MAX_E) + 255) & ~(uintptr_t)255);
    const int64_t EP = ((E + 3) / 4) * 4;
    float* tile = (float*)(((uintptr_t)(qT + ((R + 7) / 8) * 8 * EP) + 255) & ~(uintptr_t)255);
    int32_t* list = (int32_t*)(tile + RT * C);   // with topk_idx: RT rows of C indices behind the RT score rows, within (R + 1) * C
    launch_row_scalars(score_kind, q, M, E, qsq, st);
    launch_row_scalars(score_kind, cohort, C, E, rsq, st);
    launch_pad_weights(score_kind == VM_SCORE_WEIGHTED_L1 ? weights : nullptr, E, wpad, st);
    const int splits = score_splits(RT, C, 2048);
    const int tps = (int)(((C + ST_RT - 1) / ST_RT + splits - 1) / splits);
    for (int64_t row0 = 0; row0 < M; row0 += RT) {
        const int64_t rows = RT < M - row0 ? RT : M - row0;
        launch_pairdist_qt(q + row0 * E, rows, E, qT, st, score_kind == VM_SCORE_PLDA ? E - 1 : -1);
        const int64_t self_col0 = self_row0 >= 0 ? self_row0 + row0 : -1;
        const dim3 grid((unsigned)((rows + ST_T - 1) / ST_T), (unsigned)splits);
#define VM_CS(KD) hipLaunchKernelGGL(cohort_score_kernel<KD>, grid, dim3(512), 0, st, qT, cohort, rows, C, E, self_col0, qsq + row0, rsq, wpad, \
                                     tps, tile)
        switch (score_kind) {
            case VM_DIST_EUCLIDEAN: VM_CS(VM_DIST_EUCLIDEAN); break;
            case VM_DIST_COSINE: VM_CS(VM_DIST_COSINE); break;
            case VM_DIST_DOT: VM_CS(VM_DIST_DOT); break;
            case VM_SCORE_WEIGHTED_L1: VM_CS(VM_SCORE_WEIGHTED_L1); break;
            case VM_SCORE_PLDA: VM_CS(VM_SCORE_PLDA); break;
            default: VM_CS(VM_SCORE_NEG_EUCLIDEAN); break;
        }
#undef VM_CS
        launch_cohort_select(tile, rows, C, K, row0, 0, mu, sigma, rsig, count, topk_idx, list, st);
        const int rc = check_launch("vm_cohort_topk_stats");
        if (rc != 0) return rc;
    }
    return 0;
}
