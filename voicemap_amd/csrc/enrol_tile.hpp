// "Rows against speaker models": the ONE tile kernel behind vm_[plda_]speaker_{identify, trial_hist, trial_hist_norm, trial_calib_sums}
// and the three launchers of those eight entry points.  model_tile_kernel<Score, MODE, NORM> holds, once and as plain statements, the
// tile geometry and thread map, the row prologue, the prefetch / stash stage pipeline, the accumulate loop, the model loop and
// everything that happens to a finished fp32 score -- the order of the trials of one query ((uint32 key, speaker), NaN last), rank /
// best; the class histogram with pair_hist_kernel's (verif.hip) window, slot and NaN conventions; the calibration sums with
// pair_calib_kernel's (calib.hip) terms and fixed-order reduction.  What differs between the back ends comes from the score policy
// `Score` (EnScore<KIND>, enrol.hip: the geometric kinds; PeScore, plda_enrol.hip: multi-session PLDA), passed by value:
//   EC, NM                       components per stage and float64 model operands staged through LDS beside the query operand
//   op[NM], width, PADDED[, pitch] the model operands ((S, width) float64) and the components scored; PADDED: q's rows are `pitch`
//                                floats wide, more than `width` and a multiple of 4 (else they are `width` wide and there is no pitch)
//   row_term(m, ok), model_term(s, ok), count_ok(n)   the per-row and per-model scalar of the finish; "is a count of n rows a model"
//   acc(a, q, p[NM]), finish(a, row_term, model_term) the per-component chain and the one rounding to fp32
// The policy's pointers reach the kernel inside a by-value struct, so they carry no __restrict__ as kernel parameters can; they are
// scratch of the call that nothing else writes, and the compiled resources are those of the restrict-qualified kernels it replaces.
// A policy is a template parameter of one body, not a set of functions over the kernel's register arrays: an earlier attempt to share
// the epilogue as functions taking references to before[] / best[] / und[][] compiled to other code (branches where the kernel has
// selects, an unrolled window loop of another shape), which is why the epilogue used to be shared as text macros.  Inside one templated
// body the same statements are the kernel's own; the policy's members are scalars and a two-element array, and vanish on inlining.
#pragma once
#include "calib_terms.hpp"
#include "enrol_score.hpp"
#include "score_tile.hpp"

namespace vm {

// what model_tile_kernel does with a finished score: the matrix / rank / best of identify, the class histogram, the calibration sums
enum class EnMode { IDENTIFY, HIST, CALIB };

constexpr int EN_TQ = 64, EN_TS = 64, EN_LD = 66, EN_MAX_WIN = 4;
constexpr int EN_LDS_HIST_WORDS = 2 * 4 * (1024 + 3);   // = VH_LDS_HIST_WORDS (verif.hip): the same limits on windows and bins
typedef __attribute__((ext_vector_type(2))) double f64x2;

struct EnWindows {
    uint32_t lo[EN_MAX_WIN];
    uint32_t shift[EN_MAX_WIN];
};

static inline char* en_align(void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// The statistics of a NORMALISED trial histogram (S-norm / AS-norm of model trials), all fp32 on the device: per query row of the call
// mu_q / rsig_q and, under leave-one-out, mu_own / rsig_own (the row's own speaker WITHOUT the row); per model mu_s / rsig_s.  The plain
// kernels (NORM = false) never read it.
struct EnNorm {
    const float *mu_q, *rsig_q, *mu_s, *rsig_s, *mu_own, *rsig_own;
};

// The calibration mode's arguments: llr = a s + b at the offset tau (cal_terms, calib_terms.hpp) and the workgroups' partial sums
// part (CAL_SUMS, gridDim.x * gridDim.y) float64, workgroup (x, y) owning column y * gridDim.x + x.  The other modes never read it.
struct EnCalib {
    double a, b, tau;
    double* part;
};

// grid (query tiles of 64 rows, splits of the model tiles (HIST and CALIB)); 256 threads: ts = tid & 15 owns the models
// {2 ts, 2 ts + 1, 32 + 2 ts, 33 + 2 ts} of a tile, tq = tid >> 4 the queries 4 tq .. 4 tq + 3, in 4 x 4 float64 accumulators.  `own`: the
// score of every row against its OWN speaker (under leave-one-out that model differs from the shared one: the cell takes this score
// rather than a patched one).  IDENTIFY: the score matrix (NaN where the cell is no trial) and, per row, the count of speakers before
// the own one and the best (key, speaker) -- integer sums and minima kept in registers over all model tiles and merged over the 16 lanes
// of a row at the end.  HIST: every trial is counted once per window -- under / over in the lane's registers, a bin in the
// workgroup's u32 LDS histogram -- or, a NaN, once in the lane's NaN count; one flush of 64-bit integer atomics per workgroup.  CALIB:
// every trial adds its six cal_terms to the lane's float64 accumulators of its class (u32 counts; a NaN or infinite score is counted
// as skipped and adds nothing else), carried over the workgroup's model tiles in ascending tile order; then the shuffle tree per wave,
// the four waves in order through LDS, and the workgroup's column of cal.part -- zeros where its split holds no tile; no LDS
// histogram, no atomics.  NORM (HIST and CALIB): the finished score becomes vh_norm's (score_tile.hpp) s' = 0.5f ((d - mu_q) rsig_q +
// (d - mu_M) rsig_M) before it is binned or summed, (mu_M, rsig_M) the own pair under leave-one-out in the own-speaker cell, the
// model's everywhere else.
template <class Score, EnMode MODE, bool NORM>
__global__ __launch_bounds__(256) void model_tile_kernel(Score sc, const float* __restrict__ q, const int32_t* __restrict__ q_label, int64_t M,
                                                         const int32_t* __restrict__ count, int64_t S, int loo,
                                                         const float* __restrict__ own, float* __restrict__ scores,
                                                         float* __restrict__ true_score, int32_t* __restrict__ rank,
                                                         float* __restrict__ best_val, int32_t* __restrict__ best_idx, EnWindows win,
                                                         int n_win, int bins, int splits, unsigned long long* __restrict__ ghist,
                                                         EnNorm nrm, EnCalib cal) {
    constexpr bool HIST = MODE == EnMode::HIST, CALIB = MODE == EnMode::CALIB;
    constexpr int EC = Score::EC, NM = Score::NM;
    constexpr int QP = EC / 16, MP = EC / 8;   // per thread and stage: pieces of 4 floats of q, pieces of 2 doubles of each model operand
    __shared__ __attribute__((aligned(16))) double qs[EC * EN_LD];
    __shared__ __attribute__((aligned(16))) double ps[NM][EC * EN_LD];
    __shared__ uint32_t hist[HIST ? EN_LDS_HIST_WORDS : 1];
    const int tid = threadIdx.x, lane = tid & 63, ts = tid & 15, tq = tid >> 4;
    const int slots = bins + 3;
    const int n_words = n_win * 2 * slots;
    const int64_t mb = (int64_t)blockIdx.x * EN_TQ;
    const int n_tiles = (int)((S + EN_TS - 1) / EN_TS);
    const int tps = (n_tiles + splits - 1) / splits;
    const int t_lo = blockIdx.y * tps;
    const int t_hi = min(n_tiles, t_lo + tps);
    if (t_lo >= t_hi) {   // workgroup-uniform
        if constexpr (CALIB) {
            if (tid < CAL_SUMS) cal.part[(int64_t)tid * gridDim.x * gridDim.y + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = 0.0;
        }
        return;
    }
    if (HIST) {
        for (int i = tid; i < n_words; i += 256) hist[i] = 0u;
    }

    // the thread's four query rows: own speaker ql (-1: none), whether that trial exists, its score and key; the NORM statistics
    const float nanf_ = __uint_as_float(0x7fc00000u);
    int32_t ql[4];
    bool okm[4], own_ok[4];
    double rterm[4];
    float ownv[4];
    uint32_t okey[4];
    float n_mq[4], n_rq[4], n_mo[4], n_ro[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = mb + tq * 4 + i;
        okm[i] = m < M;
        int32_t l = okm[i] ? q_label[m] : -1;
        if (l < 0 || l >= S) l = -1;
        ql[i] = l;
        own_ok[i] = l >= 0 && sc.count_ok(count[l] - (loo ? 1 : 0));
        rterm[i] = sc.row_term(m, okm[i]);
        ownv[i] = okm[i] ? own[m] : nanf_;
        okey[i] = score_key_nan_last(ownv[i]);
        n_mq[i] = (NORM && okm[i]) ? nrm.mu_q[m] : 0.f;
        n_rq[i] = (NORM && okm[i]) ? nrm.rsig_q[m] : 0.f;
        n_mo[i] = (NORM && loo && okm[i]) ? nrm.mu_own[m] : 0.f;
        n_ro[i] = (NORM && loo && okm[i]) ? nrm.rsig_own[m] : 0.f;
    }
    // per row: the number of speakers before the own one, the best (key, speaker) and its score; per window and class the under / over
    // counts, per class the NaN count
    uint32_t before[4] = {0u, 0u, 0u, 0u};
    unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    float bestf[4] = {nanf_, nanf_, nanf_, nanf_};
    uint32_t und[EN_MAX_WIN][2], ovr[EN_MAX_WIN][2], nanc[2] = {0u, 0u};
#pragma unroll
    for (int v = 0; v < EN_MAX_WIN; ++v) und[v][0] = und[v][1] = ovr[v][0] = ovr[v][1] = 0u;
    // CALIB: per class the six sums of cal_terms, the trials summed and the trials skipped (at most 16 per lane and tile: no overflow)
    double csum[2][6];
    uint32_t ccnt[2] = {0u, 0u}, cskp[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) csum[c][k] = 0.0;

    const int W = sc.width;
    int pitch = W;
    if constexpr (Score::PADDED) pitch = sc.pitch;
    const int nchunk = (W + EC - 1) / EC;
    const int n_stage = (t_hi - t_lo) * nchunk;   // workgroup-uniform: every barrier below is reached by all 256 threads
    const bool vec = Score::PADDED || (pitch & 3) == 0;
    // a stage = 64 query rows x EC components (fp32, QP pieces of 4 per thread) and, per model operand, 64 models x EC components (fp64,
    // MP pieces of 2).  Components >= W read as zero; with vec, c % 4 == 0 and c < W <= pitch, pitch % 4 == 0: the 4 floats lie in the row
    // (and, unless PADDED, inside W).
    auto fetch = [&](int st, f32x4 (&vq)[QP], f64x2 (&vp)[NM][MP]) {
        const int ec = (st % nchunk) * EC;
        const int64_t s0 = (int64_t)(t_lo + st / nchunk) * EN_TS;
#pragma unroll
        for (int k = 0; k < QP; ++k) {
            const int piece = tid + 256 * k, r = piece / (EC / 4), c = ec + (piece % (EC / 4)) * 4;
            const int64_t row = mb + r;
            if (vec) {
                const bool ok = row < M && c < W;
                const f32x4 x = *reinterpret_cast<const f32x4*>(q + (ok ? row * pitch + c : 0));
#pragma unroll
                for (int u = 0; u < 4; ++u) vq[k][u] = (ok && (!Score::PADDED || c + u < W)) ? x[u] : 0.f;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) vq[k][u] = (row < M && c + u < W) ? q[row * pitch + c + u] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < MP; ++k) {
            const int piece = tid + 256 * k, r = piece / (EC / 2), c = ec + (piece % (EC / 2)) * 2;
            const int64_t row = s0 + r;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bool ok = row < S && c + u < W;
                if constexpr (NM == 1) {
                    vp[0][k][u] = ok ? sc.op[0][row * W + c + u] : 0.0;
                } else {
                    // One guarded load (a branch) per operand made the compiler copy the whole staging tuple around each: 22 more VGPRs
                    // and a wave fewer per SIMD in the identify form.  So: unconditional loads from element 0 where the piece lies
                    // outside (S, W >= 1), masked afterwards.  With one operand the guarded form stays: it is the code the geometric
                    // kernels had, and the unconditional one timed 0.5 - 1 % slower there (profiles/model_tile_refactor.txt, section 3).
                    const int64_t at = ok ? row * W + c + u : 0;
#pragma unroll
                    for (int o = 0; o < NM; ++o) {
                        const double x = sc.op[o][at];
                        vp[o][k][u] = ok ? x : 0.0;
                    }
                }
            }
        }
    };
    auto stash = [&](const f32x4 (&vq)[QP], const f64x2 (&vp)[NM][MP]) {
#pragma unroll
        for (int k = 0; k < QP; ++k) {
            const int piece = tid + 256 * k, r = piece / (EC / 4), c = (piece % (EC / 4)) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) qs[(c + u) * EN_LD + r] = (double)vq[k][u];
        }
#pragma unroll
        for (int k = 0; k < MP; ++k) {
            const int piece = tid + 256 * k, r = piece / (EC / 2), c = (piece % (EC / 2)) * 2;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int o = 0; o < NM; ++o) ps[o][(c + u) * EN_LD + r] = vp[o][k][u];
        }
    };
    f32x4 nq[QP];
    f64x2 np[NM][MP];
    fetch(0, nq, np);
    double acc[4][4];
    for (int st = 0; st < n_stage; ++st) {
        const int t = t_lo + st / nchunk, ck = st % nchunk;
        const int ew = min(EC, W - ck * EC);
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
            const double qv[4] = {qa[0], qa[1], qb[0], qb[1]};
            double pv[4][NM];
#pragma unroll
            for (int o = 0; o < NM; ++o) {
                const f64x2 pa = *reinterpret_cast<const f64x2*>(ps[o] + e * EN_LD + ts * 2);
                const f64x2 pb = *reinterpret_cast<const f64x2*>(ps[o] + e * EN_LD + 32 + ts * 2);
                pv[0][o] = pa[0], pv[1][o] = pa[1], pv[2][o] = pb[0], pv[3][o] = pb[1];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Score::acc(acc[i][j], qv[i], pv[j]);
        }
        if (ck != nchunk - 1) continue;
        // the tile's scores are complete: each of the thread's 4 models against each of its 4 rows
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t s = (int64_t)t * EN_TS + (j >> 1) * 32 + ts * 2 + (j & 1);
            const bool oks = s < S;
            const double mterm = sc.model_term(s, oks);
            const bool has_model = oks && sc.count_ok(count[s]);
            const float n_ms = (NORM && oks) ? nrm.mu_s[s] : 0.f;
            const float n_rs = (NORM && oks) ? nrm.rsig_s[s] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t m = mb + tq * 4 + i;
                const bool is_own = oks && (int64_t)ql[i] == s;
                const bool trial = okm[i] && (is_own ? own_ok[i] : has_model);
                float d = Score::finish(acc[i][j], rterm[i], mterm);
                if (is_own) d = ownv[i];
                if constexpr (NORM) {
                    const bool o_ = loo && is_own;
                    d = vh_norm(d, n_mq[i], n_rq[i], o_ ? n_mo[i] : n_ms, o_ ? n_ro[i] : n_rs);
                }
                if constexpr (CALIB) {
                    // pair_calib_kernel's masked form: the terms of 0.0 where the cell adds nothing, selected away
                    const bool fin = (__float_as_uint(d) & 0x7f800000u) != 0x7f800000u;   // neither NaN nor infinite
                    const bool use = trial && fin;
                    ccnt[0] += use && is_own;
                    ccnt[1] += use && !is_own;
                    cskp[0] += trial && !fin && is_own;
                    cskp[1] += trial && !fin && !is_own;
                    double x[6];
                    cal_terms(use ? (double)d : 0.0, is_own, cal.a, cal.b, cal.tau, x);
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        csum[0][k] += (use && is_own) ? x[k] : 0.0;
                        csum[1][k] += (use && !is_own) ? x[k] : 0.0;
                    }
                } else if (!HIST) {
                    if (scores != nullptr && okm[i] && oks) scores[m * S + s] = trial ? d : nanf_;
                    if (trial) {
                        const uint32_t k = score_key_nan_last(d);
                        const unsigned long long cand = ((unsigned long long)k << 32) | (uint32_t)s;
                        if (cand < best[i]) {
                            best[i] = cand;
                            bestf[i] = d;
                        }
                        if (!is_own && (k < okey[i] || (k == okey[i] && s < (int64_t)ql[i]))) before[i] += 1u;
                    }
                } else if (trial) {
                    const int cls = is_own ? 0 : 1;
                    if (d != d) {
                        nanc[cls] += 1u;
                        continue;
                    }
                    const uint32_t k = score_key_nan_last(d);
#pragma unroll
                    for (int v = 0; v < EN_MAX_WIN; ++v) {
                        if (v >= n_win) break;
                        const bool under = k < win.lo[v];
                        const uint32_t b = (k - win.lo[v]) >> win.shift[v];
                        const bool over = !under && b >= (uint32_t)bins;
                        und[v][cls] += under;
                        ovr[v][cls] += over;
                        if (!under && !over) atomicAdd(&hist[(v * 2 + cls) * slots + b], 1u);
                    }
                }
            }
        }
    }

    // The end of a workgroup, reached by all of its threads (the histogram flush and the calibration reduction hold a barrier).
    auto wave_sum_u = [](uint32_t x) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        return x;
    };
    if constexpr (CALIB) {
        // the wave's sums (a fixed shuffle tree; the counts are integers), the four waves in order, the workgroup's column of part
        __shared__ double red[4][CAL_SUMS];
        const int w = tid >> 6;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t n = wave_sum_u(ccnt[c]), ns = wave_sum_u(cskp[c]);
            if (lane == 0) {
                red[w][c * CAL_TERMS + 0] = (double)n;
                red[w][c * CAL_TERMS + 1] = (double)ns;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double v = wave_sum_d(csum[c][k]);
                if (lane == 0) red[w][c * CAL_TERMS + 2 + k] = v;
            }
        }
        __syncthreads();
        if (tid < CAL_SUMS) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += red[k][tid];
            cal.part[(int64_t)tid * gridDim.x * gridDim.y + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
        }
        return;
    }
    if (!HIST) {
        // merge over the 16 lanes of a query row -- integer sums and minima, any order gives the same result -- and lane ts == 0 writes
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                before[i] += __shfl_xor(before[i], o, 64);
                const unsigned long long ob = __shfl_xor(best[i], o, 64);
                const float of = __shfl_xor(bestf[i], o, 64);
                if (ob < best[i]) {
                    best[i] = ob;
                    bestf[i] = of;
                }
            }
            const int64_t m = mb + tq * 4 + i;
            if (ts == 0 && okm[i]) {
                rank[m] = own_ok[i] ? (int32_t)before[i] : -1;
                true_score[m] = own_ok[i] ? ownv[i] : nanf_;
                best_idx[m] = best[i] == ~0ull ? -1 : (int32_t)(uint32_t)best[i];
                best_val[m] = bestf[i];
            }
        }
        return;
    }
    // the lanes' under / over / NaN counts join the LDS histogram, which is flushed once with 64-bit integer atomics into ghist
    const uint32_t nan0 = wave_sum_u(nanc[0]), nan1 = wave_sum_u(nanc[1]);
#pragma unroll
    for (int v = 0; v < EN_MAX_WIN; ++v) {
        if (v >= n_win) break;
        const uint32_t c[6] = {wave_sum_u(und[v][0]), wave_sum_u(ovr[v][0]), nan0, wave_sum_u(und[v][1]), wave_sum_u(ovr[v][1]), nan1};
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (c[k] != 0u) atomicAdd(&hist[(v * 2 + k / 3) * slots + bins + k % 3], c[k]);
        }
    }
    __syncthreads();
    for (int i = tid; i < n_words; i += 256) {
        const uint32_t c = hist[i];
        if (c != 0u) __hip_atomic_fetch_add(&ghist[i], (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the launchers' side --------------------------------------------------------------------------------------------------------------
// the (key_lo, shift) pairs of a trial-histogram call, checked and packed
static inline int en_windows(const char* what, const int64_t* host_windows, int n_windows, int bins, const void* hist, EnWindows* win) {
    VM_REQUIRE(host_windows && hist, "%s: null pointer", what);
    VM_REQUIRE(n_windows >= 1 && n_windows <= EN_MAX_WIN && bins >= 1, "%s: 1..%d windows, bins >= 1", what, EN_MAX_WIN);
    VM_REQUIRE((int64_t)n_windows * 2 * (bins + 3) <= EN_LDS_HIST_WORDS, "%s: %d windows x %d bins exceed %d LDS words", what, n_windows, bins,
               EN_LDS_HIST_WORDS);
    for (int v = 0; v < n_windows; ++v) {
        const int64_t lo = host_windows[2 * v], sh = host_windows[2 * v + 1];
        VM_REQUIRE(lo >= 0 && lo <= 0xffffffffLL && sh >= 0 && sh <= 31, "%s: window %d: key_lo in [0, 2^32), shift in [0, 31]", what, v);
        win->lo[v] = (uint32_t)lo;
        win->shift[v] = (uint32_t)sh;
    }
    return 0;
}

// model tiles split over blockIdx.y: a workgroup counts at most 64 x 64 x tiles trials in its u32 LDS bins (2^19 tiles), and a small
// M still fills the chip
static inline int64_t en_hist_splits(int64_t M, int64_t S) {
    const int64_t qb = cdiv(M, EN_TQ), nt = cdiv(S, EN_TS);
    int64_t splits = cdiv(2048, qb);
    const int64_t s_min = cdiv(nt, (1 << 19));
    if (splits < s_min) splits = s_min;
    if (splits > nt) splits = nt;
    if (splits < 1) splits = 1;
    return splits;
}

// the statistics of a _norm entry point, checked
static inline int en_check_norm(const char* what, const EnNorm& n, int leave_one_out) {
    VM_REQUIRE(n.mu_q && n.rsig_q && n.mu_s && n.rsig_s, "%s: null pointer", what);
    VM_REQUIRE((n.mu_own == nullptr) == (n.rsig_own == nullptr), "%s: mu_own and rsig_own go together", what);
    VM_REQUIRE(leave_one_out != 0 || n.mu_own == nullptr, "%s: mu_own / rsig_own must be NULL without leave_one_out", what);
    VM_REQUIRE(leave_one_out == 0 || n.mu_own != nullptr, "%s: leave_one_out needs mu_own / rsig_own", what);
    return 0;
}

// The three launchers.  `Call` is a back end's arguments (EnCall, enrol.hip; PeCall, plda_enrol.hip): q, q_label, M, count, S, loo, and
//   check(what, ws)        its argument checks
//   stage(ws, st, launch)  its scratch layout in ws and its prepare launches, then launch(score policy, own-speaker scores) once
// Each runs checks -> windows -> scratch -> prepare -> grid / splits -> kernel (-> the final sum of the calibration partials).
struct EnOutputs {
    float *scores, *true_score;
    int32_t* rank;
    float* best_val;
    int32_t* best_idx;
};

template <class Call>
static int model_identify(const char* what, const Call& a, const EnOutputs& o, void* ws, void* stream) {
    if (int rc = a.check(what, ws)) return rc;
    VM_REQUIRE(o.true_score && o.rank && o.best_val && o.best_idx, "%s: null pointer", what);
    if (a.M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(a.M, EN_TQ), 1);
    a.stage(ws, st, [&](auto sc, const float* own) {
        hipLaunchKernelGGL((model_tile_kernel<decltype(sc), EnMode::IDENTIFY, false>), grid, dim3(256), 0, st, sc, a.q, a.q_label, a.M, a.count,
                           a.S, a.loo, own, o.scores, o.true_score, o.rank, o.best_val, o.best_idx, EnWindows{}, 0, 0, 1,
                           (unsigned long long*)nullptr, EnNorm{}, EnCalib{});
    });
    return check_launch(what);
}

// norm == NULL: the plain histogram; else the NORM instantiation with its statistics
template <class Call>
static int model_trial_hist(const char* what, const Call& a, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist,
                            const EnNorm* norm, void* ws, void* stream) {
    if (norm != nullptr) {
        if (int rc = en_check_norm(what, *norm, a.loo)) return rc;
    }
    if (int rc = a.check(what, ws)) return rc;
    EnWindows win{};
    if (int rc = en_windows(what, host_windows, n_windows, bins, hist, &win)) return rc;
    if (a.M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int splits = (int)en_hist_splits(a.M, a.S);
    const dim3 grid((unsigned)cdiv(a.M, EN_TQ), (unsigned)splits);
    a.stage(ws, st, [&](auto sc, const float* own) {
        auto launch = [&](auto kernel, const EnNorm& n) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, sc, a.q, a.q_label, a.M, a.count, a.S, a.loo, own, (float*)nullptr,
                               (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, win, n_windows, bins, splits,
                               (unsigned long long*)hist, n, EnCalib{});
        };
        if (norm == nullptr) launch(model_tile_kernel<decltype(sc), EnMode::HIST, false>, EnNorm{});
        else launch(model_tile_kernel<decltype(sc), EnMode::HIST, true>, *norm);
    });
    return check_launch(what);
}

// The calibration sums' partials: the histogram's grid, one column of CAL_SUMS doubles per workgroup, in front of the call's scratch
static inline int64_t en_calib_parts(int64_t M, int64_t S) { return M > 0 && S > 0 ? cdiv(M, EN_TQ) * en_hist_splits(M, S) : 0; }
static inline int64_t en_calib_part_bytes(int64_t M, int64_t S) { return en_calib_parts(M, S) * CAL_SUMS * 8 + 256; }

// calib (2, CAL_TERMS) float64 is WRITTEN: the kernel's partials, then calib_final_kernel over them (M == 0: zeros).  The six
// statistics are NULL all together (raw scores: the plain instantiation) or follow en_check_norm.
template <class Call>
static int model_trial_calib(const char* what, const Call& a, const EnNorm& norm, double ca, double cb, double tau, double* calib, void* ws,
                             void* stream) {
    const bool normed = norm.mu_q || norm.rsig_q || norm.mu_s || norm.rsig_s || norm.mu_own || norm.rsig_own;
    if (normed) {
        if (int rc = en_check_norm(what, norm, a.loo)) return rc;
    }
    if (int rc = a.check(what, ws)) return rc;
    VM_REQUIRE(calib != nullptr, "%s: null pointer", what);
    VM_REQUIRE((((uintptr_t)calib) & 7) == 0, "%s: calib must be 8-byte aligned", what);
    VM_REQUIRE(ca - ca == 0.0 && cb - cb == 0.0 && tau - tau == 0.0, "%s: a, b and tau must be finite", what);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)en_align(ws);
    const int64_t n_part = en_calib_parts(a.M, a.S);
    if (a.M > 0) {
        const int splits = (int)en_hist_splits(a.M, a.S);
        const dim3 grid((unsigned)cdiv(a.M, EN_TQ), (unsigned)splits);
        a.stage(part + n_part * CAL_SUMS, st, [&](auto sc, const float* own) {
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, sc, a.q, a.q_label, a.M, a.count, a.S, a.loo, own, (float*)nullptr,
                                   (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, EnWindows{}, 0, 0, splits,
                                   (unsigned long long*)nullptr, norm, EnCalib{ca, cb, tau, part});
            };
            if (!normed) launch(model_tile_kernel<decltype(sc), EnMode::CALIB, false>);
            else launch(model_tile_kernel<decltype(sc), EnMode::CALIB, true>);
        });
    }
    hipLaunchKernelGGL(calib_final_kernel, dim3(1), dim3(64 * CAL_SUMS), 0, st, (const double*)part, n_part, calib);
    return check_launch(what);
}

}  // namespace vm
