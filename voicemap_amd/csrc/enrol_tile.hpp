// What the two "rows against speaker models" tile kernels share (enrol.hip en_tile_kernel: the geometric kinds; plda_enrol.hip
// pe_tile_kernel: multi-session PLDA): the tile geometry, the histogram windows, and everything that happens to a finished fp32 score --
// the order of the trials of one query ((uint32 key, speaker), NaN last), rank / best, the class histogram with pair_hist_kernel's
// (verif.hip) window, slot and NaN conventions -- and the launchers' window parsing and model-tile splits.  One statement of each, so
// the entry points of both files order and bin alike.
//
// The device side is shared as TEXT (macros), not as functions: en_tile_kernel's epilogue was written on the kernel's own register
// arrays, and the same statements behind references compile to other code (branches where the kernel has selects, an unrolled window
// loop of another shape; seen when plda_enrol.hip was added).  A macro leaves every instantiation of en_tile_kernel the instruction
// stream it had.  The macros use the names both kernels give their state; each lists the names it reads.
#pragma once
#include "enrol_score.hpp"
#include "score_tile.hpp"

namespace vm {

constexpr int EN_TQ = 64, EN_TS = 64, EN_EC = 32, EN_LD = 66, EN_MAX_WIN = 4;
constexpr int EN_LDS_HIST_WORDS = 2 * 4 * (1024 + 3);   // = VH_LDS_HIST_WORDS (verif.hip): the same limits on windows and bins
typedef __attribute__((ext_vector_type(2))) double f64x2;

struct EnWindows {
    uint32_t lo[EN_MAX_WIN];
    uint32_t shift[EN_MAX_WIN];
};

static inline char* en_align(void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// The statistics of a NORMALISED trial histogram (enrol_norm.hip: S-norm / AS-norm of model trials), all fp32 on the device: per query
// row of the call mu_q / rsig_q and, under leave-one-out, mu_own / rsig_own (the row's own speaker WITHOUT the row); per model mu_s /
// rsig_s.  The plain kernels (NORM = false) never read it.
struct EnNorm {
    const float *mu_q, *rsig_q, *mu_s, *rsig_s, *mu_own, *rsig_own;
};

// NORM only, shared as text like the epilogue below.  EN_NORM_ROWS: the statistics of the thread's four query rows (reads mb, tq, okm,
// loo, nrm).  EN_NORM_MODEL: those of model s, inside the loop over the thread's models (reads oks, s).  EN_NORM_CELL(d): the finished
// score d of a cell becomes vh_norm's (score_tile.hpp) s' = 0.5f ((d - mu_q) rsig_q + (d - mu_M) rsig_M), every operation rounded on its
// own; (mu_M, rsig_M) is the own pair under leave-one-out in the own-speaker cell, the model's everywhere else.
#define EN_NORM_ROWS                                                     \
    float n_mq[4], n_rq[4], n_mo[4], n_ro[4];                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                      \
        const int64_t m = mb + tq * 4 + i;                               \
        n_mq[i] = (NORM && okm[i]) ? nrm.mu_q[m] : 0.f;                  \
        n_rq[i] = (NORM && okm[i]) ? nrm.rsig_q[m] : 0.f;                \
        n_mo[i] = (NORM && loo && okm[i]) ? nrm.mu_own[m] : 0.f;         \
        n_ro[i] = (NORM && loo && okm[i]) ? nrm.rsig_own[m] : 0.f;       \
    }
#define EN_NORM_MODEL                                      \
    const float n_ms = (NORM && oks) ? nrm.mu_s[s] : 0.f;  \
    const float n_rs = (NORM && oks) ? nrm.rsig_s[s] : 0.f
#define EN_NORM_CELL(d)                                                                        \
    if constexpr (NORM) {                                                                      \
        const bool o_ = loo && is_own;                                                         \
        d = vh_norm(d, n_mq[i], n_rq[i], o_ ? n_mo[i] : n_ms, o_ ? n_ro[i] : n_rs);            \
    }

// The per-thread state of a tile kernel's epilogue: per query row i of the thread's four, the number of speakers before the own one
// and the best (key, speaker) with its score; per window and class the under / over counts, per class the NaN count.  Reads nanf_.
#define EN_TILE_STATE                                                                        \
    uint32_t before[4] = {0u, 0u, 0u, 0u};                                                   \
    unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};                               \
    float bestf[4] = {nanf_, nanf_, nanf_, nanf_};                                           \
    uint32_t und[EN_MAX_WIN][2], ovr[EN_MAX_WIN][2], nanc[2] = {0u, 0u};                     \
    _Pragma("unroll") for (int v = 0; v < EN_MAX_WIN; ++v) und[v][0] = und[v][1] = ovr[v][0] = ovr[v][1] = 0u

// One finished score d of a cell, INSIDE the loop over the thread's query rows i (a NaN trial `continue`s it).  The cell: query row i
// (global row m, valid okm[i], own speaker ql[i] whose score has key okey[i]) against model s (valid oks); `trial` and `is_own` say
// what it is.  HIST false: the score matrix (NaN where the cell is no trial), the row's best (key, speaker) and the count of speakers
// before the own one.  HIST true: the trial is counted once per window -- under / over in the lane's registers, a bin in the
// workgroup's u32 LDS histogram `hist` -- or, a NaN, once in the lane's NaN count.  Reads scores, S, win, n_win, bins, slots too.
#define EN_TILE_CELL(d)                                                                                                  \
    if (!HIST) {                                                                                                         \
        if (scores != nullptr && okm[i] && oks) scores[m * S + s] = trial ? d : nanf_;                                   \
        if (trial) {                                                                                                     \
            const uint32_t k = score_key_nan_last(d);                                                                    \
            const unsigned long long cand = ((unsigned long long)k << 32) | (uint32_t)s;                                 \
            if (cand < best[i]) {                                                                                        \
                best[i] = cand;                                                                                          \
                bestf[i] = d;                                                                                            \
            }                                                                                                            \
            if (!is_own && (k < okey[i] || (k == okey[i] && s < (int64_t)ql[i]))) before[i] += 1u;                       \
        }                                                                                                                \
    } else if (trial) {                                                                                                  \
        const int cls = is_own ? 0 : 1;                                                                                  \
        if (d != d) {                                                                                                    \
            nanc[cls] += 1u;                                                                                             \
            continue;                                                                                                    \
        }                                                                                                                \
        const uint32_t k = score_key_nan_last(d);                                                                        \
        _Pragma("unroll") for (int v = 0; v < EN_MAX_WIN; ++v) {                                                         \
            if (v >= n_win) break;                                                                                       \
            const bool under = k < win.lo[v];                                                                            \
            const uint32_t b = (k - win.lo[v]) >> win.shift[v];                                                          \
            const bool over = !under && b >= (uint32_t)bins;                                                             \
            und[v][cls] += under;                                                                                        \
            ovr[v][cls] += over;                                                                                         \
            if (!under && !over) atomicAdd(&hist[(v * 2 + cls) * slots + b], 1u);                                        \
        }                                                                                                                \
    }

// The end of a workgroup, reached by all of its threads (the histogram flush holds a barrier).  HIST false: merge over the 16 lanes of
// a query row -- integer sums and minima, any order gives the same result -- and lane ts == 0 writes rank / true_score / best_*; the
// kernel RETURNS.  HIST true: the lanes' under / over / NaN counts join the LDS histogram, which is flushed once with 64-bit integer
// atomics into ghist.  Reads mb, tq, ts, lane, tid, okm, own_ok, ownv, n_win, bins, slots, n_words.
#define EN_TILE_FINISH                                                                                                               \
    if (!HIST) {                                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                              \
            _Pragma("unroll") for (int o = 1; o < 16; o <<= 1) {                                                                     \
                before[i] += __shfl_xor(before[i], o, 64);                                                                           \
                const unsigned long long ob = __shfl_xor(best[i], o, 64);                                                            \
                const float of = __shfl_xor(bestf[i], o, 64);                                                                        \
                if (ob < best[i]) {                                                                                                  \
                    best[i] = ob;                                                                                                    \
                    bestf[i] = of;                                                                                                   \
                }                                                                                                                    \
            }                                                                                                                        \
            const int64_t m = mb + tq * 4 + i;                                                                                       \
            if (ts == 0 && okm[i]) {                                                                                                 \
                rank[m] = own_ok[i] ? (int32_t)before[i] : -1;                                                                       \
                true_score[m] = own_ok[i] ? ownv[i] : nanf_;                                                                         \
                best_idx[m] = best[i] == ~0ull ? -1 : (int32_t)(uint32_t)best[i];                                                    \
                best_val[m] = bestf[i];                                                                                              \
            }                                                                                                                        \
        }                                                                                                                            \
        return;                                                                                                                      \
    }                                                                                                                                \
    auto wave_sum_u = [](uint32_t x) {                                                                                               \
        _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);                                                \
        return x;                                                                                                                    \
    };                                                                                                                               \
    const uint32_t nan0 = wave_sum_u(nanc[0]), nan1 = wave_sum_u(nanc[1]);                                                           \
    _Pragma("unroll") for (int v = 0; v < EN_MAX_WIN; ++v) {                                                                         \
        if (v >= n_win) break;                                                                                                       \
        const uint32_t c[6] = {wave_sum_u(und[v][0]), wave_sum_u(ovr[v][0]), nan0, wave_sum_u(und[v][1]), wave_sum_u(ovr[v][1]), nan1}; \
        if (lane == 0) {                                                                                                             \
            _Pragma("unroll") for (int k = 0; k < 6; ++k)                                                                            \
                if (c[k] != 0u) atomicAdd(&hist[(v * 2 + k / 3) * slots + bins + k % 3], c[k]);                                      \
        }                                                                                                                            \
    }                                                                                                                                \
    __syncthreads();                                                                                                                 \
    for (int i = tid; i < n_words; i += 256) {                                                                                       \
        const uint32_t c = hist[i];                                                                                                  \
        if (c != 0u) __hip_atomic_fetch_add(&ghist[i], (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);           \
    }

// ---- the launchers' side --------------------------------------------------------------------------------------------------------------
// The whole of a trial-histogram call -- argument checks, windows, the staging launches, the tile kernel -- for the geometric kinds
// (enrol.hip) and multi-session PLDA (plda_enrol.hip); norm == NULL: the plain histogram.  vm_[plda_]speaker_trial_hist and their
// _norm forms (enrol_norm.hip) are these two calls.
int en_trial_hist(const char* what, const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                  const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows, int n_windows, int bins,
                  uint64_t* hist, const EnNorm* norm, void* ws, void* stream);
int pe_trial_hist(const char* what, const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                  const int32_t* count, int64_t S, const double* A, const double* beta, const double* C, const double* G, int n_max,
                  int leave_one_out, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist, const EnNorm* norm, void* ws,
                  void* stream);

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

}  // namespace vm
