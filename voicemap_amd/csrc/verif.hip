// All-pairs speaker verification (the reference's experiments/verification_accuracy.py is a stub; SURVEY.md:78 "unimplemented"):
// every unordered pair {i, j}, i < j, of a cached (N, E) embedding matrix is scored and the score is BINNED ON THE CHIP -- per class
// (target = same speaker code, non-target otherwise) -- so the N x N matrix never exists (train-clean-360: 5.4e9 pairs, 43 GB of fp32).
// voicemap_amd/verification.py turns the histograms into EER / ROC / threshold metrics, zooming into bins until they are exact.
//
// Binning is on the order-preserving uint32 key of the fp32 score (-0.0 first canonicalised to +0.0; key = bits | 2^31 for a
// non-negative value, ~bits for a negative one), so every count is an integer comparison that numpy reproduces bit for bit.  A window
// (key_lo, shift) puts key k in bin (k - key_lo) >> shift when k >= key_lo and that is < bins; three extra slots per window and class
// count keys below key_lo (under), the rest (over) and NaN scores.
//
// The tile loop is score_tile_loop's (score_tile.hpp), kept here as a copy (see pair_hist_kernel): every score is bit-identical to
// dist[i][j] of vm_pairdist_argmin.  Only reference tiles that hold some j > i are visited and the pairs j <= i are masked.  Counts go
// into per-workgroup u32 LDS histograms (ds_add_u32: integer adds, order-independent) and each workgroup flushes its non-zero bins once
// with 64-bit agent-scope atomic adds into the u64 global counts: results are bit-identical from run to run.
//
// vm_pair_score_hist_norm (NORM): the same pass on cohort-normalised scores (cohort.hip computes the per-row statistics): the pair
// {i, j} is binned on 0.5 (a rsig[i] + b rsig[j]), a = s - mu[i], b = s - mu[j], each operation rounded on its own (no fma contraction,
// so numpy's fp32 reproduces it).  The query side's mu / rsig are wave-uniform registers, the reference side's are read beside its labels.
#include "score_tile.hpp"

namespace vm {

constexpr int VH_MAX_WIN = 4;
// LDS histogram words per workgroup: 4 windows x 1024 bins or 1 x 4096, two classes, three extra slots.  With the 34 KiB reference
// stage that is 67 KiB per workgroup: two workgroups (16 waves) per CU.
constexpr int VH_LDS_HIST_WORDS = 2 * 4 * (1024 + 3);

struct VhWindows {
    uint32_t lo[VH_MAX_WIN];
    uint32_t shift[VH_MAX_WIN];
};

// grid (query blocks of 64 rows of [row_lo, row_lo + M), splits of the block's reference tiles); 512 threads; the first
// n_win * 2 * (bins + 3) words of the LDS histogram are used.  ghist (n_win, 2, bins + 3) u64, accumulated.  NORM: the score is
// normalised with mu / rsig (N) first (the plain pass, NORM = false, never reads them).
template <int KIND, bool NORM = false>
__global__ __launch_bounds__(512) void pair_hist_kernel(const float* __restrict__ qT, const float* __restrict__ ref,
                                                        const int32_t* __restrict__ label, int64_t N, int E, int64_t row_lo, int64_t M,
                                                        const float* __restrict__ rsq, const float* __restrict__ wpad, VhWindows win,
                                                        int n_win, int bins, int splits, unsigned long long* __restrict__ ghist,
                                                        const float* __restrict__ mu, const float* __restrict__ rsig) {
    constexpr int RT = ST_RT, RP = ST_RP;
    __shared__ __attribute__((aligned(16))) float rs[RT * RP];
    __shared__ uint32_t hist[VH_LDS_HIST_WORDS];
    const int slots = bins + 3;
    const int n_words = n_win * 2 * slots;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t mb = row_lo + (int64_t)blockIdx.x * ST_T;   // the block's first query row (global index)
    const int n_tiles = (int)((N + RT - 1) / RT);
    // reference tiles holding some j > i for a query of this block: from the tile of row mb + 1 on, split over blockIdx.y
    const int t_first = (int)((mb + 1) / RT);
    const int tps = (n_tiles - t_first + splits - 1) / splits;
    const int t_lo = t_first + blockIdx.y * tps;
    const int t_hi = min(n_tiles, t_lo + tps);
    if (t_lo >= t_hi) return;   // workgroup-uniform: nothing to count, nothing to flush

    for (int i = tid; i < n_words; i += 512) hist[i] = 0u;

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
    // its own copy of score_tile_loop (score_tile.hpp): through the shared one pass 1 took 20.50 instead of 20.19 ms, normalised 21.21 / 20.22
    const int nchunk = (EP + ST_EC - 1) / ST_EC;
    const int n_stage = (t_hi - t_lo) * nchunk;
    const bool vec = (E & 3) == 0;
    auto fetch = [&](int s, f32x4 (&v)[4]) {
        const int64_t n0 = (int64_t)(t_lo + s / nchunk) * RT;
        const int ec = (s % nchunk) * ST_EC;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int piece = tid + 512 * k, r = piece >> 4, c = (piece & 15) * 4;
            const int64_t row = n0 + r;
            const int col = ec + c;
            if (vec) {
                const bool ok = row < N && col < E;
                const f32x4 x = *reinterpret_cast<const f32x4*>(ref + (ok ? row * E + col : 0));
                v[k] = ok ? x : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[k][u] = (row < N && col + u < E) ? ref[row * E + col + u] : 0.f;
            }
        }
    };
    auto stash = [&](const f32x4 (&v)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int piece = tid + 512 * k, r = piece >> 4, c = (piece & 15) * 4;
            *reinterpret_cast<f32x4*>(rs + r * RP + c) = v[k];
        }
    };
    // under / over / NaN counts per lane in registers: in a zoom pass nearly every pair falls outside the window, and 64 lanes adding
    // to ONE LDS word serialise (measured: each such window cost about as much as the whole pass)
    uint32_t und[VH_MAX_WIN][2], ovr[VH_MAX_WIN][2], nanc[2] = {0u, 0u};
#pragma unroll
    for (int v = 0; v < VH_MAX_WIN; ++v) und[v][0] = und[v][1] = ovr[v][0] = ovr[v][1] = 0u;
    f32x4 nxt[4];
    fetch(0, nxt);
    float acc[8][2];
    for (int s = 0; s < n_stage; ++s) {
        const int t = t_lo + s / nchunk, ck = s % nchunk;
        const int ec = ck * ST_EC;
        const int ew4 = min(ST_EC, EP - ec) / 4;
        const int64_t n0 = (int64_t)t * RT;
        __syncthreads();   // the previous stage's readers are done (and, at s = 0, the histogram is zero)
        stash(nxt);
        if (s + 1 < n_stage) fetch(s + 1, nxt);
        __syncthreads();
        if (ck == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i][0] = acc[i][1] = 0.f;
        }
        const float* qe = qg + (ec / 4) * 32;
        const float* we = wpad + ec;
#pragma unroll 2
        for (int e4 = 0; e4 < ew4; ++e4) {
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(rs + lane * RP + e4 * 4);
            const f32x4 r1 = *reinterpret_cast<const f32x4*>(rs + (lane + 64) * RP + e4 * 4);
            f32x4 wv = {0.f, 0.f, 0.f, 0.f};
            if (KIND == VM_SCORE_WEIGHTED_L1) wv = *reinterpret_cast<const f32x4*>(we + e4 * 4);   // uniform: a scalar load
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(qe + e4 * 32 + i * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (KIND == VM_DIST_EUCLIDEAN || KIND == VM_SCORE_NEG_EUCLIDEAN) {
                        const float d0 = qv[c] - r0[c], d1 = qv[c] - r1[c];
                        acc[i][0] = fmaf(d0, d0, acc[i][0]);
                        acc[i][1] = fmaf(d1, d1, acc[i][1]);
                    } else if (KIND == VM_SCORE_WEIGHTED_L1) {
                        acc[i][0] = fmaf(wv[c], fabsf(qv[c] - r0[c]), acc[i][0]);
                        acc[i][1] = fmaf(wv[c], fabsf(qv[c] - r1[c]), acc[i][1]);
                    } else {
                        acc[i][0] = fmaf(qv[c], r0[c], acc[i][0]);
                        acc[i][1] = fmaf(qv[c], r1[c], acc[i][1]);
                    }
                }
            }
        }
        if (ck != nchunk - 1) continue;
        float rn[2] = {1.f, 1.f};
        int32_t rl[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t nn = n0 + lane + 64 * j;
            if (KIND == VM_DIST_COSINE) rn[j] = sqrtf(nn < N ? rsq[nn] : 1.f);
            if (KIND == VM_SCORE_PLDA) rn[j] = nn < N ? rsq[nn] : 0.f;
            rl[j] = nn < N ? label[nn] : 0;
        }
        float rmu[2], rrs[2];
        if constexpr (NORM) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t nn = n0 + lane + 64 * j;
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
                if (nn < N && nn > m && m < row_hi) {
                    const bool tgt = rl[j] == ql[i];
                    const int cls = tgt ? 0 : 1;
                    if (d != d) {
                        nanc[0] += tgt;
                        nanc[1] += !tgt;
                        continue;
                    }
                    const uint32_t k = score_key(d);
#pragma unroll
                    for (int v = 0; v < VH_MAX_WIN; ++v) {
                        if (v >= n_win) break;
                        const bool under = k < win.lo[v];
                        const uint32_t b = (k - win.lo[v]) >> win.shift[v];
                        const bool over = !under && b >= (uint32_t)bins;
                        und[v][0] += under && tgt;
                        und[v][1] += under && !tgt;
                        ovr[v][0] += over && tgt;
                        ovr[v][1] += over && !tgt;
                        if (!under && !over) atomicAdd(&hist[(v * 2 + cls) * slots + b], 1u);
                    }
                }
            }
        }
    }
    // the register counts: one wave sum each, added by lane 0
    auto wave_sum_u = [](uint32_t x) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        return x;
    };
    const uint32_t nan0 = wave_sum_u(nanc[0]), nan1 = wave_sum_u(nanc[1]);
#pragma unroll
    for (int v = 0; v < VH_MAX_WIN; ++v) {
        if (v >= n_win) break;
        const uint32_t c[6] = {wave_sum_u(und[v][0]), wave_sum_u(ovr[v][0]), nan0, wave_sum_u(und[v][1]), wave_sum_u(ovr[v][1]), nan1};
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (c[q] != 0u) atomicAdd(&hist[(v * 2 + q / 3) * slots + bins + q % 3], c[q]);
        }
    }
    __syncthreads();
    for (int i = tid; i < n_words; i += 512) {
        const uint32_t c = hist[i];
        if (c != 0u) __hip_atomic_fetch_add(&ghist[i], (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static int vh_splits(int64_t M, int64_t N) {
    const int s = score_splits(M, N, 4096);   // >= 4096 workgroups before the triangle empties the late blocks' ranges
    // a workgroup counts at most 64 x 128 x tiles pairs in its u32 LDS bins
    const int s_min = (int)cdiv(cdiv(N, ST_RT), (1 << 19) - 1);
    return s < s_min ? s_min : s;
}

}  // namespace vm

extern "C" int64_t vm_pair_score_hist_workspace_bytes(int64_t N, int E) {
    if (N <= 0 || E <= 0) return 0;
    const int64_t EP = ((E + 3) / 4) * 4;
    // squared row norms, the zero-padded weights, the scalar-path copy of (up to) all rows as queries
    return N * 4 + 256 + vm::ST_MAX_E * 4 + 256 + ((N + 7) / 8) * 8 * EP * 4 + 256;
}

namespace vm {

static int vh_run(const char* what, const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights,
                  int64_t row_lo, int64_t row_hi, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist, const float* mu,
                  const float* rsig, void* ws, void* stream) {
    VM_REQUIRE(emb && label && host_windows && hist && ws, "%s: null pointer", what);
    VM_REQUIRE(N > 0 && N < (1LL << 31) && E > 0 && E <= ST_MAX_E, "%s: bad sizes (N < 2^31, E <= %d)", what, ST_MAX_E);
    VM_REQUIRE((score_kind >= VM_DIST_EUCLIDEAN && score_kind <= VM_SCORE_NEG_EUCLIDEAN) || score_kind == VM_SCORE_PLDA,
               "%s: unknown score_kind %d", what, score_kind);
    VM_REQUIRE(plda_width_ok(score_kind, E), "%s: VM_SCORE_PLDA needs E %% 4 == 0 and E >= 4", what);
    VM_REQUIRE(score_kind != VM_SCORE_WEIGHTED_L1 || weights, "%s: weighted_l1 needs weights", what);
    VM_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= N, "%s: bad row range", what);
    VM_REQUIRE(n_windows >= 1 && n_windows <= VH_MAX_WIN && bins >= 1, "%s: 1..%d windows, bins >= 1", what, VH_MAX_WIN);
    VM_REQUIRE((int64_t)n_windows * 2 * (bins + 3) <= VH_LDS_HIST_WORDS, "%s: %d windows x %d bins exceed %d LDS words", what, n_windows, bins,
               VH_LDS_HIST_WORDS);
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)emb) & 15) == 0, "%s: emb must be 16-byte aligned when E %% 4 == 0", what);
    VhWindows win{};
    for (int v = 0; v < n_windows; ++v) {
        const int64_t lo = host_windows[2 * v], sh = host_windows[2 * v + 1];
        VM_REQUIRE(lo >= 0 && lo <= 0xffffffffLL && sh >= 0 && sh <= 31, "%s: window %d: key_lo in [0, 2^32), shift in [0, 31]", what, v);
        win.lo[v] = (uint32_t)lo;
        win.shift[v] = (uint32_t)sh;
    }
    const int64_t M = row_hi - row_lo;
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* rsq = (float*)ws;
    float* wpad = (float*)(((uintptr_t)(rsq + N) + 255) & ~(uintptr_t)255);
    float* qT = (float*)(((uintptr_t)(wpad + ST_MAX_E) + 255) & ~(uintptr_t)255);
    launch_row_scalars(score_kind, emb, N, E, rsq, st);
    launch_pad_weights(score_kind == VM_SCORE_WEIGHTED_L1 ? weights : nullptr, E, wpad, st);
    launch_pairdist_qt(emb + row_lo * (int64_t)E, M, E, qT, st, score_kind == VM_SCORE_PLDA ? E - 1 : -1);
    const int splits = vh_splits(M, N);
    const dim3 grid((unsigned)((M + ST_T - 1) / ST_T), (unsigned)splits);
    unsigned long long* gh = (unsigned long long*)hist;
#define VM_VH(K, NM) hipLaunchKernelGGL((pair_hist_kernel<K, NM>), grid, dim3(512), 0, st, qT, emb, label, N, E, row_lo, M, rsq, wpad, win, \
                                        n_windows, bins, splits, gh, mu, rsig)
#define VM_VH_KIND(NM)                                                 \
    switch (score_kind) {                                              \
        case VM_DIST_EUCLIDEAN: VM_VH(VM_DIST_EUCLIDEAN, NM); break;   \
        case VM_DIST_COSINE: VM_VH(VM_DIST_COSINE, NM); break;         \
        case VM_DIST_DOT: VM_VH(VM_DIST_DOT, NM); break;               \
        case VM_SCORE_WEIGHTED_L1: VM_VH(VM_SCORE_WEIGHTED_L1, NM); break; \
        case VM_SCORE_PLDA: VM_VH(VM_SCORE_PLDA, NM); break;           \
        default: VM_VH(VM_SCORE_NEG_EUCLIDEAN, NM); break;             \
    }
    if (mu == nullptr) {
        VM_VH_KIND(false);
    } else {
        VM_VH_KIND(true);
    }
#undef VM_VH_KIND
#undef VM_VH
    return check_launch(what);
}

}  // namespace vm

extern "C" int vm_pair_score_hist(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights,
                                  int64_t row_lo, int64_t row_hi, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist,
                                  void* ws, void* stream) {
    return vm::vh_run("vm_pair_score_hist", emb, label, N, E, score_kind, weights, row_lo, row_hi, host_windows, n_windows, bins, hist,
                      nullptr, nullptr, ws, stream);
}

extern "C" int vm_pair_score_hist_norm(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights,
                                       int64_t row_lo, int64_t row_hi, const int64_t* host_windows, int n_windows, int bins,
                                       const float* mu, const float* rsig, uint64_t* hist, void* ws, void* stream) {
    VM_REQUIRE(mu && rsig, "vm_pair_score_hist_norm: null pointer");
    return vm::vh_run("vm_pair_score_hist_norm", emb, label, N, E, score_kind, weights, row_lo, row_hi, host_windows, n_windows, bins, hist,
                      mu, rsig, ws, stream);
}
