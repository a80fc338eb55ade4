// The tile loop of everything that scores cached embeddings -- pairdist_kernel (eval.hip), cohort_score_kernel (cohort.hip), mine_kernel
// (mine.hip), pair_calib_kernel (calib.hip), ahc_dist_kernel (cluster.hip) call it; pair_hist_kernel (verif.hip) keeps a copy, because it measured slower through the
// call -- and the small helpers around it.  Every score of theirs is bit-identical to dist[i][j] of vm_pairdist_argmin because they run
// THIS text; what a kernel does with a finished tile (argmin, histogram, score tile, selection lists, calibration sums) is its own
// epilogue in its own file.
#pragma once
#include "common.hpp"

namespace vm {

// queries per workgroup, references per stage, components per stage, LDS row pitch (68 floats = 17 bank quads), the widest embedding
constexpr int ST_T = 64, ST_RT = 128, ST_EC = 64, ST_RP = ST_EC + 4, ST_MAX_E = 256;

// ---- the order-preserving uint32 key of an fp32 score ------------------------------------------------------------------------------
// -0.0 is first canonicalised to +0.0; key = bits | 2^31 for a non-negative value, ~bits for a negative one.
__device__ inline uint32_t score_key(float s) {
    uint32_t u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;   // -0.0 == +0.0: one key
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// ... with every NaN at 2^32 - 1, above every other key
__device__ inline uint32_t score_key_nan_last(float s) { return s != s ? 0xffffffffu : score_key(s); }
// the score of a key (the +0.0 of a zero)
__device__ inline float score_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the cohort-normalised score of vm_pair_score_hist_norm and vm_pair_calib_sums: fp32, every operation rounded on its own
__device__ inline float vh_norm(float s, float mi, float ri, float mj, float rj) {
#pragma clang fp contract(off)
    const float a = s - mi;
    const float b = s - mj;
    const float x = a * ri;
    const float y = b * rj;
    return 0.5f * (x + y);
}

// VM_SCORE_PLDA: the rows are PLDA-space rows (voicemap_amd/plda.py) whose LAST column is the row's own term h.  The tile loop runs its
// dot branch over all E components with the query copy's component E - 1 written as zero (fmaf(0, r, acc) == acc: the chain is that of
// components 0 .. E - 2), and the finishing line is s = (h_q + h_r) - acc, each operation rounded on its own.  A row term that is not
// finite makes the score NaN from either side: 0 * inf (or 0 * NaN) in the chain for the reference row, plda_row_term for the query row.
__device__ inline float plda_row_term(float h) { return (__float_as_uint(h) & 0x7f800000u) == 0x7f800000u ? __uint_as_float(0x7fc00000u) : h; }
__device__ inline float plda_finish(float hq, float hr, float acc) {
#pragma clang fp contract(off)
    const float t = hq + hr;
    return t - acc;
}

// ---- preparation launches (defined in eval.hip) --------------------------------------------------------------------------------------
// row squared norms (fmaf, ascending component per lane, wave sum) and the scalar-path query layout qT of the tile loop; zero_col >= 0:
// that component of every query is written as zero (VM_SCORE_PLDA: E - 1)
void launch_rowsq(const float* x, int64_t rows, int E, float* out, hipStream_t st);
void launch_pairdist_qt(const float* q, int64_t M, int E, float* qT, hipStream_t st, int zero_col = -1);
// VM_SCORE_PLDA's per-row scalar in place of the squared norm: out[r] = x[r][E - 1]
void launch_rowterm(const float* x, int64_t rows, int E, float* out, hipStream_t st);
// the per-row scalars of a score kind into `out` (cosine: squared norms, PLDA: row terms, every other kind: nothing)
inline void launch_row_scalars(int kind, const float* x, int64_t rows, int E, float* out, hipStream_t st) {
    if (kind == VM_DIST_COSINE) launch_rowsq(x, rows, E, out, st);
    else if (kind == VM_SCORE_PLDA) launch_rowterm(x, rows, E, out, st);
}
// what every scorer asks of VM_SCORE_PLDA's width
inline bool plda_width_ok(int kind, int E) { return kind != VM_SCORE_PLDA || (E >= 4 && (E & 3) == 0); }
// wpad[0 .. ST_MAX_E) = w[0 .. E) followed by zeros (all zeros for w == NULL): the weights of VM_SCORE_WEIGHTED_L1
void launch_pad_weights(const float* w, int E, float* wpad, hipStream_t st);

// ---- the cohort selection (defined in cohort.hip; shared with enrol_norm.hip) ----------------------------------------------------------
// rows of one score tile of C-entry lines (a multiple of 64 within the tile cap, at most M)
int64_t cs_tile_rows(int64_t M, int64_t C);
// vm_cohort_topk_stats' selection and statistics of `lines` lines of C entries: the rows of a tile (lines, C) (col_ld == 0) or the
// columns of a tile (C, col_ld).  Line r writes mu / sigma / rsig / count [row0 + r] and, if topk_idx, its K slots; list: lines x C int32
// of scratch (read only with topk_idx).
void launch_cohort_select(const float* tile, int64_t lines, int64_t C, int64_t K, int64_t row0, int64_t col_ld, float* mu, float* sigma,
                          float* rsig, int32_t* count, int32_t* topk_idx, int32_t* list, hipStream_t st);

// splits of the reference tiles so that the grid holds at least `target` workgroups (2048 = 8 per CU), one tile per split at the least
inline int score_splits(int64_t rows, int64_t refs, int64_t target) {
    const int64_t nt = cdiv(refs, ST_RT);
    int64_t s = cdiv(target, cdiv(rows, ST_T));
    if (s > nt) s = nt;
    if (s < 1) s = 1;
    return (int)s;
}

// ---- the tile loop -------------------------------------------------------------------------------------------------------------------
// Workgroup = 8 waves; a wave owns 8 queries -- WAVE-UNIFORM, so their components arrive through scalar loads (SGPR operands of the
// subtract / FMA: no LDS read, no vector register) from its group `qg` of qT -- and lane l the references n0 + l and n0 + l + 64 of a
// 128-reference stage, whose 64 components per stage it reads from LDS 16 bytes at a time: ONE LDS read per 32 component pairs.
// The euclidean distance is the direct form sum (a - b)^2 -- no ||a||^2 + ||b||^2 - 2ab cancellation -- 2 VALU instructions per component
// pair: the bound is fp32 VALU issue (2 x M x N x E / 64 wave instructions; v_pk_* do not issue faster on gfx950).
//
// How it came to this, on the 13 002 x 104 014 x 64 shard of BASELINE.json config 5 (profiles/r06_pairdist.txt): the round-5 kernel
// (16 x 16 threads, 4 x 4 register tiles, both operands from LDS) ran 8.9 ms -- it was LDS-bound: a thread's four ADJACENT reference rows
// put lanes tx, tx + 4, tx + 8, tx + 12 on the same banks (4-way conflicts on every reference read).  Rows 16 apart + register prefetch
// of the next stage: 5.5 ms, and the dot product at 3.5 ms showed the LDS still level with the VALU (8 reads per 64 component pairs).
// Round 6 made the queries wave-uniform (pairdist_qt_kernel lays them out for the scalar path) and the lanes references.
//
// rs: the workgroup's LDS stage, ST_RT * ST_RP floats, 16-byte aligned.  ref (N, E); wpad is read only for VM_SCORE_WEIGHTED_L1.  Whole
// 512-thread workgroup (two barriers per stage).  For every reference tile t of [t_lo, t_hi), tile(n0 = t * ST_RT, acc) is called once
// with acc[i][j] = the ascending-component fmaf chain of query i and reference n0 + lane + 64 j: sum (q - r)^2 (euclidean and its
// negation), sum w |q - r| (weighted L1) or sum q r (cosine, dot, PLDA).  Rows past N and components past E enter as zeros.  `tile` is taken
// BY VALUE: as a forwarding reference pairdist_kernel<cosine> went from 94 to 99 VGPRs and from 5 to 4 waves per SIMD.
template <int KIND, typename Tile>
__device__ __forceinline__ void score_tile_loop(float* rs, const float* __restrict__ qg, const float* __restrict__ ref, int64_t N, int E,
                                                const float* __restrict__ wpad, int t_lo, int t_hi, Tile tile) {
    constexpr int RT = ST_RT, RP = ST_RP;
    const int EP = ((E + 3) / 4) * 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int nchunk = (EP + ST_EC - 1) / ST_EC;
    const int n_stage = (t_hi - t_lo) * nchunk;
    const bool vec = (E & 3) == 0;
    // stage s = (tile t_lo + s / nchunk, components (s % nchunk) * 64 ..): this thread's four 16-byte pieces, piece = tid + 512 k
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
    f32x4 nxt[4];
    if (n_stage > 0) fetch(0, nxt);
    float acc[8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i][0] = acc[i][1] = 0.f;
    for (int s = 0; s < n_stage; ++s) {
        const int t = t_lo + s / nchunk, ck = s % nchunk;
        const int ec = ck * ST_EC;
        const int ew4 = min(ST_EC, EP - ec) / 4;
        __syncthreads();  // the previous stage's readers are done
        stash(nxt);
        if (s + 1 < n_stage) fetch(s + 1, nxt);   // in flight while this stage is consumed
        __syncthreads();
        const float* qe = qg + (ec / 4) * 32;
#pragma unroll 2
        for (int e4 = 0; e4 < ew4; ++e4) {
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(rs + lane * RP + e4 * 4);
            const f32x4 r1 = *reinterpret_cast<const f32x4*>(rs + (lane + 64) * RP + e4 * 4);
            f32x4 wv = {0.f, 0.f, 0.f, 0.f};
            if (KIND == VM_SCORE_WEIGHTED_L1) wv = *reinterpret_cast<const f32x4*>(wpad + ec + e4 * 4);   // uniform: a scalar load
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(qe + e4 * 32 + i * 4);   // uniform address: a scalar load
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
        if (ck == nchunk - 1) {
            tile((int64_t)t * RT, acc);
            // zeroed here, not under `ck == 0` in front of the component loop: there it compiled to 16 selects per stage and
            // vm_pairdist_argmin lost 0.4 - 1.1 % (profiles/score_tile_refactor.txt)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i][0] = acc[i][1] = 0.f;
        }
    }
}

}  // namespace vm
