// Hard-pair mining over cached embeddings (voicemap_amd/mining.py): for every anchor row of a row shard of emb (N, E) its k_neg NEAREST
// rows of another speaker and its k_pos FARTHEST rows of its own speaker under the training distance -- the pairs a siamese step still
// learns from once uniformly drawn negatives lie beyond the margin.  Only the (M, K) lists leave the chip: no M x N score tile exists.
//
// mine_kernel's scores come from score_tile_loop (score_tile.hpp): every one is bit-identical to dist[i][j] of vm_pairdist_argmin.  Its
// own part is the epilogue: a small-K selection.
//
// An entry is ONE uint64: (order key << 32) | (j << 1) | (the score was -0.0).  The order key is score_key (score_tile.hpp) for the
// negatives and its complement for the positives, so "the K smallest entries, ascending" is the contract's (key, j) order for the first and (key
// descending, j ascending) for the second; the low bit only carries the sign of a zero back to the value output (j is unique per
// anchor, so it never decides an order).  Entries are totally ordered: the K smallest of a set do not depend on the order of arrival.
//
// An anchor's list lives in REGISTERS of the wave that owns it: lane p holds entry p (K <= 64), ascending, ~0 = empty.  The order key
// of its current worst entry (lane K - 1) is kept wave-uniform; a lane's candidate takes part only if its key is not above it -- after the
// first K candidates that is rare (about K ln(n / K) times per anchor) -- and the passing lanes of a ballot are inserted one by one: compare
// with the whole worst entry, count the entries below (ballot + popcount), shift the rest up one lane.  No LDS beside the reference
// stage, no atomics.  (The bar is the 32-bit key, not the 64-bit entry: 16 wave-uniform registers fewer, which keeps the kernel at
// four waves per SIMD without spills; a candidate that ties with the worst entry on the key pays the uniform branch.)
//
// The candidate range is split over blockIdx.y so the grid fills the chip; each split leaves its partial lists (splits, M, K) in the
// workspace and mine_merge_kernel (one wave per anchor) folds them with the same insertion and decodes index and score.
#include "score_tile.hpp"

namespace vm {

constexpr int MN_MAX_K = 64;
constexpr unsigned long long MN_EMPTY = ~0ull;

__device__ inline unsigned long long mn_readlane(unsigned long long v, int src) {   // src wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// Whole wave.  `list`: lane p = entry p of an ascending list of K entries (lanes >= K: empty); `thr`: the order key (high word) of entry
// K - 1, wave-uniform -- the cheap per-candidate test; a candidate that ties with it on the key is settled against the whole entry
// here.  Every lane whose `pass` holds offers `c`; those below the worst entry are inserted in lane order.
__device__ inline void mn_insert(unsigned long long& list, uint32_t& thr, unsigned long long c, bool pass, int K, int lane) {
    unsigned long long b = __ballot(K > 0 && pass && (uint32_t)(c >> 32) <= thr);
    while (b != 0ull) {
        const int src = __builtin_ctzll(b);
        b &= b - 1ull;
        const unsigned long long cv = mn_readlane(c, src);
        if (cv < mn_readlane(list, K - 1)) {   // wave-uniform: an earlier insertion of this ballot may have lowered the bar
            const bool lt = list < cv;         // a prefix of the lanes: the list is ascending
            const int pos = __popcll(__ballot(lt));
            const unsigned long long up = __shfl_up(list, 1, 64);
            list = lane >= K ? MN_EMPTY : (lt ? list : (lane == pos ? cv : up));
            thr = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(list >> 32), K - 1);
        }
    }
}

// grid (anchor blocks of 64 rows of [row_lo, row_lo + M), splits of the candidate tiles); 512 threads.  part_neg (splits, M, k_neg) /
// part_pos (splits, M, k_pos) uint64 entries.
template <int KIND>
__global__ __launch_bounds__(512, 4) void mine_kernel(const float* __restrict__ qT, const float* __restrict__ ref,
                                                   const int32_t* __restrict__ label, int64_t N, int E, int64_t row_lo, int64_t M,
                                                   const float* __restrict__ rsq, const float* __restrict__ neg_floor, int k_neg, int k_pos,
                                                   int tiles_per_split, unsigned long long* __restrict__ part_neg,
                                                   unsigned long long* __restrict__ part_pos) {
    constexpr int RT = ST_RT;
    __shared__ __attribute__((aligned(16))) float rs[ST_RT * ST_RP];
    const int EP = ((E + 3) / 4) * 4, E4 = EP / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = row_lo + (int64_t)blockIdx.x * ST_T + 8 * w;   // this wave's first anchor (global row)
    const int64_t ml0 = m0 - row_lo;                                   // ... as a row of qT
    const int64_t last_group = (M - 1) >> 3;   // a wave past the last anchor computes on the last group and keeps nothing
    const float* qg = qT + ((ml0 >> 3) < last_group ? (ml0 >> 3) : last_group) * (int64_t)E4 * 32;
    const int64_t row_hi = row_lo + M;
    float qn[8];
    int32_t ql[8];
    uint32_t fkey[8];   // a negative needs key >= fkey: key(floor) + 1, or 0 without a floor
    bool aok[8];
    unsigned long long nl[8], pl[8];
    uint32_t nthr[8], pthr[8];   // the order key of each list's worst entry
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool ok = m0 + i < row_hi;
        qn[i] = (KIND == VM_DIST_COSINE && ok) ? sqrtf(rsq[m0 + i]) : 1.f;
        ql[i] = ok ? label[m0 + i] : -1;
        aok[i] = ok && ql[i] >= 0;
        const float fl = (ok && neg_floor != nullptr) ? neg_floor[m0 + i - row_lo] : __uint_as_float(0x7fc00000u);
        fkey[i] = fl != fl ? 0u : score_key(fl) + 1u;   // key(+inf) + 1 still fits
        nl[i] = pl[i] = MN_EMPTY;
        nthr[i] = pthr[i] = 0xffffffffu;
    }
    const int n_tiles = (int)((N + RT - 1) / RT);
    const int t_lo = blockIdx.y * tiles_per_split;
    const int t_hi = min(n_tiles, t_lo + tiles_per_split);
    score_tile_loop<KIND>(rs, qg, ref, N, E, nullptr, t_lo, t_hi, [&](int64_t n0, const float (&acc)[8][2]) {
        float rn[2] = {1.f, 1.f};
        int32_t rl[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t nn = n0 + lane + 64 * j;
            if (KIND == VM_DIST_COSINE) rn[j] = sqrtf(nn < N ? rsq[nn] : 1.f);
            rl[j] = nn < N ? label[nn] : -1;   // a row past N takes part like an unlabelled one: never
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t nn = n0 + lane + 64 * j;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float d;
                if (KIND == VM_DIST_EUCLIDEAN) {
                    d = sqrtf(acc[i][j]);
                } else if (KIND == VM_DIST_COSINE) {
                    d = 1.f - acc[i][j] / (qn[i] * rn[j]);
                } else {
                    d = -acc[i][j];
                }
                const uint32_t key = score_key(d);
                const bool cand = aok[i] && rl[j] >= 0 && d == d && nn != m0 + i;
                const bool same = rl[j] == ql[i];
                const uint32_t low = ((uint32_t)nn << 1) | (__float_as_uint(d) == 0x80000000u ? 1u : 0u);
                // the whole wave calls: the ballots inside see every lane
                mn_insert(nl[i], nthr[i], ((unsigned long long)key << 32) | low, cand && !same && key >= fkey[i], k_neg, lane);
                mn_insert(pl[i], pthr[i], ((unsigned long long)(~key) << 32) | low, cand && same, k_pos, lane);
            }
        }
    });
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (m0 + i >= row_hi) break;   // wave-uniform
        const int64_t slot = (int64_t)blockIdx.y * M + (ml0 + i);
        if (lane < k_neg) part_neg[slot * k_neg + lane] = nl[i];
        if (lane < k_pos) part_pos[slot * k_pos + lane] = pl[i];
    }
}

// One wave per anchor: the K smallest entries of its `splits` partial lists, decoded.  comp: the order key is the complemented key
// (the positives).  idx / val (M, K): -1 / NaN where the list ends.
__global__ __launch_bounds__(256) void mine_merge_kernel(const unsigned long long* __restrict__ part, int64_t M, int K, int splits, int comp,
                                                         int32_t* __restrict__ idx, float* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= M) return;   // wave-uniform
    unsigned long long list = MN_EMPTY;
    uint32_t thr = 0xffffffffu;
    for (int s = 0; s < splits; ++s) {
        const unsigned long long c = lane < K ? part[((int64_t)s * M + row) * K + lane] : MN_EMPTY;
        mn_insert(list, thr, c, c != MN_EMPTY, K, lane);
    }
    if (lane >= K) return;
    int32_t j = -1;
    uint32_t bits = 0x7fc00000u;
    if (list != MN_EMPTY) {
        const uint32_t ok = (uint32_t)(list >> 32), low = (uint32_t)list;
        const uint32_t key = comp ? ~ok : ok;
        j = (int32_t)(low >> 1);
        bits = (low & 1u) ? 0x80000000u : ((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
    }
    idx[row * K + lane] = j;
    val[row * K + lane] = __uint_as_float(bits);
}

static inline int64_t mn_pad(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

}  // namespace vm

extern "C" int64_t vm_mine_pairs_workspace_bytes(int64_t N, int E, int64_t row_lo, int64_t row_hi, int k_neg, int k_pos) {
    if (N <= 0 || E <= 0 || row_lo < 0 || row_hi <= row_lo || k_neg < 0 || k_pos < 0) return 0;
    const int64_t M = row_hi - row_lo, EP = ((E + 3) / 4) * 4;
    // squared row norms, the scalar-path copy of the anchors, the partial lists of every split
    return 256 + vm::mn_pad(N * 4) + vm::mn_pad(((M + 7) / 8) * 8 * EP * 4) + (int64_t)vm::score_splits(M, N, 2048) * M * (k_neg + k_pos) * 8;
}

extern "C" int vm_mine_pairs(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, int64_t row_lo, int64_t row_hi,
                             int k_neg, int k_pos, const float* neg_floor, int32_t* neg_idx, float* neg_val, int32_t* pos_idx,
                             float* pos_val, void* ws, void* stream) {
    using namespace vm;
    VM_REQUIRE(emb && label && ws, "vm_mine_pairs: null pointer");
    VM_REQUIRE(k_neg >= 0 && k_neg <= MN_MAX_K && k_pos >= 0 && k_pos <= MN_MAX_K, "vm_mine_pairs: k_neg, k_pos must be in [0, %d]", MN_MAX_K);
    VM_REQUIRE(k_neg + k_pos > 0, "vm_mine_pairs: k_neg and k_pos are both zero");
    VM_REQUIRE((k_neg > 0) == (neg_idx != nullptr) && (k_neg > 0) == (neg_val != nullptr),
               "vm_mine_pairs: neg_idx and neg_val go with k_neg > 0 (both) or k_neg == 0 (both NULL)");
    VM_REQUIRE((k_pos > 0) == (pos_idx != nullptr) && (k_pos > 0) == (pos_val != nullptr),
               "vm_mine_pairs: pos_idx and pos_val go with k_pos > 0 (both) or k_pos == 0 (both NULL)");
    VM_REQUIRE(N > 0 && N < (1LL << 31) && E > 0 && E <= ST_MAX_E, "vm_mine_pairs: bad sizes (N < 2^31, E <= %d)", ST_MAX_E);
    VM_REQUIRE(score_kind >= VM_DIST_EUCLIDEAN && score_kind <= VM_DIST_DOT,
               "vm_mine_pairs: score_kind must be in (euclidean, cosine, dot_product)");
    VM_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= N, "vm_mine_pairs: bad row range");
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)emb) & 15) == 0, "vm_mine_pairs: emb must be 16-byte aligned when E %% 4 == 0");
    const int64_t M = row_hi - row_lo;
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t EP = ((E + 3) / 4) * 4;
    char* p = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* rsq = (float*)p;
    p += mn_pad(N * 4);
    float* qT = (float*)p;
    p += mn_pad(((M + 7) / 8) * 8 * EP * 4);
    const int splits = score_splits(M, N, 2048);
    unsigned long long* part_neg = (unsigned long long*)p;
    unsigned long long* part_pos = part_neg + (int64_t)splits * M * k_neg;
    if (score_kind == VM_DIST_COSINE) launch_rowsq(emb, N, E, rsq, st);
    launch_pairdist_qt(emb + row_lo * (int64_t)E, M, E, qT, st);
    const int n_tiles = (int)((N + ST_RT - 1) / ST_RT);
    const int tps = (n_tiles + splits - 1) / splits;
    const dim3 grid((unsigned)((M + ST_T - 1) / ST_T), (unsigned)splits);
#define VM_MN(KD) hipLaunchKernelGGL(mine_kernel<KD>, grid, dim3(512), 0, st, qT, emb, label, N, E, row_lo, M, rsq, neg_floor, k_neg, k_pos, tps, \
                                     part_neg, part_pos)
    if (score_kind == VM_DIST_EUCLIDEAN) VM_MN(VM_DIST_EUCLIDEAN);
    else if (score_kind == VM_DIST_COSINE) VM_MN(VM_DIST_COSINE);
    else VM_MN(VM_DIST_DOT);
#undef VM_MN
    const dim3 mg((unsigned)((M + 3) / 4));
    if (k_neg > 0) hipLaunchKernelGGL(mine_merge_kernel, mg, dim3(256), 0, st, part_neg, M, k_neg, splits, 0, neg_idx, neg_val);
    if (k_pos > 0) hipLaunchKernelGGL(mine_merge_kernel, mg, dim3(256), 0, st, part_pos, M, k_pos, splits, 1, pos_idx, pos_val);
    return check_launch("vm_mine_pairs");
}
