// Batched agglomerative clustering of cached embeddings (voicemap_amd/diarization.py): the windows of R recordings lie back to back in
// emb (N, E); every recording is clustered on its own -- single, complete or average linkage under one of the three distances --
// and only the merge lists, the labels and the cluster counts leave the chip.  voicemap_amd/diarization.py ahc_reference is the numpy
// statement of the contract (include/voicemap_hip.h), matched bit for bit.
//
// Three steps on one stream:
//   1. launch_rowsq (cosine) and launch_pairdist_qt over all N rows (score_tile.hpp, defined in eval.hip).
//   2. ahc_dist_kernel: the block-diagonal distances.  One workgroup per GLOBAL group of 64 rows, whatever recordings they belong to;
//      its reference tiles run from the first tile of the first recording the group touches to the last tile of the last one, the
//      scores come from score_tile_loop -- every one bit-identical to dist[i][j] of vm_pairdist_argmin -- and the epilogue stores a
//      score only where query and reference lie in the same recording: D_r[i][j] at ws + mat0[r] + i n_r + j.  The diagonal is NaN.
//   3. ahc_merge_kernel: one workgroup per recording runs the whole merge loop.  The matrix stays in global memory (only this
//      workgroup touches it: __syncthreads() orders its stores and loads); rep / size / every row's cached nearest partner live in LDS.
//
// The cached partner of row k is the smallest (key, j) over the active j > k, so the smallest (key, k) over the rows is the
// contract's (key, a, b).  After a merge of (a, b), a < b: row a and every row whose cached partner was a or b (b only, for a < k < b)
// are scanned again, one wave per row; a row k < a whose partner was another compares its new D[k][a] with the cache; rows k > b hold
// neither a nor b among their partners.  Under single linkage a row k < a never needs the scan: its new D[k][a] is its old minimum.
//
// What bounds the loop: the step counter t < n - 1 in a workgroup-uniform register; the stop decision is written to LDS by one lane
// and read by every thread after a barrier; no barrier sits in divergent control flow; a scan runs over at most n columns.
#include "score_tile.hpp"

namespace vm {

constexpr int AHC_MAX_N = VM_AHC_MAX_N;
constexpr int AHC_THREADS = 1024, AHC_WAVES = AHC_THREADS / 64, AHC_CHUNKS = AHC_MAX_N / AHC_THREADS;
constexpr unsigned long long AHC_NONE = ~0ull;   // a row without a partner: above every (key, row, partner) entry
static_assert(AHC_MAX_N <= 65535 && AHC_MAX_N % AHC_THREADS == 0, "an entry holds row and partner in 16 bits each");

// the last r in [0, R) with row0[r] <= row: the recording of `row` (an empty recording never holds a row).  At most 32 steps; the
// index never leaves [0, R) whatever the table holds.
__device__ inline int ahc_recording(const int64_t* __restrict__ row0, int R, int64_t row) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (row0[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

// grid = groups of 64 rows of emb; 512 threads; wave w owns the rows m0 + 8 w .. + 7.  D: the matrices back to back (sq_total floats).
template <int KIND>
__global__ __launch_bounds__(512) void ahc_dist_kernel(const float* __restrict__ qT, const float* __restrict__ emb, int64_t N, int E,
                                                       const int64_t* __restrict__ row0, const int64_t* __restrict__ mat0, int R,
                                                       const float* __restrict__ rsq, float* __restrict__ D) {
    __shared__ __attribute__((aligned(16))) float rs[ST_RT * ST_RP];
    const int EP = ((E + 3) / 4) * 4, E4 = EP / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t g0 = (int64_t)blockIdx.x * ST_T;
    const int64_t m0 = g0 + 8 * w;
    const int64_t last_group = (N - 1) >> 3;   // a wave past the last row computes on the last group and stores nothing
    const float* qg = qT + ((m0 >> 3) < last_group ? (m0 >> 3) : last_group) * (int64_t)E4 * 32;
    // the recording of each of this wave's rows: its first row, the row behind its last, its matrix (wave-uniform)
    int qlo[8], qhi[8];   // N < 2^31
    int64_t qmat[8];
    float qn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + i;
        qlo[i] = qhi[i] = 0;
        qmat[i] = 0;
        qn[i] = 1.f;
        if (m < N) {
            if (i > 0 && m < qhi[i - 1]) {
                qlo[i] = qlo[i - 1], qhi[i] = qhi[i - 1], qmat[i] = qmat[i - 1];
            } else {
                const int r = ahc_recording(row0, R, m);
                qlo[i] = (int)row0[r], qhi[i] = (int)row0[r + 1], qmat[i] = mat0[r];
            }
            if (KIND == VM_DIST_COSINE) qn[i] = sqrtf(rsq[m]);
            if (KIND == VM_SCORE_PLDA) qn[i] = plda_row_term(rsq[m]);
        }
    }
    // the group's reference tiles: workgroup-uniform
    const int64_t g_last = (g0 + ST_T - 1 < N - 1) ? g0 + ST_T - 1 : N - 1;
    const int64_t ref_lo = row0[ahc_recording(row0, R, g0)];
    int64_t ref_hi = row0[ahc_recording(row0, R, g_last) + 1];
    if (ref_hi > N) ref_hi = N;
    const int t_lo = (int)((ref_lo < 0 ? 0 : ref_lo) / ST_RT);
    const int t_hi = (int)((ref_hi + ST_RT - 1) / ST_RT);
    score_tile_loop<KIND>(rs, qg, emb, N, E, nullptr, t_lo, t_hi, [&](int64_t n0, const float (&acc)[8][2]) {
        float rn[2] = {1.f, 1.f};
        if (KIND == VM_DIST_COSINE) {
#pragma unroll
            for (int j = 0; j < 2; ++j) rn[j] = sqrtf(n0 + lane + 64 * j < N ? rsq[n0 + lane + 64 * j] : 1.f);
        }
        if (KIND == VM_SCORE_PLDA) {
#pragma unroll
            for (int j = 0; j < 2; ++j) rn[j] = n0 + lane + 64 * j < N ? rsq[n0 + lane + 64 * j] : 0.f;
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
                } else if (KIND == VM_DIST_COSINE) {
                    d = 1.f - acc[i][j] / (qn[i] * rn[j]);
                } else if (KIND == VM_SCORE_PLDA) {
                    d = plda_finish(qn[i], rn[j], acc[i][j]);
                } else {
                    d = -acc[i][j];
                }
                if (nn == m) d = __uint_as_float(0x7fc00000u);
                // both rows in one recording (qlo = qhi = 0 for a row past N): a wave = 256 contiguous bytes of a matrix row
                if (nn >= qlo[i] && nn < qhi[i]) D[qmat[i] + (m - qlo[i]) * (int64_t)(qhi[i] - qlo[i]) + (nn - qlo[i])] = d;
            }
        }
    });
}

__device__ inline unsigned long long ahc_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ov = __shfl_xor(v, o, 64);
        v = ov < v ? ov : v;
    }
    return v;
}

__device__ inline unsigned long long ahc_entry(float d, int row, int partner) {
    return ((unsigned long long)score_key_nan_last(d) << 32) | ((unsigned long long)row << 16) | (unsigned long long)partner;
}

// D[k][a] after the merge of a and b (sa, sb, ss = size_a, size_b, size_a + size_b as floats; da = D[k][a], db = D[k][b]).  A tie of
// the keys keeps D[k][a].  Average: two products, a sum and a quotient, each rounded on its own; a NaN result is the canonical quiet NaN.
__device__ inline float ahc_link(int linkage, float da, float db, float sa, float sb, float ss) {
#pragma clang fp contract(off)
    if (linkage == VM_LINK_SINGLE) return score_key_nan_last(db) < score_key_nan_last(da) ? db : da;
    if (linkage == VM_LINK_COMPLETE) return score_key_nan_last(db) > score_key_nan_last(da) ? db : da;
    const float x = sa * da;
    const float y = sb * db;
    const float s = x + y;
    const float q = s / ss;
    return q != q ? __uint_as_float(0x7fc00000u) : q;
}

// Whole wave: the smallest (key, k, j) over the active j > k of row k of the n x n matrix D, AHC_NONE if there is none.
__device__ inline unsigned long long ahc_scan_row(const float* D, int n, int k, const int* rep, int lane) {
    unsigned long long m = AHC_NONE;
    for (int j = k + 1 + lane; j < n; j += 64) {
        if (rep[j] == j) {
            const unsigned long long e = ahc_entry(D[k * n + j], k, j);
            m = e < m ? e : m;
        }
    }
    return ahc_wave_min(m);
}

// grid = recordings; AHC_THREADS threads.  D_all is read AND written (no __restrict__: every step reads what the last one stored).
__global__ __launch_bounds__(AHC_THREADS) void ahc_merge_kernel(float* D_all, const int64_t* __restrict__ row0,
                                                                const int64_t* __restrict__ mat0, int linkage, float threshold,
                                                                const int32_t* __restrict__ target, int32_t* __restrict__ merge_a,
                                                                int32_t* __restrict__ merge_b, float* __restrict__ merge_h,
                                                                int32_t* __restrict__ merge_size, int32_t* __restrict__ labels,
                                                                int32_t* __restrict__ n_clusters) {
    __shared__ int rep[AHC_MAX_N];                   // k for an active slot, else the slot it was merged into (always a lower one)
    __shared__ int size[AHC_MAX_N];
    __shared__ unsigned long long best[AHC_MAX_N];   // (key << 32) | (k << 16) | partner: row k's cached nearest partner
    __shared__ unsigned short list[AHC_MAX_N];       // the rows to scan again; at the end, the number of every final cluster
    __shared__ unsigned long long wred[AHC_WAVES];
    __shared__ int wcnt[AHC_CHUNKS * AHC_WAVES];
    __shared__ int pick[3];                          // a, b, stop
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t lo = row0[r], n64 = row0[r + 1] - lo;
    if (n64 <= 0 || n64 > AHC_MAX_N) {   // workgroup-uniform; a table the caller should have refused leaves -1 and touches nothing else
        if (tid == 0) n_clusters[r] = n64 == 0 ? 0 : -1;
        return;
    }
    const int n = (int)n64;
    float* D = D_all + mat0[r];
    int T = target != nullptr ? target[r] : 1;
    if (T < 1) T = 1;
    for (int k = tid; k < n; k += AHC_THREADS) {
        rep[k] = k;
        size[k] = 1;
    }
    __syncthreads();
    if (n > T) {   // workgroup-uniform; a recording that merges nothing (target >= n) never reads its matrix
        for (int k = w; k < n; k += AHC_WAVES) {
            const unsigned long long e = ahc_scan_row(D, n, k, rep, lane);
            if (lane == 0) best[k] = e;
        }
    }
    __syncthreads();
    int c = n, t = 0;
    for (; t < n - 1; ++t) {
        if (c <= T) break;
        // ---- the smallest (key, a, b)
        unsigned long long m = AHC_NONE;
        for (int k = tid; k < n; k += AHC_THREADS) {
            const unsigned long long e = best[k];   // AHC_NONE for a retired row
            m = e < m ? e : m;
        }
        m = ahc_wave_min(m);
        if (lane == 0) wred[w] = m;
        __syncthreads();
        if (w == 0) {
            m = ahc_wave_min(lane < AHC_WAVES ? wred[lane] : AHC_NONE);
            if (lane == 0) {
                const int a = (int)((m >> 16) & 0xffffu), b = (int)(m & 0xffffu);
                int stop = 1;
                if (m != AHC_NONE) {
                    const float h = D[a * n + b];
                    stop = (threshold == threshold && !(h <= threshold)) ? 1 : 0;
                    if (!stop) {
                        merge_a[lo + t] = a;
                        merge_b[lo + t] = b;
                        merge_h[lo + t] = h;
                        merge_size[lo + t] = size[a] + size[b];
                    }
                }
                pick[0] = a, pick[1] = b, pick[2] = stop;
            }
        }
        __syncthreads();
        const int a = pick[0], b = pick[1];
        if (pick[2]) break;   // every thread reads the same word
        // ---- the linkage update of row and column a; who has to be scanned again
        const float sa = (float)size[a], sb = (float)size[b], ss = (float)(size[a] + size[b]);
        bool again[AHC_CHUNKS];
        int before[AHC_CHUNKS];
#pragma unroll
        for (int ch = 0; ch < AHC_CHUNKS; ++ch) {
            const int k = ch * AHC_THREADS + tid;
            again[ch] = false;
            if (k < n && k != b && rep[k] == k) {
                if (k == a) {
                    again[ch] = true;
                } else {
                    const float v = ahc_link(linkage, D[a * n + k], D[b * n + k], sa, sb, ss);
                    D[a * n + k] = v;
                    D[k * n + a] = v;
                    if (k < a) {
                        const unsigned long long cur = best[k];
                        const int p = (int)(cur & 0xffffu);
                        if ((p == a || p == b) && linkage != VM_LINK_SINGLE) {
                            again[ch] = true;
                        } else {
                            const unsigned long long e = ahc_entry(v, k, a);
                            if (e < cur) best[k] = e;
                        }
                    } else if (k < b) {
                        again[ch] = (int)(best[k] & 0xffffu) == b;
                    }
                }
            }
            const unsigned long long bal = __ballot(again[ch]);
            before[ch] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[ch * AHC_WAVES + w] = __popcll(bal);
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int ch = 0; ch < AHC_CHUNKS; ++ch) {
            for (int q = 0; q < AHC_WAVES; ++q) {
                if (q == w && again[ch]) list[total + before[ch]] = (unsigned short)(ch * AHC_THREADS + tid);
                total += wcnt[ch * AHC_WAVES + q];
            }
        }
        if (tid == 0) {   // b is retired
            size[a] += size[b];
            size[b] = 0;
            rep[b] = a;
            best[b] = AHC_NONE;
        }
        __syncthreads();
        for (int i = w; i < total; i += AHC_WAVES) {
            const int k = list[i];
            const unsigned long long e = ahc_scan_row(D, n, k, rep, lane);
            if (lane == 0) best[k] = e;
        }
        __syncthreads();
        c -= 1;
    }
    __syncthreads();
    // ---- the indices that hold no merge
    for (int i = t + tid; i < n; i += AHC_THREADS) {
        merge_a[lo + i] = -1;
        merge_b[lo + i] = -1;
        merge_h[lo + i] = __uint_as_float(0x7fc00000u);
        merge_size[lo + i] = -1;
    }
    // ---- labels: the final clusters numbered in ascending order of their slot
    bool root[AHC_CHUNKS];
    int before[AHC_CHUNKS];
#pragma unroll
    for (int ch = 0; ch < AHC_CHUNKS; ++ch) {
        const int k = ch * AHC_THREADS + tid;
        root[ch] = k < n && rep[k] == k;
        const unsigned long long bal = __ballot(root[ch]);
        before[ch] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[ch * AHC_WAVES + w] = __popcll(bal);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int ch = 0; ch < AHC_CHUNKS; ++ch) {
        for (int q = 0; q < AHC_WAVES; ++q) {
            if (q == w && root[ch]) list[ch * AHC_THREADS + tid] = (unsigned short)(total + before[ch]);
            total += wcnt[ch * AHC_WAVES + q];
        }
    }
    __syncthreads();
    for (int k = tid; k < n; k += AHC_THREADS) {
        int x = k;
        for (int it = 0; it < n && rep[x] != x; ++it) x = rep[x];
        labels[lo + k] = list[x];
    }
    if (tid == 0) n_clusters[r] = c;
}

static inline int64_t ahc_pad(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

}  // namespace vm

extern "C" int64_t vm_ahc_workspace_bytes(int64_t N, int E, int64_t R, int64_t sq_total) {
    if (N <= 0 || E <= 0 || R <= 0 || sq_total < 0) return 0;
    const int64_t EP = ((E + 3) / 4) * 4;
    // the matrices, N squared norms, all rows in scalar-path layout
    return vm::ahc_pad(sq_total * 4) + vm::ahc_pad(N * 4) + vm::ahc_pad(((N + 7) / 8) * 8 * EP * 4);
}

extern "C" int vm_ahc(const float* emb, int64_t N, int E, const int64_t* row0, const int64_t* mat0, int64_t R, int64_t sq_total,
                      int dist_kind, int linkage, float threshold, const int32_t* target, int32_t* merge_a, int32_t* merge_b,
                      float* merge_h, int32_t* merge_size, int32_t* labels, int32_t* n_clusters, void* ws, void* stream) {
    using namespace vm;
    VM_REQUIRE(N >= 0 && N < (1LL << 31) && R >= 0 && R < (1LL << 31) && E > 0 && E <= ST_MAX_E,
               "vm_ahc: bad sizes (N < 2^31, R < 2^31, 0 < E <= %d)", ST_MAX_E);
    VM_REQUIRE(sq_total >= 0 && sq_total <= N * (int64_t)AHC_MAX_N, "vm_ahc: sq_total must be in [0, N * %d]", AHC_MAX_N);
    VM_REQUIRE((dist_kind >= VM_DIST_EUCLIDEAN && dist_kind <= VM_DIST_DOT) || dist_kind == VM_SCORE_PLDA,
               "vm_ahc: dist_kind must be in (euclidean, cosine, dot_product, plda)");
    VM_REQUIRE(plda_width_ok(dist_kind, E), "vm_ahc: VM_SCORE_PLDA needs E %% 4 == 0 and E >= 4");
    VM_REQUIRE(linkage >= VM_LINK_SINGLE && linkage <= VM_LINK_AVERAGE, "vm_ahc: linkage must be in (single, complete, average)");
    if (R == 0 || N == 0) return 0;
    VM_REQUIRE(emb && row0 && mat0 && ws, "vm_ahc: null pointer");
    VM_REQUIRE(merge_a && merge_b && merge_h && merge_size && labels && n_clusters, "vm_ahc: null output pointer");
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)emb) & 15) == 0, "vm_ahc: emb must be 16-byte aligned when E %% 4 == 0");
    VM_REQUIRE((((uintptr_t)ws) & 15) == 0, "vm_ahc: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)ws;
    float* D = (float*)p;
    p += ahc_pad(sq_total * 4);
    float* rsq = (float*)p;
    p += ahc_pad(N * 4);
    float* qT = (float*)p;
    launch_row_scalars(dist_kind, emb, N, E, rsq, st);
    launch_pairdist_qt(emb, N, E, qT, st, dist_kind == VM_SCORE_PLDA ? E - 1 : -1);
    const dim3 grid((unsigned)((N + ST_T - 1) / ST_T));
#define VM_AD(KD) hipLaunchKernelGGL(ahc_dist_kernel<KD>, grid, dim3(512), 0, st, qT, emb, N, E, row0, mat0, (int)R, rsq, D)
    if (dist_kind == VM_DIST_EUCLIDEAN) VM_AD(VM_DIST_EUCLIDEAN);
    else if (dist_kind == VM_DIST_COSINE) VM_AD(VM_DIST_COSINE);
    else if (dist_kind == VM_SCORE_PLDA) VM_AD(VM_SCORE_PLDA);
    else VM_AD(VM_DIST_DOT);
#undef VM_AD
    hipLaunchKernelGGL(ahc_merge_kernel, dim3((unsigned)R), dim3(AHC_THREADS), 0, st, D, row0, mat0, linkage, threshold, target, merge_a,
                       merge_b, merge_h, merge_size, labels, n_clusters);
    return check_launch("vm_ahc");
}
