// Triplet loss with mining inside the batch (include/voicemap_hip.h, vm_triplet_loss): two launches, no atomics, every sum in one
// fixed order.
//   launch 1 (triplet_anchor_kernel): workgroup a is anchor a.  Its row of squared distances goes into LDS (each wave one candidate
//     at a time: a lane's components ascending with fmaf, then the xor butterfly), the two selections are butterflies on (s, j), and
//     in ALL mode the triplets are walked positives ascending (a loop the whole workgroup takes together), a thread's negatives
//     ascending.  It writes the anchor's row of the pair-weight matrix W (N, N) -- W[a][j] = +-(accumulated weight) / d_aj, 0 where
//     s_aj == 0 -- with its loss term, its counts and a flag for a non-finite distance.
//   launch 2 (triplet_grad_kernel): workgroup i < N, thread t: demb[i][t] = scale * sum_j (W[i][j] + W[j][i]) (e_i[t] - e_j[t]) / norm,
//     j ascending; the norm (V, A or T) is an integer sum every workgroup forms for itself.  Workgroup N forms the means in row order.
#include "common.hpp"

namespace vm {

constexpr int TR_MAX_N = 1024;   // the anchor's row of s: 4 KiB of LDS; four candidates per thread of a 256-thread workgroup
constexpr int TR_MAX_E = 256;    // four components per lane
constexpr int TR_U = TR_MAX_N / 256;

struct TrWs {   // the workspace, in this order
    float* W;          // (N, N)
    float* row_loss;   // (N)  sum of the anchor's loss terms
    int32_t* cnt;      // (N)  HARD: 1 for a valid anchor; ALL: the anchor's triplets
    int32_t* act;      // (N)  of those, the ones with x > 0
    int32_t* bad;      // (N)  1: the anchor met a non-finite squared distance
};
__host__ __device__ inline TrWs tr_ws(void* ws, int64_t N) {
    TrWs w;
    w.W = (float*)ws;
    w.row_loss = w.W + N * N;
    w.cnt = (int32_t*)(w.row_loss + N);
    w.act = w.cnt + N;
    w.bad = w.act + N;
    return w;
}

__device__ inline int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// softplus(x) = max(x, 0) + log1p(exp(-|x|)) and its derivative sigmoid(x), neither overflowing
__device__ inline float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ inline float sigmoid_f(float x) {
    const float t = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : t) / (1.f + t);
}

// (val, idx) orders: idx < 0 is "none"; `far` = first by (val descending, idx ascending), else by (val ascending, idx ascending)
__device__ inline void take(float& v, int& i, float ov, int oi, bool far) {
    if (oi >= 0 && (i < 0 || (far ? ov > v : ov < v) || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}

__global__ __launch_bounds__(256) void triplet_anchor_kernel(const float* __restrict__ emb, const int32_t* __restrict__ label, int N, int E,
                                                             int mining, int soft, float margin, int32_t* __restrict__ hard_pos,
                                                             int32_t* __restrict__ hard_neg, TrWs ws, int train) {
    __shared__ float s_s[TR_MAX_N];       // s_aj, then (ALL) d_aj
    __shared__ int32_t s_lab[TR_MAX_N];
    __shared__ float s_wp[TR_MAX_N];      // ALL: the weight of positive j
    __shared__ float s_part[4][TR_MAX_N]; // ALL: per wave, per positive (in order of appearance) the sum of its triplets' weights
    __shared__ int32_t s_posidx[TR_MAX_N];
    __shared__ float s_rv[2][4];
    __shared__ int32_t s_ri[5][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x;
    const int la = label[a];
    float* Wrow = ws.W + (int64_t)a * N;
    if (la < 0) {   // takes no part (uniform)
        if (train)
            for (int j = tid; j < N; j += 256) Wrow[j] = 0.f;
        if (tid == 0) {
            ws.row_loss[a] = 0.f;
            ws.cnt[a] = ws.act[a] = ws.bad[a] = 0;
            if (hard_pos) hard_pos[a] = -1;
            if (hard_neg) hard_neg[a] = -1;
        }
        return;
    }
    for (int j = tid; j < N; j += 256) s_lab[j] = label[j];
    // the row of squared distances: direct form, no norm expansion
    float av[TR_MAX_E / 64];
#pragma unroll
    for (int u = 0; u < TR_MAX_E / 64; ++u) av[u] = (lane + 64 * u < E) ? emb[(int64_t)a * E + lane + 64 * u] : 0.f;
    for (int j0 = wave; j0 < N; j0 += 16) {   // four candidates per trip: their loads are independent and in flight together
        float d2[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + 4 * b;
            d2[b] = 0.f;
            if (j < N) {   // (uniform)
                const float* r = emb + (int64_t)j * E;
#pragma unroll
                for (int u = 0; u < TR_MAX_E / 64; ++u)
                    if (lane + 64 * u < E) {
                        const float d = av[u] - r[lane + 64 * u];
                        d2[b] = fmaf(d, d, d2[b]);
                    }
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float s = wave_sum(d2[b]);
            if (lane == 0 && j0 + 4 * b < N) s_s[j0 + 4 * b] = s;
        }
    }
    __syncthreads();
    // selections, set sizes and the non-finite flag: candidate j = tid + 256 u
    float pv = 0.f, nv = 0.f;
    int pi = -1, ni = -1, npos = 0, nneg = 0, bad = 0;
#pragma unroll
    for (int u = 0; u < TR_U; ++u) {
        const int j = tid + 256 * u;
        if (j < N && s_lab[j] >= 0) {
            const float s = s_s[j];
            if (!(fabsf(s) < INFINITY)) bad = 1;   // the anchor's own row included: s_aa is 0 for a finite row
            if (j != a) {
                if (s_lab[j] == la) {
                    ++npos;
                    take(pv, pi, s, j, true);
                } else {
                    ++nneg;
                    take(nv, ni, s, j, false);
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        take(pv, pi, __shfl_xor(pv, o, 64), __shfl_xor(pi, o, 64), true);
        take(nv, ni, __shfl_xor(nv, o, 64), __shfl_xor(ni, o, 64), false);
    }
    npos = wave_sum_i(npos);
    nneg = wave_sum_i(nneg);
    bad = wave_sum_i(bad);
    if (lane == 0) {
        s_rv[0][wave] = pv;
        s_rv[1][wave] = nv;
        s_ri[0][wave] = pi;
        s_ri[1][wave] = ni;
        s_ri[2][wave] = npos;
        s_ri[3][wave] = nneg;
        s_ri[4][wave] = bad;
    }
    __syncthreads();
    pv = s_rv[0][0], pi = s_ri[0][0], nv = s_rv[1][0], ni = s_ri[1][0];
    for (int w = 1; w < 4; ++w) {   // the four waves in order: every thread ends with the same pair
        take(pv, pi, s_rv[0][w], s_ri[0][w], true);
        take(nv, ni, s_rv[1][w], s_ri[1][w], false);
    }
    npos = s_ri[2][0] + s_ri[2][1] + s_ri[2][2] + s_ri[2][3];
    nneg = s_ri[3][0] + s_ri[3][1] + s_ri[3][2] + s_ri[3][3];
    bad = (s_ri[4][0] + s_ri[4][1] + s_ri[4][2] + s_ri[4][3]) != 0;
    const bool valid = npos > 0 && nneg > 0 && !bad && pi >= 0 && ni >= 0;
    if (tid == 0) {
        if (hard_pos) hard_pos[a] = valid ? pi : -1;
        if (hard_neg) hard_neg[a] = valid ? ni : -1;
    }
    if (!valid) {   // (uniform) no triplet, or a non-finite distance: the loss term carries the NaN, the flag poisons the gradient
        if (train)
            for (int j = tid; j < N; j += 256) Wrow[j] = 0.f;
        if (tid == 0) {
            ws.row_loss[a] = bad ? NAN : 0.f;
            ws.cnt[a] = ws.act[a] = 0;
            ws.bad[a] = bad;
        }
        return;
    }
    if (mining == VM_TRIPLET_HARD) {
        const float dp = sqrtf(pv), dn = sqrtf(nv);
        const float x = soft ? dp - dn : (margin + dp) - dn;
        const float g = soft ? sigmoid_f(x) : (x > 0.f ? 1.f : 0.f);
        if (train)
            for (int j = tid; j < N; j += 256) Wrow[j] = (j == pi && pv > 0.f) ? g / dp : (j == ni && nv > 0.f) ? -g / dn : 0.f;
        if (tid == 0) {
            ws.row_loss[a] = soft ? softplus_f(x) : fmaxf(x, 0.f);
            ws.cnt[a] = 1;
            ws.act[a] = x > 0.f ? 1 : 0;
            ws.bad[a] = 0;
        }
        return;
    }
    // VM_TRIPLET_ALL: every (p, n); distances once
    __syncthreads();   // (s_s is about to be rewritten; the selections above read it)
    for (int j = tid; j < N; j += 256) s_s[j] = sqrtf(s_s[j]);
    __syncthreads();
    float dn[TR_U], wn[TR_U];
    bool isn[TR_U];
#pragma unroll
    for (int u = 0; u < TR_U; ++u) {
        const int j = tid + 256 * u;
        isn[u] = j < N && s_lab[j] >= 0 && s_lab[j] != la;
        dn[u] = isn[u] ? s_s[j] : 0.f;
        wn[u] = 0.f;
    }
    float loss = 0.f;
    int act = 0, q = 0;
    for (int p = 0; p < N; ++p) {
        if (s_lab[p] != la || p == a) continue;   // (uniform)
        const float base = soft ? s_s[p] : margin + s_s[p];
        float wsum = 0.f;
#pragma unroll
        for (int u = 0; u < TR_U; ++u)
            if (isn[u]) {
                const float x = base - dn[u];
                const float g = soft ? sigmoid_f(x) : (x > 0.f ? 1.f : 0.f);
                loss += soft ? softplus_f(x) : fmaxf(x, 0.f);
                act += x > 0.f ? 1 : 0;
                wn[u] += g;
                wsum += g;
            }
        wsum = wave_sum(wsum);
        if (lane == 0) s_part[wave][q] = wsum;
        if (tid == 0) s_posidx[q] = p;
        ++q;
    }
    loss = wave_sum(loss);
    act = wave_sum_i(act);
    if (lane == 0) {
        s_rv[0][wave] = loss;
        s_ri[0][wave] = act;
    }
    __syncthreads();
    for (int k = tid; k < q; k += 256) {
        const int p = s_posidx[k];
        const float w = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
        s_wp[p] = s_s[p] > 0.f ? w / s_s[p] : 0.f;
    }
    __syncthreads();
    if (train) {
#pragma unroll
        for (int u = 0; u < TR_U; ++u) {
            const int j = tid + 256 * u;
            if (j < N) Wrow[j] = isn[u] ? (dn[u] > 0.f ? -wn[u] / dn[u] : 0.f) : (s_lab[j] == la && j != a) ? s_wp[j] : 0.f;
        }
    }
    if (tid == 0) {
        ws.row_loss[a] = ((s_rv[0][0] + s_rv[0][1]) + s_rv[0][2]) + s_rv[0][3];
        ws.cnt[a] = npos * nneg;
        ws.act[a] = s_ri[0][0] + s_ri[0][1] + s_ri[0][2] + s_ri[0][3];
        ws.bad[a] = 0;
    }
}

// the integer sum of v[0 .. N) over the workgroup (exact: the order does not matter); every thread returns it
__device__ inline int64_t block_sum_i(const int32_t* __restrict__ v, int N, int64_t* red) {
    int64_t s = 0;
    for (int j = threadIdx.x; j < N; j += 256) s += v[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();   // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void triplet_grad_kernel(const float* __restrict__ emb, int N, int E, int mining, int soft, float grad_scale,
                                                           TrWs ws, float* __restrict__ loss_acc, float* __restrict__ demb, int train) {
    __shared__ float s_c[TR_MAX_N];
    __shared__ int64_t s_red[4];
    __shared__ float s_l[4];
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const int64_t cnt = block_sum_i(ws.cnt, N, s_red);   // HARD: V; ALL: T
    const int64_t act = block_sum_i(ws.act, N, s_red);   // A
    const int64_t norm = (mining == VM_TRIPLET_ALL && !soft) ? act : cnt;
    const float fnorm = (float)(norm > 0 ? norm : 1);
    if (train && i < N) {
        const bool bad = block_sum_i(ws.bad, N, s_red) != 0;
        for (int j = tid; j < N; j += 256) s_c[j] = ws.W[(int64_t)i * N + j] + ws.W[(int64_t)j * N + i];
        __syncthreads();
        if (tid >= E) return;
        const float ei = emb[(int64_t)i * E + tid];
        const float* col = emb + tid;
        float acc = 0.f;
#pragma unroll 8
        for (int j = 0; j < N; ++j) {
            const float c = s_c[j];
            const float t = fmaf(c, ei - col[(int64_t)j * E], acc);
            acc = c != 0.f ? t : acc;   // a row that takes no part may hold anything: it is never multiplied in
        }
        demb[(int64_t)i * E + tid] = bad ? NAN : grad_scale * (acc / fnorm);
        return;
    }
    // the means: a thread's rows ascending, the butterfly, the four waves in order
    float l = 0.f;
    for (int j = tid; j < N; j += 256) l += ws.row_loss[j];
    l = wave_sum(l);
    if ((tid & 63) == 0) s_l[tid >> 6] = l;
    __syncthreads();
    if (tid == 0) {
        loss_acc[0] = (((s_l[0] + s_l[1]) + s_l[2]) + s_l[3]) / fnorm;
        loss_acc[1] = cnt > 0 ? (float)act / (float)cnt : 0.f;
    }
}

}  // namespace vm

using namespace vm;

extern "C" int vm_triplet_loss_supported(int64_t N, int E) { return N >= 2 && N <= TR_MAX_N && E >= 1 && E <= TR_MAX_E; }

extern "C" int64_t vm_triplet_loss_workspace_bytes(int64_t N, int E, int mining) {
    (void)E;
    (void)mining;
    return N > 0 ? (N * N + 4 * N) * (int64_t)sizeof(float) : 0;
}

extern "C" int vm_triplet_loss(const float* emb, const int32_t* label, int64_t N, int E, int mining, int soft, float margin,
                               float grad_scale, int32_t* hard_pos, int32_t* hard_neg, float* loss_acc, float* demb, void* ws,
                               void* stream) {
    VM_REQUIRE(emb && label && loss_acc && ws, "vm_triplet_loss: null pointer (emb, label, loss_acc, ws)");
    VM_REQUIRE(N >= 2 && E >= 1, "vm_triplet_loss: bad sizes (N >= 2, E >= 1; got %lld, %d)", (long long)N, E);
    VM_REQUIRE(mining == VM_TRIPLET_HARD || mining == VM_TRIPLET_ALL, "vm_triplet_loss: mining must be VM_TRIPLET_HARD or VM_TRIPLET_ALL");
    VM_REQUIRE(soft == 0 || soft == 1, "vm_triplet_loss: soft must be 0 or 1");
    VM_REQUIRE(soft || (margin >= 0.f && margin < INFINITY), "vm_triplet_loss: the hinge needs a finite margin >= 0");
    if (!vm_triplet_loss_supported(N, E)) {
        set_error("vm_triplet_loss: N <= %d, E <= %d (got %lld, %d)", TR_MAX_N, TR_MAX_E, (long long)N, E);
        return VM_ERR_UNSUPPORTED;
    }
    const int train = demb != nullptr;
    const TrWs w = tr_ws(ws, N);
    hipLaunchKernelGGL(triplet_anchor_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, emb, label, (int)N, E, mining, soft, margin,
                       hard_pos, hard_neg, w, train);
    int rc = check_launch("vm_triplet_loss");
    if (rc) return rc;
    hipLaunchKernelGGL(triplet_grad_kernel, dim3(train ? (unsigned)N + 1 : 1u), dim3(256), 0, (hipStream_t)stream, emb, (int)N, E, mining, soft,
                       grad_scale, w, loss_acc, demb, train);
    return check_launch("vm_triplet_loss(grad)");
}
