// Angular-margin softmax head on cosines (include/voicemap_hip.h, vm_margin_softmax): three launches, no atomics, every sum in one
// fixed order.
//   launch 1 (margin_colnorm_kernel): thread c: m_c = sqrtf(sum_t w[t][c]^2), t ascending with fmaf.
//   launch 2 (margin_row_kernel): workgroup i is row i.  e_i goes into LDS, the row of cosines into LDS (class c belongs to thread
//     c % 256: the reads of w coalesce), then the first maximum, the softmax of the un-margined row (prob), the margin at the label,
//     the logsumexp of the margined row, the row's loss term and hit, the g row (to ws and, divided by m_c, back into LDS) and the
//     row's demb (wave v takes the components t = v, v + 4, ...; a lane's classes ascending, then the xor butterfly).
//   launch 3 (margin_wgrad_kernel): workgroup (tile of 64 classes, tile of 16 components): lane = class, a wave four components;
//     rows ascending.  The last workgroup forms the two means in row order and zeroes grad_b.
#include "common.hpp"

namespace vm {

constexpr int MG_MAX_N = 4096;
constexpr int MG_MAX_S = 16384;   // the row of cosines: 64 KiB of the CU's 160 KiB LDS
constexpr int MG_MAX_E = 256;     // four components per lane
constexpr int MG_SMALL_S = 2048;  // rows up to here use the 8 KiB form of launch 2 (more workgroups per CU)

struct MgWs {   // the workspace, in this order
    float* m;          // (S)     column norms
    float* ehat;       // (N, E)  e_i / n_i (zeros for a zero row)
    float* row_loss;   // (N)
    float* row_hit;    // (N)
    float* g;          // (N, S)
    float* c;          // (N, S)  the cosines launch 3 reads
};
__host__ __device__ inline MgWs mg_ws(void* ws, int64_t N, int S, int E) {
    MgWs w;
    w.m = (float*)ws;
    w.ehat = w.m + S;
    w.row_loss = w.ehat + N * E;
    w.row_hit = w.row_loss + N;
    w.g = w.row_hit + N;
    w.c = w.g + N * S;
    return w;
}

struct MgPar {   // ANGULAR: cos_m, sin_m, th, mm rounded once from double on the host
    int kind;
    float margin, scale, cos_m, sin_m, th, mm;
};

// every thread returns the sum: the butterfly, then the four waves in order
__device__ inline float mg_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();   // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// (v, i) first by (v descending, i ascending); a NaN is never taken (comparisons only: no fmaxf, which would drop it silently elsewhere)
__device__ inline void mg_take(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ inline void mg_block_max(float& v, int& i, float* red, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mg_take(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = v;
        redi[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = red[0], i = redi[0];
    for (int w = 1; w < 4; ++w) mg_take(v, i, red[w], redi[w]);
}

__global__ __launch_bounds__(256) void margin_colnorm_kernel(const float* __restrict__ w, int S, int E, float* __restrict__ m) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= S) return;
    float ss = 0.f;
#pragma unroll 8
    for (int t = 0; t < E; ++t) {
        const float v = w[(int64_t)t * S + c];
        ss = fmaf(v, v, ss);
    }
    m[c] = sqrtf(ss);
}

template <int CAP>
__global__ __launch_bounds__(256) void margin_row_kernel(const float* __restrict__ emb, const float* __restrict__ w,
                                                         const int32_t* __restrict__ labels, int N, int S, int E, MgPar par, float grad_scale,
                                                         float* __restrict__ cosine, float* __restrict__ prob, int32_t* __restrict__ pred,
                                                         float* __restrict__ demb, MgWs ws) {
    __shared__ float s_row[CAP];   // the cosines, later g_c / m_c
    __shared__ float s_e[MG_MAX_E];
    __shared__ float s_rv[4];
    __shared__ int s_ri[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const bool train = labels != nullptr && demb != nullptr;
    // e_i and its sum of squares (every wave forms the same sum)
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < MG_MAX_E / 64; ++u) {
        const int t = lane + 64 * u;
        const float v = t < E ? emb[i * E + t] : 0.f;
        ss = fmaf(v, v, ss);
        if (wave == 0 && t < E) s_e[t] = v;
    }
    ss = wave_sum(ss);
    const float n = sqrtf(ss);
    const bool zero_row = ss == 0.f;
    __syncthreads();
    // the row of cosines and its first maximum
    float mx = -INFINITY;
    int mi = INT_MAX;
    for (int c = tid; c < S; c += 256) {
        const float* wc = w + c;
        float dot = 0.f;
#pragma unroll 8
        for (int t = 0; t < E; ++t) dot = fmaf(s_e[t], wc[(int64_t)t * S], dot);
        const float mc = ws.m[c];
        float cs = 0.f;
        if (!zero_row && mc != 0.f) {
            cs = dot / (n * mc);
            cs = cs < -1.f ? -1.f : (cs > 1.f ? 1.f : cs);   // (a NaN passes)
        }
        s_row[c] = cs;
        if (cosine) cosine[i * S + c] = cs;
        if (train) ws.c[i * S + c] = cs;
        mg_take(mx, mi, cs, c);
    }
    mg_block_max(mx, mi, s_rv, s_ri);   // (its barriers also publish s_row)
    if (mi >= S) mi = 0;                // a row without a comparable cosine
    if (pred && tid == 0) pred[i] = mi;
    if (prob) {   // (uniform) the softmax of the un-margined row
        const float zm = par.scale * mx;
        float su = 0.f;
        for (int c = tid; c < S; c += 256) su += expf(par.scale * s_row[c] - zm);
        su = mg_block_sum(su, s_rv);
        for (int c = tid; c < S; c += 256) prob[i * S + c] = expf(par.scale * s_row[c] - zm) / su;
    }
    if (labels == nullptr) return;
    const int y = labels[i];
    if (y < 0 || y >= S) {   // (uniform) the row takes no part
        if (train) {
            for (int c = tid; c < S; c += 256) ws.g[i * S + c] = 0.f;
            if (tid < E) demb[i * E + tid] = 0.f;
        }
        if (tid == 0) ws.row_loss[i] = ws.row_hit[i] = 0.f;
        return;
    }
    // the target logit
    const float cy = s_row[y];
    float cp = cy, df = 1.f;
    if (par.kind == VM_MARGIN_COSINE) {
        cp = cy - par.margin;
    } else if (par.kind == VM_MARGIN_ANGULAR) {
        if (cy > par.th) {
            float v = fmaf(-cy, cy, 1.f);
            v = v < 0.f ? 0.f : v;
            const float sin_t = sqrtf(v);
            cp = fmaf(cy, par.cos_m, -(sin_t * par.sin_m));
            df = fmaf(par.sin_m, cy / (sin_t > VM_MARGIN_SIN_FLOOR ? sin_t : VM_MARGIN_SIN_FLOOR), par.cos_m);
        } else {
            cp = cy - par.mm;
        }
    }
    const float zy = par.scale * cp;
    float zmax = -INFINITY;
    for (int c = tid; c < S; c += 256) {
        const float z = c == y ? zy : par.scale * s_row[c];
        zmax = z > zmax ? z : zmax;
    }
    int dummy = 0;
    mg_block_max(zmax, dummy, s_rv, s_ri);
    float se = 0.f;
    for (int c = tid; c < S; c += 256) se += expf((c == y ? zy : par.scale * s_row[c]) - zmax);
    const float Z = mg_block_sum(se, s_rv);
    if (tid == 0) {
        ws.row_loss[i] = logf(Z) - (zy - zmax);
        ws.row_hit[i] = mi == y ? 1.f : 0.f;
    }
    if (!train) return;
    // g row, A_i = sum_c g_ic c_ic, and g_c / m_c back into LDS (a thread rewrites only its own classes)
    const float coef = par.scale / (float)N;
    float a = 0.f;
    for (int c = tid; c < S; c += 256) {
        const float cs = s_row[c];
        const float p = expf((c == y ? zy : par.scale * cs) - zmax) / Z;
        float g = coef * (p - (c == y ? 1.f : 0.f));
        if (c == y) g *= df;
        ws.g[i * S + c] = g;
        a = fmaf(g, cs, a);
        const float mc = ws.m[c];
        s_row[c] = mc != 0.f ? g / mc : 0.f;
    }
    const float A = mg_block_sum(a, s_rv);   // (its barriers also publish s_row)
    // demb: wave v takes t = v, v + 4, ..., four of them at a time
    for (int t0 = wave; t0 < E; t0 += 16) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = lane; c < S; c += 64) {
            const float gm = s_row[c];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (t0 + 4 * b < E) acc[b] = fmaf(gm, w[(int64_t)(t0 + 4 * b) * S + c], acc[b]);   // (uniform)
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int t = t0 + 4 * b;
            const float s = wave_sum(acc[b]);
            if (lane == 0 && t < E) {
                const float eh = zero_row ? 0.f : s_e[t] / n;
                ws.ehat[i * E + t] = eh;
                demb[i * E + t] = zero_row ? 0.f : grad_scale * (fmaf(-A, eh, s) / n);
            }
        }
    }
}

constexpr int MG_TC = 64;   // launch 3: classes per workgroup (one per lane)
constexpr int MG_TT = 16;   // components per workgroup (four per wave)

__global__ __launch_bounds__(256) void margin_wgrad_kernel(const float* __restrict__ w, int N, int S, int E, float grad_scale, MgWs ws,
                                                           float* __restrict__ loss_acc, float* __restrict__ grad_w,
                                                           float* __restrict__ grad_b, int n_ct, int n_tiles) {
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x < n_tiles) {
        const int c = (blockIdx.x % n_ct) * MG_TC + lane;
        const int t0 = (blockIdx.x / n_ct) * MG_TT + wave * 4;
        if (c >= S || t0 >= E) return;
        const float* gcol = ws.g + c;
        const float* ccol = ws.c + c;
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, B = 0.f;
#pragma unroll 4
        for (int i = 0; i < N; ++i) {
            const float g = gcol[(int64_t)i * S];
            const float cs = ccol[(int64_t)i * S];
            const float* eh = ws.ehat + (int64_t)i * E + t0;
            const bool on = g != 0.f;   // a row that takes no part holds g = 0 and anything else: it is never multiplied in
            B = on ? fmaf(g, cs, B) : B;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (t0 + b < E) acc[b] = on ? fmaf(g, eh[b], acc[b]) : acc[b];
        }
        const float mc = ws.m[c];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (t0 + b < E) {
                const int64_t o = (int64_t)(t0 + b) * S + c;
                grad_w[o] = mc != 0.f ? grad_scale * (fmaf(-B, w[o] / mc, acc[b]) / mc) : 0.f;
            }
        return;
    }
    // the means: a thread's rows ascending, the butterfly, the four waves in order
    if (grad_b)
        for (int c = tid; c < S; c += 256) grad_b[c] = 0.f;
    float l = 0.f, h = 0.f;
    for (int j = tid; j < N; j += 256) {
        l += ws.row_loss[j];
        h += ws.row_hit[j];
    }
    l = wave_sum(l);
    h = wave_sum(h);
    if (lane == 0) {
        red[0][wave] = l;
        red[1][wave] = h;
    }
    __syncthreads();
    if (tid == 0) {
        loss_acc[0] = (((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / (float)N;
        loss_acc[1] = (((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) / (float)N;
    }
}

}  // namespace vm

using namespace vm;

extern "C" int vm_margin_softmax_supported(int64_t N, int S, int E) {
    return N >= 1 && N <= MG_MAX_N && S >= 2 && S <= MG_MAX_S && E >= 1 && E <= MG_MAX_E;
}

extern "C" int64_t vm_margin_softmax_workspace_bytes(int64_t N, int S, int E) {
    return N > 0 && S > 0 && E > 0 ? (S + N * E + 2 * N + 2 * N * S) * (int64_t)sizeof(float) : 0;
}

extern "C" int vm_margin_softmax(const float* emb, const float* w, const int32_t* labels, int64_t N, int S, int E, int kind, float margin,
                                 float scale, float grad_scale, float* cosine, float* prob, int32_t* pred, float* loss_acc, float* demb,
                                 float* grad_w, float* grad_b, void* ws, void* stream) {
    VM_REQUIRE(emb && w && ws, "vm_margin_softmax: null pointer (emb, w, ws)");
    VM_REQUIRE(N >= 1 && S >= 2 && E >= 1, "vm_margin_softmax: bad sizes (N >= 1, S >= 2, E >= 1; got %lld, %d, %d)", (long long)N, S, E);
    VM_REQUIRE(kind == VM_MARGIN_NONE || kind == VM_MARGIN_COSINE || kind == VM_MARGIN_ANGULAR,
               "vm_margin_softmax: kind must be VM_MARGIN_NONE, VM_MARGIN_COSINE or VM_MARGIN_ANGULAR");
    VM_REQUIRE(margin >= 0.f && (double)margin < 1.5707963267948966, "vm_margin_softmax: the margin must be finite with 0 <= margin < pi / 2");
    VM_REQUIRE(scale > 0.f && scale < INFINITY, "vm_margin_softmax: the scale must be finite and positive");
    VM_REQUIRE(labels == nullptr || loss_acc, "vm_margin_softmax: loss_acc required with labels");
    VM_REQUIRE(demb == nullptr || (labels && grad_w), "vm_margin_softmax: demb needs labels and grad_w");
    if (!vm_margin_softmax_supported(N, S, E)) {
        set_error("vm_margin_softmax: N <= %d, S <= %d, E <= %d (got %lld, %d, %d)", MG_MAX_N, MG_MAX_S, MG_MAX_E, (long long)N, S, E);
        return VM_ERR_UNSUPPORTED;
    }
    const double md = (double)margin;
    MgPar par;
    par.kind = kind;
    par.margin = margin;
    par.scale = scale;
    par.cos_m = (float)cos(md);
    par.sin_m = (float)sin(md);
    par.th = (float)-cos(md);
    par.mm = (float)(md * sin(md));
    const bool train = labels != nullptr && demb != nullptr;
    const MgWs s = mg_ws(ws, N, S, E);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(margin_colnorm_kernel, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, st, w, S, E, s.m);
    int rc = check_launch("vm_margin_softmax(norms)");
    if (rc) return rc;
    if (S <= MG_SMALL_S)
        hipLaunchKernelGGL(margin_row_kernel<MG_SMALL_S>, dim3((unsigned)N), dim3(256), 0, st, emb, w, labels, (int)N, S, E, par, grad_scale,
                           cosine, prob, pred, train ? demb : nullptr, s);
    else
        hipLaunchKernelGGL(margin_row_kernel<MG_MAX_S>, dim3((unsigned)N), dim3(256), 0, st, emb, w, labels, (int)N, S, E, par, grad_scale,
                           cosine, prob, pred, train ? demb : nullptr, s);
    rc = check_launch("vm_margin_softmax(rows)");
    if (rc || labels == nullptr) return rc;
    const int n_ct = (int)cdiv(S, MG_TC);
    const int n_tiles = train ? n_ct * (int)cdiv(E, MG_TT) : 0;
    hipLaunchKernelGGL(margin_wgrad_kernel, dim3((unsigned)n_tiles + 1u), dim3(256), 0, st, w, (int)N, S, E, grad_scale, s, loss_acc,
                       train ? grad_w : nullptr, train ? grad_b : nullptr, n_ct, n_tiles);
    return check_launch("vm_margin_softmax(grad_w)");
}
