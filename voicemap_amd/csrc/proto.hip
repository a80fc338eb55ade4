// Prototypical loss on a k-way n-shot episode (include/voicemap_hip.h, vm_proto_loss): two launches, no atomics, every sum in one
// fixed order.
//   launch 1 (proto_query_kernel): a workgroup stages the k prototypes in LDS (support rows summed in row order, divided by n) and
//     walks its queries: squared distances (each wave one class at a time, a lane's components ascending, then the xor butterfly),
//     the softmax over classes in wave 0 (registers), the query's loss term / hit and its demb row (classes ascending).
//   launch 2 (proto_support_kernel): workgroup c < k sums r[j][c] * (q_j - p_c) over the queries in row order and writes the n support
//     rows of class c; workgroup k forms the loss and accuracy means.
#include "common.hpp"

namespace vm {

constexpr int PR_MAX_K = 128;      // two classes per lane of the softmax wave
constexpr int PR_MAX_N = 16;
constexpr int PR_MAX_E = 256;      // one component per thread of a 256-thread workgroup
constexpr int PR_MAX_KE = 16384;   // the prototypes: 64 KiB of the CU's 160 KiB LDS
constexpr int PR_MAX_GRID = 1024;  // launch 1: queries beyond it are walked by the same workgroups (the prototypes are staged once)

// p[t] of class c: the n support rows in row order, then one division (what vm_nshot_distances' mean is, in fp32)
__device__ inline float proto_component(const float* __restrict__ emb, int c, int n, int E, int t) {
    const float* s = emb + ((int64_t)c * n) * E + t;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += s[(int64_t)i * E];
    return acc / (float)n;
}

__global__ __launch_bounds__(256) void proto_query_kernel(const float* __restrict__ emb, const int32_t* __restrict__ labels, int k, int n,
                                                          int64_t m, int E, float alpha, float grad_scale, float* __restrict__ logits,
                                                          float* __restrict__ demb, float* __restrict__ ws) {
    __shared__ float ps[PR_MAX_KE];   // [k][E]
    __shared__ float lg[PR_MAX_K];
    __shared__ float rs[PR_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int idx = tid; idx < k * E; idx += 256) ps[idx] = proto_component(emb, idx / E, n, E, idx % E);
    __syncthreads();
    const float coef = 2.f * alpha / (float)m;
    float* r_ws = ws;                                   // (m, k)  softmax - onehot
    float* row_loss = ws ? ws + m * k : nullptr;        // (m)
    float* row_hit = ws ? ws + m * k + m : nullptr;     // (m)
    for (int64_t j = blockIdx.x; j < m; j += gridDim.x) {
        const float* q = emb + ((int64_t)k * n + j) * E;
        float qv[PR_MAX_E / 64];
#pragma unroll
        for (int u = 0; u < PR_MAX_E / 64; ++u) qv[u] = (lane + 64 * u < E) ? q[lane + 64 * u] : 0.f;
        for (int c = wave; c < k; c += 4) {
            const float* p = ps + c * E;
            float d2 = 0.f;
#pragma unroll
            for (int u = 0; u < PR_MAX_E / 64; ++u)
                if (lane + 64 * u < E) {
                    const float d = qv[u] - p[lane + 64 * u];
                    d2 = fmaf(d, d, d2);
                }
            d2 = wave_sum(d2);
            if (lane == 0) {
                const float l = -alpha * d2;
                lg[c] = l;
                logits[j * k + c] = l;
            }
        }
        __syncthreads();
        if (labels != nullptr) {   // (uniform)
            if (wave == 0) {
                const int c1 = lane + 64;
                const float l0 = lane < k ? lg[lane] : -INFINITY, l1 = c1 < k ? lg[c1] : -INFINITY;
                float mx = l0;
                int mi = lane;
                if (l1 > mx) {   // (strictly: the lower class keeps a tie)
                    mx = l1;
                    mi = c1;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float om = __shfl_xor(mx, o, 64);
                    const int oi = __shfl_xor(mi, o, 64);
                    if (om > mx || (om == mx && oi < mi)) {
                        mx = om;
                        mi = oi;
                    }
                }
                const float e0 = lane < k ? expf(l0 - mx) : 0.f, e1 = c1 < k ? expf(l1 - mx) : 0.f;
                const float S = wave_sum(e0 + e1);
                const int y = labels[j];
                const bool ok = y >= 0 && y < k;   // a label outside [0, k): the query contributes nothing
                if (lane < k) rs[lane] = ok ? e0 / S - (lane == y ? 1.f : 0.f) : 0.f;
                if (c1 < k) rs[c1] = ok ? e1 / S - (c1 == y ? 1.f : 0.f) : 0.f;
                if (lane == 0) {
                    row_loss[j] = ok ? logf(S) - (lg[y] - mx) : 0.f;
                    row_hit[j] = (ok && mi == y) ? 1.f : 0.f;
                }
            }
            if (demb != nullptr) {
                __syncthreads();
                for (int c = tid; c < k; c += 256) r_ws[j * k + c] = rs[c];
                if (tid < E) {
                    float acc = 0.f;
                    for (int c = 0; c < k; ++c) acc = fmaf(rs[c], ps[c * E + tid], acc);
                    demb[((int64_t)k * n + j) * E + tid] = grad_scale * (coef * acc);
                }
            }
        }
        __syncthreads();   // lg / rs are rewritten by the next query
    }
}

__global__ __launch_bounds__(256) void proto_support_kernel(const float* __restrict__ emb, int k, int n, int64_t m, int E, float alpha,
                                                            float grad_scale, const float* __restrict__ ws, float* __restrict__ loss_acc,
                                                            float* __restrict__ demb, int with_grad) {
    __shared__ float red[2][4];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    if (with_grad && c < k) {
        if (tid >= E) return;
        const float pc = proto_component(emb, c, n, E, tid);
        const float* q = emb + ((int64_t)k * n) * E + tid;
        const float* r = ws + c;
        float acc = 0.f;
        for (int64_t j = 0; j < m; ++j) acc = fmaf(r[j * k], q[j * E] - pc, acc);
        const float g = grad_scale * ((2.f * alpha / (float)m) * acc / (float)n);
        for (int i = 0; i < n; ++i) demb[((int64_t)c * n + i) * E + tid] = g;
        return;
    }
    // the means: a thread's rows ascending, the butterfly, the four waves in order
    const float* row_loss = ws + m * k;
    const float* row_hit = row_loss + m;
    float l = 0.f, h = 0.f;
    for (int64_t j = tid; j < m; j += 256) {
        l += row_loss[j];
        h += row_hit[j];
    }
    l = wave_sum(l);
    h = wave_sum(h);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = l;
        red[1][tid >> 6] = h;
    }
    __syncthreads();
    if (tid == 0) {
        loss_acc[0] = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (float)m;
        loss_acc[1] = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (float)m;
    }
}

}  // namespace vm

using namespace vm;

extern "C" int vm_proto_loss_supported(int k, int n, int64_t m, int E) {
    return k >= 2 && k <= PR_MAX_K && n >= 1 && n <= PR_MAX_N && E >= 1 && E <= PR_MAX_E && (int64_t)k * E <= PR_MAX_KE && m >= 1 &&
           m < (1LL << 31);
}

extern "C" int64_t vm_proto_loss_workspace_bytes(int k, int n, int64_t m, int E) {
    (void)n;
    (void)E;
    return k > 0 && m > 0 ? (m * k + 2 * m) * (int64_t)sizeof(float) : 0;
}

extern "C" int vm_proto_loss(const float* emb, const int32_t* labels, int k, int n, int64_t m, int E, float alpha, float grad_scale,
                             float* logits, float* loss_acc, float* demb, float* ws, void* stream) {
    VM_REQUIRE(emb && logits, "vm_proto_loss: null pointer (emb, logits)");
    VM_REQUIRE(k >= 2 && n >= 1 && m >= 1 && E >= 1, "vm_proto_loss: bad sizes (k >= 2, n >= 1, m >= 1, E >= 1; got %d, %d, %lld, %d)", k, n,
               (long long)m, E);
    VM_REQUIRE(alpha > 0.f, "vm_proto_loss: alpha must be positive");
    VM_REQUIRE(labels == nullptr || (loss_acc && ws), "vm_proto_loss: loss_acc and ws (vm_proto_loss_workspace_bytes) required with labels");
    if (!vm_proto_loss_supported(k, n, m, E)) {
        set_error("vm_proto_loss: k <= %d, n <= %d, E <= %d, k * E <= %d, m < 2^31 (got %d, %d, %d, %lld)", PR_MAX_K, PR_MAX_N, PR_MAX_E,
                  PR_MAX_KE, k, n, E, (long long)m);
        return VM_ERR_UNSUPPORTED;
    }
    const bool train = labels != nullptr && demb != nullptr;
    hipLaunchKernelGGL(proto_query_kernel, dim3((unsigned)(m < PR_MAX_GRID ? m : PR_MAX_GRID)), dim3(256), 0, (hipStream_t)stream, emb, labels, k,
                       n, m, E, alpha, grad_scale, logits, train ? demb : nullptr, labels ? ws : nullptr);
    int rc = check_launch("vm_proto_loss");
    if (rc || labels == nullptr) return rc;
    hipLaunchKernelGGL(proto_support_kernel, dim3(train ? (unsigned)k + 1 : 1u), dim3(256), 0, (hipStream_t)stream, emb, k, n, m, E, alpha,
                       grad_scale, (const float*)ws, loss_acc, demb, (int)train);
    return check_launch("vm_proto_loss(support)");
}
