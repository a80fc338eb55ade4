// VBx: variational-Bayes HMM diarization over PLDA-space rows (voicemap_amd/diarization.py vbx; Landini et al., "Bayesian HMM clustering
// of x-vector sequences", 2022).  The windows of R recordings lie back to back in rows (N, P), PLDA-space rows of which the columns
// w = 0 .. D - 1 are read; every recording is a Bayesian HMM of its own whose states are speakers, whose state distributions come from
// the two-covariance model in the diagonalised space (within covariance I, between covariance diag(psi)), and which is iterated by
// variational Bayes from given (or label-made) posteriors.  voicemap_amd/diarization.py vbx_reference is the numpy statement of the
// contract (include/voicemap_hip.h): the same sums in the same order, so the two differ by the exp and log routines and nothing else.
//
// Two launches on one stream: vbx_rowterm_kernel over all N rows (G_t, one thread per row), then vbx_kernel, one workgroup of 256
// threads per recording, which runs the whole loop.  Per iteration:
//   speaker posteriors  the K D sums F_kd and the K sums N_k are an index space dealt to the 256 threads; each is a chain over ascending
//                       t in a register.  They are turned into alpha in place in LDS (K x (D + 1) float64: lanes that read different
//                       speakers of one component hit different banks); thread k then forms q_k and ent_k over ascending d.
//   emissions           thread (t, k) of an n x K index space: an fma chain over ascending d against alpha in LDS; then thread t takes
//                       the row maximum m_t and replaces lp by p = exp(lp - m_t).
//   forward / backward  wave 0, lane k = speaker k: a step is one product-sum per lane, one wave-wide sum (a butterfly over the next
//                       power of two >= K, its first four stages DPP moves: every lane ends with the same bits) and one division.
//                       p is fetched eight rows ahead, c and the chain starts 64 rows at a time, so no load waits inside the
//                       recurrence.  No exp, no log.
//   the rest            wave 0: pi' over ascending t, lane k.  Waves 1 .. 3: gamma = a b, the first maximum of every row, and
//                       log c_t + m_t per row; thread 0 then adds those in ascending t.
// What bounds the loops: n, K, iters are workgroup-uniform; every __syncthreads() is reached by all 256 threads (the only early exits
// are taken by the whole workgroup, on values every thread reads from the same word).  A table the caller should have refused leaves
// iters_run = -1 and touches nothing else.  Every product, sum and quotient is rounded on its own unless it is written as fma.
#include "common.hpp"

#pragma clang fp contract(off)

namespace vm {

constexpr int VB_THREADS = 256, VB_MAX_K = VM_VBX_MAX_K, VB_MAX_ITERS = 64, VB_MAX_D = 255;
static_assert(VB_MAX_K == 64, "a forward / backward step is one lane per speaker of one wave");

struct VbxScratch {
    double* G;   // N: -1/2 (|z_t|^2 + D log 2 pi)
    double* c;   // N: the forward scales
    double* m;   // N: the row maxima of lp, then log c_t + m_t
    double* p;   // em_total: lp, then exp(lp - m_t)
    double* a;   // em_total
    double* b;   // em_total
};

static inline int64_t vb_pad(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

static VbxScratch vb_scratch(void* ws, int64_t N, int64_t em_total) {
    VbxScratch s;
    char* q = (char*)ws;
    s.G = (double*)q;
    q += vb_pad(N * 8);
    s.c = (double*)q;
    q += vb_pad(N * 8);
    s.m = (double*)q;
    q += vb_pad(N * 8);
    s.p = (double*)q;
    q += vb_pad(em_total * 8);
    s.a = (double*)q;
    q += vb_pad(em_total * 8);
    s.b = (double*)q;
    return s;
}

// One DPP move of a double (two 32-bit halves); CTRL: quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E, row_half_mirror = 0x141,
// row_mirror = 0x140.  All lanes of the wave are active wherever this is called.
template <int CTRL>
__device__ inline double vb_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// SUM_k of the contract.  Lane k holds v_k (0 in the lanes past K); Kp = the next power of two >= K.  Stage o = 1, 2, .., Kp / 2 adds
// the lane k ^ o: an addition does not care which operand comes first, so after stage o the 2 o lanes of a group hold the same bits.
// That is why stages 4 and 8 may read the MIRRORED lane of their 8 / 16 lanes instead (7 - j lies in the other quad, 15 - j in the other
// group of 8, and all lanes there hold what lane k ^ o holds): the four stages inside a row of 16 lanes are DPP moves, no LDS crossbar.
// Lane 0's value is handed to all (the lanes from Kp on hold sums of zeros).
__device__ inline double vb_wave_sum(double v, int Kp) {
    if (Kp > 1) v = v + vb_dpp<0xB1>(v);
    if (Kp > 2) v = v + vb_dpp<0x4E>(v);
    if (Kp > 4) v = v + vb_dpp<0x141>(v);
    if (Kp > 8) v = v + vb_dpp<0x140>(v);
    if (Kp > 16) v = v + __shfl_xor(v, 16, 64);
    if (Kp > 32) v = v + __shfl_xor(v, 32, 64);
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__device__ inline double vb_inv_l(double Fr, double Nk, double psi) { return 1.0 / (1.0 + (Fr * Nk) * psi); }

// grid = ceil(N / 256): G_t of every row
__global__ __launch_bounds__(256) void vbx_rowterm_kernel(const float* __restrict__ rows, int64_t N, int P, int D,
                                                          const double* __restrict__ ib, double dlog2pi, double* __restrict__ G) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const float* x = rows + t * P;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
        const double w = (double)x[d];
        acc = fma(ib[d], w * w, acc);   // w * w is exact: w is an fp32 value
    }
    G[t] = -0.5 * (acc + dlog2pi);
}

// grid = recordings; VB_THREADS threads; dynamic LDS: VB_MAX_K * (D + 1) doubles.  gamma, pi and the workspace are read AND written (no
// __restrict__: every phase reads what the last one stored; __syncthreads() orders them inside the workgroup).
__global__ __launch_bounds__(VB_THREADS) void vbx_kernel(const float* __restrict__ rows, int64_t N, int P, int D,
                                                         const int64_t* __restrict__ row0, const int64_t* __restrict__ em0, int64_t em_total,
                                                         const int32_t* __restrict__ n_models, const int32_t* __restrict__ labels_in,
                                                         const int32_t* __restrict__ chain_start, const double* __restrict__ psi_g,
                                                         const double* __restrict__ r_g, double loop_prob, double fa, double fb,
                                                         double q0, double epsilon, int iters, const double* __restrict__ gamma_in,
                                                         const double* __restrict__ pi_in, int32_t* __restrict__ labels_out, double* gamma_all,
                                                         double* pi_all, double* __restrict__ elbo_all, int32_t* __restrict__ iters_run,
                                                         const double* __restrict__ G_all, double* c_all, double* m_all, double* p_all,
                                                         double* a_all, double* b_all) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* A = reinterpret_cast<double*>(smem);   // K x (D + 1): F, then alpha
    __shared__ double rs[VB_MAX_D + 1], psis[VB_MAX_D + 1];
    __shared__ double Nk[VB_MAX_K], qk[VB_MAX_K], entk[VB_MAX_K], pis[VB_MAX_K], pinew[VB_MAX_K];
    __shared__ double elbo_now;
    __shared__ int degenerate;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int LD = D + 1;
    const int64_t lo = row0[r], n64 = row0[r + 1] - lo;
    const int64_t e_lo = em0[r], e_n = em0[r + 1] - e_lo;
    const int K = n_models[r];
    // workgroup-uniform: every thread reads the same words
    if (n64 == 0) {
        if (tid == 0) iters_run[r] = 0;
        return;
    }
    if (K < 1 || K > VB_MAX_K || lo < 0 || n64 < 0 || lo + n64 > N || e_lo < 0 || e_n != n64 * K || e_lo + e_n > em_total) {
        if (tid == 0) iters_run[r] = -1;
        return;
    }
    const int n = (int)n64;   // N < 2^31
    const float* x = rows + lo * P;
    const double* G = G_all + lo;
    double* c = c_all + lo;
    double* m = m_all + lo;
    double* gam = gamma_all + e_lo;
    double* p = p_all + e_lo;
    double* a = a_all + e_lo;
    double* b = b_all + e_lo;
    double* pi_out = pi_all + (int64_t)r * VB_MAX_K;
    double* elbo = elbo_all + (int64_t)r * iters;
    const int32_t* cs = chain_start != nullptr ? chain_start + lo : nullptr;
    const int32_t* lab = labels_in + lo;
    int32_t* lab_new = labels_out + lo;
    const double inf = __longlong_as_double(0x7ff0000000000000ll), qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double Fr = fa / fb;
    int Kp = 1;   // the next power of two >= K
    while (Kp < K) Kp <<= 1;

    // ---- the start: gamma, pi, the tables, an all-NaN elbo
    for (int d = tid; d < D; d += VB_THREADS) {
        rs[d] = r_g[d];
        psis[d] = psi_g[d];
    }
    if (tid < VB_MAX_K) {
        const double v = tid < K ? (pi_in != nullptr ? pi_in[(int64_t)r * VB_MAX_K + tid] : 1.0 / (double)K) : 0.0;
        pis[tid] = v;
        pi_out[tid] = v;
    }
    for (int i = tid; i < iters; i += VB_THREADS) elbo[i] = qnan;
    {
        const double den = 1.0 + (double)(K - 1) * q0, hit = 1.0 / den, miss = q0 / den, flat = 1.0 / (double)K;
        int k = tid % K;
        for (int64_t t = tid / K; t < n;) {   // the flat index t K + k advances by VB_THREADS
            const int64_t i = t * K + k;
            if (gamma_in != nullptr) {
                gam[i] = gamma_in[e_lo + i];
            } else {
                const int32_t l = lab[t];
                gam[i] = (l >= 0 && l < K) ? (l == k ? hit : miss) : flat;
            }
            t += VB_THREADS / K;
            k += VB_THREADS % K;
            if (k >= K) {
                k -= K;
                t += 1;
            }
        }
    }
    if (tid == 0) iters_run[r] = 0;
    __syncthreads();

    double elbo_prev = 0.0;
    for (int it = 1; it <= iters; ++it) {
        // ---- speaker posteriors: F_kd and N_k, each a chain over ascending t
        for (int i = tid; i < K * D + K; i += VB_THREADS) {
            double acc = 0.0;
            if (i < K * D) {
                const int k = i / D, d = i - k * D;
                const double rd = rs[d];
                const float* xd = x + d;
                const double* g = gam + k;
#pragma unroll 4
                for (int t = 0; t < n; ++t) acc = fma(g[(int64_t)t * K], rd * (double)xd[(int64_t)t * P], acc);
                A[k * LD + d] = acc;
            } else {
                const int k = i - K * D;
                const double* g = gam + k;
#pragma unroll 4
                for (int t = 0; t < n; ++t) acc = acc + g[(int64_t)t * K];
                Nk[k] = acc;
            }
        }
        __syncthreads();
        for (int i = tid; i < K * D; i += VB_THREADS) {
            const int k = i / D, d = i - k * D;
            const double il = vb_inv_l(Fr, Nk[k], psis[d]);
            A[k * LD + d] = (Fr * il) * A[k * LD + d];
        }
        __syncthreads();
        if (tid < K) {
            double q = 0.0, ent = 0.0;
            const double nk = Nk[tid];
            for (int d = 0; d < D; ++d) {
                const double il = vb_inv_l(Fr, nk, psis[d]);   // never stored: the bits alpha was made from
                const double al = A[tid * LD + d], a2 = al * al;
                q = fma(il + a2, psis[d], q);
                ent = ent + (((log(il) - il) - a2) + 1.0);
            }
            qk[tid] = q;
            entk[tid] = ent;
        }
        __syncthreads();
        // ---- emissions: lp, then the row maximum and p = exp(lp - m_t)
        {
            int k = tid % K;
            for (int64_t t = tid / K; t < n;) {
                const float* xt = x + t * P;
                const double* al = A + k * LD;
                double acc = 0.0;
                for (int d = 0; d < D; ++d) acc = fma(rs[d] * (double)xt[d], al[d], acc);
                p[t * K + k] = fa * ((acc - 0.5 * qk[k]) + G[t]);
                t += VB_THREADS / K;
                k += VB_THREADS % K;
                if (k >= K) {
                    k -= K;
                    t += 1;
                }
            }
        }
        __syncthreads();
        for (int t = tid; t < n; t += VB_THREADS) {
            double* pt = p + (int64_t)t * K;
            double mx = pt[0];
            for (int k = 1; k < K; ++k) mx = pt[k] > mx ? pt[k] : mx;
            m[t] = mx;
            for (int k = 0; k < K; ++k) pt[k] = exp(pt[k] - mx);
        }
        if (tid == 0) degenerate = 0;
        __syncthreads();
        // ---- forward: wave 0, lane k
        if (w == 0) {
            const double pk = lane < K ? pis[lane] : 0.0;
            double ap = 0.0, nxt[8];
            bool bad = false;
            unsigned long long starts = 0ull;
#pragma unroll
            for (int j = 0; j < 8; ++j) nxt[j] = (lane < K && j < n) ? p[(int64_t)j * K + lane] : 0.0;
            for (int g0 = 0; g0 < n && !bad; g0 += 8) {
                if ((g0 & 63) == 0) {
                    const int tt = g0 + lane;
                    starts = __ballot(tt < n && (tt == 0 || (cs != nullptr && cs[tt] != 0)));
                }
                double cur[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    cur[j] = nxt[j];
                    const int tn = g0 + 8 + j;
                    nxt[j] = (lane < K && tn < n) ? p[(int64_t)tn * K + lane] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int t = g0 + j;
                    if (t < n && !bad) {   // wave-uniform
                        const double lam = ((starts >> (t & 63)) & 1ull) ? 0.0 : loop_prob;
                        const double at = cur[j] * (lam * ap + (1.0 - lam) * pk);
                        const double ct = vb_wave_sum(at, Kp);
                        if (ct > 0.0 && ct < inf) {
                            ap = at / ct;
                            if (lane < K) a[(int64_t)t * K + lane] = ap;
                            if (lane == 0) c[t] = ct;
                        } else {
                            bad = true;
                        }
                    }
                }
            }
            if (bad && lane == 0) degenerate = 1;
        }
        __syncthreads();
        if (degenerate) {   // the recording stops: the labels it came with, everything else as the last complete iteration left it
            for (int t = tid; t < n; t += VB_THREADS) lab_new[t] = lab[t];
            if (tid == 0) iters_run[r] = -2;
            return;
        }
        // ---- backward: wave 0, lane k.  Step u takes row u's p, c and chain start and gives b[u - 1].
        if (w == 0) {
            const double pk = lane < K ? pis[lane] : 0.0;
            double bc = 1.0, nxt[8], cu = 0.0;
            int su = 0;
            if (lane < K) b[(int64_t)(n - 1) * K + lane] = 1.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) nxt[j] = (lane < K && n - 1 - j >= 1) ? p[(int64_t)(n - 1 - j) * K + lane] : 0.0;
            for (int g0 = 0; g0 < n - 1; g0 += 8) {   // steps u = n - 1 - g0 - j
                if ((g0 & 63) == 0) {   // lane i: row n - 1 - g0 - i
                    const int uu = n - 1 - g0 - lane;
                    cu = uu >= 1 ? c[uu] : 1.0;
                    su = (uu >= 1 && cs != nullptr && cs[uu] != 0) ? 1 : 0;
                }
                double cur[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    cur[j] = nxt[j];
                    const int un = n - 1 - g0 - 8 - j;
                    nxt[j] = (lane < K && un >= 1) ? p[(int64_t)un * K + lane] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int u = n - 1 - g0 - j;
                    if (u >= 1) {   // wave-uniform
                        const int src = (g0 & 63) + j;
                        const double cv = __shfl(cu, src, 64);
                        const double lam = __shfl(su, src, 64) != 0 ? 0.0 : loop_prob;
                        const double pb = cur[j] * bc;
                        const double s = vb_wave_sum(pk * pb, Kp);
                        bc = (lam * pb + (1.0 - lam) * s) / cv;
                        if (lane < K) b[(int64_t)(u - 1) * K + lane] = bc;
                    }
                }
            }
        }
        __syncthreads();
        // ---- wave 0: pi'.  Waves 1 .. 3: gamma, the labels, log c_t + m_t
        if (w == 0) {
            if (lane < K) {
                const double pk = pis[lane];
                double acc = 0.0;
#pragma unroll 4
                for (int t = 0; t < n; ++t) {
                    const double lam = (t == 0 || (cs != nullptr && cs[t] != 0)) ? 0.0 : loop_prob;
                    acc = acc + ((((1.0 - lam) * pk) * p[(int64_t)t * K + lane]) * b[(int64_t)t * K + lane]) / c[t];
                }
                pinew[lane] = acc;
            }
        } else {
            for (int t = tid - 64; t < n; t += VB_THREADS - 64) {
                const double* at = a + (int64_t)t * K;
                const double* bt = b + (int64_t)t * K;
                double* gt = gam + (int64_t)t * K;
                double best = -1.0;
                int arg = 0;
                for (int k = 0; k < K; ++k) {
                    const double g = at[k] * bt[k];
                    gt[k] = g;
                    if (g > best) {   // the first maximum
                        best = g;
                        arg = k;
                    }
                }
                lab_new[t] = arg;
                m[t] = log(c[t]) + m[t];
            }
        }
        __syncthreads();
        if (tid == 0) {
            double lpx = 0.0, ent = 0.0;
#pragma unroll 8
            for (int t = 0; t < n; ++t) lpx = lpx + m[t];
            for (int k = 0; k < K; ++k) ent = ent + entk[k];
            elbo_now = lpx + (fb * 0.5) * ent;
        }
        if (tid < K) {
            double tot = 0.0;
            for (int j = 0; j < K; ++j) tot = tot + pinew[j];
            const double v = pinew[tid] / tot;
            pi_out[tid] = v;
            pis[tid] = v;   // pinew is read by the other lanes: pis is not, until the next barrier
        }
        __syncthreads();
        const double e = elbo_now;
        if (tid == 0) {
            elbo[it - 1] = e;
            iters_run[r] = it;
        }
        if (it > 1 && e - elbo_prev < epsilon) break;
        elbo_prev = e;
    }
}

}  // namespace vm

extern "C" int64_t vm_vbx_workspace_bytes(int64_t N, int D, int64_t R, int64_t em_total) {
    if (N <= 0 || D <= 0 || R <= 0 || em_total < 0) return 0;
    return 3 * vm::vb_pad(N * 8) + 3 * vm::vb_pad(em_total * 8);
}

extern "C" int vm_vbx(const float* rows, int64_t N, int P, int D, const int64_t* row0, const int64_t* em0, int64_t R, int64_t em_total,
                      const int32_t* n_models, const int32_t* labels_in, const int32_t* chain_start, const double* psi, const double* r,
                      const double* ib, double loop_prob, double fa, double fb, double init_smooth, double epsilon, int iters,
                      const double* gamma_in, const double* pi_in, int32_t* labels_out, double* gamma, double* pi, double* elbo,
                      int32_t* iters_run, void* ws, void* stream) {
    using namespace vm;
    VM_REQUIRE(N >= 0 && N < (1LL << 31) && R >= 0 && R < (1LL << 31) && D > 0 && D <= VB_MAX_D && P >= D,
               "vm_vbx: bad sizes (N < 2^31, R < 2^31, 0 < D <= %d, P >= D)", VB_MAX_D);
    VM_REQUIRE(em_total >= 0 && em_total <= N * (int64_t)VB_MAX_K, "vm_vbx: em_total must be in [0, N * %d]", VB_MAX_K);
    VM_REQUIRE(loop_prob >= 0.0 && loop_prob < 1.0, "vm_vbx: loop_prob must be in [0, 1)");
    VM_REQUIRE(fa > 0.0 && fa < __builtin_inf() && fb > 0.0 && fb < __builtin_inf(), "vm_vbx: fa and fb must be finite and > 0");
    VM_REQUIRE(init_smooth >= 0.0 && init_smooth < __builtin_inf(), "vm_vbx: init_smooth must be finite and >= 0");
    VM_REQUIRE(epsilon == epsilon, "vm_vbx: epsilon must not be NaN");
    VM_REQUIRE(iters >= 1 && iters <= VB_MAX_ITERS, "vm_vbx: iters must be in [1, %d]", VB_MAX_ITERS);
    VM_REQUIRE(row0 && em0 && n_models && iters_run, "vm_vbx: null pointer");
    if (R == 0) return 0;
    VM_REQUIRE(psi && r && ib && pi && elbo, "vm_vbx: null pointer");
    VM_REQUIRE(N == 0 || (rows && labels_in && ws), "vm_vbx: null pointer");
    VM_REQUIRE(N == 0 || (labels_out && gamma), "vm_vbx: null output pointer");
    VM_REQUIRE(labels_out == nullptr || labels_out != labels_in, "vm_vbx: labels_out must not be labels_in");
    VM_REQUIRE(gamma == nullptr || gamma != gamma_in, "vm_vbx: gamma must not be gamma_in");
    VM_REQUIRE(pi != pi_in, "vm_vbx: pi must not be pi_in");
    VM_REQUIRE((((uintptr_t)ws) & 15) == 0, "vm_vbx: ws must be 16-byte aligned");
    const size_t lds = (size_t)VB_MAX_K * (D + 1) * sizeof(double);
    VM_REQUIRE(lds + 8192 <= lds_per_block_limit(), "vm_vbx: D = %d needs more LDS than the device grants a workgroup", D);
    hipStream_t st = (hipStream_t)stream;
    const VbxScratch s = vb_scratch(ws, N, em_total);
    if (N > 0)
        hipLaunchKernelGGL(vbx_rowterm_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, rows, N, P, D, ib,
                           (double)D * 1.8378770664093453, s.G);
    hipLaunchKernelGGL(vbx_kernel, dim3((unsigned)R), dim3(VB_THREADS), lds, st, rows, N, P, D, row0, em0, em_total, n_models, labels_in,
                       chain_start, psi, r, loop_prob, fa, fb, exp(-init_smooth), epsilon, iters, gamma_in, pi_in, labels_out, gamma, pi,
                       elbo, iters_run, s.G, s.c, s.m, s.p, s.a, s.b);
    return check_launch("vm_vbx");
}
