// Viterbi resegmentation for speaker diarization (voicemap_amd/diarization.py resegment): the windows of R recordings lie back to back
// in emb (N, E), every window carries the label of a cluster of its recording (or none), and every recording is re-labelled on its own:
// one model per cluster, every window scored against every model, the label sequence decoded by a sticky HMM, the models estimated
// again from the decoded labels, a few times over.  voicemap_amd/diarization.py reseg_reference is the numpy statement of the contract
// (include/voicemap_hip.h), matched bit for bit on the decode and, on the emissions, as vm_speaker_identify is by its numpy twin.
//
// Two launches on one stream: launch_en_rownorm over all N rows (enrol.hip), then reseg_kernel, one workgroup of 256 threads per
// recording, which runs the whole loop.  Per iteration:
//   models     thread e owns component e of all K models, held in LDS as float64 (row stride E + 1: lanes that read different models
//              of one component hit different banks).  The rows are walked in ascending order; a row adds its contribution
//              (en_contrib) to the model its label names, so every model's sum is vm_speaker_sums' for that label.  The sums are then
//              turned into the models in place (en_model) and thread k takes |p_k|.
//   emissions  thread (t, k) of an n x K index space: an en_acc chain over ascending e, en_finish, NaN / no model -> +inf; stored to
//              `emis` (or to the workspace when the caller wants none).
//   decode     the chains of the recording are dealt to the 4 waves in turn.  Lane k of a wave holds c[t][k]; a step is a wave-wide
//              minimum, one ballot (the first lane holding it), one add and one select per lane.  The 64 stay / switch bits of a row
//              and j* go to the workspace (9 bytes per row); at the end of its chain the wave traces back through them, 64 rows at a
//              time, writes the new labels and counts the rows that changed.  No barrier inside the decode.
//   stop rule  the four counts are summed (integers), every thread reads the same total.
// The chains' final costs wait in the workspace at each chain's first row; wave 0 adds them in chain order at the end.
//
// What bounds the loops: n, K, iters and the chain table are workgroup- or wave-uniform; every __syncthreads() is reached by all 256
// threads (the only early exits are taken by the whole workgroup, on values every thread reads from the same word).  A table the caller
// should have refused (K out of range, row0 / em0 that do not go together) leaves iters_run = -1 and touches nothing else.
#include "enrol_score.hpp"

namespace vm {

constexpr int RS_THREADS = 256, RS_WAVES = RS_THREADS / 64, RS_MAX_K = VM_RESEG_MAX_K, RS_MAX_ITERS = 16;
static_assert(RS_MAX_K == 64, "a decode step is one lane per model of one wave");

struct ResegScratch {
    double* norm;               // N: |e_u| of every row
    unsigned long long* stay;   // N: bit k of row t = model k stayed (c[t-1][k] <= sw)
    double* fin;                // N: at a chain's first row, the chain's final minimum
    unsigned char* jstar;       // N: the first minimum of c[t-1][.]
    float* emis;                // em_total: the emissions when the caller passes none
};

static inline int64_t rs_pad(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

static ResegScratch rs_scratch(void* ws, int64_t N) {
    ResegScratch a;
    char* p = (char*)ws;
    a.norm = (double*)p;
    p += rs_pad(N * 8);
    a.stay = (unsigned long long*)p;
    p += rs_pad(N * 8);
    a.fin = (double*)p;
    p += rs_pad(N * 8);
    a.jstar = (unsigned char*)p;
    p += rs_pad(N);
    a.emis = (float*)p;
    return a;
}

__device__ inline double rs_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        v = ov < v ? ov : v;
    }
    return v;
}

// Whole wave, lane k holding c[k] (+inf in the lanes past K; never NaN): the lowest k whose c[k] equals the minimum.
__device__ inline int rs_first_min(double c, unsigned long long valid) {
    const double m = rs_wave_min(c);
    const unsigned long long hit = __ballot(c == m) & valid;
    return hit != 0ull ? (int)__builtin_ctzll(hit) : 0;
}

// grid = recordings; RS_THREADS threads; dynamic LDS: RS_MAX_K * (E + 1) doubles.  labels_out, the emissions and the workspace are
// read AND written (no __restrict__: every iteration reads what the last one stored; __syncthreads() orders them inside the workgroup).
template <int KIND>
__global__ __launch_bounds__(RS_THREADS) void reseg_kernel(const float* __restrict__ emb, int64_t N, int E, const int64_t* __restrict__ row0,
                                                           const int64_t* __restrict__ em0, int64_t em_total,
                                                           const int32_t* __restrict__ n_models, const int32_t* __restrict__ labels_in,
                                                           const int32_t* __restrict__ chain_start, double switch_cost, int iters,
                                                           int32_t* labels_out, double* __restrict__ path_cost,
                                                           int32_t* __restrict__ iters_run, int32_t* __restrict__ n_changed, float* emis_all,
                                                           const double* __restrict__ norm, unsigned long long* stay_all, double* fin_all,
                                                           unsigned char* jstar_all) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* P = reinterpret_cast<double*>(smem);   // K x (E + 1): the sums, then the models
    __shared__ double pn[RS_MAX_K], msum[RS_MAX_K];
    __shared__ int32_t count[RS_MAX_K];
    __shared__ int wchg[RS_WAVES];
    __shared__ int any_model;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int LD = E + 1;
    const int64_t lo = row0[r], n64 = row0[r + 1] - lo;
    const int64_t e_lo = em0[r], e_n = em0[r + 1] - e_lo;
    const int K = n_models[r];
    // workgroup-uniform: every thread reads the same words
    if (n64 == 0) {
        if (tid == 0) iters_run[r] = 0;
        return;
    }
    if (K < 1 || K > RS_MAX_K || lo < 0 || n64 < 0 || lo + n64 > N || e_lo < 0 || e_n != n64 * K || e_lo + e_n > em_total) {
        if (tid == 0) iters_run[r] = -1;
        return;
    }
    const int n = (int)n64;   // N < 2^31
    const float* x = emb + lo * E;
    const double* nrm = norm + lo;
    float* em = emis_all + e_lo;
    unsigned long long* stay = stay_all + lo;
    double* fin = fin_all + lo;
    unsigned char* jstar = jstar_all + lo;
    const int32_t* cs = chain_start != nullptr ? chain_start + lo : nullptr;
    int32_t* lab_new = labels_out + lo;
    const int32_t* lab = labels_in + lo;
    const unsigned long long valid = K == 64 ? ~0ull : ((1ull << K) - 1ull);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const float inff = __uint_as_float(0x7f800000u);

    for (int it = 1; it <= iters; ++it) {
        // ---- models: the sums of vm_speaker_sums, label by label, rows ascending
        for (int i = tid; i < K * LD; i += RS_THREADS) P[i] = 0.0;
        if (tid < K) {
            msum[tid] = 0.0;
            count[tid] = 0;
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const int32_t l = lab[t];
            const double nr = nrm[t];
            const double v = tid < E ? (double)x[(int64_t)t * E + tid] : 0.0;
            if (l >= 0 && l < K) {   // workgroup-uniform
                if (tid < E) P[l * LD + tid] += en_contrib<KIND>(v, nr);
                if (tid == 0) {
                    msum[l] += nr;
                    count[l] += 1;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < K * E; i += RS_THREADS) {
            const int k = i / E, e = i - k * E;
            const int32_t c = count[k];
            P[k * LD + e] = c > 0 ? en_model<KIND>(P[k * LD + e], msum[k], (double)c) : 0.0;
        }
        __syncthreads();
        if (tid < K) {
            double a = 0.0;
            for (int e = 0; e < E; ++e) a = fma(P[tid * LD + e], P[tid * LD + e], a);
            pn[tid] = __dsqrt_rn(a);
        }
        if (tid == 0) {
            int any = 0;
            for (int k = 0; k < K; ++k) any |= count[k] > 0 ? 1 : 0;
            any_model = any;
        }
        __syncthreads();
        // ---- emissions: vm_speaker_identify's score of (row t, model k), leave_one_out = 0
        int k = tid % K;
        for (int64_t t = tid / K; t < n;) {   // the flat index t K + k advances by RS_THREADS
            const int64_t i = t * K + k;
            const float* q = x + t * E;
            const double* p = P + k * LD;
            double acc = 0.0;
            for (int e = 0; e < E; ++e) acc = en_acc<KIND>(acc, (double)q[e], p[e]);
            const float d = en_finish<KIND>(acc, KIND == VM_DIST_COSINE ? nrm[t] : 1.0, KIND == VM_DIST_COSINE ? pn[k] : 1.0);
            em[i] = (count[k] > 0 && d == d) ? d : inff;
            t += RS_THREADS / K;
            k += RS_THREADS % K;
            if (k >= K) {
                k -= K;
                t += 1;
            }
        }
        __syncthreads();
        if (!any_model) {   // only at it == 1: a decode always leaves a model with a row
            for (int t = tid; t < n; t += RS_THREADS) lab_new[t] = -1;
            if (tid == 0) {
                path_cost[r] = __longlong_as_double(0x7ff8000000000000ll);
                iters_run[r] = 0;
                n_changed[r] = 0;
            }
            return;
        }
        // ---- decode: wave w takes the chains w, w + 4, ...
        int changed = 0;
        {
            int chain = -1, t0 = 0;
            bool mine = false;
            double c = inf;
            // the end of this wave's chain t0 .. t1: its first minimum, then the way back, 64 rows at a time
            auto finish = [&](int t1) {
                int cur = rs_first_min(c, valid);
                const double cend = __shfl(c, cur, 64);
                if (lane == 0) fin[t0] = cend;
                for (int hi = t1; hi >= t0; hi -= 64) {
                    const int t = hi - lane;   // lane i: row hi - i
                    unsigned long long m = 0ull;
                    int js = 0;
                    if (t > t0) {
                        m = stay[t];
                        js = jstar[t];
                    }
                    const int cnt = hi - t0 + 1 < 64 ? hi - t0 + 1 : 64;
                    int own = 0;
                    for (int i = 0; i < cnt; ++i) {
                        if (lane == i) own = cur;
                        const unsigned long long mi = __shfl(m, i, 64);
                        const int ji = __shfl(js, i, 64);
                        if (hi - i > t0) cur = ((mi >> cur) & 1ull) ? cur : ji;
                    }
                    if (t >= t0) {
                        changed += lab[t] != own ? 1 : 0;
                        lab_new[t] = own;
                    }
                }
            };
            for (int64_t base = 0; base < n; base += 64) {
                const int64_t tt = base + lane;
                const bool st = tt < n && (tt == 0 || (cs != nullptr && cs[tt] != 0));
                const unsigned long long starts = __ballot(st);
                const int cnt = n - base < 64 ? (int)(n - base) : 64;
                for (int i = 0; i < cnt; ++i) {
                    const int t = (int)base + i;
                    if ((starts >> i) & 1ull) {   // wave-uniform
                        if (mine) finish(t - 1);
                        chain += 1;
                        mine = (chain % RS_WAVES) == w;
                        t0 = t;
                        if (mine) c = lane < K ? (double)em[(int64_t)t * K + lane] : inf;
                    } else if (mine) {
                        const double ev = lane < K ? (double)em[(int64_t)t * K + lane] : inf;
                        const int j = rs_first_min(c, valid);
                        const double sw = __shfl(c, j, 64) + switch_cost;
                        const bool keep = c <= sw;   // a tie stays
                        const unsigned long long km = __ballot(keep);
                        if (lane == 0) {
                            stay[t] = km;
                            jstar[t] = (unsigned char)j;
                        }
                        c = ev + (keep ? c : sw);
                    }
                }
            }
            if (mine) finish(n - 1);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
        if (lane == 0) wchg[w] = changed;
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int q = 0; q < RS_WAVES; ++q) total += wchg[q];
        if (tid == 0) {
            n_changed[r] = total;
            iters_run[r] = it;
        }
        lab = lab_new;
        __syncthreads();   // wchg is written again in the next iteration; the new labels are read by every thread
        if (total == 0) break;
    }
    // ---- the path cost: the chains' final minima, added in chain order
    if (w == 0) {
        double pc = 0.0;
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t tt = base + lane;
            const bool st = tt < n && (tt == 0 || (cs != nullptr && cs[tt] != 0));
            const double f = st ? fin[tt] : 0.0;
            unsigned long long starts = __ballot(st);
            while (starts != 0ull) {   // wave-uniform
                const int i = (int)__builtin_ctzll(starts);
                pc = pc + __shfl(f, i, 64);
                starts &= starts - 1ull;
            }
        }
        if (lane == 0) path_cost[r] = pc;
    }
}

}  // namespace vm

extern "C" int64_t vm_reseg_workspace_bytes(int64_t N, int E, int64_t R, int64_t em_total) {
    if (N <= 0 || E <= 0 || R <= 0 || em_total < 0) return 0;
    return 3 * vm::rs_pad(N * 8) + vm::rs_pad(N) + vm::rs_pad(em_total * 4);
}

extern "C" int vm_reseg(const float* emb, int64_t N, int E, const int64_t* row0, const int64_t* em0, int64_t R, int64_t em_total,
                        const int32_t* n_models, const int32_t* labels_in, const int32_t* chain_start, int kind, double switch_cost,
                        int iters, int32_t* labels_out, double* path_cost, int32_t* iters_run, int32_t* n_changed, float* emis, void* ws,
                        void* stream) {
    using namespace vm;
    VM_REQUIRE(N >= 0 && N < (1LL << 31) && R >= 0 && R < (1LL << 31) && E > 0 && E <= EN_MAX_E,
               "vm_reseg: bad sizes (N < 2^31, R < 2^31, 0 < E <= %d)", EN_MAX_E);
    VM_REQUIRE(em_total >= 0 && em_total <= N * (int64_t)RS_MAX_K, "vm_reseg: em_total must be in [0, N * %d]", RS_MAX_K);
    VM_REQUIRE(kind != VM_SCORE_PLDA, "vm_reseg: VM_SCORE_PLDA is refused: the mean of PLDA-space rows is not a PLDA-space row "
               "(the last column is quadratic in the row)");
    VM_REQUIRE(kind >= VM_DIST_EUCLIDEAN && kind <= VM_DIST_DOT, "vm_reseg: kind must be in (euclidean, cosine, dot_product)");
    VM_REQUIRE(switch_cost >= 0.0 && switch_cost < __builtin_inf(), "vm_reseg: switch_cost must be finite and >= 0");
    VM_REQUIRE(iters >= 1 && iters <= RS_MAX_ITERS, "vm_reseg: iters must be in [1, %d]", RS_MAX_ITERS);
    VM_REQUIRE(row0 && em0 && n_models && iters_run, "vm_reseg: null pointer");
    if (R == 0) return 0;
    VM_REQUIRE(N == 0 || (emb && labels_in && ws), "vm_reseg: null pointer");
    VM_REQUIRE(N == 0 || (labels_out && path_cost && n_changed), "vm_reseg: null output pointer");
    VM_REQUIRE(labels_out == nullptr || labels_out != labels_in, "vm_reseg: labels_out must not be labels_in");
    VM_REQUIRE((((uintptr_t)ws) & 15) == 0, "vm_reseg: ws must be 16-byte aligned");
    const size_t lds = (size_t)RS_MAX_K * (E + 1) * sizeof(double);
    VM_REQUIRE(lds + 2048 <= lds_per_block_limit(), "vm_reseg: E = %d needs more LDS than the device grants a workgroup", E);
    hipStream_t st = (hipStream_t)stream;
    const ResegScratch a = rs_scratch(ws, N);
    if (N > 0) launch_en_rownorm(emb, N, E, a.norm, st);
#define VM_RS(KD)                                                                                                                     \
    hipLaunchKernelGGL(reseg_kernel<KD>, dim3((unsigned)R), dim3(RS_THREADS), lds, st, emb, N, E, row0, em0, em_total, n_models,        \
                       labels_in, chain_start, switch_cost, iters, labels_out, path_cost, iters_run, n_changed,                         \
                       emis != nullptr ? emis : a.emis, a.norm, a.stay, a.fin, a.jstar)
    if (kind == VM_DIST_EUCLIDEAN) VM_RS(VM_DIST_EUCLIDEAN);
    else if (kind == VM_DIST_COSINE) VM_RS(VM_DIST_COSINE);
    else VM_RS(VM_DIST_DOT);
#undef VM_RS
    return check_launch("vm_reseg");
}
