// n-shot k-way evaluation distances (voicemap/utils.py:159-206): per task, k class prototypes from n support
// embeddings each, distance to the query embedding, argmin.  The reference does this per task in float64 numpy
// after two predict() calls; here all tasks of an evaluation run go through one launch (fp64 accumulation).
#include "score_tile.hpp"

namespace vm {

// grid = tasks, block = 64 (one wave): lane <-> class (k <= 64 per pass, looped above that).
__global__ __launch_bounds__(64) void nshot_kernel(const float* __restrict__ query, const float* __restrict__ support, int k,
                                                   int n, int E, int dist_kind, float* __restrict__ pred,
                                                   int32_t* __restrict__ argmin_out) {
    const int64_t task = blockIdx.x;
    const float* q = query + task * E;
    const float* s = support + task * (int64_t)k * n * E;
    double best = INFINITY;
    int besti = 0x7fffffff, bestn = 0;
    for (int cb = 0; cb < k; cb += 64) {
        const int cls = cb + (int)threadIdx.x;
        double d = INFINITY;
        if (cls < k) {
            const float* sc = s + (int64_t)cls * n * E;
            if (dist_kind == VM_DIST_EUCLIDEAN) {
                double acc = 0.0;
                for (int j = 0; j < E; ++j) {
                    double mean = 0.0;
                    for (int i = 0; i < n; ++i) mean += (double)sc[i * E + j];
                    mean /= (double)n;
                    const double df = (double)q[j] - mean;
                    acc += df * df;
                }
                d = sqrt(acc);
            } else {
                // per-sample magnitudes
                double magsum = 0.0, dot = 0.0, mu2 = 0.0, q2 = 0.0;
                for (int j = 0; j < E; ++j) q2 += (double)q[j] * (double)q[j];
                for (int i = 0; i < n; ++i) {
                    double m2 = 0.0;
                    for (int j = 0; j < E; ++j) m2 += (double)sc[i * E + j] * (double)sc[i * E + j];
                    magsum += sqrt(m2);
                }
                for (int j = 0; j < E; ++j) {
                    double mu = 0.0;  // mean unit vector component
                    for (int i = 0; i < n; ++i) {
                        double m2 = 0.0;
                        for (int jj = 0; jj < E; ++jj) m2 += (double)sc[i * E + jj] * (double)sc[i * E + jj];
                        mu += (double)sc[i * E + j] / sqrt(m2);
                    }
                    mu /= (double)n;
                    dot += (double)q[j] * mu;
                    mu2 += mu * mu;
                }
                if (dist_kind == VM_DIST_COSINE) {
                    d = 1.0 - dot / (sqrt(q2) * sqrt(mu2));
                } else {
                    d = -(dot * (magsum / (double)n));
                }
            }
            pred[task * k + cls] = (float)d;
        }
        // wave argmin, first minimum wins; a NaN distance orders below everything, like numpy.argmin (utils.py:200 takes
        // np.argmin of the distances: the first NaN if there is one)
        double dv = (cls < k && d != d) ? -INFINITY : d;
        int dn = (cls < k && d != d) ? 1 : 0;
        int di = cls < k ? cls : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(dv, o, 64);
            const int on = __shfl_xor(dn, o, 64);
            const int oi = __shfl_xor(di, o, 64);
            if (on > dn || (on == dn && (od < dv || (od == dv && oi < di)))) {
                dv = od;
                dn = on;
                di = oi;
            }
        }
        if (dn > bestn || (dn == bestn && (dv < best || (dv == best && di < besti)))) {
            best = dv;
            bestn = dn;
            besti = di;
        }
    }
    if (threadIdx.x == 0) argmin_out[task] = besti;
}

}  // namespace vm

using namespace vm;

extern "C" int vm_nshot_distances(const float* query, const float* support, int64_t tasks, int k, int n, int E, int dist_kind,
                                  float* pred, int32_t* argmin, void* stream) {
    VM_REQUIRE(query && support && pred && argmin, "vm_nshot_distances: null pointer");
    VM_REQUIRE(tasks > 0 && k > 0 && n > 0 && E > 0, "vm_nshot_distances: bad sizes");
    VM_REQUIRE(dist_kind >= VM_DIST_EUCLIDEAN && dist_kind <= VM_DIST_DOT,
               "vm_nshot_distances: Distance must be in (euclidean, cosine, dot_product)");
    hipLaunchKernelGGL(nshot_kernel, dim3((unsigned)tasks), dim3(64), 0, (hipStream_t)stream, query, support, k, n, E, dist_kind,
                       pred, argmin);
    return check_launch("vm_nshot_distances");
}

// ------------------------------------------------------------------------------------------------------------------------------
// Batched evaluation over a CACHED embedding matrix (SURVEY 8f.2 / BASELINE.json config 5: "batched embedding forward +
// pairwise-distance matrix over train-clean-360, sharded").  The reference embeds k*n + 1 windows per task with two predict()
// calls (voicemap/utils.py:121-212, experiments/k_way_accuracy.py:52-69); with an evaluation set whose crops are deterministic
// (stochastic=False, the reference's validation datasets) every file has ONE embedding, so the corpus is embedded once into an
// (N, E) fp32 matrix and a task is k*n + 1 row indices.
// ------------------------------------------------------------------------------------------------------------------------------
namespace vm {

constexpr int NSI_MAX_EL = 4;  // elements of an embedding per lane: E <= 256

// vm_nshot_indexed: one wave per task, lane <-> embedding component(s); the arithmetic of voicemap/utils.py:159-206 in float64
// (per-class mean of the support embeddings -> L2; mean of the unit vectors -> cosine; mean magnitude x mean unit vector -> negative
// dot product), the rows gathered from the cached matrix by index.
__global__ __launch_bounds__(256) void nshot_indexed_kernel(const float* __restrict__ emb, int64_t n_rows, const int32_t* __restrict__ query_idx,
                                                            const int32_t* __restrict__ support_idx, int64_t tasks, int k, int n, int E,
                                                            int dist_kind, float* __restrict__ pred, int32_t* __restrict__ argmin_out) {
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task >= tasks) return;
    const int EL = (E + 63) / 64;
    double q[NSI_MAX_EL];
    // an index outside [0, n_rows) never leaves the matrix: it is clamped (and the task is then simply wrong -- the host checks ranges)
    auto row_of = [&](int32_t i) { return emb + (int64_t)(i < 0 ? 0 : (i >= n_rows ? n_rows - 1 : i)) * E; };
    const float* qrow = row_of(query_idx[task]);
    double q2 = 0.0;
#pragma unroll
    for (int u = 0; u < NSI_MAX_EL; ++u) {
        const int e = lane + 64 * u;
        q[u] = (u < EL && e < E) ? (double)qrow[e] : 0.0;
        q2 += q[u] * q[u];
    }
    if (dist_kind != VM_DIST_EUCLIDEAN) q2 = wave_sum_d(q2);
    const int32_t* sidx = support_idx + task * (int64_t)k * n;
    double best = INFINITY;
    int besti = 0x7fffffff, bestn = 0;
    for (int cls = 0; cls < k; ++cls) {
        double acc[NSI_MAX_EL];
#pragma unroll
        for (int u = 0; u < NSI_MAX_EL; ++u) acc[u] = 0.0;
        double magsum = 0.0;
        for (int i = 0; i < n; ++i) {
            const float* srow = row_of(sidx[cls * n + i]);
            double v[NSI_MAX_EL], m2 = 0.0;
#pragma unroll
            for (int u = 0; u < NSI_MAX_EL; ++u) {
                const int e = lane + 64 * u;
                v[u] = (u < EL && e < E) ? (double)srow[e] : 0.0;
                m2 += v[u] * v[u];
            }
            if (dist_kind == VM_DIST_EUCLIDEAN) {
#pragma unroll
                for (int u = 0; u < NSI_MAX_EL; ++u) acc[u] += v[u];
            } else {
                const double mag = sqrt(wave_sum_d(m2));
                magsum += mag;
#pragma unroll
                for (int u = 0; u < NSI_MAX_EL; ++u) acc[u] += v[u] / mag;
            }
        }
        double d;
        if (dist_kind == VM_DIST_EUCLIDEAN) {
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < NSI_MAX_EL; ++u) {
                const double df = q[u] - acc[u] / (double)n;
                s += df * df;
            }
            d = sqrt(wave_sum_d(s));
        } else {
            double dot = 0.0, mu2 = 0.0;
#pragma unroll
            for (int u = 0; u < NSI_MAX_EL; ++u) {
                const double mu = acc[u] / (double)n;
                dot += q[u] * mu;
                mu2 += mu * mu;
            }
            dot = wave_sum_d(dot);
            mu2 = wave_sum_d(mu2);
            d = dist_kind == VM_DIST_COSINE ? 1.0 - dot / (sqrt(q2) * sqrt(mu2)) : -(dot * (magsum / (double)n));
        }
        if (lane == 0 && pred != nullptr) pred[task * k + cls] = (float)d;
        // first minimum wins; a NaN distance orders below everything, like numpy.argmin (utils.py:200)
        const int dn = d != d ? 1 : 0;
        const double dv = dn ? -INFINITY : d;
        if (dn > bestn || (dn == bestn && dv < best)) {
            best = dv;
            bestn = dn;
            besti = cls;
        }
    }
    if (lane == 0) argmin_out[task] = besti;
}

// vm_pairdist_argmin: the (M, N) distance matrix between a block of query rows and the whole reference matrix, fp32, with the
// nearest reference row per query (first minimum; the query's own row can be excluded).  The scores are score_tile_loop's
// (score_tile.hpp); the epilogue here is the distance store and the argmin.

__global__ __launch_bounds__(256) void rowsq_kernel(const float* __restrict__ x, int64_t rows, int E, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float s = 0.f;
    for (int e = lane; e < E; e += 64) s = fmaf(x[r * E + e], x[r * E + e], s);
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}

// q (M, E) -> qT: per group of 8 queries and per 4 components the 8 x 4 values back to back (128 bytes): what a wave of
// pairdist_kernel takes per component step through the SCALAR path.  [group][e4][query in group][4]; rows past M / components past E: 0.
// zero_col >= 0: that component is written as zero (VM_SCORE_PLDA's row term, which the chain must skip).
__global__ __launch_bounds__(256) void pairdist_qt_kernel(const float* __restrict__ q, int64_t M, int E, int EP, int zero_col,
                                                          float* __restrict__ qT) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t groups = (M + 7) / 8;
    if (i >= groups * 8 * EP) return;
    const int c = (int)(i & 3), qi = (int)((i >> 2) & 7);
    const int64_t r = i >> 5;
    const int e4 = (int)(r % (EP / 4));
    const int64_t g = r / (EP / 4);
    const int64_t m = g * 8 + qi;
    const int e = e4 * 4 + c;
    qT[i] = (m < M && e < E && e != zero_col) ? q[m * E + e] : 0.f;
}

// out[r] = x[r][E - 1]: the row term of a PLDA-space row
__global__ __launch_bounds__(256) void rowterm_kernel(const float* __restrict__ x, int64_t rows, int E, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < rows) out[r] = x[r * E + E - 1];
}

__global__ __launch_bounds__(256) void pad_weights_kernel(const float* __restrict__ w, int E, float* __restrict__ wpad) {
    const int e = threadIdx.x;
    if (e < ST_MAX_E) wpad[e] = (w != nullptr && e < E) ? w[e] : 0.f;
}

// grid (query blocks of 64 rows, splits of the reference tiles); 512 threads; wave w owns the queries m0 + 8 w .. + 7.
template <int DIST>
__global__ __launch_bounds__(512) void pairdist_kernel(const float* __restrict__ qT, const float* __restrict__ ref, int64_t M, int64_t N,
                                                       int E, int64_t q_row0, const float* __restrict__ qsq,
                                                       const float* __restrict__ rsq, int tiles_per_split, float* __restrict__ dist,
                                                       float* __restrict__ part_val, int32_t* __restrict__ part_idx) {
    __shared__ __attribute__((aligned(16))) float rs[ST_RT * ST_RP];
    const int EP = ((E + 3) / 4) * 4, E4 = EP / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * ST_T + 8 * w;          // this wave's first query
    // its group's rows of qT (wave-uniform).  A wave past the last query (M not a multiple of 64) computes on the LAST group's rows --
    // qT holds ceil(M / 8) groups and nothing behind them -- and stores nothing (every use below is guarded by m < M).
    const int64_t last_group = (M - 1) >> 3;
    const float* qg = qT + ((m0 >> 3) < last_group ? (m0 >> 3) : last_group) * (int64_t)E4 * 32;
    float qn[8], bestv[8];
    int besti[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        qn[i] = (DIST == VM_DIST_COSINE && m0 + i < M) ? sqrtf(qsq[m0 + i]) : 1.f;
        if (DIST == VM_SCORE_PLDA) qn[i] = m0 + i < M ? plda_row_term(qsq[m0 + i]) : 0.f;
        bestv[i] = INFINITY;
        besti[i] = 0x7fffffff;
    }
    const int n_tiles = (int)((N + ST_RT - 1) / ST_RT);
    const int t_lo = blockIdx.y * tiles_per_split;
    const int t_hi = min(n_tiles, t_lo + tiles_per_split);
    score_tile_loop<DIST>(rs, qg, ref, N, E, nullptr, t_lo, t_hi, [&](int64_t n0, const float (&acc)[8][2]) {
        float rn[2] = {1.f, 1.f};
        if (DIST == VM_DIST_COSINE) {
#pragma unroll
            for (int j = 0; j < 2; ++j) rn[j] = sqrtf(n0 + lane + 64 * j < N ? rsq[n0 + lane + 64 * j] : 1.f);
        }
        if (DIST == VM_SCORE_PLDA) {
#pragma unroll
            for (int j = 0; j < 2; ++j) rn[j] = n0 + lane + 64 * j < N ? rsq[n0 + lane + 64 * j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // ascending reference index within a lane: the first minimum is kept
            const int64_t nn = n0 + lane + 64 * j;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t m = m0 + i;
                float d;
                if (DIST == VM_DIST_EUCLIDEAN) {
                    d = sqrtf(acc[i][j]);
                } else if (DIST == VM_DIST_COSINE) {
                    d = 1.f - acc[i][j] / (qn[i] * rn[j]);
                } else if (DIST == VM_SCORE_PLDA) {
                    d = plda_finish(qn[i], rn[j], acc[i][j]);
                } else {
                    d = -acc[i][j];
                }
                if (dist != nullptr && m < M && nn < N) dist[m * N + nn] = d;   // a wave = 256 contiguous bytes of a row
                if (nn < N && m < M && (q_row0 < 0 || nn != q_row0 + m) && d < bestv[i]) {
                    bestv[i] = d;
                    besti[i] = (int)nn;
                }
            }
        }
    });
    // a lane's minimum is the first in ITS references; across lanes the smaller index wins a tie
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float bv = bestv[i];
        int bi = besti[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov < bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0 && m0 + i < M) {
            part_val[(int64_t)blockIdx.y * M + m0 + i] = bv;
            part_idx[(int64_t)blockIdx.y * M + m0 + i] = bi;
        }
    }
}

__global__ __launch_bounds__(256) void pairdist_final_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx,
                                                             int64_t M, int splits, float* __restrict__ best_val,
                                                             int32_t* __restrict__ best_idx) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float bv = INFINITY;
    int bi = 0x7fffffff;
    for (int s = 0; s < splits; ++s) {  // splits cover ascending reference ranges: strict < keeps the first minimum
        const float v = part_val[(int64_t)s * M + m];
        if (v < bv) {
            bv = v;
            bi = part_idx[(int64_t)s * M + m];
        }
    }
    best_val[m] = bv;
    best_idx[m] = bi == 0x7fffffff ? -1 : bi;
}

// launchers of the preparation kernels for the other scorers (declared in score_tile.hpp)
void launch_rowsq(const float* x, int64_t rows, int E, float* out, hipStream_t st) {
    hipLaunchKernelGGL(rowsq_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, rows, E, out);
}
void launch_pairdist_qt(const float* q, int64_t M, int E, float* qT, hipStream_t st, int zero_col) {
    const int EP = ((E + 3) / 4) * 4;
    const int64_t qt_n = ((M + 7) / 8) * 8 * (int64_t)EP;
    hipLaunchKernelGGL(pairdist_qt_kernel, dim3((unsigned)((qt_n + 255) / 256)), dim3(256), 0, st, q, M, E, EP, zero_col, qT);
}
void launch_rowterm(const float* x, int64_t rows, int E, float* out, hipStream_t st) {
    hipLaunchKernelGGL(rowterm_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, x, rows, E, out);
}

void launch_pad_weights(const float* w, int E, float* wpad, hipStream_t st) {
    hipLaunchKernelGGL(pad_weights_kernel, dim3(1), dim3(256), 0, st, w, E, wpad);
}

}  // namespace vm

extern "C" int vm_nshot_indexed(const float* emb, int64_t n_rows, const int32_t* query_idx, const int32_t* support_idx, int64_t tasks,
                                int k, int n, int E, int dist_kind, float* pred, int32_t* argmin, void* stream) {
    VM_REQUIRE(emb && query_idx && support_idx && argmin, "vm_nshot_indexed: null pointer");
    VM_REQUIRE(tasks > 0 && k > 0 && n > 0 && E > 0 && n_rows > 0, "vm_nshot_indexed: bad sizes");
    VM_REQUIRE(E <= 64 * vm::NSI_MAX_EL, "vm_nshot_indexed: embedding dimension %d > %d", E, 64 * vm::NSI_MAX_EL);
    VM_REQUIRE(dist_kind >= VM_DIST_EUCLIDEAN && dist_kind <= VM_DIST_DOT,
               "vm_nshot_indexed: Distance must be in (euclidean, cosine, dot_product)");
    VM_REQUIRE((tasks + 3) / 4 < (1LL << 31), "vm_nshot_indexed: too many tasks for one launch");
    hipLaunchKernelGGL(vm::nshot_indexed_kernel, dim3((unsigned)((tasks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, emb, n_rows, query_idx,
                       support_idx, tasks, k, n, E, dist_kind, pred, argmin);
    return vm::check_launch("vm_nshot_indexed");
}

extern "C" int64_t vm_pairdist_workspace_bytes(int64_t M, int64_t N) {
    if (M <= 0 || N <= 0) return 0;
    // partial minima per split, the two squared-norm vectors, and the scalar-path copy of the queries (8-row groups x up to ST_MAX_E)
    return (int64_t)vm::score_splits(M, N, 2048) * M * 8 + (M + N) * 4 + 256 + ((M + 7) / 8) * 8 * (int64_t)vm::ST_MAX_E * 4 + 256;
}

extern "C" int vm_pairdist_argmin(const float* q, const float* ref, int64_t M, int64_t N, int E, int dist_kind, int64_t q_row0,
                                  float* dist, float* best_val, int32_t* best_idx, void* ws, void* stream) {
    using namespace vm;
    VM_REQUIRE(q && ref && best_val && best_idx && ws, "vm_pairdist_argmin: null pointer");
    VM_REQUIRE(M > 0 && N > 0 && E > 0 && E <= ST_MAX_E, "vm_pairdist_argmin: bad sizes (E <= %d)", ST_MAX_E);
    VM_REQUIRE(N < (1LL << 31) && (M + ST_T - 1) / ST_T < (1LL << 31), "vm_pairdist_argmin: matrix too large for one launch");
    VM_REQUIRE((dist_kind >= VM_DIST_EUCLIDEAN && dist_kind <= VM_DIST_DOT) || dist_kind == VM_SCORE_PLDA,
               "vm_pairdist_argmin: Distance must be in (euclidean, cosine, dot_product, plda)");
    VM_REQUIRE(plda_width_ok(dist_kind, E), "vm_pairdist_argmin: VM_SCORE_PLDA needs E %% 4 == 0 and E >= 4");
    const int splits = score_splits(M, N, 2048);
    float* part_val = (float*)ws;
    int32_t* part_idx = (int32_t*)(part_val + (int64_t)splits * M);
    float* qsq = (float*)(part_idx + (int64_t)splits * M);
    float* rsq = qsq + M;
    hipStream_t st = (hipStream_t)stream;
    if (dist_kind == VM_DIST_COSINE) {
        hipLaunchKernelGGL(rowsq_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, q, M, E, qsq);
        hipLaunchKernelGGL(rowsq_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, ref, N, E, rsq);
    } else if (dist_kind == VM_SCORE_PLDA) {
        launch_rowterm(q, M, E, qsq, st);
        launch_rowterm(ref, N, E, rsq, st);
    }
    // the scalar-path copy of the queries behind the squared norms (16-byte aligned)
    float* qT = (float*)(((uintptr_t)(rsq + N) + 255) & ~(uintptr_t)255);
    launch_pairdist_qt(q, M, E, qT, st, dist_kind == VM_SCORE_PLDA ? E - 1 : -1);
    const int n_tiles = (int)((N + ST_RT - 1) / ST_RT);
    const int tps = (n_tiles + splits - 1) / splits;
    VM_REQUIRE((E & 3) != 0 || (((uintptr_t)ref) & 15) == 0, "vm_pairdist_argmin: ref must be 16-byte aligned when E %% 4 == 0");
    const dim3 grid((unsigned)((M + ST_T - 1) / ST_T), (unsigned)splits);
#define VM_PD(D) hipLaunchKernelGGL(pairdist_kernel<D>, grid, dim3(512), 0, st, qT, ref, M, N, E, q_row0, qsq, rsq, tps, dist, part_val, part_idx)
    if (dist_kind == VM_DIST_EUCLIDEAN) VM_PD(VM_DIST_EUCLIDEAN);
    else if (dist_kind == VM_DIST_COSINE) VM_PD(VM_DIST_COSINE);
    else if (dist_kind == VM_SCORE_PLDA) VM_PD(VM_SCORE_PLDA);
    else VM_PD(VM_DIST_DOT);
#undef VM_PD
    hipLaunchKernelGGL(pairdist_final_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, part_val, part_idx, M, splits, best_val,
                       best_idx);
    return check_launch("vm_pairdist_argmin");
}
