// The two kernels of the PLDA back end (voicemap_amd/plda.py): the float64 scatter matrix of the fit, and the projection of rows into
// LDA / PLDA space.  Scoring PLDA-space rows is no kernel of its own: it is score kind VM_SCORE_PLDA of the scorers (score_tile.hpp).
//
// vm_scatter_f64: out = sum_r (x_r - mean)(x_r - mean)^T over the rows with label >= 0, in float64.  One pass over x: a workgroup takes one
// chunk of SC_CHUNK rows and one 64 x 64 tile of the upper triangle, stages SC_SB rows at a time in LDS as float64 differences (rounded
// once) and keeps a 4 x 4 float64 register tile per thread, an fma chain over ascending rows.  Every (chunk, tile) writes its partial
// into the workspace; a second launch sums the partials of an entry in ascending chunk order and stores it on both sides of the
// diagonal.  No float atomics: the result is a function of the inputs alone, exactly symmetric, bit-identical from run to run.
// N D^2 / 2 fma for 10^5 rows of 64 is a latency-bound fraction of a millisecond: nothing more elaborate is built.
//
// vm_plda_project: y = A (x - mean) in float64 (ascending e, fma chain), optionally scaled to length sqrt(D), stored as fp32; with
// `quad` the row becomes a PLDA-space row: zero padding up to P - 1 and the row term h in the last column.  One workgroup per block of
// PJ_RB rows: the rows sit in LDS as fp32 (transposed: a wave reads 32 consecutive rows of one component), A goes through LDS PJ_DC rows
// at a time (a wave reads two addresses per step: a broadcast), the float64 results wait in LDS for the row's norm, and the finished
// fp32 rows -- contiguous in `out` -- leave through one linear copy, 16 bytes per lane where P % 4 == 0.
#include "common.hpp"

namespace vm {

constexpr int SC_CHUNK = 512, SC_SB = 32, SC_TILE = 64;

// grid (chunks of SC_CHUNK rows, tiles ti <= tj of the upper triangle); 256 threads = 16 x 16, thread (ty, tx) owns the entries
// (ti * 64 + 4 ty + u, tj * 64 + 4 tx + v).  part (n_chunks, D, D): only entries with i <= j are written (and read).
__global__ __launch_bounds__(256) void scatter_part_kernel(const float* __restrict__ x, const int32_t* __restrict__ label,
                                                           const double* __restrict__ mean, int64_t N, int D, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double As[SC_SB][SC_TILE];
    __shared__ __attribute__((aligned(16))) double Bs[SC_SB][SC_TILE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // blockIdx.y -> (ti, tj), ti <= tj < nT, row by row of the triangle (nT <= 4: at most 10 tiles)
    const int nT = (D + SC_TILE - 1) / SC_TILE;
    int ti = 0, tj = 0, p = (int)blockIdx.y;
    for (int i = 0; i < nT; ++i) {
        if (p < nT - i) {
            ti = i, tj = i + p;
            break;
        }
        p -= nT - i;
    }
    const bool diag = ti == tj;
    const int64_t r_begin = (int64_t)blockIdx.x * SC_CHUNK;
    const int64_t r_end = r_begin + SC_CHUNK < N ? r_begin + SC_CHUNK : N;
    const int lc = tid & 63, lr = tid >> 6;
    const int colA = ti * SC_TILE + lc, colB = tj * SC_TILE + lc;
    const double mA = colA < D ? mean[colA] : 0.0, mB = colB < D ? mean[colB] : 0.0;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += SC_SB) {
        __syncthreads();   // the previous batch's readers are done
#pragma unroll
        for (int k = 0; k < SC_SB / 4; ++k) {
            const int rr = lr + 4 * k;
            const int64_t row = r0 + rr;
            // a row past the chunk or with a negative label enters as a zero difference: fma(0, 0, acc) == acc
            const bool ok = row < r_end && (label == nullptr || label[row] >= 0);
            As[rr][lc] = (ok && colA < D) ? (double)x[row * D + colA] - mA : 0.0;
            if (!diag) Bs[rr][lc] = (ok && colB < D) ? (double)x[row * D + colB] - mB : 0.0;
        }
        __syncthreads();
        const double(*Bp)[SC_TILE] = diag ? As : Bs;
#pragma unroll 4
        for (int rr = 0; rr < SC_SB; ++rr) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = As[rr][4 * ty + u];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = Bp[rr][4 * tx + v];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
    }
    double* pc = part + (int64_t)blockIdx.x * D * D;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = ti * SC_TILE + 4 * ty + u, j = tj * SC_TILE + 4 * tx + v;
            if (i < D && j < D && i <= j) pc[i * D + j] = acc[u][v];
        }
}

// one thread per entry (i, j), i <= j: the partials in ascending chunk order, stored at (i, j) and (j, i)
__global__ __launch_bounds__(256) void scatter_final_kernel(const double* __restrict__ part, int64_t n_chunks, int D,
                                                            double* __restrict__ out) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= D * D) return;
    const int i = idx / D, j = idx % D;
    if (i > j) return;
    double s = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) s += part[c * D * D + idx];
    out[i * D + j] = s;
    out[j * D + i] = s;
}

constexpr int PJ_RB = 32, PJ_DC = 16;

// |y| and the row term: float64, ascending d, every product and sum rounded on its own (what a numpy loop does)
__device__ inline double pj_add_sq(double s, double y) {
#pragma clang fp contract(off)
    const double q = y * y;
    return s + q;
}
__device__ inline double pj_add_quad(double s, double q, double v) {
#pragma clang fp contract(off)
    const double vv = v * v;   // exact: v is an fp32 value
    const double t = q * vv;
    return s + t;
}
__device__ inline double pj_scale(double y, double sd, double nrm) {
#pragma clang fp contract(off)
    const double t = y * sd;
    return t / nrm;
}

// grid = blocks of PJ_RB rows; 256 threads: thread = (row tid & 31, slot tid >> 5), a slot takes every 8th row of A.
template <int EMAX, int DMAX>
__global__ __launch_bounds__(256) void plda_project_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                           const double* __restrict__ A, int64_t N, int E, int D, int length_norm,
                                                           const double* __restrict__ quad, double c0, float* __restrict__ out, int P) {
    constexpr int XS_BYTES = EMAX * PJ_RB * 4, AS_BYTES = PJ_DC * EMAX * 8;
    static_assert(PJ_RB * (DMAX + 4) * 4 <= XS_BYTES + AS_BYTES, "the finished rows alias the staged rows and the A chunk");
    __shared__ __attribute__((aligned(16))) unsigned char smem[XS_BYTES + AS_BYTES];
    __shared__ __attribute__((aligned(16))) double ys[DMAX * PJ_RB];   // [d][row]
    __shared__ double ms[EMAX];
    __shared__ double nrm_s[PJ_RB];
    float* xs = reinterpret_cast<float*>(smem);                 // [e][row]
    double* As = reinterpret_cast<double*>(smem + XS_BYTES);    // [d in chunk][e], pitch EMAX
    float* os = reinterpret_cast<float*>(smem);                 // [row][P], once xs and As are done with
    const int tid = threadIdx.x, r = tid & (PJ_RB - 1), slot = tid >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * PJ_RB;
    const int n_valid = (int)(N - row0 < PJ_RB ? N - row0 : PJ_RB);
    // the block's rows are contiguous in x: a linear read, transposed into LDS
    for (int idx = tid; idx < PJ_RB * E; idx += 256) {
        const int rr = idx / E, e = idx - rr * E;
        xs[e * PJ_RB + rr] = rr < n_valid ? x[row0 * E + idx] : 0.f;
    }
    for (int e = tid; e < E; e += 256) ms[e] = mean[e];
    for (int dc0 = 0; dc0 < D; dc0 += PJ_DC) {
        __syncthreads();   // the previous chunk's readers are done (and, first, xs / ms are staged)
        const int nd = D - dc0 < PJ_DC ? D - dc0 : PJ_DC;
        for (int idx = tid; idx < nd * E; idx += 256) {
            const int dl = idx / E, e = idx - dl * E;
            As[dl * EMAX + e] = A[(int64_t)dc0 * E + idx];
        }
        __syncthreads();
        for (int dl = slot; dl < nd; dl += 8) {
            const double* a = As + dl * EMAX;
            double acc = 0.0;
            for (int e = 0; e < E; ++e) acc = fma(a[e], (double)xs[e * PJ_RB + r] - ms[e], acc);
            ys[(dc0 + dl) * PJ_RB + r] = acc;
        }
    }
    __syncthreads();
    if (tid < PJ_RB) {
        double ss = 0.0;
        if (length_norm)
            for (int d = 0; d < D; ++d) ss = pj_add_sq(ss, ys[d * PJ_RB + tid]);
        nrm_s[tid] = sqrt(ss);
    }
    __syncthreads();
    const double sd = sqrt((double)D);
    for (int idx = tid; idx < D * PJ_RB; idx += 256) {
        const int d = idx / PJ_RB, rr = idx - d * PJ_RB;
        double y = ys[idx];
        const double nrm = nrm_s[rr];
        if (length_norm && nrm != 0.0) y = pj_scale(y, sd, nrm);   // a zero row stays zero
        os[rr * P + d] = (float)y;
    }
    __syncthreads();
    if (quad != nullptr && tid < PJ_RB) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = pj_add_quad(s, quad[d], (double)os[tid * P + d]);   // the STORED values
        for (int d = D; d < P - 1; ++d) os[tid * P + d] = 0.f;
        os[tid * P + P - 1] = (float)(s + c0);
    }
    __syncthreads();
    float* ob = out + row0 * P;
    const int total = n_valid * P;
    if ((P & 3) == 0) {
        for (int i4 = tid; i4 < total / 4; i4 += 256) reinterpret_cast<f32x4*>(ob)[i4] = reinterpret_cast<const f32x4*>(os)[i4];
    } else {
        for (int i = tid; i < total; i += 256) ob[i] = os[i];
    }
}

}  // namespace vm

using namespace vm;

extern "C" int vm_scatter_f64_chunk_rows(void) { return SC_CHUNK; }

extern "C" int64_t vm_scatter_f64_workspace_bytes(int64_t N, int D) {
    if (N <= 0 || D <= 0) return 0;
    return cdiv(N, SC_CHUNK) * (int64_t)D * D * 8;   // one (D, D) float64 partial per chunk of rows
}

extern "C" int vm_scatter_f64(const float* x, const int32_t* label, const double* mean, int64_t N, int D, double* out, void* ws,
                              void* stream) {
    VM_REQUIRE(x && mean && out && ws, "vm_scatter_f64: null pointer");
    VM_REQUIRE(N > 0 && N < (1LL << 31) && D > 0 && D <= 256, "vm_scatter_f64: bad sizes (0 < N < 2^31, 0 < D <= 256)");
    VM_REQUIRE((((uintptr_t)mean) & 7) == 0 && (((uintptr_t)out) & 7) == 0 && (((uintptr_t)ws) & 7) == 0,
               "vm_scatter_f64: mean, out and ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_chunks = cdiv(N, SC_CHUNK);
    const int nT = (D + SC_TILE - 1) / SC_TILE;
    const dim3 grid((unsigned)n_chunks, (unsigned)(nT * (nT + 1) / 2));
    hipLaunchKernelGGL(scatter_part_kernel, grid, dim3(256), 0, st, x, label, mean, N, D, (double*)ws);
    hipLaunchKernelGGL(scatter_final_kernel, dim3((unsigned)((D * D + 255) / 256)), dim3(256), 0, st, (const double*)ws, n_chunks, D, out);
    return check_launch("vm_scatter_f64");
}

extern "C" int vm_plda_project(const float* x, const double* mean, const double* A, int64_t N, int E, int D, int length_norm,
                               const double* quad, double c0, float* out, int P, void* stream) {
    VM_REQUIRE(x && mean && A && out, "vm_plda_project: null pointer");
    VM_REQUIRE(N > 0 && N < (1LL << 31) && E > 0 && E <= 255 && D > 0 && D <= 255, "vm_plda_project: bad sizes (0 < N < 2^31, 0 < D, E <= 255)");
    VM_REQUIRE(P == (quad == nullptr ? D : 4 * ((D + 1 + 3) / 4)), "vm_plda_project: P must be D without quad, 4 ceil((D + 1) / 4) with it");
    VM_REQUIRE((((uintptr_t)mean) & 7) == 0 && (((uintptr_t)A) & 7) == 0 && (((uintptr_t)quad) & 7) == 0,
               "vm_plda_project: mean, A and quad must be 8-byte aligned");
    VM_REQUIRE((P & 3) != 0 || (((uintptr_t)out) & 15) == 0, "vm_plda_project: out must be 16-byte aligned when P %% 4 == 0");
    VM_REQUIRE(c0 - c0 == 0.0, "vm_plda_project: c0 must be finite");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(N, PJ_RB));
    if (E <= 64 && D <= 64)
        hipLaunchKernelGGL((plda_project_kernel<64, 64>), grid, dim3(256), 0, st, x, mean, A, N, E, D, length_norm, quad, c0, out, P);
    else
        hipLaunchKernelGGL((plda_project_kernel<256, 256>), grid, dim3(256), 0, st, x, mean, A, N, E, D, length_norm, quad, c0, out, P);
    return check_launch("vm_plda_project");
}
