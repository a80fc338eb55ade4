// Does the clock the chip holds under a dense 16-bit MFMA loop depend on the MFMA shape?  v_mfma_f32_32x32x16 against
// v_mfma_f32_16x16x32, f16 and bf16, random non-zero operands, the conv GEMM kernels' wave geometry: 256 threads, two workgroups
// per CU (two waves per SIMD), a 128 (rows) x 64 (channels) fp32 tile per wave = 128 accumulator registers, 32 of K per iteration
// (16 MFMAs of 32x32x16 or 32 of 16x16x32: the same FLOPs, the same 12 operand fragments of 16 bytes per lane).
//   hipcc --offload-arch=gfx950 -O3 mfma_shape_probe.hip -o mfma_shape_probe && ./mfma_shape_probe
// Two arms: "reg" keeps the 12 fragments in registers; "lds" re-reads all 12 with ds_read_b128 every iteration from a
// [256 + 128 rows][64 B] stage with the kernels' XOR swizzle (conflict-free for both shapes), double-buffered in registers.
// Reported per (type, arm, shape): median wall time of 5 warm launches, TFLOP/s and wave cycles per 32-deep K step (s_memtime,
// median over waves); then the 16x16x32 : 32x32x16 ratios of FLOP/s and of cycles.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

template <typename T> struct M;
template <> struct M<__bf16> {
    using V8 = bf16x8;
    __device__ static f32x16 run32(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c, 0, 0, 0);
    }
    __device__ static f32x4 run16(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c, 0, 0, 0);
    }
};
template <> struct M<_Float16> {
    using V8 = f16x8;
    __device__ static f32x16 run32(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c, 0, 0, 0);
    }
    __device__ static f32x4 run16(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c, 0, 0, 0);
    }
};

constexpr int A_ROWS = 256, B_ROWS = 128, ROW_B = 64, STAGE = (A_ROWS + B_ROWS) * ROW_B;  // 24 KB
constexpr int BLOCKS = 512;

#define DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
// the wait names the twelve fragments, so no MFMA that reads them is scheduled above it
#define WAIT12(a, b)                                                                                                          \
    asm volatile("s_waitcnt lgkmcnt(0)"                                                                                      \
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(b[0]), \
                   "+v"(b[1]), "+v"(b[2]), "+v"(b[3]))

// SHAPE 32: a[2 i + ks] = rows 32 i + (l & 31) of the wave's 128, chunk 2 ks + (l >> 5); b[2 j + ks] likewise of its 64 channels.
// SHAPE 16: a[i] = rows 16 i + (l & 15), chunk l >> 4; b[j] likewise.  Byte address: row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4).
template <int SHAPE>
struct Addr {
    uint32_t a0, a1, b0, b1;   // SHAPE 16 uses a0 / b0 only
    __device__ Addr(int lane, int wm, int wn) {
        if (SHAPE == 32) {
            const int r = lane & 31, kh = lane >> 5, ra = wm * 128 + r, rb = A_ROWS + wn * 64 + r;
            a0 = ra * ROW_B + (((0 + kh) ^ ((ra >> 2) & 3)) << 4);
            a1 = ra * ROW_B + (((2 + kh) ^ ((ra >> 2) & 3)) << 4);
            b0 = rb * ROW_B + (((0 + kh) ^ ((rb >> 2) & 3)) << 4);
            b1 = rb * ROW_B + (((2 + kh) ^ ((rb >> 2) & 3)) << 4);
        } else {
            const int r = lane & 15, q = lane >> 4, ra = wm * 128 + r, rb = A_ROWS + wn * 64 + r;
            a0 = a1 = ra * ROW_B + ((q ^ ((ra >> 2) & 3)) << 4);
            b0 = b1 = rb * ROW_B + ((q ^ ((rb >> 2) & 3)) << 4);
        }
    }
};

template <int SHAPE>
__device__ inline void read12(u32x4 (&a)[8], u32x4 (&b)[4], const Addr<SHAPE>& ad) {
    if (SHAPE == 32) {
        DSR(a[0], ad.a0, 0);    DSR(a[1], ad.a1, 0);    DSR(a[2], ad.a0, 2048); DSR(a[3], ad.a1, 2048);
        DSR(a[4], ad.a0, 4096); DSR(a[5], ad.a1, 4096); DSR(a[6], ad.a0, 6144); DSR(a[7], ad.a1, 6144);
        DSR(b[0], ad.b0, 0);    DSR(b[1], ad.b1, 0);    DSR(b[2], ad.b0, 2048); DSR(b[3], ad.b1, 2048);
    } else {
        DSR(a[0], ad.a0, 0);    DSR(a[1], ad.a0, 1024); DSR(a[2], ad.a0, 2048); DSR(a[3], ad.a0, 3072);
        DSR(a[4], ad.a0, 4096); DSR(a[5], ad.a0, 5120); DSR(a[6], ad.a0, 6144); DSR(a[7], ad.a0, 7168);
        DSR(b[0], ad.b0, 0);    DSR(b[1], ad.b0, 1024); DSR(b[2], ad.b0, 2048); DSR(b[3], ad.b0, 3072);
    }
}

// 128 accumulator registers either way
template <int SHAPE> struct Acc;
template <> struct Acc<32> { f32x16 v[4][2]; };
template <> struct Acc<16> { f32x4 v[8][4]; };

template <typename T>
__device__ inline void mma(Acc<32>& c, const u32x4 (&a)[8], const u32x4 (&b)[4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) c.v[i][j] = M<T>::run32(b[2 * j + ks], a[2 * i + ks], c.v[i][j]);
}
template <typename T>
__device__ inline void mma(Acc<16>& c, const u32x4 (&a)[8], const u32x4 (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c.v[i][j] = M<T>::run16(b[j], a[i], c.v[i][j]);
}

// iters counts PAIRS of 32-deep K steps
template <typename T, int SHAPE, bool LDS>
__global__ __launch_bounds__(256, 2) void shape_kernel(float* __restrict__ sink, unsigned long long* __restrict__ cyc, int iters) {
    __shared__ __attribute__((aligned(16))) char stage[STAGE];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    // dense operands of ordinary magnitude: exponent near 1.0, random sign and fraction bits (zeros would clock higher)
    const uint32_t base = std::is_same<T, __bf16>::value ? 0x3F003F00u : 0x38003800u;
    for (int i = tid; i < STAGE / 4; i += 256) {
        uint32_t h = (uint32_t)(i * 2654435761u + blockIdx.x * 97u);
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        reinterpret_cast<uint32_t*>(stage)[i] = base | (h & 0x80FF80FFu);
    }
    __syncthreads();
    Acc<SHAPE> c;
    if (SHAPE == 32) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) reinterpret_cast<f32x16*>(&c)[i][e] = 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) reinterpret_cast<f32x4*>(&c)[i][e] = 0.f;
    }
    const Addr<SHAPE> ad(lane, wm, wn);
    u32x4 a0[8], b0[4], a1[8], b1[4];
    read12<SHAPE>(a0, b0, ad);
    WAIT12(a0, b0);
    read12<SHAPE>(a1, b1, ad);
    WAIT12(a1, b1);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        if (LDS) {
            read12<SHAPE>(a1, b1, ad);
            mma<T>(c, a0, b0);
            WAIT12(a1, b1);
            read12<SHAPE>(a0, b0, ad);
            mma<T>(c, a1, b1);
            WAIT12(a0, b0);
        } else {
            mma<T>(c, a0, b0);
            mma<T>(c, a1, b1);
        }
    }
    float t = 0.f;
    if (SHAPE == 32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) t += reinterpret_cast<f32x16*>(&c)[i][0] + reinterpret_cast<f32x16*>(&c)[i][15];
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) t += reinterpret_cast<f32x4*>(&c)[i][0] + reinterpret_cast<f32x4*>(&c)[i][3];
    }
    asm volatile("" : "+v"(t));   // the accumulators are complete before the second stamp
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 4 + w] = t1 - t0;
    if (t == 123.456f) sink[blockIdx.x * 256 + tid] = t;   // never true: keeps the chain alive
}

static float* d_sink;
static unsigned long long* d_cyc;
static hipEvent_t e0, e1;

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));              \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

struct Result { double ms, tflops, cyc_per_iter; };

template <typename T, int SHAPE, bool LDS>
static Result run(int iters) {
    const double flop = (double)BLOCKS * 4 * iters * 2 * (2.0 * 128 * 64 * 32);
    std::vector<float> ms(5);
    for (int rep = -3; rep < 5; ++rep) {   // three warm launches of this very kernel, then five timed
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL((shape_kernel<T, SHAPE, LDS>), dim3(BLOCKS), dim3(256), 0, 0, d_sink, d_cyc, iters);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float t;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 0) ms[rep] = t;
    }
    std::sort(ms.begin(), ms.end());
    std::vector<unsigned long long> h(BLOCKS * 4);
    CHECK(hipMemcpy(h.data(), d_cyc, h.size() * 8, hipMemcpyDeviceToHost));   // of the last launch
    std::sort(h.begin(), h.end());
    Result r;
    r.ms = ms[2];
    r.tflops = flop / (r.ms * 1e-3) / 1e12;
    r.cyc_per_iter = (double)h[h.size() / 2] / (2.0 * iters);   // per 32-deep K step
    return r;
}

template <typename T>
static void sweep(const char* tname, int iters) {
    for (int arm = 0; arm < 2; ++arm) {
        const Result r32 = arm ? run<T, 32, true>(iters) : run<T, 32, false>(iters);
        const Result r16 = arm ? run<T, 16, true>(iters) : run<T, 16, false>(iters);
        const Result again = arm ? run<T, 32, true>(iters) : run<T, 32, false>(iters);   // the first shape once more: drift of the box
        const char* an = arm ? "lds" : "reg";
        printf("%-5s %s  32x32x16  %7.3f ms  %7.1f TFLOP/s  %7.1f cyc/kstep\n", tname, an, r32.ms, r32.tflops, r32.cyc_per_iter);
        printf("%-5s %s  16x16x32  %7.3f ms  %7.1f TFLOP/s  %7.1f cyc/kstep\n", tname, an, r16.ms, r16.tflops, r16.cyc_per_iter);
        printf("%-5s %s  32x32x16  %7.3f ms  %7.1f TFLOP/s  %7.1f cyc/kstep  (repeat)\n", tname, an, again.ms, again.tflops, again.cyc_per_iter);
        printf("%-5s %s  ratio 16x16x32 : 32x32x16   FLOP/s %.3f   cycles %.3f\n", tname, an, r16.tflops / (0.5 * (r32.tflops + again.tflops)),
               r16.cyc_per_iter / (0.5 * (r32.cyc_per_iter + again.cyc_per_iter)));
    }
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 2400;   // pairs of K steps: about 3 ms a launch
    CHECK(hipMalloc(&d_sink, BLOCKS * 256 * 4));
    CHECK(hipMalloc(&d_cyc, BLOCKS * 4 * 8));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int warm = 0; warm < 300; ++warm)   // about a second of load: the clocks settle
        hipLaunchKernelGGL((shape_kernel<_Float16, 32, true>), dim3(BLOCKS), dim3(256), 0, 0, d_sink, d_cyc, iters);
    CHECK(hipDeviceSynchronize());
    printf("# %d blocks x 4 waves, %d K-step pairs per launch; median of 5 warm launches; wave cycles by s_memtime\n",
           BLOCKS, iters);
    for (int pass = 0; pass < 2; ++pass) {
        printf("# pass %d\n", pass);
        sweep<_Float16>("f16", iters);
        sweep<__bf16>("bf16", iters);
    }
    return 0;
}
