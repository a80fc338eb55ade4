// Speed perturbation of the resident int16 corpus: an integer polyphase resampler by the rational U / D (U output samples per D input
// samples; voicemap_amd/speed.py resample_reference is the numpy statement and is what the tests compare against, bit for bit).
// Utterance u = the lens[u] samples x[0..len-1] at audio[offsets[u]]; with n = U T taps and c = n / 2 it gives n_out = ceil(len U / D)
// samples
//   acc[m] = sum_k taps[m D + c - k U] x[k]  over the k with 0 <= k < len and 0 <= m D + c - k U < n                       (int64)
//          = sum_{i < T} taps[p + i U] x[q - i]   with q = (m D + c) / U, p = (m D + c) % U   (x = 0 outside the file)
//   y[m]   = clip((acc[m] + (1 << (shift - 1))) >> shift, -32768, 32767)     (arithmetic shift; shift = 0 adds nothing)
// at out[new_offsets[u] + m].  The outputs of all utterances form one flat list, utterance u's at [out_base[u], out_base[u + 1]); a
// fixed grid of workgroups takes an equal run of consecutive tiles of that list each and finds a tile's utterance by a binary search of
// out_base, so the utterance never sits in grid.y.  A tile is cut where an utterance ends; for each piece the workgroup stages the
// input span the piece reads (piece D / U + T samples, zeros outside the file) in LDS next to the tap table, then every thread computes
// SP_PER consecutive outputs and stores them as one 16-byte word (2-byte stores up to the destination's first 16-byte boundary and
// after its last).  The accumulator is 32 bits wide only where phase_abs_max, the caller's bound on sum_i |taps[p + i U]|, proves that
// no partial sum can leave int32 (phase_abs_max * 2^15 < 2^31), and 64 bits wide otherwise.  No atomics, no workgroup waits on
// another, every loop is bounded by an argument or a constant, nothing outside a file is read.
#include "common.hpp"

namespace vm {

constexpr int SP_T = 256;                        // threads per workgroup
constexpr int SP_GRID = 4096;                    // workgroups, an equal run of consecutive tiles each (the output total is on the device)
constexpr int SP_PER = 8;                        // consecutive outputs per thread: one 16-byte store (speed.py THREAD_OUTPUTS)
constexpr int SP_TILE = SP_T * SP_PER;           // outputs per tile at most (speed.py TILE_OUTPUTS)
constexpr int SP_SPAN = 4096;                    // input samples a piece may read: its tile shrinks until they fit (speed.py SPAN)
constexpr int SP_MAX_UD = 64, SP_MAX_T = 64, SP_MAX_SHIFT = 30;
constexpr int64_t SP_NARROW_MAX = 65535;         // phase_abs_max up to here: 32-bit accumulation is exact (speed.py NARROW_MAX)

typedef __attribute__((ext_vector_type(4))) int32_t i32x4;

// outputs per tile: the most whose input span, (tile - 1) D / U + 1 + T samples at most, fits SP_SPAN (speed.py tile_outputs)
static inline int sp_tile_outputs(int U, int D, int T) {
    int64_t t = ((int64_t)(SP_SPAN - T - 1) * U) / D;
    if (t > SP_TILE) t = SP_TILE;
    if (t >= SP_PER) t -= t % SP_PER;
    return (int)t;
}

// the utterance a workgroup last worked in (it walks CONSECUTIVE tiles: the search runs once per utterance)
struct SpUtt {
    int64_t lo, hi, off, len, dst;   // its outputs [lo, hi) of the flat list, its first sample, its length, its first output sample
};
__device__ inline void sp_locate(SpUtt& c, const int64_t* __restrict__ out_base, const int64_t* __restrict__ offsets,
                                 const int64_t* __restrict__ lens, const int64_t* __restrict__ new_offsets, int64_t n_utts, int64_t g) {
    if (g >= c.lo && g < c.hi) return;
    int64_t lo = 0, hi = n_utts;   // the largest u with out_base[u] <= g (utterances without outputs never match)
    for (int it = 0; it < 64 && hi - lo > 1; ++it) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (out_base[mid] <= g) lo = mid; else hi = mid;
    }
    c.lo = out_base[lo], c.hi = out_base[lo + 1], c.off = offsets[lo], c.len = lens[lo], c.dst = new_offsets[lo];
}

// output j of a piece: r = p0 + j D is (m D + c) less U times the piece's first q, so q - q0 = r / U and the phase is r % U; xs points at
// the staged sample x[q0] (x[q0 - i] at xs[-i])
template <bool WIDE>
__device__ inline int16_t sp_output(const int32_t* __restrict__ s_taps, const int16_t* __restrict__ xs, int r, int U, int T, int shift,
                                    int64_t rnd) {
    const int dq = (int)((unsigned)r / (unsigned)U), p = r - dq * U;
    const int32_t* __restrict__ h = s_taps + p;
    const int16_t* __restrict__ x = xs + dq;
    int64_t acc;
    if (WIDE) {
        acc = 0;
        for (int i = 0; i < T; ++i) acc += (int64_t)h[i * U] * (int64_t)x[-i];
    } else {   // |tap| <= 65535 and |x| <= 32768: 24-bit factors, and every partial sum is below 2^31
        int32_t a = 0;
        for (int i = 0; i < T; ++i) a += __mul24(h[i * U], (int)x[-i]);
        acc = a;
    }
    int64_t y = (acc + rnd) >> shift;
    y = y < -32768 ? -32768 : (y > 32767 ? 32767 : y);
    return (int16_t)y;
}

template <bool WIDE>
__global__ __launch_bounds__(SP_T) void resample_kernel(const int16_t* __restrict__ audio, const int64_t* __restrict__ offsets,
                                                        const int64_t* __restrict__ lens, const int64_t* __restrict__ out_base,
                                                        int64_t n_utts, int U, int D, const int32_t* __restrict__ taps, int T, int shift,
                                                        int tile, const int64_t* __restrict__ new_offsets, int16_t* __restrict__ out) {
    __shared__ int32_t s_taps[SP_MAX_UD * SP_MAX_T];
    __shared__ __attribute__((aligned(16))) int16_t s_x[SP_SPAN + 16];
    const int t = threadIdx.x;
    const int64_t total = out_base[n_utts];
    const int64_t n_tiles = (total + tile - 1) / tile, per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tile0 = blockIdx.x * per, tile1 = tile0 + per < n_tiles ? tile0 + per : n_tiles;
    if (tile0 >= tile1) return;   // (the whole workgroup)
    for (int i = t; i < U * T; i += SP_T) s_taps[i] = taps[i];   // (the first barrier below comes before any read)
    const int c = (U * T) >> 1;
    const int64_t rnd = shift > 0 ? (int64_t)1 << (shift - 1) : 0;
    SpUtt ut = {0, 0, 0, 0, 0};
    for (int64_t tl = tile0; tl < tile1; ++tl) {
        const int64_t g1 = (tl + 1) * tile < total ? (tl + 1) * tile : total;
        int64_t g = tl * tile;
        for (int piece = 0; piece < tile && g < g1; ++piece) {   // the tile's pieces, one per utterance it touches (each holds an output)
            sp_locate(ut, out_base, offsets, lens, new_offsets, n_utts, g);
            const int64_t a = g - ut.lo, e = g1 < ut.hi ? g1 : ut.hi;   // the piece: outputs a .. a + n - 1 of the utterance
            const int n = (int)(e - g);
            const int64_t v0 = a * D + c, q0 = v0 / U;
            const int p0 = (int)(v0 - q0 * U);
            const int64_t k_lo = q0 - (T - 1);                                    // the first sample the piece reads ...
            const int span = (int)(((int64_t)p0 + (int64_t)(n - 1) * D) / U) + T;    // ... and how many: at most SP_SPAN - 1
            // staging: LDS word w holds samples kw + 8 w .. + 7, where kw <= k_lo is chosen so that a word is 16-byte aligned in the
            // corpus too.  A word that lies inside the file is one 16-byte load; the others are read sample by sample, zeros outside.
            const int16_t* __restrict__ src = audio + ut.off;
            const int sh = (int)(((int64_t)((uintptr_t)src >> 1) + k_lo) & 7);
            const int64_t kw = k_lo - sh;
            const int nw = (sh + span + 7) >> 3;
            __syncthreads();   // the piece before has been computed (first time: the taps are in place)
            for (int w = t; w < nw; w += SP_T) {
                const int64_t k = kw + 8 * (int64_t)w;
                i32x4 v;
                if (k >= 0 && k + 8 <= ut.len) {
                    v = *(const i32x4*)(src + k);
                } else {
                    uint32_t s[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) s[j] = (k + j >= 0 && k + j < ut.len) ? (uint32_t)(uint16_t)src[k + j] : 0u;
                    v.x = (int32_t)(s[0] | (s[1] << 16)), v.y = (int32_t)(s[2] | (s[3] << 16));
                    v.z = (int32_t)(s[4] | (s[5] << 16)), v.w = (int32_t)(s[6] | (s[7] << 16));
                }
                ((i32x4*)s_x)[w] = v;
            }
            __syncthreads();
            const int16_t* __restrict__ xs = s_x + sh + (T - 1);   // x[q0]
            int16_t* __restrict__ d = out + ut.dst + a;
            int head = (int)(((16 - ((uintptr_t)d & 15)) & 15) >> 1);
            head = head < n ? head : n;
            const int nb = (n - head) >> 3, tail0 = head + (nb << 3);
            for (int j = t; j < head; j += SP_T) d[j] = sp_output<WIDE>(s_taps, xs, p0 + j * D, U, T, shift, rnd);
            i32x4* __restrict__ body = (i32x4*)(d + head);
            for (int b = t; b < nb; b += SP_T) {
                uint32_t y[SP_PER];
#pragma unroll
                for (int j = 0; j < SP_PER; ++j)
                    y[j] = (uint32_t)(uint16_t)sp_output<WIDE>(s_taps, xs, p0 + (head + b * SP_PER + j) * D, U, T, shift, rnd);
                i32x4 v;
                v.x = (int32_t)(y[0] | (y[1] << 16)), v.y = (int32_t)(y[2] | (y[3] << 16));
                v.z = (int32_t)(y[4] | (y[5] << 16)), v.w = (int32_t)(y[6] | (y[7] << 16));
                body[b] = v;
            }
            for (int j = tail0 + t; j < n; j += SP_T) d[j] = sp_output<WIDE>(s_taps, xs, p0 + j * D, U, T, shift, rnd);
            g = e;
        }
    }
}

}  // namespace vm

using namespace vm;

extern "C" int vm_resample_i16(const void* audio, const int64_t* offsets, const int64_t* lens, const int64_t* out_base, int64_t n_utts,
                               int U, int D, const int32_t* taps, int T, int shift, int64_t phase_abs_max, const int64_t* new_offsets,
                               void* out, void* stream) {
    const char* me = "vm_resample_i16";
    VM_REQUIRE(U >= 1 && U <= SP_MAX_UD && D >= 1 && D <= SP_MAX_UD, "%s: U and D must be in [1, %d]", me, SP_MAX_UD);
    VM_REQUIRE(T >= 1 && T <= SP_MAX_T, "%s: T (taps per phase) must be in [1, %d]", me, SP_MAX_T);
    VM_REQUIRE(shift >= 0 && shift <= SP_MAX_SHIFT, "%s: shift must be in [0, %d]", me, SP_MAX_SHIFT);
    VM_REQUIRE(phase_abs_max >= 0 && phase_abs_max < ((int64_t)1 << 47), "%s: phase_abs_max must be in [0, 2^47)", me);
    VM_REQUIRE(n_utts >= 0 && n_utts < (1LL << 31), "%s: n_utts must be in [0, 2^31)", me);
    if (n_utts == 0) return VM_OK;
    VM_REQUIRE(audio && offsets && lens && out_base && taps && new_offsets && out, "%s: null pointer", me);
    VM_REQUIRE(((uintptr_t)audio & 1) == 0 && ((uintptr_t)out & 1) == 0, "%s: audio and out must be 2-byte aligned", me);
    VM_REQUIRE(((uintptr_t)taps & 3) == 0, "%s: taps must be 4-byte aligned", me);
    const int tile = sp_tile_outputs(U, D, T);
    hipStream_t st = (hipStream_t)stream;
    if (phase_abs_max <= SP_NARROW_MAX)
        hipLaunchKernelGGL(resample_kernel<false>, dim3(SP_GRID), dim3(SP_T), 0, st, (const int16_t*)audio, offsets, lens, out_base, n_utts,
                           U, D, taps, T, shift, tile, new_offsets, (int16_t*)out);
    else
        hipLaunchKernelGGL(resample_kernel<true>, dim3(SP_GRID), dim3(SP_T), 0, st, (const int16_t*)audio, offsets, lens, out_base, n_utts,
                           U, D, taps, T, shift, tile, new_offsets, (int16_t*)out);
    return check_launch(me);
}
