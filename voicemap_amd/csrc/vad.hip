// Voice activity detection on the resident int16 corpus and the compaction of the kept frames (voicemap_amd/vad.py states the rule in
// numpy and is what the tests compare against, bit for bit).  Utterance u = the lens[u] samples at audio[offsets[u]], cut into
// F = ceil(len / Fr) frames (the last one short); all per-frame arrays are flat over the corpus, utterance u's frames at
// [frame_base[u], frame_base[u + 1]).
//   energy pass   E_f = sum of s^2 over the frame (int64; integer sums: any order gives the same bits)
//   decide pass   T = sum_f E_f;  a_f = E_f > 0 && D(E_f) * D(len) >= rel * (D(T) * D(n_f)) && D(E_f) >= floor * D(n_f)  (double
//                 multiplies only, in this association);  p = runs of >= min_run active frames;  v = p widened by hang frames;
//                 V = sum v_f n_f < min_keep keeps the utterance whole;  dst = exclusive scan of v_f n_f
//   compact       out[new_offsets[u] + dst_f + t] = s[f Fr + t] for the kept frames
// The energy and compact passes run over tiles of the flat frame list, a fixed grid of workgroups with an equal run of consecutive tiles
// each: a tile's position in that list names its (utterance, frames) through a binary search of frame_base, so the utterance never sits
// in grid.y (65535 there; a corpus has more files).  The decide pass
// is one workgroup per utterance in grid.x.  No atomics, no workgroup waits on another, every loop is bounded by an argument or by a
// length the arguments hold.
#include "common.hpp"

namespace vm {

constexpr int VAD_T = 256;                       // threads per workgroup, all three kernels
constexpr int VAD_GRID = 4096;                   // workgroups of the tiled passes, an equal run of consecutive tiles each (the frame total is on the device)
constexpr int VAD_MAX_FRAME = 4096, VAD_MAX_RUN = 64, VAD_MAX_HANG = 256;
constexpr int VAD_CH = 1024;                     // frames per chunk of the decide pass (4 per thread); vad.py DECIDE_CHUNK
constexpr int VAD_PER = VAD_CH / VAD_T;
constexpr int VAD_HALO = VAD_MAX_HANG + VAD_MAX_RUN - 1;

typedef __attribute__((ext_vector_type(4))) int32_t i32x4;

// the utterance of flat frame g: the largest u with frame_base[u] <= g (utterances without frames never match)
__device__ inline int64_t vad_find_utt(const int64_t* __restrict__ frame_base, int64_t n_utts, int64_t g) {
    int64_t lo = 0, hi = n_utts;
    for (int it = 0; it < 64 && hi - lo > 1; ++it) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (frame_base[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// the utterance a thread last worked in: a workgroup walks CONSECUTIVE tiles, so the search runs once per utterance, not once per frame
struct VadUtt {
    int64_t u, lo, hi, off, len;   // its index, its frames [lo, hi) of the flat list, its first sample, its length
};
__device__ inline void vad_locate(VadUtt& c, const int64_t* __restrict__ frame_base, const int64_t* __restrict__ offsets,
                                  const int64_t* __restrict__ lens, int64_t n_utts, int64_t g) {
    if (g >= c.lo && g < c.hi) return;
    const int64_t u = vad_find_utt(frame_base, n_utts, g);
    c.u = u, c.lo = frame_base[u], c.hi = frame_base[u + 1], c.off = offsets[u], c.len = lens[u];
}

__device__ inline uint32_t vad_sq2(int32_t w) {   // the squares of the two int16 halves of a word: at most 2^31 together
    const int32_t a = (int32_t)(int16_t)(w & 0xffff), b = w >> 16;
    return (uint32_t)(a * a) + (uint32_t)(b * b);
}

// ---- energy: 2^lg lanes per frame, 256 >> lg frames per tile.  Within a frame: the samples before the first 16-byte boundary and
// after the last one are read one by one, the body as 16-byte words (the start of an utterance is only 2-byte aligned).  Nothing
// outside the frame is read.
__global__ __launch_bounds__(VAD_T) void vad_energy_kernel(const int16_t* __restrict__ audio, const int64_t* __restrict__ offsets,
                                                           const int64_t* __restrict__ lens, const int64_t* __restrict__ frame_base,
                                                           int64_t n_utts, int Fr, int lg, int64_t* __restrict__ energy) {
    const int G = 1 << lg, fpt = VAD_T >> lg;
    const int lane = threadIdx.x & (G - 1), slot = threadIdx.x >> lg;
    const int64_t total = frame_base[n_utts];
    const int64_t n_tiles = (total + fpt - 1) / fpt, per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tile0 = blockIdx.x * per, tile1 = tile0 + per < n_tiles ? tile0 + per : n_tiles;
    VadUtt ut = {0, 0, 0, 0, 0};
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t g = tile * fpt + slot;
        int64_t acc = 0;
        bool live = false;
        if (g < total) {
            vad_locate(ut, frame_base, offsets, lens, n_utts, g);
            const int64_t s0 = (g - ut.lo) * Fr, len = ut.len;
            if (s0 < len) {
                live = true;
                const int nf = (int)(len - s0 < Fr ? len - s0 : Fr);
                const int16_t* __restrict__ s = audio + ut.off + s0;
                int head = (int)(((16 - ((uintptr_t)s & 15)) & 15) >> 1);
                head = head < nf ? head : nf;
                const int nb = (nf - head) >> 3, tail0 = head + (nb << 3);
                for (int i = lane; i < head; i += G) acc += (int32_t)s[i] * (int32_t)s[i];
                const i32x4* __restrict__ body = (const i32x4*)(s + head);
                for (int c = lane; c < nb; c += G) {
                    const i32x4 w = body[c];
                    acc += (int64_t)vad_sq2(w.x) + (int64_t)vad_sq2(w.y) + (int64_t)vad_sq2(w.z) + (int64_t)vad_sq2(w.w);
                }
                for (int i = tail0 + lane; i < nf; i += G) acc += (int32_t)s[i] * (int32_t)s[i];
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);   // (every lane of the wave gets here)
        if (live && lane == 0) energy[g] = acc;
    }
}

// ---- decide: one workgroup per utterance.  It walks the frames in chunks of VAD_CH with the kept-sample count carried from chunk to
// chunk; a chunk's v needs p over hang more frames on either side, and that p needs a over min_run - 1 more.
__global__ __launch_bounds__(VAD_T) void vad_decide_kernel(const int64_t* __restrict__ lens, const int64_t* __restrict__ frame_base,
                                                           int Fr, double rel, double floor_e, int m, int h, int64_t min_keep,
                                                           const int64_t* __restrict__ energy, uint8_t* __restrict__ mask,
                                                           int64_t* __restrict__ dst, int64_t* __restrict__ new_lens,
                                                           int32_t* __restrict__ info) {
    __shared__ uint8_t sa[VAD_CH + 2 * VAD_HALO + 2];
    __shared__ uint8_t sp[VAD_CH + 2 * VAD_MAX_HANG];
    __shared__ int64_t red[3][VAD_T / 64];
    __shared__ int64_t wtot[VAD_T / 64];
    const int64_t u = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, wl = t & 63;
    const int64_t len = lens[u], fb = frame_base[u];
    const int64_t F = len > 0 ? (len + Fr - 1) / Fr : 0;
    const int64_t* __restrict__ E = energy + fb;
    // T
    int64_t T = 0;
    for (int64_t f = t; f < F; f += VAD_T) T += E[f];
    for (int o = 32; o > 0; o >>= 1) T += __shfl_xor(T, o, 64);
    if (wl == 0) red[0][wave] = T;
    __syncthreads();
    T = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    __syncthreads();
    const double dlen = (double)len, dT = (double)T;
    const int H = h + m - 1;
    int64_t carry = 0, n_act = 0, n_kept = 0;
    for (int64_t c0 = 0; c0 < F; c0 += VAD_CH) {
        // a over the chunk and its halo of hang + min_run - 1 frames on either side (frames outside [0, F) are inactive)
        for (int i = t; i < VAD_CH + 2 * H; i += VAD_T) {
            const int64_t f = c0 - H + i;
            uint8_t a = 0;
            if (f >= 0 && f < F) {
                const int64_t e = E[f];
                const int64_t rest = len - f * Fr;
                const double nf = (double)(rest < Fr ? rest : (int64_t)Fr), de = (double)e;
                a = (e > 0 && de * dlen >= rel * (dT * nf) && de >= floor_e * nf) ? 1 : 0;
                if (i >= H && i < H + VAD_CH) n_act += a;
            }
            sa[i] = a;
        }
        __syncthreads();
        // p over the chunk and hang frames on either side: the run of active frames through the frame is at least m long
        for (int j = t; j < VAD_CH + 2 * h; j += VAD_T) {
            const int i = j + m - 1;
            uint8_t p = 0;
            if (sa[i]) {
                int run = 1;
                for (int k = 1; k < m && sa[i - k]; ++k) ++run;
                for (int k = 1; k < m && sa[i + k]; ++k) ++run;
                p = run >= m ? 1 : 0;
            }
            sp[j] = p;
        }
        __syncthreads();
        // v, and the exclusive scan of v n_f: a thread owns VAD_PER consecutive frames
        uint8_t v[VAD_PER];
        int64_t nfs[VAD_PER], mine = 0;
#pragma unroll
        for (int q = 0; q < VAD_PER; ++q) {
            const int fl = t * VAD_PER + q;
            const int64_t f = c0 + fl;
            v[q] = 0;
            nfs[q] = 0;
            if (f < F) {
                for (int d = 0; d <= 2 * h; ++d)
                    if (sp[fl + d]) {
                        v[q] = 1;
                        break;
                    }
                const int64_t rest = len - f * Fr;
                nfs[q] = rest < Fr ? rest : (int64_t)Fr;
                mine += v[q] ? nfs[q] : 0;
                n_kept += v[q];
            }
        }
        int64_t inc = mine;   // inclusive scan over the wave, then over the four waves
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t up = __shfl_up(inc, o, 64);
            if (wl >= o) inc += up;
        }
        if (wl == 63) wtot[wave] = inc;
        __syncthreads();
        int64_t before = carry;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        const int64_t chunk_total = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
        int64_t pos = before + inc - mine;
#pragma unroll
        for (int q = 0; q < VAD_PER; ++q) {
            const int64_t f = c0 + t * VAD_PER + q;
            if (f < F) {
                mask[fb + f] = v[q];
                dst[fb + f] = pos;
                pos += v[q] ? nfs[q] : 0;
            }
        }
        carry += chunk_total;
        __syncthreads();   // sa, sp and wtot are free for the next chunk
    }
    // the counts, then the fallback
    for (int o = 32; o > 0; o >>= 1) {
        n_act += __shfl_xor(n_act, o, 64);
        n_kept += __shfl_xor(n_kept, o, 64);
    }
    if (wl == 0) {
        red[1][wave] = n_act;
        red[2][wave] = n_kept;
    }
    __syncthreads();
    n_act = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    n_kept = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    const bool fallback = carry < min_keep;
    if (fallback) {   // kept whole (the workgroup's own earlier stores to mask / dst are ordered before these by the barriers above)
        for (int64_t f = t; f < F; f += VAD_T) {
            mask[fb + f] = 1;
            dst[fb + f] = f * Fr;
        }
    }
    if (t == 0) {
        new_lens[u] = fallback ? len : carry;
        info[u * 4 + 0] = (int32_t)F;
        info[u * 4 + 1] = (int32_t)n_act;
        info[u * 4 + 2] = (int32_t)(fallback ? F : n_kept);
        info[u * 4 + 3] = fallback ? 1 : 0;
    }
}

// ---- compact: the tiling of the energy pass; a kept frame is copied by its 2^lg lanes.  Stores: 2-byte up to the first 16-byte
// boundary of the DESTINATION and after the last, 16-byte in between.  The source of a 16-byte store sits at any 2-byte offset R from a
// 16-byte boundary: where the two aligned source words around it lie inside the frame they are loaded whole and shifted into place,
// elsewhere (the frame's first and last words) the eight samples are read one by one.  Nothing outside the frame is read or written.
template <int R>
__device__ inline i32x4 vad_funnel(const i32x4 lo, const i32x4 hi) {   // samples R .. R + 7 of the sixteen in (lo, hi)
    const uint32_t w[8] = {(uint32_t)lo.x, (uint32_t)lo.y, (uint32_t)lo.z, (uint32_t)lo.w,
                           (uint32_t)hi.x, (uint32_t)hi.y, (uint32_t)hi.z, (uint32_t)hi.w};
    constexpr int q = R >> 1;
    i32x4 o;
    if (R & 1) {
        o.x = (int32_t)((w[q] >> 16) | (w[q + 1] << 16));
        o.y = (int32_t)((w[q + 1] >> 16) | (w[q + 2] << 16));
        o.z = (int32_t)((w[q + 2] >> 16) | (w[q + 3] << 16));
        o.w = (int32_t)((w[q + 3] >> 16) | (w[q + 4] << 16));
    } else {
        o.x = (int32_t)w[q], o.y = (int32_t)w[q + 1], o.z = (int32_t)w[q + 2], o.w = (int32_t)w[q + 3];
    }
    return o;
}

__global__ __launch_bounds__(VAD_T) void vad_compact_kernel(const int16_t* __restrict__ audio, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ lens, const int64_t* __restrict__ frame_base,
                                                            const uint8_t* __restrict__ mask, const int64_t* __restrict__ dst,
                                                            const int64_t* __restrict__ new_offsets, int64_t n_utts, int Fr, int lg,
                                                            int16_t* __restrict__ out) {
    const int G = 1 << lg, fpt = VAD_T >> lg;
    const int lane = threadIdx.x & (G - 1), slot = threadIdx.x >> lg;
    const int64_t total = frame_base[n_utts];
    const int64_t n_tiles = (total + fpt - 1) / fpt, per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tile0 = blockIdx.x * per, tile1 = tile0 + per < n_tiles ? tile0 + per : n_tiles;
    VadUtt ut = {0, 0, 0, 0, 0};
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t g = tile * fpt + slot;
        if (g >= total || !mask[g]) continue;
        vad_locate(ut, frame_base, offsets, lens, n_utts, g);
        const int64_t s0 = (g - ut.lo) * Fr, len = ut.len;
        if (s0 >= len) continue;
        const int nf = (int)(len - s0 < Fr ? len - s0 : Fr);
        const int16_t* __restrict__ s = audio + ut.off + s0;
        int16_t* __restrict__ d = out + new_offsets[ut.u] + dst[g];
        int head = (int)(((16 - ((uintptr_t)d & 15)) & 15) >> 1);
        head = head < nf ? head : nf;
        const int nb = (nf - head) >> 3, tail0 = head + (nb << 3);
        for (int i = lane; i < head; i += G) d[i] = s[i];
        const int R = (int)(((uintptr_t)(s + head) & 15) >> 1);        // the body's source offset from a 16-byte boundary, in samples
        const int16_t* __restrict__ sal = s + head - R;                // that boundary (at or before the frame's first body sample)
        i32x4* __restrict__ dbody = (i32x4*)(d + head);
        for (int c = lane; c < nb; c += G) {
            const int e0 = head + (c << 3);                            // the chunk's first sample in the frame
            // aligned source words [e0 - R, e0 - R + 8) and, if R > 0, [e0 - R + 8, e0 - R + 16): inside [0, nf)?
            const bool whole = e0 - R >= 0 && e0 - R + (R ? 16 : 8) <= nf;
            i32x4 o;
            if (whole) {
                const i32x4* __restrict__ w = (const i32x4*)(sal + (c << 3));
                const i32x4 lo = w[0];
                const i32x4 hi = R ? w[1] : lo;
                switch (R) {
                    case 0: o = lo; break;
                    case 1: o = vad_funnel<1>(lo, hi); break;
                    case 2: o = vad_funnel<2>(lo, hi); break;
                    case 3: o = vad_funnel<3>(lo, hi); break;
                    case 4: o = vad_funnel<4>(lo, hi); break;
                    case 5: o = vad_funnel<5>(lo, hi); break;
                    case 6: o = vad_funnel<6>(lo, hi); break;
                    default: o = vad_funnel<7>(lo, hi); break;
                }
            } else {
                const uint16_t* __restrict__ q = (const uint16_t*)(s + e0);
                o.x = (int32_t)((uint32_t)q[0] | ((uint32_t)q[1] << 16));
                o.y = (int32_t)((uint32_t)q[2] | ((uint32_t)q[3] << 16));
                o.z = (int32_t)((uint32_t)q[4] | ((uint32_t)q[5] << 16));
                o.w = (int32_t)((uint32_t)q[6] | ((uint32_t)q[7] << 16));
            }
            dbody[c] = o;
        }
        for (int i = tail0 + lane; i < nf; i += G) d[i] = s[i];
    }
}

// lanes per frame: one 16-byte word each where the frame allows, a power of two in [1, 64]
static inline int vad_lanes_log2(int frame) {
    const int words = (frame + 7) / 8;
    int lg = 0;
    while ((1 << lg) < words && lg < 6) ++lg;
    return lg;
}

}  // namespace vm

using namespace vm;

extern "C" int vm_vad_frames(const void* audio, const int64_t* offsets, const int64_t* lens, const int64_t* frame_base, int64_t n_utts,
                             int frame, double rel, double floor_e, int min_run, int hang, int64_t min_keep, int64_t* energy, void* mask,
                             int64_t* dst, int64_t* new_lens, int32_t* info, void* stream) {
    const char* me = "vm_vad_frames";
    VM_REQUIRE(frame >= 1 && frame <= VAD_MAX_FRAME, "%s: frame must be in [1, %d]", me, VAD_MAX_FRAME);
    VM_REQUIRE(min_run >= 1 && min_run <= VAD_MAX_RUN, "%s: min_run must be in [1, %d]", me, VAD_MAX_RUN);
    VM_REQUIRE(hang >= 0 && hang <= VAD_MAX_HANG, "%s: hang must be in [0, %d]", me, VAD_MAX_HANG);
    VM_REQUIRE(rel >= 0.0 && floor_e >= 0.0, "%s: rel and floor_e must be non-negative numbers", me);
    VM_REQUIRE(n_utts >= 0 && n_utts < (1LL << 31), "%s: n_utts must be in [0, 2^31)", me);
    if (n_utts == 0) return VM_OK;
    VM_REQUIRE(audio && offsets && lens && frame_base && energy && mask && dst && new_lens && info, "%s: null pointer", me);
    VM_REQUIRE(((uintptr_t)audio & 1) == 0, "%s: audio must be 2-byte aligned", me);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vad_energy_kernel, dim3(VAD_GRID), dim3(VAD_T), 0, st, (const int16_t*)audio, offsets, lens, frame_base, n_utts,
                       frame, vad_lanes_log2(frame), energy);
    hipLaunchKernelGGL(vad_decide_kernel, dim3((unsigned)n_utts), dim3(VAD_T), 0, st, lens, frame_base, frame, rel, floor_e, min_run, hang,
                       min_keep, (const int64_t*)energy, (uint8_t*)mask, dst, new_lens, info);
    return check_launch(me);
}

extern "C" int vm_vad_compact(const void* audio, const int64_t* offsets, const int64_t* lens, const int64_t* frame_base, const void* mask,
                              const int64_t* dst, const int64_t* new_offsets, int64_t n_utts, int frame, void* out, void* stream) {
    const char* me = "vm_vad_compact";
    VM_REQUIRE(frame >= 1 && frame <= VAD_MAX_FRAME, "%s: frame must be in [1, %d]", me, VAD_MAX_FRAME);
    VM_REQUIRE(n_utts >= 0 && n_utts < (1LL << 31), "%s: n_utts must be in [0, 2^31)", me);
    if (n_utts == 0) return VM_OK;
    VM_REQUIRE(audio && offsets && lens && frame_base && mask && dst && new_offsets && out, "%s: null pointer", me);
    VM_REQUIRE(((uintptr_t)audio & 1) == 0 && ((uintptr_t)out & 1) == 0, "%s: audio and out must be 2-byte aligned", me);
    hipLaunchKernelGGL(vad_compact_kernel, dim3(VAD_GRID), dim3(VAD_T), 0, (hipStream_t)stream, (const int16_t*)audio, offsets, lens,
                       frame_base, (const uint8_t*)mask, dst, new_offsets, n_utts, frame, vad_lanes_log2(frame), (int16_t*)out);
    return check_launch(me);
}
