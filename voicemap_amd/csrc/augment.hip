// Waveform augmentation inside the preprocessing launch of device-resident training (voicemap_amd/augment.py states the semantics in
// float64): window n = the raw_len samples at audio[offsets[n]], and at the DECIMATED positions i = 0..L0-1 only (the reference decimates
// with x[::ds] and no anti-alias filter, voicemap/utils.py:29, so nothing else is ever seen)
//   a_i = sum_{j <= min(i ds, R-1)} r[j] s[i ds - j]        reverberation: a causal FIR with zero history before the crop start
//   v_i = sum_{k < K} noise[noff[n,k] + i ds]               babble
//   y_i = gain (a_i + g v_i),  g = sqrt(Pa / (Pv snr_lin))  Pa, Pv the mean squares over the window's L0 positions
// followed by the whitening of preproc.hip on y.  Only the FIR runs in fp32 (VALU, fp32 accumulation); every sum, g and the whitening
// are fp64 in a fixed order, as in preproc.hip, so a launch is bit-reproducible and the identity launch (K = 0, no RIR, gain 1) is
// vm_crop_decimate_whiten bit for bit.
#include "common.hpp"

namespace vm {

constexpr int AUG_HALO_L = 15, AUG_HALO = 31;   // conv 1's SAME halo (preproc.hip)
constexpr int AUG_SEG = 8;                      // partial-sum segments per window (preproc.hip WS_SEG: the same split, the same order)
constexpr int AUG_SPLIT = 8;                    // workgroups per output row (preproc.hip WA_SPLIT)

__device__ inline float aug_ld(const void* p, int is_i16, int64_t i) {
    return is_i16 ? (float)((const int16_t*)p)[i] * (1.0f / 32768.0f) : ((const float*)p)[i];
}
__device__ inline bool aug_has_rir(const int32_t* rir_id, int n_rirs, int64_t n) {
    return n_rirs > 0 && rir_id[n] >= 0 && rir_id[n] < n_rirs;
}

__device__ inline float fir_to_f(float v) { return v; }
__device__ inline float fir_to_f(int16_t v) { return (float)v * (1.0f / 32768.0f); }

// ---- the decimating FIR ---------------------------------------------------------------------------------------------------------
// Polyphase: with j = p + m ds,  a_i = sum_p sum_m r_p[m] s_p[i - m],  r_p[m] = r[p + m ds],  s_p[k] = s[k ds - p]  -- ds ordinary FIRs
// over the decimated grid, L0 R multiply-adds per window.  A workgroup of 256 threads makes a tile of 2048 outputs of one window, a
// thread 8 CONSECUTIVE ones: for a block of 8 taps it needs the 15 samples s_p[i_base - m0 - 7 .. i_base - m0 + 7], 8 of which it
// already holds from the block before -- 64 FMAs per two ds_read_b128 of samples and two (broadcast: every lane the same address) of
// taps.  Per phase and chunk of 256 taps the workgroup stages the chunk's taps and the TILE + 256 samples they touch in LDS; the
// samples are read from global memory at stride ds (9 loads per thread against 2048 FMAs).
// LDS image of the samples: threads read 16-byte pieces at a stride of 8 words, which alone puts lanes t and t + 8 on the same banks;
// 4 words of padding after every 128 (16 lanes' worth) spreads the 16 lanes of a ds_read_b128 group over all 64 banks when the
// block index is a multiple of 16, and leaves at most a 2-way conflict otherwise (LDS cycles stay below half the FMA cycles).
constexpr int FIR_T = 256, FIR_O = 8, FIR_TILE = FIR_T * FIR_O, FIR_MC = 256;
constexpr int FIR_SEG = FIR_TILE + FIR_MC;
__device__ __host__ constexpr int fir_phys(int l) { return l + 4 * (l >> 7); }
constexpr int FIR_SEG_WORDS = fir_phys(FIR_SEG) + 4;

template <typename S>
__global__ __launch_bounds__(FIR_T) void fir_decimate_kernel(const S* __restrict__ audio, const int64_t* __restrict__ offsets,
                                                              int64_t raw_len, int ds, int64_t L0, const float* __restrict__ rirs,
                                                              int n_rirs, int R, const int32_t* __restrict__ rir_id,
                                                              float* __restrict__ a) {
    __shared__ __attribute__((aligned(16))) float seg[FIR_SEG_WORDS];
    __shared__ __attribute__((aligned(16))) float taps[FIR_MC];
    const int64_t n = blockIdx.y;
    if (!aug_has_rir(rir_id, n_rirs, n)) return;   // (uniform over the workgroup) no RIR: no FIR work, `a` is never read for this window
    const S* __restrict__ s = audio + offsets[n];
    const float* __restrict__ r = rirs + (int64_t)rir_id[n] * R;
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * FIR_TILE;
    const int64_t i_end = i0 + FIR_TILE < L0 ? i0 + FIR_TILE : L0;   // one past the tile's last output
    float acc[FIR_O];
#pragma unroll
    for (int o = 0; o < FIR_O; ++o) acc[o] = 0.f;
    for (int p = 0; p < ds && p < R; ++p) {
        const int64_t Mp = ((int64_t)R - p + ds - 1) / ds;   // taps of this phase
        const int64_t mlim = Mp < i_end ? Mp : i_end;        // causal: tap m reaches output i only for m <= i
        for (int64_t m0 = 0; m0 < mlim; m0 += FIR_MC) {
            __syncthreads();   // the chunk before is consumed
            {
                const int64_t m = m0 + t;
                taps[t] = m < Mp ? r[p + m * ds] : 0.f;
            }
            const int64_t kmin = i0 - m0 - FIR_MC;   // s_p index of seg[0]; a multiple of 8
            for (int l = t; l < FIR_SEG; l += FIR_T) {
                const int64_t tt = (kmin + l) * ds - p;   // sample of the crop: zero history before it, nothing at or past raw_len
                seg[fir_phys(l)] = (tt >= 0 && tt < raw_len) ? fir_to_f(s[tt]) : 0.f;
            }
            __syncthreads();
            const int64_t left = mlim - m0;
            const int mb_end = left < FIR_MC ? (int)((left + 7) & ~(int64_t)7) : FIR_MC;
            float hi[8], lo[8], rr[8];
            {
                const float4* q = (const float4*)&seg[fir_phys(FIR_O * t + FIR_MC)];
                const float4 h0 = q[0], h1 = q[1];
                hi[0] = h0.x, hi[1] = h0.y, hi[2] = h0.z, hi[3] = h0.w, hi[4] = h1.x, hi[5] = h1.y, hi[6] = h1.z, hi[7] = h1.w;
            }
            for (int mb = 0; mb < mb_end; mb += 8) {
                const float4* q = (const float4*)&seg[fir_phys(FIR_O * t + FIR_MC - mb - 8)];
                const float4 l0 = q[0], l1 = q[1];
                lo[0] = l0.x, lo[1] = l0.y, lo[2] = l0.z, lo[3] = l0.w, lo[4] = l1.x, lo[5] = l1.y, lo[6] = l1.z, lo[7] = l1.w;
                const float4* w = (const float4*)&taps[mb];
                const float4 r0 = w[0], r1 = w[1];
                rr[0] = r0.x, rr[1] = r0.y, rr[2] = r0.z, rr[3] = r0.w, rr[4] = r1.x, rr[5] = r1.y, rr[6] = r1.z, rr[7] = r1.w;
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int o = 0; o < FIR_O; ++o)   // output i_base + o, tap m0 + mb + u: sample s_p[i_base - m0 - mb + (o - u)]
                        acc[o] = fmaf(rr[u], o - u >= 0 ? hi[o - u] : lo[8 + o - u], acc[o]);
#pragma unroll
                for (int e = 0; e < 8; ++e) hi[e] = lo[e];
            }
        }
    }
    const int64_t ib = i0 + (int64_t)FIR_O * t;
#pragma unroll
    for (int o = 0; o < FIR_O; ++o)
        if (ib + o < L0) a[n * L0 + ib + o] = acc[o];
}

// ---- sums: per (window, segment) partials of a, a^2, v, v^2, a v over the decimated positions (fp64; the split, the thread stride
// and the reduction tree are whiten_stats_kernel's).  grid = (n_windows, AUG_SEG).
__global__ __launch_bounds__(256) void aug_stats_kernel(const void* __restrict__ audio, int is_i16, const int64_t* __restrict__ offsets,
                                                        int ds, int64_t L0, const void* __restrict__ noise, int noise_i16,
                                                        const int64_t* __restrict__ noff, int K, const float* __restrict__ a_ws,
                                                        int n_rirs, const int32_t* __restrict__ rir_id, double* __restrict__ part,
                                                        int64_t n_windows) {
    __shared__ double red[5][4];
    const int64_t n = blockIdx.x;
    const int seg = blockIdx.y;
    const bool rir = aug_has_rir(rir_id, n_rirs, n);
    const int64_t off = offsets[n];
    const int64_t per = (L0 + AUG_SEG - 1) / AUG_SEG;
    const int64_t i1 = (seg + 1) * per < L0 ? (seg + 1) * per : L0;
    double s = 0.0, q = 0.0, sv = 0.0, qv = 0.0, sav = 0.0;
    for (int64_t i = seg * per + threadIdx.x; i < i1; i += 256) {
        const double v = rir ? (double)a_ws[n * L0 + i] : (double)aug_ld(audio, is_i16, off + i * ds);
        s += v;
        q += v * v;
        if (K > 0) {
            double b = 0.0;
            for (int k = 0; k < K; ++k) b += (double)aug_ld(noise, noise_i16, noff[n * K + k] + i * ds);
            sv += b;
            qv += b * b;
            sav += v * b;
        }
    }
    double w[5] = {s, q, sv, qv, sav};
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        w[c] = wave_sum_d(w[c]);
        if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = w[c];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int c = threadIdx.x;
        part[((int64_t)c * n_windows + n) * AUG_SEG + seg] = (red[c][0] + red[c][1]) + (red[c][2] + red[c][3]);
    }
}

// ---- per window: g from the window's mean squares, then the partials of y = gain (a + g v) and y^2 per segment in the layout the
// whitening reads.  One thread per window; every sum in index order.
__global__ __launch_bounds__(256) void aug_finalize_kernel(const double* __restrict__ part, int64_t n_windows, int64_t L0, int K,
                                                           const float* __restrict__ snr_lin, const float* __restrict__ gain,
                                                           double* __restrict__ g_out, double* __restrict__ psum,
                                                           double* __restrict__ psq) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_windows) return;
    const double* pa = part + (0 * n_windows + n) * AUG_SEG;
    const double* qa = part + (1 * n_windows + n) * AUG_SEG;
    const double* pv = part + (2 * n_windows + n) * AUG_SEG;
    const double* qv = part + (3 * n_windows + n) * AUG_SEG;
    const double* av = part + (4 * n_windows + n) * AUG_SEG;
    double g = 0.0;
    if (K > 0 && snr_lin[n] > 0.f) {
        double A = 0.0, V = 0.0;
        for (int k = 0; k < AUG_SEG; ++k) {
            A += qa[k];
            V += qv[k];
        }
        const double Pa = A / (double)L0, Pv = V / (double)L0;
        if (Pa > 0.0 && Pv > 0.0) g = sqrt(Pa / (Pv * (double)snr_lin[n]));
    }
    const double G = (double)gain[n];
    g_out[n] = g;
    for (int k = 0; k < AUG_SEG; ++k) {
        // (g == 0 leaves the speech terms alone: with gain 1 the partials are the plain kernel's, bit for bit)
        psum[n * AUG_SEG + k] = g != 0.0 ? G * (pa[k] + g * pv[k]) : G * pa[k];
        psq[n * AUG_SEG + k] = g != 0.0 ? (G * G) * (qa[k] + 2.0 * g * av[k] + (g * g) * qv[k]) : (G * G) * qa[k];
    }
}

// ---- whitening of y with conv 1's halo: whiten_apply_kernel of preproc.hip with y in the place of the decimated sample.
// grid = (AUG_SPLIT, n_windows).
__global__ __launch_bounds__(256) void aug_apply_kernel(const void* __restrict__ audio, int is_i16, const int64_t* __restrict__ offsets,
                                                        int ds, int64_t L0, int whitening, int64_t wpt, float rms,
                                                        const void* __restrict__ noise, int noise_i16, const int64_t* __restrict__ noff,
                                                        int K, const float* __restrict__ gain, const float* __restrict__ a_ws,
                                                        int n_rirs, const int32_t* __restrict__ rir_id, const double* __restrict__ g_in,
                                                        const double* __restrict__ psum, const double* __restrict__ psq,
                                                        float* __restrict__ out) {
    __shared__ double red[4];
    const int64_t n = blockIdx.y;
    const bool rir = aug_has_rir(rir_id, n_rirs, n);
    const int64_t off = offsets[n];
    double m = 0.0, sc = 1.0;
    if (whitening) {
        const int64_t tw = n / wpt;
        double q = 0.0;
        for (int64_t j = threadIdx.x; j < wpt * AUG_SEG; j += 256) q += psq[tw * wpt * AUG_SEG + j];
        q = wave_sum_d(q);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
        __syncthreads();
        const double tot = (red[0] + red[1]) + (red[2] + red[3]);
        sc = (double)rms / sqrt(tot / ((double)wpt * (double)L0));
        double s = 0.0;
        for (int k = 0; k < AUG_SEG; ++k) s += psum[n * AUG_SEG + k];
        m = s / (double)L0;
    }
    const double g = g_in[n], G = (double)gain[n];
    const int64_t row = L0 + AUG_HALO, per = (row + AUG_SPLIT - 1) / AUG_SPLIT;
    const int64_t i1 = (blockIdx.x + 1) * per < row ? (blockIdx.x + 1) * per : row;
    for (int64_t i = blockIdx.x * per + threadIdx.x; i < i1; i += 256) {
        const int64_t t = i - AUG_HALO_L;
        float v = 0.f;
        if (t >= 0 && t < L0) {
            double y = rir ? (double)a_ws[n * L0 + t] : (double)aug_ld(audio, is_i16, off + t * ds);
            if (g != 0.0) {
                double b = 0.0;
                for (int k = 0; k < K; ++k) b += (double)aug_ld(noise, noise_i16, noff[n * K + k] + t * ds);
                y += g * b;
            }
            y *= G;
            v = (float)((y - m) * sc);
        }
        out[n * row + i] = v;
    }
}

}  // namespace vm

using namespace vm;

// doubles: 5 partial planes + the two whitening planes, (n_windows, AUG_SEG) each, and g (n_windows); then a (n_windows, L0) fp32
static inline int64_t aug_ws_doubles(int64_t n_windows) { return (7 * AUG_SEG + 1) * n_windows; }

extern "C" int64_t vm_crop_augment_workspace_bytes(int64_t n_windows, int64_t L0) {
    if (n_windows <= 0 || L0 <= 0) return 0;
    return aug_ws_doubles(n_windows) * (int64_t)sizeof(double) + n_windows * L0 * (int64_t)sizeof(float);
}

extern "C" int vm_crop_augment_decimate_whiten(const void* audio, int raw_is_i16, const int64_t* offsets, int64_t n_windows,
                                               int64_t raw_len, int downsampling, int whitening, float rms, int64_t windows_per_tower,
                                               const void* noise, int noise_is_i16, const int64_t* noise_offsets, int K,
                                               const float* snr_lin, const float* gain, const float* rirs, int n_rirs, int R,
                                               const int32_t* rir_id, float* out, void* ws, void* stream) {
    const char* me = "vm_crop_augment_decimate_whiten";
    VM_REQUIRE(audio && offsets && out && ws && snr_lin && gain, "%s: null pointer", me);
    VM_REQUIRE(n_windows > 0 && n_windows < 65536 && raw_len > 0 && downsampling > 0 && windows_per_tower > 0, "%s: bad sizes", me);
    VM_REQUIRE(n_windows % windows_per_tower == 0, "%s: n_windows must be a multiple of windows_per_tower", me);
    VM_REQUIRE(K >= 0 && (K == 0 || (noise && noise_offsets)), "%s: K > 0 needs noise and noise_offsets", me);
    VM_REQUIRE(n_rirs >= 0 && (n_rirs == 0 || (rirs && rir_id && R >= 1 && R <= 8192)),
               "%s: n_rirs > 0 needs rirs, rir_id and 1 <= R <= 8192", me);
    const int ds = downsampling;
    const int64_t L0 = (raw_len + ds - 1) / ds;
    VM_REQUIRE((L0 + FIR_TILE - 1) / FIR_TILE < (1LL << 31), "%s: raw_len too long", me);
    double* part = (double*)ws;
    double* psum = part + 5 * AUG_SEG * n_windows;
    double* psq = psum + AUG_SEG * n_windows;
    double* g = psq + AUG_SEG * n_windows;
    float* a = (float*)(part + aug_ws_doubles(n_windows));
    hipStream_t st = (hipStream_t)stream;
    if (n_rirs > 0) {
        const dim3 gf((unsigned)((L0 + FIR_TILE - 1) / FIR_TILE), (unsigned)n_windows);
        if (raw_is_i16)
            hipLaunchKernelGGL((fir_decimate_kernel<int16_t>), gf, dim3(FIR_T), 0, st, (const int16_t*)audio, offsets, raw_len, ds, L0,
                               rirs, n_rirs, R, rir_id, a);
        else
            hipLaunchKernelGGL((fir_decimate_kernel<float>), gf, dim3(FIR_T), 0, st, (const float*)audio, offsets, raw_len, ds, L0, rirs,
                               n_rirs, R, rir_id, a);
    }
    hipLaunchKernelGGL(aug_stats_kernel, dim3((unsigned)n_windows, AUG_SEG), dim3(256), 0, st, audio, raw_is_i16, offsets, ds, L0, noise,
                       noise_is_i16, noise_offsets, K, a, n_rirs, rir_id, part, n_windows);
    hipLaunchKernelGGL(aug_finalize_kernel, dim3((unsigned)((n_windows + 255) / 256)), dim3(256), 0, st, part, n_windows, L0, K, snr_lin,
                       gain, g, psum, psq);
    hipLaunchKernelGGL(aug_apply_kernel, dim3(AUG_SPLIT, (unsigned)n_windows), dim3(256), 0, st, audio, raw_is_i16, offsets, ds, L0,
                       whitening, windows_per_tower, rms, noise, noise_is_i16, noise_offsets, K, gain, a, n_rirs, rir_id, g, psum, psq,
                       out);
    return check_launch(me);
}
