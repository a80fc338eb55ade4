/*
 * voicemap_hip.h -- C ABI of libvoicemap_hip.so (gfx950 / MI355X).
 *
 * The reference (oscarknagg/voicemap) has no FFI of its own: its hot path is Keras-2.2.2 layer calls
 * that TensorFlow lowers to cuDNN/Eigen kernels.  Each entry point below replaces one such implicit
 * device op (or a fusion of several); the reference line that *creates* the op is cited.  Host code
 * (voicemap_amd/ *.py, the mirror of voicemap/{models,utils,librispeech}.py) binds these with ctypes;
 * INTEGRATION.md shows the stub.
 *
 * Conventions (every function):
 *   - plain pointers are DEVICE pointers unless named host_*; sizes are explicit; no torch types.
 *   - `dtype` selects the storage type of activations / GEMM operands: VM_F32, VM_F32S, VM_BF16 or VM_F16 (the enum below).
 *     Accumulation, batch statistics, the tail (global max -> dense -> head -> loss) and the optimizer are always fp32.
 *   - enqueue-only on `stream` (a hipStream_t passed as void*); no host sync, no allocation; re-entrant per
 *     stream.  Process-global mutable state: (a) the kernel-selection table behind vm_set_tuning, (b) a pool of zero-initialised
 *     ticket words in device memory that the fused two-stage reductions draw from (round robin per launch; every launch leaves its
 *     words zero again) -- it makes those entry points, like the table, not thread-safe across host threads.  The table
 *     (below): every selectable kernel computes the same result (each is parity-tested against the oracle, and bit-exactly on
 *     exactly representable inputs: tests/test_gpu_conv_exact.py), so
 *     the table changes speed, never values; it is read at launch time and is not thread-safe -- set it before
 *     work is enqueued from other threads, or leave the defaults (what the drop-in surface does).
 *   - returns 0 on success, <0 on error (VM_ERR_*); vm_last_error() gives a thread-local message.
 *   - activation layout is Keras' channels-last.  "padded" tensors are (N, L+2, C) with one zero halo
 *     row before and after each window so that a k=3 SAME convolution reads rows t..t+2 with no branch;
 *     the halo rows are zeroed once by the owner (vm_fill_zero) and never written.
 *   - "towers": BatchNorm statistics are taken per encoder call (voicemap/models.py:52-53 calls the
 *     shared encoder twice), so windows [0,wpt) are tower 0, [wpt,2*wpt) tower 1, ... with
 *     wpt = windows_per_tower.
 */
#ifndef VOICEMAP_HIP_H
#define VOICEMAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* VM_F32S: fp32 storage like VM_F32; the k=3 convolution GEMMs (vm_conv_fwd / vm_conv_dgrad / vm_conv_wgrad) form every product
 * from bf16 hi/lo halves of the fp32 operands (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulation: ~2^-17 relative per product
 * instead of exact) on the bf16 matrix pipe, which is 16x faster than the fp32 one.  Every other entry point treats it as VM_F32. */
/* VM_F16: IEEE half storage (11 significand bits against bf16's 8: ~8x less rounding per stored value at the same bytes and the same
 * matrix-pipe rate, v_mfma_f32_32x32x16_f16).  Every entry point that takes VM_BF16 takes it.  Its exponent range is narrow (6e-8 ..
 * 65504), so the caller scales the loss gradient (vm_siamese_head_loss / vm_softmax_cce `grad_scale`) and un-scales in
 * vm_adam_clip_step (`grad_prescale`); everything between them is linear in the gradient. */
enum { VM_F32 = 0, VM_BF16 = 1, VM_F32S = 2, VM_F16 = 3 };
enum { VM_OK = 0, VM_ERR_ARG = -1, VM_ERR_LAUNCH = -2, VM_ERR_UNSUPPORTED = -3 };
enum { VM_LOSS_CONTRASTIVE = 0, VM_LOSS_BCE = 1 };
enum { VM_HEAD_UNIFORM_EUCLIDEAN = 0, VM_HEAD_WEIGHTED_L1 = 1 };
enum { VM_DIST_EUCLIDEAN = 0, VM_DIST_COSINE = 1, VM_DIST_DOT = 2 };
/* score kinds of vm_pair_score_hist beside the three VM_DIST_*: the weighted_l1 head's sum (voicemap/models.py:55-60 before its bias and
 * sigmoid), and the uniform_euclidean head's distance negated (the order of sigmoid(w d + b) when the head kernel w is negative). */
enum { VM_SCORE_WEIGHTED_L1 = 3, VM_SCORE_NEG_EUCLIDEAN = 4, VM_SCORE_PLDA = 6 };
/* VM_SCORE_PLDA: the score of two PLDA-space rows (vm_plda_project with `quad`; voicemap_amd/plda.py): minus the two-covariance PLDA
 * log-likelihood ratio, lower = more alike.  (The value is 6: 5 stays an unknown kind, which every scorer refuses with VM_ERR_ARG as before
 * -- callers rely on that refusal.)  A row of width E (E % 4 == 0 and 4 <= E <= 256, else VM_ERR_ARG) holds its own term h in its
 * LAST column.  For rows i, j:
 *   acc = the dot kinds' chain: fmaf over components 0 .. E - 2 in ascending order, from 0;
 *   t = h_i + h_j;  s = t - acc;  in fp32, each rounded on its own.
 * NaN handling follows the dot kinds; a row term that is not finite (inf or NaN) gives a NaN score whichever side the row is on.
 * Accepted by vm_pairdist_argmin, vm_pair_score_hist, vm_pair_score_hist_norm, vm_cohort_topk_stats, vm_pair_calib_sums and vm_ahc, with
 * bit-identical scores in all of them; `weights` is not read.  vm_mine_pairs, the n-shot entry points and the speaker models (vm_speaker_*)
 * do not take it: PLDA is a back end, not a training signal, and a speaker model of several rows is not a PLDA-space row -- speaker
 * models are scored by the book by vm_plda_speaker_identify / vm_plda_speaker_trial_hist below. */

const char* vm_last_error(void);
/* 11.  History: 11 = vm_program_run / vm_program_table_hash, the native runner of a recorded step (round 6), and since then, additive within 11: vm_pair_score_hist[_workspace_bytes] (all-pairs verification histograms), vm_cohort_topk_stats / vm_cohort_stats_workspace_bytes / vm_pair_score_hist_norm (cohort score normalisation, S-norm / AS-norm), the *_varlen forward entry points (whole utterances in length-masked buckets: vm_crop_decimate_whiten_varlen, vm_conv1_fused_fwd_varlen, vm_conv_fwd_pool_varlen, vm_bn_drop_pool_fwd_varlen, vm_bn_drop_pool_gmax_fwd_varlen, vm_global_maxpool_fwd_varlen), VM_SCORE_PLDA / vm_scatter_f64[_workspace_bytes, _chunk_rows] / vm_plda_project (the PLDA back end), vm_plda_speaker_identify / vm_plda_speaker_trial_hist[_workspace_bytes] (multi-session PLDA speaker models), vm_speaker_loo_sums / vm_[plda_]speaker_cohort_stats / vm_[plda_]speaker_trial_hist_norm[_workspace_bytes] (S-norm / AS-norm of speaker-model trials); 10 = config 4's log-mel image at twice the storage significand (vm_stft_logmel_f16s_split, vm_conv2d_first_fwd_split, vm_conv2d_first_bn_pool_stack, vm_bn_pool2d_stack_fwd_split) (round 6); 9 = the last block in pair form (vm_bn_drop_pool_gmax_partials_e, vm_bn_bwd_gmax_finalize_e, vm_bn_pool_bwd_apply_pairs_gmax) (round 6); 8 = vm_mfma_rate_probe[_flops], vm_bn_bwd_gmax_finalize; vm_pairdist_workspace_bytes grew by the scalar-path copy of the queries (round 6); 7 = the fused tail (vm_tail_fwd_bwd, vm_tail_param_grads, vm_bn_drop_pool_gmax_partials), vm_event_* / vm_stream_wait_event, centred tiles (`ctr_out` of vm_fold_bn_weights, `e_center` of vm_conv_fwd_fold / vm_bn_pool_bwd_apply_pairs, `tile_center` of vm_bn_finalize) (round 5); 6 = packed weights (vm_pack_nt_weights[_batch]; the `*_packed` argument of vm_conv_fwd_fold / vm_conv_fwd_pool /
 * vm_conv_dgrad_bnred; `bias`, `wf_packed` and the fourth hb row of vm_fold_bn_weights), the centred block-1 extreme (`center_bias` /
 * `shift_adj` / `mean_adj` of vm_bn_finalize) (round 4).  Earlier: 1 = round 1; 2 = vm_bn_finalize gained the zero-debias arguments (round 2); 3 = VM_F16, `dtype` in vm_conv1_fused_*,
 * `grad_scale` in the loss entry points, `skip_nonfinite` in vm_adam_clip_step, vm_embed_* / vm_pairdist_* (round 3); 4 = the folded-BatchNorm training forward
 * (vm_fold_bn_weights, vm_conv_fwd_fold, vm_conv_wgrad_fold, vm_du_tower_sums, vm_bn_pool_bwd_apply_pairs; vm_conv1_fused_fwd mode 2;
 * `wt` in vm_prep_conv_weights_batch; `sqnorm_parts` in vm_adam_clip_step; vm_siamese_head_reduce; vm_conv_fwd_flat, vm_conv2d_first_*,
 * `src_padded` in vm_fold_windows) (round 3); 5 = vm_bn_pool2d_stack_fwd, vm_fold_pool_windows_bwd, vm_colsum_strided, the operand-order basis of
 * vm_stft_split_basis (round 3). */
int vm_abi_version(void);
/* device smoke: hipGetDeviceProperties gcnArchName must start with "gfx950". */
int vm_check_device(void);

int vm_fill_zero(void* ptr, int64_t bytes, void* stream);
/* Stream-ordering primitives (hipEventCreateWithFlags(DisableTiming) / hipEventRecord / hipStreamWaitEvent) for a host that REPLAYS a
 * recorded sequence of the calls below with the ordering between its streams (voicemap_amd/engine.py records one training step per
 * configuration -- the reference's train_on_batch, experiments/train_siamese.py:65-94 runs it 500 times per epoch with identical
 * shapes -- and replays it without re-deriving pointers and dispatch decisions: at the reference's batch sizes the step is bound by
 * the host).  event_out receives an opaque handle. */
int vm_event_create(void** event_out);
int vm_event_destroy(void* event);
int vm_event_record(void* event, void* stream);
int vm_stream_wait_event(void* stream, void* event);
/* A recorded training step made from C (round 6).  The Python side records the C-ABI calls of one step -- entry point, argument list,
 * event records / waits between its streams -- and replays that list while the configuration stays the same (voicemap_amd/program.py
 * Program; the reference runs the same train_on_batch 500 times an epoch, experiments/train_siamese.py:65-94).  At the reference's own
 * batch sizes the step is bound by the host making ~70 calls, and ~1.5 us of each is the binding's argument marshalling: vm_program_run
 * takes the list as int64 words  [function id, argc, argument words ...]*  (pointers and integers as they are, floats / doubles as their
 * bits) and makes the calls itself, in order, stopping at the first non-zero return code (its word index in *fail_at).  Function ids are
 * positions in the name-sorted table of int-returning entry points whose arguments are pointers / int / int64_t / float / double
 * (csrc/program_run.hip, generated by tools/gen_program_run.py from the prototypes of this header); vm_program_table_hash() identifies that table so
 * that a binding generated from another one refuses to run. */
int vm_program_run(const int64_t* words, int64_t n_words, int64_t* fail_at);
int64_t vm_program_table_hash(void);
/* Measurement aid (round 6; not part of the drop-in surface, bench.py only): every SIMD of the device issuing dense
 * v_mfma_f32_32x32x16 (VM_BF16 / VM_F16 operands, non-zero values) back to back from registers for `iters` x 8 instructions per
 * wave -- the rate the part SUSTAINS under its power limit, which the step's GEMM launches (they run on that limit) are priced
 * against beside the nominal 2.5 PFLOP/s.  sink: 512 * 256 floats (never written).  vm_mfma_rate_probe_flops: the FLOPs of one launch. */
int vm_mfma_rate_probe(int dtype, int iters, float* sink, void* stream);
int64_t vm_mfma_rate_probe_flops(int iters);
/* Kernel-selection table for the tests that pin a fallback kernel and for A/B measurements (process-global, see the conventions
 * above; not part of the drop-in surface: voicemap_amd never calls it outside bench.py --tune).  Unknown keys / values out of
 * range return VM_ERR_ARG.  Keys:
 *   "nt_n2" 0..3      forward / dgrad, 16-bit storage: conv_nt2r_kernel (254 x 128 tiles, two workgroups per CU, input-resident A
 *                     by LDS-DMA; bit 0 forward, bit 1 dgrad; default 3); where it is off or does not serve the shape:
 *   "nt3" 0..3, "nt3_lean" 0..3   conv_nt3_kernel (weights L2 -> registers from the packed copy) for forward (bit 0) / dgrad (bit 1) where
 *                     the packed weights are given, and its lean prologue (defaults 3, 3); off: conv_nt2r_kernel
 *   "nt_glds" 0|1     the 128 x 128 LDS-DMA kernel where K * sizeof(T) % 64 == 0 (default 1), else the register-staged 128 x 128 one
 *   "tn_x" 0|1        wgrad, 16-bit storage: the input-resident (3 taps x 128 ci) x 128 co LDS-DMA tile (default 1), else
 *   "tn9" 0|1         ... with the free-running K loop (conv_tn9_kernel, default 1) or the READ / MFMA slots (conv_tn8x_kernel)
 *   "tn9_stages" 0|1  conv_tn9_kernel's split-K ranges are 64-position stages of a tower's window stream (default 1: the launch is
 *                     balanced to one stage) or whole windows.  Changes vm_conv_wgrad_splits / vm_conv_wgrad_workspace_bytes: set it
 *                     before plans are sized
 *   "tn_tile" 128|256 the tile of the register-transposing wgrad kernels (default 256 where the layer is wide enough)
 *   "fuse_finalize" mask 0..31   which two-stage column reductions finish inside their stage-1 launch (the last-arriving workgroup of
 *                     a channel block runs the finalize; bit-identical to the two launches): bit 0 vm_bn_finalize, bit 1
 *                     vm_bn_bwd_finalize / vm_bn_bwd_from_sums_finalize, bit 2 vm_colsum*, bit 3 vm_du_tower_sums, bit 4 = only where
 *                     the reduction is narrow and short (C <= 128, <= 4096 rows per tower).  Default 17: the statistics of small
 *                     layers -- a saved launch pays only there (measurements in bnpool.hip)
 *   "f1_blocks", "f1_fwd_blocks"   target workgroup counts of the fused block-1 kernels (launch geometry; the fp32 partial sums of a
 *                     window are grouped differently, i.e. results change in the last bits; defaults 1024, 1024).
 *   "f1_products" 1|2|3   (round 6; VM_F16 storage only -- VM_BF16 always takes 3) the 16-bit products that carry the block-1
 *                     convolution: 3 = waveform and filters split hi + lo in bf16 (xh*wh + xl*wh + xh*wl, ~16 significand bits of
 *                     both); 2 (default) = the waveform rounded to half, the filters split hi + lo in halves (xh*wh + xh*wl); 1 =
 *                     xh*wh.  NOT result-preserving: it is the operand precision of block 1 (embeddings against the CPU oracle at the
 *                     bench batch 6.98e-4 / 7.37e-4 / 7.99e-4, profiles/r06_block1_products.txt).
 *   "apply_order" 0|1|2   walk of vm_bn_pool_bwd_apply* over the windows: 0 = the segments of all windows together, 1 / 2 =
 *                     window-major ascending / descending (default 2: it starts on the windows the producer of dp wrote last, which the
 *                     memory-side cache still holds).  Bit-identical. */
int vm_set_tuning(const char* key, int value);

/* ---- a6: preprocess_instances / whiten  (voicemap/utils.py:22-34, 88-101) --------------------------
 * raw: (n_windows, raw_len) fp32 (or int16 if raw_is_i16, scaled by 1/32768).  Takes every
 * `downsampling`-th sample (utils.py:29), subtracts the per-window mean (utils.py:94-95) and multiplies
 * by ONE scalar per tower rms/sqrt(mean(batch^2)) of the un-centred decimated batch (utils.py:98).
 * out: (n_windows, L0 + 31) fp32 = the conv-1 input with its SAME halo (15 zeros left, 16 right).
 * ws: >= vm_decimate_whiten_workspace_bytes(n_windows).  whitening=0 skips utils.py:30-31. */
int64_t vm_decimate_whiten_workspace_bytes(int64_t n_windows);
int vm_decimate_whiten(const void* raw, int raw_is_i16, int64_t n_windows, int64_t raw_len, int downsampling,
                       int whitening, float rms, int64_t windows_per_tower, float* out, void* ws, void* stream);
/* The same with the crop of voicemap/librispeech.py:103-137 done on the device: `audio` is a resident buffer of decoded
 * recordings (int16 or fp32, all files back to back -- voicemap_amd/shards.py), window n is the raw_len samples starting at
 * audio[offsets[n]] (offsets: n_windows int64 on the device).  The host only chooses the offsets. */
int vm_crop_decimate_whiten(const void* audio, int raw_is_i16, const int64_t* offsets, int64_t n_windows, int64_t raw_len,
                            int downsampling, int whitening, float rms, int64_t windows_per_tower, float* out, void* ws,
                            void* stream);
/* Whole utterances (encoder.predict on a recording of any length, voicemap/models.py:6-41 with input_shape=None): window n is the
 * raw_lens[n] samples at audio[offsets[n]] (both n_windows int64 on the device), decimated to Ln = ceil(raw_lens[n] / ds) <= L0 samples
 * and whitened ALONE (windows_per_tower = 1: its own mean and scale, fp64 sums over its own Ln samples).  out: (n_windows, L0 + 31);
 * every position past Ln is zero (conv 1's SAME padding).  No sample at or past raw_lens[n] is read.  With every raw_lens[n] equal to
 * raw_len, bit-identical to vm_crop_decimate_whiten(..., windows_per_tower = 1).  ws: vm_decimate_whiten_workspace_bytes(n_windows).
 *
 * Length masking, the rule of every *_varlen entry point: the windows of a bucket share the padded length L0 and carry their valid
 * length lens[n] (int32, device) at the input of the launch.  Every pooled row at or past floor(lens[n] / pool) is written as ZERO --
 * it is the next convolution's SAME padding -- and the global max sees valid rows only.  Valid rows are then exactly what the
 * encoder computes on the recording alone: a valid conv row reads at most one row past the valid length, which is that zero.  The
 * plain GEMM convolutions (vm_conv_fwd, vm_conv1_fwd) need no varlen form: their rows past lens[n] are computed and never read. */
int vm_crop_decimate_whiten_varlen(const void* audio, int raw_is_i16, const int64_t* offsets, const int64_t* raw_lens,
                                   int64_t n_windows, int64_t L0, int downsampling, int whitening, float rms, float* out, void* ws,
                                   void* stream);

/* Waveform augmentation inside the crop (device-resident training only; voicemap_amd/augment.py augment_reference states it in
 * float64).  Window n is the raw_len samples s[t] = audio[offsets[n] + t]; everything is defined at the decimated positions
 * i = 0..L0-1 (t = i * downsampling), the only samples the network sees:
 *   reverb  a_i = sum_{j=0}^{min(i ds, R-1)} r[j] s[i ds - j],  r = rirs[rir_id[n]] (R fp32 taps, causal, direct path at tap 0); zero
 *           history before the crop start; rir_id[n] < 0: a_i = s[i ds].  A decimating FIR: L0 * R multiply-adds per window, fp32 VALU
 *           with fp32 accumulation (the one fp32 part); windows without an RIR run none of it.
 *   noise   v_i = sum_{k<K} noise[noise_offsets[n * K + k] + i ds] (K launch-wide; `noise` a resident buffer like `audio`, which it
 *           may be);  g = sqrt(Pa / (Pv snr_lin[n])) with Pa, Pv the means of a_i^2, v_i^2;  g = 0 if K == 0, Pa == 0, Pv == 0 or
 *           snr_lin[n] <= 0 (the host passes 10^(snr_dB / 10); no transcendental on the device).
 *   gain    y_i = gain[n] (a_i + g v_i)
 *   then the whitening of vm_decimate_whiten on y (per-window mean, one scale per tower, the 15 / 16 zero halo).
 * Every sum, g and the whitening are fp64 in a fixed order: launches are bit-reproducible, and with K = 0, every rir_id < 0 (or
 * n_rirs = 0) and gain = 1 the output is vm_crop_decimate_whiten's bit for bit.  No sample before audio[offsets[n]] or at / past
 * audio[offsets[n] + raw_len] is read, and none off the decimated grid unless the window has an RIR.  snr_lin, gain: n_windows fp32;
 * rir_id: n_windows int32; noise_offsets: (n_windows, K) int64 -- all on the device.  K == 0 permits noise = noise_offsets = NULL,
 * n_rirs == 0 permits rirs = rir_id = NULL; R <= 8192.  ws: >= vm_crop_augment_workspace_bytes(n_windows, L0). */
int64_t vm_crop_augment_workspace_bytes(int64_t n_windows, int64_t L0);
int vm_crop_augment_decimate_whiten(const void* audio, int raw_is_i16, const int64_t* offsets, int64_t n_windows, int64_t raw_len,
                                    int downsampling, int whitening, float rms, int64_t windows_per_tower, const void* noise,
                                    int noise_is_i16, const int64_t* noise_offsets, int K, const float* snr_lin, const float* gain,
                                    const float* rirs, int n_rirs, int R, const int32_t* rir_id, float* out, void* ws, void* stream);

/* ---- voice activity detection on the resident int16 corpus (voicemap_amd/csrc/vad.hip; voicemap_amd/vad.py vad_reference is the
 * numpy statement, matched bit for bit).  Utterance u: the lens[u] int16 samples s[0..len-1] at audio[offsets[u]], 1 <= len < 2^31,
 * cut into F = ceil(len / frame) frames of n_f = min(frame, len - f frame) samples.  frame_base: n_utts + 1 entries, the exclusive
 * cumulative sum of F (the host holds the lengths); energy, mask (one byte per frame) and dst are flat over all frames, utterance u's at
 * frame_base[u]..frame_base[u + 1].
 *   E_f = sum of s_t^2 over frame f, T = sum_f E_f (int64).  With D() = int64 -> double and * = one IEEE double multiply, frame f is active
 *   a_f = E_f > 0  &&  D(E_f) * D(len) >= rel * (D(T) * D(n_f))  &&  D(E_f) >= floor_e * D(n_f)      (rel = 10^(-dB / 10) from the host)
 *   p_f = some g in [f - min_run + 1, f], g >= 0, g + min_run - 1 <= F - 1, with a_g .. a_{g + min_run - 1} all set   (short bursts dropped)
 *   v_f = some g in [max(0, f - hang), min(F - 1, f + hang)] with p_g                                                   (hangover)
 *   V = sum_f v_f n_f;  V < min_keep: the utterance is kept whole -- every v_f = 1, V = len, fallback = 1
 *   dst_f = sum_{g < f} v_g n_g;  mask = v, new_lens[u] = V, info (n_utts, 4) = F, sum a, sum v (after the fallback), fallback.
 * Two launches (energies over tiles of the flat frame list; then one workgroup per utterance, in grid.x), no atomics, bit-reproducible.
 * No sample outside [offsets[u], offsets[u] + lens[u]) is read.  1 <= frame <= 4096, 1 <= min_run <= 64, 0 <= hang <= 256 (so
 * E_f <= 2^42, T < 2^61), else an error and no launch; n_utts == 0 returns without a launch. */
int vm_vad_frames(const void* audio, const int64_t* offsets, const int64_t* lens, const int64_t* frame_base, int64_t n_utts,
                  int frame, double rel, double floor_e, int min_run, int hang, int64_t min_keep,
                  int64_t* energy, void* mask, int64_t* dst, int64_t* new_lens, int32_t* info, void* stream);
/* The trimmed corpus of vm_vad_frames' mask / dst: out[new_offsets[u] + dst_f + t] = s[f frame + t] for every frame with v_f = 1, t < n_f
 * (the kept frames of every utterance in order); new_offsets: the host's exclusive cumulative sum of new_lens.  One launch; 16-byte
 * stores on the aligned body of a frame's destination, 2-byte accesses on its edges; nothing outside a kept frame is read. */
int vm_vad_compact(const void* audio, const int64_t* offsets, const int64_t* lens, const int64_t* frame_base, const void* mask,
                   const int64_t* dst, const int64_t* new_offsets, int64_t n_utts, int frame, void* out, void* stream);

/* ---- speed perturbation of the resident int16 corpus (voicemap_amd/csrc/speed.hip; voicemap_amd/speed.py resample_reference is the
 * numpy statement, matched bit for bit): an integer polyphase resampler by U / D, U output samples per D input samples.  Utterance u:
 * the lens[u] >= 0 int16 samples x[0..len-1] at audio[offsets[u]]; taps: U T int32 on the device, c = U T / 2;
 *   n_out  = ceil(len U / D)
 *   acc[m] = sum over 0 <= k < len with 0 <= m D + c - k U < U T of taps[m D + c - k U] x[k]                 (int64)
 *   out[new_offsets[u] + m] = clip((acc[m] + (1 << (shift - 1))) >> shift, -32768, 32767)   (arithmetic shift; shift = 0 adds nothing)
 * out_base: n_utts + 1 entries ON THE DEVICE, the exclusive cumulative sum of n_out (the host knows every length in closed form: no
 * read-back); new_offsets[u]: where utterance u's output starts in out, in any order.  phase_abs_max: an upper bound on
 * max_p sum_i |taps[p + i U]|, below 2^47; the accumulator is 32 bits wide only where it proves that exact (phase_abs_max < 2^16) and 64
 * bits wide otherwise.  One launch over tiles of the flat output list (a fixed grid in x, a tile's utterance found by binary search of
 * out_base), no atomics, bit-reproducible; no sample outside [offsets[u], offsets[u] + lens[u]) is read and nothing outside the n_out
 * outputs of an utterance is written.  1 <= U, D, T <= 64, 0 <= shift <= 30, else an error and no launch; n_utts == 0 returns without a
 * launch. */
int vm_resample_i16(const void* audio, const int64_t* offsets, const int64_t* lens, const int64_t* out_base, int64_t n_utts,
                    int U, int D, const int32_t* taps, int T, int shift, int64_t phase_abs_max,
                    const int64_t* new_offsets, void* out, void* stream);

/* ---- a1 block 1: Conv1D(filters, 32, padding='same', activation='relu')  (voicemap/models.py:13-16) --
 * x: (n_windows, L + 31) fp32 from vm_decimate_whiten; w: (32, 1, F) fp32 Keras layout; bias (F).
 * z: (n_windows, L, F) `dtype`, = relu(conv + bias).  If stat_sum != NULL also writes per-(window, tile)
 * partial sums of z and z^2 (fp32) for the BatchNorm that follows: stat_sum/stat_sq are
 * (n_windows * vm_conv1_stat_rows(L), F). */
int64_t vm_conv1_stat_rows(int64_t L);
int vm_conv1_fwd(const float* x, const float* w, const float* bias, int64_t n_windows, int64_t L, int F,
                 int dtype, void* z, float* stat_sum, float* stat_sq, void* stream);
/* wgrad of block 1: dW[k][c] = sum_{n,t} x[n][t+k] * du[n][t][c] over all windows.
 * du: (n_windows, L+2, F) padded `dtype`.  ws: vm_conv1_wgrad_workspace_bytes() of scratch for the per-window partials;
 * grad_w (32,1,F) is overwritten with the fixed-order sum (deterministic). */
int64_t vm_conv1_wgrad_workspace_bytes(int64_t n_windows, int F);
int vm_conv1_wgrad(const float* x, const void* du, int64_t n_windows, int64_t L, int F, int dtype,
                   float* ws, float* grad_w, void* stream);

/* Fused block 1 for 16-bit storage (dtype VM_BF16 or VM_F16; voicemap/models.py:13-19: Conv1D(F,32) -> BatchNormalization -> SpatialDropout1D ->
 * MaxPool1D(pool)): the full-resolution relu(conv) tensor is never written.
 *   training (inference = 0): out = e (n_windows, L/pool, F) bf16 = per-pool-window max (gamma >= 0) or min (gamma < 0) of
 *     relu(conv+b), rounded to bf16 -- BN is a monotone per-channel affine, so pooling commutes with it; the affine +
 *     dropout are then applied to e by vm_bn_drop_pool_fwd(z = e, L = L/pool, pool = 1).  gamma_or_scale = gamma (F);
 *     shift ignored; stat_sum / stat_sq as for vm_conv1_fwd (over all L positions), taken from the fp32 accumulator:
 *     relu(conv+b) itself is never stored, so it has no storage rounding -- the statistics, the pool arg-max and the
 *     backward recompute all see the same fp32 values.
 *   inference (inference = 1): out = padded act (n_windows, L/pool + 2, F) bf16 = bf16(extreme * scale + shift);
 *     gamma_or_scale = scale, shift from vm_bn_infer_affine.
 *   training, padded extreme (inference = 2): as 0, but e is written as a padded activation tensor (n_windows, L/pool + 2, F), rows
 *     1 .. L/pool (halo rows untouched: the caller zeroes them once) -- the input layout of vm_conv_fwd_fold.
 * pool: 2 or 4. */
int vm_conv1_fused_fwd(const float* x, const float* w, const float* bias, const float* gamma_or_scale, const float* shift,
                       int64_t n_windows, int64_t L, int F, int pool, int inference, int dtype, void* out, float* stat_sum,
                       float* stat_sq, void* stream);
/* mode 1 (inference) over a length-masked bucket (see vm_crop_decimate_whiten_varlen): lens[n] = the valid positions of window n's
 * input x; pooled rows at or past lens[n] / pool are zero (+0, whatever x holds past the last tap of position (lens[n] / pool) * pool - 1,
 * NaN included) and a 32-position tile past the last valid pool group runs no MFMA.  lens[n] < pool: the whole window is zero;
 * lens[n] > L counts as L.  The halo rows 0 and L / pool + 1 are the caller's in every case.  With every lens[n] == L the output is
 * bit-identical to mode 1 of vm_conv1_fused_fwd. */
int vm_conv1_fused_fwd_varlen(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                              const int32_t* lens, int64_t n_windows, int64_t L, int F, int pool, int dtype, void* out, void* stream);
/* Backward of the same block from dp (n_windows, L/pool, F) `dtype`: recomputes the conv tile on the matrix cores,
 * evaluates the pool/dropout/BN/ReLU backward in registers (c1, c2 from vm_bn_pool_bwd_reduce(z = e, pool = 1) +
 * vm_bn_bwd_finalize(count = wpt*L)) and accumulates grad_w (32,1,F) and grad_b (F) (overwritten; fixed order). */
int64_t vm_conv1_fused_bwd_workspace_bytes(int64_t n_windows, int64_t L, int F);
int vm_conv1_fused_bwd(const float* x, const float* w, const float* bias, const void* dp, const float* scale,
                       const float* mean, const float* invstd, const float* drop, const float* c1, const float* c2,
                       int64_t n_windows, int64_t windows_per_tower, int64_t L, int F, int pool, int dtype, void* ws,
                       float* grad_w, float* grad_b, void* stream);

/* ---- a1 blocks 2-4: Conv1D(c_out, 3, padding='same', activation='relu')  (voicemap/models.py:22,27,32)
 * implicit GEMM on MFMA.  in: padded (n_windows, L+2, c_in) `dtype`; wf: (c_out, 3*c_in) `dtype` from
 * vm_prep_conv_weights; z: (n_windows, L, c_out) `dtype`.  stat_* as for vm_conv1_fwd with
 * vm_conv_stat_rows(L) rows per window (NULL in inference). */
int64_t vm_conv_stat_rows(int64_t L);
int vm_conv_fwd(const void* in, const void* wf, const float* bias, int64_t n_windows, int64_t L, int c_in,
                int c_out, int dtype, void* z, float* stat_sum, float* stat_sq, void* stream);
/* vm_conv_fwd for windows too short to fill a tile (the 2-D variant: 149 .. 37 positions): every window of `in` carries its own zero
 * halo rows, so the concatenation of all windows is one valid k = 3 sequence; it is run as ONE window on the 128-row kernels and the
 * epilogue drops the halo positions (their results are junk) and writes the rest to the same un-padded z (n_windows, L, c_out) --
 * bit-identical to vm_conv_fwd.  stat_sum / stat_sq: vm_conv_flat_stat_rows(n_windows, L) rows in all (one per 128 rows of the
 * concatenation) instead of vm_conv_stat_rows(L) per window: a caller with BatchNorm statistics per tower launches once per tower. */
int64_t vm_conv_flat_stat_rows(int64_t n_windows, int64_t L);
int vm_conv_fwd_flat(const void* in, const void* wf, const float* bias, int64_t n_windows, int64_t L, int c_in, int c_out, int dtype,
                     void* z, float* stat_sum, float* stat_sq, void* stream);
/* vm_conv_fwd (training form: statistics required) that also writes the pool-window extreme of z for MaxPool1D(2):
 * e[n][q][c] = max(z[n][2q][c], z[n][2q+1][c]) where gamma[c] >= 0, the min where gamma[c] < 0 -- the element the max-pool of the
 * BatchNorm output will select, known before the statistics are (sign(scale) = sign(gamma)).  e: unpadded (n_windows, L/2, c_out).
 * vm_bn_drop_pool_fwd(e, ..., L/2, pool = 1) then gives the bit-identical pooled output from a pooled-size tensor, and
 * vm_conv_dgrad_bnred can take its sums against e directly (red_a_padded = 0).  Same kernel restriction as vm_conv_fwd_pool. */
int vm_conv_fwd_e_supported(int64_t n_windows, int64_t L, int c_in, int c_out, int dtype);
int vm_conv_fwd_e(const void* in, const void* wf, const float* bias, const float* gamma, int64_t n_windows, int64_t L,
                  int c_in, int c_out, int dtype, void* z, float* stat_sum, float* stat_sq, void* e, void* stream);
/* Training forward WITHOUT the BatchNorm / pool pass between two blocks (dropout rate 0).  The max-pool of a BatchNorm output picks
 * the pool-window extreme e of the conv output (vm_conv_fwd_e, vm_conv1_fused_fwd), and BatchNorm is a per-channel affine
 * y = scale[c] * e + shift[c] -- so the next Conv1D can read e itself with the affine folded into its weights:
 *     conv(y)[t][co] = sum_k sum_ci (W[k][ci][co] * scale[ci]) * e[t + k - 1][ci]  +  bias[co] + sum_{k inside} hb[k][co],
 *     hb[k][co] = sum_ci W[k][ci][co] * shift[ci];   tap 0 is outside the window at t = 0, tap 2 at t = L - 1 (SAME pads y with 0).
 * BatchNorm statistics are per encoder call ("tower": windows [t * windows_per_tower, (t + 1) * windows_per_tower)), so there is one
 * set of folded weights per tower.  vm_fold_bn_weights: wt = the fp32 kernel in wf's layout (c_out, 3 * c_in) (the `wt` output of
 * vm_prep_conv_weights_batch) + scale / shift (towers, c_in) + the layer's bias (c_out) -> wf_folded (towers, c_out, 3 * c_in) `dtype`
 * and / or wf_packed (the same values in vm_pack_nt_weights' fragment order; either may be NULL) and hb (towers, 4, c_out) fp32: rows
 * 0..2 the per-tap constants, row 3 = bias + their sum (what the accumulators of vm_conv_fwd_fold start from).  vm_conv_fwd_fold: hb
 * as written by vm_fold_bn_weights (its `bias` argument is not read: row 3 of hb carries it); wf_packed (optional): the fragment-
 * order copy, used where the shape has a conv_nt3_kernel (128 / 256 / 384 / 512 input channels);  in_e = padded extreme (n_windows, L + 2, c_in) of the layer below (zero halo
 * rows), z / stat_* as vm_conv_fwd; e (optional) = this layer's own extreme for MaxPool1D(2), PADDED (n_windows, L/2 + 2, c_out), the
 * maximum where gamma >= 0 else the minimum.  16-bit storage, conv_nt2r_kernel shapes only (vm_conv_fwd_fold_supported).  The
 * pooled BatchNorm output is never materialised: -1 read and -1 write of it per block and no pass over z in the forward.
 * o (optional, with e): the OTHER element of every position pair, unpadded (n_windows, L/2, c_out), with its sign bit set where the
 * extreme is the pair's second element (z >= 0 after the ReLU: the bit is free; ties: the first element is the extreme).  (e, o)
 * together are z, so with o given z is NOT written and may be NULL -- the epilogue stores as many bytes as a plain forward --
 * and the backward takes the pair form (vm_bn_pool_bwd_apply_pairs).
 * vm_conv_wgrad_fold is the matching weight gradient, vm_conv_dgrad[_bnred] is unchanged (it takes the un-folded wd). */
int vm_fold_bn_weights(const float* wt, const float* scale, const float* shift, const float* bias, int towers, int c_in, int c_out,
                       int dtype, void* wf_folded, void* wf_packed, float* hb, float* ctr_out, void* stream);
/* ctr_out (towers, c_out) or NULL (round 5): the centre of each output channel's tile for vm_conv_fwd_fold's `e_center` --
 * ctr = max(row 3 of hb, 0) rounded to the storage type (the pedestal the accumulators start from: conv bias + the contribution of
 * the input's BatchNorm shifts); row 3 of hb is then written with ctr already taken off. */
int vm_conv_fwd_fold_supported(int64_t n_windows, int64_t L, int c_in, int c_out, int dtype, int with_e);
int vm_conv_fwd_fold(const void* in_e, const void* wf_folded, const float* bias, const float* hb, const float* gamma,
                     int64_t n_windows, int64_t windows_per_tower, int64_t L, int c_in, int c_out, int dtype, void* z, float* stat_sum,
                     float* stat_sq, void* e, void* o, const void* wf_packed, const float* e_center, void* stream);
/* e_center (towers, c_out) or NULL (round 5; VM_F16 with the (e, o) output only): vm_fold_bn_weights' ctr_out.  The tile is computed
 * and rounded CENTRED: t = relu(z) - ctr, one rounding of a value whose size is the distance from the channel's pedestal instead of
 * the pedestal (a half spends its 11 bits on the latter otherwise: 1.06e-3 -> 0.66e-3 on the embeddings of the trained-like state of
 * tests/test_gpu_fullsize_oracle.py).  e receives the centred extreme, o the other element UN-centred (so that its sign bit stays
 * free for the position flag), stat_sum / stat_sq the sums of t and t^2: vm_bn_finalize's tile_center, vm_bn_pool_bwd_apply_pairs'
 * e_center and the *_adj constants take it from there. */
/* The k = 3 GEMM weights in the order the matrix cores consume them (round 4).  bt: `towers` matrices (n_rows, 3 * a_c) `dtype` back
 * to back -- wf (n_rows = c_out, a_c = c_in), wd (n_rows = c_in, a_c = c_out) of vm_prep_conv_weights, wf_folded of
 * vm_fold_bn_weights; packed: the same elements as [tower][n_rows / 64][K tile = (channel chunk of 32, tap)][32-row half][16-channel
 * half][64 lanes][8 values], i.e. every 1 KB piece is one v_mfma_f32_32x32x16 operand fragment of a wave and a wave's stream through a
 * K loop is contiguous.  The entry points that take a `*_packed` argument (vm_conv_fwd_fold, vm_conv_fwd_pool, vm_conv_dgrad_bnred)
 * then load the weights from L2 straight into registers (conv_nt3_kernel) instead of staging them in LDS; NULL there = the staged
 * kernel.  Same results bit for bit (the same products in the same order).  16-bit storage, n_rows % 128 == 0, a_c % 32 == 0. */
int vm_pack_nt_weights_supported(int n_rows, int a_c, int dtype);
int vm_pack_nt_weights(const void* bt, int towers, int n_rows, int a_c, int dtype, void* packed, void* stream);
/* the same for n (<= 8) matrices in ONE launch: host arrays, one entry per matrix. */
int vm_pack_nt_weights_batch(int n, const void* const* bt, const int* towers, const int* n_rows, const int* a_c, int dtype,
                             void* const* packed, void* stream);
/* inference-mode forward of a whole block in one launch: Conv1D + bias + ReLU, the BatchNorm affine (scale / shift per channel from
 * vm_bn_infer_affine: (c_out) floats each) and MaxPool1D(2), models.py:22-35 with learning_phase 0.  act: padded pooled output
 * (n_windows, L/2 + 2, c_out), halo rows untouched; the conv output z is never written.  Bit-identical to vm_conv_fwd followed by
 * vm_bn_drop_pool_fwd(pool = 2, drop = NULL).  Served by the 256 x 128 input-resident kernel only (16-bit storage, even L):
 * vm_conv_fwd_pool_supported() says whether a shape is, VM_ERR_UNSUPPORTED otherwise. */
int vm_conv_fwd_pool_supported(int64_t n_windows, int64_t L, int c_in, int c_out, int dtype);
int vm_conv_fwd_pool(const void* in, const void* wf, const float* bias, const float* scale, const float* shift,
                     int64_t n_windows, int64_t L, int c_in, int c_out, int dtype, void* act, const void* wf_packed, void* stream);
/* The same over a length-masked bucket (see vm_crop_decimate_whiten_varlen; models.py:22-35): lens[n] = the valid positions of window n.
 * Pooled rows at or past lens[n] / 2 are zero (+0, whatever `in` holds past row 2 * (lens[n] / 2), NaN included); a 254-row tile with
 * no valid pool group writes its zeros and issues no MFMA.  lens[n] < 2: the whole window is zero; lens[n] > L counts as L.  The halo
 * rows of act are the caller's in every case.  With every lens[n] == L the output is bit-identical to vm_conv_fwd_pool's.  Served
 * where vm_conv_fwd_pool_supported() says so. */
int vm_conv_fwd_pool_varlen(const void* in, const void* wf, const float* bias, const float* scale, const float* shift,
                            const int32_t* lens, int64_t n_windows, int64_t L, int c_in, int c_out, int dtype, void* act,
                            const void* wf_packed, void* stream);
/* dgrad: dx[n][t][ci] = sum_{k,co} du[n][t+1-k][co] * W[k][ci][co].  du padded (n_windows, L+2, c_out);
 * wd: (c_in, 3*c_out) `dtype` tap-flipped copy from vm_prep_conv_weights; dx: (n_windows, L, c_in). */
int vm_conv_dgrad(const void* du, const void* wd, int64_t n_windows, int64_t L, int c_in, int c_out, int dtype,
                  void* dx, void* stream);
/* vm_conv_dgrad that also forms, from the output tile it holds on chip, the two sums the BatchNorm backward of the layer BELOW
 * needs (that layer's output gradient is exactly this dx; keras BatchNormalization backward, voicemap/models.py:23,28,33):
 *   red_s0[row][ci] = sum_t dx[n][t][ci],   red_s1[row][ci] = sum_t dx[n][t][ci] * red_a[n][t][ci]
 * as vm_conv_dgrad_bnred_rows(L) partial rows per window (fp32, (n_windows * rows, c_in), every row written).  red_a: a
 * (n_windows, L, c_in) tensor of `dtype` -- the pooled output of the layer below (red_a_padded = 1: stored (L + 2) rows with a
 * halo row either side, as vm_bn_drop_pool_fwd writes it) or its pool-window extreme (red_a_padded = 0).  dx is written as by
 * vm_conv_dgrad (the sums use dx as rounded to `dtype`).  Served by the 256 x 128 input-resident kernel only:
 * vm_conv_dgrad_bnred_supported() says whether the shape / dtype / current tuning is, VM_ERR_UNSUPPORTED otherwise.
 * vm_bn_bwd_from_sums turns the rows into the partials vm_bn_bwd_finalize takes, replacing vm_bn_pool_bwd_reduce[_pooled]. */
int64_t vm_conv_dgrad_bnred_rows(int64_t L);
int vm_conv_dgrad_bnred_supported(int64_t n_windows, int64_t L, int c_in, int c_out, int dtype);
int vm_conv_dgrad_bnred(const void* du, const void* wd, int64_t n_windows, int64_t L, int c_in, int c_out, int dtype,
                        void* dx, const void* red_a, int red_a_padded, float* red_s0, float* red_s1, const void* wd_packed,
                        void* stream);
/* wgrad: dW[k][ci][co] = sum_{n,t} in[n][t+k][ci] * du[n][t+1][co] (both padded).  Split over windows into
 * vm_conv_wgrad_splits() slabs in ws (fp32), then summed in fixed order into grad_w (3, c_in, c_out). */
int vm_conv_wgrad_splits(int64_t n_windows, int64_t L, int c_in, int c_out);
int64_t vm_conv_wgrad_workspace_bytes(int64_t n_windows, int64_t L, int c_in, int c_out);
int vm_conv_wgrad(const void* in, const void* du, int64_t n_windows, int64_t L, int c_in, int c_out, int dtype,
                  void* ws, float* grad_w, void* stream);
/* wgrad of a layer that ran vm_conv_fwd_fold: the layer's true input is y = scale_t[ci] * e + shift_t[ci] inside the window (t = the
 * tower of the window: n_windows / windows_per_tower towers, scale / shift (towers, c_in)), 0 in the padding, hence
 *     dW[k][ci][co] = sum_t scale_t[ci] * (sum_{n in t, pos} e[n][pos+k][ci] * du[n][pos+1][co]) + shift_t[ci] * dsum[t][k][co]
 * -- the same split GEMM on e with every slab inside one tower, then one fixed-order pass that sums the slabs per tower and applies
 * the two factors.  dsum (towers, 3, c_out) from vm_du_tower_sums. */
int64_t vm_conv_wgrad_fold_workspace_bytes(int64_t n_windows, int64_t windows_per_tower, int64_t L, int c_in, int c_out);
int vm_conv_wgrad_fold(const void* in_e, const void* du, int64_t n_windows, int64_t windows_per_tower, int64_t L, int c_in, int c_out,
                       int dtype, const float* scale, const float* shift, const float* dsum, void* ws, float* grad_w, void* stream);
/* dsum == NULL above leaves the slabs in ws (the GEMM needs nothing but e and du, so it can start before vm_du_tower_sums has run);
 * this is the second half: the per-tower slab sums with the two factors applied -> grad_w. */
int vm_conv_wgrad_fold_finish(const void* ws, int64_t n_windows, int64_t windows_per_tower, int64_t L, int c_in, int c_out,
                              const float* scale, const float* shift, const float* dsum, float* grad_w, void* stream);
/* fp32 Keras kernel (3, c_in, c_out) -> wf (c_out, 3*c_in) and wd (c_in, 3*c_out) in `dtype`. */
int vm_prep_conv_weights(const float* w, int c_in, int c_out, int dtype, void* wf, void* wd, void* stream);
/* the same for n_layers (<= 8) layers in ONE launch: host arrays of device pointers / channel counts, one entry per layer.  wt
 * (optional array, entries may be NULL): also the fp32 kernel itself in wf's layout (c_out, 3*c_in) -- what vm_fold_bn_weights reads. */
int vm_prep_conv_weights_batch(int n_layers, const float* const* w, const int* c_in, const int* c_out, int dtype,
                               void* const* wf, void* const* wd, float* const* wt, void* stream);

/* ---- a1-BN: BatchNormalization()  (voicemap/models.py:17,23,28,33; Keras defaults eps 1e-3, momentum .99)
 * Reduces the conv partials per tower in a fixed order (fp64), producing per-tower
 *   mean, invstd = rsqrt(var_biased + eps), scale = gamma*invstd, shift = beta - mean*scale     (each (n_towers, C))
 * and applies the moving-average updates tower by tower:  moving -= (moving - batch) * (1 - momentum), with the
 * batch variance multiplied by n/(n-(1+eps)) first when unbiased_moving_var != 0 (Keras 2.2.x). */
/* ws (all three reducers below): >= vm_colreduce_workspace_bytes(n_segments, C) bytes of scratch for the first of the
 * two deterministic reduction stages (n_segments = n_towers; 1 for vm_colsum).  * zd_biased (n_towers, 2, C) fp32 or NULL: Keras 2.2.2's moving_average_update is TF 1.10's assign_moving_average with
 * zero_debias=True -- per encoder call a zero-initialised biased accumulator b -= (b - value)(1 - momentum) and
 * moving = b * zd_correction with zd_correction = 1 / (1 - momentum^t), t = number of training steps so far (host side); the
 * towers are applied in order.  NULL = the plain exponential average moving -= (moving - value)(1 - momentum). */
int64_t vm_colreduce_workspace_bytes(int n_segments, int C);
int vm_bn_finalize(const float* stat_sum, const float* stat_sq, int64_t rows_per_tower, int n_towers, int C,
                   double count_per_tower, const float* gamma, const float* beta, float eps, float momentum,
                   int unbiased_moving_var, float* moving_mean, float* moving_var, float* mean, float* invstd,
                   float* scale, float* shift, void* ws, float* zd_biased, float zd_correction, const float* center_bias,
                   float* shift_adj, float* mean_adj, const float* tile_center, void* stream);
/* tile_center (n_towers, C) or NULL, exclusive with center_bias (round 5): the layer ran as vm_conv_fwd_fold with `e_center` -- its
 * statistics partials are sums over t = z - ctr and its pool extreme is stored as e - ctr, ctr = tile_center[tower][c].  The sums are
 * taken back to z here (sum z = sum t + n ctr, sum z^2 = sum t^2 + 2 ctr sum t + n ctr^2, fp64) and shift_adj / mean_adj carry the
 * offset for the consumers of the stored extreme exactly as with center_bias. */
/* center_bias (C) or NULL, with shift_adj / mean_adj (n_towers, C): block 1's pool extreme is stored CENTRED in the folded training
 * path (vm_conv1_fused_fwd mode 2 writes e - ctr, ctr = max(conv bias, 0): the whitened waveform makes conv-1 outputs small next to a
 * bias, and a 16-bit value would spend its significand on that pedestal).  Its consumers are linear in e, so the offset moves into
 * their constants: shift_adj = shift + scale * ctr is the shift over the STORED value (vm_fold_bn_weights / vm_conv_wgrad_fold_finish of
 * block 2), mean_adj = mean - ctr the mean against which the sums over the stored value are taken (vm_bn_bwd_from_sums[_finalize]). */
/* inference affine from moving statistics (one "tower"). */
int vm_bn_infer_affine(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                       float eps, int C, float* scale, float* shift, void* stream);

/* BN apply + SpatialDropout1D + MaxPool1D(pool)  (voicemap/models.py:17-19 etc.)
 * y = (z*scale[tower] + shift[tower]) * drop[n][c];  out[n][1+q][c] = max_{j<pool} y[n][q*pool+j][c], q < L/pool.
 * z: (n_windows, L, C); drop: (n_windows, C) fp32 keep-mask/(1-rate) or NULL; out: padded (n_windows, L/pool + 2, C). */
int vm_bn_drop_pool_fwd(const void* z, const float* scale, const float* shift, const float* drop,
                        int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int pool, int dtype,
                        void* out, void* stream);
/* backward, pass 1: partials of sum(dy) and sum(dy*zhat) over the pooled positions, where dy is dp routed to
 * the first maximum of each pool window.  dp: (n_windows, L/pool, C).
 * part_*: (n_windows * vm_bn_part_rows(), C) fp32: every pass kernel fills all vm_bn_part_rows() rows of a window -- one per
 * workgroup of the window for long windows; for short ones (pooled rows x channel vectors < 2 048: the 2-D variant) one workgroup
 * takes the whole window, writes row 0 and zero-fills the others -- so a consumer simply adds all rows. */
int vm_bn_part_rows(void);
int vm_bn_pool_bwd_reduce(const void* z, const void* dp, const float* scale, const float* shift, const float* mean,
                          const float* invstd, const float* drop, int64_t n_windows, int64_t windows_per_tower,
                          int64_t L, int C, int pool, int dtype, float* part_dy, float* part_dyz, void* stream);
/* reduce those partials per tower: c1 = sum(dy)/count, c2 = sum(dy*zhat)/count (each (n_towers, C)); and add the
 * parameter gradients over all towers: grad_gamma = sum(dy*zhat), grad_beta = sum(dy)  (overwritten). */
/* vm_bn_bwd_from_sums followed by vm_bn_bwd_finalize in two launches instead of three and without the (n_windows * part_rows, C) partial
 * tensors in between: the per-window map is applied to the dgrad epilogue's partial rows on their way into the column sums (fp64).
 * Same arguments as the two calls; ws >= vm_colreduce_workspace_bytes(n_towers, C). */
int vm_bn_bwd_from_sums_finalize(const float* s0, const float* sa, int64_t rows_per_window, const void* z, const void* dp,
                                 const float* scale, const float* shift, const float* mean, const float* invstd, const float* drop,
                                 int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, int a_is_act,
                                 double count_per_tower, float* c1, float* c2, float* grad_gamma, float* grad_beta, void* ws,
                                 void* stream);
int vm_bn_bwd_finalize(const float* part_dy, const float* part_dyz, int64_t n_windows, int64_t windows_per_tower,
                       int C, double count_per_tower, float* c1, float* c2, float* grad_gamma, float* grad_beta,
                       void* ws, void* stream);
/* vm_bn_pool_bwd_reduce with the pool-window extreme of z recovered from the POOLED forward output `act` (padded
 * (n_windows, L/pool + 2, C), as written by vm_bn_drop_pool_fwd with the same scale / shift / drop) instead of re-derived from
 * z: ext = act / (scale*drop) - shift/scale.  Reads two pooled-size tensors instead of z + dp; differs from the z form by the
 * storage rounding of act (bit-identical sums are NOT guaranteed; channels with scale == 0 use z).  Throughput-mode option. */
int vm_bn_pool_bwd_reduce_pooled(const void* z, const void* act, const void* dp, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, const float* drop, int64_t n_windows,
                                 int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, float* part_dy,
                                 float* part_dyz, void* stream);
/* the same partials from the sums vm_conv_dgrad_bnred left behind (s0, sa: (n_windows * rows_per_window, C)).  a_is_act = 1:
 * sa was taken against the pooled output, the extreme is recovered as in vm_bn_pool_bwd_reduce_pooled (z is read only for
 * channels with scale == 0); a_is_act = 0: sa was taken against the extreme itself (z may be NULL).  L, pool: this block's
 * pre-pool length and pool size (dp is (n_windows, L / pool, C)). */
int vm_bn_bwd_from_sums(const float* s0, const float* sa, int64_t rows_per_window, const void* z, const void* dp,
                        const float* scale, const float* shift, const float* mean, const float* invstd, const float* drop,
                        int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, int a_is_act,
                        float* part_dy, float* part_dyz, void* stream);
/* backward, pass 2: du[n][1+t][c] = [z>0] * scale * (dy - c1 - zhat*c2)  (padded (n_windows, L+2, C) out), plus
 * partial column sums of du -> part_du (n_windows * vm_bn_part_rows(), C) for the conv bias gradient. */
int vm_bn_pool_bwd_apply(const void* z, const void* dp, const float* scale, const float* shift, const float* mean,
                         const float* invstd, const float* drop, const float* c1, const float* c2,
                         int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int pool, int dtype,
                         void* du, float* part_du, void* stream);
/* The same two passes for the LAST block, with dp given in the sparse form GlobalMaxPool1D's backward produces:
 * dp[n][q][c] = dg[n][c] if q == gidx[n][c] else 0 (dg, gidx as in vm_global_maxpool_fwd/bwd).  Avoids writing and
 * re-reading the dense (n_windows, L/pool, C) tensor (voicemap/models.py:35-37). */
int vm_bn_pool_bwd_reduce_gmax(const void* z, const float* dg, const int32_t* gidx, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* drop, int64_t n_windows,
                               int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, float* part_dy,
                               float* part_dyz, void* stream);
/* vm_bn_pool_bwd_reduce_gmax + vm_bn_bwd_finalize in one launch (round 6; the same sums in fp64, per (tower, channel) by one 32-lane
 * group): c1 / c2 (towers, C), grad_gamma / grad_beta (C) as vm_bn_bwd_finalize writes them (voicemap/models.py:32-37 backward). */
int vm_bn_bwd_gmax_finalize(const void* z, const float* dg, const int32_t* gidx, const float* scale, const float* shift,
                            const float* mean, const float* invstd, const float* drop, int64_t n_windows,
                            int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, double count_per_tower, float* c1,
                            float* c2, float* grad_gamma, float* grad_beta, void* stream);
int vm_bn_pool_bwd_apply_gmax(const void* z, const float* dg, const int32_t* gidx, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const float* drop, const float* c1, const float* c2,
                              int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, void* du,
                              float* part_du, void* stream);
/* vm_bn_pool_bwd_apply for pool = 2 with z given as the pair tensors of vm_conv_fwd_fold: e PADDED (n_windows, L/2 + 2, C), o
 * (n_windows, L/2, C) with the position flag in its sign bit.  Same arithmetic and outputs.  16-bit storage, L even. */
int vm_bn_pool_bwd_apply_pairs(const void* e, const void* o, const void* dp, const float* scale, const float* shift, const float* mean,
                               const float* invstd, const float* drop, const float* c1, const float* c2, int64_t n_windows,
                               int64_t windows_per_tower, int64_t L, int C, int dtype, void* du, float* part_du, const float* e_center,
                               void* stream);
/* e_center (towers, C) or NULL: e was stored centred (vm_conv_fwd_fold e_center); the kernel adds ctr back (fp32) before it applies
 * ReLU's mask and the BatchNorm-backward constants, which stay those of z (mean, not mean_adj). */
/* out[c] = sum_r part[r][c] in fixed order (bias gradients). */
int vm_colsum(const float* part, int64_t rows, int C, float* out, void* ws, void* stream);
/* The part_* tensors have vm_bn_part_rows() rows per window; a pass over short windows (the 2-D variant) fills only the first
 * vm_bn_part_rows_used(L, C, pool, dtype) of them and zeroes the rest.  vm_colsum_strided sums rows 0, row_step, 2 row_step, ...
 * (`rows` of them) -- with row_step = vm_bn_part_rows() the one live row per window instead of eight. */
int vm_bn_part_rows_used(int64_t L, int C, int pool, int dtype);
int vm_colsum_strided(const float* part, int64_t rows, int row_step, int C, float* out, void* ws, void* stream);
/* vm_colsum of the apply pass's part_du (n_windows * vm_bn_part_rows(), C) per tower, plus what vm_conv_wgrad_fold needs:
 * dsum[t][k][c] = sum over the windows of tower t and the positions whose tap k lies inside the window of du[n][pos][c] (k = 1: all
 * positions; k = 0: all but position 0; k = 2: all but position L - 1; du: padded (n_windows, L + 2, C) `dtype`).  grad_b (optional,
 * C) = the sum over all towers (the conv bias gradient).  ws: vm_colreduce_workspace_bytes(towers, C). */
int vm_du_tower_sums(const float* part_du, const void* du, int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int dtype,
                     float* grad_b, float* dsum, void* ws, void* stream);

/* LAST block only: vm_bn_drop_pool_fwd fused with GlobalMaxPool1D (voicemap/models.py:31-37).  The pooled tensor of the
 * last block is never materialised: gmax / gidx are exactly what vm_global_maxpool_fwd would return for it (values rounded
 * to `dtype`, gidx = first maximum).  ws: vm_bn_drop_pool_gmax_workspace_bytes(n_windows, C) bytes. */
int64_t vm_bn_drop_pool_gmax_workspace_bytes(int64_t n_windows, int C);
int vm_bn_drop_pool_gmax_fwd(const void* z, const float* scale, const float* shift, const float* drop, int64_t n_windows,
                             int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, float* gmax, int32_t* gidx,
                             void* ws, void* stream);
/* Inference over a length-masked bucket (see vm_crop_decimate_whiten_varlen; models.py:22-37 with learning_phase 0, no dropout):
 * lens[n] = the valid rows of window n's z, lens[n] >= pool.  vm_bn_drop_pool_fwd_varlen writes zeros at pooled rows >= lens[n] / pool;
 * vm_bn_drop_pool_gmax_fwd_varlen takes the global max over pooled rows < lens[n] / pool only (gidx a valid row).  Every storage mode
 * and odd lengths: the shapes the fused launches do not serve. */
int vm_bn_drop_pool_fwd_varlen(const void* z, const float* scale, const float* shift, const int32_t* lens, int64_t n_windows, int64_t L,
                               int C, int pool, int dtype, void* out, void* stream);
int vm_bn_drop_pool_gmax_fwd_varlen(const void* z, const float* scale, const float* shift, const int32_t* lens, int64_t n_windows,
                                    int64_t L, int C, int pool, int dtype, float* gmax, int32_t* gidx, void* ws, void* stream);
/* The first launch of vm_bn_drop_pool_gmax_fwd alone: part_v / part_i receive the vm_bn_part_rows() partial (value, position) rows
 * of every window ((n_windows * rows, C) each; two arrays so that the two towers' launches can fill the halves of one pair of
 * arrays); vm_tail_fwd_bwd (below) finishes them inside its own launch. */
int vm_bn_drop_pool_gmax_partials(const void* z, const float* scale, const float* shift, const float* drop, int64_t n_windows,
                                  int64_t windows_per_tower, int64_t L, int C, int pool, int dtype, float* part_v, int32_t* part_i,
                                  void* stream);
/* The LAST block in pair form (round 6; 16-bit storage): vm_conv_fwd_fold leaves (e, o) for it like for the blocks below -- e PADDED
 * (n_windows, Lq + 2, C), Lq = L / 2 -- and the GlobalMaxPool1D pass reads e alone: BatchNorm is monotone per channel, so
 * max_j fma(z_j, s, h) == fma(ext_j z, s, h), the values and first-maximum positions are those of vm_bn_drop_pool_gmax_partials on z,
 * from half the bytes.  voicemap/models.py:31-37.  The backward's sparse sums (vm_bn_bwd_gmax_finalize_e: vm_bn_bwd_gmax_finalize with
 * e in z's place) and apply pass (vm_bn_pool_bwd_apply_pairs_gmax: vm_bn_pool_bwd_apply_gmax on the (e, o) pair form; du padded
 * (n_windows, L + 2, C) as there) take the same tensors. */
int vm_bn_drop_pool_gmax_partials_e(const void* e, const float* scale, const float* shift, const float* drop, int64_t n_windows,
                                    int64_t windows_per_tower, int64_t Lq, int C, int dtype, float* part_v, int32_t* part_i,
                                    void* stream);
int vm_bn_bwd_gmax_finalize_e(const void* e, const float* dg, const int32_t* gidx, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const float* drop, int64_t n_windows, int64_t windows_per_tower,
                              int64_t Lq, int C, int dtype, double count_per_tower, float* c1, float* c2, float* grad_gamma,
                              float* grad_beta, void* stream);
int vm_bn_pool_bwd_apply_pairs_gmax(const void* e, const void* o, const float* dg, const int32_t* gidx, const float* scale,
                                    const float* shift, const float* mean, const float* invstd, const float* drop, const float* c1,
                                    const float* c2, int64_t n_windows, int64_t windows_per_tower, int64_t L, int C, int dtype, void* du,
                                    float* part_du, void* stream);

/* ---- a1 tail: GlobalMaxPool1D + Dense(E)  (voicemap/models.py:37-39) ------------------------------------
 * act: padded (n_windows, L+2, C) `dtype`; gmax (n_windows, C) fp32; gidx (n_windows, C) int32 = first argmax. */
int vm_global_maxpool_fwd(const void* act, int64_t n_windows, int64_t L, int C, int dtype, float* gmax,
                          int32_t* gidx, void* stream);
/* GlobalMaxPool1D over the valid rows of a length-masked bucket: rows t < lens[n] (>= 1) of window n's padded act only; same values
 * and first-maximum rows as vm_global_maxpool_fwd on them.  Segment-parallel (a bucket may hold a few very long windows):
 * ws >= vm_bn_drop_pool_gmax_workspace_bytes(n_windows, C). */
int vm_global_maxpool_fwd_varlen(const void* act, const int32_t* lens, int64_t n_windows, int64_t L, int C, int dtype, float* gmax,
                                 int32_t* gidx, void* ws, void* stream);
/* dp: (n_windows, L, C) `dtype`, zero except dp[n][gidx[n][c]][c] = dg[n][c]. */
int vm_global_maxpool_bwd(const float* dg, const int32_t* gidx, int64_t n_windows, int64_t L, int C, int dtype,
                          void* dp, void* stream);
/* out[r][o] = sum_i in[r][i]*w[i][o] + b[o]   (w: (n_in, n_out) Keras Dense kernel; all fp32). */
int vm_dense_fwd(const float* in, const float* w, const float* b, int64_t rows, int n_in, int n_out, float* out,
                 void* stream);
/* grad_w[i][o] = sum_r in[r][i]*dout[r][o]; grad_b[o] = sum_r dout[r][o]; din[r][i] = sum_o dout[r][o]*w[i][o]
 * (din may be NULL; grad_w and grad_b may both be NULL: then only din -- the two halves are independent launches and a caller may
 * put the parameter half on another stream).  Fixed summation order. */
int vm_dense_bwd(const float* in, const float* w, const float* dout, int64_t rows, int n_in, int n_out,
                 float* grad_w, float* grad_b, float* din, void* stream);

/* ---- a2 + a3/a4: siamese head + loss, forward and backward in one launch ----------------------------------
 * (voicemap/models.py:55-69; voicemap/utils.py:77-85; 'binary_crossentropy' experiments/train_siamese.py:57)
 * emb: (2*pairs, E) fp32, rows [0,pairs) = tower 0, [pairs, 2*pairs) = tower 1.
 * head_kind UNIFORM_EUCLIDEAN: d = sqrt(sum (e1-e2)^2), p = sigmoid(w[0]*d + b);  WEIGHTED_L1: p = sigmoid(sum w[j]|e1-e2|_j + b).
 * y: (pairs) fp32 labels, 0 = same speaker (voicemap/librispeech.py:194).  y may be NULL for predict-only
 * (then loss/backward outputs are not touched).
 * pred (pairs); loss_acc[0] = loss, [1] = binary accuracy; demb (2*pairs, E); grad_hw (1 or E); grad_hb (1).
 * ws: 4*pairs floats of scratch (per-pair terms, summed in fixed order by a second small launch); unused when y is NULL.
 * grad_scale: every gradient output (demb, grad_hw, grad_hb) is multiplied by it -- 1 for fp32 / bf16 storage; the loss scale of
 * VM_F16 storage, whose activation gradients would otherwise fall under half's 6e-8; loss_acc and pred are not scaled.
 * loss_acc may be NULL with y given: then only the per-pair pass runs (pred, demb, ws) and the caller enqueues vm_siamese_head_reduce
 * (the fixed-order sums: loss_acc, grad_hw, grad_hb -- nobody's input before the optimizer) where it likes, e.g. on another stream. */
int vm_siamese_head_loss(const float* emb, const float* head_w, const float* head_b, const float* y, int64_t pairs,
                         int E, int head_kind, int loss_kind, float grad_scale, float* pred, float* loss_acc, float* demb,
                         float* grad_hw, float* grad_hb, float* ws, void* stream);
int vm_siamese_head_reduce(const float* emb, const float* ws, int64_t pairs, int E, int head_kind, float* loss_acc, float* grad_hw,
                           float* grad_hb, void* stream);

/* ---- the whole tail of a siamese training step, forward and backward (SURVEY 8(b) `vm_tail_fwd_bwd`) -------------------------
 * GlobalMaxPool1D -> Dense(E) (voicemap/models.py:37-39) -> twin distance -> Dense(1, sigmoid) (models.py:55-69) -> loss
 * (voicemap/utils.py:77-85 / 'binary_crossentropy' experiments/train_siamese.py:57) -> d loss / d emb -> d loss / d gmax.
 * All of it is local to a pair: ONE launch, one workgroup per pair (windows b and pairs + b), replaces gmax_segments + vm_dense_fwd +
 * the per-pair pass of vm_siamese_head_loss + the input half of vm_dense_bwd.  What crosses pairs and is nobody's input before the
 * optimizer -- loss_acc, the head's and the dense layer's parameter gradients -- is vm_tail_param_grads, a second launch the
 * caller may put on another stream (it replaces vm_siamese_head_reduce + the parameter half of vm_dense_bwd).  Bit-identical to the
 * six launches they replace (same summation orders).
 *   gmax_part_v / gmax_part_i: the partial rows of vm_bn_drop_pool_gmax_partials ((2*pairs * seg_rows, C), seg_rows =
 *               vm_bn_part_rows()), or both NULL when gmax / gidx (2*pairs, C) are already final (vm_global_maxpool_fwd); with
 *               parts, gmax and gidx are WRITTEN here.
 *   dense_w (C, E), dense_b (E) or NULL; head_w / head_b / y / head_kind / loss_kind / grad_scale as in vm_siamese_head_loss.
 *   outputs: emb (2*pairs, E), pred (pairs), demb (2*pairs, E), dgmax (2*pairs, C), ws (4*pairs: the per-pair terms).
 * vm_tail_fwd_bwd_supported: C <= 1024 and E <= 256 (the pair's rows live in LDS). */
int vm_tail_fwd_bwd_supported(int C, int E);
int vm_tail_fwd_bwd(const float* gmax_part_v, const int32_t* gmax_part_i, int seg_rows, float* gmax, int32_t* gidx, const float* dense_w, const float* dense_b,
                    const float* head_w, const float* head_b, const float* y, int64_t pairs, int C, int E, int head_kind,
                    int loss_kind, float grad_scale, float* emb, float* pred, float* demb, float* dgmax, float* ws, void* stream);
int vm_tail_param_grads(const float* gmax, const float* demb, const float* emb, const float* ws, int64_t pairs, int C, int E,
                        int head_kind, float* loss_acc, float* grad_dense_w, float* grad_dense_b, float* grad_hw, float* grad_hb,
                        void* stream);

/* ---- a9: classifier head Dense(num_classes, softmax) + categorical CE  (experiments/train_classifier.py:112,115)
 * logits (rows, n_classes) fp32 -> prob; labels int32 (rows); loss_acc[0] = mean CE (Keras clip 1e-7), [1] = accuracy;
 * dlogits = grad_scale * d loss / d logits (may be NULL).  labels may be NULL for predict-only.  ws: 2*rows floats. */
int vm_softmax_cce(const float* logits, const int32_t* labels, int64_t rows, int n_classes, float grad_scale, float* prob,
                   float* loss_acc, float* dlogits, float* ws, void* stream);

/* ---- a9b: prototypical loss on a k-way n-shot episode (Snell et al. 2017; this project's own objective, the reference has none)
 * emb (k*n + m, E) fp32: rows [0, k*n) the support set, class-major (class c owns rows c*n .. c*n + n - 1: the layout of
 * vm_nshot_distances' support), rows [k*n, k*n + m) the queries; labels int32 (m) in [0, k).
 *   p_c = mean of class c's n support rows;  logits[j][c] = -alpha * sum_t (q_j[t] - p_c[t])^2  (written, (m, k), never scaled);
 *   loss_acc[0] = mean_j (logsumexp_c logits[j] - logits[j][y_j]) (row maximum subtracted, no clip), [1] = the share of queries whose
 *   first maximum is y_j (alpha = 1: the argmin of vm_nshot_distances(VM_DIST_EUCLIDEAN));
 *   demb (k*n + m, E) = grad_scale * d loss / d emb, every row written: with r = softmax - onehot a query row gets
 *   (2 alpha / m) sum_c r[j][c] p_c, every support row of class c (2 alpha / (m n)) sum_j r[j][c] (q_j - p_c).
 * labels NULL: predict-only (logits alone; loss_acc, demb, ws untouched).  demb NULL with labels: evaluation (loss_acc alone).
 * A label outside [0, k) takes its query out of every sum (no loss term, no hit, no gradient; its logits are still written) while the
 * means still divide by m.  Two launches: per query, then per class (+ the means); every sum in a fixed order (support rows in row
 * order, the E components per lane ascending then an xor butterfly, classes ascending, queries in row order), no atomics: results
 * are bit-identical run to run.  vm_proto_loss_supported: 2 <= k <= 128, 1 <= n <= 16, 1 <= E <= 256, k * E <= 16384 (the prototypes
 * live in LDS), 1 <= m < 2^31; VM_ERR_UNSUPPORTED outside.  ws: vm_proto_loss_workspace_bytes (r (m, k), loss terms, hits). */
int vm_proto_loss_supported(int k, int n, int64_t m, int E);
int vm_proto_loss(const float* emb, const int32_t* labels, int k, int n, int64_t m, int E, float alpha, float grad_scale,
                  float* logits, float* loss_acc, float* demb, float* ws, void* stream);
int64_t vm_proto_loss_workspace_bytes(int k, int n, int64_t m, int E);

/* ---- a9c: triplet loss with mining inside the batch (Hermans et al. 2017 "batch hard" / "batch all", FaceNet's margin; this
 * project's own objective, the reference has none; csrc/triplet.hip)
 * Inputs.  emb (N, E) fp32; label (N) int32, the speaker of every row: any values, rows in any order.  A row with label < 0 takes
 * no part: it is no anchor and no candidate, its demb row is written as zeros, and its contents are never used.
 * Distances.  s_ij = sum_t (e_i[t] - e_j[t])^2 in fp32, the direct form (no norm expansion: all terms are non-negative), a lane's
 * components t = lane, lane + 64, ... ascending with fmaf, then the xor butterfly;  d_ij = sqrtf(s_ij).
 * Candidate sets.  For a participating anchor a: P_a = {j != a : label[j] == label[a]}, N_a = {j : label[j] >= 0, label[j] != label[a]}.
 * The anchor is VALID iff both are non-empty.
 * VM_TRIPLET_HARD.  hp(a) = the element of P_a first by (s descending, j ascending), hn(a) = the element of N_a first by (s ascending,
 * j ascending): s is compared, never d, and the order is total, so the choice is a function of the inputs alone.
 *   x_a = margin + d_a,hp - d_a,hn (soft == 1: the margin is ignored, x_a = d_a,hp - d_a,hn).
 *   hinge (soft == 0): l_a = max(0, x_a), weight g_a = 1 iff x_a > 0, else 0;
 *   soft:              l_a = max(x_a, 0) + log1p(exp(-|x_a|)), weight g_a = sigmoid(x_a).
 *   loss_acc[0] = (1 / V) sum over valid anchors l_a, V = the number of valid anchors;  loss_acc[1] = the share of valid anchors with
 *   x_a > 0;  V = 0: loss 0, share 0, demb all zeros.
 * VM_TRIPLET_ALL.  Every triplet (a, p in P_a, n in N_a) counts, x = margin + d_ap - d_an (soft: d_ap - d_an); T = their number.
 *   hinge: loss_acc[0] = sum over the triplets with x > 0 of x / max(1, A), A = their number (the "non-zero" mean); a triplet's
 *          weight is 1 / A iff x > 0;  loss_acc[1] = A / T.
 *   soft:  loss_acc[0] = mean over the T triplets of softplus(x); weight sigmoid(x) / T;  loss_acc[1] = the share with x > 0.
 * hard_pos, hard_neg (N) int32 receive hp(a), hn(a) in both modes, -1 where the anchor is not valid; either may be NULL.
 * Gradient.  demb (N, E) = grad_scale * d loss / d emb, every row written; the selections and A are constants.  A pair (a, j) whose
 * triplets' weights sum to c (positive as a positive, negative as a negative) adds c (e_a - e_j) / d_aj to row a and its negative to
 * row j; a pair with s_aj == 0 adds nothing: no epsilon, no division by zero, the result stays finite.
 * demb NULL: evaluation -- loss_acc and the indices are written, demb is not touched.
 * Non-finite input.  If a participating row holds a non-finite value, loss_acc[0] is NaN and every element of demb is NaN (an anchor
 * that meets a non-finite s flags the call): the f16 loss-scale skip relies on it.
 * Limits.  2 <= N <= 1024, 1 <= E <= 256 (vm_triplet_loss_supported; VM_ERR_UNSUPPORTED above, VM_ERR_ARG below); the hinge needs a
 * finite margin >= 0; mining and soft in range; refused before any launch.
 * Order of the sums (no float atomics; two calls are bit-identical; grad_scale times a power of two scales demb exactly).  Launch 1,
 * one workgroup of 256 threads per anchor: candidate j belongs to thread j % 256; a selection is a thread's candidates ascending,
 * the butterfly on (s, j), the four waves in order.  ALL: the positives ascending (the whole workgroup together), a thread's negatives
 * ascending -- a negative's weight and the thread's loss accumulate in that order, a positive's weight is the butterfly over the lanes
 * then the four waves in order, the anchor's loss likewise.  Launch 2: row i, component t:
 * grad_scale * ((sum_j (W[i][j] + W[j][i]) (e_i[t] - e_j[t]), j ascending, fmaf) / norm), W[a][j] = +-c_aj / d_aj, norm = V, A or T
 * (an integer sum); the loss: a thread's rows ascending, the butterfly, the four waves in order, one division.
 * ws >= vm_triplet_loss_workspace_bytes(N, E, mining) = (N N + 4 N) * 4: W (N, N), the anchors' loss terms, counts and flags. */
int vm_triplet_loss_supported(int64_t N, int E);
int64_t vm_triplet_loss_workspace_bytes(int64_t N, int E, int mining);
int vm_triplet_loss(const float* emb, const int32_t* label, int64_t N, int E, int mining, int soft, float margin, float grad_scale,
                    int32_t* hard_pos, int32_t* hard_neg, float* loss_acc, float* demb, void* ws, void* stream);
enum { VM_TRIPLET_HARD = 0, VM_TRIPLET_ALL = 1 };

/* ---- a9d: softmax over scaled cosines with a margin at the label (NormFace; CosFace / AM-softmax; ArcFace / AAM-softmax; this
 * project's own objective, the reference has none; csrc/margin.hip).  The head of the classifier trained for cosine scoring.
 * Inputs.  emb (N, E) fp32; w (E, S) fp32, the Dense kernel of the classifier head: column c is class c; labels (N) int32.  The
 * head's bias takes no part.
 * Cosines.  ss_i = sum_t e_i[t]^2, n_i = sqrtf(ss_i); ssw_c = sum_t w[t][c]^2, m_c = sqrtf(ssw_c); d_ic = sum_t e_i[t] w[t][c];
 *   c_ic = d_ic / (n_i * m_c) (one product, one division), then clamped to [-1, 1] by comparisons (a NaN stays a NaN); the clamp
 *   passes the gradient through.  ss_i == 0 or ssw_c == 0 exactly: c_ic = 0, and the zero row / zero column receives a zero
 *   gradient (no epsilon).  e_hat_i[t] = e_i[t] / n_i, w_hat_c[t] = w[t][c] / m_c (zeros for a zero row / column).
 *   cosine (N, S) <- c_ic, prob (N, S) <- softmax_c(scale * c_ic) = expf(scale c_ic - scale cmax_i) / sum_c of the same, pred (N)
 *   int32 <- the first maximum of row i of c (a NaN is never a maximum; a row without one: 0); never margined; each may be NULL.
 * Target logit.  y = labels[i], c = c_iy.  VM_MARGIN_NONE: c' = c, f = 1.  VM_MARGIN_COSINE: c' = c - margin, f = 1.
 *   VM_MARGIN_ANGULAR: cos_m, sin_m, th = -cos_m, mm = margin sin_m are computed in double from the float margin on the host and
 *   rounded once to float; sin_t = sqrtf(max(0, fmaf(-c, c, 1))).  c > th: c' = fmaf(c, cos_m, -(sin_t sin_m)),
 *   f = dc'/dc = fmaf(sin_m, c / max(sin_t, VM_MARGIN_SIN_FLOOR), cos_m);  otherwise c' = c - mm, f = 1.
 *   z_ic = scale * c_ic for c != y, z_iy = scale * c'.
 * Loss.  l_i = logf(sum_c expf(z_ic - zmax_i)) - (z_iy - zmax_i), zmax_i the row's maximum of z, no clip;
 *   loss_acc[0] = (1 / N) sum_i l_i;  loss_acc[1] = (1 / N) #{i : pred_i == y_i} (from the un-margined cosines: what the model
 *   predicts).  A row whose label is outside [0, S) is taken out of every sum: no loss term, no hit, a zero demb row, nothing in
 *   grad_w; its cosine, prob and pred are still written; the means still divide by N.
 * Gradients.  g_ic = (scale / N) * (expf(z_ic - zmax_i) / Z_i - [c == y]) (* f at c == y);  A_i = sum_c g_ic c_ic;  B_c = sum_i g_ic c_ic;
 *   demb[i][t]   = grad_scale * ((sum_c (g_ic / m_c) w[t][c] - A_i e_hat_i[t]) / n_i)          (g_ic / m_c := 0 where m_c == 0)
 *   grad_w[t][c] = grad_scale * ((sum_i g_ic e_hat_i[t] - B_c w_hat_c[t]) / m_c)               ((E, S), every element written)
 *   grad_b (S) is written as zeros when not NULL: the bias stays in the parameter layout and never moves.
 * Modes.  labels NULL: predict only -- cosine, prob, pred alone.  demb NULL with labels: evaluation -- loss_acc and those three
 *   alone (grad_w, grad_b untouched).  demb given: labels, loss_acc and grad_w are required.  ws is always required.
 * Non-finite input.  A non-finite component in a participating row or in any class column makes loss_acc[0] NaN and the demb of that
 *   row (of every participating non-zero row, for a column) NaN: no clamp, max or comparison swallows a NaN.  The f16 loss-scale skip
 *   relies on it.
 * Limits.  1 <= N <= 4096, 2 <= S <= 16384, 1 <= E <= 256 (vm_margin_softmax_supported; VM_ERR_UNSUPPORTED above, VM_ERR_ARG
 *   below); a finite margin with 0 <= margin < pi / 2 (every kind), a finite scale > 0, kind in range; refused before any launch.
 * Order of the sums (three launches, no float atomics; two calls are bit-identical; grad_scale times a power of two scales demb and
 *   grad_w exactly).  ss_i: a lane's components t = lane, lane + 64, ... ascending with fmaf, then the xor butterfly.  ssw_c and d_ic:
 *   t ascending with fmaf.  Row i is one workgroup of 256 threads, class c belongs to thread c % 256.  The first maximum, zmax_i: a
 *   thread's classes ascending, the butterfly on (value, c), the four waves in order.  Z_i, the prob denominator and A_i (fmaf): a
 *   thread's classes ascending, the butterfly, the four waves in order.  demb's sum over c: a lane's classes c = lane, lane + 64, ...
 *   ascending with fmaf, the butterfly; then fmaf(-A_i, e_hat_i[t], sum) / n_i.  grad_w's sum over i and B_c: rows ascending with
 *   fmaf, a row with g_ic == 0 skipped; then fmaf(-B_c, w_hat_c[t], sum) / m_c.  The means: a thread's rows i = tid, tid + 256, ...
 *   ascending, the butterfly, the four waves in order, one division by N.
 * ws >= vm_margin_softmax_workspace_bytes(N, S, E) = (S + N E + 2 N + 2 N S) * 4: m, e_hat, the rows' loss terms and hits, g, c. */
#define VM_MARGIN_SIN_FLOOR 0.015625f /* 2^-6: the floor of sin_t in dc'/dc; a definition, not a tolerance */
int vm_margin_softmax_supported(int64_t N, int S, int E);
int64_t vm_margin_softmax_workspace_bytes(int64_t N, int S, int E);
int vm_margin_softmax(const float* emb, const float* w, const int32_t* labels, int64_t N, int S, int E, int kind, float margin,
                      float scale, float grad_scale, float* cosine, float* prob, int32_t* pred, float* loss_acc, float* demb,
                      float* grad_w, float* grad_b, void* ws, void* stream);
enum { VM_MARGIN_NONE = 0, VM_MARGIN_COSINE = 1, VM_MARGIN_ANGULAR = 2 };

/* ---- a5: Adam(clipnorm=1.)  (experiments/train_siamese.py:56; Keras 2.2.2 optimizers.py) -------------------
 * sqnorm: 1 fp32 on device <- sum(g^2) over the flat gradient buffer (fixed order; ws >= vm_sqnorm_workspace_bytes).  sqnorm may be
 * NULL: then only the partial sums are left in ws, for vm_adam_clip_step's sqnorm_parts (one launch less). */
int64_t vm_sqnorm_workspace_bytes(int64_t n);
int vm_grad_sqnorm(const float* g, int64_t n, void* ws, float* sqnorm, void* stream);
/* g *= grad_prescale (e.g. 1/world after an all-reduce sum); norm = grad_prescale*sqrt(*sqnorm);
 * if clipnorm > 0 and norm >= clipnorm: g *= clipnorm/norm;  m,v,p updated with lr_t = lr*sqrt(1-b2^t)/(1-b1^t)
 * (computed on the host, passed in), p -= lr_t*m/(sqrt(v)+eps).
 * skip_nonfinite != 0 (needs sqnorm): a step whose gradient norm is inf / NaN leaves p, m, v untouched (loss-scaled VM_F16
 * training: an overflowed activation gradient costs one step instead of the model) and increments the caller's running count *skipped
 * (1 int32 on the device, zeroed by the caller, may be NULL); with 0 the update is Keras' own arithmetic, NaNs included.
 * sqnorm_parts (optional): the ws vm_grad_sqnorm(…, sqnorm = NULL) filled -- every workgroup then adds the partials itself (same
 * order, same value) and *sqnorm (if not NULL) receives the sum; without it *sqnorm is read. */
int vm_adam_clip_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                      float eps, float clipnorm, float grad_prescale, float* sqnorm, const void* sqnorm_parts, int skip_nonfinite,
                      int32_t* skipped, void* stream);

/* ---- a8: n-shot evaluation distances  (voicemap/utils.py:159-206) ------------------------------------------
 * For each task: query embedding (E) vs k class prototypes built from n support embeddings each
 * (support: (tasks, k*n, E), query: (tasks, E), fp32); writes pred (tasks, k) as float64-accumulated distances
 * and argmin (tasks) int32.  dist_kind per VM_DIST_*. */
int vm_nshot_distances(const float* query, const float* support, int64_t tasks, int k, int n, int E, int dist_kind,
                       float* pred, int32_t* argmin, void* stream);

/* ---- f2 / BASELINE.json config 5: evaluation over a CACHED embedding matrix -----------------------------------------
 * The reference embeds the k*n + 1 windows of every task anew (voicemap/utils.py:121-212; the sweep of
 * experiments/k_way_accuracy.py:52-69 does so 38 000 times).  Its evaluation datasets are built with stochastic=False
 * (experiments/train_siamese.py:44), i.e. every file has ONE window; embed the corpus once into emb (n_rows, E) fp32 and a task
 * is k*n + 1 row indices.
 * vm_nshot_indexed: vm_nshot_distances with the rows gathered by index: query_idx (tasks), support_idx (tasks, k*n) laid out
 * [class_1]*n + ... + [class_k]*n like voicemap/librispeech.py:224-237; float64 arithmetic of voicemap/utils.py:159-206;
 * pred (tasks, k) may be NULL; argmin (tasks) int32, first minimum, a NaN distance first like numpy.argmin.  E <= 256. */
int vm_nshot_indexed(const float* emb, int64_t n_rows, const int32_t* query_idx, const int32_t* support_idx, int64_t tasks, int k,
                     int n, int E, int dist_kind, float* pred, int32_t* argmin, void* stream);
/* vm_pairdist_argmin: the pairwise-distance matrix between q (M, E) and ref (N, E), fp32, and per query row the nearest reference
 * row (first minimum).  dist_kind: EUCLIDEAN sqrt(sum (a-b)^2) (direct form, no norm-expansion cancellation), COSINE
 * 1 - a.b / (|a| |b|), DOT -a.b.  q_row0 >= 0: query row m IS reference row q_row0 + m (q is a row shard of ref -- the
 * data-parallel form: all-gather the embeddings, every rank takes its rows) and is excluded from its own argmin; -1: no exclusion.
 * dist (M, N) may be NULL (argmin only: nothing but best_val / best_idx (M) leaves the chip; best_idx = -1 if every distance of the
 * row is NaN).  ws >= vm_pairdist_workspace_bytes(M, N).  E <= 256, N < 2^31.  dist_kind may also be VM_SCORE_PLDA (q and ref are
 * PLDA-space rows; see the enum). */
int64_t vm_pairdist_workspace_bytes(int64_t M, int64_t N);
int vm_pairdist_argmin(const float* q, const float* ref, int64_t M, int64_t N, int E, int dist_kind, int64_t q_row0, float* dist,
                       float* best_val, int32_t* best_idx, void* ws, void* stream);
/* vm_pair_score_hist: all-pairs speaker verification -- what the reference's experiments/verification_accuracy.py (a stub: "determines the
 * best verification distance threshold on the validation set and then ... estimate the true verification accuracy on the test set")
 * needs, without the N x N matrix.  Every pair {i, j}, row_lo <= i < row_hi, i < j < N, of emb (N, E) is scored -- score_kind
 * VM_DIST_* bit-identical to dist[i][j] of vm_pairdist_argmin, VM_SCORE_WEIGHTED_L1 = sum_e weights[e] |a_e - b_e| (ascending e, fmaf),
 * VM_SCORE_NEG_EUCLIDEAN = -euclidean, VM_SCORE_PLDA as stated at the enum -- and counted by class (0: label[i] == label[j], 1: otherwise) into the bins of each of
 * n_windows (<= 4) windows on the order-preserving uint32 key of the score (-0.0 taken as +0.0; bits | 2^31 if non-negative, ~bits if
 * negative).  host_windows (n_windows, 2) int64 on the HOST: key_lo, shift (<= 31): key k goes to bin (k - key_lo) >> shift if k >= key_lo
 * and that is < bins, else to slot bins (k < key_lo) or bins + 1; a NaN score to slot bins + 2.  hist (n_windows, 2, bins + 3) uint64 is
 * ACCUMULATED (row ranges / ranks sum).  n_windows * 2 * (bins + 3) <= 8216 (4 windows x 1024 bins, 1 x 4096).  weights (E) only for
 * VM_SCORE_WEIGHTED_L1.  ws >= vm_pair_score_hist_workspace_bytes(N, E).  E <= 256, N < 2^31. */
int64_t vm_pair_score_hist_workspace_bytes(int64_t N, int E);
int vm_pair_score_hist(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights, int64_t row_lo,
                       int64_t row_hi, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist, void* ws, void* stream);
/* vm_cohort_topk_stats: per-row cohort statistics for score normalisation (S-norm: K = C; AS-norm: the top K).  Query rows q (M, E),
 * cohort rows cohort (C, E).
 * Scores.  For query row m and cohort row c, s_mc is the same score vm_pair_score_hist would give the pair, bit for bit: for VM_DIST_*
 * bit-identical to dist[m][c] of vm_pairdist_argmin(q, cohort, ...); VM_SCORE_NEG_EUCLIDEAN the negated euclidean; VM_SCORE_WEIGHTED_L1
 * the ascending-e fmaf sum with `weights`.  E <= 256.
 * Exclusion.  If self_row0 >= 0, query row m is cohort row self_row0 + m and that pair is skipped (the convention of q_row0 of
 * vm_pairdist_argmin).  NaN scores are skipped.
 * Selection.  Let V be the remaining scores and K' = min(K, |V|).  The selection is the K' smallest of V by (uint32 key of the score,
 * cohort index) ascending; the key is vm_pair_score_hist's, with -0.0 taken as +0.0.  "Smallest" means most alike.  Ties at the K-th key
 * are broken by the lower cohort index, so exactly K' are chosen.  K = C means S-norm over the whole cohort.  K >= 1.
 * Outputs.  count[m] = K'.  mu[m] and sigma[m] are the mean and the population standard deviation of the selected scores, accumulated in
 * float64 and rounded to fp32 once.  rsig[m] = (float)(1.0 / (double)sigma[m]).  If K' = 0, mu, sigma and rsig are NaN; if sigma = 0,
 * rsig = +inf.  topk_idx (M, K) int32 is optional (NULL: not written): the selected cohort indices in (key, index) order, padded with -1.
 * Determinism.  Bit-identical from run to run: a fixed summation order, no float atomics.
 * ws >= vm_cohort_stats_workspace_bytes(M, C, E) (a score tile of at most ~192 MB).  M, C < 2^31. */
int64_t vm_cohort_stats_workspace_bytes(int64_t M, int64_t C, int E);
int vm_cohort_topk_stats(const float* q, int64_t M, const float* cohort, int64_t C, int E, int score_kind, const float* weights,
                         int64_t self_row0, int64_t K, float* mu, float* sigma, float* rsig, int32_t* count, int32_t* topk_idx, void* ws,
                         void* stream);
/* vm_pair_score_hist_norm: vm_pair_score_hist on normalised scores.  mu, rsig (N) fp32 on the device, indexed by row (vm_cohort_topk_stats
 * of the rows of emb).  The pair {i, j} is binned on  a = s - mu[i];  b = s - mu[j];  s' = 0.5f * (a * rsig[i] + b * rsig[j])  in fp32,
 * in exactly that order, every operation rounded on its own (no contraction into fma).  Everything else as vm_pair_score_hist; ws >=
 * vm_pair_score_hist_workspace_bytes(N, E). */
int vm_pair_score_hist_norm(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights, int64_t row_lo,
                            int64_t row_hi, const int64_t* host_windows, int n_windows, int bins, const float* mu, const float* rsig,
                            uint64_t* hist, void* ws, void* stream);
/* vm_pair_calib_sums: the sums of score calibration (csrc/calib.hip, voicemap_amd/calibration.py) -- prior-weighted logistic regression
 * llr = a s + b over the trials of vm_pair_score_hist, Cllr, and the Bayes-threshold detection costs -- reduced on the chip.
 * Trials.  Exactly vm_pair_score_hist's: unordered pairs {i, j}, row_lo <= i < row_hi, i < j < N; class 0 (target) iff label[i] ==
 * label[j], class 1 otherwise.  s is the fp32 score of score_kind (same bits as vm_pair_score_hist's); with mu / rsig (both or neither)
 * it is replaced by vm_pair_score_hist_norm's normalised score, in exactly that fp32 order.  A trial whose s is NaN or infinite is
 * skipped and counted in n_skipped.
 * Per-trial terms, in float64, every operation rounded on its own (no contraction into fma):
 *   z = a * s + b + tau;  t = -z for a target, +z for a non-target;  e = exp(-|t|);  loss = max(t, 0) + log1p(e);
 *   p = 1 / (1 + e) if t >= 0, else e / (1 + e);  w = e / ((1 + e) * (1 + e)).
 * sums (2, 8) float64 on the device, OVERWRITTEN: per class  n, n_skipped, L = sum loss, P0 = sum p, P1 = sum p * s, W0 = sum w,
 * W1 = sum w * s, W2 = sum (w * s) * s.  The counts are exact.
 * Determinism.  Per-lane accumulators, a fixed-order wave / workgroup reduction, per-workgroup partials in ws and a fixed-order final
 * sum in a second launch; no floating-point atomics.  Bit-identical from run to run for the same arguments; a row range cut into
 * several calls sums in another order (within rounding).
 * vm_pair_calib_sums_splits(M, N): the splits of the reference tiles of a call with M = row_hi - row_lo rows (the grid is
 * ceil(M / 64) x splits workgroups; query block k visits the 128-row tiles from that of row row_lo + 64 k + 1 on).
 * a, b, tau finite; sums 8-byte aligned; the other limits are vm_pair_score_hist's.  ws >= vm_pair_calib_sums_workspace_bytes(N, E). */
int64_t vm_pair_calib_sums_workspace_bytes(int64_t N, int E);
int64_t vm_pair_calib_sums_splits(int64_t M, int64_t N);
int vm_pair_calib_sums(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, const float* weights, int64_t row_lo,
                       int64_t row_hi, const float* mu, const float* rsig, double a, double b, double tau, double* sums, void* ws,
                       void* stream);
/* Speaker models: enrolment, S-way identification and model-trial verification (csrc/enrol.hip, voicemap_amd/enrolment.py) -- the
 * exhaustive limit of the reference's n-shot k-way metric (voicemap/utils.py:159-206 with k = every speaker, n = every (other) file).
 * Rows emb (N, E) fp32, label (N) int32: the dense speaker index in [0, S), anything else (-1) = the row is not enrolled.  kind is
 * VM_DIST_*.  Everything below is float64 until a score is rounded to fp32 ONCE.
 *   |e_u| = sqrt(sum_e e^2), ascending e, correctly rounded root.  Contribution c_u: euclidean e_u; cosine e_u / |e_u|; dot_product
 *   e_u / |e_u| and the magnitude |e_u|.
 *   sum_s = sum of c_u, msum_s = sum of |e_u| (written for every kind) over the enrolled rows of s IN ASCENDING ROW ORDER; count_s.  The
 *   order is part of the contract: bit-identical from run to run and from rank to rank (no float atomics).
 *   Model of speaker s as seen by query row m: n = count_s, Sigma = sum_s; with leave_one_out != 0 and q_label[m] == s (query row m is
 *   then one of the enrolled rows of s): n = count_s - 1, Sigma = sum_s - c_m, msum likewise.  n == 0: no model -- (m, s) is NOT A TRIAL
 *   and is counted nowhere.  p = Sigma / n (euclidean, cosine); p = (msum / n) (Sigma / n) (dot_product).
 *   Score of the trial (m, s): euclidean sqrt(sum_e (q_e - p_e)^2) in the direct form; cosine 1 - q.p / (|q| |p|); dot_product -q.p; sums
 *   over ascending e.  Lower = more alike.  These are oracle.n_shot_prediction's numbers for a task whose support rows are the enrolled rows.
 *   Order of the trials of one query: (uint32 key of the fp32 score, speaker index) ascending; the key is vm_pair_score_hist's (-0.0 as
 *   +0.0); NaN scores come after every number, among themselves by speaker index.
 * vm_speaker_sums: sums (S, E) f64, msum (S) f64, count (S) int32 on the device.  ws >= vm_speaker_sums_workspace_bytes(N, E, S).
 * vm_speaker_identify: query rows q (M, E), q_label (M) (the own speaker, -1 / out of range: none).  scores (M, S) fp32 may be NULL;
 *   where (m, s) is not a trial it holds NaN.  best_idx[m] = the first speaker in the order (-1: the row has no trial), best_val[m] its
 *   score.  rank[m] = the number of speakers before the own speaker in the order (0 = identified); -1 if the row has no own speaker or
 *   that speaker has no model for the row.  true_score[m] = the score against the own speaker (NaN where rank is -1).
 * vm_speaker_trial_hist: every trial binned by class (0: s == q_label[m], 1: otherwise) with exactly the window / slot / NaN-slot
 *   conventions and limits of vm_pair_score_hist; hist (n_windows, 2, bins + 3) uint64 is ACCUMULATED (row ranges / ranks sum).  Its
 *   scores are bit-identical to vm_speaker_identify's matrix.
 * E <= 256; M, N, S < 2^31; q 16-byte aligned when E % 4 == 0.  ws >= the matching *_workspace_bytes(M, E, S). */
int64_t vm_speaker_sums_workspace_bytes(int64_t N, int E, int64_t S);
int vm_speaker_sums(const float* emb, const int32_t* label, int64_t N, int E, int64_t S, int kind, double* sums, double* msum, int32_t* count,
                    void* ws, void* stream);
int64_t vm_speaker_identify_workspace_bytes(int64_t M, int E, int64_t S);
int vm_speaker_identify(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                        const int32_t* count, int64_t S, int kind, int leave_one_out, float* scores, float* true_score, int32_t* rank,
                        float* best_val, int32_t* best_idx, void* ws, void* stream);
int64_t vm_speaker_trial_hist_workspace_bytes(int64_t M, int E, int64_t S);
int vm_speaker_trial_hist(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                          const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows, int n_windows, int bins,
                          uint64_t* hist, void* ws, void* stream);
/* vm_mine_pairs: hard-pair mining for siamese training (csrc/mine.hip, voicemap_amd/mining.py): per anchor row its k_neg nearest rows of
 * another speaker and its k_pos farthest rows of its own speaker, selected on the chip -- no M x N score tile is written anywhere.
 * Anchors and candidates.  Anchors are the rows row_lo <= i < row_hi of emb (N, E) fp32 (M = row_hi - row_lo; the row-shard form of
 * vm_pair_score_hist); the candidates of anchor i are all rows j != i of emb.  label (N) int32: the speaker of every row.
 * Scores.  score_kind is VM_DIST_EUCLIDEAN, VM_DIST_COSINE or VM_DIST_DOT, lower = more alike; s_ij is bit-identical to dist[i][j] of
 * vm_pairdist_argmin(emb + row_lo * E, emb, ...).  Order key: vm_pair_score_hist's uint32 key, -0.0 taken as +0.0.
 * Who takes part.  A candidate with label[j] < 0 or with a NaN score is never selected; an anchor with label[i] < 0 gets empty lists.
 * Negatives.  Eligible: label[j] != label[i] and, if neg_floor is not NULL (device, M fp32, indexed by i - row_lo),
 * key(s_ij) > key(neg_floor[i - row_lo]) -- strictly; a NaN floor means no floor for that anchor.  The list holds the k_neg eligible
 * candidates that are smallest by (key, j) ascending, in that order.
 * Positives.  Eligible: label[j] == label[i].  The list holds the k_pos largest by key, ties to the lower j: (key descending, j
 * ascending), in that order.
 * Outputs.  neg_idx (M, k_neg) int32 = j and neg_val (M, k_neg) fp32 = s_ij (its own bits: a -0.0 stays -0.0); pos_idx / pos_val
 * (M, k_pos) likewise; unused slots hold -1 and NaN.  Either pair is optional AS A PAIR: both NULL together with its k = 0.
 * Limits.  0 <= k_neg, k_pos <= 64, not both zero; E <= 256; N < 2^31; emb 16-byte aligned when E % 4 == 0.
 * Determinism.  (key, j) is a total order, so the lists are a function of the inputs alone: bit-identical from run to run and however
 * the row range is cut into calls; no float atomics, nothing depends on the order of arrival.
 * ws >= vm_mine_pairs_workspace_bytes(...): N squared norms, the anchors in scalar-path layout (O(M E)) and the partial lists of the
 * candidate splits, (splits, M, k_neg + k_pos) x 8 bytes. */
int64_t vm_mine_pairs_workspace_bytes(int64_t N, int E, int64_t row_lo, int64_t row_hi, int k_neg, int k_pos);
int vm_mine_pairs(const float* emb, const int32_t* label, int64_t N, int E, int score_kind, int64_t row_lo, int64_t row_hi, int k_neg,
                  int k_pos, const float* neg_floor, int32_t* neg_idx, float* neg_val, int32_t* pos_idx, float* pos_val, void* ws,
                  void* stream);
/* vm_ahc: batched agglomerative clustering for speaker diarization (csrc/cluster.hip, voicemap_amd/diarization.py; ahc_reference there is
 * the numpy statement, matched bit for bit).  emb (N, E) fp32 holds the windows of R recordings back to back.  row0 / mat0: R + 1 int64
 * each ON THE DEVICE, the exclusive cumulative sums of the recordings' window counts n_r and of n_r^2 (row0[R] == N, mat0[R] ==
 * sq_total; the host holds the lengths, as with vm_vad_frames' frame_base).  dist_kind is VM_DIST_EUCLIDEAN, VM_DIST_COSINE, VM_DIST_DOT or
 * VM_SCORE_PLDA (PLDA-space rows), lower = more alike; linkage is one of VM_LINK_*.
 * Per recording, its rows renumbered 0 .. n - 1 ("slots"):
 *   D[i][j] (i != j) is bit-identical to dist[i][j] of vm_pairdist_argmin on the same rows (symmetric bit for bit).  Every slot starts as
 *   an active cluster of size 1; c = the number of active clusters, T = max(1, target[r]) (target: R int32 on the device; NULL = 1).
 *   While c > T:  among the active pairs a < b take the smallest by (key(D[a][b]), a, b), key = vm_pair_score_hist's uint32 key with -0.0 as
 *   +0.0 and every NaN last;  h = D[a][b];  if threshold is not NaN and !(h <= threshold): stop (so a NaN h stops);  record merge t as
 *   (a, b, h, size_a + size_b);  for every other active k set D[k][a] = D[a][k] =
 *     single:   the one of D[k][a], D[k][b] with the smaller key (NaN loses; equal keys keep D[k][a]),
 *     complete: the one with the larger key (NaN wins; equal keys keep D[k][a]),
 *     average:  (size_a * D[k][a] + size_b * D[k][b]) / (size_a + size_b) in fp32, the sizes converted exactly, each product, the sum and
 *               the IEEE quotient rounded on its own (no FMA); a NaN result is stored as the quiet NaN 0x7fc00000;
 *   slot b is retired, size_a += size_b, c -= 1.
 * Outputs, on the device.  merge_a, merge_b, merge_size (N) int32 and merge_h (N) fp32: merge t of recording r at row0[r] + t; every index
 * of the recording that holds no merge (always row0[r] + n_r - 1) gets -1 / NaN.  labels (N) int32: the final clusters numbered 0 .. c - 1
 * in ascending order of their slot (= their lowest member row).  n_clusters (R) int32: the final c, 0 for an empty recording.
 * (key, a, b) is a total order: the outputs are a function of the inputs alone -- no atomics, bit-identical from run to run.
 * Limits.  0 <= n_r <= VM_AHC_MAX_N, E <= 256, N < 2^31; emb 16-byte aligned when E % 4 == 0; ws 16-byte aligned; a bad argument is an
 * error before any launch; R == 0 or N == 0 returns without a launch (nothing is written: the caller knows every recording is empty).
 * The launcher cannot see the device tables: n_r > VM_AHC_MAX_N, a negative n_r or a mat0 that does not go with row0 must be refused
 * by the caller (voicemap_amd/diarization.py cluster does).  The merge kernel leaves n_clusters[r] = -1 and nothing else for a recording
 * whose n_r is out of range.
 * Launches: the squared norms (cosine) and the scalar-path copy of all rows; the block-diagonal distances (one workgroup per 64 rows);
 * the merge loop, one workgroup per recording, O(n^2) typically and O(n^3) at worst.
 * ws >= vm_ahc_workspace_bytes(N, E, R, sq_total).  Its first sq_total floats are the matrices, D_r[i][j] at mat0[r] + i n_r + j, as the
 * merge loop left them (the diagonal is NaN); then N squared norms and the rows in scalar-path layout. */
enum { VM_LINK_SINGLE = 0, VM_LINK_COMPLETE = 1, VM_LINK_AVERAGE = 2 };
enum { VM_AHC_MAX_N = 2048 };
int64_t vm_ahc_workspace_bytes(int64_t N, int E, int64_t R, int64_t sq_total);
int vm_ahc(const float* emb, int64_t N, int E, const int64_t* row0, const int64_t* mat0, int64_t R, int64_t sq_total, int dist_kind,
           int linkage, float threshold, const int32_t* target, int32_t* merge_a, int32_t* merge_b, float* merge_h, int32_t* merge_size,
           int32_t* labels, int32_t* n_clusters, void* ws, void* stream);
/* vm_reseg: Viterbi resegmentation for speaker diarization (csrc/reseg.hip, voicemap_amd/diarization.py; reseg_reference there is the numpy
 * statement).  emb (N, E) fp32 holds the windows of R recordings back to back IN TIME ORDER; recording r owns rows row0[r] .. row0[r + 1]
 * (n_r of them) and K_r = n_models[r] models.  row0 / em0: R + 1 int64 each ON THE DEVICE, the exclusive cumulative sums of n_r and of
 * n_r K_r (row0[R] == N, em0[R] == em_total; the host holds the lengths, as with vm_ahc's mat0).  n_models (R), labels_in (N) and
 * chain_start (N, or NULL) int32 on the device.  labels_in[i] in [0, K_r) names the model row i belongs to; anything else (-1 by
 * convention): the row belongs to no model yet.  A non-zero chain_start[i] starts a new chain at row i; the first row of a recording
 * always starts one.  kind is VM_DIST_EUCLIDEAN, VM_DIST_COSINE or VM_DIST_DOT.  VM_SCORE_PLDA is refused: the mean of PLDA-space rows is
 * not a PLDA-space row, because their last column is quadratic in the row.
 * Per recording, its rows renumbered 0 .. n - 1, lab = labels_in; for it = 1 .. iters:
 *   Models.  For k < K: sum_k, msum_k, count_k are exactly vm_speaker_sums' for the rows of this recording with lab == k (float64
 *   contributions added in ascending row order); a row whose label is outside [0, K) enrols nowhere.
 *   Emissions.  e[t][k] = the fp32 score vm_speaker_identify states for the trial (row t, model k) with leave_one_out = 0 (float64 until
 *   the single rounding); count_k == 0 or a NaN score: e[t][k] = +inf.
 *   Decode, per chain t0 .. t1, in float64, every operation rounded on its own:  c[t0][k] = (double)e[t0][k];  for t > t0:  j* = the
 *   first minimum of c[t-1][.] (lowest index on ties),  sw = c[t-1][j*] + switch_cost,
 *   c[t][k] = (double)e[t][k] + (c[t-1][k] <= sw ? c[t-1][k] : sw)  (a tie stays),  the back pointer of (t, k) is k or j* accordingly.
 *   The chain ends in the first minimum of c[t1][.]; the labels are the back trace from there.
 *   Stop rule.  n_changed[r] = the number of rows whose new label differs from lab; if it is 0: stop; else lab = the new labels.
 * Outputs, on the device.  labels_out (N) int32: the last decode's labels -- model indices, never renumbered: a cluster that dies keeps
 * its number.  path_cost (R) float64: the sum of the chains' final minima of the last decode, added in chain order from 0.0.  iters_run
 * (R) int32: the number of decodes done.  n_changed (R) int32: the last decode's.  emis (em_total fp32, may be NULL): the emissions of
 * the last iteration run, e[t][k] at em0[r] + t K_r + k.
 *   No model with count > 0 (every label outside [0, K)):  labels_out = -1, path_cost = NaN, iters_run = 0, n_changed = 0, emis = +inf.
 *   Empty recording:  nothing is written but iters_run = 0.
 * The outputs are a function of the inputs alone -- no atomics, bit-identical from run to run.
 * Limits.  1 <= K_r <= VM_RESEG_MAX_K, E <= 256, N < 2^31, switch_cost finite and >= 0, 1 <= iters <= 16; no cap on n_r; labels_out
 * must not be labels_in; ws 16-byte aligned; a bad argument is an error before any launch; R == 0 returns without a launch.  The
 * launcher cannot see the device tables: a K_r out of range, or row0 / em0 that do not go together (em0[r + 1] - em0[r] != n_r K_r, a
 * range outside [0, N] / [0, em_total]), must be refused by the caller (voicemap_amd/diarization.py resegment does); the kernel leaves
 * iters_run[r] = -1 and nothing else for such a recording.
 * Launches: the row norms of all N rows; then one workgroup of 256 threads per recording for the whole loop.  The models live in LDS as
 * float64, VM_RESEG_MAX_K (E + 1) x 8 bytes (132 KB at E = 256: the entry point compares it with the device's per-block limit, as
 * vm_stft_logmel does); a decode step is one lane per model plus a wave-wide first minimum; the recording's chains are dealt to the
 * four waves in turn.  O(n K E) per iteration for the emissions, O(n) sequential steps for the models and per chain.
 * ws >= vm_reseg_workspace_bytes(N, E, R, em_total): N row norms, 9 bytes of back pointers and one float64 per row, em_total floats. */
enum { VM_RESEG_MAX_K = 64 };
int64_t vm_reseg_workspace_bytes(int64_t N, int E, int64_t R, int64_t em_total);
int vm_reseg(const float* emb, int64_t N, int E, const int64_t* row0, const int64_t* em0, int64_t R, int64_t em_total,
             const int32_t* n_models, const int32_t* labels_in, const int32_t* chain_start, int kind, double switch_cost, int iters,
             int32_t* labels_out, double* path_cost, int32_t* iters_run, int32_t* n_changed, float* emis, void* ws, void* stream);
/* vm_vbx: VBx, variational-Bayes HMM diarization over PLDA-space rows (csrc/vbx.hip, voicemap_amd/diarization.py vbx; vbx_reference there
 * is the numpy statement; Landini et al., "Bayesian HMM clustering of x-vector sequences", 2022).  The resegmentation that goes with a
 * PLDA back end: the states of the HMM are speakers, a speaker is a Gaussian posterior over its mean in the diagonalised space (within
 * covariance I, between covariance diag(psi)), the assignments are soft and the speaker priors may shrink to nothing.
 * Inputs.  rows (N, P) fp32: PLDA-space rows as vm_plda_project with `quad` writes them, IN TIME ORDER; only the columns w = 0 .. D - 1
 * are read.  row0, em0, n_models, labels_in, chain_start: vm_reseg's tables and conventions (K_r = n_models[r] speakers, a label
 * outside [0, K_r) = no cluster, em0 the cumulative sums of n_r K_r).  psi, r, ib (D) float64 on the device: r_d = sqrt(1 + 2 psi_d), so
 * that rho = r w = sqrt(psi) z; ib_d = 1 / b_d = (1 + 2 psi_d) / psi_d, so that |z|^2 = sum ib_d w_d^2.  The tables are taken as they
 * are: nothing here depends on their coming from a psi.  gamma_in (em_total float64) and pi_in (R x 64 float64), each may be NULL: a
 * warm start.
 * Per recording, its rows renumbered 0 .. n - 1, everything float64, every operation rounded on its own unless it is written as fma:
 *   Start.  gamma = gamma_in, or with q = exp(-init_smooth) (taken on the host) and den = 1 + (K - 1) q:  gamma[t][k] = 1 / den where
 *   labels_in[t] == k, q / den for the other k, 1 / K in a row of no cluster.  pi_k = pi_in, or 1 / K.  F = fa / fb.
 *   For it = 1 .. iters:
 *   Speaker posteriors.  N_k = sum_t gamma[t][k];  F_kd = fma(gamma[t][k], rho_td, .), rho_td = r_d * (double)w_td;  both over ascending
 *   t from 0.0.  invL_kd = 1 / (1 + (F * N_k) * psi_d);  alpha_kd = (F * invL_kd) * F_kd;  over ascending d from 0.0:
 *   q_k = fma(invL_kd + alpha_kd^2, psi_d, q_k),  ent_k = ent_k + (((log(invL_kd) - invL_kd) - alpha_kd^2) + 1).
 *   Emissions.  G_t = -0.5 * (fma(ib_d, w_td^2, .) over ascending d + (double)D * 1.8378770664093453);
 *   lp[t][k] = fa * ((fma(rho_td, alpha_kd, .) over ascending d - 0.5 * q_k) + G_t);  m_t = max_k lp[t][k];  p[t][k] = exp(lp[t][k] - m_t).
 *   Forward.  lambda_t = loop_prob, but 0 at t = 0 and at every chain start.  at[k] = p[t][k] * (lambda_t * a[t-1][k] + (1 - lambda_t) *
 *   pi_k);  c_t = SUM_k at[k];  a[t][k] = at[k] / c_t.  SUM_k: the terms padded with zeros to the next power of two K', then for
 *   o = 1, 2, 4, .., K'/2:  v[k] = v[k] + v[k ^ o] for all k at once;  the sum is v[0].
 *   Backward.  b[n-1][k] = 1;  pb[k] = p[t+1][k] * b[t+1][k];  s = SUM_k (pi_k * pb[k]);
 *   b[t][k] = (lambda_{t+1} * pb[k] + (1 - lambda_{t+1}) * s) / c_{t+1}.   gamma[t][k] = a[t][k] * b[t][k].
 *   Priors.  pi'_k = sum over ascending t of ((((1 - lambda_t) * pi_k) * p[t][k]) * b[t][k]) / c_t;  pi_k = pi'_k / (sum over ascending
 *   j of pi'_j).
 *   Bound.  log_pX = sum over ascending t of (log(c_t) + m_t);  ELBO_it = log_pX + (fb * 0.5) * (sum over ascending k of ent_k).  After
 *   the prior update: stop if it > 1 and ELBO_it - ELBO_{it-1} < epsilon; the iteration that stops is counted and its results are kept.
 *   Degenerate.  A c_t that is 0 or not finite (a prior has underflowed to exactly 0 under the best-emitting speaker) stops the
 *   recording: iters_run = -2, labels_out = labels_in, everything else as the last complete iteration (or the start) left it.
 * Outputs, on the device.  labels_out (N) int32: the first maximum of gamma[t][.], never renumbered.  gamma (em_total float64, also the
 * working copy: it must not be gamma_in).  pi (R x 64 float64; the entries past K_r are 0).  elbo (R x iters float64, NaN past
 * iters_run).  iters_run (R) int32: 0 for an empty recording (nothing else is written), -1 for tables the caller should have refused
 * (voicemap_amd/diarization.py vbx refuses them; nothing else is touched, as in vm_reseg), -2 as above.
 * The outputs are a function of the inputs alone -- no atomics, every sum in a fixed order, bit-identical from run to run.
 * Limits.  1 <= K_r <= VM_VBX_MAX_K, 1 <= D <= 255, D <= P, N < 2^31, 0 <= loop_prob < 1, fa, fb finite and > 0, init_smooth finite and
 * >= 0, epsilon not NaN (-inf: never stop), 1 <= iters <= 64; ws 16-byte aligned; a bad argument is an error before any launch; R == 0
 * returns without a launch.
 * Launches: G_t of all N rows, ceil(N / 256) workgroups of 256 threads; then R workgroups of 256 threads, one per recording, for the
 * whole loop.  alpha lives in LDS as float64, VM_VBX_MAX_K (D + 1) x 8 bytes (131 KB at D = 255: the entry point compares it with the
 * device's per-block limit, as vm_reseg does).  O(n K D) per iteration for the sums and the emissions, 2 n sequential steps of one wave
 * for the forward-backward, n more of one lane per speaker for the priors.
 * ws >= vm_vbx_workspace_bytes(N, D, R, em_total): three float64 per row (G, c, m) and three per emission (p, a, b), each table rounded
 * up to 256 bytes: 3 pad(8 N) + 3 pad(8 em_total). */
enum { VM_VBX_MAX_K = 64 };
int64_t vm_vbx_workspace_bytes(int64_t N, int D, int64_t R, int64_t em_total);
int vm_vbx(const float* rows, int64_t N, int P, int D, const int64_t* row0, const int64_t* em0, int64_t R, int64_t em_total,
           const int32_t* n_models, const int32_t* labels_in, const int32_t* chain_start, const double* psi, const double* r,
           const double* ib, double loop_prob, double fa, double fb, double init_smooth, double epsilon, int iters,
           const double* gamma_in, const double* pi_in, int32_t* labels_out, double* gamma, double* pi, double* elbo,
           int32_t* iters_run, void* ws, void* stream);

/* ---- the PLDA back end (csrc/plda.hip, voicemap_amd/plda.py): the statistics of the fit and the projection into PLDA space -----------
 * vm_scatter_f64: out (D, D) float64 = sum over the rows r of x (N, D) fp32 with label[r] >= 0 (label NULL: all rows) of
 * (x_r - mean)(x_r - mean)^T.  mean (D) float64 ON THE DEVICE.  Arithmetic: d = (double)x - mean, rounded once; per entry an fma chain over
 * ascending rows within a chunk of vm_scatter_f64_chunk_rows() rows, the chunks' partials (in ws) summed in ascending chunk order by a
 * second launch.  Only i <= j is computed and the entry is stored on both sides: out is exactly symmetric.  No float atomics:
 * bit-identical from run to run.  0 < D <= 256, 0 < N < 2^31; mean, out, ws 8-byte aligned; ws >= vm_scatter_f64_workspace_bytes(N, D)
 * (one (D, D) partial per chunk).  Per-speaker sums and counts are vm_speaker_sums' (euclidean kind).
 * vm_plda_project: rows x (N, E) fp32 -> out (N, P) fp32.  mean (E), A (D, E) row-major, quad (D) or NULL: float64 on the device.
 *   y_d = sum_e A[d][e] * ((double)x_e - mean_e), float64, ascending e (fma chain);
 *   length_norm != 0:  y_d <- (y_d * sqrt((double)D)) / |y|,  |y| = sqrt(sum_d y_d^2), ascending d, every product and sum rounded on its
 *   own; a row with |y| == 0 stays zero;
 *   out[.][d] = (float)y_d.
 *   quad == NULL: P == D.  Otherwise P == 4 * ceil((D + 1) / 4): a PLDA-space row (VM_SCORE_PLDA) -- columns D .. P - 2 are zero and
 *   column P - 1 = (float)(sum_d quad[d] * (v_d * v_d) + c0), v_d the STORED fp32 value widened to float64, ascending d, every operation
 *   rounded on its own.
 * 0 < D, E <= 255, 0 < N < 2^31; c0 finite; out 16-byte aligned when P % 4 == 0 (then it is written 16 bytes at a time). */
int vm_scatter_f64_chunk_rows(void);
int64_t vm_scatter_f64_workspace_bytes(int64_t N, int D);
int vm_scatter_f64(const float* x, const int32_t* label, const double* mean, int64_t N, int D, double* out, void* ws, void* stream);
int vm_plda_project(const float* x, const double* mean, const double* A, int64_t N, int E, int D, int length_norm, const double* quad,
                    double c0, float* out, int P, void* stream);
/* Multi-session PLDA speaker models (csrc/plda_enrol.hip, voicemap_amd/enrolment.py enrol(plda=...)): a query row against a speaker model
 * of n enrolment rows, scored by minus the two-covariance log-likelihood ratio of the row against the n rows together.  In the
 * diagonalised space z = V^T (x - mu) (within covariance I, between covariance diag(psi)) the ratio depends on the enrolment rows only
 * through their sum and n.  Stated on the columns w = sqrt(b) z, b = psi / (1 + 2 psi), of PLDA-space rows (vm_plda_project with quad):
 *   beta[n][d] = psi_d / (1 + n psi_d),  A[n][d] = (1 + n psi_d) / (2 b_d (1 + (n + 1) psi_d)),  G[d] = 1 / (2 b_d (1 + psi_d)),
 *   C[n] = 1/2 sum_d log((1 + psi_d)(1 + n psi_d) / (1 + (n + 1) psi_d)),
 *   score(m, s) = -llr = sum_d A[n][d] (w_md - beta[n][d] Sigma_sd)^2 - sum_d G[d] w_md^2 - C[n],  lower = more alike;
 * at n = 1 it is VM_SCORE_PLDA's quantity.  The entry points take the tables as they are (PldaModel.model_tables makes them); nothing
 * here depends on their coming from a psi.
 * Inputs.  q (M, P) fp32 PLDA-space rows, of which only columns 0 .. D - 1 are read; q_label (M) as in vm_speaker_identify.  sums (S, P)
 * float64 and count (S) int32: vm_speaker_sums' with VM_DIST_EUCLIDEAN on the enrolled PLDA-space rows (E = P); columns >= D are ignored.
 * A, beta: (n_max + 1, D) float64 row-major, C: (n_max + 1), G: (D) float64, all on the device; row 0 is never read.
 * Arithmetic, float64 until ONE rounding to fp32, every operation rounded on its own unless it is written as fma:
 *   n = count_s, Sigma = sum_s; with leave_one_out != 0 and q_label[m] == s: n = count_s - 1 and Sigma_d = sum_sd - (double)w_md.
 *   (m, s) is NOT A TRIAL, and is counted nowhere, unless 1 <= n <= n_max (the launcher cannot see count).
 *   mu_d = beta[n][d] * Sigma_d;  t = (double)w_md - mu_d;  u = A[n][d] * t;  acc = fma(u, t, acc), ascending d from 0.0;
 *   g_m = fma(G[d], (double)w_md * (double)w_md, g_m), ascending d from 0.0;
 *   score = (float)((acc - g_m) - C[n]).
 * Outputs and order: exactly vm_speaker_identify's (scores (M, S) may be NULL and holds NaN where (m, s) is not a trial; the order of the
 * trials of one query is (uint32 key, speaker) with NaN last; rank, best_idx, best_val, true_score) and vm_speaker_trial_hist's (window,
 * slot and NaN-slot conventions and limits; hist is ACCUMULATED).  The two entry points score bit-identically; no float atomics: the
 * outputs are a function of the inputs alone.
 * Limits.  1 <= D < P <= 256, P % 4 == 0, M, S < 2^31, S >= 1, n_max >= 1; q 16-byte aligned, sums and the tables 8-byte aligned.  A bad
 * argument is an error before any launch.  M == 0 returns without a launch.  ws >= the matching *_workspace_bytes(M, D, S).
 * Launches: the per-speaker operands mu_s, A[count_s], C[count_s] (one workgroup per speaker); g_m and the own-speaker score (one thread
 * per row); the tile kernel, 64 rows x 64 models per step with w, mu and A staged through LDS as float64 in chunks of 16 components. */
int64_t vm_plda_speaker_identify_workspace_bytes(int64_t M, int D, int64_t S);
int vm_plda_speaker_identify(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums, const int32_t* count,
                             int64_t S, const double* A, const double* beta, const double* C, const double* G, int n_max,
                             int leave_one_out, float* scores, float* true_score, int32_t* rank, float* best_val, int32_t* best_idx,
                             void* ws, void* stream);
int64_t vm_plda_speaker_trial_hist_workspace_bytes(int64_t M, int D, int64_t S);
int vm_plda_speaker_trial_hist(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums, const int32_t* count,
                               int64_t S, const double* A, const double* beta, const double* C, const double* G, int n_max,
                               int leave_one_out, const int64_t* host_windows, int n_windows, int bins, uint64_t* hist, void* ws,
                               void* stream);
/* Score normalisation of speaker-model trials: S-norm / AS-norm (csrc/enrol_norm.hip, voicemap_amd/enrolment.py model_score_norm).
 * Notation of the two blocks above (vm_speaker_sums ... vm_plda_speaker_trial_hist).  score(r, model) is the fp32 trial score of that
 * block for the back end in use -- float64, rounded once -- and NaN where the model has no rows: n == 0, or for PLDA n outside 1..n_max.
 * Cohort.  A set of C rows other than the query rows and the enrolled rows, used two ways: as C cohort ROWS, and as S_c cohort MODELS
 * (vm_speaker_sums over all of its rows, with the kind / the PLDA tables of the enrolled models).
 * Three sets of statistics, each selected and reduced by exactly vm_cohort_topk_stats' rules: NaN scores are skipped; K' = min(K,
 * remaining); the K' smallest by (uint32 score key with -0.0 as +0.0, index) ascending; mu the mean and sigma the population standard
 * deviation, accumulated in float64 in a fixed order and rounded to fp32 once; rsig = (float)(1.0 / (double)sigma); K' = 0 gives NaN,
 * sigma = 0 gives rsig = +inf; count = K'; the optional topk_idx (lines, K) int32 in (key, index) order, padded with -1.
 *   1. Query side: for every query row m, over the cohort models s_c, score(q_m, cohort model s_c): mu_q, rsig_q (M).
 *   2. Model side: for every enrolled model s, over the cohort rows c, score(cohort row c, model s): mu_s, rsig_s (S).
 *   3. Own side, leave-one-out only: query row m sees its own speaker's model without itself -- Sigma = sum_s - c_m, msum likewise,
 *      n = count_s - 1 -- and that VIRTUAL model has its own statistics over the cohort rows: mu_own, rsig_own (M), NaN where the row
 *      has no own model.
 *   The scores of sets 1 and 2 are bit-identical to vm_speaker_identify's (vm_plda_speaker_identify's) `scores` matrix for the same
 *   operands with leave_one_out = 0; those of set 3 to that matrix with the virtual models as the models.
 * Normalised trial score, fp32, every operation rounded on its own (no contraction into fma), as vm_pair_score_hist_norm:
 *   a = s - mu_q[m];  b = s - mu_M;  s' = 0.5f * (a * rsig_q[m] + b * rsig_M)
 * with (mu_M, rsig_M) = (mu_own[m], rsig_own[m]) when leave_one_out != 0 and s == q_label[m], and (mu_s[s], rsig_s[s]) otherwise.
 * Trials, classes, windows, slots, the NaN slot, accumulation and limits are exactly vm_speaker_trial_hist's.
 * vm_speaker_loo_sums: the virtual model of every row of q (M, E) / q_label (M): out_sums (M, E) f64, out_msum (M) f64, out_count (M)
 *   int32.  c_m and |e_m| are formed exactly as vm_speaker_sums forms them; one float64 subtraction per component.  A row whose q_label
 *   is outside [0, S), or whose speaker has count <= 1, gets count 0 and zeros.  With kind = VM_DIST_EUCLIDEAN and E = P it serves
 *   PLDA-space rows (Sigma_d = sum_sd - (double)w_md).  ws >= vm_speaker_loo_sums_workspace_bytes(M, E).
 * vm_speaker_cohort_stats: rows q (M, E) against the models sums / msum / count (S).  side = 0: per row over the S models (outputs of
 *   length M); side = 1: per model over the M rows (outputs of length S).  topk_idx may be NULL.  K >= 1.  The scores are written a
 *   chunk of lines at a time by vm_speaker_identify itself into a tile of at most ~192 MB in ws (vm_cohort_topk_stats' cap) and
 *   selected down its rows (side 0) or its columns (side 1).  ws >= vm_speaker_cohort_stats_workspace_bytes(M, E, S, side).
 * vm_plda_speaker_cohort_stats: the same with P, D and the tables A, beta, C, G, n_max in place of msum and kind, as
 *   vm_plda_speaker_identify takes them.  ws >= vm_plda_speaker_cohort_stats_workspace_bytes(M, D, S, side).
 * vm_speaker_trial_hist_norm / vm_plda_speaker_trial_hist_norm: the histograms of s'.  mu_q, rsig_q (M, indexed like q), mu_s, rsig_s (S)
 *   fp32 on the device; mu_own, rsig_own (M) are NULL together, must be NULL when leave_one_out == 0 and are needed when it is not.
 *   ws >= the matching *_workspace_bytes (those of the plain histograms).
 * Every bad argument is an error before any launch, outputs untouched; M == 0 returns without a launch.  No float atomics: every output
 * is bit-identical from run to run. */
int64_t vm_speaker_loo_sums_workspace_bytes(int64_t M, int E);
int vm_speaker_loo_sums(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                        const int32_t* count, int64_t S, int kind, double* out_sums, double* out_msum, int32_t* out_count, void* ws,
                        void* stream);
int64_t vm_speaker_cohort_stats_workspace_bytes(int64_t M, int E, int64_t S, int side);
int vm_speaker_cohort_stats(const float* q, int64_t M, int E, const double* sums, const double* msum, const int32_t* count, int64_t S,
                            int kind, int side, int64_t K, float* mu, float* sigma, float* rsig, int32_t* cnt, int32_t* topk_idx, void* ws,
                            void* stream);
int64_t vm_plda_speaker_cohort_stats_workspace_bytes(int64_t M, int D, int64_t S, int side);
int vm_plda_speaker_cohort_stats(const float* q, int64_t M, int P, int D, const double* sums, const int32_t* count, int64_t S,
                                 const double* A, const double* beta, const double* C, const double* G, int n_max, int side, int64_t K,
                                 float* mu, float* sigma, float* rsig, int32_t* cnt, int32_t* topk_idx, void* ws, void* stream);
int64_t vm_speaker_trial_hist_norm_workspace_bytes(int64_t M, int E, int64_t S);
int vm_speaker_trial_hist_norm(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                               const int32_t* count, int64_t S, int kind, int leave_one_out, const int64_t* host_windows, int n_windows,
                               int bins, const float* mu_q, const float* rsig_q, const float* mu_s, const float* rsig_s,
                               const float* mu_own, const float* rsig_own, uint64_t* hist, void* ws, void* stream);
int64_t vm_plda_speaker_trial_hist_norm_workspace_bytes(int64_t M, int D, int64_t S);
int vm_plda_speaker_trial_hist_norm(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                    const int32_t* count, int64_t S, const double* A, const double* beta, const double* C, const double* G,
                                    int n_max, int leave_one_out, const int64_t* host_windows, int n_windows, int bins, const float* mu_q,
                                    const float* rsig_q, const float* mu_s, const float* rsig_s, const float* mu_own,
                                    const float* rsig_own, uint64_t* hist, void* ws, void* stream);
/* Calibration of speaker-model trials (csrc/enrol_tile.hpp CALIB mode, csrc/calib_terms.hpp, voicemap_amd/enrolment.py
 * fit_model_calibration / model_cllr / model_detection_costs): vm_pair_calib_sums' sums over the trials of vm_speaker_trial_hist.
 * Trials, scores, leave-one-out, the not-a-trial rule and the limits are exactly those of vm_speaker_trial_hist
 * (vm_plda_speaker_trial_hist): every (m, s) whose model exists is a trial, class 0 (target) iff s == q_label[m], class 1 otherwise; s
 * is the fp32 score of that entry point, bit-identical to vm_[plda_]speaker_identify's `scores` matrix.  A cell that is not a trial
 * -- no model, row >= M, model >= S -- adds nothing anywhere.
 * Statistics.  mu_q, rsig_q, mu_s, rsig_s, mu_own, rsig_own all NULL: the raw scores.  Otherwise they are
 * vm_[plda_]speaker_trial_hist_norm's, under its rules (mu_own / rsig_own NULL together, NULL without leave_one_out, needed with it),
 * and s is replaced by its normalised score s', in exactly that fp32 order.
 * Per-trial terms and the eight sums per class: exactly vm_pair_calib_sums' (float64, every operation rounded on its own); a trial
 * whose s is NaN or infinite adds to n_skipped alone.  calib (2, 8) float64 on the device is WRITTEN, not accumulated (row ranges and
 * ranks are added by the caller):  n, n_skipped, L, P0, P1, W0, W1, W2.  The counts are exact.  M == 0 writes zeros.
 * Determinism.  The grid is the histogram's: ceil(M / 64) query tiles x vm_speaker_trial_calib_sums_splits(M, S) splits of the 64-model
 * tiles (0 if M or S <= 0; the same for both back ends).  Per-lane float64 accumulators (u32 counts) carried over the workgroup's tiles
 * in ascending order, a fixed shuffle tree per wave, the four waves in order, one column of partials per workgroup in ws (zeros where a
 * split holds no tile), and vm_pair_calib_sums' fixed-order final sum in a second launch.  No floating-point atomics: bit-identical
 * from run to run for the same arguments; a row range cut into several calls sums in another order (within rounding).
 * a, b, tau finite; calib 8-byte aligned.  Every bad argument is an error before any launch.  ws >= the matching *_workspace_bytes. */
int64_t vm_speaker_trial_calib_sums_splits(int64_t M, int64_t S);
int64_t vm_speaker_trial_calib_sums_workspace_bytes(int64_t M, int E, int64_t S);
int vm_speaker_trial_calib_sums(const float* q, const int32_t* q_label, int64_t M, int E, const double* sums, const double* msum,
                                const int32_t* count, int64_t S, int kind, int leave_one_out, const float* mu_q, const float* rsig_q,
                                const float* mu_s, const float* rsig_s, const float* mu_own, const float* rsig_own, double a, double b,
                                double tau, double* calib, void* ws, void* stream);
int64_t vm_plda_speaker_trial_calib_sums_workspace_bytes(int64_t M, int D, int64_t S);
int vm_plda_speaker_trial_calib_sums(const float* q, const int32_t* q_label, int64_t M, int P, int D, const double* sums,
                                     const int32_t* count, int64_t S, const double* A, const double* beta, const double* C,
                                     const double* G, int n_max, int leave_one_out, const float* mu_q, const float* rsig_q,
                                     const float* mu_s, const float* rsig_s, const float* mu_own, const float* rsig_own, double a, double b,
                                     double tau, double* calib, void* ws, void* stream);

/* ---- a10 / f4: log-mel front-end and the 2-D CNN encoder variant (BASELINE.json config 4) -------------------
 * NOT in the reference (nothing to cite under /root/reference); the specification is DESIGN.md section 9 and the
 * CPU oracle is oracle/voicemap_oracle.py (logmel_features, encoder2d_forward): parity unpinned by construction.
 *
 * vm_stft_logmel: raw (n_clips, raw_len) fp32 or int16 16 kHz windows -> frames of win_length samples every `hop` samples
 * (T = vm_stft_frames: no centre padding), 512-point DFT of the windowed frame, power of bins 0..255, mel projection, log:
 *   out[(b * n_mels + m)][1 + t] = log(sum_k melw[k][m] * |X_t[k]|^2 + log_floor)
 * written in `dtype` as the block-1 input of the 2-D encoder: n_clips * n_mels windows of T + 2 rows (halo rows are not
 * written: the caller zeroes the buffer once), 1 channel.  basis: (win_length, 512) fp32 = the analysis window times
 * [cos(2 pi k n / 512) for k < 256 | -sin(2 pi k n / 512) for k < 256]; melw: (256, n_mels) fp32; both built by the host side
 * (voicemap_amd/spectro.py).  n_mels in {32, 64, 96, 128}.  win_length in 2 .. 512, as far as the device's LDS goes: a workgroup holds
 * 32 frames, 32 * (win_length + 1) * 4 bytes here and 2 * 32 * (round_up(win_length, 16) + 8) * 2 bytes in the f16 entry points below --
 * 65 664 bytes at win_length = 512 and 66 560 bytes at win_length > 496, both past 64 KiB.  Every entry point compares its need with the
 * device's per-block limit (hipDeviceAttributeMaxSharedMemoryPerBlock; 160 KiB on an MI355X, which runs 512) and fails with an error,
 * `out` untouched, where the limit is lower. */
int64_t vm_stft_frames(int64_t raw_len, int win_length, int hop);
int vm_stft_logmel(const void* raw, int is_int16, int64_t n_clips, int64_t raw_len, int win_length, int hop, const float* basis,
                   const float* melw, int n_mels, float log_floor, int dtype, void* out, void* stream);
/* vm_stft_logmel with the DFT on the f16 matrix pipe: the windowed basis and the (x 256) samples are split into two f16 halves each
 * (22 significand bits) and the three significant products accumulated in fp32 -- ~2^-21 relative per product against fp32's 2^-24, at
 * 1/5 of the matrix time (an fp32 MFMA moves K = 2 per 64 clocks).  Meant for the 16-bit storage modes, whose log-mel image is rounded
 * to 11 / 8 significand bits anyway; the fp32-storage mode keeps vm_stft_logmel.  basis16: vm_stft_split_basis_bytes(win_length) bytes
 * filled ONCE by vm_stft_split_basis from the fp32 basis; everything else as vm_stft_logmel. */
int64_t vm_stft_split_basis_bytes(int win_length);
int vm_stft_split_basis(const float* basis, int win_length, void* basis16, void* stream);
int vm_stft_logmel_f16s(const void* raw, int is_int16, int64_t n_clips, int64_t raw_len, int win_length, int hop, const void* basis16,
                        const float* melw, int n_mels, float log_floor, int dtype, void* out, void* stream);
/* ... which also leaves what the 16-bit storage type dropped as a second plane of the same layout: out_lo = image - out, rounded to
 * `dtype` (halo rows not written).  The log-mel image is the one tensor of the variant with a pedestal (mean -1.7, range -10 .. 5 on
 * speech-like clips) and ONE channel: its 11-bit rounding alone moved config 4's embeddings by 7.7e-4 of the 1e-3 budget
 * (tools/probe/config4_storage_sites.py); two planes cost 2 bytes per pixel more.  16-bit storage only. */
int vm_stft_logmel_f16s_split(const void* raw, int is_int16, int64_t n_clips, int64_t raw_len, int win_length, int hop, const void* basis16,
                              const float* melw, int n_mels, float log_floor, int dtype, void* out, void* out_lo, void* stream);
/* First Conv2D(3 x 3) of the variant (one input channel) with its own kernels instead of as a band-stacked GEMM with K = 24, N = 32
 * (16-bit storage and C % 32 == 0: one v_mfma_f32_32x32x16 per 32 positions x 32 channels, the nine taps as K, and
 * v_mfma_f32_16x16x32 tiles with the positions as K for the gradient; otherwise on the vector ALUs):
 * in: block input (n_clips * M, L + 2, 1) `dtype` with zero halo rows; w: the fp32 kernel (3, Cs, C) of the flat store (Cs >= 3, the
 * entries km >= 3 are padding), rounded to `dtype` inside like the GEMM path's copy; z (n_clips * M, L, C) = relu(conv + bias);
 * stat_sum / stat_sq (optional): the BatchNorm partial sums of the stored z, vm_conv_stat_rows(L) rows per window.  C % 8 == 0,
 * C <= 128.  vm_conv2d_first_wgrad: the matching kernel gradient (3, Cs, C) from du (n_clips * M, L + 2, C) (padding entries 0);
 * the layer has no input gradient. */
int vm_conv2d_first_supported(int C, int dtype);
int vm_conv2d_first_fwd(const void* in, const float* w, const float* bias, int64_t n_clips, int M, int64_t L, int Cs, int C, int dtype,
                        void* z, float* stat_sum, float* stat_sq, void* stream);
/* vm_conv2d_first_fwd on the two-plane image (in + in_lo of vm_stft_logmel_f16s_split) with the filters split the same way inside
 * (w = w_hi + w_lo, both `dtype`): the three significant products in w_hi + in_lo w_hi + in w_lo are 27 of the 32 K slots of TWO
 * matrix instructions per 32 positions x 32 channels, fp32 accumulation -- image and filters enter at ~2 x the storage significand
 * (the layer has 9 taps and one input channel: the second instruction is the whole price).  Same z layout, statistics and rounding
 * of the stored z as vm_conv2d_first_fwd; the weight gradient keeps vm_conv2d_first_wgrad on the high plane.  z_lo (optional): what
 * the storage type dropped of relu(conv + bias) as a second plane of z's layout.  The statistics are those of the two-plane value
 * (z + z_lo, stored or not): what vm_conv2d_first_bn_pool_stack recomputes and vm_bn_pool2d_stack_fwd_split reads back (the backward
 * keeps reading z alone).  16-bit storage and C % 32 == 0 only. */
int vm_conv2d_first_fwd_split(const void* in, const void* in_lo, const float* w, const float* bias, int64_t n_clips, int M, int64_t L, int Cs,
                              int C, int dtype, void* z, void* z_lo, float* stat_sum, float* stat_sq, void* stream);
int64_t vm_conv2d_first_wgrad_workspace_bytes(int64_t n_clips, int M, int C);
int vm_conv2d_first_wgrad(const void* in, const void* du, int64_t n_clips, int M, int64_t L, int Cs, int C, int dtype, void* ws,
                          float* grad_w, void* stream);
/* Conv2D(3 x 3, SAME) over (T, M) = the k = 3 convolution along T (vm_conv_fwd / _dgrad / _wgrad) of the band-stacked tensor:
 * x: (n_clips * M windows, rows, C) with rows = T + 2 (halo rows included: they are copied, so they stay zero);
 * out: (n_clips * M, rows, Cs), out[(b, m)][row][dm * C + c] = x[(b, m + dm - 1)][row][c] (0 outside the clip's M bands),
 * channels [3 C, Cs) = 0 (Cs >= 3 C, a multiple of 8 for the convolution kernels).  W2d[kt][km][ci][co] = W1d[kt][km * C + ci][co]. */
int vm_stack_windows(const void* x, int64_t n_clips, int M, int64_t rows, int C, int Cs, int dtype, void* out, void* stream);
/* adjoint of vm_stack_windows on un-padded rows: dxs (n_clips * M, L, Cs) -> dx (n_clips * M, L, C),
 * dx[(b, m)][t][c] = sum_dm dxs[(b, m - dm + 1)][t][dm * C + c].  src_padded != 0: dxs is (n_clips * M, L + 2, Cs) and rows 1 .. L of a
 * window are read -- the layout a dgrad over a clip's concatenated windows leaves (its outputs at the halo positions are not used). */
int vm_fold_windows(const void* dxs, int64_t n_clips, int M, int64_t L, int C, int Cs, int src_padded, int dtype, void* dx, void* stream);
/* mel half of MaxPool2D(2, 2): out[(b, m')][row][c] = max(q[(b, 2m')], q[(b, 2m'+1)]) over (n_clips * M, rows, C) -> (n_clips *
 * (M / 2), rows, C) (floor: an odd last band is dropped); backward: q as in the forward (rows = L + 2 with halo), dout (n_clips *
 * (M / 2), L, C), dq (n_clips * M, L, C) = dout routed to the first maximum of each pair. */
int vm_pool_windows_fwd(const void* q, int64_t n_clips, int M, int64_t rows, int C, int dtype, void* out, void* stream);
int vm_pool_windows_bwd(const void* q, const void* dout, int64_t n_clips, int M, int64_t L, int C, int dtype, void* dq, void* stream);
/* One block boundary of the 2-D variant in one pass (round 3; bit-identical to the three / two passes they replace):
 * vm_bn_pool2d_stack_fwd = vm_bn_drop_pool_fwd(pool 2) -> vm_pool_windows_fwd -> vm_stack_windows.  z (n_clips * M, L, C), scale / shift
 * (towers, C) with `clips_per_tower` clips a tower, drop (n_clips * M, C) or NULL; writes q (n_clips * M, L / 2 + 2, C) rows 1 .. L / 2
 * (kept for the backward) and the stacked block input xs (n_clips * (M / 2), L / 2 + 2, Cs).  NEITHER tensor's halo rows, out-of-clip band
 * slots or channels [3 C, Cs) are written: zero both once after allocation.  C, Cs multiples of the 16-byte vector.
 * vm_fold_pool_windows_bwd = vm_fold_windows -> vm_pool_windows_bwd: dxs (n_clips * (M / 2), L (+ 2 if src_padded), Cs) and q as above
 * (L = its un-padded rows) -> dq (n_clips * M, L, C).  s0 / sa (optional, both or neither; (n_clips * M * vm_fold_pool_windows_rows(...), C)
 * fp32): the sums of dq and of dq * q per window and workgroup row -- what vm_bn_bwd_from_sums_finalize(..., rows_per_window =
 * vm_fold_pool_windows_rows, a_is_act = 1) turns into the BatchNorm-backward constants of the block below without a pass over (z, dq). */
int vm_bn_pool2d_stack_fwd(const void* z, const float* scale, const float* shift, const float* drop, int64_t n_clips, int M,
                           int64_t clips_per_tower, int64_t L, int C, int Cs, int dtype, void* q, void* xs, void* stream);
/* Block 1's boundary without the round trip of z: given the BatchNorm affine (the statistics come from vm_conv2d_first_fwd_split, which
 * also leaves z for the backward), RECOMPUTE relu(conv + bias) on the two-plane image -- nine taps of a cache-resident one-channel
 * image: cheaper than reading z back -- apply scale / shift (+ drop) to the fp32 accumulator, pool 2 x 2 and write what
 * vm_bn_pool2d_stack_fwd writes (q per band, the band-stacked xs from the STORED q values; same layouts, same never-written halo /
 * out-of-clip / padding entries).  The rounding of block 1's conv output is gone from the forward (5.0e-4 of config 4's f16 embedding
 * error) and so are its bytes.  in / in_lo / w / bias / Cs as vm_conv2d_first_fwd_split; scale / shift (towers, C); drop (n_clips * M, C)
 * or NULL; Cs2 = channel pitch of xs (>= 3 C).  16-bit storage, C in {32, 64, 96, 128}. */
int vm_conv2d_first_bn_pool_stack(const void* in, const void* in_lo, const float* w, const float* bias, const float* scale, const float* shift,
                                  const float* drop, int64_t n_clips, int M, int64_t clips_per_tower, int64_t L, int Cs, int C, int Cs2,
                                  int dtype, void* q, void* xs, void* stream);
/* vm_bn_pool2d_stack_fwd on a z that came as two planes (vm_conv2d_first_fwd_split): the affine is taken of z + z_lo in fp32. */
int vm_bn_pool2d_stack_fwd_split(const void* z, const void* z_lo, const float* scale, const float* shift, const float* drop, int64_t n_clips,
                                 int M, int64_t clips_per_tower, int64_t L, int C, int Cs, int dtype, void* q, void* xs, void* stream);
int64_t vm_fold_pool_windows_rows(int64_t L, int C, int Cs, int dtype);
int vm_fold_pool_windows_bwd(const void* dxs, const void* q, int64_t n_clips, int M, int64_t L, int C, int Cs, int src_padded, int dtype,
                             void* dq, float* s0, float* sa, void* stream);
/* mel half of GlobalMaxPool2D: out[b][c] = max over m < M_valid of gmax[(b, m)][c] (fp32; first maximum -> widx[b][c]);
 * backward: dg[(b, m)][c] = dout[b][c] if m == widx[b][c] else 0. */
int vm_clip_max_fwd(const float* gmax, int64_t n_clips, int M, int M_valid, int C, float* out, int32_t* widx, void* stream);
int vm_clip_max_bwd(const float* dout, const int32_t* widx, int64_t n_clips, int M, int C, float* dg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VOICEMAP_HIP_H */
