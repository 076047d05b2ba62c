/*
 * rvc_amd.h -- C ABI of librvc_amd.so: the MI355X (gfx950) kernels of the RVC inference hot path and of the tools around
 * training that share them (feature extraction, index build, dataset preprocessing, checkpoint validation).
 *
 * The reference (codename0og/codename-rvc-fork-3) is 100 % Python: it has no FFI / plugin interface,
 * the boundary it offers is Python method signatures.  Each entry point below replaces
 * the body of one reference call; the reference-side binding a maintainer would add is a ctypes stub,
 * shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer named *_dev is a device (HBM) address owned by the caller (e.g. torch tensor.data_ptr());
 *     *_host pointers are host addresses; nothing here allocates caller-visible memory;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); every launch is
 *     asynchronous on it; 0 / NULL = the default stream;
 *   - every function returns 0 on success, non-zero on error; rvc_last_error() describes the last failure
 *     of the calling thread;
 *   - a handle is bound to the device that was current when it was created; distinct handles are independent.
 *     rvc_decoder_forward only READS the handle (weights, tables) and works in the caller's workspace, so several threads
 *     may run forwards of one handle concurrently, each with its own stream and workspace (VoiceConverter.convert_batch
 *     does); create / set_tensor / finalize / set_tap / destroy must not overlap any other call on the same handle;
 *   - a process may drive several devices, one host thread per device, with that device current on the calling thread for
 *     every call (the handles and *_dev pointers it passes live there).  What the library sets or uploads once -- kernel
 *     attributes, its built-in tables -- is kept per device;
 *   - tensors are dense, row-major, fp32 unless said otherwise.
 */
#ifndef RVC_AMD_H
#define RVC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVC_AMD_ABI_VERSION 4   /* 3: round-5 additions (K3f, K12-K14, branch streams); 4: round-6 additions (K3f / K3d with one-term taps, K3f's runtime switch, K3u, K10b); no existing signature changed */

/* ---- library ------------------------------------------------------------------------------------ */

int rvc_abi_version(void);
/* NUL-terminated description of the calling thread's last error ("" if none). */
const char *rvc_last_error(void);

/* ---- K1: feature retrieval --------------------------------------------------------------------- *
 * Replaces `index.search(npy, k=8)` + the weighting/blend of
 * rvc/infer/pipeline.py:497-507 (`Pipeline._retrieve_speaker_embeddings`), where `index` is the faiss
 * index read at pipeline.py:555 and `big_npy = index.reconstruct_n(0, ntotal)` (pipeline.py:556).
 * Search is exact brute-force squared L2 over big_npy (faiss IndexFlat semantics: ascending distance,
 * ties -> lower id).  The returned distances are sum_k (q_k - x_k)^2 evaluated in fp32 in a fixed order (faiss' flat
 * scanner form), identical whichever internal regime finds the candidates:
 *   <= 64 queries            one streaming pass over the fp32 index (HBM-bound)
 *   more, >= 16384 rows      fp16 matrix-core screening pass with a proven error bound -> candidate superset -> exact
 *                            re-scoring (csrc/knn_screen.hip); a query whose candidate list overflows is answered by an
 *                            exact scan inside the same call
 *   otherwise                fp32 matrix-core GEMM with per-lane top-8 lists
 */

/* Per-index derived data, built once when the index is loaded ("aux" blob, opaque, caller-owned device memory):
 * ||x_n||^2, an fp16 copy of the rows, and the index-wide maxima the screening bound needs. */
int rvc_knn_index_aux_bytes(int64_t n_rows, int dim, size_t *bytes);
int rvc_knn_index_build(const float *index_dev, int64_t n_rows, int dim, void *aux_dev, size_t aux_bytes, void *stream);

/* bytes of scratch rvc_knn_search needs for (n_rows, n_queries, dim).  In the fp16-screened regime (> 64 queries, >= 16384 rows)
 * this is ~42 KB per query (8192 candidate ids + up to 2048 sample minima + the fp16 copy of the query): 67 MB at the 1599
 * queries of a 30 s clip.  The scratch is per concurrent search -- a caller with several streams in flight holds one per
 * stream -- and grows linearly with n_queries: split very long query sets rather than sizing for them. */
int rvc_knn_workspace_bytes(int64_t n_rows, int64_t n_queries, int dim, int k, size_t *bytes);

/* out_d2_dev [n_queries,k] squared distances ascending; out_ids_dev [n_queries,k] int64 row ids (-1 where the index has
 * fewer than k rows). k must be 8, dim % 32 == 0.  aux_dev: what rvc_knn_index_build filled for this index. */
int rvc_knn_search(const float *index_dev, const void *aux_dev, int64_t n_rows, int dim,
                   const float *queries_dev, int64_t n_queries, int k,
                   float *out_d2_dev, int64_t *out_ids_dev,
                   void *workspace_dev, size_t workspace_bytes, void *stream);

/* Exact ranking of caller-supplied candidates: for every query the best k of the rows listed in cand_ids_dev
 * [n_queries][cap] (int32 row ids, negative = empty) by sum_k (q_k - x_k)^2, ties -> lower id; -1 / +inf where fewer than k
 * candidates exist.  This is the last step of every rvc_knn_search regime, exported for the inverted-file mode: a faiss
 * `IVF{n},Flat` index searched with nprobe lists (extract_index.py:62-64, pipeline.py:499) is "nearest nprobe centroids
 * (rvc_knn_search over the centroids), then rank the members of those lists".  dim: 256, 512, 768 or 1024. */
int rvc_knn_rank_candidates(const float *index_dev, const void *aux_dev, int64_t n_rows, int dim, const float *queries_dev,
                            int64_t n_queries, const int32_t *cand_ids_dev, int cap, int k, float *out_d2_dev,
                            int64_t *out_ids_dev, void *stream);

/* Test hook, per calling thread (searches issued by other host threads keep choosing by shape): 0 = choose the regime by
 * shape (default), 1 = never screen (fp32 GEMM / streaming only), 2 = screen whenever the shape allows it (>= 4096 rows,
 * dim a multiple of 256).  Results do not depend on it.  Candidate ids handed to rvc_knn_rank_candidates that are negative
 * or >= n_rows are ignored. */
int rvc_knn_set_mode(int mode);

/* pipeline.py:500-506: w = (1/d2)^2, w /= sum(w); out = index_rate * sum_k w_k * index[id_k] + (1-index_rate) * feats.
 * feats_dev/out_dev: [n_queries, dim] (may alias).  Neighbours with id < 0 (index smaller than k) are left out of the
 * sums; d2 == 0 is not guarded, as in the reference (an exact duplicate of a query gives inf/inf there too). */
int rvc_knn_blend(const float *index_dev, int dim, const float *feats_dev, const float *d2_dev,
                  const int64_t *ids_dev, int64_t n_queries, int k, float index_rate,
                  float *out_dev, void *stream);

/* ---- K4: RMVPE log-mel front end --------------------------------------------------------------- *
 * Replaces `MelSpectrogram.forward(audio, center=True)` as configured at
 * rvc/lib/predictors/RMVPE.py:438 (n_fft = win = 1024, hop 160, 128 HTK mel bands 30-8000 Hz,
 * log(clamp(., 1e-5)); forward at RMVPE.py:388-417) and the reflect pad of the frame axis to a multiple
 * of 32 done in `mel2hidden` (RMVPE.py:452-455).
 * audio_dev: [batch, n_samples]; mel_dev: [batch, 128, n_frames_padded] where n_frames = n_samples/160 + 1 and
 * n_frames_padded >= n_frames is the row stride (columns >= n_frames are filled by reflection).
 */
int rvc_logmel_workspace_bytes(int batch, int64_t n_samples, size_t *bytes);
int rvc_logmel_rmvpe(const float *audio_dev, int batch, int64_t n_samples, float *mel_dev,
                     int64_t n_frames_padded, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- K4b: the same transform as a handle, for the training-side features --------------------------------------- *
 * Replaces `spectrogram_torch` / `mel_spectrogram_torch` of rvc/train/mel_processing.py:53-146 (feature side of
 * rvc/train/extract): reflect pad `pad` samples per side, frames of n_fft every hop (center = False
 * in torch.stft terms), periodic hann(win_length) centred in n_fft, |X| = sqrt(re^2 + im^2 + mag_eps),
 * mel = log(max(M |X|, log_floor)) with the caller's mel matrix M [n_mels][n_fft/2+1] (host, fp32; librosa.filters.mel in
 * the reference, mel_processing.py:113-119).  The reference's values: n_fft 2048, hop 480 (sr / 100), win 2048,
 * pad (n_fft - hop) / 2, mag_eps 1e-6, log_floor 1e-5, 128 bands at 48 kHz (rvc/configs/48000.json).
 * audio_dev [batch][n_samples]; mel_dev [batch][n_mels][n_frames] and/or spec_dev [batch][n_fft/2+1][n_frames] (either may
 * be NULL); n_frames from rvc_mel_frames.  The handle is read-only after creation. */
typedef struct rvc_mel rvc_mel;
int rvc_mel_create(int n_fft, int hop, int win_length, int pad, float mag_eps, float log_floor, const float *mel_host, int n_mels,
                   rvc_mel **out);
int rvc_mel_destroy(rvc_mel *h);
int rvc_mel_frames(const rvc_mel *h, int64_t n_samples, int64_t *n_frames);
int rvc_mel_workspace_bytes(const rvc_mel *h, int batch, int64_t n_samples, size_t *bytes);
int rvc_mel_forward(const rvc_mel *h, const float *audio_dev, int batch, int64_t n_samples, float *mel_dev, float *spec_dev,
                    void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- input front end: rational resampling --------------------------------------------------------------------- *
 * Replaces `librosa.resample(audio, orig_sr=sr, target_sr=sample_rate, res_type="soxr_vhq")` of `load_audio` /
 * `load_audio_infer` (rvc/lib/utils.py:21-50, 53-85; soxr is third-party and absent: parity unpinned, the filter is this
 * build's own Kaiser design).  y[j] = sum_m h[m] * xup[j * down + (n_taps - 1) / 2 - m] with xup the input zero-stuffed by
 * `up` (scipy.signal.upfirdn / resample_poly convention); float64 throughout. h_dev: the caller's FIR, gain `up`. */
int rvc_resample_poly_f64(const double *x_dev, int64_t n_in, int up, int down, const double *h_dev, int64_t n_taps,
                          double *y_dev, int64_t n_out, void *stream);

/* ---- K6: zero-phase high-pass ------------------------------------------------------------------ *
 * Replaces `signal.filtfilt(bh, ah, audio)` (rvc/infer/pipeline.py:562; 5th-order Butterworth, pipeline.py:23-28)
 * with SciPy's defaults (padtype "odd", padlen 18, lfilter_zi initial conditions), float64, on the device.
 * coef_host (host memory, 17 doubles): b[6], a[6] (a[0] == 1), zi[5] = scipy.signal.lfilter_zi(b, a).
 * x_dev, y_dev: [n] float64 (must not alias), n > 18.  Every chunk of 512 samples starts from a state summed over the `terms`
 * samples in front of it with a tabulated response; `terms` follows the coefficients (4096 for the pipeline's filter, more for
 * slower poles; rvc_filtfilt_order5_terms returns it, host only).  Refused: a non-finite coefficient, a[0] != 1, a pole on or
 * outside the unit circle, poles so slow that the table would pass 2^17 terms.  A refused call writes nothing.  Agrees with an
 * extended-precision evaluation to within a few times SciPy's own float64 error on the same input (csrc/filtfilt.hip). */
int rvc_filtfilt_workspace_bytes(int64_t n, size_t *bytes);
int rvc_filtfilt_order5_terms(const double *coef_host, int64_t *terms);
int rvc_filtfilt_order5(const double *x_dev, int64_t n, const double *coef_host, double *y_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- K5: RMVPE BiGRU recurrence -------------------------------------------------------------- *
 * Replaces the sequential part of `self.gru(x)[0]` (rvc/lib/predictors/RMVPE.py:515-536, nn.GRU(384, 256,
 * num_layers=1, batch_first, bidirectional)).  The caller computes the input projections for all steps with one
 * GEMM: gi_dev [batch][n_steps][2][768] = W_ih x_t + b_ih (direction 0 = forward, 1 = reverse; gate order r,z,n).
 * whhT_dev [2][256][768] = W_hh transposed per direction, bhh_dev [2][768]; out_dev [batch][n_steps][512]
 * (forward hidden in [0,256), reverse in [256,512), as torch lays it out).
 * workspace_dev: rvc_bigru_workspace_bytes() bytes of scratch for the multi-workgroup variant (4 workgroups per
 * direction exchange h through it); NULL selects the single-workgroup-per-direction variant.
 * The multi-workgroup variant needs its 8 workgroups running at the same time.  A launch that shares the GPU with other
 * streams may see them start late; every wait is bounded, and a (batch item, direction) whose wait ran out is
 * recomputed by the single-workgroup recurrence inside the same call (device-side decision, no host round trip).
 * rvc_bigru_status reports, after synchronising `stream`, how many (batch item, direction) pairs of the LAST forward on
 * that workspace were recomputed; rvc_bigru_set_spin_limit changes the bound (polls per wait; 0 restores the default
 * 2^22) -- a test hook to force the recompute path. */
int rvc_bigru_workspace_bytes(int batch, size_t *bytes);
int rvc_bigru_status(const void *workspace_dev, int batch, int *n_redone_host, void *stream);
int rvc_bigru_set_spin_limit(unsigned polls);
int rvc_bigru_forward(const float *gi_dev, const float *whhT_dev, const float *bhh_dev, float *out_dev,
                      int batch, int64_t n_steps, int hidden, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- K7: softmax attention (HuBERT encoder layers, TextEncoder relative-position layers) ------- *
 * Replaces (a) the softmax(Q K^T * scale) V of transformers' HubertAttention inside
 * `model(feats)["last_hidden_state"]` (call site rvc/infer/pipeline.py:450, wrapper rvc/lib/utils.py:31-34; third-party
 * arithmetic, no mask, no dropout at inference) and (b) `MultiHeadAttention.attention` of the TextEncoder
 * (rvc/lib/algorithm/attentions.py:101-141 with the window-10 relative-position terms of :115-141, 143-180; unmasked,
 * i.e. all frames valid).
 * qkv_dev [batch][n_frames][3][n_heads][head_dim] is the output of ONE fused q/k/v projection GEMM (the caller's);
 * out_dev [batch][n_frames][n_heads * head_dim] is the layout the output projection consumes.  head_dim: 64 or 96.
 * emb_rel_k_dev / emb_rel_v_dev: [21][head_dim] relative-position embeddings shared by the heads (both or neither):
 *   score[i][j] += scale * q_i . emb_rel_k[j - i + 10],  out_i += sum_r p[i][i + r - 10] emb_rel_v[r],  |j - i| <= 10.
 * fp32 throughout (matrix cores in exact-fp32 mode); exp is evaluated as 2^(x log2 e) on the hardware exp unit.
 * head_dim 64 without relative terms (HuBERT) runs both GEMMs on the bf16 matrix cores instead, every fp32 operand split exactly into
 * three bf16 (six products, fp32 accumulate: fp32-level results, max abs error vs float64 ~4e-6 at 1599 frames); its 8-wave workgroups
 * request the CU's whole LDS like every kernel of this library that issues bf16 matrix instructions.
 * workspace_dev: rvc_attention_workspace_bytes() bytes (partial results when the keys are split; the K / V fragment slab of the bf16 form).
 * The size query accepts exactly what the forward accepts: batch > 0, n_heads > 0, n_frames >= 0, head_dim 64 or 96. */
int rvc_attention_workspace_bytes(int batch, int64_t n_frames, int n_heads, int head_dim, size_t *bytes);
int rvc_attention_qkv_f32(const float *qkv_dev, const float *emb_rel_k_dev, const float *emb_rel_v_dev, float *out_dev,
                          int batch, int64_t n_frames, int n_heads, int head_dim, float scale, void *workspace_dev,
                          size_t workspace_bytes, void *stream);

/* ---- K8: conv epilogue of the RMVPE U-Net ------------------------------------------------------ *
 * out = relu(x + bias[c]) + res, the tail of `ConvBlockRes.forward` (rvc/lib/predictors/RMVPE.py:25-64: conv ->
 * BatchNorm (eval, folded by the caller: bias = folded shift) -> ReLU, and after the second conv `+ shortcut(x)` / `+ x`).
 * x_dev/out_dev/res_dev [batch][channels][inner] (inner = H*W, a multiple of 4); bias_dev [channels] or NULL;
 * res_dev NULL for no residual; relu 0/1; out_dev may alias x_dev. */
int rvc_bias_relu_add_f32(const float *x_dev, const float *bias_dev, const float *res_dev, float *out_dev, int batch,
                          int channels, int64_t inner, int relu, void *stream);

/* out = gelu(GroupNorm(num_groups = channels)(x)) -- the normalisation + activation behind the first feature-extractor conv of
 * `transformers`' HubertModel (pipeline.py:450; HubertGroupNormConvLayer: Conv1d -> GroupNorm(512, 512) -> GELU): per (batch,
 * channel) row mean / variance over `length` (float64 accumulation, biased variance, eps inside the square root), affine
 * gamma / beta [channels] (NULL: 1 / 0), exact erf GELU.  x_dev / out_dev [batch][channels][length]; out_dev may alias x_dev. */
int rvc_rownorm_gelu_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev, float *out_dev, int batch, int channels,
                         int64_t length, float eps, void *stream);

/* WaveNet gate of the flow (rvc/lib/algorithm/commons.py:142-157, modules.py:93-97): acts = tanh(x[:H]) * sigmoid(x[H:]).
 * x_dev [batch][2*hidden][length] (the conditioning is already inside: the producing conv adds it as its bias),
 * out_dev [batch][hidden][length]. */
int rvc_gate_tanh_sigmoid_f32(const float *x_dev, float *out_dev, int batch, int hidden, int64_t length, void *stream);

/* Scheduling hint: how many utterances the caller keeps in flight on separate streams (default 1).  With more than one,
 * kernels stop shrinking their tiles to balance a launch across the CUs on its own -- the other streams fill the idle
 * block slots, and the larger tiles re-read their weights from L2 half as often.  No effect on results.
 * This one is the process-wide default (used by rvc_conv1d_forward and by decoder handles without a hint of their own);
 * rvc_decoder_set_concurrency_hint below sets it per handle, so that two converters in one process do not share it. */
int rvc_set_concurrency_hint(int utterances_in_flight);

/* ---- K2/K3: vocoder ("dec" of Synthesizer) ---------------------------------------------------- *
 * Replaces `self.dec(z * x_mask, nsff0, g=g)` at rvc/lib/algorithm/synthesizers.py:254-258, i.e.
 *   RVC_DEC_NSF    HiFiGANNSFGenerator.forward  rvc/lib/algorithm/generators/hifigan_nsf.py:173-207
 *   RVC_DEC_MRF    HiFiGANMRFGenerator.forward  rvc/lib/algorithm/generators/hifigan_mrf.py:339-366
 *   RVC_DEC_REFINE RefineGANGenerator.forward   rvc/lib/algorithm/generators/refinegan.py:368-405
 * Weights are handed over once, by state-dict name with weight-norm already folded (w = g*v/||v||),
 * fp32, host memory; the library repacks them into its own HBM layouts.
 */
typedef struct rvc_decoder rvc_decoder;

enum { RVC_DEC_NSF = 0, RVC_DEC_MRF = 1, RVC_DEC_REFINE = 2 };

typedef struct rvc_decoder_config {
    int kind;                 /* RVC_DEC_* */
    int sample_rate;          /* 32000 / 40000 / 48000 */
    int in_channels;          /* inter_channels, 192 */
    int upsample_initial_channel; /* 512 */
    int gin_channels;         /* 256 */
    int n_ups;                /* number of upsample stages, <= 8 */
    int upsample_rates[8];
    int upsample_kernel_sizes[8];
    int n_res_kernels;        /* 3 */
    int res_kernel_sizes[4];  /* 3,7,11 */
    int res_dilations[4];     /* 1,3,5 (same for every kernel size) */
    int n_res_dilations;      /* 3 */
    int weight_storage;       /* 0: fp32.  1: the ResBlock / MRF-layer conv weights (98 % of the vocoder's weight bytes) are kept
                                 in HBM as bf16 and widened to fp32 inside the conv kernel (BASELINE cfg 4: "bf16 weights ...
                                 alt ResBlock kernel path"); the arithmetic stays fp32.  NSF / MRF only.
                                 This is a NUMERICS mode (bf16-VALUED taps), not a footprint reduction: the layers that run on
                                 the bf16 matrix cores keep fragment slabs of those taps (three bf16 per transformed tap: 126 B
                                 per (c_out, c_in) pair at 11 taps against 44 B of fp32 taps), so the handle holds MORE weight
                                 bytes than with fp32 storage. */
} rvc_decoder_config;

int rvc_decoder_create(const rvc_decoder_config *cfg, rvc_decoder **out);
/* name: state-dict key without the "dec." prefix, e.g. "ups.0.weight", "resblocks.3.convs1.1.bias". */
int rvc_decoder_set_tensor(rvc_decoder *dec, const char *name, const float *data_host,
                           const int64_t *shape, int ndim);
/* call after the last set_tensor: checks that every tensor arrived, builds derived tables */
int rvc_decoder_finalize(rvc_decoder *dec);
int rvc_decoder_destroy(rvc_decoder *dec);

/* samples produced per input frame (prod(upsample_rates)) */
int rvc_decoder_upp(const rvc_decoder *dec);
int rvc_decoder_workspace_bytes(const rvc_decoder *dec, int batch, int64_t n_frames, size_t *bytes);

/* Explicit noise inputs, in the order and shapes the reference draws them (SURVEY §7 hard part 1):
 *   NSF:    src_randn_dev [batch, T*upp]                         (hifigan.py:223; the rand of :189 is zeroed)
 *   MRF:    src_rand_dev [batch, 9] (hifigan_mrf.py:143), src_randn_dev [batch, T*upp, 9] (hifigan_mrf.py:172)
 *   REFINE: src_rand_dev [batch, 1], src_randn_dev [batch, T*upp, 1], adain_randn_dev = the 24 AdaIN draws
 *           concatenated in call order (refinegan.py:111)
 * Unused pointers may be NULL. */
typedef struct rvc_decoder_noise {
    const float *src_rand_dev;
    const float *src_randn_dev;
    const float *adain_randn_dev;
} rvc_decoder_noise;

/* z_dev [batch, in_channels, T] (already multiplied by x_mask), f0_dev [batch, T], g_dev [batch, gin_channels],
 * out_dev [batch, T*upp] = tanh(conv_post(...)). */
int rvc_decoder_forward(rvc_decoder *dec, const float *z_dev, const float *f0_dev, const float *g_dev,
                        const rvc_decoder_noise *noise, int batch, int64_t n_frames, float *out_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream);

/* The pipeline pads every segment with x_pad seconds of reflected audio, runs the model on the padded clip and trims the pad off the
 * waveform again (rvc/infer/pipeline.py: `audio_pad = np.pad(audio, (self.t_pad, self.t_pad), mode="reflect")` ...
 * `[self.t_pad_tgt : -self.t_pad_tgt]`).  After the source module the NSF / MRF vocoder (hifigan_nsf.py:173-207) is a stack of
 * convolutions with a short receptive field, so the samples that are kept do not depend on most of the padded frames.
 *
 * rvc_decoder_window_margin: *frames = the number of input frames on EACH side of an output frame that it can depend on through z or
 * the source samples, derived layer by layer from the configuration (conv_pre, each transposed conv and its noise conv, the widest
 * ResBlock branch per stage, conv_post; rounded up to whole frames): 10 for 48 k (rates 12,10,2,2), 11 for 40 k and 32 k.  A pure
 * host function: no handle, no device.  RefineGAN (interpolated source, a down path) is not covered: *frames = -1.
 *
 * rvc_decoder_forward_window: rvc_decoder_forward's samples [keep_lo * upp, keep_hi * upp) -- equal up to fp32 rounding -- into
 * out_dev [batch, (keep_hi - keep_lo) * upp], from the SAME full-length inputs (z_dev [batch, in_channels, n_frames], f0_dev, the noise
 * tensors at their full lengths).  The sine phase is a running sum over every earlier frame, so the phase carry still comes from
 * the whole contour; the source samples and every conv only run over frames [max(0, keep_lo - margin), min(n_frames, keep_hi + margin)).
 * 0 <= keep_lo < keep_hi <= n_frames; (0, n_frames) makes exactly rvc_decoder_forward's launches.  The workspace of
 * rvc_decoder_workspace_bytes(dec, batch, n_frames) is sufficient.  An error for a RefineGAN handle and while a debug tap is set
 * (rvc_decoder_set_tap): use rvc_decoder_forward for those. */
int rvc_decoder_window_margin(const rvc_decoder_config *cfg, int *frames);
int rvc_decoder_forward_window(rvc_decoder *dec, const float *z_dev, const float *f0_dev, const float *g_dev,
                               const rvc_decoder_noise *noise, int batch, int64_t n_frames, int64_t keep_lo, int64_t keep_hi,
                               float *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Per-handle scheduling hint (see rvc_set_concurrency_hint); 0 = follow the process-wide default.  May be called while
 * forwards of this handle are running on other threads: it only affects forwards that start afterwards. */
int rvc_decoder_set_concurrency_hint(rvc_decoder *dec, int utterances_in_flight);

/* The ResBlock branches of a stage (`xs += self.resblocks[i * self.num_kernels + j](x)`, hifigan_nsf.py:195-203 /
 * hifigan_mrf.py:353-361) depend on the stage's input only.  With side_streams > 0 (or -1: one per branch after the first) a
 * SHORT stage (batch x channels x samples <= 3 rounds of the 256 CUs' 128 x 256 blocks; stage 0 of a 30 s clip at 48 k is
 * 1.17 rounds, so every launch leaves most of the chip idle through its second round) runs its branches side by side on
 * streams owned by the handle, each branch's last launch adding into the running sum after its predecessor's; the caller's
 * stream waits for the last one, so the call is ordered on `stream` exactly as before and results are bit-identical.
 * Default 0 (every launch on the caller's stream): one forward on an idle device gets 5 % (30 s) to 27 % (3 s) shorter, a
 * pipeline that already keeps two utterances in flight does not, and traced kernel durations then contain the time the branches
 * share the chip (profiles/r05_branch_streams.txt).
 * Changes the workspace size (every stream owns two ping-pong buffers): query rvc_decoder_workspace_bytes afterwards. */
int rvc_decoder_set_branch_parallel(rvc_decoder *dec, int side_streams);

/* The arithmetic of the square 128- / 256-channel ResBlock / MRF-layer convs of this handle.  Call between rvc_decoder_create and
 * rvc_decoder_finalize (refused afterwards: the tap slabs are packed at finalize).
 *   0 (default): exact -- fp32 operands as exact bf16 triples, six matrix products per multiply-add (K3y / K3f); nothing changes.
 *   1: error-corrected fp16 pairs (K3h, rvc_conv1d_f16x2_forward below): three matrix products per multiply-add, the fp32 result
 *      to ~2^-22 relative per product instead of exactly; a layer whose taps the pair cannot hold (|w| > 65504, non-finite) and
 *      every layer K3h is not the faster kernel for stay on the exact path.  Upsamplers, non-square convs and the 32- / 64-channel
 *      stages are untouched.
 * Refused for any other mode and on a handle created with weight_storage = 1 (its taps already cost three products). */
int rvc_decoder_set_arithmetic(rvc_decoder *dec, int mode);

/* Debug hook for the parity tests: after stage `stage` of the next forward calls, copy that stage's output
 * ([batch][C_stage][L_stage], the mean of the three ResBlocks) to tap_dev; stage -1 = har_source [batch][T*upp].
 * tap_dev = NULL switches it off. */
int rvc_decoder_set_tap(rvc_decoder *dec, int stage, float *tap_dev);

/* ---- generic fp32 conv1d (the decoder's work-horse, exported for unit tests) -------------------- *
 * y[b,co,t] = out_scale * ( bias[co] + sum_{ci,k} w[co,ci,k] * act(x[b,ci,t + (k - (K-1)/2)*dil]) + res[b,co,t] + acc[b,co,t] )
 * with act = leaky_relu(slope_in) (slope_in = 1 -> identity), zero padding, K odd.
 * w_packed_dev is the [K][C_in][C_out] repack produced by rvc_conv1d_pack_weight.
 * res_dev / acc_dev / bias_dev may be NULL.  C_in % 8 == 0, C_out % 32 == 0. */
int rvc_conv1d_pack_weight(const float *w_host, int c_out, int c_in, int k, float *w_packed_dev, void *stream);
int rvc_conv1d_forward(const float *x_dev, const float *w_packed_dev, const float *bias_dev,
                       const float *res_dev, const float *acc_dev, float *y_dev,
                       int batch, int c_in, int c_out, int64_t length, int k, int dilation,
                       float slope_in, float out_scale, void *stream);

/* ---- multi-GPU: index replication ---------------------------------------------------------------- *
 * The path shards by utterance, one process per GPU (the reference's own multi-GPU precedent is the file striding of
 * rvc/train/extract/extract.py:141-152, 198); its only exchange is making `big_npy` (pipeline.py:556) resident on
 * every GPU, which replaces the per-call `faiss.read_index` of pipeline.py:555 on each worker.  These entries wrap RCCL
 * (bound at run time, so a single-GPU process never loads it):
 *   rank 0:      rvc_comm_unique_id(id)  ->  the host side hands the 128 bytes to every rank (TCP store, file, ...)
 *   every rank:  rvc_comm_create(id, n_ranks, rank, &comm)      collective, on the rank's own current device
 *                rvc_index_broadcast(comm, buf, bytes, root, stream)   ONE ncclBroadcast of raw bytes, in place
 *                rvc_checksum64(buf, bytes, out2, stream)       replica == root's?  (compare the two words across ranks)
 *                rvc_comm_destroy(comm)
 * A communicator is bound to the device current at creation; calls on one communicator must not be concurrent. */
typedef struct rvc_comm rvc_comm;
#define RVC_COMM_ID_BYTES 128
int rvc_comm_unique_id(unsigned char *id_host /* [RVC_COMM_ID_BYTES] */);
int rvc_comm_create(const unsigned char *id_host, int n_ranks, int rank, rvc_comm **out);
int rvc_comm_destroy(rvc_comm *comm);
/* n_ranks as RCCL reports it (ncclCommCount), this rank, RCCL's version code, and which librccl was bound; comm may be
 * NULL (library facts only) and any output pointer may be NULL. */
int rvc_comm_info(const rvc_comm *comm, int *n_ranks, int *rank, int *rccl_version, char *library_path,
                  size_t library_path_bytes);
int rvc_index_broadcast(rvc_comm *comm, void *buf_dev, size_t bytes, int root, void *stream);
/* out2_dev[0] = sum of the buffer's little-endian 32-bit words, out2_dev[1] = sum of (i + 1) * word_i, both mod 2^64
 * (a trailing 1-3 bytes are zero-extended into a last word).  Computed in HBM: the index never crosses PCIe. */
int rvc_checksum64(const void *buf_dev, size_t bytes, uint64_t *out2_dev, void *stream);

/* ---- K10: conv2d 3x3 (padding 1) / 1x1, stride 1, of RMVPE's U-Net blocks (RMVPE.py:13-287) ---------------------------- *
 * y = act(conv(x) + bias) + res  with act = ReLU when relu != 0 -- ConvBlockRes with its BatchNorms folded into the weights
 * (eval mode): conv -> BN -> ReLU, then the skip path added after the activation.  fp32 on the matrix cores, k-ordered
 * accumulation; deep levels split K over several workgroups and sum the partials in a fixed order (bit-reproducible).
 * x [batch][C_in][H][W], y / res [batch][C_out][H][W]; C_in a multiple of 8, W a power of two in 4..128.
 * w_packed: rvc_conv2d_packed_floats() floats filled by rvc_conv2d_pack_weight from torch's [C_out][C_in][kh][kw].
 * workspace: rvc_conv2d_workspace_bytes() bytes (0 for shapes that do not split), caller-owned, reusable across calls on one
 * stream. */
int rvc_conv2d_packed_floats(int c_out, int c_in, int kh, int kw, size_t *out);
int rvc_conv2d_pack_weight(const float *w_host, int c_out, int c_in, int kh, int kw, float *w_dev, void *stream);
int rvc_conv2d_workspace_bytes(int batch, int c_in, int c_out, int height, int width, int kh, int kw, size_t *out);
int rvc_conv2d_forward(const float *x_dev, const float *w_packed_dev, const float *bias_dev, const float *res_dev,
                       float *y_dev, int batch, int c_in, int c_out, int height, int width, int kh, int kw, int relu,
                       void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- K10b: the same 3x3 conv on the bf16 matrix cores, every fp32 operand split exactly into three bf16 (six products of order
 * <= 2^-16, fp32 accumulate: fp32-level results, not bit-equal to K10's k-ordered fp32 chain).  Replaces the same ConvBlockRes convs
 * (RMVPE.py:13-64) for the shapes rvc_conv2d_bf16x3_supported() returns 1 for: C_in a multiple of 16, C_out <= 64 or a multiple of
 * 128, W a power of two in 4..128 (and <= 256 / 128 / 64 pixels for <= 32 / <= 64 / more output channels); 3x3 only.
 * u: rvc_conv2d_bf16x3_weight_bytes() bytes filled by rvc_conv2d_bf16x3_pack_weight from torch's HOST [C_out][C_in][3][3].
 * workspace: rvc_conv2d_bf16x3_workspace_bytes() bytes (the K-split deep levels; partials summed in a fixed order). */
int rvc_conv2d_bf16x3_supported(int c_in, int c_out, int height, int width);
int rvc_conv2d_bf16x3_weight_bytes(int c_out, int c_in, int kh, int kw, size_t *bytes);
int rvc_conv2d_bf16x3_pack_weight(const float *w_host, int c_out, int c_in, int kh, int kw, void *u_dev, void *stream);
int rvc_conv2d_bf16x3_workspace_bytes(int batch, int c_in, int c_out, int height, int width, size_t *out);
int rvc_conv2d_bf16x3_forward(const float *x_dev, const void *u_dev, const float *bias_dev, const float *res_dev, float *y_dev,
                              int batch, int c_in, int c_out, int height, int width, int relu, void *workspace_dev,
                              size_t workspace_bytes, void *stream);

/* ---- the same conv in its fast form (unit-test entry of what the decoder uses for its ResBlock layers) ---------------- *
 * Winograd / Toom-Cook over groups of taps -- F(4,3) for 3 taps, F(4,4) for 7 and 11: identical mathematics, 1.5 / 3.5 / 5.25
 * multiply-adds per output instead of 3 / 7 / 11; fp32 throughout, one layer agrees with float64 to ~5e-7 relative RMS (direct
 * fp32 form: ~2e-7).
 * K in {3, 7, 11}, dilation 1..5, C_in a multiple of 8, C_out a multiple of 32, leaky slope in [0, 1], C_in * L < 2^29.
 * u_dev: 3 G * C_in * C_out floats laid out [3 G][C_in / 2][C_out][2] (the taps, zero-padded to a multiple of three, input
 * channel pairs interleaved) filled by rvc_conv1d_wino_pack_weight from the [C_out][C_in][K] host weights. */
int rvc_conv1d_wino_pack_weight(const float *w_host, int c_out, int c_in, int k, float *u_dev, void *stream);
int rvc_conv1d_wino_forward(const float *x_dev, const float *u_dev, const float *bias_dev, const float *res_dev,
                            const float *acc_dev, float *y_dev, int batch, int c_in, int c_out, int64_t length, int k,
                            int dilation, float slope_in, float out_scale, void *stream);

/* ---- ... and on the bf16 matrix cores with fp32-exact operands (what the decoder uses for its 7- / 11-tap layers at
 * >= 64 channels and its 3-tap layers at c_out % 128 == 0) ------------------------------------------------------------------------------------------------------- *
 * The same F(4,4) form with every fp32 operand split exactly into three bf16 numbers (8 + 8 + 8 significand bits) and the six
 * products of order <= 2^-16 formed by v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the dropped terms are below 2^-23
 * of a product.  One layer agrees with float64 as closely as the fp32 Winograd form does.
 * K in {7, 11}, dilation 1..5, C_in a multiple of 16, C_out a multiple of 64, leaky slope in [0, 1], C_in * L < 2^29;
 * K = 3 (F(4,3): six points, one tap group) with C_out a multiple of 128.
 * u_dev: rvc_conv1d_winobf_weight_bytes() bytes -- the tap transform, evaluated in float64 on the host, rounded to fp32, split
 * into three bf16 and laid out as matrix-instruction fragments by rvc_conv1d_winobf_pack_weight, in the order the kernel that will
 * read them consumes them: C_out % 128 == 0 runs csrc/winobf2.hip (one transform point per wave, 128-channel x 64-column blocks),
 * other C_out csrc/winobf.hip (64 x 128 blocks) -- a slab is only valid for the (C_out, C_in, K) it was packed for.
 * Both kernels request the CU's whole LDS (like the bf16x3 GEMM below): no other workgroup ever shares their CU. */
int rvc_conv1d_winobf_weight_bytes(int c_out, int c_in, int k, size_t *bytes);
int rvc_conv1d_winobf_pack_weight(const float *w_host, int c_out, int c_in, int k, void *u_dev, void *stream);
int rvc_conv1d_winobf_forward(const float *x_dev, const void *u_dev, const float *bias_dev, const float *res_dev,
                              const float *acc_dev, float *y_dev, int batch, int c_in, int c_out, int64_t length, int k,
                              int dilation, float slope_in, float out_scale, void *stream);

/* ---- K3f: one ResBlock (dilated conv -> conv) pair of the 32- / 64-channel stages in ONE launch ------------------------------- *
 * Replaces, per dilation d of ResBlock.forward (rvc/lib/algorithm/residuals.py:75-86; the MRF layer of
 * rvc/lib/algorithm/generators/hifigan_mrf.py has the same body):
 *     xt = leaky_relu(x, slope); xt = conv1_d(xt); xt = leaky_relu(xt, slope); xt = conv2(xt); x = xt + x
 * plus the generator's running sum over its parallel ResBlocks and the final 1 / n (hifigan_nsf.py:196-205):
 *     y = out_scale * (conv2(leaky(conv1_d(leaky(x)) + b1)) + b2 + x [+ acc])
 * Direct form on the bf16 matrix cores, every fp32 operand (taps, activations, the intermediate) split exactly into three
 * bf16 and the six products of order <= 2^-16 accumulated in fp32 (csrc/resblock_bf.hip); the intermediate stays in LDS.
 * C in {32, 64} with K in {3, 7, 11}, or C = 128 with K in {3, 7}; dilation 1..5 (conv2's is 1), leaky slope in [0, 1],
 * C * L * 4 < 2^31; x and y must not alias.
 * u_dev: rvc_resblock_bf16x3_weight_bytes() bytes filled by rvc_resblock_bf16x3_pack_weight from the two [C][C][K] host weights.
 * Persistent: one 8-wave workgroup per CU that requests the CU's whole LDS (the rule for every bf16 matrix kernel here). */
int rvc_resblock_bf16x3_weight_bytes(int c, int k, size_t *bytes);
int rvc_resblock_bf16x3_pack_weight(const float *w1_host, const float *w2_host, int c, int k, void *u_dev, void *stream);
int rvc_resblock_bf16x3_forward(const float *x_dev, const void *u_dev, const float *b1_dev, const float *b2_dev,
                                const float *acc_dev, float *y_dev, int batch, int c, int64_t length, int k, int dilation,
                                float slope, float out_scale, void *stream);
/* The same pair with bf16-VALUED taps -- the weights of a handle created with weight_storage = 1 (BASELINE cfg 4: "MRF-HiFi-GAN,
 * bf16 weights, alt ResBlock kernel path"; MRFLayer.forward, rvc/lib/algorithm/generators/hifigan_mrf.py:13-83, is the body above).
 * A bf16-valued tap IS the first term of its split (w = w_0 exactly), so w x = w_0 x_0 + w_0 x_1 + w_0 x_2 is the whole product:
 * THREE matrix products per multiply-add instead of six, one 1 KiB tap fragment per (tap, 16 input channels, 32 output channels)
 * instead of three; activations and the intermediate keep their exact three-way split, so the result is the fp32 result of the
 * pair on the rounded taps to the same ~2^-23 as the six-product form.  pack_weight ROUNDS the fp32 taps it is given to bf16
 * (round to nearest even, what weight_storage = 1 and torch's .bfloat16() do).  Shapes and rules as above. */
int rvc_resblock_bf16w_weight_bytes(int c, int k, size_t *bytes);
int rvc_resblock_bf16w_pack_weight(const float *w1_host, const float *w2_host, int c, int k, void *u_dev, void *stream);
int rvc_resblock_bf16w_forward(const float *x_dev, const void *u_dev, const float *b1_dev, const float *b2_dev,
                               const float *acc_dev, float *y_dev, int batch, int c, int64_t length, int k, int dilation,
                               float slope, float out_scale, void *stream);
/* ---- K3d: ONE square conv with bf16-VALUED taps, direct form, for the layers the fused pair cannot hold in LDS ------------------ *
 * Replaces one conv of the same ResBlock / MRFLayer body (rvc/lib/algorithm/residuals.py:75-86, hifigan_mrf.py:13-83) at
 * C = 256 (K = 3, 7, 11) and C = 128 (K = 11; K = 3 / 7 accepted too) in a decoder handle created with weight_storage = 1:
 *     y = out_scale * (conv_d(leaky(x, slope)) + bias [+ res] [+ acc])
 * One-term taps (rounded to bf16 by pack_weight, round to nearest even) against activations split exactly into three bf16: three
 * matrix products per multiply-add, no Winograd transform; persistent 8-wave workgroups walking (64 columns x all channels) tiles
 * (csrc/convbf1.hip).  dilation 1..5, C * L * 4 < 2^31; y must not alias x (res and acc may alias y). */
int rvc_conv1d_bf16w_weight_bytes(int c, int k, size_t *bytes);
int rvc_conv1d_bf16w_pack_weight(const float *w_host, int c, int k, void *u_dev, void *stream);
int rvc_conv1d_bf16w_forward(const float *x_dev, const void *u_dev, const float *bias_dev, const float *res_dev,
                             const float *acc_dev, float *y_dev, int batch, int c, int64_t length, int k, int dilation,
                             float slope_in, float out_scale, void *stream);
/* ---- K3h: ONE square conv with fp32 taps on error-corrected fp16 PAIRS (the opt-in fast-fp32 vocoder mode) --------------------- *
 * Replaces one conv of the ResBlock / MRFLayer body (rvc/lib/algorithm/residuals.py:75-86, hifigan_mrf.py:13-83) at C = 128 / 256,
 * K = 3, 7, 11 in a decoder handle with rvc_decoder_set_arithmetic(dec, 1):
 *     y = out_scale * (conv_d(leaky(x, slope)) + bias [+ res] [+ acc])
 * Ootomo & Yokota's split: v -> (hi = fp16(v), lo = fp16((v - hi) 2^11)), w x ~= w_hi x_hi + 2^-11 (w_hi x_lo + w_lo x_hi): three fp16
 * matrix products per multiply-add, two fp32 accumulators per tile (the cross terms share the 2^11 scale) combined before the bias;
 * the dropped w_lo x_lo term is ~2^-22 of the product.  Measured relative RMS against float64: 1.5e-7 .. 3.5e-7 at activation
 * amplitudes 1e-3 .. 1e3, the level of F.conv1d in fp32 (profiles/fastfp32_conv_shapes.txt).  fp16 subnormals contribute (the
 * conversions and the matrix instruction keep them); below |x| ~ 6e-5 the hi part itself is subnormal and the error grows.  Activations are clamped to +-65504 after
 * the leaky ReLU (finite, less accurate results beyond; a NaN activation counts as -65504); pack_weight REFUSES taps with |w| > 65504
 * or a non-finite value.  Bit-reproducible from launch to launch.
 * u_dev: rvc_conv1d_f16x2_weight_bytes() = (C / 16) K (C / 32) 2048 bytes: per (64-channel chunk, tap, 16 input channels, 32 output
 * channels) one 1 KiB fragment of w_hi and one of w_lo 2^11.  Persistent 8-wave workgroups that own their CU (csrc/convbf1.hip).
 * dilation 1..5, leaky slope in [0, 1], C * L * 4 < 2^31; y must not alias x (res and acc may alias y). */
int rvc_conv1d_f16x2_weight_bytes(int c, int k, size_t *bytes);
int rvc_conv1d_f16x2_pack_weight(const float *w_host, int c, int k, void *u_dev, void *stream);
int rvc_conv1d_f16x2_forward(const float *x_dev, const void *u_dev, const float *bias_dev, const float *res_dev,
                             const float *acc_dev, float *y_dev, int batch, int c, int64_t length, int k, int dilation,
                             float slope_in, float out_scale, void *stream);
/* ---- K3u: the vocoder's upsampling step on the bf16 matrix cores (exact bf16x3 operands) -------------------------------------- *
 * Replaces, per stage i of HiFiGANNSFGenerator.forward / HiFiGANMRFGenerator.forward (rvc/lib/algorithm/generators/hifigan_nsf.py:184-193,
 * hifigan_mrf.py:349-357):   x = leaky_relu(x, slope); x = ups[i](x); x = x + noise_convs[i](har_source)
 *     y[co][t] = bias[co] + ConvTranspose1d(leaky(x))[co][t] + sum_k noise_w[co][k] har[t nc_stride + k - nc_pad]
 * ConvTranspose1d(c_in, c_out, ksize, stride = rate, padding = pad) with ksize <= 2 rate in polyphase form (a GEMM with rows
 * (channel, phase), two taps); the noise conv (one input channel, nc_k taps, stride nc_stride; nc_k = 0: none) enters as
 * (rate - 1) nc_stride + nc_k < 64 extra GEMM rows read straight from har_source [batch][har_len], plus a row of ones whose taps are the
 * bias (so pack_weight takes it: ups bias + noise-conv bias [c_out]); without a noise conv bias_dev is added on the way out.
 * Accepted shapes (weight_bytes and pack_weight refuse every other): rate in {2, 8, 10, 12}, and rate * c_out >= 128 for 8, 10 and 12;
 * c_in a positive multiple of 64; c_out >= 1; rate <= ksize <= 2 rate; nc_k >= 0, and nc_stride >= 1 with
 * (rate - 1) nc_stride + nc_k <= 63 when nc_k > 0.  length_out = (length_in - 1) rate - 2 pad + ksize.  Every fp32 operand split exactly
 * into three bf16, six products, fp32 accumulate (csrc/upsbf.hip); persistent whole-CU workgroups. */
int rvc_upsample_bf16x3_weight_bytes(int c_in, int c_out, int rate, int ksize, int nc_k, int nc_stride, size_t *bytes);
int rvc_upsample_bf16x3_pack_weight(const float *up_w_host, const float *noise_w_host, const float *bias_host, int c_in, int c_out,
                                    int rate, int ksize, int nc_k, int nc_stride, void *u_dev, void *stream);
int rvc_upsample_bf16x3_forward(const float *x_dev, const float *har_dev, int64_t har_len, const void *u_dev, const float *bias_dev,
                                float *y_dev, int batch, int c_in, int c_out, int64_t length_in, int rate, int ksize, int pad,
                                int nc_k, int nc_stride, int nc_pad, float slope_in, void *stream);
/* Process-wide runtime switch for K3f inside rvc_decoder_finalize (default 1): decoder handles finalized while it is 0 keep the
 * (conv, conv) pairs of their narrow stages on the unfused kernels (csrc/resblock.hip, winobf.hip, wino.hip) -- the fall-back an
 * operator reaches for without rebuilding the library.  The entry points above are not affected. */
int rvc_resblock_bf16x3_set_enabled(int enabled);

/* ---- K11: fp32 GEMM / strided conv1d on the bf16 matrix cores with fp32-exact operands ------------------------------------ *
 * Replaces the fp32 library GEMMs behind `transformers`' HubertModel at rvc/infer/pipeline.py:450: the attention / FFN
 * projections (nn.Linear: y = act(x W^T + b) + res, x [n_rows][in] row-major) and the stride-2 convolutions of the feature
 * extractor (nn.Conv1d without padding + GELU, x [batch][C_in][L] channel-major).  Every fp32 operand is split exactly into three
 * bf16 numbers and the six products of order <= 2^-16 are accumulated in fp32 (csrc/gemmbf.hip).
 * The kernel launches one 8-wave workgroup per CU and requests the CU's whole LDS: a workgroup issuing bf16 matrix instructions
 * that shares a CU with a workgroup of the fp32 Winograd kernel behind rvc_decoder_forward corrupts THAT kernel's results
 * (measured on MI355X, profiles/r03_mfma_cohabitation.txt), so this one never shares; results agree with float64 as
 * closely as an fp32 GEMM does.  act: 0 none, 1 GELU (erf form, what torch.nn.functional.gelu computes).
 * Weights: rvc_gemm_bf16x3_weight_bytes() bytes filled by rvc_gemm_bf16x3_pack_weight from the [out][in] (linear, conv_taps = 1) or
 * [C_out][C_in][taps] (conv, conv_taps = taps, k_total = taps * C_in) host tensor.  out / C_out a multiple of 128, in / C_in of 16. * rvc_conv1d_bf16x3 also takes c_in = 1 with k <= 16, no padding, batch 1 (HuBERT's first layer: Conv1d(1, 512, 10, stride 5)); the
 * kernel reads nothing beyond x[l_in - 1].  rvc_gemm_bf16x3_weight_bytes / _pack_weight pad such a weight to one k16 step.
 * rvc_conv1d_bf16x3 writes l_out = (l_in + 2 padding - k) / stride + 1 columns per channel, and NOTHING when l_in + 2 padding < k.
 */
int rvc_gemm_bf16x3_weight_bytes(int m, int k_total, size_t *bytes);
int rvc_gemm_bf16x3_pack_weight(const float *w_host, int m, int k_total, int conv_taps, void *a_dev, void *stream);
int rvc_linear_bf16x3(const float *x_dev, const void *a_dev, const float *bias_dev, const float *res_dev, float *y_dev,
                      int64_t n_rows, int in_features, int out_features, int act, void *stream);
int rvc_conv1d_bf16x3(const float *x_dev, const void *a_dev, const float *bias_dev, float *y_dev, int batch, int c_in,
                      int c_out, int64_t l_in, int k, int stride, int padding, int act, void *stream);

/* ---- K12: the GEMMs of HuBERT's transformer layers with BOTH operands pre-split ------------------------------------------------ *
 * Replaces the nn.Linear / LayerNorm / GELU modules of `transformers`' HubertEncoderLayer (q/k/v, attention output, feed-forward)
 * behind rvc/infer/pipeline.py:450.  Same exact bf16x3 arithmetic as K11; the activations arrive as three bf16 planes
 * [split][n_rows_padded][features] (their sum is the fp32 value exactly), so the kernel's main loop is LDS-DMA + matrix
 * instructions only (csrc/linbf.hip).  Rows n_rows .. n_rows_padded - 1 of a plane are never read into a stored result and
 * never written: they need no initialisation.
 * rvc_split_rows_bf16x3: fp32 [n_rows][k] -> planes.
 * rvc_linear_bf16x3_presplit: a_dev = rvc_gemm_bf16x3_pack_weight's slab of the [out][in] weight.  mode 0: y_dev [n_rows][out]
 *   = x W^T + bias; mode 1: ys_dev planes [3][n_rows_padded][out] of gelu(x W^T + bias) (erf form); mode 2: y_dev
 *   [k_parts][n_rows][out] partial sums over k_parts equal slices of in_features (no bias) -- the grid filler for the 768-wide
 *   outputs; mode 3: y_dev [n_rows][out] = gelu(x W^T + bias).  in_features a multiple of 32 (and of 32 k_parts), n_rows_padded a
 *   multiple of 128.  One 8-wave workgroup per CU, whole LDS.
 * rvc_bias_residual_layernorm_bf16x3: y = LayerNorm(sum of the parts + bias + res) * gamma + beta over `features` (256, 768 or 1024),
 *   written as fp32 (y_dev, may be NULL) and as planes (ys_dev, may be NULL): HubertEncoderLayer's `hidden = layer_norm(hidden +
 *   dropout(attn))` / `final_layer_norm(hidden + feed_forward(hidden))` fused with the split-K reduction. */
int rvc_split_rows_bf16x3(const float *x_dev, void *xs_dev, int64_t n_rows, int64_t n_rows_padded, int k, void *stream);
int rvc_linear_bf16x3_presplit(const void *xs_dev, const void *a_dev, const float *bias_dev, float *y_dev, void *ys_dev,
                               int64_t n_rows, int64_t n_rows_padded, int in_features, int out_features, int mode, int k_parts,
                               void *stream);
int rvc_bias_residual_layernorm_bf16x3(const float *parts_dev, int n_parts, const float *bias_dev, const float *res_dev,
                                       const float *gamma_dev, const float *beta_dev, float eps, float *y_dev, void *ys_dev,
                                       int64_t n_rows, int64_t n_rows_padded, int features, void *stream);

/* ---- K12 / K13: HuBERT's feature extractor on time-major frames ---------------------------------------------------------------- *
 * Replaces `transformers`' HubertFeatureEncoder behind rvc/infer/pipeline.py:450 (conv_layers[0] = HubertGroupNormConvLayer:
 * Conv1d(1, 512, 10, stride 5, bias = False) -> GroupNorm(512, 512) -> GELU; conv_layers[1..6] = HubertNoLayerNormConvLayer:
 * Conv1d(512, 512, 3 or 2, stride 2, bias = False) -> GELU) for batch 1.  The activations travel TIME-MAJOR, [frame][channel], as
 * three bf16 planes [split][frames_padded][channels]: the window of a strided conv -- taps x channels values -- is then one
 * contiguous run starting stride x channels after its predecessor's, i.e. the conv IS K12's GEMM with a different row stride
 * and needs no im2col, no transposes and no fp32 copy of the 196 MB first-layer output.
 * rvc_hubert_conv0_frames_bf16x3 (csrc/hubert_front.hip): layer 0 from the 16 kHz samples; the conv is evaluated twice (float64
 *   statistics over the clip, then normalise + GELU + split) instead of being stored.  w_dev [channels][taps] fp32, taps = 10,
 *   channels a multiple of 64, at most 1024 (the size query refuses every other count, like the forward); workspace of
 *   rvc_hubert_conv0_workspace_bytes(channels) = channels * 136 bytes; ys_dev planes with n_frames_padded >= (n_samples - taps) /
 *   stride + 1 rows.
 * rvc_conv1d_frames_bf16x3 (csrc/linbf.hip): xs_dev planes [3][n_frames_in_padded][channels]; a_dev = rvc_gemm_bf16x3_pack_weight's
 *   slab of the [out][taps * channels] matrix W[o][k * channels + c] = conv.weight[o][c][k]; output frames (n_frames_in - taps) /
 *   stride + 1; modes 0 / 1 / 3 of rvc_linear_bf16x3_presplit (ys_dev planes [3][n_frames_out_padded][out_channels] or y_dev
 *   [frames_out][out_channels] fp32).  taps * channels a multiple of 32, stride * channels of 8, out_channels of 128,
 *   n_frames_out_padded of 128.  Rows of the last 128-frame tile beyond the input are read (inside the planes' allocation, or
 *   as zeros beyond it) but their results are not stored. */
int rvc_hubert_conv0_workspace_bytes(int channels, size_t *bytes);
int rvc_hubert_conv0_frames_bf16x3(const float *wav_dev, int64_t n_samples, const float *w_dev, int channels, int taps, int stride,
                                   const float *gamma_dev, const float *beta_dev, float eps, void *workspace_dev,
                                   size_t workspace_bytes, void *ys_dev, int64_t n_frames_padded, void *stream);
int rvc_conv1d_frames_bf16x3(const void *xs_dev, int64_t n_frames_in, int64_t n_frames_in_padded, int channels, int taps, int stride,
                             const void *a_dev, const float *bias_dev, float *y_dev, void *ys_dev, int64_t n_frames_out_padded,
                             int out_channels, int mode, void *stream);

/* ---- K14: HuBERT's convolutional position embedding -------------------------------------------------------------------------- *
 * Replaces `transformers`' HubertPositionalConvEmbedding.forward behind rvc/infer/pipeline.py:450 (weight-normed Conv1d(D, D, 128,
 * padding = 64, groups = 16) -> HubertSamePadLayer (drop the last frame) -> GELU) for one clip, time-major:
 *   y_dev[t][o] = gelu(bias[o] + sum_{k, c} W[o][c][k] * x_dev[t + k - padding][group(o) * CG + c]),  t = 0 .. n_frames - 1,
 * x_dev / y_dev [n_frames][d] fp32 (the caller adds the residual and applies encoder.layer_norm, e.g. with
 * rvc_bias_residual_layernorm_bf16x3 and n_parts = 1).  bf16 matrix cores, fp32 operands split exactly into three bf16
 * (csrc/posconv.hip): a block keeps its 128 + taps - 1 frames of one group's channels in LDS for the whole K loop, the weights
 * stream through by LDS-DMA.  d / groups = 48 or 64, taps <= 128.  a_dev: rvc_posconv_bf16x3_weight_bytes() bytes filled by
 * rvc_posconv_bf16x3_pack_weight from the host tensor conv.weight [d][d / groups][taps] (weight norm folded).
 * One 8-wave workgroup per CU, whole LDS. */
int rvc_posconv_bf16x3_weight_bytes(int d, int groups, int taps, size_t *bytes);
int rvc_posconv_bf16x3_pack_weight(const float *w_host, int d, int groups, int taps, void *a_dev, void *stream);
int rvc_posconv_gelu_bf16x3(const float *x_dev, const void *a_dev, const float *bias_dev, float *y_dev, int64_t n_frames, int d,
                            int groups, int taps, int padding, void *stream);

/* ---- K15: the FCPE pitch estimator between its GEMMs (csrc/fcpe.hip) ------------------------------------------------------------ *
 * The conv-only conformer of rvc/lib/predictors/torchfcpe (f0_method = "fcpe"): its dense layers run on K11, these four fp32
 * kernels are the rest.  Every entry checks its arguments before any device call and launches on `stream`.
 * rvc_glu_dwconv_silu_f32: nn.GLU(dim=1) -> DepthWiseConv1d(K, same padding) -> nn.SiLU of ConformerConvModule
 *   (model_conformer_naive.py:144-151) on time-major rows.  x_dev [n_rows][2C]: columns [0, C) the value, [C, 2C) the gate;
 *   u[t][c] = x[t][c] * sigmoid(x[t][C + c]);  v[t][c] = bias[c] + sum_j w[c][j] * u[t + j - K/2][c], u = 0 outside [0, n_rows);
 *   y_dev[t][c] = v * sigmoid(v).  w_dev [C][K], bias_dev [C], y_dev [n_rows][C].  C a multiple of 64, K odd, 1 <= K <= 31,
 *   n_rows >= 1, every pointer 16-byte aligned.
 * rvc_layernorm_rows_f32: nn.LayerNorm(F) per row of x_dev [n_rows][F] (model_conformer_naive.py:142, models.py:83): biased
 *   variance from centred squares around the row mean (two passes, float64), gamma_dev / beta_dev [F].  F a multiple of 64, <= 1024.
 * rvc_groupnorm_lrelu_f32: nn.GroupNorm(groups, C) -> nn.LeakyReLU(slope) of input_stack (models.py:66-71) on channel-major
 *   x_dev / y_dev [C][L]; biased variance over the (C / groups) x L elements of a group, taken as per-workgroup centred partial sums
 *   merged in float64.  workspace_dev: rvc_groupnorm_workspace_bytes(C, L, groups) bytes, 8-byte aligned.  groups divides C.
 * rvc_fcpe_decode_f32: sigmoid + latent2cents_local_decoder + cent_to_f0 + the uv mask (models.py:120, 149-176, 246-251,
 *   models_infer.py:204-207).  logits_dev [n_rows][ld], ld >= out_dims the row stride (columns >= out_dims are never read);
 *   latent = sigmoid(logit); per row the maximum and the LOWEST index attaining it; the nine indices argmax - 4 .. argmax + 4, each
 *   clamped to [0, out_dims - 1] (a clamped duplicate counts as often as it occurs); cents = sum(cent_table * latent) / sum(latent)
 *   over the nine; f0 = 0 when max <= threshold, else 10 * 2^(cents / 1200), and 0 when that is below f0_min.  f0_dev [n_rows];
 *   latent_dev [n_rows][out_dims] or NULL. */
int rvc_glu_dwconv_silu_f32(const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int64_t n_rows, int C, int K,
                            void *stream);
int rvc_layernorm_rows_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev, float eps, float *y_dev, int64_t n_rows,
                           int F, void *stream);
int rvc_groupnorm_workspace_bytes(int C, int64_t L, int groups, size_t *bytes);
int rvc_groupnorm_lrelu_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev, int groups, float eps, float slope,
                            float *y_dev, int C, int64_t L, void *workspace_dev, size_t workspace_bytes, void *stream);
int rvc_fcpe_decode_f32(const float *logits_dev, const float *cent_table_dev, int out_dims, int ld, float threshold, float f0_min,
                        float *f0_dev, float *latent_dev, int64_t n_rows, void *stream);

/* ---- K16: k-means for the feature-index builder -------------------------------------------------- *
 * Replaces the CPU clustering of rvc/train/process/extract_index.py:43-69: `MiniBatchKMeans(n_clusters=10000).fit(big_npy)`
 * above 2e5 rows, and the coarse-quantiser training + `add` of `faiss.index_factory(768, f"IVF{n_ivf},Flat")`.  Both are Lloyd
 * iterations over the [n_rows, dim] fp32 feature matrix; the two device steps of one iteration are exported here and the host
 * bookkeeping (sort by assignment, empty-cluster re-seeding, the inverted lists) is rvc_amd/lib/kmeans.py.
 * Common contract: dim a multiple of 32 in [32, 1024]; n_centroids >= 1; n_rows >= 0; both below 2^31; x, the centroid arrays
 * and the workspace 16-byte aligned; every argument is checked before anything touches the device; n_rows == 0 returns 0 and
 * launches nothing; all launches are asynchronous on `stream`; each call is a pure function of its inputs (no atomics, fixed
 * merge orders), so two calls give identical bits.
 *
 * rvc_kmeans_workspace_bytes: the scratch both calls ask for at this shape (one buffer serves both; the larger of the two):
 *   assign   n_centroids floats (||c||^2) + stripes x n_rows x 8 bytes, where stripes =
 *            min(ceil(1024 / ceil(n_rows / 128)), ceil(n_centroids / 512)) centroid stripes -- one from 131 k rows on: 16 MB at
 *            2 M rows, which is one call;
 *   update   (n_rows / 256 + n_centroids + 1) partial sums of dim doubles.
 * rvc_kmeans_assign: out_ids_dev[r] = the centroid nearest to row r, out_d2_dev[r] = its squared distance.
 *   Selection is by the GEMM-form score ||c||^2 - 2 x.c, the dot product on the exact-fp32 matrix cores as ONE fmaf chain
 *   over k = 0 .. dim - 1; equal scores go to the lower centroid id; the result does not depend on tiling or striping.
 *   out_d2 is sum_k (x_k - c_k)^2 of the chosen centroid only, evaluated directly in fp32: 64 interleaved fmaf chains
 *   (chain l takes the 4-float groups l, l + 64, ...), summed by the butterfly l ^ 32, 16, 8, 4, 2, 1.  Rows and centroids that
 *   do not fill a 128-tile are masked inside the kernel.
 * rvc_kmeans_update: the members of centroid j are rows order_dev[offsets_dev[j] .. offsets_dev[j + 1]) (order_dev: n_rows int32
 *   row ids, offsets_dev: n_centroids + 1 int64, ascending, as torch.argsort(ids, stable=True) + a cumulative bincount give
 *   them); out[j] = (float)(float64 sum over the members in list order / count), or old_centroids_dev[j] when it has none.
 *   Entries of order_dev that are negative or >= n_rows are skipped and not counted; offsets are clamped to [0, n_rows].  Lists
 *   longer than 256 members are summed in pieces of 256 whose partial sums are added in piece order.  out may alias old. */
int rvc_kmeans_workspace_bytes(int64_t n_rows, int64_t n_centroids, int dim, size_t *bytes);
int rvc_kmeans_assign(const float *x_dev, int64_t n_rows, int dim, const float *centroids_dev, int64_t n_centroids,
                      int32_t *out_ids_dev, float *out_d2_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int rvc_kmeans_update(const float *x_dev, int64_t n_rows, int dim, const int32_t *order_dev, const int64_t *offsets_dev,
                      int64_t n_centroids, const float *old_centroids_dev, float *out_centroids_dev, void *workspace_dev,
                      size_t workspace_bytes, void *stream);

/* ---- K17: the dataset preprocessor (csrc/preprocess.hip) ----------------------------------------------------- *
 * The device steps of rvc/train/preprocess/preprocess.py + slicer.py.  Common contract: every argument is checked on the host
 * before anything touches the device; sample indices are 64-bit; all launches are asynchronous on `stream`; no atomics, fixed
 * summation orders: two calls give identical bits.
 *
 * rvc_lfilter_order5_f64 replaces `signal.lfilter(self.b_high, self.a_high, audio)` (preprocess.py:146): y = lfilter(b, a, x),
 *   causal, zero initial state, float64, SciPy's operation sequence without FMA contraction.  coef_host (host memory, 12
 *   doubles): b[6], a[6] with a[0] == 1 and every pole inside the unit circle.  x_dev, y_dev: [n], n >= 0, must not alias.
 *   Chunks of 2048 outputs are run side by side, each from a zero state `warm` samples earlier (from sample 0 where that is
 *   nearer: those chunks are bit-exact); warm = the smallest multiple of 32 with rho^warm <= 2^-53, rho the largest pole
 *   radius of a[] -- rvc_lfilter_order5_warmup returns it.  Agrees with SciPy to the conditioning of the recurrence
 *   (csrc/preprocess.hip).
 * rvc_frame_rms_f64 replaces `get_rms(y, frame_length, hop_length)` (slicer.py:199-235): pad = frame_length / 2 zeros on both
 *   sides, frame t covers padded samples [t * hop, t * hop + frame_length), n_frames = (n + 2 * pad - frame_length) / hop + 1
 *   by floor division (0 frames when the padded signal is shorter than a frame), out[t] = sqrt(sum of squares / frame_length).
 *   frame_length >= 1, hop >= 1, n >= 0; rvc_frame_rms_frames gives n_frames and the workspace for a shape (one double per
 *   hop-long piece of the padded signal).  Every sample is read once when frame_length is a multiple of hop.
 * rvc_slice_export_f32 replaces the per-slice `astype(np.float32)` + `librosa.resample(slice, orig_sr=sr, target_sr=16000)`
 *   pairs of process_audio_segment / simple_cut (preprocess.py:64-126) with one launch per file.  bounds_host (host memory,
 *   n_seg x 2 int64): half-open sample ranges [start_s, end_s) with 0 <= start_s <= end_s <= n; they may overlap, touch or be
 *   empty.  seg_dev: the same table in device memory; off_full_dev / off_lo_dev: n_seg + 1 int64 each, the exclusive prefix sums
 *   of len_s = end_s - start_s and of ceil(len_s * up / down) (last entry = n_full / n_lo, which must match the host table).
 *     full[off_full[s] + i] = (float)x[start_s + i]                                             (round to nearest)
 *     lo[off_lo[s] + j]     = (float) sum_m h[m] * xup_s[j * down + (n_taps - 1) / 2 - m],  j < ceil(len_s * up / down)
 *   xup_s = segment s ALONE zero-stuffed by `up`, zeros outside it: rvc_resample_poly_f64's convention per segment, float64
 *   accumulation in ascending m.  up, down >= 1, n_taps odd.  A refused call writes nothing. */
int rvc_lfilter_order5_warmup(const double *coef_host, int64_t *warm);
int rvc_lfilter_order5_f64(const double *x_dev, int64_t n, const double *coef_host, double *y_dev, void *stream);
int rvc_frame_rms_frames(int64_t n, int64_t frame_length, int64_t hop, int64_t *n_frames, size_t *workspace_bytes);
int rvc_frame_rms_f64(const double *x_dev, int64_t n, int64_t frame_length, int64_t hop, double *out_dev, int64_t n_frames,
                      void *workspace_dev, size_t workspace_bytes, void *stream);
int rvc_slice_export_f32(const double *x_dev, int64_t n, const int64_t *bounds_host, const int64_t *seg_dev,
                         const int64_t *off_full_dev, const int64_t *off_lo_dev, int64_t n_seg, int up, int down,
                         const double *h_dev, int64_t n_taps, float *full_dev, int64_t n_full, float *lo_dev, int64_t n_lo,
                         void *stream);

/* ---- K18: clean_audio, a non-stationary spectral gate (csrc/spectralgate.hip) ---------------------------------- *
 * Replaces `noisereduce.reduce_noise(y=audio, sr=sr, prop_decrease=p)` (rvc/infer/infer.py:77-93) in its default,
 * stationary=False form.  noisereduce absent: parity with the wheel unpinned -- the algorithm below IS the contract, and the
 * yardstick is its float64 SciPy restatement in tests/spectral_gate_ref.py.
 *
 * Constants: n_fft = win = 1024, hop = 256, time_constant_s = 2, thresh = 2, slope = 10, freq_mask_smooth_hz = 500,
 * time_mask_smooth_ms = 50.  Chunks: [0, n) when n <= chunk_size, else [s, min(s + chunk_size, n)) for s = 0, chunk_size, ...;
 * chunk [s, e) is filtered inside the buffer c = y[s - padding : e + padding] (zeros outside [0, n)), L = e - s + 2 padding, and
 * out[s:e] = filtered[padding : padding + e - s].  Chunks are independent.  Filtering one buffer:
 *   1. S = STFT of c: periodic hann(1024), hop 256, 512 zeros on each side, F = L / 256 + 1 frames (scipy.signal.stft,
 *      boundary='zeros', padded=False; its 1 / sum(win) scaling cancels against step 7 and is not applied);
 *   2. A = |S|;
 *   3. M = the one-pole smoother f[t] = b A[t] + (1 - b) f[t - 1] run forward, then backward over f, along time per bin, each
 *      pass starting as if the sample before its first equalled it (scipy.signal.filtfilt([b], [1, b - 1], padtype=None));
 *      t = 2 sr / 256, b = (sqrt(1 + 4 t^2) - 1) / (2 t^2);
 *   4. mask = 1 / (1 + exp(-((A - M) / M - 2) * 10)); a bin that is zero in every frame (M == 0) takes (A - M) / M = 0: its mask
 *      is finite and its output zero, where noisereduce yields NaN for digital silence;
 *   5. mask = the 2-D convolution (mode "same", zeros outside) of mask with outer(ramp(nf), ramp(nt)) / sum, applied as its two
 *      1-D factors; nf = int(500 / (sr / 512)) bins, nt = int(50 / ((256 / sr) * 1000)) frames, ramp(k)[d] = (k + 1 - |d|) / (k + 1)
 *      for |d| <= k (11 x 19 points at 48 kHz); nf, nt and b are evaluated on the host in float64 with exactly these expressions;
 *   6. mask = mask * prop_decrease + (1 - prop_decrease);
 *   7. x = the inverse rDFT of S * mask per frame (imaginary parts of the DC and Nyquist bins ignored), times the window,
 *      overlap-added, divided by the running sum of win^2 of the frames that cover the sample, trimmed by 512 on each side:
 *      L - L % 256 samples; filtered = x followed by zeros (that tail lies in the padding whenever padding >= 256).
 * Arithmetic: fp32 throughout, except the state of the recurrence of step 3, which is float64 (M itself is kept as fp32).  Both
 * transforms are dense DFTs on the exact-fp32 matrix cores: a dot product is summed as fmaf chains in index order over
 * consecutive ranges of its terms -- 16 chains of 64 samples forward, 4 chains of 288 spectral rows inverse -- whose sums are
 * added in range order.  Every output sample sums its <= 4 frames in frame order, nothing is accumulated atomically: two
 * calls give identical bits, on any stream.  Against the float64 restatement the output deviates by 4 to 10 times what SciPy's
 * own float32 path does (4e-7 .. 8e-7 absolute on a signal of amplitude 0.5).
 *
 * rvc_spectral_gate_params: nf, nt, b of `sr` and, where the pointers are not NULL, the normalised 1-D factors of step 5 as
 *   freq_taps[0 .. nf] / time_taps[0 .. nt] (the weight at distance |d|; host memory, room for 51 doubles each).  No device access.
 * rvc_spectral_gate_workspace_bytes: the scratch one call needs: 17.5 KiB per frame of min(number of chunks, chunks per group)
 *   chunks, where a group holds as many whole chunks as fit into 8192 frames (at least one).  It depends on chunk_size and
 *   padding but, once the signal fills one group, not on n: longer signals are walked group by group.  0 when n == 0.
 * rvc_spectral_gate_f32: y_dev[n] -> out_dev[n] (fp32, must not alias), asynchronous on `hip_stream` (the library's usual
 *   trailing `void *stream` argument).  Refused with an error, before anything touches the device: a NULL y_dev, out_dev or
 *   workspace_dev; n < 0; sr outside [5120, 256000] (nt or nf would be 0); prop_decrease outside [0, 1]; chunk_size < 1;
 *   padding < 0; min(chunk_size, n) + 2 padding above 2^27 samples; workspace_bytes below the size query's answer.  n == 0
 *   succeeds and writes nothing.  The DFT bases and the window are uploaded once per device, on the first call there. */
int rvc_spectral_gate_params(int sr, int *nf, int *nt, double *b, double *freq_taps, double *time_taps);
int rvc_spectral_gate_workspace_bytes(int64_t n, int sr, int64_t chunk_size, int64_t padding, size_t *bytes);
int rvc_spectral_gate_f32(const float *y_dev, int64_t n, int sr, float prop_decrease, int64_t chunk_size, int64_t padding,
                          float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* ---- K19: formant_shifting, a cepstral spectral-envelope edit (csrc/formant.hip) --------------------------------- *
 * Replaces `stftpitchshift.StftPitchShift(1024, 32, sr).shiftpitch(audio, factors=1, quefrency=formant_qfrency * 1e-3,
 * distortion=formant_timbre)` (rvc/lib/utils.py:70-82) on the 16 kHz input.  stftpitchshift absent: parity with the wheel
 * unpinned -- the algorithm below IS the contract, and the yardstick is its float64 SciPy restatement in
 * tests/formant_shift_ref.py.
 *
 * Input x[n], fp32, at sr.  Constants: N = 1024, H = 32, B = 513.  Q = int(quefrency_s * sr), d = distortion.
 *   1. Frames.  F = (n - N) / H + 1 (integer division); frame t is x[tH .. tH + N), no centre padding, times the periodic Hann
 *      window w[i] = 0.5 - 0.5 cos(2 pi i / N); forward rDFT scaled by 1 / N: S[t][k], k < B.
 *   2. Envelope, only when Q > 0, per frame.  L[k] = log10 |S[k]|.  Cepstrum c[q] = L[0] + (-1)^q L[512] +
 *      2 sum_{k=1..511} L[k] cos(2 pi q k / N) (irfft(L, norm="forward")).  Lifter: keep c[0], double c[1 .. Q-1], keep c[Q]
 *      once, zero above.  E[k] = 10 ** ((1 / N) sum_q c'[q] cos(2 pi q k / N)) (rfft(c', norm="forward").real).  A value is "not
 *      normal" when it is inf, NaN or below the smallest normal number of its type.  mask1 = notnormal(E).  G[k] = |S[k]| / E[k],
 *      and 0 where mask1.
 *   3. Warp.  If d == 1, E' = E.  Otherwise E[mask1] = 0 and E is resampled linearly: m = int(B * d); for i < min(B, m):
 *      pos = i * (B / m), j = trunc(pos), f = pos - j, E'[i] = f E[j+1] + (1 - f) E[j] when j < B - 1, else 0; E'[i] = 0 for
 *      i >= min(B, m).  mask2 = notnormal(E').  G[k] *= E'[k], and 0 where mask2.  So for d < 1 the bins from int(513 d) up are
 *      silenced (the wheel's behaviour).  With Q == 0, G = |S|: the call is only the STFT round trip.
 *   4. Output spectrum Y = G S / |S|, and 0 where |S| == 0.  (The wheel's phase-vocoder encode / decode with factors = 1 is the
 *      identity on the phase modulo 2 pi and is not built.)
 *   5. Inverse.  Unscaled inverse rDFT of Y (irfft(norm="forward"): DC and Nyquist counted once, their imaginary parts ignored),
 *      times w H / sum(w^2), overlap-added at tH.  Output sample s is the sum of its <= 32 frames in frame order, as a gather: no
 *      atomics, identical bits on every call.  Samples at or beyond (F - 1) H + N are 0.  The output has length n.  The tapered
 *      first and last 1024 samples and the dead tail are the wheel's own edge behaviour.
 * Degenerate frames: a frame with any bin of magnitude exactly 0 (digital silence) has L = -inf, its whole envelope is NaN, every
 * bin is masked and the frame contributes zeros -- zeros on the device too, never NaN or inf.
 * Arithmetic: both transforms are K18's dense DFTs on the exact-fp32 matrix cores (16 fmaf chains of 64 samples forward, 4 of 288
 * spectral rows inverse, added in range order); |S|, L, c, E, E' and G are float64 on the device, cosines from a 1024-entry
 * float64 table at (q k) mod 1024, the warp positions float64 with exactly the expressions of step 3; "not normal" is tested on
 * the fp32 rounding of E and E'; the gain ratio G / |S| and everything after it are fp32.  Against the float64 restatement the
 * output deviates by 1 to 5 times what SciPy's own float32 path does on the tests' cases (1e-7 .. 6e-7 absolute at a peak of
 * 0.3), and by 15 times on a 30 s signal.
 *
 * rvc_formant_shift_workspace_bytes: the scratch one call needs: 15.25 KiB per frame of min(F, group) frames rounded up to 128,
 *   plus 141 824 bytes; group = group_frames, or 8192 when that is 0.  Once the signal fills one group it does not depend on n:
 *   longer signals are walked group by group, the 31 last inverse frames of a group kept for the next one's overlap-add, so the
 *   output does not depend on group_frames either.  Refuses n and group_frames as the forward call does.
 * rvc_formant_shift_f32: x_dev[n] -> out_dev[n], asynchronous on `hip_stream` (the library's usual trailing `void *stream`
 *   argument).  Refused with an error, before anything touches the device: a NULL x_dev, out_dev or workspace_dev;
 *   out_dev == x_dev; n < 1024 (the wheel cannot frame it either); n above 2^27; sr < 1; quefrency_s < 0, or Q > 511; distortion
 *   not finite or <= 0, or int(513 * distortion) < 1; group_frames neither 0 nor a multiple of 128 in [128, 8192];
 *   workspace_bytes below the size query's answer. */
int rvc_formant_shift_workspace_bytes(int64_t n, int group_frames, size_t *bytes);
int rvc_formant_shift_f32(const float *x_dev, int64_t n, int sr, double quefrency_s, double distortion, int group_frames,
                          float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* ---- K20: the validation losses (csrc/valmetrics.hip) --------------------------------------------------------------- *
 * The sums behind the three figures the reference's validation_loop logs per item (rvc/train/train.py:1478-1579): a
 * multi-resolution STFT loss (`auraloss.freq.MultiResolutionSTFTLoss()` with its defaults), SI-SDR (train.py:244-257) and the
 * mel L1 (train.py:1525-1532).  auraloss absent: parity with the wheel unpinned -- the algorithm below IS the contract, and the
 * yardstick is its float64 torch.stft restatement in tests/validation_ref.py.  PESQ is not built.
 *
 * Every entry point writes float64 SUMS to device memory and the host finishes the square roots, quotients and logarithms.
 * Every sum is accumulated in float64: per thread in index order, per workgroup as 256 values added in thread order, and the
 * workgroups' partial sums by a second kernel (256 interleaved sums in workgroup order, then added in order).  Nothing is
 * accumulated atomically: two calls give identical bits, on any stream.
 *
 * Multi-resolution STFT sums.  x (the prediction) and y (the target): fp32 [n].  For each resolution (n_fft, hop, win), the same
 * for both signals:
 *   1. Frames as torch.stft(center=True, pad_mode="reflect") takes them: the signal is extended by n_fft / 2 samples on each side
 *      by reflection without repeating the edge sample, F = 1 + n / hop frames (integer division), frame t starts at t hop of the
 *      extended signal; window = the periodic Hann window of `win` samples, w[i] = 0.5 - 0.5 cos(2 pi i / win), zero-padded to
 *      n_fft with (n_fft - win) / 2 zeros in front; S[t][k] = the unscaled rDFT, k <= n_fft / 2.
 *   2. P[t][k] = max(re^2 + im^2, eps); mag = sqrt(P).
 *   3. out[4 r + 0] = sum (ymag - xmag)^2, out[4 r + 1] = sum ymag^2 (= sum Py), out[4 r + 2] = sum |log xmag - log ymag|
 *      (= sum 0.5 |log Px - log Py|), out[4 r + 3] = F (n_fft / 2 + 1), the number of terms, for resolution r.
 *   The host forms sc = sqrt(out[0] / out[1]), lm = out[2] / out[3], and the loss = the mean over the resolutions of sc + lm.
 * Arithmetic: the DFT is a GEMM on the exact-fp32 matrix cores over the `win` samples the window keeps: a dot product is summed
 * as fmaf chains in sample order over consecutive ranges of 64 samples whose sums are added in range order; the window (fp32
 * roundings of float64 values) multiplies the sample in fp32; cosines and sines are fp32 roundings of float64 values looked up at
 * (sample index * k) mod n_fft.  The Nyquist bin is computed as sum (-1)^i of the windowed frame.  P, the square roots, the
 * logarithms and the three sums are float64.  A workgroup owns 32 frames x 256 bins and keeps both signals' samples in LDS; no
 * spectrogram is written to HBM.  x == y gives exactly 0 for the first and third sum; two silent signals give 0 too, and a
 * positive second sum (F (n_fft / 2 + 1) eps).
 *
 * rvc_mrstft_sums_workspace_bytes: the scratch one call needs: 24 bytes per workgroup, ceil(F / 32) (n_fft / 512) workgroups per
 *   resolution.  No device access; refuses what the forward call refuses about n and the resolutions.
 * rvc_mrstft_sums_f32: x_dev[n], y_dev[n] -> out_dev[4 n_res] float64, asynchronous on `hip_stream` (the library's usual trailing
 *   `void *stream` argument); n_fft, hop, win: host arrays of n_res entries.  Refused with an error, before anything touches the
 *   device: a NULL x_dev, y_dev, out_dev, workspace_dev or host array; a signal not 4-byte aligned, out_dev or workspace_dev not
 *   8-byte aligned; n_res outside [1, 4]; n_fft other than 512, 1024 and 2048; win outside [1, n_fft]; hop outside [1, 512];
 *   n <= n_fft / 2 (the reflect padding is undefined); n above 2^27; eps not positive and finite; workspace_bytes below the
 *   size query's answer.
 *
 * SI-SDR sums.  out[0] = sum p, out[1] = sum t; then with pc = p - out[0] / n and tc = t - out[1] / n (float64): out[2] =
 * sum pc tc, out[3] = sum tc^2, out[4] = sum pc^2: two passes over the signals.  The host evaluates the reference's expression:
 * s = out[2] / (out[3] + eps), projection energy s^2 out[3], noise energy out[4] - 2 s out[2] + s^2 out[3], SI-SDR =
 * 10 log10(projection / noise + eps).  (The noise energy is a difference of sums: once it falls below their float64 resolution,
 * 2^-48 out[4], the host takes it as 0 and the result is +inf, which is what the reference's fp32 expression gives for an
 * identical pair.)
 * rvc_si_sdr_sums_workspace_bytes / rvc_si_sdr_sums_f32: preds_dev[n], target_dev[n] -> out_dev[5] float64.  Refused: NULL or
 *   misaligned pointers as above, n < 2, a short workspace (24 bytes per workgroup, min(1024, ceil(n / 256)) workgroups).
 *
 * Mean absolute difference sum.  a and b: row-major fp32 matrices of `rows` rows with row strides a_stride and b_stride (in
 * elements); out[0] = sum over r < rows, c < min_t of |a[r][c] - b[r][c]| (the difference in float64); the mean is
 * out[0] / (rows min_t).  With a the mel of the prediction, b the mel of the target and min_t the shorter of their widths this is
 * F.l1_loss(y_hat_mel[..., :min_t], mel[..., :min_t]).
 * rvc_mean_abs_diff_workspace_bytes / rvc_mean_abs_diff_f32: -> out_dev[1] float64.  Refused: NULL or misaligned pointers as
 *   above, rows or min_t below 1 or above 2^27, more than 2^40 elements, a stride below min_t, a short workspace (8 bytes per
 *   workgroup, min(1024, ceil(rows min_t / 256)) workgroups). */
int rvc_mrstft_sums_workspace_bytes(int64_t n, const int *n_fft, const int *hop, const int *win, int n_res, size_t *bytes);
int rvc_mrstft_sums_f32(const float *x_dev, const float *y_dev, int64_t n, const int *n_fft, const int *hop, const int *win, int n_res,
                        double eps, double *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);
int rvc_si_sdr_sums_workspace_bytes(int64_t n, size_t *bytes);
int rvc_si_sdr_sums_f32(const float *preds_dev, const float *target_dev, int64_t n, double *out_dev, void *workspace_dev,
                        size_t workspace_bytes, void *hip_stream);
int rvc_mean_abs_diff_workspace_bytes(int64_t rows, int64_t min_t, size_t *bytes);
int rvc_mean_abs_diff_f32(const float *a_dev, int64_t a_stride, const float *b_dev, int64_t b_stride, int64_t rows, int64_t min_t,
                          double *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* ---- K21: the seam of block-by-block conversion, SOLA (csrc/sola.hip) ----------------------------------------------- *
 * Streaming conversion (rvc_amd/infer/realtime.py) converts a window [carried history | new block] per push and keeps the last
 * B + X + S samples of the result.  Two consecutive results never line up in phase -- the synthesizer draws fresh noise per call
 * -- so each one is slid against the tail saved from the previous one to the lag of best normalised correlation and crossfaded
 * (synchronised overlap-add).  The reference has no such mode: the algorithm below IS the contract, and the yardstick is its
 * float64 NumPy restatement in tests/sola_ref.py.
 *
 * Lengths in output samples: X = xfade, S = search, B = block.  infer[0 .. B + X + S), fp32; buf[0 .. X), fp32, in/out: the tail
 * the previous call saved, zeros after a reset; fade_in[0 .. X), fp32: the caller's fade, for the stream sin^2(pi i / (2 X))
 * evaluated in float64 and rounded to fp32.
 *   1. Score.  For every lag o in 0 .. S inclusive: nom(o) = sum_{i < X} infer[o + i] buf[i], den(o) = sqrt(sum_{i < X}
 *      infer[o + i]^2 + 1e-8), score(o) = nom(o) / den(o).
 *   2. offset = the LOWEST o that attains the maximum score.  An all-zero buf scores 0 everywhere and gives offset 0.
 *   3. out[i] = infer[offset + i] for i < B; for i < X instead out[i] = infer[offset + i] fade_in[i] + buf[i] (1 - fade_in[i]).
 *   4. buf[i] <- infer[offset + B + i], i < X (read for step 3 before it is overwritten).
 *   5. *offset_dev = offset (int32, device memory; the library never reads it back).
 * Arithmetic: fp32.  The two sums of a lag are accumulated per lane over i = lane, lane + 256, ... in index order, the 256 lanes'
 * sums added by a fixed tree (within a wave of 64 at distances 32, 16, .. 1, then the four waves in order); the quotient and the
 * square root are correctly rounded; steps 3 and 4 are plain fp32 expressions and copies.  Nothing is accumulated atomically: two
 * calls give identical bits, on any stream.  A NaN score (a NaN or inf in infer) never wins step 2, which then still yields a lag in
 * 0 .. S.  Two launches, no synchronisation, no host copy.
 *
 * rvc_sola_workspace_bytes: the scratch one call needs, 4 (S + 1) bytes (the scores).  Refused: a NULL bytes; xfade < 1; search
 *   < 0; either above 2^24.  No device access.
 * rvc_sola_f32: asynchronous on `hip_stream` (the library's usual trailing `void *stream` argument).  Refused with an error, before
 *   anything touches the device: a NULL infer_dev, buf_dev, fade_in_dev, out_dev, offset_dev or workspace_dev; xfade < 1; xfade >
 *   block; search < 0; n_infer above 2^24; n_infer != block + xfade + search; workspace_bytes below the size query's answer;
 *   out_dev[0 .. B) overlapping infer_dev[0 .. n_infer) or buf_dev[0 .. X); buf_dev overlapping infer_dev.
 * rvc_stream_window_f32: window_dev[0 .. n_hist + n_block) = [hist_dev | block_dev], then hist_dev <- the last n_hist samples of
 *   the window (for n_block >= n_hist the end of the block; otherwise the history moves up by n_block).  One launch of one
 *   workgroup -- the two steps are ordered by its barrier -- sized for a second or two of 16 kHz audio.  n_hist == 0 is allowed
 *   (the window is the block), and so is n_block == 0; n_hist + n_block == 0 launches nothing.  Refused, before anything touches
 *   the device: a NULL pointer (also with a length of 0); a negative length; n_hist + n_block above 2^24; window_dev overlapping
 *   hist_dev[0 .. n_hist) or block_dev[0 .. n_block). */
int rvc_sola_workspace_bytes(int64_t xfade, int64_t search, size_t *bytes);
int rvc_sola_f32(const float *infer_dev, int64_t n_infer, float *buf_dev, const float *fade_in_dev, int64_t xfade, int64_t search,
                 int64_t block, float *out_dev, int *offset_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);
int rvc_stream_window_f32(float *hist_dev, int64_t n_hist, const float *block_dev, int64_t n_block, float *window_dev,
                          void *hip_stream);

/* ---- K22: post_process, the effects board (csrc/effects.hip) -------------------------------------------------------- *
 * Replaces the `pedalboard` chain of post_process_audio (rvc/infer/infer.py:130-191) on the converted waveform.  The pedalboard
 * wheel (JUCE underneath) is absent: the formulas below were written down from memory of JUCE / pedalboard and could not be
 * checked against either, so parity with the wheel is unpinned -- the algorithm below IS the contract, and the yardstick is its
 * float64 NumPy restatement in tests/effects_ref.py.  Parameters are constant over the signal: JUCE's 50 ms parameter smoothing
 * is NOT modelled.  PitchShift (Rubber Band) is not built and has no entry point.
 *
 * Every call: mono fp32 x[n] -> fp32 out[n] (tails are cut at n), asynchronous on `hip_stream`.  dB values become linear factors
 * as 10^(dB / 20) in double on the host and are rounded to fp32 once; so are 1 - mix, 1 - damp and the other derived constants.
 *   pointwise   `stages` is a set of gain 1 | distortion 2 | bitcrush 4 | clipping 8; the enabled ones run in that order in one
 *               pass.  gain: y = x g, g = 10^(gain_db / 20).  distortion: y = tanh(x 10^(drive_db / 20)).  bitcrush: y = rint(x 2^b)
 *               / 2^b, round-half-even, 0 < b <= 32.  clipping: y = clamp(x, -t, t), t = 10^(clip_threshold_db / 20).
 *   delay       D = floor(delay_seconds sr), D >= 1.  d[m] = x[m - D] + fb d[m - D] (0 for m < D); y[m] = (1 - mix) x[m] + mix d[m].
 *   chorus      per sample m, in float64: ph = frac(rate_hz m / sr), lfo = sin(2 pi ph), ms = max(1, centre_delay_ms + (10 depth)
 *               lfo), dl = ms sr / 1000, i = floor(dl), f = dl - i (then fp32).  p[m] = x[m] - fb w[m - 1]; w[m] = p[m - i] + f
 *               (p[m - i - 1] - p[m - i]) with p[< 0] = 0, w[-1] = 0; y[m] = (1 - mix) x[m] + mix w[m].
 *   reverb      Freeverb, mono path.  in = 0.015 x, or 0 when freeze_mode >= 0.5.  Eight parallel combs of length (sr T) / 44100
 *               (integer division), T = 1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617, each: o = line[idx]; last = o (1 - damp) +
 *               last damp; line[idx] = in + last feedback.  Their outputs added in that order go through four series allpasses, T =
 *               556, 441, 341, 225, each: b = line[idx]; line[idx] = in + 0.5 b; out = b - in.  y = out wet1 + x dry.  damp = 0.4
 *               damping, feedback = 0.28 room_size + 0.7 (frozen: damp = 0, feedback = 1); wet1 = 1.5 wet_level (1 + width), dry =
 *               2 dry_level.
 *   compressor  e[m] = a + c (e[m - 1] - a), a = |x[m]|, e[-1] = 0, c = c_attack if a > e[m - 1] else c_release; c_* =
 *               exp(-2 pi 1000 / (sr t_ms)) for t_ms = attack_ms / release_ms, and 0 when t_ms <= 1e-3.  gain = 1 if e < thr else
 *               (e / thr)^(1 / ratio - 1), thr = 10^(threshold_db / 20); y = gain x.
 *   limiter     compressor(-10 dB, ratio 4, attack 2 ms, release 200 ms), then compressor(threshold_db, ratio 1000, attack
 *               0.001 ms (c_attack = 0), release_ms), then times 10^(7.5 / 40) 10^(-threshold_db / 20), then clamp to [-1, 1].
 * Arithmetic: fp32 (subnormals kept), a x + b as one fused multiply-add where the formula has that shape; the chorus tap position
 * float64.  Where the state lives: the delay and the allpasses keep their line in a register (one lane per residue class mod the
 * line's length: no line exists in memory); a comb's line is its output row in the workspace and its damping filter is scanned
 * over chunks of the comb's length by one workgroup; the chorus with feedback keeps p[] in the workspace and walks blocks of the
 * shortest tap delay in ONE workgroup (slow: n / block steps; feedback 0 is a plain gather); the compressor runs chunks of the
 * signal from the two entry states 0 and max|x| -- every step is a monotone map of the state, in floating point too, so a chunk
 * whose two end states are bit-identical has THE end state -- then chains the chunks that did not close and runs every chunk from
 * its exact entry state.  Its output is the sequential recurrence's bit for bit and does not depend on `chunk` (0: the library
 * chooses ceil(28 / -ln max(c_attack, c_release)), at least 256).  A release so long that no chunk closes degrades to one lane
 * walking the signal: correct, and slow.  No atomics except a maximum: two calls give identical bits.
 *
 * Accepted: 0 <= n <= 2^27 (n == 0 succeeds and touches nothing); 8000 <= sr <= 96000.  Refused with an error that names the
 * argument, before anything touches the device: a NULL pointer; n or sr outside that; any dB value outside [-200, 200]; stages
 * outside 1 .. 15 (only the enabled stages' parameters are looked at); bit_depth outside (0, 32]; delay_seconds outside [0, 60] or
 * shorter than one sample; feedback outside [-1, 1]; mix outside [0, 1]; rate_hz outside [0, 100]; depth outside [0, 10];
 * centre_delay_ms, or centre_delay_ms + 10 depth, outside [0, 100]; room_size, damping, wet_level, dry_level, width, freeze_mode
 * outside [0, 1]; ratio outside [1, 1e6]; attack_ms, release_ms outside [0, 1e6]; chunk < 0; limiter neither 0 nor 1; NaN
 * anywhere; workspace_bytes below the size query's answer; out_dev overlapping x_dev (pointwise alone allows out_dev == x_dev);
 * the workspace overlapping either.
 *
 * rvc_fx_reverb_params: the eight comb and four allpass lengths at sr (host only).  rvc_fx_ballistics: c_attack and c_release in
 *   double, as the compressor derives them before rounding to fp32 (host only).
 * rvc_fx_chorus_workspace_bytes: 0 for feedback == 0 (workspace_dev may then be NULL), else 12 n.  rvc_fx_reverb_workspace_bytes:
 *   36 n.  rvc_fx_compressor_workspace_bytes: 16 + 12 ceil(n / chunk) rounded up to 16 (chunk 0 counts as 256), plus 4 n for the
 *   limiter (`limiter` = 1). */
int rvc_fx_pointwise_f32(const float *x_dev, int64_t n, int stages, double gain_db, double drive_db, double bit_depth,
                         double clip_threshold_db, float *out_dev, void *hip_stream);
int rvc_fx_delay_f32(const float *x_dev, int64_t n, int sr, double delay_seconds, double feedback, double mix, float *out_dev,
                     void *hip_stream);
int rvc_fx_chorus_workspace_bytes(int64_t n, double feedback, size_t *bytes);
int rvc_fx_chorus_f32(const float *x_dev, int64_t n, int sr, double rate_hz, double depth, double centre_delay_ms, double feedback,
                      double mix, float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);
int rvc_fx_reverb_params(int sr, int *comb_len, int *allpass_len);
int rvc_fx_reverb_workspace_bytes(int64_t n, size_t *bytes);
int rvc_fx_reverb_f32(const float *x_dev, int64_t n, int sr, double room_size, double damping, double wet_level, double dry_level,
                      double width, double freeze_mode, float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);
int rvc_fx_ballistics(int sr, double attack_ms, double release_ms, double *c_attack, double *c_release);
int rvc_fx_compressor_workspace_bytes(int64_t n, int64_t chunk, int limiter, size_t *bytes);
int rvc_fx_compressor_f32(const float *x_dev, int64_t n, int sr, double threshold_db, double ratio, double attack_ms,
                          double release_ms, int64_t chunk, float *out_dev, void *workspace_dev, size_t workspace_bytes,
                          void *hip_stream);
int rvc_fx_limiter_f32(const float *x_dev, int64_t n, int sr, double threshold_db, double release_ms, int64_t chunk, float *out_dev,
                       void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* ---- K23: the audio analyzer's spectral features (csrc/specfeat.hip) -------------------------------------------------- *
 * What calculate_features of the reference's audio analyzer (rvc/lib/tools/analyzer.py) takes from librosa 0.11 with the defaults
 * its calls use: stft -> |S|, spectral_centroid, spectral_bandwidth, spectral_rolloff, and amplitude_to_db(|S|, ref = np.max) for
 * the figure.  librosa absent: parity with the wheel unpinned -- the algorithm below IS the contract, and the yardstick is its
 * float64 scipy.fft restatement in tests/spectral_features_ref.py.
 *
 * x: fp32 [n] at `sr`.  N = 2048, H = 512, B = 1025.
 *   1. Frames.  center = True with pad_mode = "constant": x is extended by 1024 zeros on each side; F = 1 + n / 512 frames (integer
 *      division); frame t is xpad[t H .. t H + N) times the periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / N); S[t][k] = the
 *      unscaled rDFT, k < B; m = |S| (fp32).
 *   2. Per frame, in float64 over the fp32 magnitudes, with f_k = k sr / N: s0 = sum m; mn = m / s0, or m / 1 when s0 is below the
 *      smallest normal float32 (normalize(norm = 1) and its `tiny` threshold); centroid c = sum f_k mn_k; bandwidth =
 *      sqrt(sum mn_k (f_k - c)^2) (p = 2, norm = True); roll-off = f_j for the first j whose cumulative sum m_0 + .. + m_j is at
 *      least roll_percent s0.  A frame of digital silence gives 0, 0 and 0 Hz, never NaN.
 *   3. dB plane (optional): R = the maximum of m over the whole signal; db = 10 log10(max(1e-10, m^2)) - 10 log10(max(1e-10, R^2)),
 *      then max(db, max(db) - 80).  An all-silent signal gives 0 everywhere.
 *   4. cent, bw, rolloff: float64 [F].  mag and db: fp32 [F][B], frame-major, each optional: a NULL pointer skips that plane, and
 *      with both NULL no spectrogram reaches HBM at all.
 * Arithmetic: the DFT is a GEMM on the exact-fp32 matrix cores: a dot product is summed as fmaf chains in sample order over
 * consecutive ranges of 64 samples whose sums are added in range order; the window (fp32 roundings of float64 values) multiplies
 * the sample in fp32; cosines and sines are fp32 roundings of float64 values looked up at (sample index * k) mod 2048.  The Nyquist
 * bin is computed as sum (-1)^i of the windowed frame.  |S| is formed in FLOAT64 from the fp32 real and imaginary parts
 * (sqrt(re^2 + im^2), the squares exact) and rounded to fp32 once.  A workgroup owns 32 frames and all their bins and keeps the
 * magnitudes in LDS; the sums of step 2 are float64, partial per range of 64 consecutive bins (the last range holds bin 1024 too)
 * and merged in bin order.  The bandwidth is the TWO-PASS form: the centroid is merged first, then sum mn_k (f_k - c)^2 runs over the
 * magnitudes held in LDS -- no difference of moments.  The roll-off scan of a range starts from the merged sum of the ranges
 * before it.  The dB plane is float64 per element (log10) and rounded to fp32; its maximum is found in a first pass (per-workgroup
 * maxima of m, merged per group of launches) and applied in a second, in place.  Nothing is accumulated atomically and a maximum
 * does not depend on order: two calls give identical bits, on any stream, with or without either plane.
 *
 * rvc_spectral_features_workspace_bytes: the scratch one call needs: 256 bytes + 4 per workgroup of one launch group (ceil(F / 32)
 *   workgroups, at most 128 = 4096 frames: a longer signal is walked group by group and needs no more), rounded up to 256.  No device access;
 *   refuses n < 1 and n above 2^27.
 * rvc_spectral_features_f32: asynchronous on `hip_stream` (the library's usual trailing `void *stream` argument).  Refused with an
 *   error, before anything touches the device: a NULL x_dev, cent_dev, bw_dev, rolloff_dev or workspace_dev; a signal, plane or
 *   workspace not 4-byte aligned, a curve not 8-byte aligned; n < 1 or n > 2^27; sr < 1; roll_percent not finite or outside the
 *   open interval (0, 1); db_dev == mag_dev when both are non-NULL; workspace_bytes below the size query's answer. */
int rvc_spectral_features_workspace_bytes(int64_t n, size_t *bytes);
int rvc_spectral_features_f32(const float *x_dev, int64_t n, int sr, double roll_percent, float *mag_dev, float *db_dev,
                              double *cent_dev, double *bw_dev, double *rolloff_dev, void *workspace_dev, size_t workspace_bytes,
                              void *hip_stream);

/* ---- K24: the conversion scorer (csrc/convscore.hip) ------------------------------------------------------------------ *
 * How good is a conversion: the mel-cepstral distortion against a parallel target after dynamic time warping, and the F0 tracking
 * errors between the input and the converted output.  The reference has no such tool and no third-party MCD package was
 * available: the algorithm below IS the contract, and the yardstick is its float64 NumPy restatement in
 * tests/conversion_score_ref.py.  Parity with any MCD package is unpinned.
 *
 * rvc_melcep_f32: x fp32 [n] at `sr` (a multiple of 200 in 8000 .. 48000) -> c fp32 [T][n_coef].
 *   1. hop = sr / 200 (5 ms); T = 1 + n / hop (integer division); frame t is samples [t hop - 512, t hop + 512) of x extended with
 *      zeros, times the periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / 1024); S[t][k] = the unscaled rDFT, k <= 512.
 *   2. P[k] = re^2 + im^2;  M[m] = sum_k W[m][k] P[k] with W = mel_dev, fp32 [n_mels][513], row-major (the caller's filterbank);
 *      L[m] = 0.5 ln(max(M[m], 1e-10));  c[k] = (1 / n_mels) sum_m L[m] cos(pi k (2 m + 1) / (2 n_mels)), k = 1 .. n_coef (c[0], the
 *      energy term, is left out).
 *   Arithmetic: the DFT is the GEMM of K18 / K19 on the exact-fp32 matrix cores (window times sample in fp32; a dot product summed as
 *   16 fmaf chains of 64 samples added in order).  Everything after it is FLOAT64: P from the fp32 re and im; M as 64 interleaved
 *   partial sums (bins k = lane mod 64) merged by a fixed pairwise tree; the log; the DCT summed in order of m with the cosine
 *   argument reduced exactly; one rounding to fp32 at the end.  The power spectrum goes through the workspace, a group of at most
 *   2048 frames at a time, so the scratch does not grow with the signal.  Digital silence gives c = 0 exactly up to the DCT's own
 *   rounding (every L[m] is 0.5 ln 1e-10).  Two calls give identical bits.
 *   Refused: a NULL or misaligned pointer; n < 1 or n > 2^27; sr outside the rule; n_coef outside 1 .. 40; n_mels outside
 *   n_coef + 1 .. 128; workspace_bytes below rvc_melcep_workspace_bytes(n, sr) (= 8704 bytes per frame of one group rounded up to
 *   128 frames: 17 MiB from 2048 frames on).
 *
 * rvc_dtw_f64: a fp32 [Ta][dim], b fp32 [Tb][dim], 1 <= Ta, Tb <= 16384, 1 <= dim <= 64.
 *   d(i, j) = sqrt(sum_q (a[i][q] - b[j][q])^2) in float64, the terms added in the order q = 0 .. dim - 1 (fused multiply-add).
 *   D(0, 0) = d(0, 0); otherwise D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)) in float64; the predecessors are tried in
 *   that order and a later one replaces the best only when STRICTLY smaller; a predecessor outside the lattice counts as +inf.
 *   band < 0: every cell is admissible.  band >= 1: cell (i, j) is admissible iff |j (Ta - 1) - i (Tb - 1)| <= band max(Ta - 1, Tb - 1);
 *   every cell is admissible when Ta == 1 or Tb == 1.  band == 0 is refused.  An inadmissible cell has D = +inf.
 *   out_dev: double [2] = {D(Ta - 1, Tb - 1), L}.  path_dev: int32 [Ta + Tb - 1][2]; rows 0 .. L - 1 receive the warping path (i, j)
 *   from (0, 0) to (Ta - 1, Tb - 1), rows past L are left untouched.
 *   One workgroup walks the lattice along its anti-diagonals, 1024 rows at a time (512 above dim 32); no workgroup waits on another,
 *   nothing spins, and the backtrace stops after Ta + Tb - 1 steps whatever the features hold.  Two calls give identical bits.
 *   rvc_dtw_workspace_bytes(Ta, Tb): 8 Tb (the row handed from one pass to the next) + 4 Ta ceil(Tb / 16) (the predecessor of every
 *   cell, 2 bits each) + 8 (Ta + Tb - 1) (the path backwards), each rounded up to 256: 64.4 MiB at 16384 x 16384.
 *   Refused: a NULL or misaligned pointer; Ta, Tb or dim outside the limits; band == 0; a workspace below the query's answer.
 *
 * rvc_frame_dist_sum_f64: out_dev[0] = sum_{t < T} d(t, t) of the first T frames of a and b (the aligned distortion, no DTW): 256
 *   partial sums (t mod 256) added in order.  1 <= T <= 2^24, 1 <= dim <= 64.
 *
 * rvc_f0_track_sums_f64: two float64 F0 contours of n frames (1 <= n <= 2^27); a frame is voiced when f0 > 0 (NaN: unvoiced).
 *   out_dev: double [12].  Over the frames voiced in BOTH, with la = log2 a, lb = log2 b, r = 1200 log2(b / a):
 *     [0] their count  [1] sum r  [2] sum la  [3] sum lb  [4] sum la^2  [5] sum lb^2  [6] sum la lb
 *     [7] sum (r - rbar)^2 and [8] the count of |r - rbar| > 1200 log2(1.2), rbar = [1] / [0] (a second pass in the same launch)
 *   [9] frames voiced in a alone  [10] in b alone  [11] in neither.  Every sum is 256 partial sums (frame mod 256) added in order.
 * All four are asynchronous on `hip_stream` and synchronise nothing. */
int rvc_melcep_workspace_bytes(int64_t n, int sr, size_t *bytes);
int rvc_melcep_f32(const float *x_dev, int64_t n, int sr, const float *mel_dev, int n_mels, int n_coef, float *out_dev,
                   void *workspace_dev, size_t workspace_bytes, void *hip_stream);
int rvc_dtw_workspace_bytes(int64_t Ta, int64_t Tb, size_t *bytes);
int rvc_dtw_f64(const float *a_dev, int64_t Ta, const float *b_dev, int64_t Tb, int dim, int64_t band, double *out_dev, int *path_dev,
                void *workspace_dev, size_t workspace_bytes, void *hip_stream);
int rvc_frame_dist_sum_f64(const float *a_dev, const float *b_dev, int64_t T, int dim, double *out_dev, void *hip_stream);
int rvc_f0_track_sums_f64(const double *f0_a_dev, const double *f0_b_dev, int64_t n, double *out_dev, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RVC_AMD_H */
