/* nbss_hip.h — C ABI of the MI355X-native SpatialNet hot path (libnbss_hip.so).
 *
 * The reference (Audio-WestlakeU/NBSS) is pure Python; its "plugin API" for this path is the
 * nn.Module contract `arch.forward([B,F,T,2C]) -> [B,F,T,2*Spk]` (SharedTrainer.py:117-122)
 * plus models/io/{stft,norm,loss}.py.  Every implicit ATen/cuDNN/cuBLAS/cuFFT kernel that
 * contract reaches is replaced by one entry point below; each comment cites the reference
 * site it stands in for.  Conventions:
 *   - plain pointers + sizes only, no torch types; all pointers are DEVICE pointers owned by
 *     the caller (no ownership transfer, no hidden allocation);
 *   - asynchronous on `stream` (a hipStream_t passed as void*); re-entrant, callable from any
 *     host thread (PyTorch's autograd thread calls the *_bwd entry points);
 *   - returns 0 on success, a negative NBSS_E* code otherwise; never throws or exits;
 *   - `dtype` = element type of the [B,F,T,H] residual stream and of the packed weights:
 *        NBSS_F32  fp32 stream, exact-f32 MFMA (v_mfma_f32_16x16x4_f32)
 *        NBSS_BF16 bf16 stream, bf16 MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate/statistics
 *     master parameters, gradients, STFT/iSTFT, loss and optimizer state are always fp32.
 */
#ifndef NBSS_HIP_H
#define NBSS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBSS_F32 0
#define NBSS_BF16 1

#define NBSS_OK 0
#define NBSS_EINVAL (-1)       /* bad argument */
#define NBSS_EUNSUPPORTED (-2) /* shape/config this build has no kernel for */
#define NBSS_ELAUNCH (-3)      /* HIP launch error */

/* SpatialNet hyper-parameters: models/arch/SpatialNet.py:154-171 (ctor) + batch geometry.
 * Geometries this build has kernels for (anything else: NBSS_EUNSUPPORTED):
 *   small  H 96,  FFN 192, SQ 8,  4 heads   (configs/SpatialNet.yaml:16-24)          forward + backward (fused training kernels)
 *   large  H 192, FFN 384, SQ 16, 4 heads   (the "for large" comments of that file)  forward + backward (geometry-generic backward, csrc/gbwd.hip:
 *                                                                                     one tensor pass per operation, every intermediate in ws)
 *   both with conv groups (8, 8), kernel sizes (5, 3), encoder kernel 5; C_in % 4 == 0, C_in / C_out <= 16.
 *   F <= 272 (n_fft 256 -> 129, n_fft 512 -> 257); fp32-stream backward of the small geometry: F <= 160 (F-conv block).
 *   T <= 256 for a forward that saves state and for every backward; forward without `acts`: T <= 4096. */
typedef struct nbss_cfg {
    int32_t B, F, T;         /* batch, frequencies (129 | 257), frames (251 for 4 s) */
    int32_t C_in, C_out;     /* dim_input (2*channels), dim_output (2*speakers) */
    int32_t H, FFN, SQ;      /* dim_hidden, dim_ffn, dim_squeeze */
    int32_t L, heads;        /* num_layers, num_heads */
    int32_t enc_ks;          /* encoder_kernel_size */
    int32_t f_ks, t_ks;      /* kernel_size = (f, t) */
    int32_t f_groups, t_groups; /* conv_groups = (f, t) */
    int32_t full_share;      /* layers > full_share reuse layer full_share's LinearGroup */
    int32_t dtype;           /* NBSS_F32 | NBSS_BF16 */
} nbss_cfg;

/* ---- parameter geometry ------------------------------------------------------------------
 * Parameters (and their gradients) live in ONE flat fp32 buffer; tensors appear in the
 * reference's state_dict order (SURVEY.md §8(b) checkpoint contract):
 *   encoder.weight, encoder.bias,
 *   per layer l: fconv1.0.{weight,bias} fconv1.1.{weight,bias} fconv1.2.weight
 *                norm_full.{weight,bias} squeeze.0.{weight,bias} full.{weight,bias}
 *                unsqueeze.0.{weight,bias} fconv2.0.* fconv2.1.* fconv2.2.weight
 *                norm_mhsa.{weight,bias} mhsa.in_proj_{weight,bias} mhsa.out_proj.{weight,bias}
 *                tconvffn.{0,1,3,5,6,8,10}.{weight,bias}
 *   decoder.weight, decoder.bias
 * A shared `full` keeps the owner's offset (numel still reported, so offsets may repeat).
 * nbss_param_table fills offsets[i] / numels[i] (in floats) and returns the entry count
 * (2 + 38*L + 2), or a negative error.  Pass NULL arrays to query the count only. */
int nbss_param_table(const nbss_cfg* cfg, int64_t* offsets, int64_t* numels, int max_entries);
int64_t nbss_param_count(const nbss_cfg* cfg);   /* floats in the flat buffer */

/* Packed MFMA weight fragments (+transposes for backward), rebuilt from the fp32 master
 * copy after every optimizer step.  bytes needed / repack. */
int64_t nbss_packed_bytes(const nbss_cfg* cfg);
int nbss_pack_params(const nbss_cfg* cfg, const float* params, void* packed, void* stream);

/* ---- SpatialNet sub-blocks, forward --------------------------------------------------------
 * x/y: residual stream [B,F,T,H] of cfg->dtype.  y may not alias x (x is what backward
 * re-reads).  `layer` selects the parameter slice. */

/* encoder nn.Conv1d(C_in,H,5,'same') along T (SpatialNet.py:175,205).  xin [B,F,T,C_in]. */
int nbss_encoder_fwd(const nbss_cfg* cfg, const float* params, const void* packed, const void* xin, void* y, void* stream);
/* decoder nn.Linear(H,C_out) (SpatialNet.py:200,216).  out [B,F,T,C_out] fp32. */
int nbss_decoder_fwd(const nbss_cfg* cfg, const float* params, const void* packed, const void* x, float* out, void* stream);
/* x + _fconv(fconv1|fconv2): LN -> grouped Conv1d along F -> PReLU (SpatialNet.py:85,87,116-127). which = 0|1 */
int nbss_fconv_fwd(const nbss_cfg* cfg, const float* params, const void* packed, int layer, int which, const void* x, void* y, void* stream);
/* x + _full: LN -> squeeze+SiLU -> LinearGroup over F -> unsqueeze+SiLU (SpatialNet.py:86,129-146). */
int nbss_full_fwd(const nbss_cfg* cfg, const float* params, const void* packed, int layer, const void* x, void* y, void* stream);
/* x + _tsa: LN -> nn.MultiheadAttention over T per (b,f) (SpatialNet.py:88,93-100).
 * o_save (optional, nbss_mhsa_save_bytes(cfg) bytes): what backward needs besides the block input — the attention output
 * before out_proj ([B,F,T,H] of cfg->dtype) followed by the fp32 log2-sum-exp of every (token, head) score row. */
int64_t nbss_mhsa_save_bytes(const nbss_cfg* cfg);
int nbss_mhsa_fwd(const nbss_cfg* cfg, const float* params, const void* packed, int layer, const void* x, void* y, void* o_save, void* stream);
/* x + _tconvffn (SpatialNet.py:90,102-114,61-73).
 * t_save (optional, nbss_tconvffn_save_bytes(cfg) bytes; that is 0 — pass NULL — for the geometries / stream types whose backward
 * kernel recomputes the chain itself): what a training-mode forward keeps for nbss_tconvffn_bwd — the bf16 outputs of the 1x1 conv and of
 * the three grouped T-convs (tconvffn.1 / .3 / .5 / .8 of SpatialNet.py:61-73, group-major), the LayerNorm statistics of every token
 * and the GroupNorm statistics of every (sequence, group). */
int64_t nbss_tconvffn_save_bytes(const nbss_cfg* cfg);
int nbss_tconvffn_fwd(const nbss_cfg* cfg, const float* params, const void* packed, int layer, const void* x, void* y, void* t_save, void* stream);

/* ---- SpatialNet sub-blocks, backward (autograd of the forward entry points) ------------------
 * x: the forward INPUT of the block (the only saved activation; everything else is recomputed
 * on chip), dy: gradient w.r.t. the block output, dx: gradient w.r.t. x (may not alias dy).
 * Parameter gradients are ACCUMULATED (+=) into `grads`, a flat fp32 buffer with the layout of
 * `params`; zero it at the start of a step.  `ws` is caller-provided scratch of at least
 * nbss_workspace_bytes(cfg) bytes (per-token LayerNorm statistics and the operands of the
 * weight-gradient contractions). */
int64_t nbss_workspace_bytes(const nbss_cfg* cfg);
/* t_save: the forward's saved state (see nbss_tconvffn_fwd), or NULL: the forward chain is recomputed from x (where
 * nbss_tconvffn_save_bytes(cfg) > 0 that costs one more forward launch: the saved state is rebuilt inside ws, then the same kernels run) */
int nbss_tconvffn_bwd(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, int layer, const void* x, const void* dy,
                      const void* t_save, void* dx, void* ws, void* stream);
int nbss_mhsa_bwd(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, int layer, const void* x, const void* dy,
                  const void* o_save, void* dx, void* ws, void* stream);
int nbss_fconv_bwd(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, int layer, int which, const void* x,
                   const void* dy, void* dx, void* ws, void* stream);
int nbss_full_bwd(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, int layer, const void* x, const void* dy,
                  void* dx, void* ws, void* stream);
/* decoder: x = decoder input stream, dout = fp32 gradient of the [B,F,T,C_out] output */
int nbss_decoder_bwd(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, const void* x, const float* dout, void* dx,
                     void* ws, void* stream);
/* encoder: weight/bias gradient only (the network input needs none); dy = gradient of the encoder output */
int nbss_encoder_bwd(const nbss_cfg* cfg, float* grads, const void* xin, const void* dy, void* stream);

/* ---- whole network (SpatialNet.forward, SpatialNet.py:202-220, and its autograd) ---------------
 * Native sequencing of the sub-block kernels: encoder, L x [fconv1, full, fconv2, mhsa, tconvffn],
 * decoder.  xin [B,F,T,C_in] of cfg->dtype, out/dout [B,F,T,C_out] fp32.
 * acts: nbss_acts_bytes() bytes holding the 5L+1 block inputs, the L attention outputs and the L T-ConvFFN
 * saves that backward re-reads; pass NULL for inference (then ws, >= nbss_workspace_bytes() + two [B,F,T,H] stream tensors, is used
 * as two ping-pong stream buffers behind one workspace).  Backward accumulates into `grads` and needs ws >= nbss_train_ws_bytes():
 * one workspace per sub-block kind of a layer + three gradient stream buffers — the walk launches everything that only produces
 * parameter gradients on a library-owned second stream (fork / done / join events; csrc/side.h), overlapping it with the next
 * sub-blocks' data-gradient kernels, and the copies keep those launches' operands alive.  When a backward call returns, the
 * caller's stream has been made to wait for that second stream: work enqueued on `stream` afterwards (the gradient all-reduce,
 * the optimizer) sees every gradient of the range.  NBSS_SIDE_STREAM=0 in the environment keeps everything on `stream`. */
int64_t nbss_acts_bytes(const nbss_cfg* cfg);
int64_t nbss_train_ws_bytes(const nbss_cfg* cfg);
int nbss_spatialnet_fwd(const nbss_cfg* cfg, const float* params, const void* packed, const void* xin, void* acts, void* ws, float* out,
                        void* stream);
int nbss_spatialnet_bwd(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, const void* xin, const void* acts,
                        const float* dout, void* ws, void* stream);
/* The same walk in pieces, for overlapping the data-parallel gradient exchange with backward (the role of DDP's reverse-order
 * buckets): layers [layer_lo, layer_hi), plus the decoder when layer_hi == L (dout needed only then) and the
 * encoder when layer_lo == 0.  Calls must cover L..0 in descending, adjacent ranges; after a call the gradients of the layers
 * it covered are final, except the LinearGroup shared through full_share, which is final after layer 0. */
/* Threading: the walks share ONE set of library-owned streams and events per process (csrc/capi.hip: SideState) — one walk at a time per
 * process (the one-process-per-GPU model of this library); concurrent walks from several host threads or engines are not supported.  Under
 * HIP-graph capture of `stream` the walks stay in order on it. */
int nbss_spatialnet_bwd_range(const nbss_cfg* cfg, const float* params, float* grads, const void* packed, const void* xin, const void* acts,
                              const float* dout, void* ws, int layer_hi, int layer_lo, void* stream);

/* ---- signal front / back end (always fp32 arithmetic) ------------------------------------------
 * n_fft in {256, 512}, hop = n_fft/2, win_len = n_fft; window 0 = periodic hann, 1 = sqrt-hann
 * (models/io/stft.py:23-35).  `tables` = windowed DFT matrices packed as MFMA fragments, built once
 * per (n_fft, window) into caller memory of nbss_stft_tables_bytes() bytes. */
int64_t nbss_stft_tables_bytes(int n_fft);
int nbss_stft_tables(int n_fft, int window, float* tables, void* stream);
/* STFT.stft (stft.py:49-66) + Norm('frequency', online=True).norm (norm.py:77-81,94) + the
 * [B,C,F,T] complex -> [B,F,T,2C] real re-layout of TrainModule.forward (SharedTrainer.py:113-117).
 * x [B,C,N] fp32 -> X [B,F,T,2C] of `dtype` (T = N/hop + 1), xrmm [B,F,T] fp32 = |X_ref| + 1e-6.
 * N is unrestricted apart from N >= n_fft (NBSS_EINVAL below that): rows of x that do not start on a
 * 16-byte boundary (N % 4 != 0) are read sample by sample, aligned rows with 16-byte loads. */
int nbss_stft_norm_fwd(int n_fft, int dtype, int B, int C, int N, int ref_channel, const float* tables, const float* x, void* X, float* xrmm,
                       void* stream);
/* Norm.inorm (norm.py:97-108) + STFT.istft (stft.py:68-97): out [B,F,T,2S] fp32 -> y [B,S,N].
 * ws: nbss_istft_ws_bytes() bytes of scratch (overlap-add buffer). */
int64_t nbss_istft_ws_bytes(int n_fft, int B, int S, int N);
int nbss_inorm_istft_fwd(int n_fft, int B, int S, int N, const float* tables, const float* out, const float* xrmm, float* ws, float* y,
                         void* stream);
/* adjoint: dy [B,S,N] -> dout [B,F,T,2S] */
int nbss_inorm_istft_bwd(int n_fft, int B, int S, int N, const float* tables, const float* dy, const float* xrmm, float* dout, void* stream);

/* Loss(neg_si_sdr, pit=True).forward (models/io/loss.py:21-29,95-118; torchmetrics si_sdr + pit
 * 'permutation-wise'/'min').  preds/target [B,S,N] fp32.  loss: 1 float (mean over the batch),
 * perm [B,S] (prediction index paired with target s), dpreds (optional) = d loss / d preds.
 * ws: nbss_pit_ws_bytes() bytes. */
int64_t nbss_pit_ws_bytes(int B, int S);
int nbss_pit_neg_sisdr(int B, int S, int N, const float* preds, const float* target, float* loss, int32_t* perm, float* dpreds, float* ws,
                       void* stream);

/* Loss(loss_func, pit).forward for the reference's other objectives (models/io/loss.py:15-71,95-118; torchmetrics snr,
 * source_aggregated_signal_distortion_ratio, pit 'permutation-wise'/'min'; zero_mean=False, eps = float32 epsilon):
 *   NBSS_LOSS_SI_SDR  -mean_s si_sdr(p_s, t_s)                         (neg_si_sdr, as nbss_pit_neg_sisdr)
 *   NBSS_LOSS_SNR     -mean_s 10 log10((|t_s|^2 + eps) / (|t_s - p_s|^2 + eps))           (neg_snr)
 *   NBSS_LOSS_SA_SDR  -10 log10((sum_s |t_s|^2 + eps) / (sum_s |t_s - p_s|^2 + eps))     (neg_sa_sdr; with
 *                     NBSS_LOSS_SCALE_INVARIANT the targets are first scaled by (sum_s <p_s,t_s> + eps) / (sum_s |t_s|^2 + eps))
 *   NBSS_LOSS_MSE     mean over S*N elements of (p - t)^2                                 (cc_mse / _mse)
 * flags: NBSS_LOSS_PIT = minimum over the speaker permutations in itertools order (first wins a tie); clear = estimate s
 * paired with target s.  NBSS_LOSS_SCALE_INVARIANT: SA-SDR only (NBSS_EINVAL with another kind).
 * preds/target [B,S,N] fp32, N = any flattened trailing size; S <= 4, B <= 1024 (NBSS_EUNSUPPORTED beyond).
 * loss: 1 float (mean over the batch), perm [B,S] (prediction index paired with target s), dpreds (optional) = d loss / d preds.
 * The distortion energies |t - p|^2 of SNR, unscaled SA-SDR and MSE are accumulated element-wise, not formed from dot products.
 * ws: nbss_pit_loss_ws_bytes() bytes of floats = partial sums | per-item loss [B] | pairing coefficients [3 B S]; the caller may
 * read the per-item losses from that tail after the call (nbss_pit_ws_bytes() has the same tail). */
#define NBSS_LOSS_SI_SDR 0
#define NBSS_LOSS_SNR 1
#define NBSS_LOSS_SA_SDR 2
#define NBSS_LOSS_MSE 3
#define NBSS_LOSS_PIT 1
#define NBSS_LOSS_SCALE_INVARIANT 2
int64_t nbss_pit_loss_ws_bytes(int kind, int B, int S);
int nbss_pit_loss(int kind, int flags, int B, int S, int N, const float* preds, const float* target, float* loss, int32_t* perm, float* dpreds,
                  float* ws, void* stream);

/* ---- evaluation metrics (csrc/metrics.hip) -------------------------------------------------------------------------------------------------
 * What the reference's validation and test steps compute on the device (SharedTrainer.py:163-182,239-248 through
 * models/utils/metrics.py:14-151: torchmetrics signal_noise_ratio, scale_invariant_signal_distortion_ratio, scale_invariant_signal_noise_ratio,
 * signal_distortion_ratio) and its recover_scale (models/utils/metrics.py:192-218).  preds / target [B,S,N] fp32, estimate s paired with target s;
 * S <= 4, B <= 1024 (NBSS_EUNSUPPORTED beyond).  Every sum is accumulated in fp64 in a fixed order, no atomics: two calls give the same bits.
 *
 * nbss_signal_ratios: out [B][S][3] fp32 = SNR, SI-SDR, SI-SNR in dB, one pass over the signals; eps = float32 epsilon:
 *   SNR    10 log10((|t|^2 + eps) / (|t - p|^2 + eps)), the distortion accumulated element by element          (metrics.py:79-81)
 *   SI-SDR alpha = (<p,t> + eps) / (|t|^2 + eps); 10 log10((|alpha t|^2 + eps) / (|alpha t - p|^2 + eps))       (metrics.py:73-75)
 *   SI-SNR SI-SDR of the two signals minus their means                                                         (metrics.py:76-78)
 * ws: nbss_signal_ratios_ws_bytes() bytes. */
int64_t nbss_signal_ratios_ws_bytes(int B, int S);
int nbss_signal_ratios(int B, int S, int N, const float* preds, const float* target, float* out, void* ws, void* stream);
/* nbss_sdr: torchmetrics signal_distortion_ratio(preds, target, filter_length, zero_mean) (metrics.py:66-69; SharedTrainer.py:167: `sdr`), BSS-eval
 * with a distortion filter of filter_length taps, fp64 from the first step on: t / max(|t|, 1e-6), p / max(|p|, 1e-6); r[k] = sum_n t[n] t[n+k],
 * b[k] = sum_n t[n] p[n+k] (linear correlations, k < filter_length); Toeplitz(r) x = b by Levinson-Durbin; coh = <b, x>;
 * sdr [B][S] fp32 = 10 log10(coh / (1 - coh)).  flags: NBSS_SDR_ZERO_MEAN subtracts each signal's mean first (torchmetrics' default is off).
 * 1 <= filter_length <= 512 (torchmetrics' default) and N >= filter_length, else NBSS_EUNSUPPORTED.  A silent target or estimate gives NaN, as it does there.
 * ws: nbss_sdr_ws_bytes() bytes. */
#define NBSS_SDR_ZERO_MEAN 1
int64_t nbss_sdr_ws_bytes(int B, int S, int N, int filter_length);
int nbss_sdr(int B, int S, int N, int filter_length, int flags, const float* preds, const float* target, float* sdr, void* ws, void* stream);
/* nbss_recover_scale: recover_scale(preds, mixture, scale_src_together, norm_if_exceed_1) (metrics.py:192-218; SharedTrainer.py:239-242): preds
 * [B,S,N], mixture [B,N] -> out [B,S,N] = a_s preds_s with the least-squares scales a [S] of min |sum_s a_s p_s - x| per utterance, from the normal
 * equations (S x S Gram matrix and right-hand side accumulated and solved in fp64); NBSS_SCALE_TOGETHER: one scale for sum_s p_s.
 * NBSS_SCALE_NORM_IF_EXCEED_1: a source whose scaled maximum magnitude exceeds 1 is divided by it.  The result is defined only when the Gram matrix
 * is non-singular (linearly independent estimates; with NBSS_SCALE_TOGETHER: a non-zero sum) — otherwise it is inf / NaN, no error is raised.
 * out may not alias preds.  ws: nbss_recover_scale_ws_bytes() bytes; its last B S doubles hold the applied scales after the call. */
#define NBSS_SCALE_TOGETHER 1
#define NBSS_SCALE_NORM_IF_EXCEED_1 2
int64_t nbss_recover_scale_ws_bytes(int B, int S);
int nbss_recover_scale(int B, int S, int N, int flags, const float* preds, const float* mixture, float* out, void* ws, void* stream);

/* ---- STOI and extended STOI (csrc/stoi.hip) --------------------------------------------------------------------------------------------------
 * Short-time objective intelligibility (Taal et al., 2011) and extended STOI (Jensen & Taal, 2016), what the reference's test step takes from
 * torchmetrics -> pystoi (a package this port does not use; parity with it is not pinned, this comment is the definition).
 * Per pair (estimate y, clean x), both of N samples at rate fs.  EPS = 2^-52.
 * 1. Resample to 10 kHz.  fs in {8000, 10000, 16000} (NBSS_EUNSUPPORTED otherwise); p/q = 5/4 for 8000, 5/8 for 16000, none for 10000.
 *    Taps: fc = 1 / (2 max(p, q)), L = ceil((60 - 8) / (28.714 fc / 10)), t = -L .. L,
 *    h = kaiser(2 L + 1, beta = 0.1102 (60 - 8.7)) 2 p fc sinc(2 fc t), then h <- p h / sum(h): 365 taps for 5/4, 581 for 5/8.
 *    Output sample m = sum_k h[m q - k p + L] x[k], zeros outside the signal; ceil(N p / q) output samples
 *    (scipy.signal.resample_poly(x, p, q, window=h / p)).
 * 2. Silent-frame removal.  w = hanning(258)[1:-1]; frames of 256 samples starting at 0, 128, ... < len - 256 (the last candidate start is excluded
 *    when len - 256 is a multiple of 128).  E_k = 20 log10(|w x_k| + EPS) of clean frame k; frame k is kept iff E_k > max_k E - 40.  The windowed
 *    kept frames of x are overlap-added at hop 128, in order; the frames of y use the same mask, from x alone.  K kept frames leave signals of
 *    128 (K - 1) + 256 samples.
 * 3. Spectra.  Frames of the compacted signals: 256 samples at hop 128, starts < len - 256 again: K - 1 frames.  Each is multiplied by w, then a
 *    real DFT of 512 points (zero-padded) gives 257 bins.
 * 4. One-third-octave bands.  15 bands, centres 150 2^(k/3), edges 150 2^((2 k -+ 1) / 6); bin grid f_j = j 10000 / 512.  Band k sums |X_j|^2 over
 *    j in [argmin_j (f_j - low_k)^2, argmin_j (f_j - high_k)^2); the band value is the square root of that sum: X, Y [15, K - 1].
 * 5. Segments.  All runs of 30 consecutive frames: M = K - 30 segments.  If K - 1 < 30 the result is 1e-5 and the call does not fail.
 * 6. STOI (flag clear).  Per segment and band: alpha = |X| / (|Y| + EPS), norms over the 30 frames; Y' = min(alpha Y, X (1 + 10^(15/20)));
 *    d = <X - mean(X), Y' - mean(Y')> / ((|X - mean(X)| + EPS) (|Y' - mean(Y')| + EPS)).  The result is the mean of d over segments and bands.
 * 7. eSTOI (NBSS_STOI_EXTENDED).  Per segment, each band row of X and Y has its mean over time subtracted and is divided by (its norm + EPS); each
 *    frame column then has its mean over bands subtracted and is divided by (its norm + EPS).  The result is sum(X~ Y~) / (30 M).
 * preds / target [B,S,N] fp32, estimate s paired with target s -> out [B][S] fp32.  S <= 4, B <= 1024, N <= 2^24 and at least 257 resampled samples,
 * else NBSS_EUNSUPPORTED.  The resampler accumulates in fp64, the spectra are fp32 (matrix cores), steps 2 and 5 - 7 are fp64.  No atomics, every
 * element of out is written once, two calls give the same bits, an item's value does not depend on the other items of the batch.
 * ws: nbss_stoi_ws_bytes() bytes (negative: the error code); its first 2 L + 1 doubles hold the taps h after the call. */
#define NBSS_STOI_EXTENDED 1
int64_t nbss_stoi_ws_bytes(int B, int S, int N, int fs);
int nbss_stoi(int B, int S, int N, int fs, int flags, const float* preds, const float* target, float* out /*[B][S]*/, void* ws, void* stream);

/* ---- Room impulse responses by the image-source method (csrc/rir.hip; nbss_amd/rir.py: simulate_rir) -----------------------------------------
 * What the reference's generate_rirs.py takes from gpuRIR (a CUDA-only package; parity with it is not pinned, this comment is the definition):
 * Allen & Berkley's image sources of a shoebox room with the Hann-windowed sinc of fractional delay.  Per room b of the batch:
 *   room_sz [B][3], beta [B][6] = (x0, x1, y0, y1, z0, z1) wall reflection coefficients, pos_src [B][S][3], pos_rcv [B][M][3]: fp64 DEVICE arrays;
 *   nb_img [B][3] = (Nx, Ny, Nz): int32 HOST array, read before the call returns.
 * Along axis a the image index is n = i - floor(N_a / 2), i = 0 .. N_a - 1; the image coordinate is n L_a + s_a (n even) or (n + 1) L_a - s_a (n odd);
 * wall 0 reflects floor(n / 2) times for n >= 0 and ceil(|n| / 2) times for n < 0, wall 1 ceil(n / 2) resp. floor(|n| / 2) times.
 *   A = prod_a beta_a0^r_a0 beta_a1^r_a1 / (4 pi d)   (0^0 = 1),  d = max(|image - receiver|, 1e-3 m),  x = fs d / c
 *   h[b][s][m][k] = sum_images A w(k - x),   w(u) = 0.5 (1 + cos(2 pi u / (tw fs))) sinc(u) for |u| < tw fs / 2, else 0
 * Position, distance, x and its split into integer and fraction are fp64, the window fp32, the sum over the images fp64 in an order fixed by the
 * room, (s, m) and k alone: two calls give the same bits and a room's response does not depend on the other rooms of the batch.  No atomics.
 * h [B][S][M][n_samples] fp32: every element is written exactly once.
 * k_d > 0: only images with x < k_d + round(tw fs) / 2 are summed (the early part in front of nbss_rir_tail); k_d = 0: all of them.
 * Limits (NBSS_EUNSUPPORTED outside): 1 <= N_a <= 512; 1 <= n_samples <= 65536; 2 <= tw fs and tw fs + 1 <= 257; B, S, M >= 1 (B, S M <= 65535);
 * with k_d > 0: round(tw fs) <= k_d < n_samples.
 * ws: nbss_rir_ism_ws_bytes() bytes (exact: B headers and one fp64 wall factor per room, axis and image index; NBSS_EINVAL when ws_bytes is less;
 * the count is negative when an N_a is outside its limits). */
int64_t nbss_rir_ism_ws_bytes(int B, const int32_t* nb_img);
int nbss_rir_ism(int B, int S, int M, int n_samples, double fs, double c, double tw, int k_d, const double* room_sz, const double* beta,
                 const double* pos_src, const double* pos_rcv, const int32_t* nb_img, float* h, void* ws, int64_t ws_bytes, void* stream);
/* The diffuse tail behind nbss_rir_ism(k_d > 0), this project's own definition: with K = round(tw fs), g^2 = mean_{k_d - K <= k < k_d} h[b][s][m][k]^2
 * (fp64, index order), for k >= k_d
 *   h[b][s][m][k] = g 10^(-3 (k - k_d) / (fs rt60[b])) xi(seed, b, s, m, k)
 * xi: z(v) = splitmix64 step (v += 0x9E3779B97F4A7C15; v = (v ^ v >> 30) 0xBF58476D1CE4E5B9; v = (v ^ v >> 27) 0x94D049BB133111EB; v ^ v >> 31),
 * key = z(z(z(seed + b) + s) + m), h1 = z(key + k), h2 = z(h1), u1 = ((h1 >> 41) + 1) / 2^23, u2 = (h2 >> 40) / 2^24,
 * xi = sqrt(-2 ln u1) cos(2 pi u2), evaluated in fp64: the tail does not depend on the launch geometry.  rt60 [B] fp64 device array.
 * Same limits as nbss_rir_ism with k_d > 0. */
int nbss_rir_tail(int B, int S, int M, int n_samples, double fs, double tw, int k_d, const double* rt60, int64_t seed, float* h, void* stream);
/* The same two with the switch to the tail per room (a batch draws RT60 per room, so att2t(15 dB, rt60[b]) differs from room to room):
 * k_d [B]: int32 HOST array, read before the call returns, like nb_img.
 * nbss_rir_ism_rooms: room b sums only the images with x < k_d[b] + round(tw fs) / 2 when k_d[b] > 0, all of them when k_d[b] = 0.  Everything said of
 * nbss_rir_ism holds: every element of h is written exactly once, no atomics, the order of the sum is fixed by the room, (s, m) and k alone, and a
 * room's response does not depend on the other rooms of the batch — room b is BITWISE what nbss_rir_ism gives for that room with k_d = k_d[b].
 * The limits are those of nbss_rir_ism per room: a room with 0 < k_d[b] < round(tw fs) or k_d[b] >= n_samples makes the call return NBSS_EUNSUPPORTED
 * (a negative k_d[b] NBSS_EINVAL) before anything is launched.  ws: nbss_rir_ism_ws_bytes() bytes, the same layout: the k_d travel in the kernel's
 * arguments, 256 rooms per launch.
 * nbss_rir_tail_rooms: room b gets the tail of nbss_rir_tail's definition from k_d[b] on (the same xi(seed, b, s, m, k): bitwise nbss_rir_tail with
 * k_d = k_d[b]); a room with k_d[b] = 0 is not touched.  Same limits per room. */
int nbss_rir_ism_rooms(int B, int S, int M, int n_samples, double fs, double c, double tw, const int32_t* k_d, const double* room_sz, const double* beta,
                       const double* pos_src, const double* pos_rcv, const int32_t* nb_img, float* h, void* ws, int64_t ws_bytes, void* stream);
int nbss_rir_tail_rooms(int B, int S, int M, int n_samples, double fs, double tw, const int32_t* k_d, const double* rt60, int64_t seed, float* h,
                        void* stream);

/* ---- RIR convolution of the on-device simulator (csrc/conv1d.hip; data_loaders/gpu_simulation.py: convolve_aligned_native) ---------------------
 * What the reference's convolve(wav, rir, rir_target, ref_channel, align=True) keeps of its full convolutions (utils/mix.py:122-134): the N samples
 * from the direct-path delay of the reference channel onward.
 * nbss_rir_delay: h [B][S][M][L] fp32 -> delay [B][S] int32 = the index of the maximum of h[b][s][ref_channel][:] (mix.py:130, np.argmax); on a tie
 * the LOWEST index wins.  A row that holds a NaN has no defined maximum (the call does not fail).  0 <= ref_channel < M, else NBSS_EINVAL.
 * nbss_fir_convolve: x [B][S][N], h [B][S][M][L] fp32, delay [B][S] int32 (a DEVICE array) -> y [B][S][M][N] fp32,
 *   y[b][s][m][n] = sum_{k < L} h[b][s][m][k] x[b][s][n + delay[b][s] - k],   terms whose x index lies outside [0, N) are zero
 * (mix.py:127,133: fftconvolve(mode='full')[delay : delay + N]); only this window of the linear convolution is formed.  A direct convolution on
 * the exact-fp32 matrix cores: every product is rounded once, the sum is an fp32 fmaf chain in an order fixed by n and L alone.  No atomics: two
 * calls give the same bits, and an item's result does not depend on the batch.  Any N >= 1 and L >= 1; rows on 16-byte boundaries (N % 4 == 0,
 * L % 4 == 0, base pointers aligned) are read with 16-byte loads, any other shape element by element.
 * The delays are validated on the device: one outside [0, L) is clamped into that range and `status` (one int32 on the device, or NULL; the caller
 * zeroes it) is set to 1; the call itself returns 0, and the caller who reads a non-zero status treats the result as NBSS_EINVAL (ops.fir_convolve).
 * NBSS_EINVAL: N < 1, L < 1.  Limits (NBSS_EUNSUPPORTED outside): L <= 65536 (the longest response nbss_rir_ism writes), N <= 2^24, M <= 4096,
 * B S M <= 2^22; B, S, M >= 1.  The kernel's LDS image (2048 taps of 3 microphones and the matching strip of x: 48 KB) does not grow with L, and
 * (b, s) pairs beyond 2048 are walked by the same grid.  y may not alias x or h.  No workspace. */
int nbss_rir_delay(int B, int S, int M, int L, int ref_channel, const float* h, int32_t* delay, void* stream);
int nbss_fir_convolve(int B, int S, int M, int N, int L, const float* x, const float* h, const int32_t* delay, float* y, int32_t* status, void* stream);

/* ---- RIR convolution along a trajectory: moving sources (csrc/conv_traj.hip; data_loaders/gpu_simulation.py: convolve_traj_aligned) -------------
 * nbss_fir_convolve_traj: x [B][S][N] dry sources, h [B][S][P][M][L] one RIR set per trajectory point, hop [B][S] int32 (a DEVICE array: source
 * samples per trajectory point), delay [B][S] int32 (a DEVICE array, as nbss_fir_convolve's) -> y [B][S][M][N], all fp32.  For item (b, s) let
 * H = hop[b][s], d = delay[b][s], and for a source sample j in [0, N) q = j / H, r = j % H.  x[j] is heard through at most two RIRs:
 *   mode 0 (switch; the reference's convolve_traj with an integer samples_per_rir, utils/mix.py:151-194): RIR q with weight 1;
 *   mode 1 (trapezium; convolve_traj_with_win(..., 'trapezium{ramp}'), mix.py:197-244): RIR q with weight down(r) and RIR q + 1 with weight up(r),
 *     with z = (H - ramp) / 2 (floor) and o = H - ramp - z:
 *     up(r)   = 0 for r < z;  (r - z) / (ramp - 1) for z <= r < z + ramp;  1 from there on,
 *     down(r) = 1 for r < o;  (ramp - 1 - (r - o)) / (ramp - 1) for o <= r < o + ramp;  0 from there on.
 * With the weights w_p(j) so defined,
 *   y[b][s][m][n] = sum_{k < L} sum_p w_p(j) h[b][s][p][m][k] x[b][s][j],   j = n + d - k,   terms with j outside [0, N) are zero:
 * full[:, d : d + N] of the reference functions (chime3_moving.py:204, mix.py:247-252).  Mode 1 with N < H is defined by the same closed form.
 * Required P: mode 0 ceil(N / H); mode 1 ceil((N + H - 1) / H) (the reference's len(range(0, N + hop - 1, hop))).  With that many, an index >= P is
 * reached only with weight 0 (up(0) = 0) and is NOT read; more RIRs than required are allowed and are never read.
 * A direct convolution on the exact-fp32 matrix cores, one pass per trajectory point that an output tile of 256 samples can hear: x w_p is rounded
 * once to fp32, and its product with a tap is fused into the fp32 fmaf chain, so every product of the sum is rounded once; the order of an output's
 * sum is fixed by n, L, H and d of its item alone.  No atomics, every output is stored exactly once, two calls give the same bits, an item's result
 * does not depend on the batch it shares a launch with, and there is no workspace.  Rows on 16-byte boundaries (N % 4 == 0, L % 4 == 0, base
 * pointers aligned) are read with 16-byte loads, any other shape element by element.
 * The items are validated on the device: an item with H < 1, in mode 1 with H <= ramp or ramp < 2, or with a P too small for its H gets zeros in y;
 * a delay outside [0, L) is clamped into that range, as by nbss_fir_convolve.  In both cases `status` (one int32 on the device, or NULL; the caller
 * zeroes it) is set to 1; the call itself returns 0, and the caller who reads a non-zero status treats the result as NBSS_EINVAL
 * (ops.fir_convolve_traj).  In mode 0 `ramp` is ignored.
 * NBSS_EINVAL: N < 1, L < 1, P < 1, mode outside {0, 1}.  Limits (NBSS_EUNSUPPORTED outside): those of nbss_fir_convolve applied to the B S P M
 * rows of h: L <= 65536, N <= 2^24, M <= 4096, B S P M <= 2^22; B, S, M >= 1.  The kernel's LDS image (39 KB) does not grow with L, H or P, and
 * (b, s) pairs beyond 2048 are walked by the same grid.  y may not alias x or h. */
int nbss_fir_convolve_traj(int B, int S, int P, int M, int N, int L, int mode, int ramp, const float* x, const float* h, const int32_t* hop,
                           const int32_t* delay, float* y, int32_t* status, void* stream);

/* ---- Spatially diffuse noise of the on-device simulator (csrc/diffuse.hip; data_loaders/gpu_simulation.py: gen_diffuse_noise_native) ------------
 * nbss_diffuse_noise: white [B][M][N] fp32 (M mutually independent noises per item), Cs [F][M][M][2] fp32 (complex, interleaved re / im, shared by
 * the batch; F = nfft / 2 + 1) -> noise [B][M][N] fp32 with the coherence the mixing matrices encode (utils/diffuse_noise.py:64-93).  For item b,
 * with hop = nfft / 4 and w the periodic Hann window of length nfft:
 *   1. v[m][.] = white[b][m][.] - its mean over the N samples (the mean is summed, and subtracted, in fp64).
 *   2. v is padded with nfft / 2 zeros on each side, then with zeros on the right up to the next length Np for which (Np - nfft) is a multiple of
 *      hop; T = (Np - nfft) / hop + 1 frames, frame t covers the padded samples [t hop, t hop + nfft).
 *   3. Nf[m][f][t] = sum_j w[j] frame_t[m][j] e^(-2 pi i f j / nfft).  (The 1 / sum w of scipy's forward transform cancels against its inverse.)
 *   4. X[n][f][t] = sum_m conj(Cs[f][m][n]) Nf[m][f][t]: the output channel is the LAST index of Cs.
 *   5. g_t[n][j] = w[j] irfft(X[n][.][t])[j], the real inverse of length nfft with its 1 / nfft; the imaginary parts of bins 0 and nfft / 2 are
 *      ignored, as torch.fft.irfft ignores them.
 *   6. The g_t are overlap-added at hop spacing, and the padded sample p is divided by max(sum_t w^2[p - t hop], 1e-10) over the frames that cover
 *      it: near both ends fewer than four do, and the envelope is formed from those that exist.
 *   7. noise[b][n][i] is the padded sample i + nfft / 2, i in [0, N).
 * Both transforms are DFT-as-GEMM on the exact-fp32 matrix cores, fused with the mix and the overlap-add in one kernel: white is read once and noise
 * written once.  No atomics; the order of every sum is fixed by N and M alone: two calls give the same bits, and an item's result depends neither on
 * B nor on its position in the batch.  Rows are read and written element by element: any N >= 1, no alignment demanded.  noise may not alias white.
 * ws: nbss_diffuse_noise_ws_bytes(B, M) bytes (8-byte aligned): the packed windowed DFT matrices (525 312 bytes, rewritten by every call) and the
 * B M row means in fp64; the count is negative for B < 1 or M < 1.
 * NBSS_EINVAL: N < 1, B < 1, M < 1, a NULL pointer (ws included), noise overlapping white.  NBSS_EUNSUPPORTED: nfft other than 256 (the only size
 * the simulator and the reference use), M > 16, N > 2^24, B M > 2^22.  A workgroup owns 832 output samples of all M channels of one item; its LDS
 * image (the strip of 19 hops of every channel with the mean removed, later the overlap-add image, and the mixed spectra of four row tiles) is
 * 9 264 M bytes: 54.3 KB at M = 6, 144.8 KB at M = 16.  Items beyond 128 are walked by the same grid. */
int64_t nbss_diffuse_noise_ws_bytes(int B, int M);
int nbss_diffuse_noise(int nfft, int B, int M, int N, const float* white, const float* Cs, float* ws, float* noise, void* stream);

/* clip_grad_norm_(max_norm, L2) + torch.optim.Adam(W) step on the flat fp32 buffers
 * (configs/SpatialNet.yaml:3-4,44; general_steps.py:243-271).  grads are first multiplied by
 * grad_scale (1/world_size after a SUM all-reduce).  scratch: >= 258 floats; scratch[0] returns the
 * (scaled) gradient norm.  step counts from 1.  flags: bit 0 clears grads for the next step; bit 1 selects
 * torch.optim.AdamW's decoupled weight decay (p *= 1 - lr*wd) instead of torch.optim.Adam's L2 term in the gradient. */
int nbss_clip_adam_step(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* scratch, float max_norm,
                        float grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay, int step, int flags,
                        void* stream);

/* The same update for HIP-graph replay (nbss_amd/engine.py: TrainStep.graph_step; the reference's per-step host work is Lightning's optimizer
 * loop, general_steps.py:243-271): the per-step scalars are read from the DEVICE buffer hyper[3] = {lr, 1 - beta1^step, sqrt(1 - beta2^step)},
 * which nbss_adam_hyper fills on the HOST (hyper_host: 3 floats of host memory, copied to the device by the caller before the replay) with the
 * very expressions nbss_clip_adam_step evaluates — a replayed step is bitwise the eager one. */
int nbss_clip_adam_step_dev(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* scratch, const float* hyper, float max_norm,
                            float grad_scale, float beta1, float beta2, float eps, float weight_decay, int flags, void* stream);
int nbss_adam_hyper(int step, float lr, float beta1, float beta2, float* hyper_host);

/* ---- OnlineSpatialNet: native streaming step (models/arch/OnlineSpatialNet.py:22-60,171-200,333-354; base/retention.py:194-253) -------
 * One call advances a chunk of C <= 32 frames of every (batch, frequency) sequence; all state lives in caller-owned fp32 device
 * buffers updated in place, so a whole step is a fixed launch sequence (capturable in a HIP graph).  fp32; geometry: dim_hidden 96,
 * dim_ffn 192, 8 conv groups of 24, 4 retention heads (key 24, value 48).  The cross-band blocks of a layer are per-frame operations:
 * nbss_fconv_fwd / nbss_full_fwd on the [B,F,C,H] chunk (cfg->T = C); the decoder: nbss_decoder_fwd.
 * encoder: causal Conv1d(C_in -> 96, k = 5): x [BF][C][C_in], state [BF][4][C_in] (the last four input frames), y [BF][C][96]. */
int nbss_online_encoder_step(int BF, int C, int C_in, const float* weight, const float* bias, const float* x, float* state, float* y, void* stream);
/* x += out_proj(SiLU(g) * RMSNorm_head(retention(q, k, v))) with LayerNorm(x) as input, recurrent form: kv [BF][4][24][48] and
 * scale [BF][4] (running decay sum, one copy per sequence) carry over; w*_t are the projection weights TRANSPOSED ([in][out]);
 * wk_t = NULL shares k with q ('ret(2,share_qk)'); decay [4] = the per-head gamma.  x [BF][C][96] in place. */
int nbss_online_ret_step(int BF, int C, const float* ln_w, const float* ln_b, const float* wq_t, const float* wk_t, const float* wv_t, const float* wg_t,
                         const float* wo_t, const float* decay, float* kv, float* scale, float* x, void* stream);
/* 'mhsa(N)': x += out_proj(causal windowed attention over the last `scope` frames) with LayerNorm(x) as input.  kring / vring [BF][ring][96]: the projected
 * keys / values of the last frames at slot (frame index mod ring), ring >= scope - 1 + C; pos[0] (device int32): frames seen before this chunk — every layer's
 * call of a step reads it, nbss_online_advance adds C once at the end of the step.  win_t [96][288] / wo_t [96][96]: in_proj / out_proj weights transposed. */
int nbss_online_mhsa_step(int BF, int C, int scope, int ring, const float* ln_w, const float* ln_b, const float* win_t, const float* bin, const float* wo_t,
                          const float* bo, float* kring, float* vring, const int32_t* pos, float* x, void* stream);
int nbss_online_advance(int32_t* pos, int C, void* stream);
/* 'mamba(16,4)': x += out_proj(y * SiLU(z)) with (xr, z) = in_proj(LayerNorm(x)) and y the selective scan of xr (models/arch/base/mamba.py: Mamba.step) for
 * d_model 96, expand 2, d_state 16, d_conv 4, dt_rank 6; no bias on in_proj, x_proj, out_proj.  win_t [96][384], xproj_t [192][38] (6 dt_r | 16 B | 16 C),
 * wo_t [192][96]: in_proj / x_proj / out_proj weights transposed; conv_w [192][4], conv_b [192], dtproj_w [192][6], dtproj_b [192], a_log [192][16], d [192]:
 * the module's own layouts.  conv_state [BF][3][192]: the last three inputs of the convolution, oldest first; ssm_state [BF][16][192]: h, state-major.  Both
 * are zeros for an empty stream (the transposes of Mamba.init_state's tensors).  x [BF][C][96] in place.  NBSS_EUNSUPPORTED for C > 32. */
int nbss_online_mamba_step(int BF, int C, const float* ln_w, const float* ln_b, const float* win_t, const float* conv_w, const float* conv_b,
                           const float* xproj_t, const float* dtproj_w, const float* dtproj_b, const float* a_log, const float* d, const float* wo_t,
                           float* conv_state, float* ssm_state, float* x, void* stream);
/* x += causal T-ConvFFN(x): LayerNorm -> 1x1 -> SiLU -> causal gconv -> SiLU -> causal gconv -> GroupNorm of each FRAME over (24 channels
 * x all F frequencies) -> SiLU -> causal gconv -> SiLU -> 1x1.  w1_t [96][192], w2_t [192][96] transposed; conv weights [192][24][3];
 * s1 s2 s3 [BF][2][192] = the last two input frames of the three convs; a3 [BF][C][192] and gn_sums [B + BF][C][8][2] (the per-frame
 * GroupNorm statistics (mean, sum of squared deviations from it), then every frequency's own pair over its 24 channels: combined in
 * frequency order, no atomics — bitwise repeatable; formed from deviations only, so good for any |mean| / std) are scratch. */
int nbss_online_tconvffn_step(int B, int F, int C, const float* ln_w, const float* ln_b, const float* w1_t, const float* b1, const float* c1w,
                              const float* c1b, const float* c2w, const float* c2b, const float* gn_w, const float* gn_b, const float* c3w, const float* c3b,
                              const float* w2_t, const float* b2, float* s1, float* s2, float* s3, float* a3, float* gn_sums, float* x, void* stream);

/* ---- OnlineSpatialNet: the causal T-ConvFFN for training (csrc/online_train.hip; nbss_amd/online_train.py) -----------------------------------
 * The block of nbss_online_tconvffn_step on whole utterances, forward and backward: y = x + T-ConvFFN(x) on x, y [B][F][T][96] of `dtype`
 * (NBSS_F32: fp32 MFMA; NBSS_BF16: bf16 MFMA, fp32 accumulation); parameters, gradients and every statistic fp32.  The parameters are the
 * module's own tensors in state_dict layout (NOT transposed): ln_w ln_b [96], w1 [192][96], b1 [192], c1w c2w c3w [192][24][3] with
 * c1b c2b c3b [192] (causal: output frame t reads input frames t-2 .. t, zero before frame 0), gn_w gn_b [192], w2 [96][192], b2 [96].
 * Geometry 96 / 192 / 8 groups / k 3.  NBSS_EINVAL: dtype outside {NBSS_F32, NBSS_BF16}, B < 1, F < 1, a NULL pointer (`save` of the forward
 * excepted), y == x, dx == dy or dx == x.  NBSS_EUNSUPPORTED: T outside 1 .. NBSS_T_MAX (4096), F > NBSS_F_MAX, more than 2^28 tokens.  The two
 * *_bytes calls return the same codes (negative) instead of a size.  Nothing is launched after a refusal.
 * save: nbss_online_tconvffn_train_save_bytes() bytes that the forward fills for the backward — the LayerNorm (mean, rstd) per token, the
 *   GroupNorm (mean, rstd) per (b, t, group) and the stream tensors a1, a2, a3 (pre-activations), h4 = SiLU(GroupNorm(a3)) and a4; the
 *   backward recomputes LayerNorm(x), the three other SiLUs and the GroupNorm's xhat.  save = NULL: forward only (inference).
 * ws: nbss_online_tconvffn_train_ws_bytes() bytes of scratch, for either call.
 * bwd: dx = dy + (block)'(dy) — the residual path included; every d_* buffer is ACCUMULATED into (+=), like nbss_nb_*_bwd.
 * No atomics: the GroupNorm statistics and the backward's per-frame sums are folded over the frequencies in order, parameter-gradient partials of
 * fixed token slabs in slab order — two calls give the same bits, and the y / dx rows of a batch item do not depend on the other items. */
int64_t nbss_online_tconvffn_train_save_bytes(int dtype, int B, int F, int T);
int64_t nbss_online_tconvffn_train_ws_bytes(int dtype, int B, int F, int T);
int nbss_online_tconvffn_train_fwd(int dtype, int B, int F, int T, const float* ln_w, const float* ln_b, const float* w1, const float* b1, const float* c1w,
                                   const float* c1b, const float* c2w, const float* c2b, const float* gn_w, const float* gn_b, const float* c3w, const float* c3b,
                                   const float* w2, const float* b2, const void* x, void* y, void* save, void* ws, void* stream);
int nbss_online_tconvffn_train_bwd(int dtype, int B, int F, int T, const float* ln_w, const float* ln_b, const float* w1, const float* b1, const float* c1w,
                                   const float* c1b, const float* c2w, const float* c2b, const float* gn_w, const float* gn_b, const float* c3w, const float* c3b,
                                   const float* w2, const float* b2, const void* x, const void* save, const void* dy, void* dx, float* d_ln_w, float* d_ln_b,
                                   float* d_w1, float* d_b1, float* d_c1w, float* d_c1b, float* d_c2w, float* d_c2b, float* d_gn_w, float* d_gn_b, float* d_c3w,
                                   float* d_c3b, float* d_w2, float* d_b2, void* ws, void* stream);

/* ---- OnlineSpatialNet: the chunkwise retention core for training (csrc/online_ret_train.hip; nbss_amd/online_train.py) -------------------------
 * What models/arch/base/retention.py computes between the q / k / v / g projections and out_proj for chunkwise_recurrent = True, rope = False,
 * look_ahead = 0 and chunks of 64 frames — MultiScaleRetention.chunk_recurrent_forward, the per-head RMSNorm (eps 1e-6, no affine) and the SiLU gate —
 * on BF sequences of T frames, forward and backward; 4 heads, key width 24, value width 48.  q, k, dq, dk [BF][T][96]; v, g, out, d_out, dv, dg
 * [BF][T][192]; all contiguous and of `dtype` (NBSS_F32: fp32 MFMA; NBSS_BF16: bf16 MFMA operands, fp32 accumulation).  decay [4]: the per-head gamma
 * (fp32, on the device, as nbss_online_ret_step takes it).  The decay powers, the two row scalings (the decay row sums and the clamped absolute score
 * sums, which the gradient treats as constants like the module does), the RMS statistics and the [24][48] state are fp32 in either dtype.
 * k: the keys, used as k_scale * k ('ret(2,not_share_qk)': k_scale = 24^-0.5); k = NULL shares them with q ('share_qk'; k_scale is ignored).
 * bwd: dq, dk, dv, dg are WRITTEN (not accumulated); dk includes the k_scale factor; with k = NULL dk must be NULL and dq is the sum of both roles of q.
 * NBSS_EINVAL: dtype outside {NBSS_F32, NBSS_BF16}, BF < 1, a NULL pointer other than k, dk or the forward's `save`, dk without k or k without dk,
 * `out` equal to q, k, v or g.  NBSS_EUNSUPPORTED: T outside 1 .. NBSS_T_MAX (4096), more than 2^28 tokens.  The two *_bytes calls return the same
 * codes (negative) instead of a size.  Nothing is launched after a refusal.
 * save: nbss_online_ret_train_save_bytes() bytes that the forward fills for the backward — the fp32 state at the START of every chunk,
 *   [BF][4][ceil(T / 64)][24][48]; the backward walks the chunks in reverse, carries the state's gradient, and recomputes each chunk's scores, row
 *   scalings, output and RMS statistics from q, k, v and that state.  save = NULL: forward only (inference), nothing is kept.
 * ws: nbss_online_ret_train_ws_bytes() bytes, for either call: reserved (one 256-byte piece; the kernels keep a chunk's intermediates in LDS).
 * One workgroup per (sequence, head) walks the chunks; more than 4096 pairs are covered by a grid-stride loop.  No atomics, every sum in a fixed order:
 * two calls give the same bits, and a sequence's rows do not depend on the other sequences of the launch. */
int64_t nbss_online_ret_train_save_bytes(int dtype, int64_t BF, int T);
int64_t nbss_online_ret_train_ws_bytes(int dtype, int64_t BF, int T);
int nbss_online_ret_train_fwd(int dtype, int64_t BF, int T, const void* q, const void* k, const void* v, const void* g, float k_scale,
                              const float* decay, void* out, void* save, void* ws, void* stream);
int nbss_online_ret_train_bwd(int dtype, int64_t BF, int T, const void* q, const void* k, const void* v, const void* g, float k_scale,
                              const float* decay, const void* save, const void* d_out, void* dq, void* dk, void* dv, void* dg, void* ws, void* stream);

/* ---- OnlineSpatialNet: the whole retention block for training (csrc/online_tsa_train.hip; nbss_amd/online_train.py) ---------------------------
 * y = x + out_proj(SiLU(g) * RMSNorm_head(chunk_retention(q, k, v))) with u = LayerNorm(x) (eps 1e-5, affine), q = wq u, k = 24^-0.5 wk u, v = wv u,
 * g = wg u — `SpatialNetLayer._tsa` of models/arch/OnlineSpatialNet.py with attention 'ret(2,*)' plus the residual of its caller — on BF sequences of T
 * frames, forward and backward.  x, y, dy, dx [BF][T][96], contiguous and of `dtype` (NBSS_F32: fp32 MFMA; NBSS_BF16: bf16 MFMA operands, fp32
 * accumulation; LayerNorm, RMS and decay statistics fp32 in either).  The parameters are the module's own fp32 tensors in state_dict layout, without
 * bias: ln_w ln_b [96], wq wk [96][96], wv wg [192][96], wo [96][192]; decay [4]: the per-head gamma (fp32, on the device).  The core between the
 * projections and out_proj is nbss_online_ret_train_fwd / _bwd (4 heads, key width 24, value width 48, chunks of 64 frames, no rotary positions, no
 * look-ahead); out_proj with the residual is nbss_nb_conv_t with taps = 1 (the same launches: y has the bits of chaining the two on the saved q, k, v, g).
 * wk = NULL: shared keys ('share_qk': k = q, unscaled); then d_wk must be NULL, and `share_qk` of the two *_bytes calls must be non-zero.
 * save: nbss_online_tsa_save_bytes() bytes that the forward fills for the backward, each piece 256-byte aligned: q [BF][T][96] | k (absent with shared
 *   keys) | v [BF][T][192] | g | the gated core output (the input of out_proj) [BF][T][192], all of `dtype` | (mean, rstd) [BF][T][2] fp32 | the core's
 *   chunk states (nbss_online_ret_train_save_bytes()).  The gated core output is KEPT, not recomputed (it is the operand of d_wo; the core's backward never
 *   writes it).  Per token: NBSS_F32 3 368 bytes, NBSS_BF16 1 832 (shared keys: 384 / 192 less).  u = LayerNorm(x) is never stored by the forward; the
 *   backward recomputes it into `ws` for the weight gradients.  save = NULL: forward only (inference), nothing is kept.
 * ws: nbss_online_tsa_ws_bytes() bytes of scratch, for either call (it holds the workspace of nbss_nb_conv_t_bwd, ~62 MB: allocate it once per shape).
 * bwd: dx includes the residual path; the seven d_* buffers are WRITTEN (not accumulated; they may be uninitialised): the call zeroes them before the
 *   accumulating building blocks (nbss_nb_conv_t_bwd, the fold of the LayerNorm partial rows) add to them.
 * NBSS_EINVAL: dtype outside {NBSS_F32, NBSS_BF16}, BF < 1, a NULL pointer other than wk, d_wk or the forward's `save`, d_wk without wk or wk without
 * d_wk, y == x, dx == dy, dx == x.  NBSS_EUNSUPPORTED: T outside 1 .. NBSS_T_MAX (4096), more than 2^28 tokens.  The two *_bytes calls return the same
 * codes (negative) instead of a size.  Nothing is launched after a refusal.
 * One workgroup per 128 rows in the two projection kernels (no grid cap).  No atomics, every sum in a fixed order: two calls give the same bits, and a
 * sequence's rows of y and dx do not depend on the other sequences of the launch. */
int64_t nbss_online_tsa_save_bytes(int dtype, int64_t BF, int T, int share_qk);
int64_t nbss_online_tsa_ws_bytes(int dtype, int64_t BF, int T, int share_qk);
int nbss_online_tsa_train_fwd(int dtype, int64_t BF, int T, const float* ln_w, const float* ln_b, const float* wq, const float* wk, const float* wv,
                              const float* wg, const float* wo, const float* decay, const void* x, void* y, void* save, void* ws, void* stream);
int nbss_online_tsa_train_bwd(int dtype, int64_t BF, int T, const float* ln_w, const float* ln_b, const float* wq, const float* wk, const float* wv,
                              const float* wg, const float* wo, const float* decay, const void* x, const void* save, const void* dy, void* dx,
                              float* d_ln_w, float* d_ln_b, float* d_wq, float* d_wk, float* d_wv, float* d_wg, float* d_wo, void* ws, void* stream);

/* ---- OnlineSpatialNet: the core of a Mamba block for training (csrc/online_mamba_train.hip; nbss_amd/online_train.py) ---------------------------
 * What models/arch/base/mamba.py computes between in_proj and out_proj (Mamba.core) for d_model 96, expand 2, d_state 16, d_conv 4, dt_rank 6 — the
 * causal depthwise convolution with its SiLU, x_proj, dt_proj with its softplus, the selective scan h_t = exp(dt_t A) h_{t-1} + dt_t B_t x_t,
 * y_t = C_t h_t + D x_t, and the gate y * SiLU(z) — on BF sequences of T frames, forward and backward.  xz, dxz [BF][T][384] (x | z: the output of
 * in_proj); y, dy [BF][T][192]; all contiguous and of `dtype` (NBSS_F32 or NBSS_BF16; all arithmetic is fp32 in either).  The parameters are the
 * module's own fp32 tensors in state_dict layout: conv_w [192][1][4], conv_b [192], xproj_w [38][192], dt_w [192][6], dt_b [192], A_log [192][16], D [192].
 * save: nbss_online_mamba_train_save_bytes() bytes that the forward fills for the backward, each piece 256-byte aligned: the fp32 state h at the START
 *   of every run of 8 frames [BF][ceil(T / 8)][16][192] | the x_proj outputs (dt_r, B, C) [BF][T][38] fp32.  The backward walks the runs in reverse,
 *   recomputes the states of a run into LDS from its checkpoint and carries the state's gradient (no division by the decay).  save = NULL: forward only
 *   (inference), nothing is kept.
 * ws: nbss_online_mamba_train_ws_bytes() bytes, for either call (the backward's per-workgroup partial parameter gradients, min(BF, 512) rows of 67 x 192).
 * bwd: dxz and the seven d_* buffers (fp32, the parameters' layouts) are WRITTEN (not accumulated; they may be uninitialised).
 * NBSS_EINVAL: BF < 1, T outside 1 .. NBSS_T_MAX (4096), a NULL pointer other than the forward's `save`, y == xz, dxz == xz or dy.
 * NBSS_EUNSUPPORTED: dtype outside {NBSS_F32, NBSS_BF16}, more than 2^28 tokens.  The two *_bytes calls return the same codes (negative) instead of a
 * size.  Nothing is launched after a refusal.
 * One workgroup of 192 threads (a thread per channel, its 16 states in registers) per sequence; more than 512 sequences are covered by a grid-stride
 * loop.  No atomics, every sum in a fixed order (the sums over the channels through LDS, the parameter gradients as per-workgroup partial rows that a
 * second launch folds): two calls give the same bits, and a sequence's rows of y and dxz do not depend on the other sequences of the launch. */
int64_t nbss_online_mamba_train_save_bytes(int dtype, int64_t BF, int T);
int64_t nbss_online_mamba_train_ws_bytes(int dtype, int64_t BF, int T);
int nbss_online_mamba_train_fwd(int dtype, int64_t BF, int T, const void* xz, const float* conv_w, const float* conv_b, const float* xproj_w,
                                const float* dt_w, const float* dt_b, const float* A_log, const float* D, void* y, void* save, void* ws, void* stream);
int nbss_online_mamba_train_bwd(int dtype, int64_t BF, int T, const void* xz, const float* conv_w, const float* conv_b, const float* xproj_w,
                                const float* dt_w, const float* dt_b, const float* A_log, const float* D, const void* save, const void* dy, void* dxz,
                                float* d_conv_w, float* d_conv_b, float* d_xproj_w, float* d_dt_w, float* d_dt_b, float* d_A_log, float* d_D, void* ws,
                                void* stream);

/* ---- OnlineSpatialNet: the cross-band trio for training (csrc/online_xband_train.hip; nbss_amd/online_train.py) -------------------------------
 * x1 = x + fconv1(x), x2 = x1 + full(x1), y = x2 + fconv2(x2) of models/arch/OnlineSpatialNet.py `SpatialNetLayer.forward` on x, y [B][F][T][96] of
 * `dtype`, forward and backward, through the SpatialNet-small kernels behind nbss_fconv_fwd / nbss_full_fwd and their _bwd (the same launches: the results
 * have the bits of chaining those entry points on a one-layer SpatialNet with the same parameters).  No nbss_cfg, flat buffer or packed buffer on the
 * caller's side: the 18 parameters are the module's own fp32 tensors in state_dict order and layout — fconv1.0.{weight,bias} [96], fconv1.1.weight
 * [96][12][5], fconv1.1.bias [96], fconv1.2.weight [96] (per-channel PReLU), norm_full.{weight,bias} [96], squeeze.0.weight [8][96], squeeze.0.bias [8],
 * full.weight [8][F][F], full.bias [8][F], unsqueeze.0.weight [96][8], unsqueeze.0.bias [96], fconv2.* like fconv1.* — gathered and packed inside `ws` by
 * every call.  Geometry 96 / 8, F-conv groups 8, kernel 5, zero padding, LayerNorm eps 1e-5.
 * save: nbss_online_xband_save_bytes() bytes that the forward fills for the backward: x1 and x2, two stream tensors; the backward recomputes every
 *   other intermediate from x, x1 and x2.  save = NULL: forward only, nothing kept.
 * ws: nbss_online_xband_ws_bytes() bytes of scratch, for either call (it holds the reused backward kernels' workspace, nbss_workspace_bytes of the
 *   one-layer configuration: allocate it once per shape, not per call).
 * bwd: dx includes the three residual paths; the 18 d_* buffers are WRITTEN (not accumulated; they may be uninitialised).
 * NBSS_EINVAL: dtype outside {NBSS_F32, NBSS_BF16}, B, F or T < 1, a NULL pointer (`save` of the forward excepted), y == x, dx == dy.
 * NBSS_EUNSUPPORTED: F > 272, T > 4096, more than 2^31 / 288 tokens; for the backward, a forward with `save`, and nbss_online_xband_save_bytes: T > 256,
 * or NBSS_F32 with F > 160.  The two *_bytes calls return the same codes (negative) instead of a size.  Nothing is launched after a refusal. */
int64_t nbss_online_xband_save_bytes(int dtype, int B, int F, int T);
int64_t nbss_online_xband_ws_bytes(int dtype, int B, int F, int T);
int nbss_online_xband_train_fwd(int dtype, int B, int F, int T, const float* fc1_ln_w, const float* fc1_ln_b, const float* fc1_w, const float* fc1_b,
                                const float* fc1_prelu, const float* full_ln_w, const float* full_ln_b, const float* sq_w, const float* sq_b,
                                const float* full_w, const float* full_b, const float* usq_w, const float* usq_b, const float* fc2_ln_w,
                                const float* fc2_ln_b, const float* fc2_w, const float* fc2_b, const float* fc2_prelu, const void* x, void* y, void* save,
                                void* ws, void* stream);
int nbss_online_xband_train_bwd(int dtype, int B, int F, int T, const float* fc1_ln_w, const float* fc1_ln_b, const float* fc1_w, const float* fc1_b,
                                const float* fc1_prelu, const float* full_ln_w, const float* full_ln_b, const float* sq_w, const float* sq_b,
                                const float* full_w, const float* full_b, const float* usq_w, const float* usq_b, const float* fc2_ln_w,
                                const float* fc2_ln_b, const float* fc2_w, const float* fc2_b, const float* fc2_prelu, const void* x, const void* save,
                                const void* dy, void* dx, float* d_fc1_ln_w, float* d_fc1_ln_b, float* d_fc1_w, float* d_fc1_b, float* d_fc1_prelu,
                                float* d_full_ln_w, float* d_full_ln_b, float* d_sq_w, float* d_sq_b, float* d_full_w, float* d_full_b, float* d_usq_w,
                                float* d_usq_b, float* d_fc2_ln_w, float* d_fc2_ln_b, float* d_fc2_w, float* d_fc2_b, float* d_fc2_prelu, void* ws,
                                void* stream);

/* ---- OnlineSpatialNet: the waveform ends of a streaming step (csrc/online_io.hip; nbss_amd/online_io.py: NativeWaveStreamer) ----------------
 * n_fft in {256, 512}, hop = n_fft/2, win_len = n_fft, `tables` of nbss_stft_tables; 2 <= C <= 32 frames per call (NBSS_EUNSUPPORTED outside).
 * Frame t of the stream is frame t of torch.stft(center=True): samples [(t-1) hop, (t+1) hop).  Neither call knows a first or a last chunk:
 * the caller puts the left reflect padding into `tail` before the first chunk and pushes the right one after the last sample.
 * norm: the online normalisation by the reference microphone (models/io/norm.py): NONE; FREQUENCY: xrmm [B,F,C] = |X_ref| + 1e-6;
 * UTTERANCE: xrmm [B,1,C] = mean over F of |X_ref| + 1e-6 (folded in a fixed order: bitwise repeatable, the same for every chunk size).
 * stft step: x_chunk [B,M,C hop], tail [B,M,hop] (the hop samples before the chunk; updated in place to the chunk's last hop)
 * -> feats [B,F,C,2M] (normalised; the layout the network step reads) and xrmm (may be NULL with NONE).  ws: B F C floats of scratch,
 * UTTERANCE only (else may be NULL). */
#define NBSS_ONLINE_NORM_NONE 0
#define NBSS_ONLINE_NORM_FREQUENCY 1
#define NBSS_ONLINE_NORM_UTTERANCE 2
int nbss_online_stft_step(int n_fft, int norm, int B, int M, int C, int ref_channel, const float* tables, const float* x_chunk, float* tail,
                          float* feats, float* xrmm, float* ws, void* stream);
/* istft step: out [B,F,C,2S] * xrmm -> irfft, window, overlap-add, / window envelope -> y_chunk [B,S,C hop]: the sample stream DELAYED BY ONE
 * HOP (call k returns the samples [k C hop - hop, (k+1) C hop - hop)).  ola [B,S,hop]: the windowed second half of the frame before the chunk
 * (zero at the start of a stream), updated in place.  One lane writes each sample: no atomics, y_chunk needs no clearing. */
int nbss_online_istft_step(int n_fft, int norm, int B, int S, int C, const float* tables, const float* out, const float* xrmm, float* ola,
                           float* y_chunk, void* stream);

/* ---- narrow-band building blocks (models/arch/NBC2.py:152-238 in the reference: pre-norm self-attention over time + convolutional feed-forward with
 * GroupBatchNorm, per (batch, frequency) sequence) -------------------------------------------------------------------------------------------------
 * Geometry-generic kernels (csrc/nb_blocks.hip over gb_gemm.hip, gb_rows.hip, gb_attn.hip, attn_relpos.hip, attn_kb.hip, attn_relpos_kb.hip), one operation per call on caller-owned tensors of `dtype` (NBSS_F32 | NBSS_BF16) in the [nseq][T][C] layout
 * of the reference's [B*F, T, C] activations; weights / biases / affines are the fp32 parameters in their state_dict layout.  nbss_amd/nbc2.py sequences an
 * NBC2 forward from them.  act_in / act_out: 1 = SiLU applied to the input as it is read / to the result.
 * conv_t: y[n][t][o] = sum_tap sum_i x[n][t + tap - taps/2][i] w[o][i][tap] + bias[o] (+ residual[n][t][o]), grouped, zero padded ("same"); taps = 1 is a
 * per-token Linear (w [Cout][Cin]).  x rows are ldx elements apart (ldx >= Cin; groups = 1: ldx % 8 == 0 and the columns Cin..round_up(Cin, 8) must be
 * zero; groups > 1: ldx == Cin, Cin / groups % 8 == 0).  ws: nbss_nb_ws_bytes(Cout, Cin, groups, taps) bytes of scratch (the re-laid weights). */
int64_t nbss_nb_ws_bytes(int Cout, int Cin, int groups, int taps);
int nbss_nb_conv_t(int dtype, int64_t nseq, int T, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y,
                   const void* residual, int act_in, int act_out, void* ws, void* stream);
/* LayerNorm over C (eps 1e-5): y = xhat gamma + beta; stats [rows][2] fp32 scratch (mean, rstd) */
int nbss_nb_layernorm(int dtype, int64_t rows, int C, const void* x, const float* gamma, const float* beta, void* y, float* stats, void* stream);
/* GroupBatchNorm (NBC2.py:57-145, share_along_sequence_dim = false): statistics over the F sequences of an utterance x C features per frame, from the input
 * itself; x, y [B][F][T][C]; gamma / beta [C] or NULL */
int nbss_nb_group_batch_norm(int dtype, int B, int F, int T, int C, const void* x, const float* gamma, const float* beta, float eps, int act_out, void* y,
                             void* stream);
/* softmax(q k^T / sqrt(dh)) v per (sequence, head): qkv [nseq][T][3H] (q | k | v; head h at columns h dh), o [nseq][T][H]; T <= 256, dh in {24, 48, 96}
 * (24 / 48: a head's K and V stay in LDS; 96: walked in blocks of 64 keys with a running max / sum per query, csrc/attn_kb.hip); anything else: NBSS_EUNSUPPORTED */
int nbss_nb_attention_fwd(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, void* o, void* stream);
/* the narrow-band conformer NBC (reference models/arch/NBC.py): Transformer-XL relative-position attention (NBC.py:106-143) —
 *   softmax(((q + u) k^T + (q + v) P[i - j]) * scale) v per (sequence, head); pos [2T - 1][H] = pos_proj of the sinusoid table for the offsets
 *   -(T - 1) .. T - 1 (stream dtype), u_bias / v_bias [heads][dh] fp32, scale = 1 / sqrt(d_model) in the reference; T <= 256, dh in {24, 48}
 * — and the GroupNorm(groups, C) + optional SiLU between the convolutions of its feed-forward (NBC.py:195-203; statistics over (C / groups) x T per
 * sequence, eps 1e-5): x, y [nseq][T][C]. */
int nbss_nb_attention_relpos_fwd(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, const void* pos, const float* u_bias, const float* v_bias,
                                 float scale, void* o, void* stream);
int nbss_nb_group_norm(int dtype, int64_t nseq, int T, int C, int groups, const void* x, const float* gamma, const float* beta, int act_out, void* y, void* stream);
/* the two attentions on LONG sequences, forward only (inference on whole utterances: the reference evaluates every dataset on 4 - 32 s, 400 - 2 000 frames,
 * through NBC2.py:152-238 resp. NBC.py:106-143, which materialise [nseq heads][T][T] scores): 1 <= T <= 4096, the keys walked in blocks of 64 with a running
 * max / sum per query (csrc/attn_kb.hip, csrc/attn_relpos_kb.hip: per key block also the 127 rows of pos its offsets i - j need).  Same tensors as
 * attention_fwd / attention_relpos_fwd; dh in {24, 48, 96} resp. {24, 48}; anything else: NBSS_EUNSUPPORTED.  One writer per output element, no atomics. */
int nbss_nb_attention_long_fwd(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, void* o, void* stream);
int nbss_nb_attention_relpos_long_fwd(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, const void* pos, const float* u_bias, const float* v_bias,
                                      float scale, void* o, void* stream);

/* ---- the same building blocks for TRAINING (autograd of the reference's torch.nn NBC2: NBC2.py:152-238; sequenced by nbss_amd/nbc2.py) ---------------
 * conv_t_train: conv_t without fused input / output activations, plus an optional second output y_silu = SiLU(y) (pre-activation and activation of a
 *   feed-forward step in one pass).
 * conv_t_bwd: gradients of y = conv_t(x): dx [nseq][T][ldx] = conv^T(dy) — multiplied by SiLU'(x_pre) when x_pre (the pre-activation x = SiLU(x_pre) was made
 *   from, same layout as dx) is given — and dw [Cout][Cin / groups][taps] += dy^T x, dbias [Cout] += colsum(dy) (fp32, ACCUMULATED; either of dx / dw may be
 *   NULL).  ws: nbss_nb_bwd_ws_bytes(Cout, Cin, groups, taps) bytes (the re-laid transposed weights + partial tiles of the weight gradient).
 * layernorm_bwd: dx = dres + LayerNorm'(dy) with the forward's stats; dgamma / dbeta accumulated.
 * group_batch_norm_bwd: gradient through y = act(GroupBatchNorm(x)) (statistics recomputed from x); dgamma / dbeta accumulated (NULL when not affine).
 * attention_bwd: dqkv [nseq][T][3H] from qkv and d_o = gradient w.r.t. the attention output; ws: nbss_nb_attention_bwd_ws_bytes() bytes.  Same limits as
 *   attention_fwd (T <= 256, dh in {24, 48, 96}); scores are recomputed, no atomics: bitwise repeatable. */
int64_t nbss_nb_bwd_ws_bytes(int Cout, int Cin, int groups, int taps);
int nbss_nb_conv_t_train(int dtype, int64_t nseq, int T, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y,
                         void* y_silu, const void* residual, void* ws, void* stream);
int nbss_nb_conv_t_bwd(int dtype, int64_t nseq, int T, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const void* dy,
                       const void* x_pre, void* dx, float* dw, float* dbias, void* ws, void* stream);
int nbss_nb_layernorm_bwd(int dtype, int64_t rows, int C, const void* x, const float* stats, const float* gamma, const void* dy, const void* dres, void* dx,
                          float* dgamma, float* dbeta, void* stream);
int nbss_nb_group_batch_norm_bwd(int dtype, int B, int F, int T, int C, const void* x, const float* gamma, const float* beta, float eps, int act_out, const void* dy,
                                 void* dx, float* dgamma, float* dbeta, void* stream);
int64_t nbss_nb_attention_bwd_ws_bytes(int dtype, int64_t nseq, int T, int H, int heads);
int nbss_nb_attention_bwd(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, const void* d_o, void* dqkv, void* ws, void* stream);

/* ---- ... and for training the narrow-band conformer NBC (autograd of the reference's NBC.py:73-237; sequenced by nbss_amd/nbc.py) --------------------------
 * attention_relpos_train: the relative-position attention with attention dropout (NBC.py:137): keep_bits [nseq][heads][T][ceil(T / 32)] uint32 — bit (j & 31) of
 *   word j >> 5 of row i = probability (i, j) kept — or NULL; kept probabilities are scaled by keep_scale = 1 / (1 - p).  The caller draws the bits (any RNG):
 *   forward and backward read the same tensor.
 * attention_relpos_bwd: dqkv [nseq][T][3H] from qkv, pos, the biases, the bits and d_o; dpos [2T - 1][H], du_bias / dv_bias [H] (fp32) ACCUMULATED (sums over
 *   all sequences, fixed order: no atomics).  ws: nbss_nb_attention_relpos_bwd_ws_bytes() bytes.
 * group_norm_train: group_norm that also keeps (mean, rstd) per (sequence, group) in stats [nseq * groups][2];  group_norm_bwd: gradient through
 *   y = SiLU(GroupNorm(x)) IN PLACE (dy_dx holds dy on entry, dx on return); dgamma / dbeta [C] accumulated. */
int nbss_nb_attention_relpos_train(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, const void* pos, const float* u_bias, const float* v_bias,
                                   float scale, const uint32_t* keep_bits, float keep_scale, void* o, void* stream);
int64_t nbss_nb_attention_relpos_bwd_ws_bytes(int64_t nseq, int T, int H, int heads);
int nbss_nb_attention_relpos_bwd(int dtype, int64_t nseq, int T, int H, int heads, const void* qkv, const void* pos, const float* u_bias, const float* v_bias, float scale,
                                 const uint32_t* keep_bits, float keep_scale, const void* d_o, void* dqkv, float* dpos, float* du_bias, float* dv_bias, void* ws,
                                 void* stream);
int nbss_nb_group_norm_train(int dtype, int64_t nseq, int T, int C, int groups, const void* x, const float* gamma, const float* beta, int act_out, void* y, float* stats,
                             void* stream);
int nbss_nb_group_norm_bwd(int dtype, int64_t nseq, int T, int C, int groups, const void* x, const float* stats, const float* gamma, const float* beta, void* dy_dx,
                           float* dgamma, float* dbeta, void* stream);

/* ---- the narrow-band BiLSTM (reference models/arch/blstm2_fc1.py:45-68: nn.LSTM(bidirectional) per frequency bin; sequenced by nbss_amd/blstm.py) ------------
 * One bidirectional layer's recurrences, all T steps in one persistent launch (a workgroup per tile of sequences and direction; gates GEMM on MFMA, h in LDS,
 * c in registers).  gx [nseq][T][ldg]: W_ih x + b_ih + b_hh of both directions (direction d at columns d * 4 hidden; gate order i | f | g | o), from
 * nbss_nb_conv_t.  w_hh / w_hh_reverse [4 hidden][hidden] fp32.  y [nseq][T][2 hidden] (direction d at columns d * hidden).  save (training; or NULL):
 * [2][nseq][T][5 hidden] i | f | g | o | c, stream dtype.  hidden in {128, 256}.  ws: nbss_nb_blstm_ws_bytes() bytes (the packed recurrent weights).
 * blstm_bwd: dg [nseq][T][8 hidden] = gradient w.r.t. the gate pre-activations of both directions from dy (gradient w.r.t. y) and save; the weight, bias and
 *   input gradients are dense contractions of dg (nbss_nb_conv_t_bwd). */
int64_t nbss_nb_blstm_ws_bytes(int dtype, int hidden);
int nbss_nb_blstm_fwd(int dtype, int64_t nseq, int T, int hidden, int ldg, const void* gx, const float* w_hh, const float* w_hh_reverse, void* y, void* save, void* ws,
                      void* stream);
int nbss_nb_blstm_bwd(int dtype, int64_t nseq, int T, int hidden, const void* dy, const void* save, const float* w_hh, const float* w_hh_reverse, void* dg, void* ws,
                      void* stream);

/* ---- diagnostics ---------------------------------------------------------------------------*/
/* D = A(16x32) * B(32x16) through the same MFMA fragment helpers the kernels use
 * (natural or permuted K order); used by the tests to pin the gfx950 fragment layouts. */
int nbss_selftest_mma(int dtype, int kperm, const float* A, const float* B, float* D, void* stream);
const char* nbss_build_info(void);
/* Opt-in per-kernel timing: HIP events recorded on the launch stream around each kernel whose bit is
 * set in `mask` (bit i = kernel id i, 0 .. nbss_profile_kernels()-1; 0 disables).  nbss_profile_read
 * waits for the recorded events, returns summed milliseconds / launch counts per id and clears them. */
int nbss_profile_enable(int64_t mask);
int nbss_profile_kernels(void);
const char* nbss_profile_name(int id);
int nbss_profile_read(double* total_ms, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* NBSS_HIP_H */
