/* librvc_hip.so - C ABI of the MI355X-native RVC voice-conversion inference path.
 *
 * The reference (SayanoAI/Comfy-RVC) is pure Python with no FFI; its "operator API" for this path is a set of
 * duck-typed Python callables.  Each entry point below is what a ctypes binding of that callable binds
 * (comfy-rvc_amd/_lib.py is that binding; INTEGRATION.md shows the reference-side stubs):
 *
 *   rvc_hubert_forward   <- HubertModelWithFinalProj.extract_features   lib/infer_pack/loaders.py:55-61
 *   rvc_rmvpe_forward    <- RMVPE.infer_from_audio / _with_pitch         lib/rmvpe.py:614-659 (mel :510-556, E2E :464-470,
 *                                                                        decode :607-612,:661-685)
 *   rvc_synth_infer      <- SynthesizerTrnMs{256,768}NSFsid.infer        lib/infer_pack/models.py:682-693,:798-809
 *   rvc_synth_forward    <- SynthesizerTrnMs{256,768}NSFsid.forward      lib/infer_pack/models.py:665-680,:781-796 (PosteriorEncoder :199-238)
 *   rvc_kl_loss          <- kl_loss                                      lib/train/losses.py:596-611
 *   rvc_l1_sum           <- F.l1_loss(y_mel, y_hat_mel)                  training_cli.py:570
 *   rvc_kl_loss_grad     <- loss_kl's share of loss_gen_all.backward()   training_cli.py:571,:598
 *   rvc_mel_spectrogram_vjp <- torch.autograd.grad(loss_mel, [y_hat]) through mel_spectrogram_torch   lib/train/mel_processing.py:117-150, lib/train/losses.py:76-92
 *   rvc_mel_loss_cotangents <- the backward of F.l1_loss(y_mel, y_hat_mel) / MultiScaleMelSpectrogramLoss's loss_fn   training_cli.py:569-570, lib/train/losses.py:530-561
 *   rvc_synth_flow_input_grad <- loss_kl's way through ResidualCouplingBlock in loss_gen_all.backward()   training_cli.py:598, lib/infer_pack/models.py:150-196
 *   rvc_synth_flow_weight_grad <- the same backward onto net_g.flow.parameters() (optim_g's gradients)      training_cli.py:598, lib/infer_pack/modules.py:130-209,:436-455
 *   rvc_disc_forward     <- MultiPeriodDiscriminator[V2].forward         lib/infer_pack/models.py:1024-1145 (net_d: training_cli.py:549,:567)
 *   rvc_sqerr_sums       <- discriminator_loss / generator_loss          lib/train/losses.py:571-593
 *   rvc_l1_sums          <- feature_loss                                 lib/train/losses.py:564-569
 *   rvc_disc_input_grad  <- torch.autograd.grad(loss, [wave]) through net_d      lib/train/losses.py:401-426 (gradient_norm_loss), :76-92 (LossBalancer)
 *   rvc_disc_weight_grad <- loss_disc.backward() onto net_d.parameters()            training_cli.py:559-562 (optim_d's gradients; grad_norm_d)
 *   rvc_disc_adamw_step  <- clip_grad_value_'s clamp and optim_d.step()             training_cli.py:562-563 (torch.optim.AdamW)
 *   rvc_loss_cotangents  <- the backward of the three GAN losses                 lib/train/losses.py:564-593
 *   rvc_interpolate      <- alpha * original + (1 - alpha) * generated            lib/train/losses.py:407
 *   rvc_vc_segment       <- VC.vc (features -> x2 upsample -> protect -> infer)   vc_infer_pipeline.py:25-114
 *   rvc_*_set_tensor     <- load_state_dict of the checkpoint tensors    vc_infer_pipeline.py:199-221,
 *                                                                        lib/infer_pack/loaders.py:19-31, lib/rmvpe.py:579-586
 *
 * Conventions: every function returns 0 on success and a non-zero status otherwise; rvc_last_error() gives the
 * thread-local message.  `stream` is a hipStream_t (NULL = default stream); all `*_dev` pointers are device pointers
 * owned by the caller (e.g. torch allocations); kernels are enqueued on `stream` and NOT synchronised.
 * Host pointers are only used for weights at load time.  Handles are not thread-safe; use one context per GPU/stream.
 * All tensors are float32 unless stated.  No CPU fallback exists: without a gfx950 device every call fails.
 */
#ifndef RVC_HIP_H
#define RVC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rvc_ctx rvc_ctx;
typedef struct rvc_hubert rvc_hubert;
typedef struct rvc_rmvpe rvc_rmvpe;
typedef struct rvc_synth rvc_synth;

const char* rvc_last_error(void);
const char* rvc_version(void);

int rvc_ctx_create(int device_id, rvc_ctx** out);
/* Destroying the LAST context of a device also frees that device's per-stream scratch: no call may be in flight on that device from
 * another thread at that moment (destroy the handles first, then the context, from one thread). */
int rvc_ctx_destroy(rvc_ctx* ctx);
/* bytes of activation workspace currently held by the context */
int64_t rvc_ctx_workspace_bytes(rvc_ctx* ctx);
/* Matrix-core arithmetic of the models FINALIZED on this context afterwards (state of the handle, not of the process):
 *   0 fp32 MFMA everywhere, 1 / 2 bf16x3 split where a layer is eligible (see rvc_set_conv_precision), -1 (default) the mode of the
 *   thread that calls *_finalize. */
int rvc_ctx_set_conv_precision(rvc_ctx* ctx, int mode);

/* ------------------------------------------------------------------ HuBERT / ContentVec (HF HubertModel + final_proj) */
typedef struct rvc_hubert_taps {   /* optional device buffers for intermediate tensors (NULL = skip) */
  float* conv_stack;   /* [512][T_h]   output of the 7-layer feature encoder (channel-major == HF [1,512,T_h]) */
  float* pos_conv;     /* [768][T_h]   gelu(pos_conv(x)) before the residual add                                */
  float* hidden_0;     /* [768][T_h]   hidden_states[0]                                                         */
  float* hidden_8;     /* [768][T_h]   hidden_states[8]                                                         */
} rvc_hubert_taps;

int rvc_hubert_create(rvc_ctx* ctx, rvc_hubert** out);
int rvc_hubert_set_tensor(rvc_hubert* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int rvc_hubert_finalize(rvc_hubert* h);
int rvc_hubert_destroy(rvc_hubert* h);
/* T_h = floor((L - 400) / 320) + 1 */
int64_t rvc_hubert_num_frames(int64_t L);
/* version 1: final_proj(hidden_states[8]) -> D = 256; version 2: hidden_states[11] -> D = 768.
 * n_layers = 0 runs only the layers the output needs (8 / 11); 12 reproduces the reference's full stack (timing only).
 * out_rm_dev: [T_h][D] row-major (reference layout [1,T_h,D]) or NULL; out_cm_dev: [D][T_h] channel-major or NULL. */
int rvc_hubert_forward(rvc_hubert* h, void* stream, const float* audio_dev, int64_t L, int version, int n_layers,
                       float* out_rm_dev, float* out_cm_dev, const rvc_hubert_taps* taps);

/* ------------------------------------------------------------------ RMVPE */
typedef struct rvc_rmvpe_taps {
  float* unet_out;     /* [16][T_r][128] */
  float* gru;          /* [512][T_r] channel-major (fwd | bwd) */
} rvc_rmvpe_taps;

int rvc_rmvpe_create(rvc_ctx* ctx, rvc_rmvpe** out);
int rvc_rmvpe_set_tensor(rvc_rmvpe* r, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* mel_basis [128][513] and the STFT forward basis [1026][1024] are tensors "mel_basis" / "stft.forward_basis" */
int rvc_rmvpe_finalize(rvc_rmvpe* r);
int rvc_rmvpe_destroy(rvc_rmvpe* r);
/* n = L / 160 + 1 frames.  mel_dev [128][n], salience_dev [n][360], f0_dev float64 [n]; any may be NULL. */
int rvc_rmvpe_forward(rvc_rmvpe* r, void* stream, const float* audio_dev, int64_t L, float thred, float* mel_dev,
                      float* salience_dev, double* f0_dev, const rvc_rmvpe_taps* taps);
/* Waits for `stream` and reports the last forward of this handle: 0 = ok.  The BiGRU scan's 16 workgroups exchange h_t through polled
 * device memory and need co-residency; when a hand-off times out (bounded spin) a serial, communication-free pass enqueued behind every scan
 * recomputes the recurrence (same summation order: hidden states within 2.4e-7 of a healthy run, ~6 us per step instead of ~1), so the forward still ends with valid f0 and
 * rvc_rmvpe_status stays 0 - rvc_rmvpe_repaired tells that it happened.  Non-zero (message via rvc_last_error) only when the time-out
 * was not repaired (the repair pass kept off by the test hook): f0_dev of that forward holds NaN then.
 * The reference has no counterpart (torch.nn.GRU, lib/rmvpe.py:420-428). */
int rvc_rmvpe_status(rvc_rmvpe* r, void* stream);
int rvc_rmvpe_repaired(rvc_rmvpe* r, void* stream);   /* 1: the last forward's scan timed out and was repaired by the serial pass */
/* test hook: fault & 1 makes one workgroup of the following scans exit without publishing; fault & 2 keeps the repair pass from being
 * enqueued; spin_limit (0 = default 2^24 polls) bounds how long the peers wait before they raise the flag */
int rvc_rmvpe_debug_fault(rvc_rmvpe* r, int fault, unsigned spin_limit);
/* decode alone: salience_dev [n][360] row-major -> f0 float64 [n] */
int rvc_rmvpe_decode(rvc_rmvpe* r, void* stream, const float* salience_dev, int64_t n, float thred, double* f0_dev);
/* Tail of get_f0 (reference pitch_extraction.py get_f0: transpose by `factor` = 2^(key / 12), mel-scale quantisation to 1 .. bins - 1 with np.rint), on the
 * device in float64: pitch_dev int64 [n] (coarse), pitchf_dev float32 [n] (Hz).  mel_min / mel_max = hz_to_mel(f0_min / f0_max) = 2595 log10(1 + f / 700). */
int rvc_f0_post(void* stream, const double* f0_dev, int64_t n, double factor, double mel_min, double mel_max, int bins, int64_t* pitch_dev, float* pitchf_dev);

/* ------------------------------------------------------------------ CREPE (torchcrepe.Crepe "full" / "tiny") */
/* Replaces the network inside torchcrepe.predict, which the reference calls for f0_method "crepe" / "mangio-crepe"
 * (pitch_extraction.py:76-150; torchcrepe is a third-party package, not vendored upstream: its published architecture is restated).
 * Tensors by their torchcrepe state-dict names: conv{1..6}.weight / .bias, conv{1..6}_BN.{weight,bias,running_mean,running_var},
 * classifier.weight / .bias. */
typedef struct rvc_crepe rvc_crepe;
typedef struct rvc_crepe_taps {
  float* conv1;        /* [C1][256]  ReLU(conv1) of frame 0 (before BatchNorm / pooling) */
  float* embed;        /* [4*C6][B]  flattened last feature map of the first batch of frames (B = min(n, 512)), row = position * C6 + channel */
} rvc_crepe_taps;
int rvc_crepe_create(rvc_ctx* ctx, int tiny, rvc_crepe** out);
int rvc_crepe_set_tensor(rvc_crepe* c, const char* name, const float* host_data, const int64_t* shape, int ndim);
int rvc_crepe_finalize(rvc_crepe* c);
int rvc_crepe_destroy(rvc_crepe* c);
/* frames of 1024 samples every `hop`: pad != 0 (torchcrepe's default) zero-pads the audio by 512 on both sides, n = 1 + L / hop;
 * pad == 0: n = 1 + (L - 1024) / hop */
int64_t rvc_crepe_num_frames(int64_t L, int hop, int pad);
/* audio_dev float32 [L] at 16 kHz -> probs_dev [360][n] channel-major: per-frame sigmoid outputs over the 360 pitch bins
 * (the mean / std normalisation of every frame, the six conv blocks and the classifier); decoding stays with the caller */
int rvc_crepe_forward(rvc_crepe* c, void* stream, const float* audio_dev, int64_t L, int hop, int pad, float* probs_dev, const rvc_crepe_taps* taps);

/* torchcrepe.decode.viterbi (its librosa.sequence.viterbi call included) and the periodicity gather of core.postprocess on the device:
 * bins outside [min_bin, max_bin) are masked, softmax over bins, most likely path under the triangular (width 12) transition matrix with a
 * uniform prior; bins_dev int32 [n], periodicity_dev [n] = probs[bin][frame].  Cents / dither / Hz stay on the host (numpy's RNG). */
int rvc_crepe_viterbi(void* stream, const float* probs_dev, int64_t n, int min_bin, int max_bin, int32_t* bins_dev, float* periodicity_dev);

/* ------------------------------------------------------------------ MDX23C vocal / instrumental separation (UVR chain) */
/* Replaces TFC_TDF_net.forward of reference lib/karafan/tfc_tdf.py:147-235 (with its STFT / inverse, :47-77); demix_mdxv3's chunking
 * (lib/karafan/inference.py:32-74) calls it once per chunk.  Fields = the entries of the model's yaml that the network reads
 * (lib/karafan/Data/model_2_stem_full_band_8k.yaml).  Tensors by their state-dict names plus three host-built constants:
 * "stft.basis" [2 dim_f][n_fft], "istft.basis" [n_fft][2 dim_f] (windowed DFT matrices) and "window" [n_fft] (periodic hann). */
typedef struct rvc_mdx23 rvc_mdx23;
typedef struct rvc_mdx23_config {
  int n_fft, hop, dim_f, dim_t;
  int num_channels, growth, num_scales, num_subbands, blocks_per_scale, bottleneck;
  int num_targets;       /* instruments the mask head separates (2: vocals, instrumental) */
  int audio_channels;    /* 2 */
} rvc_mdx23_config;
int rvc_mdx23_create(rvc_ctx* ctx, const rvc_mdx23_config* cfg, rvc_mdx23** out);
int rvc_mdx23_set_tensor(rvc_mdx23* m, const char* name, const float* host_data, const int64_t* shape, int ndim);
int rvc_mdx23_finalize(rvc_mdx23* m);
int rvc_mdx23_destroy(rvc_mdx23* m);
/* chunk_dev float32 [2][L] with L = hop * (dim_t - 1) -> out_dev [num_targets][2][L] */
int rvc_mdx23_forward(rvc_mdx23* m, void* stream, const float* chunk_dev, int64_t L, float* out_dev);
/* The chunk loop of demix_mdxv3 (reference lib/karafan/inference.py:52-66) in one call: n_chunks chunks of C = hop (dim_t - 1) samples every `step` samples of the
 * zero-padded stereo mix mix_dev [2][Lp] ((n_chunks - 1) step + C <= Lp); each chunk's separated signals are added (NaN as zero) into acc_dev [S][2][Lp] at the
 * chunk's offset, in chunk order, and the sum is divided by `overlap`.  acc_dev is overwritten.  The caller pads the mix and trims the result as the reference does. */
int rvc_mdx23_demix(rvc_mdx23* m, void* stream, const float* mix_dev, int64_t Lp, int64_t step, int64_t n_chunks, float overlap, float* acc_dev);
/* Chunk streams of rvc_mdx23_demix: 1 (default) = chunks in order on the caller's stream, the reference's order of additions; k = 2 .. 4: chunk c runs on stream
 * c mod k (streams, arenas and accumulators of the model's own, ordered against the caller's stream by events), the k accumulators are added in stream order -
 * reproducible, an ulp-level re-association.  For a single conversion alone on the GPU (the node); costs throughput when several clips are in flight. */
int rvc_mdx23_set_streams(rvc_mdx23* m, int k);

/* ------------------------------------------------------------------ synthesizer */
typedef struct rvc_synth_config {   /* the fields of cpt["config"] that the inference graph needs */
  int inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size;
  int n_resblock_kernels; int resblock_kernel_sizes[3]; int resblock_dilations[3][3];
  int n_upsamples; int upsample_rates[8]; int upsample_kernel_sizes[8];
  int upsample_initial_channel, spk_embed_dim, gin_channels, sr;
  int feat_dim;                    /* 768 (v2) or 256 (v1) */
  /* training forward only (rvc_synth_forward); 0 in both: an inference-only handle */
  int spec_channels;               /* rows of the linear spectrogram the posterior encoder reads (config[0]: 1025 / 513) */
  int segment_size;                /* frames of the slice the generator runs on (config[1]: 32) */
} rvc_synth_config;

typedef struct rvc_synth_taps {
  float* enc_p_layer0;  /* [192][T] */
  float* m_p;           /* [192][T] */
  float* logs_p;        /* [192][T] */
  float* z_p;           /* [192][T] */
  float* z;             /* [192][T] */
  float* sine_waves;    /* [T*upp]  SineGen output before Linear+tanh */
  float* har_source;    /* [T*upp] */
  float* gen_ups0;      /* [C0][T*u0] first upsample + noise conv */
  float* gen_last;      /* [C_last][T*upp] output of the last ResBlock stage */
} rvc_synth_taps;

int rvc_synth_create(rvc_ctx* ctx, const rvc_synth_config* cfg, rvc_synth** out);
int rvc_synth_set_tensor(rvc_synth* s, const char* name, const float* host_data, const int64_t* shape, int ndim);
int rvc_synth_finalize(rvc_synth* s);
int rvc_synth_destroy(rvc_synth* s);
int rvc_synth_upp(rvc_synth* s);
/* 1: SynthesizerTrnMs{256,768}NSFsid; 0: the no-f0 family SynthesizerTrnMs{256,768}NSFsid_nono (lib/infer_pack/models.py:812-1022),
 * decided at finalize by the checkpoint (no enc_p.emb_pitch.*, dec.m_source.*, dec.noise_convs.*).  A no-f0 model takes NULL for
 * pitch_dev, pitchf_dev and noise_src_dev in the calls below (infer(phone, phone_lengths, sid), one noise draw) and no protect blend
 * (vc_infer_pipeline.py:84,:105-108). */
int rvc_synth_has_f0(rvc_synth* s);
/* phone_dev: [T][D] row-major (reference [1,T,D]) if phone_channel_major == 0, else [D][T].
 * pitch_dev int64 [T] (coarse 1..255), pitchf_dev [T] (Hz), noise_z_dev [inter][T], noise_src_dev [T*upp]
 * (the two torch.randn_like draws of the reference, models.py:801 and :409).  out_dev [T*upp]. */
int rvc_synth_infer(rvc_synth* s, void* stream, const float* phone_dev, int phone_channel_major, const int64_t* pitch_dev,
                    const float* pitchf_dev, int sid, const float* noise_z_dev, const float* noise_src_dev, int64_t T,
                    float* out_dev, const rvc_synth_taps* taps);
/* Keep window [keep0, keep1) in frames, 0 <= keep0 < keep1 <= T: for a caller that discards the rest (VC.pipeline drops t_pad_tgt samples at either end of
 * every segment).  Only out_dev[keep0 * upp, keep1 * upp) is defined afterwards - bit for bit what rvc_synth_infer writes there; nothing is promised about
 * the other samples of out_dev [T*upp].  The text encoder, the flow and the harmonic source run at full length, the noise tensors keep their shapes; the
 * generator (conv_pre on) runs on the window widened by rvc_synth_dec_halo frames per side.  rvc_synth_infer is this call with [0, T).  With taps the
 * whole sequence is generated. */
int rvc_synth_infer_window(rvc_synth* s, void* stream, const float* phone_dev, int phone_channel_major, const int64_t* pitch_dev,
                           const float* pitchf_dev, int sid, const float* noise_z_dev, const float* noise_src_dev, int64_t T,
                           float* out_dev, const rvc_synth_taps* taps, int64_t keep0, int64_t keep1);
/* Frames of z to either side of a window that the generator's samples inside it depend on, derived from the layer table (40k_v2: 11). */
int rvc_synth_dec_halo(rvc_synth* s);
/* The frames [g0, g1) rvc_synth_infer_window generates for a keep window of a T-frame sequence in the current pair arithmetic: [keep0 - halo, keep1 + halo)
 * clamped to the sequence, g0 moved down to the next frame at which the kernels planned for the whole sequence sum every column as the full run does. */
int rvc_synth_window_frames(rvc_synth* s, int64_t T, int64_t keep0, int64_t keep1, int64_t* g0, int64_t* g1);
/* Tests only: the same call with the halo given (halo < 0: the derived one) - a halo one frame short must change samples inside the window. */
int rvc_synth_infer_window_halo(rvc_synth* s, void* stream, const float* phone_dev, int phone_channel_major, const int64_t* pitch_dev,
                                const float* pitchf_dev, int sid, const float* noise_z_dev, const float* noise_src_dev, int64_t T,
                                float* out_dev, const rvc_synth_taps* taps, int64_t keep0, int64_t keep1, int halo);

/* ---- training forward (no backward pass): SynthesizerTrnMs{256,768}NSFsid[_nono].forward for ONE item at its own length
 * (reference lib/infer_pack/models.py:665-680,:781-796,:894-903,:1000-1009): enc_p -> (m_p, logs_p); PosteriorEncoder (:199-238: pre 1x1,
 * WN(hidden, 5, 1, 16, gin), proj 1x1) -> z = m_q + noise_q exp(logs_q); the four coupling layers in the FORWARD direction, flows 0 -> 3, each followed
 * by Flip (lib/infer_pack/modules.py:436-451 with reverse=False, mean_only: x1 = m + x1) -> z_p; columns [ids, ids + seg) of z and pitchf
 * (lib/infer_pack/commons.py:150-175 slice_segments / slice_segments2) through the generator as a sequence of its own (zero padding at both cut edges,
 * the harmonic source's phase starts at the slice) -> out_dev [seg * upp].  Dropout-free arithmetic (p_dropout = 0 in every shipped configuration).
 * rvc_synth_set_tensor takes the enc_q.* tensors like every other; rvc_synth_finalize builds the posterior only when they are present (a model finalized
 * without them is what it always was and allocates nothing for it). */
int rvc_synth_has_posterior(rvc_synth* s);
typedef struct rvc_synth_forward_taps {   /* all [inter][T]; NULL = skip */
  float* z; float* z_p; float* m_p; float* logs_p; float* m_q; float* logs_q;
} rvc_synth_forward_taps;
/* phone_dev / pitch_dev / pitchf_dev / sid as rvc_synth_infer (a no-f0 model takes NULL for pitch_dev, pitchf_dev and noise_src_dev); spec_dev
 * [spec_channels][T]; noise_q_dev [inter][T] (enc_q's randn_like, models.py:237); noise_src_dev [seg * upp] (SineGen's randn_like on the slice, :409);
 * ids: first frame of the slice, 0 <= ids <= T - seg.  Errors: no posterior loaded, T < seg, ids out of range, the f0 / no-f0 argument mismatches. */
int rvc_synth_forward(rvc_synth* s, void* stream, const float* phone_dev, int phone_channel_major, const int64_t* pitch_dev, const float* pitchf_dev,
                      const float* spec_dev, int sid, const float* noise_q_dev, const float* noise_src_dev, int64_t T, int64_t ids, float* out_dev,
                      const rvc_synth_forward_taps* taps);
/* ---- the generator's backward, first step: the decoder's data pass (GeneratorNSF / Generator, reference lib/infer_pack/models.py:542-564 read backwards).
 * A tape is one item's recorded decoder pass at the handle's segment_size: created from a finalized handle with its posterior loaded, it owns the device memory of
 * every activation the backward reads and of every delta it leaves (rvc_gen_tape_bytes; 40k v2 at 32 frames: see INTEGRATION.md).  The first creation on a
 * handle also builds the backward's weight images (transposed, tap-flipped bf16 hi / lo images of the decoder's folded weights, about the decoder's weights
 * again); a handle that never creates a tape allocates nothing for any of this.  Destroy a handle's tapes before the handle.
 * Tensors are fp32 [rows][cols], read by name through rvc_gen_tape_tensor: z, har (f0 family), pre (conv_pre + cond(g), before the leaky ReLU), up{i} (stage i's
 * up-sampled sum after the noise branch), rb{i}.{j}.y{m} (m = 1, 2: the input of ResBlock j's pair m; y0 is up{i}), rb{i}.{j}.t{m} (c1(lrelu(y_m)) + b1),
 * out{i} (the stage output xs / 3), y_hat; and the deltas, the cotangent at each convolution's output: d.post (conv_post's), d.out{i} (at each ResBlock's output
 * of stage i: the stage output's cotangent / 3), d.rb{i}.{j}.t{m}, d.rb{i}.{j}.y{m}, d.up{i}, d.pre, d.cond, d.g, d.har.  An unknown name is an error. */
typedef struct rvc_gen_tape rvc_gen_tape;
int rvc_gen_tape_create(rvc_synth* s, rvc_gen_tape** out);
int rvc_gen_tape_release(rvc_gen_tape* t);
int64_t rvc_gen_tape_bytes(rvc_gen_tape* t);
int rvc_gen_tape_tensor(rvc_gen_tape* t, const char* name, float** ptr_dev, int* rows, int64_t* cols);
/* Measurement (tools/bench_gen_grad.py).  rvc_gen_tape_timing(t, 1): the passes on this tape record HIP events around the taped decoder and at the backward's stage
 * boundaries (off, the default: no event exists).  rvc_gen_tape_times waits for them and writes up to cap milliseconds to ms_host: [0] the taped decoder
 * (conv_pre .. y_hat) of the last taped forward, then the last backward's intervals in execution order - tanh + conv_post, stage n - 1 .. stage 0, conv_pre +
 * conditioning + noise branch.  Returns the number of values, 0 when nothing was recorded, -1 on error. */
int rvc_gen_tape_timing(rvc_gen_tape* t, int on);
int rvc_gen_tape_times(rvc_gen_tape* t, float* ms_host, int cap);
/* rvc_synth_forward with the decoder recorded: same arguments, same taps, but the decoder runs layer by layer (one launch per convolution, no fused ResBlock
 * kernels) and writes the tape.  out_dev is the taped y_hat: it may differ from rvc_synth_forward's by the fused kernels' rounding (both inside the 1e-3 gate);
 * a trainer uses this wave throughout, so the gradient below is exact for the wave it scored.  rvc_synth_forward itself is untouched. */
int rvc_synth_forward_tape(rvc_synth* s, void* stream, const float* phone_dev, int phone_channel_major, const int64_t* pitch_dev, const float* pitchf_dev,
                           const float* spec_dev, int sid, const float* noise_q_dev, const float* noise_src_dev, int64_t T, int64_t ids, float* out_dev,
                           const rvc_synth_forward_taps* taps, rvc_gen_tape* tape);
/* The vector-Jacobian product of the taped decoder pass: dy_hat_dev [seg * upp] -> dz_dev [inter][seg] (the sliced latent's cotangent), dcond_dev [up_init]
 * (into dec.cond's output: the float64 row sums of conv_pre's output cotangent), dg_dev [gin] (= cond_w^T dcond, into emb_g's row), dhar_dev [seg * upp] (the
 * harmonic source's; the chain through m_source belongs to the weight gradients); the last three may be NULL (the tape's d.cond, d.g and d.har are written on every call; the pointers receive copies), dhar_dev must be for a no-f0 net.  Leaky-ReLU
 * masks are read from the tape.  The ResBlock and up-sampler data gradients run on a bf16x3 MFMA kernel (conv_gen_bwd.hip); no floating-point atomics: two
 * calls give the same bits.  The weight and bias gradients are rvc_synth_dec_weight_grad's (below).  Not here: enc_q / enc_p (the flow's data pass is rvc_synth_flow_input_grad's), the optimizer.  Errors: a tape of another handle or another
 * segment, no taped forward before it, dhar from a no-f0 net.  _launch_count: the size of the plan (independent of the segment; touches no stream), -1 on error. */
int rvc_synth_dec_input_grad(rvc_synth* s, void* stream, rvc_gen_tape* tape, const float* dy_hat_dev, float* dz_dev, float* dcond_dev, float* dg_dev,
                             float* dhar_dev);
int rvc_synth_dec_input_grad_launch_count(rvc_synth* s);
/* ---- the generator's backward, second step: the decoder's weight and bias gradients.  rvc_synth_keep_parameters(s, 1) BEFORE rvc_synth_finalize makes the handle
 * keep weight_v / weight_g of dec.ups.* and dec.resblocks.* on the device (about the decoder's weights again) and makes its tapes record two more tensors, `sine`
 * [1][seg upp] (the source before m_source.l_linear; f0 family) and `g` [1][gin] (the item's emb_g row), both reached by rvc_gen_tape_tensor; every other tape
 * tensor and the taped wave keep their bits.  Without it a handle allocates and launches exactly what it did, and rvc_synth_dec_weight_grad is an error.
 * rvc_synth_dec_param_count / _param_info / _param_total list the dec.* parameter tensors, names with their "dec." prefix, in the reference module's state-dict
 * order: m_source.l_linear, noise_convs (f0 family), conv_pre, ups (bias, weight_g, weight_v), resblocks, conv_post, cond.
 * rvc_synth_dec_weight_grad: d loss / d(parameter) of every such tensor, summed over the B <= 16 items whose tapes are given (host array; each recorded by
 * rvc_synth_forward_tape and run through rvc_synth_dec_input_grad since) -> grads_dev, a HOST array of one device pointer per parameter tensor in that order,
 * each fully written.  The chain through weight norm (dim 0) is included.  Every ResBlock convolution, every up-sampler and conv_pre run on one bf16x3 MFMA GEMM
 * over all items (conv_gen_wgrad.hip: both operands split in the kernel, the leaky ReLU applied where an operand is loaded) plus one finishing launch; the
 * reduction's partial images live in a block the handle owns, at most 64 MiB.  No floating-point atomics: two calls give the same bits.  The launch count is a
 * constant of the net (_launch_count; -1 on error): it does not depend on B or on the segment.  Errors: no kept parameters, B < 1 or B > 16, a tape of another
 * handle or another segment, a tape without a taped forward or without a backward data pass after its last taped forward.
 * rvc_gen_tape_wgrad_times (timing on, the pass's FIRST tape): the last pass's intervals in milliseconds - stage 0 .. n - 1, then conv_pre and the direct kernels. */
int rvc_synth_keep_parameters(rvc_synth* s, int on);
int rvc_synth_dec_param_count(rvc_synth* s);
int rvc_synth_dec_param_info(rvc_synth* s, int k, char* name, int name_cap, int64_t* shape, int* ndim);
int64_t rvc_synth_dec_param_total(rvc_synth* s);
int rvc_synth_dec_weight_grad(rvc_synth* s, void* stream, rvc_gen_tape* const* tapes, int B, float* const* grads_dev);
int rvc_synth_dec_weight_grad_launch_count(rvc_synth* s);
int rvc_gen_tape_wgrad_times(rvc_gen_tape* t, float* ms_host, int cap);
/* ---- the generator's backward, third step: the flow's data pass (ResidualCouplingBlock, reference lib/infer_pack/models.py:150-196; ResidualCouplingLayer, WN and
 * Flip of lib/infer_pack/modules.py read backwards): the cotangent at z_p - the KL loss's, rvc_kl_loss_grad - carried to z and to the speaker embedding.
 * rvc_synth_forward_tape_flow is rvc_synth_forward_tape with one more argument: record_flow 0 is that call bit for bit (same tape, same bytes); record_flow 1
 * also records, for the item's T frames and each coupling f = 0 .. 3, what the backward reads - flow{f}.h0 [hidden][T] (pre(x0); also under flow{f}.x0),
 * flow{f}.x{i} [hidden][T] (the input of WN layer i = 0 .. 2) and flow{f}.a{i} [2 hidden][T] (in_layers[i](x{i}) plus its slice of cond_layer(g), before the gate) -
 * in a block the tape allocates when a recording forward first meets that length (rvc_gen_tape_bytes then includes it) and reaches through rvc_gen_tape_tensor.
 * The recording pass stores the 2 hidden rows that the non-recording pass gates inside the GEMM launch and gates them in a launch of its own: z_p of a recording
 * call is inside the 1e-3 gate of a non-recording call's, not promised bit-equal; the posterior's z and the taped wave do not depend on the flow and keep their
 * bits.  The first recording forward on a handle builds the pass's weight images (transposed, tap-flipped bf16 hi / lo images of the flow's folded weights).
 * rvc_synth_flow_input_grad: dz_p_dev [inter][T] -> dz_dev [inter][T], the flow's share of z's cotangent (to be added to the decoder's), and dg_dev [gin] (may
 * be NULL), its share of emb_g's row: the four couplings' cond_layer^T of the float64 row sums of d a, summed in float64 and rounded once.  The deltas stay in
 * the tape for the weight gradients: d.flow{f}.a{i} [2 hidden][T], d.flow{f}.m [inter / 2][T] (post's output cotangent), d.flow{f}.h0 [hidden][T] (pre's),
 * d.flow{f}.gc [1][6 hidden] (cond_layer's), d.flow.g [1][gin].  The transposed products run on a bf16x3 MFMA kernel (conv_flow_bwd.hip: the gate's derivative is
 * formed from the taped a where the gradient operand is gathered and split; the epilogue adds the running cotangent and applies the mask).  An item runs at its
 * own length, so every frame of the tape is inside its mask; the kernels take the length and write zero behind it.  No floating-point atomics: two calls give
 * the same bits.  _launch_count: the size of the plan, a constant of the net whatever T (touches no stream), -1 on error.  Errors: a tape of another handle, a
 * tape whose last forward did not record the flow, T other than the recorded length.  The flow's parameter gradients are rvc_synth_flow_weight_grad's (below).  Not here: enc_q / enc_p / emb_g.
 * rvc_gen_tape_flow_times (timing on): [0] the recorded flow forward, [1] the last flow backward, in milliseconds; returns the number of values, -1 on error. */
int rvc_synth_forward_tape_flow(rvc_synth* s, void* stream, const float* phone_dev, int phone_channel_major, const int64_t* pitch_dev, const float* pitchf_dev,
                                const float* spec_dev, int sid, const float* noise_q_dev, const float* noise_src_dev, int64_t T, int64_t ids, float* out_dev,
                                const rvc_synth_forward_taps* taps, rvc_gen_tape* tape, int record_flow);
int rvc_synth_flow_input_grad(rvc_synth* s, void* stream, rvc_gen_tape* tape, const float* dz_p_dev, int64_t T, float* dz_dev, float* dg_dev);
int rvc_synth_flow_input_grad_launch_count(rvc_synth* s);
int rvc_gen_tape_flow_times(rvc_gen_tape* t, float* ms_host, int cap);
/* ---- the generator's backward, fourth step: the flow's weight and bias gradients.  On a handle with kept parameters (rvc_synth_keep_parameters, which then also
 * keeps weight_v / weight_g of flow.flows.{0,2,4,6}.enc.{in_layers.*, res_skip_layers.*, cond_layer} on the device) a forward with record_flow 1 records four more
 * tensors per coupling: flow{f}.xin [inter / 2][T] (pre's input), flow{f}.out [hidden][T] (the WaveNet's summed skip output, post's input) and, written by
 * rvc_synth_flow_input_grad, d.flow{f}.x1 / d.flow{f}.x2 [hidden][T] (the x-chain cotangent at the input of layers 1 and 2) and d.flow{f}.skip [hidden][T]
 * (post^T d m).  They are copies: z_p, dz, dg and every tensor a plain handle's tape holds keep their bits, and a plain handle allocates and launches exactly
 * what it did (rvc_synth_flow_input_grad_launch_count counts the copies on a handle with kept parameters only).
 * rvc_synth_flow_param_count / _param_info / _param_total list the 100 flow.* parameter tensors in the reference module's state-dict order: per coupling pre,
 * enc.in_layers.*, enc.res_skip_layers.*, enc.cond_layer (each bias, weight_g, weight_v), post.
 * rvc_synth_flow_weight_grad: d loss / d(parameter) of every such tensor, summed over the B <= 16 items whose tapes are given, EACH AT ITS OWN LENGTH -> grads_dev,
 * a HOST array of one device pointer per tensor in that order, each fully written; the chain through weight norm (dim 0) included.  Every convolution is one
 * launch of a bf16x3 MFMA GEMM over all items (conv_flow_wgrad.hip: the reduction runs over ragged items, a stage being one item and 128 frames; a res_skip
 * layer's input tanh(a[:H]) sigmoid(a[H:]) is formed in the kernel from the taped pre-gate rows) plus one finishing launch, cond_layer one float64 launch; the
 * partial images live in the block the decoder's pass uses.  No floating-point atomics: two calls give the same bits.  _launch_count: a constant of the net (68),
 * -1 on error.  Errors: no kept parameters, B < 1 or B > 16, a tape of another handle, a tape whose last forward did not record the flow or that has not been
 * through rvc_synth_flow_input_grad since.  Not here: enc_q / enc_p / emb_g, grad_norm_g, the optimizer. */
int rvc_synth_flow_param_count(rvc_synth* s);
int rvc_synth_flow_param_info(rvc_synth* s, int k, char* name, int name_cap, int64_t* shape, int* ndim);
int64_t rvc_synth_flow_param_total(rvc_synth* s);
int rvc_synth_flow_weight_grad(rvc_synth* s, void* stream, rvc_gen_tape* const* tapes, int B, float* const* grads_dev);
int rvc_synth_flow_weight_grad_launch_count(rvc_synth* s);
/* The GEMM of that pass at any small shape, gradient launch plus finish, no weight norm:
 *   out_dev[r][c k + t] = sum_item sum_{n < n_host[item]} P[item][r][n] act(G[item])[c][n + t + off0]
 * p_dev / g_dev: HOST arrays of B <= 16 device pointers, item b dense at its own length: P [R][n_host[b]], G [C][n_host[b]] (gate 0, act = identity) or
 * [2 C][n_host[b]] (gate 1, act(G)[c] = tanh(G[c]) sigmoid(G[C + c])); elements outside [0, n_host[b]) read as zero.  R % 16 == 0, k <= 16.
 * _plan: the planner's decisions without a device (info: 8 ints as the other _plan queries, may be NULL); returns the splits, -1 when the shape does not fit. */
int rvc_gated_conv1d_weight_grad(void* stream, const float* const* p_dev, const float* const* g_dev, int B, int R, int C, int k, const int64_t* n_host, int off0,
                                 int gate, float* out_dev);
int rvc_gated_conv1d_weight_grad_plan(int B, int R, int C, int k, const int64_t* n_host, int off0, int gate, int* info);
/* The GEMM of that pass at any small shape, gradient launch plus finish, no weight norm:
 *   out_dev[r][c k + t] = sum_item sum_n a_p(P[item][r][n]) a_g(G[item][c][cstride n + tstep t + off0]),  a_x(v) = max(v, slope_x v) (slope 1: none; 0 <= slope <= 1)
 * p_dev / g_dev: HOST arrays of B <= 16 device pointers, P [R][N] and G [C][Tg] dense; elements of G outside [0, Tg) read as zero.  R % 16 == 0, k <= 16.
 * A Conv1d's weight gradient is P = delta, G = input, (cstride, tstep, off0) = (1, dilation, -pad); a ConvTranspose1d's is P = input, G = delta, (stride, 1, -pad).
 * _splits: the number of partial images the planner cuts the reduction into for the shape, -1 when the shape does not fit. */
int rvc_conv1d_weight_grad(void* stream, const float* const* p_dev, const float* const* g_dev, int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride,
                           int tstep, int off0, float slope_p, float slope_g, float* out_dev);
int rvc_conv1d_weight_grad_splits(int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride, int tstep, int off0);
/* _plan: the same query with the plan's figures in info (8 ints, or NULL), laid out as for the rvc_op_*_plan queries of the single-ops section. */
int rvc_conv1d_weight_grad_plan(int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride, int tstep, int off0, int* info);
/* kl_loss of one item (reference lib/train/losses.py:596-611): sum_dev[0] = sum over c < C, t < len of logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p)
 * (float64 accumulation, fixed order: two calls give the same bits), sum_dev[1] = len (the mask's sum); rows have pitch T_pitch >= len. */
int rvc_kl_loss(void* stream, const float* z_p_dev, const float* logs_q_dev, const float* m_p_dev, const float* logs_p_dev, int C, int64_t T_pitch,
                int64_t len, double* sum_dev);
/* The cotangents of rvc_kl_loss's sum for one item, each times scale (the caller passes weight / sum(mask)): rows c < C of pitch T_pitch, and for t < len
 *   dz_p = scale (z_p - m_p) exp(-2 logs_p), dm_p = -dz_p, dlogs_q = -scale, dlogs_p = scale (1 - (z_p - m_p)^2 exp(-2 logs_p));
 * exactly 0 for len <= t < T_pitch.  Formed in float64 from the float32 inputs and rounded once.  One launch. */
int rvc_kl_loss_grad(void* stream, const float* z_p_dev, const float* m_p_dev, const float* logs_p_dev, int C, int64_t T_pitch, int64_t len, float scale,
                     float* dz_p_dev, float* dlogs_q_dev, float* dm_p_dev, float* dlogs_p_dev);
/* sum_dev[0] = sum_i |a[i] - b[i]| over n elements, float64 accumulation in a fixed order (F.l1_loss = that / n, training_cli.py:570) */
int rvc_l1_sum(void* stream, const float* a_dev, const float* b_dev, int64_t n, double* sum_dev);

/* ------------------------------------------------------------------ discriminators (training, forward only) */
/* version 1: MultiPeriodDiscriminator (DiscriminatorS + DiscriminatorP for periods 2, 3, 5, 7, 11, 17), 2: MultiPeriodDiscriminatorV2 (+ 23, 37);
 * reference lib/infer_pack/models.py:1024-1145.  Tensor names are the reference state dict's: discriminators.<i>.convs.<l>.{weight_g, weight_v, bias} and
 * discriminators.<i>.conv_post.* (weight norm over every dimension but the first, folded by finalize), or a plain .weight; spectral-norm tensors
 * (weight_orig / weight_u) make finalize fail. */
typedef struct rvc_disc rvc_disc;
int rvc_disc_create(rvc_ctx* ctx, int version, rvc_disc** out);
int rvc_disc_set_tensor(rvc_disc* d, const char* name, const float* host_data, const int64_t* shape, int ndim);
int rvc_disc_finalize(rvc_disc* d);
int rvc_disc_release(rvc_disc* d);
/* shapes: sub-discriminators (7 or 9; 0 is DiscriminatorS), taps of sub-discriminator i (every layer's post-activation output and conv_post's output:
 * 7 for DiscriminatorS, 6 for a DiscriminatorP), and tap (i, tap) for signals of T samples: [S][C][H][p] with p = 1 for DiscriminatorS.  The score
 * of sub-discriminator i is its last tap flattened ([S][H p]).  Fails when T is not longer than the reflect pad a period needs. */
int rvc_disc_count(rvc_disc* d);
int rvc_disc_num_taps(rvc_disc* d, int i);
int rvc_disc_tap_shape(rvc_disc* d, int i, int tap, int64_t T, int* C, int* H, int* p);
/* signals_dev [S][T]: the trainer passes the B real items followed by the B generated ones (net_d(y, y_hat), training_cli.py:549,:567), so S = 2 B.
 * fmaps_dev: HOST array of one device pointer per tap, sub-discriminator-major (sum of rvc_disc_num_taps entries), each [S][C][H][p]: a layer writes its
 * tap and the next layer reads it there - the call owns no activation memory.  scores_dev: NULL, or a HOST array of rvc_disc_count device pointers
 * [S][H p] (an entry may be NULL or the last tap itself: nothing is copied then).  Every layer is one launch for all S signals. */
int rvc_disc_forward(rvc_disc* d, void* stream, const float* signals_dev, int S, int64_t T, float* const* scores_dev, float* const* fmaps_dev);
/* number of kernel launches rvc_disc_forward makes for this shape (the size of its plan; touches no stream): 6 per DiscriminatorP, 7 for
 * DiscriminatorS, whatever S; -1 on error. */
int rvc_disc_launch_count(rvc_disc* d, int S, int64_t T);
/* The GAN losses' reductions (reference lib/train/losses.py:564-593), K <= 64 tensors per call in ONE segmented float64 reduction of a fixed order (two
 * calls give the same bits).  x_dev / a_dev / b_dev, n, c: HOST arrays of K device pointers, lengths and constants; sums_dev [K] float64 on the device.
 *   rvc_sqerr_sums: sums[k] = sum_j (c[k] - x[k][j])^2     discriminator_loss (c = 1 on real scores, 0 on generated), generator_loss (c = 1)
 *   rvc_l1_sums:    sums[k] = sum_j |a[k][j] - b[k][j]|     feature_loss (the real and generated halves of every tap) */
int rvc_sqerr_sums(void* stream, const float* const* x_dev, const int64_t* n, const float* c, int K, double* sums_dev);
int rvc_l1_sums(void* stream, const float* const* a_dev, const float* const* b_dev, const int64_t* n, int K, double* sums_dev);
/* The input-gradient pass: the vector-Jacobian product of rvc_disc_forward with respect to the signals, on the feature maps that forward wrote.
 * fmaps_dev: the forward's HOST array of device pointers for these S signals (each [S][C][H][p]).  dtaps_dev: HOST array of one device pointer per tap,
 * the cotangent of that tap in the tap's shape, or NULL for zero; the last tap's is dL / dscore.  work_dev: HOST array of one device buffer per tap in
 * the tap's shape; buffer (i, l) receives dL / d(pre-activation of layer l) - the call owns no activation memory.  dsignals_dev [S][T] is fully written:
 * the sub-discriminators add into it one after the other on the stream, in index order.  The leaky ReLU's mask is taken from the saved post-activation
 * tap (slope 0.1 at exactly 0, as torch), so the pass is linear in the cotangents and exact for what the forward computed.  The dense k = 5 layers run
 * on the matrix cores (bf16x3, fp32 accumulation), one launch per layer whatever S and T; no atomics anywhere: two calls give the same bits.
 * rvc_disc_input_grad_launch_count: the size of its plan (touches no stream): 6 per DiscriminatorP, 7 for DiscriminatorS; -1 on error. */
int rvc_disc_input_grad(rvc_disc* d, void* stream, int S, int64_t T, const float* const* fmaps_dev, const float* const* dtaps_dev, float* const* work_dev,
                        float* dsignals_dev);
int rvc_disc_input_grad_launch_count(rvc_disc* d, int S, int64_t T);
/* The weight-gradient pass: dL / d(parameter) of every weight_g, weight_v (or plain weight) and bias, from the feature maps of rvc_disc_forward and the
 * per-layer deltas rvc_disc_input_grad left in work_dev for the same S signals.  OPT-IN: rvc_disc_keep_parameters(d, 1) BEFORE rvc_disc_finalize keeps
 * weight_v / weight_g on the device (about the size of the weights again) for the chain through weight norm; without it a loaded net's device memory and
 * plans are unchanged and rvc_disc_weight_grad fails.  rvc_disc_param_count / rvc_disc_param_info: the parameter tensors in the reference module's
 * state-dict order (per layer bias, weight_g, weight_v; weight, bias for a plain-weight checkpoint), name (NUL-terminated, name_cap bytes) and shape
 * (at most 8 dimensions).  grads_dev: HOST array of one device pointer per parameter tensor in that order, each fully written; the call owns no memory
 * apart from stream scratch.  dW[m][c][j] = sum_s sum_n delta[s][m][n] X[s][c][stride h' + j - pad][w], db[m] = sum_s sum_n delta[s][m][n] (float64),
 * grad_g[m] = <dW[m], v[m]> / |v[m]|, grad_v[m] = (g[m] / |v[m]|) (dW[m] - <dW[m], v[m]> / |v[m]|^2 v[m]) (torch's weight_norm(dim=0) backward).  The dense
 * k = 5 layers run on the matrix cores (bf16x3, both operands split in the kernel); every reduction is split into partial images added in index order:
 * no atomics, two calls give the same bits.  rvc_disc_weight_grad_launch_count: the size of its plan (touches no stream), two launches per layer
 * whatever S and T; -1 on error. */
int rvc_disc_keep_parameters(rvc_disc* d, int on);
int rvc_disc_param_count(rvc_disc* d);
int rvc_disc_param_info(rvc_disc* d, int k, char* name, int name_cap, int64_t* shape, int* ndim);
int rvc_disc_weight_grad(rvc_disc* d, void* stream, const float* signals_dev, int S, int64_t T, const float* const* fmaps_dev,
                         const float* const* deltas_dev, float* const* grads_dev);
int rvc_disc_weight_grad_launch_count(rvc_disc* d, int S, int64_t T);
/* The optimizer step: torch.optim.AdamW (amsgrad = False, maximize = False), float32 per element:
 *   g' = clamp(g, +-clip_value) when has_clip;  p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = v beta2 + (1 - beta2) g'^2;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),  bc_i = 1 - beta_i^step
 * Every operation is rounded on its own (no fused contraction; IEEE sqrt and division); the scalars 1 - lr wd, lr / bc1 and sqrt(bc2) are formed in double on
 * the host.  step is the step being taken (>= 1).  g is only read: the clamp happens on read.
 * rvc_adamw_step: K <= 64 tensors in ONE launch; p_dev / g_dev / m_dev / v_dev and n are HOST arrays of K device pointers and lengths.  Pointers need 4-byte
 * alignment only (a float4 body runs where the four pointers of a tensor share their offset from 16 bytes).  K > 64 fails and launches nothing. */
typedef struct rvc_adamw_hyper {
  double lr, beta1, beta2, eps, weight_decay;
  int64_t step;
  int has_clip;
  double clip_value;
} rvc_adamw_hyper;
int rvc_adamw_step(void* stream, float* const* p_dev, const float* const* g_dev, float* const* m_dev, float* const* v_dev, const int64_t* n, int K,
                   const rvc_adamw_hyper* hyper);
/* The discriminators' step (reference training_cli.py:562-563).  grads_flat_dev / exp_avg_flat_dev / exp_avg_sq_flat_dev: caller-owned flat float32 buffers of
 * rvc_disc_param_total elements in rvc_disc_param_info's order (the layout of weight_grad's buffer).  The call updates the parameters the handle holds (bias,
 * weight_g, weight_v, or the plain weight) and then, on the same stream, re-derives what the three passes read: the folded fp32 weights of the VALU layers
 * and, for the dense k = 5 layers, the forward image and the one or three transposed phase images - bit for bit what rvc_disc_finalize builds on the host from
 * the same parameters (the row norm is summed in float64 in the host's order).  Needs rvc_disc_keep_parameters(d, 1) before finalize; a plain-weight net kept
 * that way holds an fp32 master copy of its dense weights from finalize on.  rvc_disc_adamw_step_launch_count: kernel launches of one step, a constant of the
 * net (3: update, fold, images; 2 for a plain-weight net); -1 on error.  rvc_disc_get_parameters / rvc_disc_set_parameters: the parameters as one flat device
 * buffer in the same order; set re-derives weights and images with the step's kernels.  Nothing changes for a net that is never stepped. */
int rvc_disc_adamw_step(rvc_disc* d, void* stream, const float* grads_flat_dev, float* exp_avg_flat_dev, float* exp_avg_sq_flat_dev, const rvc_adamw_hyper* hyper);
int rvc_disc_adamw_step_launch_count(rvc_disc* d);
int64_t rvc_disc_param_total(rvc_disc* d);
int rvc_disc_get_parameters(rvc_disc* d, void* stream, float* flat_dev);
int rvc_disc_set_parameters(rvc_disc* d, void* stream, const float* flat_dev);
/* Cotangents of the GAN losses for K <= 64 tensors in one launch; a_dev / b_dev / out_dev, n, scale: HOST arrays of K device pointers, lengths, factors.
 *   kind 0: out = scale a             d mean(s^2) / ds with scale = 2 / numel          (discriminator_loss, generated scores)
 *   kind 1: out = -scale (1 - a)      d mean((1 - s)^2) / ds with scale = 2 / numel    (generator_loss; discriminator_loss, real scores)
 *   kind 2: out = scale sign(a - b)   d mean|r - g| / dg with a = g, b = r, scale = 1 / numel, sign(0) = 0   (feature_loss; b_dev may be NULL otherwise) */
int rvc_loss_cotangents(void* stream, int kind, const float* const* a_dev, const float* const* b_dev, const int64_t* n, const float* scale, int K,
                        float* const* out_dev);
/* out[b][t] = alpha[b] y[b][t] + (1 - alpha[b]) y_hat[b][t] (gradient_norm_loss's interpolation): every operation rounded to float32 on its own, as torch */
int rvc_interpolate(void* stream, const float* alpha_dev, const float* y_dev, const float* y_hat_dev, int B, int64_t T, float* out_dev);

/* ------------------------------------------------------------------ fused segment: VC.vc without index retrieval */
/* audio_dev [L] 16 kHz segment; pitch/pitchf as above with at least p_len = 2*T_h entries; out_dev [2*T_h*upp].
 * do_protect != 0 applies the protect blend (protect < 0.5 in the reference). */
int rvc_vc_segment(rvc_hubert* h, rvc_synth* s, void* stream, const float* audio_dev, int64_t L, int version,
                   const int64_t* pitch_dev, const float* pitchf_dev, int sid, float protect, int do_protect,
                   const float* noise_z_dev, const float* noise_src_dev, float* out_dev);

/* Same, starting from HuBERT features that already live on the device (channel-major [feat_dim][T_h]); lets the caller run
 * HuBERT on a second stream while RMVPE produces the pitch. */
int rvc_vc_segment_feats(rvc_synth* s, void* stream, const float* feats_cm_dev, const float* feats0_cm_dev, int64_t T_h, int feat_dim,
                         const int64_t* pitch_dev, const float* pitchf_dev, int sid, float protect, int do_protect,
                         const float* noise_z_dev, const float* noise_src_dev, float* out_dev);
/* feats0_cm_dev: the features before index retrieval (the reference's feats0 of the protect blend, :58-59,:89-95) or NULL when
 * no index is used. */
/* Both with a keep window in frames of the synthesizer (T = 2*T_h), as rvc_synth_infer_window: only out_dev[keep0 * upp, keep1 * upp) is defined. */
int rvc_vc_segment_window(rvc_hubert* h, rvc_synth* s, void* stream, const float* audio_dev, int64_t L, int version,
                          const int64_t* pitch_dev, const float* pitchf_dev, int sid, float protect, int do_protect,
                          const float* noise_z_dev, const float* noise_src_dev, float* out_dev, int64_t keep0, int64_t keep1);
int rvc_vc_segment_feats_window(rvc_synth* s, void* stream, const float* feats_cm_dev, const float* feats0_cm_dev, int64_t T_h, int feat_dim,
                                const int64_t* pitch_dev, const float* pitchf_dev, int sid, float protect, int do_protect,
                                const float* noise_z_dev, const float* noise_src_dev, float* out_dev, int64_t keep0, int64_t keep1);

/* ------------------------------------------------------------------ feature retrieval (vc_infer_pipeline.py:60-75) */
/* The reference looks every HuBERT frame up in a faiss IVF-Flat index over the training features big_npy [N][D]
 * (index.search(npy, k=1); pitch_extraction.py:52-73 loads it, custom_nodes/rvc_nodes.py:500-554 builds it) and blends the
 * neighbour in with weight index_rate.  rvc_index_* is that search, device resident, over the same big_npy: search returns idx [T]
 * (and optionally the squared distances faiss would report), blend writes out = index_rate * big_npy[idx] + (1 - index_rate) * feats.
 * Features are channel-major [D][T].
 * rvc_index_create: exact L2 nearest neighbour (for inputs without a cell structure: a big_npy array / the reference's preloaded tuple).
 * rvc_index_create_ivf: the semantics of the reference's own index, faiss IndexIVFFlat as RVCTrainModelNode.train_index builds it
 * ("IVF{n},Flat", nprobe 1): the nprobe centroids nearest to the query (coarse IndexFlatL2 quantiser) select the cells, only vectors of
 * those cells compete (list_of[j] = the list row j was added to); probed cells without vectors give idx -1 / score FLT_MAX and - like the
 * reference's weight arithmetic, :66-74 - a NaN frame in the blend.  nprobe <= 16, or >= nlist (= exact). */
typedef struct rvc_index rvc_index;
int rvc_index_create(rvc_ctx* ctx, const float* big_npy_host, int64_t N, int D, rvc_index** out);
int rvc_index_create_ivf(rvc_ctx* ctx, const float* big_npy_host, int64_t N, int D, const float* centroids_host /* [nlist][D] */, int nlist,
                         const int32_t* list_of_host /* [N] */, int nprobe, rvc_index** out);
int rvc_index_nprobe(const rvc_index* h);   /* 0: exact search */
int rvc_index_destroy(rvc_index* h);
int64_t rvc_index_ntotal(const rvc_index* h);
int rvc_index_search(rvc_index* h, void* stream, const float* feats_cm_dev, int64_t T, int64_t* idx_dev, float* score_dev /* may be NULL */);
int rvc_index_blend(rvc_index* h, void* stream, const float* feats_cm_dev, const int64_t* idx_dev, int64_t T, float index_rate, float* out_cm_dev);
/* Building that index (RVCTrainModelNode.train_index, custom_nodes/rvc_nodes.py:500-554, without faiss): k-means over rows_dev [N][D] (D a multiple
 * of 8) on the device.
 * rvc_kmeans_assign: label[i] = the centroid nearest to row i in squared L2 (ties: smallest index), in the arithmetic of rvc_index_search; the
 *   [K][N] scores are never stored.  dist_dev (may be NULL) receives the squared distance to that centroid.
 * rvc_kmeans_update: cent[k] = mean of the rows with label k (fp64 sum in row order, one rounding; bit-identical between runs), count[k] = their
 *   number.  Empty clusters, in increasing order, take the centroid of the then most populated cluster (smallest index on ties): the copy is
 *   multiplied by 1 + 1/1024 in even and 1 - 1/1024 in odd dimensions, the donor by the opposite factors, and the donor's count is shared
 *   (count[empty] = count[donor] / 2) - faiss Clustering.cpp::split_clusters with a fixed donor.
 * rvc_index_train: centroids = rows init_rows_host[0 .. K), then niter x (assign, update) and one last assign against the final centroids
 *   (faiss's add): label_dev is that assignment, inertia_host[i] (niter + 1 values, may be NULL) the fp64 sum of dist at assign step i.  Returns
 *   after the stream has finished. */
int rvc_kmeans_assign(rvc_ctx* ctx, void* stream, const float* rows_dev, int64_t N, int D, const float* cent_dev /* [K][D] */, int K, int32_t* label_dev,
                      float* dist_dev /* may be NULL */);
int rvc_kmeans_update(void* stream, const float* rows_dev, const int32_t* label_dev, int64_t N, int D, int K, float* cent_dev /* in: old, out: new */,
                      int32_t* count_dev);
int rvc_index_train(rvc_ctx* ctx, void* stream, const float* rows_dev, int64_t N, int D, const int64_t* init_rows_host /* [K] */, int K, int niter,
                    float* cent_dev /* [K][D] */, int32_t* label_dev, double* inertia_host /* may be NULL */);
/* Input pre-processing of VC.pipeline on the device: the zero-phase 5th-order high-pass (vc_infer_pipeline.py:19,121:
 * scipy.signal.filtfilt(bh, ah, audio) - odd extension by 18 samples, lfilter_zi initial conditions, float64), the reflect
 * padding by t_pad with the float32 cast the networks consume (:141) and the RMS frames of the filtered input that change_rms
 * uses (lib/model_utils.py:45; frame 1 s, hop 0.5 s at 16 kHz, n1 = n / 8000 + 1; may be NULL).
 * audio_dev [n] float32 (is_f64 = 0) or float64 (1); b6 / a6 / zi5 are HOST arrays (butter coefficients, lfilter_zi);
 * filt_dev [n] float64 = filtered signal, padded_dev [n + 2 t_pad] float32 (may be NULL).
 * sos18_host / sos_zi6_host (both or neither, HOST arrays): the SAME filter as three second-order sections [3][6] = {b0, b1, b2, 1, a1, a2}
 * (scipy.signal.butter(..., output="sos"); a first-order section has b2 = a2 = 0) and scipy.signal.sosfilt_zi [3][2].  With them the filter
 * runs block-propagated in the cascade form (3 launches per direction of 2 x 512 steps per thread instead of 5632: ~20 x less work at the
 * start of every conversion); equal to filtfilt(b, a) in exact arithmetic, different from scipy's transfer-function evaluation by that
 * evaluation's float64 rounding noise (~4e-8 of full scale).  Without them: the overlap-discard transfer-function kernels. */
int rvc_preprocess(void* stream, const void* audio_dev, int is_f64, int64_t n, const double* b6_host, const double* a6_host,
                   const double* zi5_host, int t_pad, double* filt_dev, float* padded_dev, double* rms1_dev, int n1,
                   const double* sos18_host, const double* sos_zi6_host);
/* Output post-processing of VC.pipeline on the device: change_rms (lib/model_utils.py:39-57; skipped when rms_mix_rate >= 1 or
 * rms1_dev == NULL) followed by peak normalisation to int16 (vc_infer_pipeline.py:188-189).  wav_dev [N] float32 is modified in
 * place; rms1_dev = RMS frames of the 16 kHz input (float64 [n1], hop 0.5 s); sr2 = output rate. */
int rvc_postprocess(void* stream, float* wav_dev, int64_t N, const double* rms1_dev, int n1, int sr2, float rms_mix_rate, int16_t* out_i16_dev);

/* ------------------------------------------------------------------ training-set preparation (reference preprocessing_utils.py:13-100) */
/* The slicer's forward high-pass: y_dev [n] float64 = scipy.signal.lfilter(bh, ah, x) from a zero state, bh, ah = butter(5, 48, "high", fs=sr),
 * with the filter given as its three normalised second-order sections sos18_host [3][6] (scipy.signal.butter(..., output="sos")) and evaluated
 * block-propagated in that cascade form (5 launches for any n).  x_dev [n] float32 (is_f64 = 0) or float64 (1).  Accurate to ~1e-13; scipy's
 * transfer-function loop carries 1e-6 .. 1e-5 of full scale of rounding noise at 32 - 48 kHz, so the two differ by THAT. */
int rvc_lfilter_hp(void* stream, const void* x_dev, int is_f64, int64_t n, const double* sos18_host, double* y_dev);
/* librosa-style centred framed RMS (lib/slicer2.py::get_rms): zero padding of win / 2 on both sides, frame j = sqrt(mean(x[j hop - win / 2 ...]^2))
 * in float64, n_frames = (n + 2 (win / 2) - win) / hop + 1.  One launch. */
int rvc_frame_rms(void* stream, const double* x_dev, int64_t n, int win, int hop, double* rms_dev, int64_t n_frames);
/* The silence scan of Slicer.slice over a HOST RMS list (no device work): the (begin, end) frame pairs of the silences to drop -> tags_host
 * [cap][2], their number -> *n_tags.  min_length / min_interval / max_sil_kept in frames, as Slicer.__init__ derives them; n_samples <=
 * min_length returns no tags (the whole recording is one clip).  cap = n_frames + 1 always suffices. */
int rvc_slice_tags(const double* rms_host, int64_t n_frames, int64_t n_samples, double threshold, int64_t min_length, int64_t min_interval,
                   int64_t max_sil_kept, int64_t* tags_host, int64_t cap, int64_t* n_tags);
/* Cuts filt_dev [n] float64 into the windows (start, length) of windows_dev [n_windows][2] (int64): gt_dev = every window cast to float32, packed
 * (total_gt = sum of lengths); y16_dev = every window resampled to target_sr exactly as rvc_resample would resample that float32 window on its
 * own (same taps, zero extension at the window's edges, ceil(length * target_sr / sr) outputs), then divided by m = max|y| / max_volume where
 * m > 1 (float32, lib/audio.py::remix_audio), packed (total_16 = sum of the output lengths).  Four launches however many windows.  Samples
 * outside [0, n) read as zero; nothing is written beyond total_gt / total_16. */
int rvc_cut_windows(void* stream, const double* filt_dev, int64_t n, const int64_t* windows_dev, int n_windows, int sr, int target_sr,
                    const double* taps_dev, int half, int up, int down, float max_volume, float* gt_dev, int64_t total_gt, float* y16_dev,
                    int64_t total_16);

/* ------------------------------------------------------------------ audio nodes (reference lib/audio.py, lib/karafan/audio_utils.py, custom_nodes/audio_nodes.py) */
/* Silence gate, step 1 (lib/karafan/audio_utils.py:129-132): for every window of `win` samples of x_dev [n] float32 (n_windows = ceil(n / win), the
 * last one may be short) the float64 sums of squares of the frames librosa.feature.rms(frame_length=win, hop_length=win) takes of that window
 * alone, centred and zero-padded: frame f covers samples [f win - win / 2, f win - win / 2 + win) of the window.  ss_dev [n_windows][2]; a
 * window of `len` samples has 1 + (len + 2 (win / 2) - win) / win frames (1 or 2), the caller ignores the other entry.  One launch. */
int rvc_gate_levels(void* stream, const float* x_dev, int64_t n, int win, double* ss_dev, int64_t n_windows);
/* Silence gate, step 2 (lib/karafan/audio_utils.py:125-165; host, no device work): the reference's loop over the window levels level_db_host
 * [n_windows] (max over the frames of 20 log10(max(1e-5, rms))) with its start / end bookkeeping and its last-window branch -> ranges_host
 * [cap][3] of (begin, end, kind), kind 0 = fade-out, 1 = zero, 2 = fade-in, ascending and disjoint; their number -> *n_ranges.
 * cap = 3 n_windows always suffices. */
int rvc_gate_ranges(const double* level_db_host, int64_t n_windows, int64_t n, int64_t win, int64_t min_size, int64_t fade, double threshold_db,
                    int64_t* ranges_host, int64_t cap, int64_t* n_ranges);
/* Silence gate, step 3 (lib/karafan/audio_utils.py:140-163): y_dev = x_dev with every range of ranges_dev [n_ranges][3] applied - the fades are
 * np.linspace(1, 0, fade) / np.linspace(0, 1, fade) in float64 multiplied into the float32 samples.  y_dev may be x_dev.  One launch. */
int rvc_gate_apply(void* stream, const float* x_dev, float* y_dev, int64_t n, const int64_t* ranges_dev, int n_ranges, int64_t fade);
/* Click removal (lib/audio.py:74-113, AudioProcessor.dynamic_thresholding / replace_clicks): mask_dev [n] (uint8) = |x| > multiplier *
 * sqrt(uniform_filter1d(x^2, size)) with scipy's "reflect" boundary and window [i - size / 2, i - size / 2 + size); the window sum in float64 over
 * the float32 squares, then float32 mean, sqrtf and multiply as the reference's float32 arrays take them.  y_dev [n] = x with the clicks replaced:
 * method 0 "median" - the median of kernel_size (odd, <= 31) neighbours of the unmodified input, reflect boundary (4 launches); method 1
 * "interpolation" - interp1d(kind="linear", fill_value="extrapolate") over the non-click samples (11 launches; with fewer than two non-click
 * samples the clicks stay).  Needs n >= size and n >= kernel_size (one reflection).  detect = 0 (replace_clicks, lib/audio.py:89-113): mask_dev
 * is the CALLER'S mask and only the fill runs; size and multiplier are not read. */
int rvc_declick(void* stream, const float* x_dev, int64_t n, int size, float multiplier, int method, int kernel_size, int detect, float* y_dev,
                uint8_t* mask_dev);
/* Peak normalisation (lib/karafan/audio_utils.py:89-107, Normalize): y = (x - mean) / max|x - mean| * gain, gain = 10^(threshold_dB / 20) as
 * float32; the mean is a float64 device reduction rounded to float32, the other steps are the reference's float32 steps; a peak of 0 leaves
 * x - mean.  y_dev may be x_dev.  3 launches. */
int rvc_peak_normalize(void* stream, const float* x_dev, int64_t n, float gain, float* y_dev);
/* The limiter at the end of lib/audio.py::remix_audio (:157-158), in place: m = max|x| / max_volume; m > 1: x / m.  2 launches. */
int rvc_peak_limit(void* stream, float* x_dev, int64_t n, float max_volume);
/* Track merge (custom_nodes/audio_nodes.py:152-170 -> lib/audio.py::pad_audio, lib/utils.py::get_merge_func): k = 2..4 float32 tracks
 * (tracks_host: k device pointers, lens_host: their lengths) zero-extended to n_out >= every length and reduced per sample by np.nanmean
 * (mode 0), np.nanmedian (1), np.nanmin (2) or np.nanmax (3) in numpy's float32 operation order; all-NaN gives NaN.  One launch. */
int rvc_merge_tracks(void* stream, const float* const* tracks_host, const int64_t* lens_host, int k, int mode, float* out_dev, int64_t n_out);
/* Segment energy (custom_nodes/audio_nodes.py:307-317, AudioBatchValueNode.get_rms over np.array_split): out_dev [k] = exact int64 sum of squares
 * of every array_split segment of x_dev [n] int16 (the first n % k segments one sample longer), k <= n.  One launch. */
int rvc_segment_energy(void* stream, const int16_t* x_dev, int64_t n, int k, int64_t* out_dev);

/* ------------------------------------------------------------------ training inputs (reference lib/train/mel_processing.py, lib/train/data_utils.py) */
/* Linear magnitude spectrograms of a ragged batch of clips (lib/train/mel_processing.py:47-87 spectrogram_torch, the spectrogram
 * TextAudioLoaderMultiNSFsid.get_audio caches, lib/train/data_utils.py:93-131; with eps = 0 and clamp = 0 the torch.abs(torch.stft(...)) of
 * mel_spectrogram_torch, :117-143): per clip F.pad(x, ((n_fft - hop) / 2,) * 2, "reflect"), frames of n_fft samples every hop, periodic Hann window
 * of n_fft, sqrt(re^2 + im^2 + eps); clamp != 0 first limits the samples to +-1.05.  One launch of an fp32 LDS FFT (radix-4 Stockham over n_fft / 2
 * packed complex values plus the real-input split; twiddles and window from float64 host tables uploaded once per (ctx, n_fft)), whatever the number
 * and the lengths of the clips.  audio_dev [n_audio] float32; clips_host [n_clips][3] int64 (HOST: the call checks every clip before it launches
 * anything and copies the table to the device itself) = (sample offset, samples N, first output column); clip c fills columns [column, column + N / hop)
 * of out_dev [n_fft / 2 + 1][pitch] float32, the reference's (Freq, Frame) layout; other columns are not touched.  n_fft 1024 or 2048 (window =
 * n_fft), 0 < hop <= n_fft with n_fft - hop even, every N > (n_fft - hop) / 2 (one reflection, as torch requires): anything else is an error and
 * launches nothing. */
int rvc_spectrogram_batch(rvc_ctx* ctx, void* stream, const float* audio_dev, int64_t n_audio, const int64_t* clips_host, int n_clips, int n_fft, int hop,
                          float eps, int clamp, float* out_dev, int64_t pitch);
/* The mel filterbank of (n_fft, n_mels) on this context (lib/train/mel_processing.py:36-39 get_mel_filters -> librosa.filters.mel) in banded form,
 * HOST arrays: row m weighs bins [first[m], first[m] + count[m]) with the next count[m] values of weights (librosa's triangles are contiguous).
 * Replaces an earlier bank of the same (n_fft, n_mels). */
int rvc_mel_filterbank_set(rvc_ctx* ctx, int n_fft, int n_mels, const int32_t* first_host, const int32_t* count_host, const float* weights_host);
/* Log-mel projection of a ragged batch (lib/train/mel_processing.py:89-96 spec_to_mel_torch, and :145-150 of mel_spectrogram_torch):
 * mel[m][t] = log(max(sum_b W[m][b] spec[b][t], 1e-5)), fp32 accumulation, for the columns of clips_host [n_clips][2] int64 (HOST) = (first column,
 * frames); spec_dev [n_fft / 2 + 1][spec_pitch], mel_dev [n_mels][mel_pitch], same columns in both.  One launch. */
int rvc_spec_to_mel_batch(rvc_ctx* ctx, void* stream, const float* spec_dev, int64_t spec_pitch, const int64_t* clips_host, int n_clips, int n_fft,
                          int n_mels, float* mel_dev, int64_t mel_pitch);
/* rvc_spectrogram_batch at the geometries of the multi-scale mel loss (lib/train/losses.py:430-561: windows 256 .. 4096 at hop = rate / 100): same
 * clip table, same output layout, same window, eps, clamp switch and magnitude.  n_fft 256, 512, 1024, 2048 or 4096; any hop > 0 with n_fft - hop even.
 * hop <= n_fft: as above (N > (n_fft - hop) / 2).  hop > n_fft: the reference's negative padding crops, so frame f starts at sample
 * f hop + (hop - n_fft) / 2, nothing is reflected and N >= hop (one frame) suffices.  N / hop frames per clip in every case.  One launch: a workgroup
 * owns 16 frames (8 at n_fft 4096, where 16 would not fit the LDS); at 256 and 512 a wave transforms four frames. */
int rvc_spectrogram_batch_ms(rvc_ctx* ctx, void* stream, const float* audio_dev, int64_t n_audio, const int64_t* clips_host, int n_clips, int n_fft, int hop,
                             float eps, int clamp, float* out_dev, int64_t pitch);
/* The vector-Jacobian product of the log-mel spectrogram: the adjoint of rvc_spectrogram_batch_ms followed by rvc_spec_to_mel_batch through the filterbank
 * set for (n_fft, n_mels).  Same clip table (HOST, [n_clips][3] = (sample offset, samples N, first column)), same geometries, same eps and clamp switches;
 * cot_mel_dev [n_mels][pitch] is the cotangent on the log-mel, clip c's frames in columns [column, column + N / hop).  d_audio_dev [n_audio]: EVERY sample
 * of every listed clip is written (the caller need not zero it; samples of no clip are not touched): the reflect padding is folded back onto the samples
 * it mirrors, samples between the frames of a hop > n_fft geometry and samples the clamp cut off (|x| > 1.05) get exactly 0, and a mel value at or above
 * the 1e-5 floor passes its cotangent (torch's clamp backward).  A workgroup redoes the forward FFT of a few frames in LDS (16 at n_fft 256 / 512, 8 at
 * 1024 / 2048, 4 at 4096), back-projects through the banded filterbank, runs the inverse transform with the uploaded twiddles and leaves the windowed
 * frame gradients in the stream's scratch; a gather kernel overlap-adds them per sample, frames in index order.  No atomics: two calls give the same
 * bits.  rvc_mel_spectrogram_vjp_launch_count() = 2 launches, whatever the number and the lengths of the clips. */
int rvc_mel_spectrogram_vjp(rvc_ctx* ctx, void* stream, const float* audio_dev, int64_t n_audio, const int64_t* clips_host, int n_clips, int n_fft, int hop,
                            float eps, int clamp, int n_mels, const float* cot_mel_dev, int64_t pitch, float* d_audio_dev);
int rvc_mel_spectrogram_vjp_launch_count(void);
/* Cotangents of the mel losses for K <= 8 pairs of log-mels in one launch; a_dev (generated) / b_dev (target) / out_dev, n, scale: HOST arrays of K device
 * pointers, lengths, factors.  out = scale d(log_weight sum loss(a, b) + mag_weight sum loss(exp a, exp b)) / da: the caller folds the means' 1 / numel
 * into scale.  loss 0 l1 (sign(0) = 0, as rvc_loss_cotangents kind 2), 1 l2, 2 smoothl1 with beta 1.  A weight <= 0 drops its term.  Every element is
 * formed in float64 from the float32 log-mels and rounded once. */
int rvc_mel_loss_cotangents(void* stream, int K, const float* const* a_dev, const float* const* b_dev, const int64_t* n, int loss, float log_weight,
                            float mag_weight, const float* scale, float* const* out_dev);
/* The K <= 8 per-scale terms of MultiScaleMelSpectrogramLoss.forward(x, y).  spec_dev[k] (HOST array of device pointers) is the magnitude spectrogram
 * [n_fft[k] / 2 + 1][pitch[k]] of the 2 B signals x_0 .. x_{B-1}, y_0 .. y_{B-1}: signal r fills columns [r row_stride[k], r row_stride[k] + nf).  Per
 * scale ONE launch projects both through the filterbank set for (n_fft[k], n_mels[k]) (log(max(., 1e-5)) as rvc_spec_to_mel_batch), forms the pointwise
 * loss (0 l1, 1 l2, 2 smoothl1 with beta 1) in fp32 and sums it in float64 in a fixed order; the log-mels are never stored.  out_dev [K][2] float64 =
 * (sum over the B n_mels nf elements of loss(log-mel x, log-mel y), the same of loss(exp(log-mel x), exp(log-mel y)) - zero unless want_mag).  K + 1 launches. */
int rvc_multiscale_mel_loss(rvc_ctx* ctx, void* stream, int K, const float* const* spec_dev, const int64_t* pitch, const int64_t* row_stride, int B, int64_t nf,
                            const int32_t* n_fft, const int32_t* n_mels, int loss, int want_mag, double* out_dev);

/* ------------------------------------------------------------------ auxiliary losses (reference lib/train/losses.py:235-277,:324-390) */
/* compute_harmonics before its min-max scaling: x_dev [B][F][T] (F, T > 14); with S = |x|, for the kernel sizes k = 3, 7, 13, 19, 29 the median of S
 * along T (harmonic) and along F (percussive) over k values, scipy.ndimage "reflect" boundaries, soft masks of power 2 and margin 1 (0.5 where both
 * medians vanish), S * mask; h_dev, p_dev [B][F][5 T] hold the five results side by side.  The medians are exact (one of the inputs); medians != 0
 * stores them (along T in h_dev, along F in p_dev) instead of the masked parts.  One launch. */
int rvc_hpss(void* stream, const float* x_dev, int B, int F, int T, float* h_dev, float* p_dev, int medians);
/* The harmonic loss of combined_aux_loss without its 5 T tensors: each of the four tensors (harmonic, percussive of org_dev and of gen_dev, [B][F][T]
 * each) is scaled by its own global min / max, (v - min) / (max - min + eps) with NaN -> eps, and sums_dev [2] float64 = (sum |gen_h - org_h|,
 * sum |gen_p - org_p|) over the B F 5 T values (fixed order).  4 launches. */
int rvc_hpss_l1(void* stream, const float* org_dev, const float* gen_dev, int B, int F, int T, float eps, double* sums_dev);
/* compute_tsi_loss before its mean: out_dev [2][B] float64 = 1 - Pearson correlation of the envelopes of org_dev and gen_dev [B][F][T] per item, row 0 for
 * dim = -1 (L2-normalise along T, max over t - 1 .. t + 1, NaN -> eps, sum along T; correlate along F), row 1 for dim = -2 (normalise and sum along
 * F; the max still runs along T, as in the reference; correlate along T).  2 max(F, T) + 2 T floats must fit 48 KB.  One launch. */
int rvc_tsi_terms(void* stream, const float* org_dev, const float* gen_dev, int B, int F, int T, float eps, double* out_dev);

/* ------------------------------------------------------------------ single ops (parity tests / kernel benchmarks) */
/* Conv1d: x_dev [Ci][Tin], w_host [Co][Ci/groups][k], y_dev [Co][Tout]; act codes: 0 none 1 lrelu 2 relu 3 gelu 4 tanh 5 sigmoid */
int rvc_op_conv1d(void* stream, const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev, float* y_dev,
                  int Ci, int Co, int Tin, int k, int stride, int pad, int dil, int groups, int pre_act, float pre_slope, int act,
                  float act_slope, int act_before_res, float out_scale, int accumulate);
/* The trainer's bf16x3 gather GEMMs at any small shape, each stated as the FORWARD operation it belongs to: weights come from the host in the module's own
 * layout and pass through the regrouping the nets use (tests/test_hip_gather_gemms.py).  Device tensors are dense fp32; the stream is synchronised on return.
 * Every entry has a pure query *_plan that needs no device: it returns what the entry reports (units per pipeline stage, or splits), -1 when the planner
 * declines the shape, and fills info (8 ints, or NULL): units, rows per workgroup, splits, grid x / y / z, pipeline stages (the fewest of any phase; for a
 * weight gradient the stages of the whole reduction), stages per split.
 *
 * rvc_op_disc_conv: y [S][Co][Hout][p] = lrelu_slope(b + conv along H of x [S][Ci][H][p]) with w_host [Co][Ci][k], stride, pad; Hout = (H + 2 pad - k) / stride + 1.
 * Ci % 16 == 0, Co % 128 == 0, k <= 16, 0 <= slope <= 1. */
int rvc_op_disc_conv(void* stream, const float* x_dev, const float* w_host, const float* bias_host, float* y_dev, int S, int Ci, int Co, int H, int p, int k,
                     int stride, int pad, float slope, int* units_out);
int rvc_op_disc_conv_plan(int S, int Ci, int Co, int H, int p, int k, int stride, int pad, int* info);
/* The data gradient of that layer for k = 5, pad = 2, stride 1 or 3, with the backward chain's epilogue: y [S][Ci][H][p] = (convT(d) + cot) * (a > 0 ? 1 : slope),
 * d_dev [S][Co][Hd][p] (Hd: the forward's output rows for H), cot_dev (or NULL) and a_dev laid out like y; w_host [Co][Ci][5], Co % 16 == 0. */
int rvc_op_disc_conv_input_grad(void* stream, const float* d_dev, const float* w_host, const float* cot_dev, const float* a_dev, float* y_dev, int S, int Ci, int Co,
                                int H, int Hd, int p, int stride, float slope, int* units_out);
int rvc_op_disc_conv_input_grad_plan(int S, int Ci, int Co, int H, int Hd, int p, int stride, int* info);
/* The weight gradient of that layer: dw_dev [Co][Ci][k] = sum over signals and outputs of d [S][Co][Hout][p] times the input x [S][Ci][H][p] the tap read (zero
 * outside the rows); gradient launch plus the nets' finishing kernel, no weight norm.  Co % 128 == 0, k <= 16. */
int rvc_op_disc_conv_weight_grad(void* stream, const float* d_dev, const float* x_dev, float* dw_dev, int S, int Ci, int Co, int H, int p, int k, int stride, int pad,
                                 int* splits_out);
int rvc_op_disc_conv_weight_grad_plan(int S, int Ci, int Co, int H, int p, int k, int stride, int pad, int* info);
/* The data gradient of the generator's 1-D convolutions with the backward chain's epilogue, y [Ci][ldY] (N columns written):
 *   y = g * (a > 0 ? scale : scale slope) + res (+ y when accumulate),  a_dev / res_dev (either may be NULL: no mask / nothing added) laid out like y,
 * g the gradient at the input of, transposed = 0: Conv1d(Ci, Co, k, dilation = step, padding = pad), w_host [Co][Ci][k], d_dev [Co][ldD] with Td = N + 2 pad -
 * (k - 1) step valid columns; transposed = 1: ConvTranspose1d(Ci, Co, k, stride = step, padding = pad), w_host [Ci][Co][k], Td = (N - 1) step - 2 pad + k.
 * Co % 16 == 0, k <= 16, pad <= (k - 1) step for a Conv1d. */
int rvc_op_conv1d_input_grad(void* stream, const float* d_dev, const float* w_host, const float* a_dev, const float* res_dev, float* y_dev, int transposed, int Ci,
                             int Co, int k, int step, int pad, int64_t N, int64_t Td, int64_t ldD, int64_t ldY, float slope, float scale, int accumulate,
                             int* bm_out, int* units_out);
int rvc_op_conv1d_input_grad_plan(int transposed, int Ci, int Co, int k, int step, int pad, int64_t N, int64_t Td, int* info);
/* k = 1 projection (torch.nn.Linear over [T, Ci] rows, reference transformers/models/hubert/modeling_hubert.py:291-477 via
 * lib/infer_pack/loaders.py:55-61) on the split-resident GEMM kernel (csrc/conv_x3s.hip): x_dev [Ci][T] fp32 is first written as the bf16
 * hi / lo image the kernel stages, y = act(W x + b [+ res]) (act_before_res: act(W x + b) + res).  y_dev fp32 [Co][T] or null;
 * ysplit_f32_dev [Co][T] or null receives the kernel's SPLIT output image read back as hi + lo.  ksplit > 0 forces the K split (reduced
 * inside the launch), am / an > 0 force the tile (64 am rows x 64 an columns).  k > 1: w_host [Co][Ci][k], a 1-D "same" convolution with
 * dilation dil whose taps are row offsets into the image (odd k, pad (k - 1) / 2 * dil <= 64). */
int rvc_op_gemm_split(void* stream, const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev, float* y_dev,
                      float* ysplit_f32_dev, int Ci, int Co, int T, int act, float act_slope, int act_before_res, float out_scale, int ksplit,
                      int am, int an, int k, int dil);
/* General stride-1 Conv1d on the same kernel, grouped and with long kernels (HuBERT's positional convolution, transformers modeling_hubert.py:
 * 61-106: Conv1d(768, 768, 128, padding 64, groups 16), output cut to T, GELU, + residual): w_host [Co][Ci / groups][k], output length T
 * (the first T positions), taps are row offsets tap * dil - pad into the zero-margined image. */
int rvc_op_conv1d_split(void* stream, const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev, float* y_dev,
                        int Ci, int Co, int T, int k, int pad, int dil, int groups, int act, int act_before_res);
/* Stride-2 Conv1d without padding on the split-resident kernel, the way HuBERT's feature-encoder layers 1 .. 6 run (transformers modeling_hubert.py HubertNoLayerNormConvLayer,
 * k = 3 / 2, stride 2, through lib/infer_pack/loaders.py:55-61): the input is turned into the DE-INTERLEAVED bf16 hi / lo image (even | odd positions) a producer's epilogue
 * would write, a tap is then a row offset; y_dev [Co][Tout] fp32, Tout = (T - k) / 2 + 1; y_img_f32_dev (or NULL): the same result read back from the de-interleaved OUTPUT
 * image (what the next stride-2 layer stages).  Test / benchmark op. */
int rvc_op_conv1d_s2_split(void* stream, const float* x_dev, const float* w_host, const float* bias_host, float* y_dev, float* y_img_f32_dev, int Ci, int Co, int T, int k,
                           int act);
/* Conv2d 3 x 3, pad 1 (reference lib/rmvpe.py:233-268 ConvBlockRes convolutions) on the same kernel over PADDED split-resident images (row pitch
 * W + 2, taps as row offsets): x_dev [Ci][H][W] plain fp32 is padded and split on the device, y = act(conv(x) + b) with the residual before
 * or after the activation, returned plain [Co][H][W]; ysplit_f32_dev as above (plain layout). */
int rvc_op_conv2d_split(void* stream, const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev, float* y_dev,
                        float* ysplit_f32_dev, int Ci, int Co, int H, int W, int act, int act_before_res, int ksplit, int am, int an);
/* ConvTranspose1d: w_host [Ci][Co][k]; y_dev [Co][(Tin-1)*u - 2*pad + k] */
int rvc_op_conv_transpose1d(void* stream, const float* x_dev, const float* w_host, const float* bias_host, float* y_dev, int Ci, int Co,
                            int Tin, int k, int u, int pad, int pre_act, float pre_slope, int accumulate);
/* Conv2d 3x3 pad 1: x_dev [Ci][H][W], w_host [Co][Ci][3][3]; ReLU-then-residual epilogue if relu != 0 */
int rvc_op_conv2d3x3(void* stream, const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev, float* y_dev,
                     int Ci, int Co, int H, int W, int relu);
/* ConvTranspose2d k3 s2 p1 op1: w_host [Ci][Co][3][3]; y_dev [Co][2H][2W] */
int rvc_op_conv_transpose2d(void* stream, const float* x_dev, const float* w_host, const float* bias_host, float* y_dev, int Ci, int Co,
                            int H, int W, int relu);
/* y[z][m][n] = sum_k a[z][k][m] * b[z][k][n] */
int rvc_op_gemm_tn(void* stream, const float* a_dev, const float* b_dev, float* y_dev, int M, int N, int K, int batch);
/* plan API for benchmarking the dominant kernel without host-side packing in the loop */
typedef struct rvc_conv1d_plan rvc_conv1d_plan;
int rvc_conv1d_plan_create(const float* w_host, const float* bias_host, int Ci, int Co, int k, int stride, int pad, int dil, int groups,
                           rvc_conv1d_plan** out);
int rvc_conv1d_plan_run(rvc_conv1d_plan* p, void* stream, const float* x_dev, int Tin, const float* res_dev, float* y_dev, int pre_act,
                        float pre_slope, int act, float act_slope);
/* One ResBlock1 pair of the generator in a single launch (reference lib/infer_pack/modules.py:295-308):
 * y = (x + conv2(lrelu(conv1(lrelu(x), dilated)))) * out_scale [+ y]; x_dev, y_dev [C][T].  Fails if the pair is not eligible. */
/* The same pair as two launches with a split-resident intermediate, the way the wide generator stages run it (reference
 * lib/infer_pack/modules.py:295-308): conv1 writes lrelu(conv1(lrelu(x)) + b1) as the bf16 hi / lo image conv2 stages by DMA.
 * Fails if the layers are not eligible for the split-resident paths at this length. */
int rvc_conv1d_plan_pair_split_run(rvc_conv1d_plan* c1, rvc_conv1d_plan* c2, void* stream, const float* x_dev, int T, float* y_dev,
                                   float out_scale, int accumulate);
int rvc_conv1d_plan_pair_run(rvc_conv1d_plan* c1, rvc_conv1d_plan* c2, void* stream, const float* x_dev, int T, float* y_dev, float out_scale,
                             int accumulate);
/* A whole ResBlock1 of the generator's 32-channel stage in ONE launch (reference lib/infer_pack/modules.py:295-308, the loop over convs1 / convs2; the
 * generator's xs += resblock(x), x = xs / 3 of models.py:555-560 is out_scale / accumulate): plans = {c1_0, c2_0, c1_1, c2_1, c1_2, c2_2};
 * y = x3 * out_scale [+ y] with x_{i+1} = x_i + c2_i(lrelu(c1_i(lrelu(x_i)))); x_dev, y_dev [32][T].  fp16x2 pair arithmetic only; bit-identical to three
 * rvc_conv1d_plan_pair_run calls.  *ran_out = 1 when the fused kernel ran, 0 when the layers / length are not eligible (nothing is written then: the caller
 * runs the pairs one by one).  noise_*_dev (all three or none): the last generator stage's noise branch (models.py GeneratorNSF.forward, x = ups(x) +
 * noise_convs[-1](har), a Conv1d(1, 32, 1)) folded into the read of x: the ResBlock sees x[c][t] + fmaf(noise_w[c], noise_src[t], noise_b[c]). */
int rvc_conv1d_plan_resblock_run(rvc_conv1d_plan* const* plans6, void* stream, const float* x_dev, int T, float* y_dev, float out_scale, int accumulate,
                                 int* ran_out, const float* noise_src_dev, const float* noise_w_dev, const float* noise_b_dev);
/* The arithmetic rvc_conv1d_plan_pair_split_run (and the generator) uses for this pair at length T under the current rvc_set_pair_arithmetic mode:
 * 1 fp16x2, 0 bf16x3 (mode 0, a layer without an fp16 image, or a length / shape the persistent kernel declines); -1 on a null argument. */
int rvc_conv1d_plan_pair_arithmetic(rvc_conv1d_plan* c1, rvc_conv1d_plan* c2, int T);
int rvc_conv1d_plan_destroy(rvc_conv1d_plan* p);
/* fused softmax(K^T Q) V + bias for head dimension 64: q_dev, k_dev channel-major [heads*64][T] (q pre-scaled), v_rm_dev row-major
 * [T][heads*64], bv_dev [heads*64] or NULL, out_dev channel-major [heads*64][T] */
int rvc_op_attention(void* stream, const float* q_dev, const float* k_dev, const float* v_rm_dev, const float* bv_dev, float* out_dev,
                     int heads, int T);
/* the synthesizer text encoder's attention (reference lib/infer_pack/attentions.py:230-267), head dimension 96, window 10:
 * softmax over keys of K^T Q + rel[k - q + 10][q] (|k - q| <= 10), times V, + bv.  rel_dev [heads][21][T] in (the Q . emb_rel_k
 * projection), pb_dev [heads][21][T] out: pb[r][q] = P[q][q + r - 10] (0 outside the sequence), the input of the rel-v projection.
 * ek_dev / ev_dev (both or neither): emb_rel_k / emb_rel_v [21][96], shared by the heads - the kernel then computes both projections itself
 * (rel = Q . E_k on the staged Q tile, out += P_band . E_v in the merge); rel_dev / pb_dev may be null in that form. */
/* attention on split-resident operands (attention_dma.hip; HuBERT's encoder layers, modeling_hubert.py:291-477): q, k, v fp32 channel-major
 * [heads*64][T]; the op builds the q / k image and the V^T image itself.  out fp32 [heads*64][T] and / or the output image read back as fp32. */
int rvc_op_attention_split(void* stream, const float* q_dev, const float* k_dev, const float* v_dev, const float* bv_dev, float* out_dev,
                           float* out_img_f32_dev, int heads, int T);
/* the text encoder's variant (head dimension 96, relative positions within +-10: reference attentions.py:230-267): ek / ev host [21][96];
 * kz > 0 forces the number of key slices merged inside the launch (0: automatic). */
int rvc_op_attention_split_rel(void* stream, const float* q_dev, const float* k_dev, const float* v_dev, const float* bv_dev, const float* ek_host,
                               const float* ev_host, float* out_dev, float* out_img_f32_dev, int heads, int T, int kz);
/* one ConvBlockRes of RMVPE's shallow U-Net levels in one launch (conv_cbr2.hip; reference lib/rmvpe.py:233-268 with BatchNorm folded):
 * y = relu(conv3x3(relu(conv3x3(x, w1) + b1), w2) + b2) + x; x, y device fp32 [C][H][W] (distinct), w host [C][C][3][3], C = 16 or 32. */
int rvc_op_cbr2_small(void* stream, const float* x_dev, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host,
                      float* y_dev, int C, int H, int W);
/* LayerNorm over channels (column-wise on [C][T]) with the split-resident image as output (layernorm_c_split_kernel: HuBERT / text-encoder layers,
 * modeling_hubert.py:291-477): y fp32 (optional) and the image read back as fp32; C a multiple of 16. */
int rvc_op_layernorm_c_split(void* stream, const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, float* y_img_f32_dev, int C, int T);
/* one 3 x 3 convolution of RMVPE's shallow levels (conv_cbr2.hip conv3_small_kernel; Ci = 16 with Co <= 64, or Ci = 32 with Co <= 32): rows below relu_rows get
 * the ReLU; rows < split_row go to y (+ res when given), the others to y2 (row - split_row): first convolution + 1 x 1 shortcut of a block in one launch. */
int rvc_op_conv3_small(void* stream, const float* x_dev, const float* w_host, const float* b_host, const float* res_dev, float* y_dev, float* y2_dev, int Ci, int Co,
                       int H, int W, int split_row, int relu_rows);
/* A WaveNet layer's in_layer with its gate in the GEMM's epilogue (reference lib/infer_pack/modules.py WN.forward: x_in = in_layers[i](x); acts =
 * fused_add_tanh_sigmoid_multiply(x_in, g_l), commons.py): y[c][t] = tanh(a[c][t] + g[c]) * sigmoid(a[H + c][t] + g[H + c]) with a = conv1d(x, w [2 H][Ci][k]) + b,
 * "same" padding; the 2 H-row tensor is never stored - the rows are packed so that a lane holds both halves of a channel - and y comes back from the image the
 * res / skip layer would stage.  g_dev [2 H] on the device (or NULL).  Test / benchmark op. */
int rvc_op_wn_in_gate_split(void* stream, const float* x_dev, const float* w_host, const float* bias_host, const float* g_dev, float* y_dev, int Ci, int H, int T, int k);
/* A fused q | k | v projection on the split-resident GEMM (the attentions of HuBERT and of the synthesizer's text encoder: transformers modeling_hubert.py HubertAttention,
 * lib/infer_pack/attentions.py:57-69): y = W x + b in ONE launch, rows [0, vt_row0) written as their bf16 hi / lo image (read back into y_img_f32_dev [vt_row0][T]), rows
 * [vt_row0, Co) written TRANSPOSED as the attention's V^T image (read back into yt_dev [ceil64(T)][Co - vt_row0]; rows T .. ceil64(T) exact zeros).  vt_row0 a multiple of
 * 128.  Test / benchmark op. */
int rvc_op_gemm_split_qkv(void* stream, const float* x_dev, const float* w_host, const float* bias_host, float* y_img_f32_dev, float* yt_dev, int Ci, int Co, int T,
                          int vt_row0);
/* the swapped product of the split-resident GEMM: yt[t][j] = sum_c x[c][t] w[row0 + j][c], j < rows (the V^T image of the attention, read back as
 * fp32 [ceil64(T)][rows]; rows t >= T are zeros).  w host [Co][Ci]. */
int rvc_op_gemm_split_swapped(void* stream, const float* x_dev, const float* w_host, float* yt_dev, int Ci, int Co, int T, int row0, int rows);
/* Test ops of the two-image split-resident product (MDX23C, csrc/model_mdx23.hip: reference lib/karafan/tfc_tdf.py:137-144, `s = shortcut(x) ... x = tfc2(x) + s`):
 * y = conv3x3(x1, w1 [Co][Ci1][3][3], zero padding) + conv1x1(x2, w2 [Co][Ci2]) as ONE launch over the padded images of x1 and x2 (plain [C][H][W] tensors in
 * and out; y_img_f32: the raw output image written beside it, read back as fp32, or null); and the swapped product with a residual in the row-major layout,
 * y[t][off + j] = sum_c x[c][t] w[j][c] + res[t][off + j] with row pitch ld (tfc_tdf.py:142, `x = x + self.tdf(x)`). */
int rvc_op_conv2d3x3_plus_1x1(void* stream, const float* x1_dev, const float* w1_host, const float* x2_dev, const float* w2_host, float* y_dev, float* y_img_f32_dev,
                              int Ci1, int Ci2, int Co, int H, int W, int ksplit);
int rvc_op_gemm_split_swapped_res(void* stream, const float* x_dev, const float* w_host, const float* res_dev, float* y_dev, int Ci, int Co, int T, int ld, int off);
int rvc_op_attention_rel(void* stream, const float* q_dev, const float* k_dev, const float* v_rm_dev, const float* bv_dev, const float* rel_dev,
                         float* pb_dev, float* out_dev, int heads, int T, const float* ek_dev, const float* ev_dev);
int rvc_op_layernorm_c(void* stream, const float* x_dev, const float* res_dev, const float* gamma_dev, const float* beta_dev, float* y_dev,
                       int C, int T);
/* optional debug outputs: rad_dev [T] per-frame phase increment, tmp_dev [T] scaled frame cumsum, phase_dev [T*upp] running phase (cycles) */
int rvc_op_sine_source(void* stream, const float* f0_dev, const float* noise_dev, float* har_dev, float* sine_dev, int T, int upp, float sr,
                       float lin_w, float lin_b, float* rad_dev, float* tmp_dev, float* phase_dev);

/* ------------------------------------------------------------------ single-op entry points of the model-glue kernels (csrc/ops.hip, csrc/split2d.hip)
 * What runs between the GEMMs, one op per call for tests/test_hip_glue_ops.py: device pointers in, scratch and images allocated inside, images handed back
 * decoded to fp32 (every image byte is 0xff before the op runs, so a row the op does not write decodes as NaN), stream synchronised on return. */
/* HuBERT feature-encoder layer 0, Conv1d(1, C, 10, stride 5, no bias) -> GroupNorm(C, C) -> GELU (eps 1e-5) from L samples of raw audio (zero beyond L):
 * out_dev fp32 [C][ld] (T1 columns written) and / or the de-interleaved image of the stride-2 consumer read back into out_img_f32_dev [C][ld] (C % 16 == 0). */
int rvc_op_hubert_conv0(void* stream, const float* audio_dev, int64_t L, const float* w_dev, const float* gamma_dev, const float* beta_dev, int C, int T1,
                        float* out_dev, float* out_img_f32_dev, int64_t ld);
/* y[t] = act(sum_c sum_j w[c][j] pre(x[c][t + j - pad])), pre = leaky ReLU of slope pre_slope, act = tanh or none; x_dev, ldx, K, pad reach the launcher
 * unchanged, *kernel_out = 1 when the four-outputs-per-thread kernel ran (K = 7, pad = 3, x_dev 16-byte aligned, ldx % 4 == 0), 0 for the one-output kernel. */
int rvc_op_conv_to1(void* stream, const float* x_dev, int64_t ldx, const float* w_dev, int Ci, int K, int pad, int T, float pre_slope, int act_tanh, float* y_dev,
                    int* kernel_out);
/* x[c][t] += b[c] + sum_j w[c][j] src[t stride + j - pad] (src zero outside [0, L)) in place; *ran_out = 0 and x untouched when the kernel declines the
 * shape (k not 1 / 4 / 8, T or ld not a multiple of 4, x_dev not 16-byte aligned). */
int rvc_op_noise_add(void* stream, float* x_dev, int64_t ld, int C, int T, const float* src_dev, int64_t L, int k, int stride, int pad, const float* w_dev,
                     const float* b_dev, int* ran_out);
/* out[b][c][r] = in[b][r][c]: row pitches ldin / ldout, batch strides bin / bout (elements) */
int rvc_op_transpose(void* stream, const float* in_dev, float* out_dev, int R, int C, int64_t ldin, int64_t ldout, int batch, int64_t bin, int64_t bout);
/* out[j][t] = src[t stride + j - pad], j < k, t < Tout; outside [0, L): zero, or reflected (reflect != 0) */
int rvc_op_frames(void* stream, const float* src_dev, float* out_dev, int L, int k, int stride, int pad, int Tout, int reflect);
/* RMVPE's U-Net input: x[t][m] = a mel[m][t'] + b for t < Tr, m < 128, t' = t reflected at the right end of the n frames; mel [128][n], x [Tr][128] */
int rvc_op_mel_to_unet(void* stream, const float* mel_dev, float* x_dev, int n, int Tr, float a, float b);
/* nearest x2 upsampling of f [D][Th] to T frames and the protect blend out = w f + (1 - w) f0 with w = 1 where pitchf >= 1, protect elsewhere
 * (do_protect; f0_dev NULL: f0 = f) */
int rvc_op_feats_prepare(void* stream, const float* f_dev, const float* f0_dev, const float* pitchf_dev, float* out_dev, int D, int Th, int T, float protect,
                         int do_protect);
/* WN gate out[c][t] = tanh(a[c][t] + g[c]) sigmoid(a[H + c][t] + g[H + c]); a [2 H][T], g [2 H]; out_dev fp32 [H][T] and / or the image form (H % 16 == 0)
 * read back into out_img_f32_dev [H][T] */
int rvc_op_wn_gate(void* stream, const float* a_dev, const float* g_dev, float* out_dev, float* out_img_f32_dev, int H, int T);
/* The level changes of RMVPE's U-Net on padded planes (row pitch W + 2, a zero column on either side; channel pitches ldx / ldy in elements).  y_dev (fp32) and
 * y_img_f32_dev (the image, read back with the same pitch ldy over the padded positions) are each optional; C % 8 == 0, % 16 for the image.
 *   pool2_pad:       AvgPool2d(2) of x [C][H][W] (x_padded: [C][H][W + 2]) -> padded level (H / 2) x (W / 2)
 *   interleave2_pad: out[c][2 h + a][2 w + b] = ph[(2 a + b) Co + c][h][w], ph padded at H x W -> level 2 H x 2 W, y padded or plain (y_padded), image padded
 *   pad2d / unpad2d: plain [C][H][W] <-> padded [C][H][W + 2] */
int rvc_op_pool2_pad(void* stream, const float* x_dev, int64_t ldx, int x_padded, int C, int H, int W, float* y_dev, float* y_img_f32_dev, int64_t ldy);
int rvc_op_interleave2_pad(void* stream, const float* ph_dev, int64_t ldp, int Co, int H, int W, float* y_dev, int y_padded, float* y_img_f32_dev, int64_t ldy);
int rvc_op_pad2d(void* stream, const float* x_dev, int64_t ldx, int C, int H, int W, float* y_dev, float* y_img_f32_dev, int64_t ldy);
int rvc_op_unpad2d(void* stream, const float* x_dev, int64_t ldx, int C, int H, int W, float* y_dev, int64_t ldy);
/* RMVPE's bidirectional GRU recurrence (hidden 256; nn.GRU gate order r, z, n) by the 16-workgroup scan alone, without the repair kernel and with the
 * product's default spin limit: gi [T][1536] = W_ih x (no bias), b_ih / b_hh [2][768], w_hh [2][768][256], out channel-major [512][T].
 * *err_out = the scan's time-out flag (0: every hand-off arrived). */
int rvc_op_gru_scan(void* stream, const float* gi_dev, const float* b_ih_dev, const float* w_hh_dev, const float* b_hh_dev, float* out_dev, int T, int* err_out);

/* Rational resampling by up/down (lowest terms): y_dev[n] = sum_m x_dev[m] * taps_dev[m*up - n*down + half], n < n_out, float64
 * accumulation, zero extension outside the input.  taps_dev: 2*half+1 float64 coefficients of a linear-phase low-pass on the
 * up-times up-sampled grid, DC gain `up`.  Replaces librosa.resample (soxr_hq) at lib/audio.py:150 (input -> 16 kHz) and
 * vc_infer_pipeline.py:186 (output -> resample_sr); the coefficients are designed on the host (comfy-rvc_amd/lib/audio.py). */
int rvc_resample(void* stream, const float* x_dev, int64_t n_in, const double* taps_dev, int half, int up, int down, float* y_dev, int64_t n_out);

/* Matrix-core arithmetic of the Conv1d layers created AFTER the call BY THE CALLING THREAD (thread-local: free-standing ops / plans,
 * and models whose context is left at mode -1; rvc_ctx_set_conv_precision is the per-handle form):
 *   0  fp32 MFMA everywhere (v_mfma_f32_32x32x2_f32; bitwise an fp32 FMA chain)
 *   1  default: every eligible layer of the models (HuBERT incl. its projections, RMVPE, the synthesizer, the feature index, MDX23C,
 *      CREPE) uses the bf16x3 split (x = hi + lo in bf16, hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation;
 *      ~1e-5 relative error per layer); grouped / Ci % 16 != 0 / under-filled launches and free-standing ops / plans stay fp32
 *   2  bf16x3 for every eligible layer (stride 1, groups 1, Ci % 16 == 0), including rvc_op_conv1d / plans (parity tests) */
int rvc_set_conv_precision(int mode);
/* Arithmetic of the generator's ResBlock pairs (reference lib/infer_pack/modules.py:295-308: x + c2(lrelu(c1(lrelu(x))))) on the persistent kernel,
 * PROCESS-WIDE, read once at the start of every conversion / plan call - a conversion uses the mode it saw when it started (switching needs no
 * reload: layers carry both weight images):
 *   1  default: fp16x2 - the weight is ONE fp16 term (2^-12 relative rounding), the activation fp16 hi + lo (22 bits), two
 *      v_mfma_f32_32x32x16_f16 per product, fp32 accumulation.  Full-size goldens stay within the 33-LSB (1e-3) gate; see DESIGN.md.
 *      Activations beyond +-131008 would saturate (fp16 range): not reachable by a tanh-terminated vocoder, and a layer whose weights
 *      exceed 60000 or are all below 2^-10 keeps mode 0 by itself.
 *   0  bf16x3 as everywhere else (three MFMAs per product, ~1e-5 relative error per layer).
 * Environment RVC_H2=0 sets the initial mode to 0.  rvc_get_pair_arithmetic returns the current mode. */
int rvc_set_pair_arithmetic(int mode);
int rvc_get_pair_arithmetic(void);

/* ------------------------------------------------------------------ kernel profiling (bench.py roofline leg) */
/* While enabled, every launch of the MFMA convolution kernels is bracketed by HIP events on its own stream and tagged with its
 * algorithmic FLOPs.  rvc_prof_collect sums them per kernel configuration into arrays of RVC_PROF_CFGS entries
 * (7 tilings x {fp32 1-D, fp32 2-D, bf16x3 1-D}, rest unused); names via rvc_prof_cfg_name. */
#define RVC_PROF_CFGS 24
int rvc_prof_enable(int on);
int rvc_prof_collect(double* ms, double* flops, int64_t* launches);
/* Same records split by roofline regime: out[cfg][0..3] = {ms, FLOPs, algorithmic HBM bytes, launches} of the launches whose
 * arithmetic intensity (FLOP per algorithmic byte: input + output + residual / accumulate operands + weights) is at or above the
 * given ridge (peak FLOP/s over peak HBM B/s of the kernel family), out[cfg][4..7] of those below it.  RVC_PROF_CFGS * 8 doubles. */
int rvc_prof_collect_ex(double* out, double ridge_fp32, double ridge_bf16x3);
const char* rvc_prof_cfg_name(int i);
/* writes one CSV row per launch recorded since rvc_prof_enable(1): kernel, tile, Ci, Co, k, dilation, stride, Tout, workgroups, us,
 * algorithmic GFLOP / MB, TFLOP/s, GB/s (profiles/ per-launch-class tables) */
int rvc_prof_dump_csv(const char* path);
/* ------------------------------------------------------------------ experiment / instrumentation hooks
 * NOT part of the product ABI: librvc_hip.so exports them only when it is built with -DRVC_EXPERIMENTS (tools/build_variant.sh: variant builds for
 * A/B timing, wait-count checks, per-phase cycle counters).  The product build also compiles every experiment knob (tile choices, kernel
 * selection, thresholds) to its default; the run-time knobs it does read are listed in INTEGRATION.md. */
#ifdef RVC_EXPERIMENTS
/* debug builds only (-DRVC_CONV_TIMING): cycle sums {blocks, prologue, stage fill, prefetch issue, MFMA, epilogue, total, -}; zeros otherwise */
int rvc_debug_conv_timing(uint64_t* out8, int reset);
/* debug builds only (-DRVC_X3P_CHECK): number of waits of the pipelined bf16x3 kernel whose compile-time vmcnt exceeded the exact
 * run-time count since the last call (must be 0); -1 in ordinary builds */
int rvc_debug_x3p_check(void);
/* kernel benchmark (tools/bench_gemm.py): `reps` back-to-back launches of the split-resident GEMM (csrc/conv_x3s.hip) for an [Co x Ci] layer
 * on T columns of device-resident random data (input image, fp32 output with a residual); ksplit / am / an as in rvc_op_gemm_split,
 * split_out != 0 writes the output as the split image (GELU epilogue) instead.  w2d > 0: a 3 x 3 convolution over a padded image of width w2d
 * (T = H (w2d + 2) positions).  nlayers distinct weight sets are cycled through (a model's layers are read once per clip: cold weights).
 * *us_out = mean microseconds per launch (HIP events). */
int rvc_debug_gemm_split_bench(void* stream, int Ci, int Co, int T, int ksplit, int am, int an, int split_out, int reps, float* us_out, int w2d,
                               int nlayers);

#endif /* RVC_EXPERIMENTS */

#ifdef __cplusplus
}
#endif
#endif /* RVC_HIP_H */
