// Internal C++ interface of the three network graphs; the extern "C" layer (rvc_api.hip) wraps these.
#pragma once
#include "model_common.h"
#include "../../include/rvc_hip.h"

namespace rvc {

typedef rvc_synth_config SynthConfig;
typedef rvc_synth_taps SynthTaps;
typedef rvc_synth_forward_taps SynthForwardTaps;
typedef rvc_hubert_taps HubertTaps;
typedef rvc_rmvpe_taps RmvpeTaps;
typedef rvc_crepe_taps CrepeTaps;

struct Synth;
Synth* synth_create(Ctx* ctx, const SynthConfig& c);
void synth_destroy(Synth* S);
void synth_set_tensor(Synth* S, const char* name, const float* d, const long long* shape, int ndim);
void synth_finalize(Synth* S);
int synth_upp(const Synth* S);
int synth_feat_dim(const Synth* S);
bool synth_has_f0(const Synth* S);      // false: *_nono family (decided by the checkpoint: no enc_p.emb_pitch)
void synth_infer(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, int sid,
                 const float* noise_z, const float* noise_src, int T, float* out, const SynthTaps* taps);
// the same with a keep window in frames: only out[keep0 upp, keep1 upp) is defined (the generator runs on the window plus synth_dec_halo_frames per side);
// halo < 0: the derived halo
void synth_infer_window(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, int sid,
                        const float* noise_z, const float* noise_src, int T, float* out, const SynthTaps* taps, long long keep0, long long keep1, int halo);
void synth_window_frames(const Synth* S, int T, long long keep0, long long keep1, int halo, int* g0, int* g1);   // the frames the generator runs on for a keep window
bool synth_has_posterior(const Synth* S); // enc_q.* were present at finalize
// the training forward of one item (reference models.py:781-796; model_synth.hip): spec [spec_channels][T], noise_q [inter][T], noise_src [seg upp], out [seg upp]
void synth_forward(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, const float* spec, int sid,
                   const float* noise_q, const float* noise_src, int T, int ids, float* out, const SynthForwardTaps* taps);
// The recorded decoder pass and its backward data pass (model_synth.hip).  A tape belongs to one handle at its segment and holds one item's decoder activations
// and deltas by name; the first creation builds the backward pass's weight images.  synth_forward_tape: synth_forward with the decoder run layer by layer into
// the tape (tape null: synth_forward itself).  synth_dec_input_grad: d y_hat [seg upp] -> dz [inter][seg], dcond [up_init], dg [gin], dhar [seg upp] (the last three
// may be null; dhar must be for a no-f0 net)
struct GenTape;
GenTape* gen_tape_create(Synth* S);
void gen_tape_destroy(GenTape* T);
size_t gen_tape_bytes(const GenTape* T);
size_t synth_gen_bwd_bytes(const Synth* S);   // device bytes of the backward pass's weight images (0 before the first tape)
void gen_tape_timing(GenTape* T, bool on);             // events around the taped decoder and at the backward's stage boundaries (off: none is created)
int gen_tape_times(GenTape* T, float* ms, int cap);    // ms[0] the taped decoder, then the backward's intervals in execution order; waits for the events
bool gen_tape_tensor(const GenTape* T, const char* name, float** p, int* rows, long long* cols);   // false: no such tensor
void synth_forward_tape(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, const float* spec,
                        int sid, const float* noise_q, const float* noise_src, int T, int ids, float* out, const SynthForwardTaps* taps, GenTape* tape,
                        bool record_flow = false);
// The flow's backward data pass on a forward recorded with record_flow (the tape then also holds, for the item's T frames, what the four couplings' backward
// reads: flow{f}.h0, flow{f}.x{i}, flow{f}.a{i}; the first such forward builds the pass's weight images): d z_p [inter][T] -> dz [inter][T] and dg [gin] (may be
// null), the flow's share of both; the deltas d.flow{f}.a{i}, d.flow{f}.m, d.flow{f}.h0, d.flow{f}.gc and d.flow.g stay in the tape.
void synth_flow_input_grad(Synth* S, hipStream_t s, GenTape* tape, const float* dzp, long long T, float* dz, float* dg);
int synth_flow_input_grad_launch_count(const Synth* S);   // pure: the size of the plan, independent of the item's length
size_t synth_flow_bwd_bytes(const Synth* S);              // device bytes of that pass's weight images (0 before the first recording forward)
int gen_tape_flow_times(GenTape* T, float* ms, int cap);  // timing on: [0] the recorded flow forward, [1] the last flow backward; waits for the events
void synth_dec_input_grad(Synth* S, hipStream_t s, GenTape* tape, const float* dy, float* dz, float* dcond, float* dg, float* dhar);
int synth_dec_input_grad_launch_count(const Synth* S);   // pure: the size of the plan, independent of the segment
// The decoder's weight-gradient pass (model_synth.hip, conv_gen_wgrad.hip): d loss / d(parameter) of every dec.* tensor summed over the B items whose tapes are
// given (each recorded, and through synth_dec_input_grad since), grads one device pointer per parameter tensor in synth_dec_param_info's order (the reference
// module's state-dict order, names with their "dec." prefix), each fully written.  Needs synth_keep_parameters(S, true) before finalize: weight_v / weight_g of
// the weight-normed layers stay on the device and a tape also records `sine` and `g` (without it nothing of a handle changes).  B <= kGenWgradMaxItems.
void synth_keep_parameters(Synth* S, bool on);
int synth_dec_param_count(const Synth* S);
void synth_dec_param_info(const Synth* S, int k, std::string& name, std::vector<long long>& shape);
long long synth_dec_param_total(const Synth* S);
size_t synth_kept_bytes(const Synth* S);
int synth_dec_weight_grad_launch_count(const Synth* S);   // pure: the size of the plan, independent of B and of the segment
void synth_dec_weight_grad(Synth* S, hipStream_t s, GenTape* const* tapes, int B, float* const* grads);
int gen_tape_wgrad_times(GenTape* T, float* ms, int cap);   // the last weight-gradient pass's intervals (its first tape, timing on): stage 0 .. n - 1, the rest
// The flow's weight-gradient pass (model_synth.hip, conv_flow_wgrad.hip): d loss / d(parameter) of every flow.* tensor (100: 25 per coupling) summed over the B
// items whose tapes are given, each at its own length (each recorded with record_flow on a handle with kept parameters - the tape then also holds flow{f}.xin,
// flow{f}.out and, after synth_flow_input_grad, d.flow{f}.x1, d.flow{f}.x2, d.flow{f}.skip - and through synth_flow_input_grad since); grads one device pointer
// per tensor in synth_flow_param_info's order (the reference module's state-dict order), each fully written.  B <= kGenWgradMaxItems.
int synth_flow_param_count(const Synth* S);
void synth_flow_param_info(const Synth* S, int k, std::string& name, std::vector<long long>& shape);
long long synth_flow_param_total(const Synth* S);
int synth_flow_weight_grad_launch_count(const Synth* S);   // pure: the size of the plan, independent of B and of the lengths
void synth_flow_weight_grad(Synth* S, hipStream_t s, GenTape* const* tapes, int B, float* const* grads);
// train_forward.hip: z = m + noise exp(logs) from stats [m | logs] (2 C rows); columns [ids, ids + seg) of x [C][T] -> y [C][seg]; the two loss reductions
void posterior_sample(hipStream_t s, const float* stats, const float* noise, float* z, int C, int T);
void segment_gather(hipStream_t s, const float* x, int C, int T, int ids, int seg, float* y);
void kl_loss_grad(hipStream_t s, const float* z_p, const float* m_p, const float* logs_p, int C, long long ldT, long long len, float scale, float* dz_p,
                  float* dlogs_q, float* dm_p, float* dlogs_p);
void kl_loss_sum(hipStream_t s, const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, int C, long long ldT, long long len, double* out2);
void l1_sum(hipStream_t s, const float* a, const float* b, long long n, double* out1);
int synth_dec_halo_frames(const Synth* S);   // pure host: frames of z the generator's output depends on to either side

// the trainer's discriminators, forward only (discriminator.hip): version 1 = MultiPeriodDiscriminator, 2 = MultiPeriodDiscriminatorV2.  signals [S][T] (the
// real items, then the generated ones); fmaps: one device pointer per tap, discriminator-major, tap (i, l) = [S][C][H][p] of disc_tap_shape; scores (or its
// entries) may be null: score i is the last tap of discriminator i, copied when a distinct buffer is given
struct Disc;
Disc* disc_create(Ctx* ctx, int version);
void disc_destroy(Disc* D);
void disc_set_tensor(Disc* D, const char* name, const float* d, const long long* shape, int ndim);
void disc_finalize(Disc* D);
int disc_count(const Disc* D);
int disc_num_taps(const Disc* D, int i);
void disc_tap_shape(const Disc* D, int i, int tap, long long T, int* C, int* H, int* p);
int disc_launch_count(const Disc* D, int S, long long T);   // size of the plan the forward launches: pure, independent of S
void disc_forward(Disc* D, hipStream_t s, const float* signals, int S, long long T, float* const* scores, float* const* fmaps);
// the vector-Jacobian product of that forward with respect to the signals: fmaps as the forward wrote them for these S signals, dtaps one cotangent per tap
// (an entry may be null: zero), work one buffer per tap in the tap's shape (receives dL / d pre-activation of its layer), dsignals [S][T] fully written
int disc_input_grad_launch_count(const Disc* D, int S, long long T);   // pure, independent of S and T
void disc_input_grad(Disc* D, hipStream_t s, int S, long long T, const float* const* fmaps, const float* const* dtaps, float* const* work, float* dsignals);
// the gradient with respect to the parameters, from the same feature maps and the deltas (`work`) of disc_input_grad over the S signals the forward saw:
// grads one device pointer per parameter tensor in disc_param_info's order (the reference module's state-dict order), each fully written.  Needs
// disc_keep_parameters(D, true) before finalize: weight_v / weight_g stay on the device for the weight-norm chain (without it nothing of a loaded net changes)
void disc_keep_parameters(Disc* D, bool on);
int disc_param_count(const Disc* D);
void disc_param_info(const Disc* D, int k, std::string& name, std::vector<long long>& shape);
int disc_weight_grad_launch_count(const Disc* D, int S, long long T);   // pure, independent of S and T: two per layer
void disc_weight_grad(Disc* D, hipStream_t s, const float* signals, int S, long long T, const float* const* fmaps, const float* const* deltas, float* const* grads);
// disc_optim.hip.  adamw_step: torch.optim.AdamW (amsgrad off, maximize off) on K <= 64 tensors in one launch, float32 per element; the arrays are on the host.
// disc_adamw_step: that update on every parameter the handle holds (grads / exp_avg / exp_avg_sq: caller-owned flat buffers in disc_param_info's order), then the
// folded weights and the weight images re-derived on the stream, bit for bit as finalize builds them.  Needs disc_keep_parameters.  The launch count is a constant
// of the net (3; 2 for a plain-weight net).  get / set: the parameters as one flat buffer in the same order; set re-derives weights and images with the same kernels
void adamw_step(hipStream_t s, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* n, int K, const rvc_adamw_hyper& h);
void disc_adamw_step(Disc* D, hipStream_t s, const float* grads, float* exp_avg, float* exp_avg_sq, const rvc_adamw_hyper& h);
int disc_adamw_step_launch_count(Disc* D);
long long disc_param_total(Disc* D);
void disc_get_parameters(Disc* D, hipStream_t s, float* flat);
void disc_set_parameters(Disc* D, hipStream_t s, const float* flat);
// cotangents of the GAN losses, K tensors per launch (kind 0: scale a; 1: -scale (1 - a); 2: scale sign(a - b)), and gradient_norm_loss's interpolation
void loss_cotangents(hipStream_t s, int kind, const float* const* a, const float* const* b, const long long* n, const float* scale, int K, float* const* out);
void interpolate_rows(hipStream_t s, const float* alpha, const float* y, const float* y_hat, int B, long long T, float* out);
// K <= 64 segments per call, out [K] float64, fixed order: sum_j (c[k] - x[k][j])^2 and sum_j |a[k][j] - b[k][j]|; pointer / length / constant arrays on the host
void sqerr_sums(hipStream_t s, const float* const* x, const long long* n, const float* c, int K, double* out);
void l1_sums(hipStream_t s, const float* const* a, const float* const* b, const long long* n, int K, double* out);

struct Hubert;
Hubert* hubert_create(Ctx* ctx);
void hubert_destroy(Hubert* H);
void hubert_set_tensor(Hubert* H, const char* name, const float* d, const long long* shape, int ndim);
void hubert_finalize(Hubert* H);
long long hubert_num_frames(long long L);
// out_rm: [T_h][D] row-major (the reference's [1,T_h,D]) or null; out_cm: channel-major [D][T_h] or null
void hubert_forward(Hubert* H, hipStream_t s, const float* audio, long long L, int version, int n_layers, float* out_rm, float* out_cm,
                    const HubertTaps* taps);

struct Rmvpe;
Rmvpe* rmvpe_create(Ctx* ctx);
void rmvpe_destroy(Rmvpe* R);
void rmvpe_set_tensor(Rmvpe* R, const char* name, const float* d, const long long* shape, int ndim);
void rmvpe_finalize(Rmvpe* R);
// mel_out [128][n], salience_out [n][360], f0_out [n] (float64); any may be null.  A failed GRU hand-off (the scan's workgroups poll each
// other) sets a sticky device flag: f0_out is then NaN and rmvpe_status reports it.
void rmvpe_forward(Rmvpe* R, hipStream_t s, const float* audio, long long L, float thred, float* mel_out, float* salience_out, double* f0_out,
                   const RmvpeTaps* taps);

// feature retrieval (index.hip): exact nearest neighbour over big_npy [N][D]
struct FeatIndex;
FeatIndex* index_create(Ctx* ctx, const float* big_npy, long long N, int D);
// the reference's own index type (faiss IndexIVFFlat): nprobe nearest centroids, then the nearest vector inside those cells only
FeatIndex* index_create_ivf(Ctx* ctx, const float* big_npy, long long N, int D, const float* centroids, int nlist, const int* list_of, int nprobe);
int index_nprobe(const FeatIndex* I);   // 0: exact search
void index_destroy(FeatIndex* I);
long long index_size(const FeatIndex* I);
int index_dim(const FeatIndex* I);
void index_search(FeatIndex* I, hipStream_t s, const float* feats_cm, int T, long long* idx, float* score);
void index_blend(FeatIndex* I, hipStream_t s, const float* feats_cm, const long long* idx, int T, float rate, float* out_cm);

// building the index (index_build.hip): k-means over rows [N][D] on the device - nearest centroid per row (ties: smallest index; dist: squared
// distance or null), centroids = fp64 means of their rows with faiss's split rule for empty clusters (bit-identical between runs), and the whole
// training: centroids from init_rows (host), niter x (assign, update), one last assign; inertia (host, niter + 1 sums of dist) may be null
void kmeans_assign(Ctx* ctx, hipStream_t s, const float* rows, long long N, int D, const float* cent, int K, int* label, float* dist);
void kmeans_update(hipStream_t s, const float* rows, const int* label, long long N, int D, int K, float* cent, int* count);
void index_train(Ctx* ctx, hipStream_t s, const float* rows, long long N, int D, const long long* init_rows, int K, int niter, float* cent, int* label,
                 double* inertia);

// training inputs (spectrogram.hip): magnitude spectrograms of a ragged batch of clips by an LDS FFT, out [n_fft / 2 + 1][pitch]; clips (HOST)
// [n_clips][3] = (sample offset, samples, first output column); one launch.  Mel: the banded filterbank of (n_fft, n_mels) is set once, then
// mel [n_mels][mel_pitch] = log(max(W spec, 1e-5)) over clips (HOST) [n_clips][2] = (first column, frames); one launch.
void spectrogram_batch(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                       int clamp, float* out, long long pitch);
void mel_filterbank_set(Ctx* ctx, int n_fft, int n_mels, const int* first, const int* count, const float* weights);
void spec_to_mel_batch(Ctx* ctx, hipStream_t s, const float* spec, long long spec_pitch, const long long* clips, int n_clips, int n_fft, int n_mels,
                       float* mel, long long mel_pitch);
void spec_state_free(Ctx* ctx);
// the adjoint of spectrogram_batch_ms followed by spec_to_mel_batch: cot [n_mels][pitch] on the log-mel -> d_audio [n_audio] (every sample of every clip is
// written); clips as spectrogram_batch, the column now the clip's first cotangent column; 2 launches
void mel_spectrogram_vjp(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                         int clamp, int n_mels, const float* cot, long long pitch, float* d_audio);
constexpr int kMelVjpLaunches = 2;
// d(log_weight mean loss(a, b) + mag_weight mean loss(exp a, exp b)) / da times scale[k] for K <= 8 pairs of log-mels; one launch
void mel_loss_cotangents(hipStream_t s, int K, const float* const* a, const float* const* b, const long long* n, int loss, float log_weight, float mag_weight,
                         const float* scale, float* const* out);
// the same for the multi-scale loss's geometries: n_fft 256 .. 4096, any hop with n_fft - hop even (hop > n_fft: frames centred in their hop, no reflection)
void spectrogram_batch_ms(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                          int clamp, float* out, long long pitch);
// K scales of MultiScaleMelSpectrogramLoss: spec[k] [n_fft[k] / 2 + 1][pitch[k]] holds 2 B rows of nf frames, row r at column r row_stride[k];
// out [K][2] float64 = sums of the pointwise loss (0 l1, 1 l2, 2 smoothl1) on the log-mels and on exp(log-mel); K + 1 launches
void multiscale_mel_loss(Ctx* ctx, hipStream_t s, int K, const float* const* spec, const long long* pitch, const long long* row_stride, int B, long long nf,
                         const int* n_fft, const int* n_mels, int loss, int want_mag, double* out);

// auxiliary losses (aux_losses.hip)
constexpr int kSegSumMax = 16;
void f64_segment_sums(hipStream_t s, const double* x, const long long* bounds, int K, double* out);      // out[k] = sum of x[bounds[k] .. bounds[k + 1]), fixed order
void hpss_parts(hipStream_t s, const float* x, int B, int F, int T, float* h, float* p, int medians);
void hpss_l1(hipStream_t s, const float* org, const float* gen, int B, int F, int T, float eps, double* out2);
void tsi_terms(hipStream_t s, const float* org, const float* gen, int B, int F, int T, float eps, double* out);

void rmvpe_decode_rm(Rmvpe* R, hipStream_t s, const float* sal_rm, long long n, float thred, double* f0);
int rmvpe_status(Rmvpe* R, hipStream_t s);                 // waits for the stream; bit 0: the last forward's GRU scan timed out
void rmvpe_debug_fault(Rmvpe* R, int fault, unsigned spin_limit);   // tests: make the next scans fail / shorten their spin limit
size_t synth_workspace(const Synth* S);
size_t hubert_workspace(const Hubert* H);
size_t rmvpe_workspace(const Rmvpe* R);

// MDX23C separation network (model_mdx23.hip): one chunk [2][hop * (dim_t - 1)] -> [S][2][chunk]
struct Mdx23;
Mdx23* mdx23_create(Ctx* ctx, const rvc_mdx23_config& c);
void mdx23_destroy(Mdx23* M);
void mdx23_set_tensor(Mdx23* M, const char* name, const float* d, const long long* shape, int ndim);
void mdx23_finalize(Mdx23* M);
void mdx23_forward(Mdx23* M, hipStream_t s, const float* audio, long long L, float* out);
void mdx23_demix(Mdx23* M, hipStream_t s, const float* mix, long long Lp, long long step, long long n_chunks, float overlap, float* acc);
void mdx23_set_streams(Mdx23* M, int k);
size_t mdx23_workspace(const Mdx23* M);

// CREPE pitch network (model_crepe.hip): probabilities [360][n] for n = crepe_num_frames(L, hop, pad) frames
struct Crepe;
Crepe* crepe_create(Ctx* ctx, int tiny);
void crepe_destroy(Crepe* M);
void crepe_set_tensor(Crepe* M, const char* name, const float* d, const long long* shape, int ndim);
void crepe_finalize(Crepe* M);
long long crepe_num_frames(long long L, int hop, int pad);
void crepe_forward(Crepe* M, hipStream_t s, const float* audio, long long L, int hop, int pad, float* probs, const CrepeTaps* taps);
size_t crepe_workspace(const Crepe* M);
void crepe_viterbi(hipStream_t s, const float* probs, int n, int lo, int hi, int* bins, float* per);   // torchcrepe.decode.viterbi + periodicity

}  // namespace rvc
