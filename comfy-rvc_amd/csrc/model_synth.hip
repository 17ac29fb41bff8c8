// SynthesizerTrnMs{256,768}NSFsid.infer as a HIP kernel graph (reference lib/infer_pack/models.py:682-693,:798-809):
// enc_p (TextEncoder + 6 relative-position attention layers) -> z_p sampling -> 4 reversed coupling layers (WN)
// -> GeneratorNSF (SineGen source, ConvTranspose1d stages, 3x ResBlock1 per stage, conv_post, tanh).
// Activations are channel-major [C][T]; weights arrive with the reference's state-dict names and are folded here.
#include "model_encoder.h"
#include "models.h"
#include "conv_kernels.h"

namespace rvc {

static OwnedConvLayer make_conv1d(const TensorStore& ts, const std::string& p, int stride, int pad, int dil, bool wn, bool bias = true,
                             float wscale = 1.f, int row0 = 0, int rows = -1, std::vector<float>* keep = nullptr) {
  std::vector<float> w; std::vector<long long> shape;
  if (wn) { const HostTensor& v = ts.get(p + ".weight_v"); w = weight_norm0(v, ts.get(p + ".weight_g")); shape = v.shape; }
  else { const HostTensor& v = ts.get(p + ".weight"); w = v.data; shape = v.shape; }
  RVC_REQUIRE(shape.size() == 3, p + ": expected a [Co][Ci][k] weight");
  int Co = (int)shape[0], Ci = (int)shape[1], k = (int)shape[2];
  std::vector<float> b;
  if (bias) b = ts.get(p + ".bias").data;
  if (rows < 0) rows = Co;
  const size_t per = (size_t)Ci * k;
  std::vector<float> ws(w.begin() + row0 * per, w.begin() + (size_t)(row0 + rows) * per);
  if (wscale != 1.f) for (auto& x : ws) x *= wscale;
  std::vector<float> bs;
  if (bias) { bs.assign(b.begin() + row0, b.begin() + row0 + rows); if (wscale != 1.f) for (auto& x : bs) x *= wscale; }
  OwnedConvLayer L;
  conv1d_layer_init(L, ws.data(), bias ? bs.data() : nullptr, rows, Ci, k, stride, pad, dil, 1);
  if (keep) *keep = std::move(ws);
  return L;
}

// modules.WN (reference lib/infer_pack/modules.py:130-209) with dilation_rate 1: n layers; the flow's couplings hold 3, the posterior encoder 16
struct WNStack {
  int n = 0;
  std::vector<OwnedConvLayer> in, res, skip;   // in_layers; res_skip_layers split into their residual (layers 0 .. n - 2) and skip rows: the plain path
  std::vector<OwnedConvLayer> in_gate;   // in_layers with their 2 H rows in wn_gate_row_order: the gate runs in the split-resident GEMM's epilogue (conv_x3s.hip), the 2 H-row tensor is never stored
  std::vector<OwnedConvLayer> rs;        // res_skip_layers 0 .. n - 2 whole (2 H rows: residual | skip): the split-resident path
  DevVec cond_w, cond_b;   // weight-normed cond_layer [2*H*n][gin]
};
struct FlowLayer {
  OwnedConvLayer pre, post;
  OwnedConvLayer post_neg; // post with negated weights (x1 - m as a plain residual add): the split-resident path (conv_x3s.hip) in the reverse direction
  WNStack wn;
};
// PosteriorEncoder (reference lib/infer_pack/models.py:199-238), built only when the checkpoint holds enc_q.*
struct Posterior {
  bool built = false;
  int spec = 0, Kp = 0;    // spectrogram rows, and the same rounded up to 32: the rows pre reads (weight columns and operand rows past `spec` are zero)
  OwnedConvLayer pre, proj;
  WNStack wn;
};
struct ResBlock { OwnedConvLayer c1[3], c2[3]; };
struct GenStage { OwnedConvLayer up, noise; DevVec noise_w, noise_b; int u = 1, k = 1, noise_k = 1, noise_s = 1; ResBlock rb[3]; };   // noise_w / _b: raw [C][k] / [C] for the streaming kernel (k <= 8)

// The decoder's backward data pass (synth_dec_input_grad).  GenHostWeights: the folded decoder weights on the HOST, kept by a finalize that loaded a posterior
// (a training checkpoint) until the first tape is created; GenBwdImages: what that creation builds from them on the device - the transposed, tap-flipped
// x3_weight_image of every ResBlock convolution and of conv_pre, the up-samplers' images, the raw noise weights.  An inference handle holds neither.
struct GenHostWeights { std::vector<float> pre; std::vector<std::vector<float>> up, noise, c1, c2; };   // c1 / c2: index (i * 3 + j) * 3 + m
struct GenBwdImages {
  bool built = false;
  DevBuf<uint16_t> pre; std::vector<DevBuf<uint16_t>> up, c1, c2; std::vector<DevVec> noise;
  size_t bytes = 0;
};
// The decoder's weight-gradient pass (synth_dec_weight_grad), opt-in through synth_keep_parameters: weight_v / weight_g of the weight-normed decoder layers on the
// device for the chain through weight norm (c1 / c2: index (i * 3 + j) * 3 + m).  DecParam: the dec.* parameter tensors in the reference module's state-dict order.
// The flow's backward data pass (synth_flow_input_grad).  FlowHostWeights: the folded weights of one coupling on the HOST, kept by a finalize that loaded a posterior
// until the first recording forward; FlowBwdImages: what that forward builds from them on the device - the transposed, tap-flipped x3_weight_image of pre, post,
// the in_layers and the res_skip layers (whole: 2 H rows, the last H).  An inference handle holds neither.
struct FlowHostWeights { std::vector<float> pre, post, in[3], rs[3]; };
struct FlowBwdImages { bool built = false; DevBuf<uint16_t> pre[4], post[4], in[4][3], rs[4][3]; size_t bytes = 0; };
struct GenKept { bool on = false; std::vector<DevVec> up_v, up_g, c1_v, c1_g, c2_v, c2_g; size_t bytes = 0; };
struct DecParam { std::string name; std::vector<long long> shape; };
// The flow's weight-gradient pass (synth_flow_weight_grad), opt-in through synth_keep_parameters as well: weight_v / weight_g of every coupling's in_layers,
// res_skip_layers and cond_layer on the device.  flow_params: the flow.* parameter tensors in the reference module's state-dict order (25 per coupling).
struct FlowKept { DevVec in_v[4][3], in_g[4][3], rs_v[4][3], rs_g[4][3], cond_v[4], cond_g[4]; };
struct SynthWeights {    // what synth_finalize builds, and what the graph has learnt about it
  DevVec emb_phone_wT, emb_phone_b, emb_pitch, emb_g;
  std::vector<EncoderLayer> enc;
  OwnedConvLayer proj;
  FlowLayer flow[4];
  Posterior post_enc;
  OwnedConvLayer conv_pre;
  DevVec dec_cond_w, dec_cond_b, conv_post_w;   // conv_post_w: raw [Ci][7] weights of the 1-channel output conv (ops.hip::conv_to1)
  std::vector<GenStage> stages;
  float lin_w = 1.f, lin_b = 0.f;
  GenHostWeights gen_host; GenBwdImages gen_bwd;
  FlowHostWeights flow_host[4]; FlowBwdImages flow_bwd;
  GenKept kept; std::vector<DecParam> dec_params; std::map<std::string, int> dec_index;
  FlowKept flow_kept; std::vector<DecParam> flow_params; std::map<std::string, int> flow_index;
  ZeroedBlock imgs;      // split-resident image block whose margins are known to be zero (split_imgs_alloc; keys: T, and the columns of the z image = the generator's window)
};
struct Synth : SynthWeights {
  Ctx* ctx = nullptr;
  Arena arena;           // activation workspace (grown on demand between launches)
  TensorStore ts;
  bool ready = false;
  // config
  int inter = 192, hidden = 192, filt = 768, n_heads = 2, n_layers = 6, ksz = 3, gin = 256, n_spk = 1, sr = 40000, feat_dim = 768;
  int up_init = 512; std::vector<int> rb_k, up_rates, up_k; std::vector<std::vector<int>> rb_d;
  int upp = 1;
  int spec_channels = 0, segment = 0;   // training forward: rows of the posterior's spectrogram, frames of the generator's slice
  bool keep_params = false;   // synth_keep_parameters: the next finalize keeps what the weight-gradient pass needs
  DevVec wgrad_part;     // the weight-gradient GEMM's partial images, every layer's in turn (at most kGenWgradPartFloats floats; grown on demand)
  bool f0 = true;        // false: the *_nono family (no pitch embedding, plain Generator: reference models.py:244-311,:812-1022)
};

Synth* synth_create(Ctx* ctx, const SynthConfig& c) {
  std::unique_ptr<Synth> S(new Synth());
  S->ctx = ctx;
  S->inter = c.inter_channels; S->hidden = c.hidden_channels; S->filt = c.filter_channels; S->n_heads = c.n_heads;
  S->n_layers = c.n_layers; S->ksz = c.kernel_size; S->gin = c.gin_channels; S->n_spk = c.spk_embed_dim; S->sr = c.sr;
  S->feat_dim = c.feat_dim; S->up_init = c.upsample_initial_channel;
  S->spec_channels = c.spec_channels; S->segment = c.segment_size;
  RVC_REQUIRE(c.n_resblock_kernels == 3, "ResBlock1 x3 expected");
  for (int i = 0; i < 3; ++i) { S->rb_k.push_back(c.resblock_kernel_sizes[i]); S->rb_d.push_back({c.resblock_dilations[i][0], c.resblock_dilations[i][1], c.resblock_dilations[i][2]}); }
  S->upp = 1;
  for (int i = 0; i < c.n_upsamples; ++i) { S->up_rates.push_back(c.upsample_rates[i]); S->up_k.push_back(c.upsample_kernel_sizes[i]); S->upp *= c.upsample_rates[i]; }
  RVC_REQUIRE(S->hidden % S->n_heads == 0, "heads must divide hidden");
  // the text encoder's relative-position attention exists for head dimension 96: every configuration the reference ships has hidden_channels 192, n_heads 2
  RVC_REQUIRE(S->hidden / S->n_heads == 96, "hidden_channels / n_heads must be 96, got " + std::to_string(S->hidden / S->n_heads));
  return S.release();
}
void synth_destroy(Synth* S) { delete S; }
void synth_set_tensor(Synth* S, const char* name, const float* d, const long long* shape, int ndim) { S->ts.set(name, d, shape, ndim); }
int synth_upp(const Synth* S) { return S->upp; }
int synth_feat_dim(const Synth* S) { return S->feat_dim; }
bool synth_has_f0(const Synth* S) { return S->f0; }
bool synth_has_posterior(const Synth* S) { return S->ready && S->post_enc.built; }
void synth_keep_parameters(Synth* S, bool on) {
  RVC_REQUIRE(!S->ready, "synth_keep_parameters: set the switch before finalize");
  S->keep_params = on;
}

// Frames of z on either side of a kept output window that the generator's result inside the window depends on (GeneratorNSF / Generator, reference
// lib/infer_pack/models.py:460-566,:244-311): the layer table walked backwards from the waveform.  h = reach in samples at the current rate.
//   conv_post (k = 7)                                  h += (k - 1) / 2
//   per stage, the widest ResBlock1                    h += sum_m [(k - 1) / 2 * d_m + (k - 1) / 2]      (convs1 dilated, convs2 plain)
//   ConvTranspose1d(k_u, stride u, padding p)          output t reads inputs q with t = q u - p + j, 0 <= j < k_u: for outputs from A u - h to B u - 1 + h (A, B whole
//                                                      input positions) that is floor((h + k_u - 1 - p) / u) inputs in front of A and ceil((h + p) / u) behind B - 1
//   conv_pre (k = 7)                                   h += (k - 1) / 2, now in frames
// The noise branch reads the harmonic source, which exists at full length: no dependence on z.  40k_v2: 3 -> 63 -> 32 -> 92 -> 47 -> 107 -> 11 -> 71 -> 8 -> 11.
int synth_dec_halo_frames(const Synth* S) {
  long long h = 3;
  for (int i = (int)S->up_rates.size() - 1; i >= 0; --i) {
    long long rb = 0;
    for (size_t j = 0; j < S->rb_k.size(); ++j) {
      long long r = 0;
      for (int d : S->rb_d[j]) r += (long long)(S->rb_k[j] - 1) / 2 * d + (S->rb_k[j] - 1) / 2;
      rb = std::max(rb, r);
    }
    h += rb;
    const long long u = S->up_rates[i], ku = S->up_k[i], p = (ku - u) / 2;
    h = std::max((h + ku - 1 - p) / u, (h + p + u - 1) / u);
  }
  return (int)(h + 3);
}

// the weight-normed layers of one modules.WN under prefix p ("flow.flows.0.enc." / "enc_q.enc."), kernel 5, dilation 1
static void make_wn(const TensorStore& ts, const std::string& p, int n, int C, WNStack& W, FlowHostWeights* keep = nullptr) {
  W.n = n;
  W.in.resize(n); W.in_gate.resize(n); W.skip.resize(n); W.res.resize(n - 1); W.rs.resize(n - 1);
  for (int i = 0; i < n; ++i) {
    W.in[i] = make_conv1d(ts, p + "in_layers." + std::to_string(i), 1, 2, 1, true, true, 1.f, 0, -1, keep ? &keep->in[i] : nullptr);
    if ((C & 15) == 0) {
      const std::string q = p + "in_layers." + std::to_string(i);
      const HostTensor& v = ts.get(q + ".weight_v");
      const std::vector<float> w = weight_norm0(v, ts.get(q + ".weight_g"));
      const std::vector<float>& b = ts.get(q + ".bias").data;
      const int Ci = (int)v.shape[1], k = (int)v.shape[2];
      RVC_REQUIRE((int)v.shape[0] == 2 * C, q + ": expected 2 H rows");
      std::vector<float> wp(w.size()), bp(b.size());
      for (int r = 0; r < 2 * C; ++r) {
        const int src = wn_gate_row_order(r, C);
        std::copy(w.begin() + (size_t)src * Ci * k, w.begin() + (size_t)(src + 1) * Ci * k, wp.begin() + (size_t)r * Ci * k);
        bp[r] = b[src];
      }
      conv1d_layer_init(W.in_gate[i], wp.data(), bp.data(), 2 * C, Ci, k, 1, 2, 1, 1);
    }
    const std::string rs = p + "res_skip_layers." + std::to_string(i);
    if (i < n - 1) {
      W.res[i] = make_conv1d(ts, rs, 1, 0, 1, true, true, 1.f, 0, C);
      W.skip[i] = make_conv1d(ts, rs, 1, 0, 1, true, true, 1.f, C, C);
      W.rs[i] = make_conv1d(ts, rs, 1, 0, 1, true, true, 1.f, 0, -1, keep ? &keep->rs[i] : nullptr);
    } else {
      W.skip[i] = make_conv1d(ts, rs, 1, 0, 1, true, true, 1.f, 0, -1, keep ? &keep->rs[i] : nullptr);
    }
  }
  W.cond_w.upload(weight_norm0(ts.get(p + "cond_layer.weight_v"), ts.get(p + "cond_layer.weight_g")));
  W.cond_b.upload(ts.get(p + "cond_layer.bias").data);
  RVC_REQUIRE(W.cond_b.n == (size_t)2 * C * n, p + "cond_layer: expected 2 H n rows");
}

void synth_finalize(Synth* S) {
  S->ready = false; static_cast<SynthWeights&>(*S) = {};   // a finalize that throws leaves the handle not ready
  const TensorStore& ts = S->ts;
  // every eligible Conv1d (stride 1, groups 1, Ci % 16 == 0) also gets a bf16x3 split weight image: the generator ResBlocks
  // (70 % of a clip's FLOPs), flow WaveNet, enc_p projections; conv_x3.hip, ~1e-5 relative error per layer
  ConvBuildScope x3scope(S->ctx->precision);
  const int C = S->hidden, kc = C / S->n_heads;
  {
    const HostTensor& w = ts.get("enc_p.emb_phone.weight", {C, S->feat_dim});
    S->emb_phone_wT.upload(transpose2d(w.data.data(), C, S->feat_dim));
    S->emb_phone_b.upload(ts.get("enc_p.emb_phone.bias", {C}).data);
    // the checkpoint decides the family, like `cpt["f0"]` does in the reference (vc_infer_pipeline.py:202-218)
    S->f0 = ts.has("enc_p.emb_pitch.weight");
    if (S->f0) S->emb_pitch.upload(ts.get("enc_p.emb_pitch.weight", {256, C}).data);
    S->emb_g.upload(ts.get("emb_g.weight").data);
    S->n_spk = (int)ts.get("emb_g.weight").shape[0];
  }
  S->enc.resize(S->n_layers);
  const float qscale = 1.f / std::sqrt((float)kc);
  for (int l = 0; l < S->n_layers; ++l) {
    EncoderLayer& e = S->enc[l];
    const std::string p = "enc_p.encoder.attn_layers." + std::to_string(l) + ".";
    const HostTensor& wq = ts.get(p + "conv_q.weight", {C, C, 1});
    const HostTensor& wk = ts.get(p + "conv_k.weight", {C, C, 1});
    // one C -> 3 C projection: q (scaled), k, v rows; v's bias is added after the attention
    const HostTensor& wv = ts.get(p + "conv_v.weight", {C, C, 1});
    std::vector<float> w(3 * (size_t)C * C), b(3 * (size_t)C, 0.f);
    for (size_t i = 0; i < (size_t)C * C; ++i) { w[i] = wq.data[i] * qscale; w[(size_t)C * C + i] = wk.data[i]; w[2 * (size_t)C * C + i] = wv.data[i]; }
    const HostTensor& bq = ts.get(p + "conv_q.bias", {C}); const HostTensor& bk = ts.get(p + "conv_k.bias", {C});
    for (int i = 0; i < C; ++i) { b[i] = bq.data[i] * qscale; b[C + i] = bk.data[i]; }
    conv1d_layer_init(e.qkv, w.data(), b.data(), 3 * C, C, 1, 1, 0, 1, 1);
    e.bv.upload(ts.get(p + "conv_v.bias", {C}).data);
    const HostTensor& rk = ts.get(p + "emb_rel_k", {1, 21, kc});
    const HostTensor& rv = ts.get(p + "emb_rel_v", {1, 21, kc});
    e.ek.upload(rk.data); e.ev.upload(rv.data);
    std::vector<uint16_t> eki, evi;
    attention_rel_images(rk.data.data(), rv.data.data(), kc, 10, eki, evi);
    e.evt_off = eki.size() * 2;
    eki.insert(eki.end(), evi.begin(), evi.end());
    e.rel_img.upload(reinterpret_cast<const float*>(eki.data()), eki.size() / 2);
    e.o = make_conv1d(ts, p + "conv_o", 1, 0, 1, false);
    const std::string f = "enc_p.encoder.ffn_layers." + std::to_string(l) + ".";
    e.ff1 = make_conv1d(ts, f + "conv_1", 1, (S->ksz - 1) / 2, 1, false);
    e.ff2 = make_conv1d(ts, f + "conv_2", 1, (S->ksz - 1) / 2, 1, false);
    RVC_REQUIRE(S->ksz % 2 == 1, "enc_p FFN kernel must be odd (symmetric same-padding)");
    e.g1.upload(ts.get("enc_p.encoder.norm_layers_1." + std::to_string(l) + ".gamma", {C}).data);
    e.b1.upload(ts.get("enc_p.encoder.norm_layers_1." + std::to_string(l) + ".beta", {C}).data);
    e.g2.upload(ts.get("enc_p.encoder.norm_layers_2." + std::to_string(l) + ".gamma", {C}).data);
    e.b2.upload(ts.get("enc_p.encoder.norm_layers_2." + std::to_string(l) + ".beta", {C}).data);
  }
  S->proj = make_conv1d(ts, "enc_p.proj", 1, 0, 1, false);
  const bool keep = ts.has("enc_q.pre.weight");   // a training checkpoint: the folded flow and decoder weights stay on the host for the backward passes' images
  for (int f = 0; f < 4; ++f) {
    FlowLayer& F = S->flow[f];
    FlowHostWeights* FH = keep ? &S->flow_host[f] : nullptr;
    const std::string p = "flow.flows." + std::to_string(2 * f) + ".";
    F.pre = make_conv1d(ts, p + "pre", 1, 0, 1, false, true, 1.f, 0, -1, keep ? &FH->pre : nullptr);
    F.post = make_conv1d(ts, p + "post", 1, 0, 1, false, true, 1.f, 0, -1, keep ? &FH->post : nullptr);
    F.post_neg = make_conv1d(ts, p + "post", 1, 0, 1, false, true, -1.f);
    make_wn(ts, p + "enc.", 3, C, F.wn, FH);
  }
  Posterior& Q = S->post_enc;
  if (ts.has("enc_q.pre.weight")) {
    // pre is a 1 x 1 projection with K = spec_channels (1025 / 513): no multiple of the 16 / 32 the GEMM family tiles K by.  The layer is built over Kp = K
    // rounded up to 32 with ZERO weight columns behind K, and synth_forward hands it an operand whose rows behind K are zero too (0 * 0, never 0 * garbage)
    const HostTensor& w = ts.get("enc_q.pre.weight");
    RVC_REQUIRE(w.shape.size() == 3 && w.shape[0] == C && w.shape[2] == 1, "enc_q.pre.weight: expected [hidden][spec_channels][1]");
    Q.spec = (int)w.shape[1];
    RVC_REQUIRE(S->spec_channels == 0 || S->spec_channels == Q.spec, "enc_q.pre.weight does not have spec_channels input rows");
    Q.Kp = (Q.spec + 31) & ~31;
    std::vector<float> wp((size_t)C * Q.Kp, 0.f);
    for (int r = 0; r < C; ++r) std::copy(w.data.begin() + (size_t)r * Q.spec, w.data.begin() + (size_t)(r + 1) * Q.spec, wp.begin() + (size_t)r * Q.Kp);
    conv1d_layer_init(Q.pre, wp.data(), ts.get("enc_q.pre.bias", {C}).data.data(), C, Q.Kp, 1, 1, 0, 1, 1);
    make_wn(ts, "enc_q.enc.", 16, C, Q.wn);
    Q.proj = make_conv1d(ts, "enc_q.proj", 1, 0, 1, false);
    RVC_REQUIRE(Q.proj.Co == 2 * S->inter && Q.proj.Ci == C, "enc_q.proj: expected [2 inter][hidden][1]");
    Q.built = true;
  }
  RVC_REQUIRE(keep == Q.built, "enc_q.pre.weight decides whether a posterior is built");   // (gen_bwd_build, flow_bwd_build)
  GenHostWeights& GH = S->gen_host;
  S->conv_pre = make_conv1d(ts, "dec.conv_pre", 1, 3, 1, false, true, 1.f, 0, -1, keep ? &GH.pre : nullptr);
  S->conv_post_w.upload(ts.get("dec.conv_post.weight").data);
  S->dec_cond_w.upload(ts.get("dec.cond.weight").data);
  S->dec_cond_b.upload(ts.get("dec.cond.bias").data);
  if (S->f0) {
    S->lin_w = ts.get("dec.m_source.l_linear.weight").data[0];
    S->lin_b = ts.get("dec.m_source.l_linear.bias").data[0];
  }
  const int nu = (int)S->up_rates.size();
  S->stages.resize(nu);
  if (keep) { GH.up.resize(nu); GH.noise.resize(nu); GH.c1.resize((size_t)nu * 9); GH.c2.resize((size_t)nu * 9); }
  for (int i = 0; i < nu; ++i) {
    GenStage& st = S->stages[i];
    const int cin = S->up_init >> i, cout = S->up_init >> (i + 1);
    st.u = S->up_rates[i]; st.k = S->up_k[i];
    const std::string up = "dec.ups." + std::to_string(i);
    const HostTensor& v = ts.get(up + ".weight_v", {cin, cout, st.k});
    std::vector<float> w = weight_norm0(v, ts.get(up + ".weight_g"));
    tconv1d_layer_init(st.up, w.data(), ts.get(up + ".bias", {cout}).data.data(), cin, cout, st.k, st.u, (st.k - st.u) / 2);
    if (keep) GH.up[i] = w;
    int sf0 = 1;
    for (int j = i + 1; j < nu; ++j) sf0 *= S->up_rates[j];
    const std::string nc = "dec.noise_convs." + std::to_string(i);
    if (i + 1 < nu) { st.noise_k = 2 * sf0; st.noise_s = sf0; } else { st.noise_k = 1; st.noise_s = 1; }
    if (S->f0) {
      const HostTensor& nw = ts.get(nc + ".weight", {cout, 1, st.noise_k});
      // Conv1d(1, C, k, stride) == Linear(k -> C) on the im2col frames of the source
      conv1d_layer_init(st.noise, nw.data.data(), ts.get(nc + ".bias", {cout}).data.data(), cout, st.noise_k, 1, 1, 0, 1, 1);
      if (keep) GH.noise[i] = nw.data;
      if (st.noise_k <= 8) { st.noise_w.upload(nw.data); st.noise_b.upload(ts.get(nc + ".bias", {cout}).data); }
    }
    for (int j = 0; j < 3; ++j) {
      const std::string rb = "dec.resblocks." + std::to_string(i * 3 + j) + ".";
      const int k = S->rb_k[j];
      for (int m = 0; m < 3; ++m) {
        const int d = S->rb_d[j][m];
        const size_t q = (size_t)(i * 3 + j) * 3 + m;
        st.rb[j].c1[m] = make_conv1d(ts, rb + "convs1." + std::to_string(m), 1, (k * d - d) / 2, d, true, true, 1.f, 0, -1, keep ? &GH.c1[q] : nullptr);
        st.rb[j].c2[m] = make_conv1d(ts, rb + "convs2." + std::to_string(m), 1, (k - 1) / 2, 1, true, true, 1.f, 0, -1, keep ? &GH.c2[q] : nullptr);
      }
    }
  }
  // the dec.* parameter tensors in the reference module's state-dict order; with keep_params: weight_v / weight_g of the weight-normed layers stay on the device
  {
    GenKept& K = S->kept;
    K.on = S->keep_params;
    auto add = [&](const std::string& name) {
      const HostTensor& t = ts.get(name);
      S->dec_index[name] = (int)S->dec_params.size();
      S->dec_params.push_back({name, t.shape});
    };
    auto add_wn = [&](const std::string& p, DevVec* v, DevVec* g) {
      add(p + ".bias"); add(p + ".weight_g"); add(p + ".weight_v");
      if (K.on) { v->upload(ts.get(p + ".weight_v").data); g->upload(ts.get(p + ".weight_g").data); K.bytes += (v->n + g->n) * sizeof(float); }
    };
    if (K.on) { K.up_v.resize(nu); K.up_g.resize(nu); K.c1_v.resize((size_t)nu * 9); K.c1_g.resize((size_t)nu * 9); K.c2_v.resize((size_t)nu * 9); K.c2_g.resize((size_t)nu * 9); }
    if (S->f0) {
      add("dec.m_source.l_linear.weight"); add("dec.m_source.l_linear.bias");
      for (int i = 0; i < nu; ++i) { add("dec.noise_convs." + std::to_string(i) + ".weight"); add("dec.noise_convs." + std::to_string(i) + ".bias"); }
    }
    add("dec.conv_pre.weight"); add("dec.conv_pre.bias");
    for (int i = 0; i < nu; ++i) add_wn("dec.ups." + std::to_string(i), K.on ? &K.up_v[i] : nullptr, K.on ? &K.up_g[i] : nullptr);
    for (int n = 0; n < nu * 3; ++n)
      for (int c = 1; c <= 2; ++c)
        for (int m = 0; m < 3; ++m) {
          const size_t q = (size_t)n * 3 + m;
          add_wn("dec.resblocks." + std::to_string(n) + ".convs" + std::to_string(c) + "." + std::to_string(m),
                 !K.on ? nullptr : (c == 1 ? &K.c1_v[q] : &K.c2_v[q]), !K.on ? nullptr : (c == 1 ? &K.c1_g[q] : &K.c2_g[q]));
        }
    add("dec.conv_post.weight"); add("dec.cond.weight"); add("dec.cond.bias");
  }
  // the flow.* parameter tensors likewise: per coupling pre, enc.in_layers.*, enc.res_skip_layers.*, enc.cond_layer, post
  {
    GenKept& K = S->kept; FlowKept& FK = S->flow_kept;
    auto add = [&](const std::string& name) {
      const HostTensor& t = ts.get(name);
      S->flow_index[name] = (int)S->flow_params.size();
      S->flow_params.push_back({name, t.shape});
    };
    auto add_wn = [&](const std::string& p, DevVec& v, DevVec& g) {
      add(p + ".bias"); add(p + ".weight_g"); add(p + ".weight_v");
      if (K.on) { v.upload(ts.get(p + ".weight_v").data); g.upload(ts.get(p + ".weight_g").data); K.bytes += (v.n + g.n) * sizeof(float); }
    };
    for (int f = 0; f < 4; ++f) {
      const std::string p = "flow.flows." + std::to_string(2 * f) + ".";
      add(p + "pre.weight"); add(p + "pre.bias");
      for (int i = 0; i < 3; ++i) add_wn(p + "enc.in_layers." + std::to_string(i), FK.in_v[f][i], FK.in_g[f][i]);
      for (int i = 0; i < 3; ++i) add_wn(p + "enc.res_skip_layers." + std::to_string(i), FK.rs_v[f][i], FK.rs_g[f][i]);
      add_wn(p + "enc.cond_layer", FK.cond_v[f], FK.cond_g[f]);
      add(p + "post.weight"); add(p + "post.bias");
    }
  }
  S->ts.clear();
  S->ready = true;
}

// ------------------------------------------------------------------------------------------------ forward
// What a generator stage asks about its nine ResBlock pairs, asked in ONE place with the length of the WHOLE sequence at that stage (Tfull) - synth_graph launches
// by the answers, synth_window_frames aligns the window by them.  split_pair: c1 writes the pair's intermediate as the split-resident image c2 stages in LDS;
// h2_pair: both halves on the persistent kernel in its fp16x2 arithmetic (the image is then fp16 hi / lo; conv_x3q.hip); period: columns after which the order of
// a column's fp32 additions repeats in every split pair (the least common multiple of conv1d_residual_period; 1 without split pairs).
struct GenPairs { bool split_pair[3][3], h2_pair[3][3]; bool any_split = false; long long period = 1; };
static long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }
static GenPairs gen_stage_pairs(const GenStage& st, int Tfull, int h2) {
  GenPairs g;
  for (int j = 0; j < 3; ++j)
    for (int m = 0; m < 3; ++m) {
      const ConvLayer& c1 = st.rb[j].c1[m]; const ConvLayer& c2 = st.rb[j].c2[m];
      g.split_pair[j][m] = conv1d_split_eligible(c1, Tfull, SPLIT_PRODUCER) && conv1d_split_eligible(c2, Tfull, SPLIT_CONSUMER);
      g.h2_pair[j][m] = g.split_pair[j][m] && conv1d_pair_h2_eligible(c1, c2, Tfull, h2);
      if (!g.split_pair[j][m]) continue;
      g.any_split = true;
      const long long per = conv1d_residual_period(c2, Tfull, g.h2_pair[j][m] ? 1 : 0);
      g.period = g.period / gcd_ll(g.period, per) * per;
    }
  return g;
}

// The split-resident front (conv_x3s.hip): the activations that feed enc_p's / the flow's / conv_pre's projections live as bf16 hi / lo
// images written by their producers; k = 3 / 5 / 7 layers read them with taps as row offsets, so the images' margins (the zero padding)
// must stay zero: the block is the graph's first allocation (nothing else ever occupies it) and is zeroed once per layout.
struct SplitImgs { unsigned char *x_s = nullptr, *attn_s = nullptr, *ff_s = nullptr, *x0_s = nullptr, *hw_s = nullptr, *acts_s = nullptr, *z_s = nullptr, *spec_s = nullptr; };
static bool wn_split_eligible(const WNStack& W) {
  bool ok = conv_x3s_eligible(W.skip[W.n - 1]);
  for (int i = 0; i < W.n && ok; ++i) ok = conv_x3s_eligible(W.in[i]) && (i == W.n - 1 || conv_x3s_eligible(W.rs[i]));
  return ok;
}
static bool synth_split_front(const Synth* S) {
  const int C = S->hidden, IC = S->inter;
  bool gs = (C & 15) == 0 && (IC & 31) == 0 && conv_x3s_eligible(S->proj) && conv_x3s_eligible(S->conv_pre);
  for (int l = 0; l < S->n_layers && gs; ++l) {
    const EncoderLayer& e = S->enc[l];
    gs = conv_x3s_eligible(e.qkv) && conv_x3s_eligible(e.o) && conv_x3s_eligible(e.ff1) && conv_x3s_eligible(e.ff2);
  }
  for (int f = 0; f < 4 && gs; ++f) {
    const FlowLayer& F = S->flow[f];
    gs = conv_x3s_eligible(F.pre) && conv_x3s_eligible(F.post_neg) && wn_split_eligible(F.wn);
  }
  return gs;
}
// the image block: T columns up to the flow, W columns of z for the generator; spec_rows > 0: also the posterior's spectrogram operand.  Zeroed when the
// layout is not the one known to be zero.
static SplitImgs split_imgs_alloc(Synth* S, hipStream_t s, Arena& A, int T, int W, int spec_rows) {
  const int C = S->hidden, IC = S->inter;
  SplitImgs m;
  const size_t img0 = A.off;
  m.x_s = A.alloc<unsigned char>(split_image_bytes(C, T)); m.attn_s = A.alloc<unsigned char>(split_image_bytes(C, T));
  m.ff_s = A.alloc<unsigned char>(split_image_bytes(S->filt, T));
  m.x0_s = A.alloc<unsigned char>(split_image_bytes(IC / 2, T)); m.hw_s = A.alloc<unsigned char>(split_image_bytes(2 * C, T));
  m.acts_s = A.alloc<unsigned char>(split_image_bytes(C, T)); m.z_s = A.alloc<unsigned char>(split_image_bytes(IC, W));
  if (spec_rows > 0) m.spec_s = A.alloc<unsigned char>(split_image_bytes(spec_rows, T));
  // (a shorter sequence in the same allocation leaves the longer one's rows behind its end: the length is part of the layout - both lengths: the z image
  // holds the generator's W columns)
  S->imgs.ensure_zero(A, img0, A.off - img0, T, W, s);
  return m;
}

// TextEncoder{256,768} (reference models.py:43-58,:90-105) up to and including proj: returns stats = [m_p | logs_p], 2 inter rows of T columns
static float* enc_p_stats(Synth* S, hipStream_t s, Arena& A, bool gs, const SplitImgs& im, const float* feat_cm, const long long* pitch, int T,
                          float* enc_p_layer0) {
  const int C = S->hidden, IC = S->inter;
  const EncoderShape sh = {C, S->n_heads, C / S->n_heads, 10, ACT_RELU, S->filt};
  const bool dry = A.dry;
  const long long tp = split_image_tp(T);
  unsigned char *x_s = im.x_s;
  ConvEpilogue E0;
  // ---- enc_p
  float* x = A.alloc<float>((size_t)C * T);
  float* xb = A.alloc<float>((size_t)C * T);
  if (!dry) {
    gemm_tn_run(s, S->emb_phone_wT.p, C, 0, feat_cm, T, 0, x, T, 0, C, T, S->feat_dim, 1, S->emb_phone_b.p, 0, E0);
    encp_embed(s, x, S->f0 ? S->emb_pitch.p : nullptr, pitch, C, T);
    if (gs) split_image_from_f32(s, x, T, C, T, x_s, tp);
  }
  {
    const size_t mark = A.off;
    // attention on split-resident operands (attention_dma_kernel.h): q / k as one image, V^T written by the q | k | v launch (or by the swapped product);
    // otherwise fp32 q / k / v
    unsigned char* qk_s = gs ? A.alloc<unsigned char>(split_image_bytes(2 * C, T)) : nullptr;
    unsigned char* vt_s = gs ? A.alloc<unsigned char>(attention_vt_bytes(C, T)) : nullptr;
    float* qk = gs ? nullptr : A.alloc<float>((size_t)3 * C * T);
    float* vr = gs ? nullptr : A.alloc<float>((size_t)T * C);
    float* attn = gs ? nullptr : A.alloc<float>((size_t)C * T);
    float* ff = gs ? nullptr : A.alloc<float>((size_t)S->filt * T);
    if (!dry) {
      if (gs) attention_vt_clear_tail(s, vt_s, C, T);
      const EncoderSplitBufs sb = {x, xb, x_s, qk_s, vt_s, im.attn_s, im.ff_s};
      const EncoderPlainBufs pb = {x, xb, qk, vr, attn, ff};
      for (int l = 0; l < S->n_layers; ++l) {
        if (gs) encoder_layer_run_split(s, S->enc[l], sh, sb, T);
        else encoder_layer_run_plain(s, S->enc[l], sh, pb, T);
        if (l == 0) tap(A, s, enc_p_layer0, x, (size_t)C * T);
      }
    }
    A.off = mark;
  }
  float* stats = A.alloc<float>((size_t)2 * IC * T);
  if (!dry) {
    if (gs) conv_x3s_run(S->proj, s, x_s, tp, T, stats, T, E0); else
    conv1d_run(S->proj, s, x, T, T, stats, T, E0);
  }
  return stats;
}

// modules.WN.forward (reference lib/infer_pack/modules.py:184-209) over an n-layer stack, full mask: the one runner of the flow's couplings (n = 3) and of the
// posterior encoder (n = 16).  In: the residual stream h = hw rows [0, H) (split-resident path: also its image, the first H channels of hw_s); out: the skip sum
// wo = hw rows [H, 2 H) (and its image behind h's).  gcond: cond_layer(g), 2 H n values.
struct WnBufs { float* hw; float* xin; float* acts; unsigned char* hw_s; unsigned char* acts_s; };
// what a recording pass keeps of a 3-layer stack (the flow's): x[i] receives layer i's input, a[i] its pre-gate activation in_layers[i](x) + gc slice (2 H rows)
struct WnRecord { float* x[3]; float* a[3]; };
// The recording variant: in_layers[i] writes its 2 H rows into the tape (the gate cannot run in the launch's epilogue, which never stores them), the gate is
// wn_gate_record - the arithmetic of wn_gate / wn_gate_split, the summed pre-gate activation stored back - and the residual stream is copied out per layer.
static void wn_run_record(hipStream_t s, const WNStack& W, const float* gcond, bool gs, const WnBufs& b, int C, int T, const WnRecord& rec) {
  const long long tp = split_image_tp(T);
  float* h = b.hw; float* wo = b.hw + (size_t)C * T;
  unsigned char* wo_s = gs ? b.hw_s + split_image_bytes(C, T) : nullptr;
  ConvEpilogue E0;
  RVC_REQUIRE(W.n == 3, "a recorded WaveNet stack has 3 layers");
  if (gs) fill(s, wo, 0.f, (long long)C * T);
  for (int i = 0; i < W.n; ++i) {
    RVC_HIP_CHECK(hipMemcpyAsync(rec.x[i], h, (size_t)C * T * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (gs) conv_x3s_run(W.in[i], s, b.hw_s, tp, T, rec.a[i], T, E0); else conv1d_run(W.in[i], s, h, T, T, rec.a[i], T, E0);
    wn_gate_record(s, rec.a[i], gcond + (size_t)i * 2 * C, gs ? nullptr : b.acts, gs ? b.acts_s : nullptr, tp, kSplitMargin, C, T);
    if (gs) {
      if (i < W.n - 1) { ConvEpilogue Ea; Ea.R = b.hw; Ea.ldR = T; Ea.ys_out = b.hw_s; Ea.ys_tp = tp; conv_x3s_run(W.rs[i], s, b.acts_s, tp, T, b.hw, T, Ea); }
      else { ConvEpilogue Ea; Ea.R = wo; Ea.ldR = T; Ea.ys_out = wo_s; Ea.ys_tp = tp; conv_x3s_run(W.skip[i], s, b.acts_s, tp, T, wo, T, Ea); }
    } else {
      ConvEpilogue Es; Es.accumulate = (i > 0);
      conv1d_run(W.skip[i], s, b.acts, T, T, wo, T, Es);
      if (i < W.n - 1) { ConvEpilogue Er; Er.R = h; Er.ldR = T; conv1d_run(W.res[i], s, b.acts, T, T, h, T, Er); }
    }
  }
}
static void wn_run(hipStream_t s, const WNStack& W, const float* gcond, bool gs, const WnBufs& b, int C, int T, const WnRecord* rec = nullptr) {
  if (rec) return wn_run_record(s, W, gcond, gs, b, C, T, *rec);
  const long long tp = split_image_tp(T);
  float* h = b.hw; float* wo = b.hw + (size_t)C * T;
  ConvEpilogue E0;
  if (gs) {
    // every layer one launch of the split-resident GEMM: the res / skip pair of a WaveNet layer is ONE 2 H-row layer accumulating in place
    // onto [h | wo] (its image output is the next in-layer's input)
    unsigned char* wo_s = b.hw_s + split_image_bytes(C, T);
    fill(s, wo, 0.f, (long long)C * T);
    for (int i = 0; i < W.n; ++i) {
      if (W.in_gate[i].Wx_ && conv_x3s_eligible(W.in_gate[i])) {
        // k = 5 over the first H channels of the [h | wo] image, the gate in the epilogue: acts leaves as its image, the 2 H-row tensor is never stored
        ConvEpilogue Eg; Eg.ys_out = b.acts_s; Eg.ys_tp = tp; Eg.gate_h = C; Eg.gate_g = gcond + (size_t)i * 2 * C;
        conv_x3s_run(W.in_gate[i], s, b.hw_s, tp, T, nullptr, T, Eg);
      } else {
        conv_x3s_run(W.in[i], s, b.hw_s, tp, T, b.xin, T, E0);                 // k = 5 over the first H channels of the [h | wo] image
        wn_gate_split(s, b.xin, gcond + (size_t)i * 2 * C, b.acts_s, tp, kSplitMargin, C, T);
      }
      if (i < W.n - 1) { ConvEpilogue Ea; Ea.R = b.hw; Ea.ldR = T; Ea.ys_out = b.hw_s; Ea.ys_tp = tp; conv_x3s_run(W.rs[i], s, b.acts_s, tp, T, b.hw, T, Ea); }
      else { ConvEpilogue Ea; Ea.R = wo; Ea.ldR = T; Ea.ys_out = wo_s; Ea.ys_tp = tp; conv_x3s_run(W.skip[i], s, b.acts_s, tp, T, wo, T, Ea); }
    }
    return;
  }
  for (int i = 0; i < W.n; ++i) {
    conv1d_run(W.in[i], s, h, T, T, b.xin, T, E0);
    wn_gate(s, b.xin, gcond + (size_t)i * 2 * C, b.acts, C, T);
    ConvEpilogue Es; Es.accumulate = (i > 0);
    conv1d_run(W.skip[i], s, b.acts, T, T, wo, T, Es);
    if (i < W.n - 1) { ConvEpilogue Er; Er.R = h; Er.ldR = T; conv1d_run(W.res[i], s, b.acts, T, T, h, T, Er); }
  }
}

// One ResidualCouplingLayer (reference lib/infer_pack/modules.py:436-455, mean_only) on cur [inter][T] in place: x1 -= m (reverse, infer) or x1 += m (forward,
// training).  The split-resident path packs post with both signs (post_neg / post): either direction is a plain residual add in the GEMM's epilogue.
static void coupling_run(Synth* S, hipStream_t s, FlowLayer& F, const float* gcond, bool gs, const SplitImgs& im, const WnBufs& b, float* cur, int T, bool reverse,
                         const WnRecord* rec = nullptr) {
  const int C = S->hidden, half = S->inter / 2;
  const long long tp = split_image_tp(T);
  float* h = b.hw; float* wo = b.hw + (size_t)C * T;
  float* x1 = cur + (size_t)half * T;
  ConvEpilogue E0;
  if (gs) {
    split_image_from_f32(s, cur, T, half, T, im.x0_s, tp);
    unsigned char* wo_s = b.hw_s + split_image_bytes(C, T);
    ConvEpilogue Eh; Eh.ys_out = b.hw_s; Eh.ys_tp = tp;
    conv_x3s_run(F.pre, s, im.x0_s, tp, T, h, T, Eh);
    wn_run(s, F.wn, gcond, gs, b, C, T, rec);
    ConvEpilogue Ep; Ep.R = x1; Ep.ldR = T;
    conv_x3s_run(reverse ? F.post_neg : F.post, s, wo_s, tp, T, x1, T, Ep);    // x1 = x1 -+ m
    return;
  }
  conv1d_run(F.pre, s, cur, T, T, h, T, E0);
  wn_run(s, F.wn, gcond, gs, b, C, T, rec);
  ConvEpilogue Ep; Ep.out_scale = reverse ? -1.f : 1.f; Ep.accumulate = 1;
  conv1d_run(F.post, s, wo, T, T, x1, T, Ep);     // x1 = x1 -+ m
}

// GeneratorNSF / Generator (reference models.py:460-566,:244-311) from conv_pre on, on the W columns [g0, g0 + W) of z [inter][T] (a T-frame sequence); har: the
// harmonic source of the whole sequence [T upp] (null: no-f0 family); out: the whole sequence's waveform, written at [g0 upp, (g0 + W) upp).  Shared by
// synth_infer (keep window plus halo) and the training forward (the slice as a sequence of its own: T = W = segment, g0 = 0).
static void gen_tail(Synth* S, hipStream_t s, Arena& A, bool gs, unsigned char* z_s, const float* z, const float* har, const float* pre_bias, int T, int g0, int W,
                     int h2, float* out, const SynthTaps* taps) {
  const int IC = S->inter;
  const bool dry = A.dry;
  // From here on every tensor holds the W columns of the window; the three full-length operands are addressed at its start: z + g0 (pitch T), har + g0 upp,
  // out + g0 upp.  Every launch is planned for the whole sequence and sized for the window: beside a stage's window length (Tc, Tn) runs the whole sequence's
  // (Tfull_c, Tfull_n), handed to every planner and, as ConvEpilogue::plan_tin, to every *_run - a window's columns are computed by the kernels, tiles and K
  // splits of the full pass.  With [0, T) the two are equal and plan_tin stays 0.  Columns within the halo of a cut edge see zero padding there and are wrong;
  // the caller keeps none of them.
  auto plan_tin = [&](int tin_full) { return W != T ? tin_full : 0; };
  const long long Nw = (long long)W * S->upp;
  const float* har_w = har ? har + (size_t)g0 * S->upp : nullptr;
  float* zw = (!gs && W != T) ? A.alloc<float>((size_t)IC * W) : nullptr;      // (the fp32 path stages rows from an aligned base: the window densely)
  float* cur = A.alloc<float>((size_t)S->up_init * W);
  if (!dry) {
    ConvEpilogue Eb; Eb.bias_override = pre_bias;
    const long long tpw = split_image_tp(W);
    Eb.plan_tin = plan_tin(T);
    if (gs) { split_image_from_f32(s, z + g0, T, IC, W, z_s, tpw); conv_x3s_run(S->conv_pre, s, z_s, tpw, W, cur, W, Eb); }     // k = 7
    else if (zw) {
      RVC_HIP_CHECK(hipMemcpy2DAsync(zw, (size_t)W * sizeof(float), z + g0, (size_t)T * sizeof(float), (size_t)W * sizeof(float), IC, hipMemcpyDeviceToDevice, s));
      conv1d_run(S->conv_pre, s, zw, W, W, cur, W, Eb);
    } else conv1d_run(S->conv_pre, s, z, T, T, cur, T, Eb);
  }
  int Tc = W, Tfull_c = T;
  const int nu = (int)S->stages.size();
  for (int i = 0; i < nu; ++i) {
    GenStage& st = S->stages[i];
    const int Cc = S->up_init >> (i + 1);
    const int Tn = Tc * st.u, Tfull_n = Tfull_c * st.u;
    float* up = A.alloc<float>((size_t)Cc * Tn);
    float* t1 = A.alloc<float>((size_t)Cc * Tn);
    float* ya = A.alloc<float>((size_t)Cc * Tn);
    float* yb = A.alloc<float>((size_t)Cc * Tn);
    float* xs = A.alloc<float>((size_t)Cc * Tn);
    float* fr = (S->f0 && st.noise_k > 1) ? A.alloc<float>((size_t)st.noise_k * Tn) : nullptr;
    // split-resident intermediate of a ResBlock pair: c1's epilogue writes t = lrelu(c1(..) + b1) as the bf16 hi / lo image c2 stages in
    // LDS (DMA, no conversion, no staging registers; 4 b128 stores per accumulator instead of 16 dword stores on c1's side)
    // h2_pair: both halves on the persistent kernel in its fp16x2 arithmetic (two MFMAs per product; conv_x3q.hip) - the pair's image is then fp16 hi / lo
    const GenPairs gp = gen_stage_pairs(st, Tfull_n, h2);
    unsigned char* t1s = gp.any_split ? A.alloc<unsigned char>(split_image_bytes(Cc, Tn)) : nullptr;
    if (!dry) {
      RVC_REQUIRE(conv1d_out_len(st.up, Tc) == Tn, "ConvTranspose1d geometry must give T_out = u * T_in");
      // up-sampled signal first (interleaved store of the transposed conv's phases, no read-modify-write), then the noise branch is
      // added by its own convolution's dense epilogue: the same two-operand fp32 sum as noise first / up-conv accumulating
      ConvEpilogue Eu; Eu.plan_tin = plan_tin(Tfull_c); Eu.pre_act = ACT_LRELU; Eu.pre_slope = 0.1f;
      conv1d_run(st.up, s, cur, Tc, Tc, up, Tn, Eu);
      ConvEpilogue En; En.plan_tin = plan_tin(Tfull_n); En.accumulate = 1;
      // last stage (one tap of the source per position) with all three ResBlocks on conv_rb3_kernel: the noise term is added where x is read
      // (the gen_ups0 tap wants the summed tensor)
      bool noise_in_rb3 = S->f0 && st.noise_k == 1 && st.noise_w.p != nullptr && Nw == (long long)Tn && !(taps && i == 0);
      // 32- / 64-channel stages in the fp16x2 arithmetic: a whole ResBlock (three pairs) in one launch, x read once, the sum written once (conv_rb3.hip).
      // Each ResBlock is planned once; the noise decision and the launches below use these same plans.
      Rb3Plan rb3[3]; bool rb3_ok[3];
      auto plan_rb3 = [&](bool noise) {
        bool all = true;
        for (int j = 0; j < 3; ++j) {
          const ConvLayer* r1[3] = {&st.rb[j].c1[0], &st.rb[j].c1[1], &st.rb[j].c1[2]};
          const ConvLayer* r2[3] = {&st.rb[j].c2[0], &st.rb[j].c2[1], &st.rb[j].c2[2]};
          rb3_ok[j] = conv_rb3_plan(r1, r2, up, Tn, Tn, Tfull_n, xs, Tn, 0.1f, 1.f / 3.f, j > 0, h2, noise ? har_w : nullptr, noise ? st.noise_w.p : nullptr,
                                    noise ? st.noise_b.p : nullptr, rb3[j]);
          all = all && rb3_ok[j];
        }
        return all;
      };
      if (!plan_rb3(noise_in_rb3) && noise_in_rb3) { noise_in_rb3 = false; plan_rb3(false); }
      if (noise_in_rb3) {
        // nothing here
      } else if (!S->f0) {
        // plain Generator: nothing is added to the up-sampled signal
      } else if (st.noise_w.p && noise_add(s, up, Tn, Cc, Tn, har_w, Nw, st.noise_k, st.noise_s, st.noise_k > 1 ? st.noise_s / 2 : 0, st.noise_w.p, st.noise_b.p)) {
        // narrow stages (k <= 8 taps of the one source channel): a streaming add instead of im2col + GEMM
      } else if (st.noise_k > 1) {
        frames(s, har_w, fr, (int)Nw, st.noise_k, st.noise_s, st.noise_s / 2, Tn, 0);
        conv1d_run(st.noise, s, fr, Tn, Tn, up, Tn, En);
      } else {
        conv1d_run(st.noise, s, har_w, Tn, Tn, up, Tn, En);
      }
      if (taps && i == 0) tap(A, s, taps->gen_ups0, up, (size_t)Cc * Tn);
      for (int j = 0; j < 3; ++j) {
        const float* in = up;
        if (rb3_ok[j]) { conv_rb3_launch(rb3[j], s); continue; }
        for (int m = 0; m < 3; ++m) {
          ConvEpilogue E2; E2.plan_tin = plan_tin(Tfull_n); E2.pre_act = ACT_LRELU; E2.pre_slope = 0.1f; E2.R = in; E2.ldR = Tn;
          float* dst = (m == 0) ? ya : (m == 1 ? yb : xs);
          if (m == 2) { E2.out_scale = 1.f / 3.f; E2.accumulate = (j > 0); }
          // narrow stages: both convs of the pair in one launch, the intermediate stays in LDS (conv_x3.hip, FUSE)
          ConvPlan pp;
          if (conv_x3_pair_plan(st.rb[j].c1[m], st.rb[j].c2[m], in, Tn, Tn, Tfull_n, dst, Tn, E2, h2, pp)) conv_plan_launch(pp, s);
          else {
            ConvEpilogue E1; E1.plan_tin = plan_tin(Tfull_n); E1.pre_act = ACT_LRELU; E1.pre_slope = 0.1f;
            if (gp.split_pair[j][m]) {
              E1.ys_out = t1s; E1.ys_tp = split_image_tp(Tn); E1.ys_slope = E2.pre_slope;       // c2's input activation, applied once by the producer
              E1.h2 = gp.h2_pair[j][m] ? 1 : 0;
              conv1d_run(st.rb[j].c1[m], s, in, Tn, Tn, nullptr, Tn, E1);
              ConvEpilogue E2s = E2; E2s.pre_act = ACT_NONE; E2s.xs_in = t1s; E2s.xs_tp = E1.ys_tp; E2s.h2 = E1.h2;
              conv1d_run(st.rb[j].c2[m], s, nullptr, Tn, Tn, dst, Tn, E2s);
            } else {
              conv1d_run(st.rb[j].c1[m], s, in, Tn, Tn, t1, Tn, E1);
              conv1d_run(st.rb[j].c2[m], s, t1, Tn, Tn, dst, Tn, E2);
            }
          }
          in = dst;
        }
      }
      if (taps && i == nu - 1) tap(A, s, taps->gen_last, xs, (size_t)Cc * Tn);
    }
    cur = xs; Tc = Tn; Tfull_c = Tfull_n;
  }
  if (!dry) conv_to1(s, cur, Tc, S->conv_post_w.p, S->up_init >> nu, 7, 3, Tc, 0.01f, 1, out + (size_t)g0 * S->upp);
}

// ------------------------------------------------------------------------------------------------ the recorded decoder pass
// One item's decoder pass at the net's segment, every tensor fp32 [rows][cols] in one allocation and found by name:
//   z [inter][seg], har [1][seg upp] (f0 family), pre [up_init][seg] (conv_pre + cond(g), before the leaky ReLU), y_hat [1][seg upp]; per stage i: up{i} (the
//   up-sampled sum after the noise branch), rb{i}.{j}.y{m} (m = 1, 2: the input of pair m; y0 is up{i}), rb{i}.{j}.t{m} (c1(lrelu(y_m)) + b1), out{i} (xs / 3)
// and the deltas of synth_dec_input_grad, the cotangent at each convolution's output:
//   d.post [1][seg upp] (conv_post's), d.out{i} (at EACH ResBlock's output of stage i: the stage output's cotangent / 3), d.rb{i}.{j}.t{m}, d.rb{i}.{j}.y{m}
//   (m = 1, 2), d.up{i} (the stage sum: the up-sampler's and the noise convolution's), d.pre (conv_pre's), d.cond [1][up_init], d.g [1][gin], d.har
// and, on a handle with kept parameters (synth_keep_parameters), what the weight-gradient pass reads beside them: sine [1][seg upp] (the source before
// m_source.l_linear; f0 family), g [1][gin] (the item's emb_g row)
struct GenTape {
  struct Tensor { size_t off; int rows; long long cols; bool flow = false; };      // flow: an offset into flow_mem
  const Synth* S = nullptr; int seg = 0; bool recorded = false;
  bool backward_done = false;      // a backward data pass has run since the last taped forward: the deltas belong to the recorded activations
  std::map<std::string, Tensor> t;
  DevVec mem; float* fr = nullptr;      // fr: the im2col frames of a wide noise convolution (scratch)
  // the flow's recording (synth_forward_tape with record_flow): its tensors live in a block of their own, laid out for the item's length when a recording
  // forward first meets that length - a tape that never records the flow holds none of it
  DevVec flow_mem; int flow_T = 0; bool flow_recorded = false; int flow_fwd_marks = 0, flow_bwd_marks = 0;
  bool flow_backward_done = false;      // synth_flow_input_grad has run since the last recording forward: the flow's deltas belong to the recorded activations
  // timing (gen_tape_timing; off: no event is ever created or recorded): events around the taped decoder and at the backward's stage boundaries
  bool timing = false; std::vector<hipEvent_t> ev; int fwd_marks = 0, bwd_marks = 0, wgrad_marks = 0;
  GenTape() = default;
  GenTape(const GenTape&) = delete; GenTape& operator=(const GenTape&) = delete;
  ~GenTape() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  void mark(hipStream_t s, int slot) {
    if (!timing) return;
    while ((int)ev.size() <= slot) { hipEvent_t e; RVC_HIP_CHECK(hipEventCreate(&e)); ev.push_back(e); }
    RVC_HIP_CHECK(hipEventRecord(ev[slot], s));
  }
  float* ptr(const std::string& name) const {
    auto it = t.find(name);
    RVC_REQUIRE(it != t.end(), "the tape holds no tensor '" + name + "'");
    return (it->second.flow ? flow_mem.p : mem.p) + it->second.off;
  }
};
constexpr int kFlowMark0 = 32;       // the flow's events: 32, 33 around the recorded flow forward, 34, 35 around its backward
constexpr int kWgradMark0 = 16;      // the weight-gradient pass's events: slots 16 .. (the forward's are 0, 1; the backward's 2 .. n + 4)
static std::string rb_name(int i, int j, const char* what, int m) { return "rb" + std::to_string(i) + "." + std::to_string(j) + "." + what + std::to_string(m); }
static void tape_check(const Synth* S, const GenTape* tape) {
  RVC_REQUIRE(tape->S == S, "the tape was created from another synthesizer handle");
  RVC_REQUIRE(tape->seg == S->segment && S->gen_bwd.built, "the tape was created for another segment_size (the handle was finalized again)");
}

// The data-gradient images (conv_gen_bwd.hip), rows = the forward's input channels padded to a multiple of 128.
// Conv1d W [Co][Ci][k] -> W' [Ci][Co][t] = W[co][ci][k - 1 - t]: tap t of the data gradient reads D at t_out + pad - (k - 1) dil + t dil
void gen_bwd_conv_image(const float* w, int Co, int Ci, int k, std::vector<uint16_t>& P) {
  RVC_REQUIRE(Co >= 16 && Co % 16 == 0 && Ci >= 1 && k >= 1 && k <= 16, "decoder convolution does not fit the data-gradient kernel");
  std::vector<float> wt((size_t)Co * Ci * k);
  for (int co = 0; co < Co; ++co)
    for (int ci = 0; ci < Ci; ++ci)
      for (int t = 0; t < k; ++t) wt[((size_t)ci * Co + co) * k + t] = w[((size_t)co * Ci + ci) * k + (k - 1 - t)];
  x3_weight_image(wt.data(), Ci, Co, k, (Ci + 127) & ~127, P);
}
// ConvTranspose1d W [Cin][Cout][k] is its own data gradient's image: tap t reads D at u t_in - pad + t
void gen_bwd_up_image(const float* w, int Cin, int Cout, int k, std::vector<uint16_t>& P) {
  RVC_REQUIRE(Cout >= 16 && Cout % 16 == 0 && Cin >= 1 && k >= 1 && k <= 16, "up-sampler does not fit the data-gradient kernel");
  x3_weight_image(w, Cin, Cout, k, (Cin + 127) & ~127, P);
}

// the backward pass's weight images, built when the first tape is created (a handle that only infers never gets here)
static void gen_bwd_build(Synth* S) {
  GenBwdImages& B = S->gen_bwd; GenHostWeights& H = S->gen_host;
  if (B.built) return;
  const int nu = (int)S->stages.size();
  RVC_REQUIRE(!H.pre.empty() && (int)H.up.size() == nu, "the decoder's folded weights were not kept (no posterior was loaded at finalize)");
  GenBwdImages N;
  auto conv_image = [&](const std::vector<float>& w, int Co, int Ci, int k, DevBuf<uint16_t>& img) {
    RVC_REQUIRE(w.size() == (size_t)Co * Ci * k, "decoder convolution: weight size");
    std::vector<uint16_t> P;
    gen_bwd_conv_image(w.data(), Co, Ci, k, P);
    img.upload(P); N.bytes += P.size() * sizeof(uint16_t);
  };
  conv_image(H.pre, S->up_init, S->inter, 7, N.pre);
  N.up.resize(nu); N.noise.resize(nu); N.c1.resize((size_t)nu * 9); N.c2.resize((size_t)nu * 9);
  for (int i = 0; i < nu; ++i) {
    const GenStage& st = S->stages[i];
    const int cin = S->up_init >> i, cout = S->up_init >> (i + 1);
    RVC_REQUIRE(H.up[i].size() == (size_t)cin * cout * st.k, "up-sampler: weight size");
    std::vector<uint16_t> P;
    gen_bwd_up_image(H.up[i].data(), cin, cout, st.k, P);
    N.up[i].upload(P); N.bytes += P.size() * sizeof(uint16_t);
    if (S->f0) { N.noise[i].upload(H.noise[i]); N.bytes += H.noise[i].size() * sizeof(float); }
    for (int j = 0; j < 3; ++j)
      for (int m = 0; m < 3; ++m) {
        const size_t q = (size_t)(i * 3 + j) * 3 + m;
        conv_image(H.c1[q], cout, cout, S->rb_k[j], N.c1[q]);
        conv_image(H.c2[q], cout, cout, S->rb_k[j], N.c2[q]);
      }
  }
  N.built = true;
  B = std::move(N);
  H = {};
}

GenTape* gen_tape_create(Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(S->post_enc.built, "no posterior encoder loaded: a tape belongs to the training forward");
  RVC_REQUIRE(S->segment > 0, "segment_size is not set in the configuration");
  gen_bwd_build(S);
  std::unique_ptr<GenTape> T(new GenTape());
  T->S = S; T->seg = S->segment;
  size_t off = 0;
  auto add = [&](const std::string& name, int rows, long long cols) {
    T->t[name] = {off, rows, cols};
    off += ((size_t)rows * (size_t)cols + 63) & ~size_t(63);
  };
  const int seg = S->segment, nu = (int)S->stages.size();
  const long long N = (long long)seg * S->upp;
  auto layout = [&](bool deltas) {      // the activations, then the deltas under the same names behind "d."
    const std::string d = deltas ? "d." : "";
    if (!deltas) { add("z", S->inter, seg); if (S->f0) add("har", 1, N); }
    add(d + "pre", S->up_init, seg);
    long long Tn = seg;
    for (int i = 0; i < nu; ++i) {
      const int Cc = S->up_init >> (i + 1);
      Tn *= S->stages[i].u;
      add(d + "up" + std::to_string(i), Cc, Tn);
      for (int j = 0; j < 3; ++j) {
        for (int m = 1; m < 3; ++m) add(d + rb_name(i, j, "y", m), Cc, Tn);
        for (int m = 0; m < 3; ++m) add(d + rb_name(i, j, "t", m), Cc, Tn);
      }
      add(d + "out" + std::to_string(i), Cc, Tn);
    }
    add(deltas ? "d.post" : "y_hat", 1, N);
  };
  layout(false); layout(true);
  add("d.cond", 1, S->up_init); add("d.g", 1, S->gin);
  if (S->f0) add("d.har", 1, N);
  // what the weight-gradient pass reads beside the activations and deltas (a handle with kept parameters only): the source before m_source.l_linear, emb_g's row
  if (S->kept.on) { if (S->f0) add("sine", 1, N); add("g", 1, S->gin); }
  size_t fr = 0;
  {
    long long Tn = seg;
    for (int i = 0; i < nu; ++i) { Tn *= S->stages[i].u; if (S->f0 && S->stages[i].noise_k > 1) fr = std::max(fr, (size_t)S->stages[i].noise_k * (size_t)Tn); }
  }
  const size_t fr_off = off; off += fr;
  T->mem.alloc(off);
  T->fr = T->mem.p + fr_off;
  return T.release();
}
void gen_tape_destroy(GenTape* T) { delete T; }
size_t gen_tape_bytes(const GenTape* T) { return (T->mem.n + T->flow_mem.n) * sizeof(float); }
size_t synth_gen_bwd_bytes(const Synth* S) { return S->gen_bwd.bytes; }
bool gen_tape_tensor(const GenTape* T, const char* name, float** p, int* rows, long long* cols) {
  auto it = T->t.find(name);
  if (it == T->t.end()) return false;
  *p = (it->second.flow ? T->flow_mem.p : T->mem.p) + it->second.off; *rows = it->second.rows; *cols = it->second.cols;
  return true;
}

// gen_tail on the slice, layer by layer on the unfused conv1d_run path (one launch per convolution), every tensor the backward pass reads written into the tape
static void gen_tail_tape(Synth* S, hipStream_t s, GenTape& tape, const float* pre_bias, float* out) {
  const int seg = S->segment, nu = (int)S->stages.size();
  const long long N = (long long)seg * S->upp;
  tape.mark(s, 0);
  const float* har = S->f0 ? tape.ptr("har") : nullptr;
  float* cur = tape.ptr("pre");
  ConvEpilogue Eb; Eb.bias_override = pre_bias;
  conv1d_run(S->conv_pre, s, tape.ptr("z"), seg, seg, cur, seg, Eb);
  int Tc = seg;
  for (int i = 0; i < nu; ++i) {
    GenStage& st = S->stages[i];
    const int Cc = S->up_init >> (i + 1), Tn = Tc * st.u;
    float* up = tape.ptr("up" + std::to_string(i));
    float* xs = tape.ptr("out" + std::to_string(i));
    RVC_REQUIRE(conv1d_out_len(st.up, Tc) == Tn, "ConvTranspose1d geometry must give T_out = u * T_in");
    ConvEpilogue Eu; Eu.pre_act = ACT_LRELU; Eu.pre_slope = 0.1f;
    conv1d_run(st.up, s, cur, Tc, Tc, up, Tn, Eu);
    ConvEpilogue En; En.accumulate = 1;
    if (!S->f0) {
      // plain Generator: nothing is added to the up-sampled signal
    } else if (st.noise_w.p && noise_add(s, up, Tn, Cc, Tn, har, N, st.noise_k, st.noise_s, st.noise_k > 1 ? st.noise_s / 2 : 0, st.noise_w.p, st.noise_b.p)) {
    } else if (st.noise_k > 1) {
      frames(s, har, tape.fr, (int)N, st.noise_k, st.noise_s, st.noise_s / 2, Tn, 0);
      conv1d_run(st.noise, s, tape.fr, Tn, Tn, up, Tn, En);
    } else {
      conv1d_run(st.noise, s, har, Tn, Tn, up, Tn, En);
    }
    for (int j = 0; j < 3; ++j) {
      const float* in = up;
      for (int m = 0; m < 3; ++m) {
        float* t = tape.ptr(rb_name(i, j, "t", m));
        float* dst = m < 2 ? tape.ptr(rb_name(i, j, "y", m + 1)) : xs;
        ConvEpilogue E1; E1.pre_act = ACT_LRELU; E1.pre_slope = 0.1f;
        conv1d_run(st.rb[j].c1[m], s, in, Tn, Tn, t, Tn, E1);
        ConvEpilogue E2; E2.pre_act = ACT_LRELU; E2.pre_slope = 0.1f; E2.R = in; E2.ldR = Tn;
        if (m == 2) { E2.out_scale = 1.f / 3.f; E2.accumulate = (j > 0); }      // out{i} = sum_j (pair 2's output) / 3, added in the order j = 0, 1, 2
        conv1d_run(st.rb[j].c2[m], s, t, Tn, Tn, dst, Tn, E2);
        in = dst;
      }
    }
    cur = xs; Tc = Tn;
  }
  float* y_hat = tape.ptr("y_hat");
  conv_to1(s, cur, Tc, S->conv_post_w.p, S->up_init >> nu, 7, 3, Tc, 0.01f, 1, y_hat);
  RVC_HIP_CHECK(hipMemcpyAsync(out, y_hat, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));
  tape.mark(s, 1); tape.fwd_marks = 2;
}

// The vector-Jacobian product of that pass (GeneratorNSF / Generator, reference models.py:542-564 read backwards): d y_hat -> d z, d cond, d g, d har, every delta
// left in the tape.  Masks come from the tape, so this is the exact gradient of what the taped forward computed.  tape null: nothing is launched, the return
// value is the number of launches of the plan (a constant of the net: it does not depend on the segment).  No atomics: two calls give the same bits.
static int dec_backward(const Synth* S, hipStream_t s, GenTape* tape, const float* dy, float* dz, float* dcond, float* dg, float* dhar) {
  const GenBwdImages& B = S->gen_bwd;
  const int seg = S->segment, nu = (int)S->stages.size();
  const long long N = (long long)seg * S->upp;
  int launches = 0;
  auto P = [&](const std::string& name) -> float* { return tape ? tape->ptr(name) : nullptr; };
  auto gemm = [&](const DevBuf<uint16_t>* img, const float* D, int Ck, int Td, const float* A, const float* Res, float* Y, int R, int Ncols, int nt, int cstride,
                  int tstep, int off0, float slope, float scale, int accumulate) {
    ++launches;
    if (!tape) return;
    ConvGenBwdArgs a{D, Td, Td, reinterpret_cast<const unsigned char*>(img->p), A, Res, Y, Ncols, R, (R + 127) & ~127, Ck, Ncols, nt, cstride, tstep, off0, slope, scale,
                     accumulate};
    ConvGenBwdPlan p;
    RVC_REQUIRE(conv_gen_bwd_plan(a, p), "decoder layer does not fit the data-gradient kernel");
    conv_gen_bwd_launch(p, s);
  };
  int marks = 0;
  auto mark = [&] { if (tape) { tape->mark(s, 2 + marks); tape->bwd_marks = ++marks; } };      // intervals: tanh + conv_post, stage nu - 1 .. 0, conv_pre + cond + noise
  mark();
  // tanh and conv_post (k = 7, no bias; F.leaky_relu's default slope 0.01 in front of it), the stage mean's 1 / 3 folded into the same store
  const int Clast = S->up_init >> nu;
  ++launches; if (tape) gen_tanh_bwd(s, dy, P("y_hat"), P("d.post"), N);
  ++launches; if (tape) gen_post_bwd(s, P("d.post"), S->conv_post_w.p, P("out" + std::to_string(nu - 1)), P("d.out" + std::to_string(nu - 1)), Clast, 7, 3, N, 0.01f, 1.f / 3.f);
  long long Tn = N;
  for (int i = nu - 1; i >= 0; --i) {
    mark();
    const GenStage& st = S->stages[i];
    const int Cc = S->up_init >> (i + 1), Cin = S->up_init >> i;
    const int Tni = (int)Tn, Tc = Tni / st.u;
    const std::string si = std::to_string(i);
    float* dup = P("d.up" + si);
    for (int j = 0; j < 3; ++j) {
      const int k = S->rb_k[j];
      const float* D = P("d.out" + si);
      for (int m = 2; m >= 0; --m) {
        const size_t q = (size_t)(i * 3 + j) * 3 + m;
        const int dil = S->rb_d[j][m];
        float* dt = P("d." + rb_name(i, j, "t", m));
        // d_t = c2^T(D) lrelu'(t_m);  d_y = D + c1^T(d_t) lrelu'(y_m), the three ResBlocks' d_y0 added into d.up{i} in the order j = 0, 1, 2
        gemm(tape ? &B.c2[q] : nullptr, D, Cc, Tni, P(rb_name(i, j, "t", m)), nullptr, dt, Cc, Tni, k, 1, 1, (k - 1) / 2 - (k - 1), 0.1f, 1.f, 0);
        float* dyv = m > 0 ? P("d." + rb_name(i, j, "y", m)) : dup;
        gemm(tape ? &B.c1[q] : nullptr, dt, Cc, Tni, m > 0 ? P(rb_name(i, j, "y", m)) : P("up" + si), D, dyv, Cc, Tni, k, 1, dil, (k * dil - dil) / 2 - (k - 1) * dil, 0.1f, 1.f,
             m == 0 && j > 0);
        D = dyv;
      }
    }
    // the up-sampler's data gradient, a stride-u convolution, times the mask (slope 0.1) of what it read: the previous stage's output (whose three ResBlocks each
    // receive a third) or conv_pre's
    gemm(tape ? &B.up[i] : nullptr, dup, Cc, Tni, i > 0 ? P("out" + std::to_string(i - 1)) : P("pre"), nullptr, i > 0 ? P("d.out" + std::to_string(i - 1)) : P("d.pre"),
         Cin, Tc, st.k, st.u, 1, -((st.k - st.u) / 2), 0.1f, i > 0 ? 1.f / 3.f : 1.f, 0);
    Tn = Tc;
  }
  mark();
  // conv_pre (k = 7, pad 3, no activation in front of it) and the conditioning: dcond = row sums of conv_pre's output cotangent, dg = cond_w^T dcond
  gemm(tape ? &B.pre : nullptr, P("d.pre"), S->up_init, seg, nullptr, nullptr, dz, S->inter, seg, 7, 1, 1, -3, 1.f, 1.f, 0);
  ++launches; if (tape) gen_row_sums(s, P("d.pre"), S->up_init, seg, P("d.cond"), dcond);
  ++launches; if (tape) gen_cond_bwd(s, S->dec_cond_w.p, P("d.cond"), S->up_init, S->gin, P("d.g"), dg);
  // the noise branch onto the harmonic source, stage by stage in index order
  if (S->f0) {
    float* dh = P("d.har");      // the sum runs in the tape (d.har is always written); the caller's dhar receives a copy of it, like dcond and dg
    long long Ti = seg;
    for (int i = 0; i < nu; ++i) {
      const GenStage& st = S->stages[i];
      Ti *= st.u;
      ++launches;
      if (tape) gen_noise_bwd(s, P("d.up" + std::to_string(i)), B.noise[i].p, dh, dhar, S->up_init >> (i + 1), st.noise_k, st.noise_s, st.noise_k > 1 ? st.noise_s / 2 : 0, Ti, N, i > 0);
    }
  }
  mark();
  return launches;
}
void gen_tape_timing(GenTape* T, bool on) { T->timing = on; if (!on) T->fwd_marks = T->bwd_marks = T->wgrad_marks = T->flow_fwd_marks = T->flow_bwd_marks = 0; }
// waits for the recorded events.  ms[0]: the taped decoder (conv_pre .. y_hat) of the last taped forward; then the last backward's intervals in execution order:
// tanh + conv_post, stage n - 1 .. stage 0, conv_pre + conditioning + noise branch.  Returns the number of values (0: timing off or nothing recorded yet).
int gen_tape_times(GenTape* T, float* ms, int cap) {
  if (!T->timing || T->fwd_marks < 2) return 0;
  int n = 0;
  auto put = [&](int a, int b) {
    if (n >= cap) return;
    RVC_HIP_CHECK(hipEventSynchronize(T->ev[b]));
    RVC_HIP_CHECK(hipEventElapsedTime(&ms[n++], T->ev[a], T->ev[b]));
  };
  put(0, 1);
  for (int k = 1; k < T->bwd_marks; ++k) put(2 + k - 1, 2 + k);
  return n;
}
int synth_dec_input_grad_launch_count(const Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  return dec_backward(S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}
void synth_dec_input_grad(Synth* S, hipStream_t s, GenTape* tape, const float* dy, float* dz, float* dcond, float* dg, float* dhar) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  tape_check(S, tape);
  RVC_REQUIRE(tape->recorded, "the tape holds no forward pass: call synth_forward_tape first");
  RVC_REQUIRE(S->f0 || !dhar, "no-f0 model: there is no harmonic source, dhar must be NULL");
  dec_backward(S, s, tape, dy, dz, dcond, dg, dhar);
  tape->backward_done = true;
}

// ------------------------------------------------------------------------------------------------ the flow's backward data pass
// ResidualCouplingBlock (reference models.py:150-196; modules.py ResidualCouplingLayer, WN, Flip) read backwards on ONE item at its own length T: d z_p -> d z and
// the flow's share of d g.  The recording forward (synth_forward_tape, record_flow) leaves per coupling f in the tape's flow block, fp32 [rows][T]:
//   flow{f}.h0 [H] (pre(x0), = flow{f}.x0), flow{f}.x{i} [H] (the input of WN layer i), flow{f}.a{i} [2 H] (in_layers[i](x{i}) + its slice of cond_layer(g))
// and the backward leaves its deltas beside them:
//   d.flow{f}.m [inter / 2] (post's output cotangent), d.flow{f}.a{i} [2 H], d.flow{f}.h0 [H] (pre's output cotangent), d.flow{f}.gc [1][6 H], d.flow.g [1][gin]
// The item runs at its own length, so its mask is all ones inside the tape; the kernels still take the length and write zero behind it.
static std::string flow_name(int f, const std::string& what) { return "flow" + std::to_string(f) + "." + what; }

// the weight images of the pass, built by the first recording forward (a handle that never records the flow never gets here)
static void flow_bwd_build(Synth* S) {
  FlowBwdImages& B = S->flow_bwd;
  if (B.built) return;
  const int H = S->hidden, half = S->inter / 2;
  RVC_REQUIRE(!S->flow_host[0].pre.empty(), "the flow's folded weights were not kept (no posterior was loaded at finalize)");
  RVC_REQUIRE(S->inter % 2 == 0 && half % 16 == 0 && H % 16 == 0, "the flow's backward kernels need inter_channels / 2 and hidden_channels to be multiples of 16");
  FlowBwdImages N;
  auto image = [&](const std::vector<float>& w, int Co, int Ci, int k, DevBuf<uint16_t>& img) {
    RVC_REQUIRE(w.size() == (size_t)Co * Ci * k, "flow convolution: weight size");
    std::vector<uint16_t> P;
    gen_bwd_conv_image(w.data(), Co, Ci, k, P);
    img.upload(P); N.bytes += P.size() * sizeof(uint16_t);
  };
  for (int f = 0; f < 4; ++f) {
    const FlowHostWeights& W = S->flow_host[f];
    image(W.pre, H, half, 1, N.pre[f]);
    image(W.post, half, H, 1, N.post[f]);
    for (int i = 0; i < 3; ++i) {
      image(W.in[i], 2 * H, H, 5, N.in[f][i]);
      image(W.rs[i], i < 2 ? 2 * H : H, H, 1, N.rs[f][i]);
    }
  }
  N.built = true;
  B = std::move(N);
  for (FlowHostWeights& W : S->flow_host) W = {};
}
size_t synth_flow_bwd_bytes(const Synth* S) { return S->flow_bwd.bytes; }

// the flow block's layout for an item of T frames: the recorded activations, the deltas, the backward's scratch (the [dx | dh] pair that a res_skip layer's
// transposed product reads as one 2 H-row operand, d acts, one ping-pong cotangent)
static void flow_tape_layout(GenTape& tape, const Synth* S, int T, hipStream_t s) {
  if (tape.flow_T == T && tape.flow_mem.p) return;
  for (auto it = tape.t.begin(); it != tape.t.end();) it = it->second.flow ? tape.t.erase(it) : std::next(it);
  const int H = S->hidden, IC = S->inter;
  size_t off = 0;
  auto add = [&](const std::string& name, int rows, long long cols) {
    tape.t[name] = {off, rows, cols, true};
    off += ((size_t)rows * (size_t)cols + 63) & ~size_t(63);
  };
  for (int f = 0; f < 4; ++f) {
    add(flow_name(f, "h0"), H, T);
    tape.t[flow_name(f, "x0")] = tape.t[flow_name(f, "h0")];      // WN's first input is pre's output: one tensor under both names
    for (int i = 1; i < 3; ++i) add(flow_name(f, "x" + std::to_string(i)), H, T);
    for (int i = 0; i < 3; ++i) add(flow_name(f, "a" + std::to_string(i)), 2 * H, T);
  }
  for (int f = 0; f < 4; ++f) {
    add("d." + flow_name(f, "m"), IC / 2, T);
    for (int i = 0; i < 3; ++i) add("d." + flow_name(f, "a" + std::to_string(i)), 2 * H, T);
    add("d." + flow_name(f, "h0"), H, T);
    add("d." + flow_name(f, "gc"), 1, 6 * H);
  }
  add("d.flow.g", 1, S->gin);
  add("flow.scratch.dxh", 2 * H, T); add("flow.scratch.dacts", H, T); add("flow.scratch.cur", IC, T);
  // what the flow's weight-gradient pass reads beside them (a handle with kept parameters only), behind everything a plain tape holds: pre's input and post's
  // input, the x-chain cotangent at the input of layers 1 and 2 and post^T d m, which flow.scratch.dxh holds only until the next layer overwrites it
  if (S->kept.on)
    for (int f = 0; f < 4; ++f) {
      add(flow_name(f, "xin"), IC / 2, T); add(flow_name(f, "out"), H, T);
      add("d." + flow_name(f, "x1"), H, T); add("d." + flow_name(f, "x2"), H, T); add("d." + flow_name(f, "skip"), H, T);
    }
  if (tape.flow_mem.n < off) { RVC_HIP_CHECK(hipStreamSynchronize(s)); tape.flow_mem.alloc(off); }      // (an earlier pass on this stream may still read the old block)
  tape.flow_T = T;
}

// tape null: nothing is launched, the return value is the number of launches of the plan (a constant of the net).  No atomics: two calls give the same bits.
static int flow_backward(const Synth* S, hipStream_t s, GenTape* tape, const float* dzp, float* dz, float* dg) {
  const FlowBwdImages& B = S->flow_bwd;
  const int H = S->hidden, IC = S->inter, half = IC / 2, T = tape ? tape->flow_T : 0, len = T;
  int launches = 0;
  auto P = [&](const std::string& name) -> float* { return tape ? tape->ptr(name) : nullptr; };
  // Y [R][T] = W'(D) (+ Res) under the mask; A: the taped pre-gate activation whose gate derivative the operand is formed with (D = d acts)
  auto gemm = [&](const DevBuf<uint16_t>* img, const float* D, const float* A, int Ck, int nt, const float* Res, float* Y, int R) {
    ++launches;
    if (!tape) return;
    ConvFlowBwdArgs a{D, T, T, A, H, reinterpret_cast<const unsigned char*>(img->p), Res, Y, T, R, (R + 127) & ~127, Ck, T, nt, -((nt - 1) / 2), len};
    ConvFlowBwdPlan p;
    RVC_REQUIRE(conv_flow_bwd_plan(a, p), "flow layer does not fit the data-gradient kernel");
    conv_flow_bwd_launch(p, s);
  };
  if (tape) { tape->mark(s, kFlowMark0 + 2); tape->flow_bwd_marks = 0; }
  float* dxh = P("flow.scratch.dxh"); float* dh = tape ? dxh + (size_t)H * T : nullptr;      // [dx | dh]: the x-chain cotangent above WN's output cotangent
  float* dacts = P("flow.scratch.dacts");
  const float* src = dzp;
  for (int f = 3; f >= 0; --f) {
    // Flip, and the coupling's x1 half: d x1 = d m = d x1' under the mask
    float* cur = (f & 1) ? P("flow.scratch.cur") : dz;
    float* dm = P("d." + flow_name(f, "m"));
    ++launches; if (tape) flow_unflip(s, src, cur, dm, IC, T, len);
    gemm(tape ? &B.post[f] : nullptr, dm, nullptr, half, 1, nullptr, dh, H);                                  // d h = post^T d m, the skip cotangent of every layer
    // a handle with kept parameters keeps what the scratch pair holds only for a while, as copies: no operand of the pass changes
    auto keep = [&](const std::string& name, const float* src) {
      if (!S->kept.on) return;
      ++launches;
      if (tape) RVC_HIP_CHECK(hipMemcpyAsync(P("d." + flow_name(f, name)), src, (size_t)H * T * sizeof(float), hipMemcpyDeviceToDevice, s));
    };
    keep("skip", dh);
    float* dgc = P("d." + flow_name(f, "gc"));
    for (int i = 2; i >= 0; --i) {
      const std::string si = std::to_string(i);
      // d acts = res_skip^T [dx | dh] (the last layer's res_skip has the skip rows only); d a = d acts times the gate's derivative, kept with its row sums
      if (i == 2) gemm(tape ? &B.rs[f][i] : nullptr, dh, nullptr, H, 1, nullptr, dacts, H);
      else gemm(tape ? &B.rs[f][i] : nullptr, dxh, nullptr, 2 * H, 1, nullptr, dacts, H);
      const float* a = P(flow_name(f, "a" + si));
      ++launches; if (tape) flow_gate_bwd(s, dacts, a, P("d." + flow_name(f, "a" + si)), dgc + (size_t)2 * H * i, H, T, len);
      // dx += in_layers[i]^T (d a): the x-chain cotangent is zero above the last layer; layer 0's is pre's output cotangent d h0
      gemm(tape ? &B.in[f][i] : nullptr, dacts, a, 2 * H, 5, i < 2 ? dxh : nullptr, i > 0 ? dxh : P("d." + flow_name(f, "h0")), H);
      if (i > 0) keep("x" + si, dxh);
    }
    gemm(tape ? &B.pre[f] : nullptr, P("d." + flow_name(f, "h0")), nullptr, H, 1, cur, cur, half);              // d x0 = d x0' + pre^T d h0
    src = cur;
  }
  // d g = sum over the couplings of cond_layer^T d gc
  ++launches;
  if (tape) {
    const float* W[4]; const float* G[4];
    for (int f = 0; f < 4; ++f) { W[f] = S->flow[f].wn.cond_w.p; G[f] = P("d." + flow_name(f, "gc")); }
    flow_cond_bwd(s, W, G, 6 * H, S->gin, P("d.flow.g"), dg);
    tape->mark(s, kFlowMark0 + 3); tape->flow_bwd_marks = tape->timing ? 2 : 0;
  }
  return launches;
}
int synth_flow_input_grad_launch_count(const Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  return flow_backward(S, nullptr, nullptr, nullptr, nullptr, nullptr);
}
void synth_flow_input_grad(Synth* S, hipStream_t s, GenTape* tape, const float* dzp, long long T, float* dz, float* dg) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  tape_check(S, tape);
  RVC_REQUIRE(tape->recorded && tape->flow_recorded && S->flow_bwd.built, "the tape holds no recorded flow: run synth_forward_tape with record_flow first");
  RVC_REQUIRE(T == tape->flow_T, "d z_p does not have the recorded item's length");
  flow_backward(S, s, tape, dzp, dz, dg);
  tape->flow_backward_done = true;
}
// [0]: the recorded flow forward (its four couplings and Flips), [1]: the last flow backward; waits for the events.  Returns the number of values
int gen_tape_flow_times(GenTape* T, float* ms, int cap) {
  if (!T->timing) return 0;
  int n = 0;
  auto put = [&](int a, int b) {
    RVC_HIP_CHECK(hipEventSynchronize(T->ev[b]));
    RVC_HIP_CHECK(hipEventElapsedTime(&ms[n++], T->ev[a], T->ev[b]));
  };
  if (T->flow_fwd_marks == 2 && n < cap) put(kFlowMark0, kFlowMark0 + 1); else return 0;
  if (T->flow_bwd_marks == 2 && n < cap) put(kFlowMark0 + 2, kFlowMark0 + 3);
  return n;
}

// ------------------------------------------------------------------------------------------------ the flow's weight-gradient pass
// d loss / d(parameter) for every flow.* tensor, summed over the B items, each at its own length, from the tapes' recorded flow and the deltas of
// synth_flow_input_grad.  Per coupling f, every sum also over the items and n < the item's length:
//   pre:               dW[o][c]    = sum_n d.h0[o][n] xin[c][n]                                   db = row sums of d.h0
//   in_layers.i:       dW[o][c][t] = sum_n d.a{i}[o][n] x{i}[c][n + t - 2]                         db = d.gc[2 H i ..), the row sums the data pass formed
//   res_skip_layers.i: dW[o][c]    = sum_n [d.x{i+1} | d.skip][o][n] gate(a{i})[c][n]              db = row sums of the pair (i = 2: d.skip alone, H rows)
//   post:              dW[o][c]    = sum_n d.m[o][n] out[c][n]                                     db = row sums of d.m
//   cond_layer:        dW[o][j]    = d.gc[o] g[j]                                                  db = d.gc
// and the chain through weight norm in the finishing step.  Every convolution is one launch of conv_flow_wgrad_kernel (the pair by a second base pointer) plus one
// finishing launch, cond_layer one finishing launch: 4 (2 + 6 + 6 + 1 + 2) = 68 whatever B and the lengths; tapes null: nothing is launched, the return value
// is that count.  The partial images live in the block the decoder's pass uses.  No atomics: two calls give the same bits.
struct FlowWgradLayer { ConvFlowWgradPlan x; FlowWgradFinishArgs f; bool gemm; };
static int flow_wgrad(Synth* S, hipStream_t s, GenTape* const* tapes, int B, float* const* grads) {
  const FlowKept& K = S->flow_kept;
  const int H = S->hidden, half = S->inter / 2;
  const bool run = tapes != nullptr;
  int launches = 0;
  auto items = [&](const std::string& name, size_t off = 0) { GenItems it{}; if (run) for (int b = 0; b < B; ++b) it.p[b] = tapes[b]->ptr(name) + off; return it; };
  auto grad = [&](const std::string& name) -> float* {
    if (!run) return nullptr;
    auto it = S->flow_index.find(name);
    RVC_REQUIRE(it != S->flow_index.end(), "no parameter tensor '" + name + "'");
    return grads[it->second];
  };
  std::vector<FlowWgradLayer> plan;
  auto finish_common = [&](FlowWgradFinishArgs& f, int R, int L, const std::string& prefix, const DevVec* v, const DevVec* g) {
    f.R = R; f.L = L; f.B = B; f.R0 = R;
    for (int b = 0; b < B; ++b) f.N[b] = tapes[b]->flow_T;
    if (v) {
      RVC_REQUIRE(v->n == (size_t)R * L && g->n == (size_t)R, "kept weight_v / weight_g do not have the layer's shape: " + prefix);
      f.v = v->p; f.g = g->p; f.gw = grad(prefix + ".weight_v"); f.gg = grad(prefix + ".weight_g");
    } else f.gw = grad(prefix + ".weight");
    f.gb = grad(prefix + ".bias");
  };
  // one convolution: Pn (R0 rows) and P2n (the rows behind them; empty: none) the tape names of the delta, Gn of the input; gc_off >= 0: the bias gradient is the
  // slice of d.flow{f}.gc there, otherwise the row sums of the delta
  auto gemm = [&](int f, const std::string& Pn, const std::string& P2n, const std::string& Gn, int R, int R0, int C, int k, int gate, const std::string& prefix,
                  const DevVec* v, const DevVec* g, long long gc_off) {
    launches += 2;
    if (!run) return;
    FlowWgradLayer L{};
    L.gemm = true;
    ConvFlowWgradArgs a{};
    const GenItems Pi = items(Pn), P2i = P2n.empty() ? Pi : items(P2n), Gi = items(Gn);
    for (int b = 0; b < B; ++b) { a.P[b] = Pi.p[b]; a.P2[b] = P2i.p[b]; a.G[b] = Gi.p[b]; a.N[b] = tapes[b]->flow_T; }
    a.B = B; a.R = R; a.R0 = R0; a.C = C; a.k = k; a.off0 = -((k - 1) / 2); a.gate = gate;
    RVC_REQUIRE(conv_flow_wgrad_plan(a, L.x), "flow layer does not fit the weight-gradient kernel: " + prefix);
    finish_common(L.f, R, C * k, prefix, v, g);
    L.f.pstride = (long long)R * C * k; L.f.splits = L.x.splits; L.f.R0 = R0;
    if (gc_off >= 0) { L.f.bias = 2; L.f.V = items("d." + flow_name(f, "gc"), (size_t)gc_off); }
    else { L.f.bias = 1; L.f.D = Pi; L.f.D2 = P2i; }
    plan.push_back(L);
  };
  for (int f = 0; f < 4; ++f) {
    const std::string p = "flow.flows." + std::to_string(2 * f) + ".";
    gemm(f, "d." + flow_name(f, "h0"), "", flow_name(f, "xin"), H, H, half, 1, 0, p + "pre", nullptr, nullptr, -1);
    for (int i = 0; i < 3; ++i) {
      const std::string si = std::to_string(i);
      gemm(f, "d." + flow_name(f, "a" + si), "", flow_name(f, "x" + si), 2 * H, 2 * H, H, 5, 0, p + "enc.in_layers." + si, &K.in_v[f][i], &K.in_g[f][i], (long long)2 * H * i);
    }
    for (int i = 0; i < 3; ++i) {
      const std::string si = std::to_string(i);
      if (i < 2) gemm(f, "d." + flow_name(f, "x" + std::to_string(i + 1)), "d." + flow_name(f, "skip"), flow_name(f, "a" + si), 2 * H, H, H, 1, 1,
                      p + "enc.res_skip_layers." + si, &K.rs_v[f][i], &K.rs_g[f][i], -1);
      else gemm(f, "d." + flow_name(f, "skip"), "", flow_name(f, "a" + si), H, H, H, 1, 1, p + "enc.res_skip_layers." + si, &K.rs_v[f][i], &K.rs_g[f][i], -1);
    }
    ++launches;
    if (run) {
      FlowWgradLayer L{};
      finish_common(L.f, 6 * H, S->gin, p + "enc.cond_layer", &K.cond_v[f], &K.cond_g[f]);
      L.f.outer = 1; L.f.bias = 2; L.f.V = items("d." + flow_name(f, "gc")); L.f.Gv = items("g");
      plan.push_back(L);
    }
    gemm(f, "d." + flow_name(f, "m"), "", flow_name(f, "out"), half, half, H, 1, 0, p + "post", nullptr, nullptr, -1);
  }
  if (run) {
    size_t most = 0;
    for (const FlowWgradLayer& L : plan) if (L.gemm) most = std::max(most, L.x.part_floats);
    if (S->wgrad_part.n < most) { RVC_HIP_CHECK(hipStreamSynchronize(s)); S->wgrad_part.alloc(most); }      // (an earlier pass on this stream may still read the old block)
    for (FlowWgradLayer& L : plan) {
      if (L.gemm) { L.x.a.part = S->wgrad_part.p; L.f.part = S->wgrad_part.p; conv_flow_wgrad_launch(L.x, s); }
      flow_wgrad_finish(s, L.f);
    }
  }
  return launches;
}
int synth_flow_param_count(const Synth* S) { RVC_REQUIRE(S->ready, "synth_finalize has not been called"); return (int)S->flow_params.size(); }
void synth_flow_param_info(const Synth* S, int k, std::string& name, std::vector<long long>& shape) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(k >= 0 && k < (int)S->flow_params.size(), "parameter index out of range");
  name = S->flow_params[k].name; shape = S->flow_params[k].shape;
}
long long synth_flow_param_total(const Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  long long n = 0;
  for (const DecParam& p : S->flow_params) { long long e = 1; for (long long d : p.shape) e *= d; n += e; }
  return n;
}
int synth_flow_weight_grad_launch_count(const Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  return flow_wgrad(const_cast<Synth*>(S), nullptr, nullptr, 1, nullptr);
}
void synth_flow_weight_grad(Synth* S, hipStream_t s, GenTape* const* tapes, int B, float* const* grads) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(S->kept.on, "flow_weight_grad needs the parameters on the device: call rvc_synth_keep_parameters(s, 1) before finalize (trainable=True)");
  RVC_REQUIRE(B >= 1 && B <= kGenWgradMaxItems, "1 <= B <= " + std::to_string(kGenWgradMaxItems) + " tapes per weight-gradient pass");
  RVC_REQUIRE(tapes && grads, "null argument");
  for (int b = 0; b < B; ++b) {
    RVC_REQUIRE(tapes[b], "null tape");
    tape_check(S, tapes[b]);
    RVC_REQUIRE(tapes[b]->recorded && tapes[b]->flow_recorded && tapes[b]->flow_T >= 1, "the tape holds no recorded flow: run synth_forward_tape with record_flow first");
    RVC_REQUIRE(tapes[b]->flow_backward_done, "the tape holds no flow backward pass after its last recording forward: call synth_flow_input_grad first");
  }
  for (size_t k = 0; k < S->flow_params.size(); ++k) RVC_REQUIRE(grads[k], "null gradient pointer");
  flow_wgrad(S, s, tapes, B, grads);
}

// ------------------------------------------------------------------------------------------------ the decoder's weight-gradient pass
// d loss / d(parameter) for every dec.* tensor, summed over the B items, from the tapes' activations and deltas (GeneratorNSF / Generator, reference models.py:460-566,
// ResBlock1 modules.py:295-308).  With lr the leaky ReLU (slope 0.1; 0.01 in front of conv_post) and every sum also over the items:
//   convs1.m of (i, j), dilation d:  dW[co][ci][t] = sum_n d.rb.t{m}[co][n] lr(y_m)[ci][n + t d - pad]          db = row sums of d.rb.t{m}
//   convs2.m:                        dW[co][ci][t] = sum_n Dy[co][n] lr(t_m)[ci][n + t - pad], Dy = d.rb.y{m+1} (m < 2) or d.out{i}     db = row sums of Dy
//   ups.i [Cin][Cout][k]:            dW[ci][co][t] = sum_n lr(prev)[ci][n] d.up{i}[co][u n + t - pad]            db = row sums of d.up{i}
//   noise_convs.i, conv_pre, cond, conv_post, m_source.l_linear: the direct kernels of conv_gen_wgrad.hip
// and the chain through weight norm in the finishing step.  Every dense convolution is one launch of conv_gen_wgrad_kernel plus one finishing launch whatever B and
// the segment; tapes null: nothing is launched, the return value is the number of launches of the plan.  No atomics: two calls give the same bits.
struct GenWgradLayer { ConvGenWgradPlan x; GenWgradFinishArgs f; int stage; };
static int dec_wgrad(Synth* S, hipStream_t s, GenTape* const* tapes, int B, float* const* grads) {
  const GenKept& K = S->kept;
  const int seg = S->segment, nu = (int)S->stages.size();
  const long long N = (long long)seg * S->upp;
  const bool run = tapes != nullptr;
  int launches = 0;
  auto items = [&](const std::string& name) { GenItems it{}; if (run) for (int b = 0; b < B; ++b) it.p[b] = tapes[b]->ptr(name); return it; };
  auto grad = [&](const std::string& name) -> float* {
    if (!run) return nullptr;
    auto it = S->dec_index.find(name);
    RVC_REQUIRE(it != S->dec_index.end(), "no parameter tensor '" + name + "'");
    return grads[it->second];
  };
  std::vector<GenWgradLayer> plan;
  // one dense layer: P / G the tape names of the two operands; prefix: the layer's state-dict prefix; v / g: the kept weight_v / weight_g (null: a plain weight
  // and no bias here); bias: the tape name of the delta whose row sums are the bias gradient (brows rows of bn columns)
  auto gemm = [&](int stage, const std::string& Pn, const std::string& Gn, int R, int C, int k, long long n, long long Tg, int cstride, int tstep, int off0, float sp, float sg,
                  const std::string& prefix, const DevVec* v, const DevVec* g, const std::string& bias, int brows, long long bn) {
    launches += 2;
    if (!run) return;
    GenWgradLayer L{};
    ConvGenWgradArgs a{};
    const GenItems Pi = items(Pn), Gi = items(Gn);
    for (int b = 0; b < B; ++b) { a.P[b] = Pi.p[b]; a.G[b] = Gi.p[b]; }
    a.B = B; a.R = R; a.C = C; a.k = k; a.N = (int)n; a.ldP = n; a.ldG = Tg; a.Tg = (int)Tg; a.cstride = cstride; a.tstep = tstep; a.off0 = off0; a.slopeP = sp; a.slopeG = sg;
    RVC_REQUIRE(n < (1LL << 31) && Tg < (1LL << 31) && conv_gen_wgrad_plan(a, L.x), "decoder layer does not fit the weight-gradient kernel: " + prefix);
    GenWgradFinishArgs& f = L.f;
    f.pstride = (long long)R * C * k; f.splits = L.x.splits; f.R = R; f.L = C * k;
    if (v) {
      RVC_REQUIRE(v->n == (size_t)R * C * k && g->n == (size_t)R, "kept weight_v / weight_g do not have the layer's shape: " + prefix);
      f.v = v->p; f.g = g->p; f.gw = grad(prefix + ".weight_v"); f.gg = grad(prefix + ".weight_g"); f.gb = grad(prefix + ".bias");
      f.D = items(bias); f.B = B; f.brows = brows; f.N = bn;
    } else {
      f.gw = grad(prefix + ".weight");
    }
    L.stage = stage;
    plan.push_back(L);
  };
  long long Tn = seg;
  for (int i = 0; i < nu; ++i) {
    const GenStage& st = S->stages[i];
    const int Cc = S->up_init >> (i + 1), Cin = S->up_init >> i;
    const long long Tc = Tn;
    Tn *= st.u;
    const std::string si = std::to_string(i);
    gemm(i, i > 0 ? "out" + std::to_string(i - 1) : "pre", "d.up" + si, Cin, Cc, st.k, Tc, Tn, st.u, 1, -((st.k - st.u) / 2), 0.1f, 1.f, "dec.ups." + si,
         run ? &K.up_v[i] : nullptr, run ? &K.up_g[i] : nullptr, "d.up" + si, Cc, Tn);
    for (int j = 0; j < 3; ++j) {
      const int k = S->rb_k[j];
      const std::string rb = "dec.resblocks." + std::to_string(i * 3 + j);
      for (int m = 0; m < 3; ++m) {
        const size_t q = (size_t)(i * 3 + j) * 3 + m;
        const int dil = S->rb_d[j][m];
        const std::string dt = "d." + rb_name(i, j, "t", m), dy = m < 2 ? "d." + rb_name(i, j, "y", m + 1) : "d.out" + si;
        gemm(i, dt, m > 0 ? rb_name(i, j, "y", m) : "up" + si, Cc, Cc, k, Tn, Tn, 1, dil, -((k * dil - dil) / 2), 1.f, 0.1f, rb + ".convs1." + std::to_string(m),
             run ? &K.c1_v[q] : nullptr, run ? &K.c1_g[q] : nullptr, dt, Cc, Tn);
        gemm(i, dy, rb_name(i, j, "t", m), Cc, Cc, k, Tn, Tn, 1, 1, -((k - 1) / 2), 1.f, 0.1f, rb + ".convs2." + std::to_string(m),
             run ? &K.c2_v[q] : nullptr, run ? &K.c2_g[q] : nullptr, dy, Cc, Tn);
      }
    }
  }
  gemm(nu, "d.pre", "z", S->up_init, S->inter, 7, seg, seg, 1, 1, -3, 1.f, 1.f, "dec.conv_pre", nullptr, nullptr, "", 0, 0);
  if (run) {
    size_t most = 0;
    for (const GenWgradLayer& L : plan) most = std::max(most, L.x.part_floats);
    if (S->wgrad_part.n < most) { RVC_HIP_CHECK(hipStreamSynchronize(s)); S->wgrad_part.alloc(most); }      // (an earlier pass on this stream may still read the old block)
    tapes[0]->mark(s, kWgradMark0);
    int stage = 0;
    for (GenWgradLayer& L : plan) {
      if (L.stage != stage) { stage = L.stage; tapes[0]->mark(s, kWgradMark0 + stage); }
      L.x.a.part = S->wgrad_part.p; L.f.part = S->wgrad_part.p;
      conv_gen_wgrad_launch(L.x, s);
      gen_wgrad_finish(s, L.f);
    }
  }
  // the direct kernels: conv_post, the conditioning (its bias sum is conv_pre's too), the noise convolutions, m_source
  const int Clast = S->up_init >> nu;
  ++launches; if (run) gen_wgrad_post(s, items("d.post"), items("out" + std::to_string(nu - 1)), B, Clast, N, 7, 3, 0.01f, grad("dec.conv_post.weight"));
  ++launches; if (run) gen_wgrad_cond(s, items("d.cond"), items("g"), B, S->up_init, S->gin, grad("dec.cond.weight"), grad("dec.cond.bias"), grad("dec.conv_pre.bias"));
  if (S->f0) {
    long long Ti = seg;
    for (int i = 0; i < nu; ++i) {
      const GenStage& st = S->stages[i];
      Ti *= st.u;
      const std::string nc = "dec.noise_convs." + std::to_string(i);
      ++launches;
      if (run) gen_wgrad_noise(s, items("d.up" + std::to_string(i)), items("har"), B, S->up_init >> (i + 1), Ti, N, st.noise_k, st.noise_s, st.noise_k > 1 ? st.noise_s / 2 : 0,
                               grad(nc + ".weight"), grad(nc + ".bias"));
    }
    ++launches; if (run) gen_wgrad_msource(s, items("d.har"), items("har"), items("sine"), B, N, grad("dec.m_source.l_linear.weight"), grad("dec.m_source.l_linear.bias"));
  }
  if (run) { tapes[0]->mark(s, kWgradMark0 + nu + 1); tapes[0]->wgrad_marks = nu + 2; }
  return launches;
}
int synth_dec_param_count(const Synth* S) { RVC_REQUIRE(S->ready, "synth_finalize has not been called"); return (int)S->dec_params.size(); }
void synth_dec_param_info(const Synth* S, int k, std::string& name, std::vector<long long>& shape) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(k >= 0 && k < (int)S->dec_params.size(), "parameter index out of range");
  name = S->dec_params[k].name; shape = S->dec_params[k].shape;
}
long long synth_dec_param_total(const Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  long long n = 0;
  for (const DecParam& p : S->dec_params) { long long e = 1; for (long long d : p.shape) e *= d; n += e; }
  return n;
}
size_t synth_kept_bytes(const Synth* S) { return S->kept.bytes; }
int synth_dec_weight_grad_launch_count(const Synth* S) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  return dec_wgrad(const_cast<Synth*>(S), nullptr, nullptr, 1, nullptr);
}
void synth_dec_weight_grad(Synth* S, hipStream_t s, GenTape* const* tapes, int B, float* const* grads) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(S->kept.on, "dec_weight_grad needs the parameters on the device: call rvc_synth_keep_parameters(s, 1) before finalize (trainable=True)");
  RVC_REQUIRE(B >= 1 && B <= kGenWgradMaxItems, "1 <= B <= " + std::to_string(kGenWgradMaxItems) + " tapes per weight-gradient pass");
  RVC_REQUIRE(tapes && grads, "null argument");
  for (int b = 0; b < B; ++b) {
    RVC_REQUIRE(tapes[b], "null tape");
    tape_check(S, tapes[b]);
    RVC_REQUIRE(tapes[b]->recorded, "the tape holds no forward pass: call synth_forward_tape first");
    RVC_REQUIRE(tapes[b]->backward_done, "the tape holds no backward pass after its last taped forward: call synth_dec_input_grad first");
  }
  for (size_t k = 0; k < S->dec_params.size(); ++k) RVC_REQUIRE(grads[k], "null gradient pointer");
  dec_wgrad(S, s, tapes, B, grads);
}
// the last weight-gradient pass's intervals on its first tape (timing on): stage 0 .. n - 1 (up-sampler and ResBlocks), then conv_pre and the direct kernels
int gen_tape_wgrad_times(GenTape* T, float* ms, int cap) {
  if (!T->timing || T->wgrad_marks < 2) return 0;
  int n = 0;
  for (int k = 1; k < T->wgrad_marks && n < cap; ++k) {
    RVC_HIP_CHECK(hipEventSynchronize(T->ev[kWgradMark0 + k]));
    RVC_HIP_CHECK(hipEventElapsedTime(&ms[n++], T->ev[kWgradMark0 + k - 1], T->ev[kWgradMark0 + k]));
  }
  return n;
}

// the phone features channel-major [feat_dim][T]: the caller's own tensor, or its transpose as the graph's first temporary
static const float* feat_cm_of(const Synth* S, hipStream_t s, Arena& A, const float* feat, int feat_channel_major, int T) {
  if (feat_channel_major) return feat;
  float* t = A.alloc<float>((size_t)S->feat_dim * T);
  if (!A.dry) transpose(s, feat, t, T, S->feat_dim, S->feat_dim, T, 1, 0, 0);
  return t;
}

static void synth_graph(Synth* S, hipStream_t s, Arena& A, const float* feat_cm, const long long* pitch, const float* pitchf, int sid,
                        const float* noise_z, const float* noise_src, int T, float* out, const SynthTaps* taps, int g0, int g1) {
  // [g0, g1): the frames the generator runs on (synth_infer: the keep window plus its halo; [0, T): the whole sequence).  Everything up to the flow is full length.
  const int W = g1 - g0;
  const int C = S->hidden, IC = S->inter;
  const bool dry = A.dry;
  const int h2 = conv_set_pair_arithmetic(-1);      // read once: the whole pass plans with the pair arithmetic it saw when it started
  const bool gs = synth_split_front(S);
  SplitImgs im;
  if (gs) im = split_imgs_alloc(S, s, A, T, W, 0);
  // ---- speaker conditioning vectors
  const float* g = S->emb_g.p + (size_t)sid * S->gin;
  float* pre_bias = A.alloc<float>(S->up_init);
  float* gcond[4];
  for (int f = 0; f < 4; ++f) gcond[f] = A.alloc<float>(6 * C);
  if (!dry) {
    gemv(s, S->dec_cond_w.p, g, S->dec_cond_b.p, pre_bias, S->up_init, S->gin, S->conv_pre.bd_);
    for (int f = 0; f < 4; ++f) gemv(s, S->flow[f].wn.cond_w.p, g, S->flow[f].wn.cond_b.p, gcond[f], 6 * C, S->gin, nullptr);
  }
  float* stats = enc_p_stats(S, s, A, gs, im, feat_cm, pitch, T, taps ? taps->enc_p_layer0 : nullptr);
  float* z = A.alloc<float>((size_t)IC * T);
  float* zf = A.alloc<float>((size_t)IC * T);
  if (!dry) {
    if (taps) { tap(A, s, taps->m_p, stats, (size_t)IC * T); tap(A, s, taps->logs_p, stats + (size_t)IC * T, (size_t)IC * T); }
    zp_sample(s, stats, noise_z, z, IC, T);
    if (taps) tap(A, s, taps->z_p, z, (size_t)IC * T);
  }
  // ---- flow (reverse)
  {
    const size_t mark = A.off;
    WnBufs wb;
    wb.hw = A.alloc<float>((size_t)2 * C * T);               // [h | wo]: the WaveNet's residual stream and its skip sum, adjacent rows
    wb.xin = A.alloc<float>((size_t)2 * C * T);
    wb.acts = gs ? nullptr : A.alloc<float>((size_t)C * T);
    wb.hw_s = im.hw_s; wb.acts_s = im.acts_s;
    if (!dry) {
      float* cur = z; float* oth = zf;
      for (int f = 3; f >= 0; --f) {
        flip_c(s, cur, oth, IC, T);
        std::swap(cur, oth);
        coupling_run(S, s, S->flow[f], gcond[f], gs, im, wb, cur, T, true);
      }
      if (cur != z) RVC_HIP_CHECK(hipMemcpyAsync(z, cur, (size_t)IC * T * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (taps) tap(A, s, taps->z, z, (size_t)IC * T);
    }
    A.off = mark;
  }
  // ---- generator
  const long long N = (long long)T * S->upp;
  float* har = S->f0 ? A.alloc<float>((size_t)N) : nullptr;
  if (S->f0) {
    float* rad = A.alloc<float>((size_t)T);
    float* tmp = A.alloc<float>((size_t)T);
    double* bsum = A.alloc<double>((size_t)((N + 1023) / 1024));
    if (!dry) {
      sine_source(s, pitchf, noise_src, har, taps ? taps->sine_waves : nullptr, rad, tmp, bsum, T, S->upp, (float)S->sr, S->lin_w, S->lin_b);
      if (taps) tap(A, s, taps->har_source, har, (size_t)N);
    }
  }
  gen_tail(S, s, A, gs, im.z_s, z, har, pre_bias, T, g0, W, h2, out, taps);
}

// SynthesizerTrnMs{256,768}NSFsid[_nono].forward for one item at its own length (reference models.py:781-796,:894-903): every mask is all ones.
static void synth_forward_graph(Synth* S, hipStream_t s, Arena& A, const float* feat_cm, const long long* pitch, const float* pitchf, const float* spec, int sid,
                                const float* noise_q, const float* noise_src, int T, int ids, float* out, const SynthForwardTaps* taps, GenTape* tape,
                                bool record_flow) {
  const int C = S->hidden, IC = S->inter, seg = S->segment;
  Posterior& Q = S->post_enc;
  const bool dry = A.dry;
  const int h2 = conv_set_pair_arithmetic(-1);
  const long long tp = split_image_tp(T);
  ConvEpilogue E0;
  bool gs = synth_split_front(S) && conv_x3s_eligible(Q.pre) && conv_x3s_eligible(Q.proj) && wn_split_eligible(Q.wn);
  for (int f = 0; f < 4 && gs; ++f) gs = conv_x3s_eligible(S->flow[f].post);
  SplitImgs im;
  if (gs) im = split_imgs_alloc(S, s, A, T, seg, Q.Kp);
  // ---- speaker conditioning vectors
  const float* g = S->emb_g.p + (size_t)sid * S->gin;
  float* pre_bias = A.alloc<float>(S->up_init);
  float* gcond[4];
  for (int f = 0; f < 4; ++f) gcond[f] = A.alloc<float>(6 * C);
  float* gcond_q = A.alloc<float>((size_t)2 * C * Q.wn.n);
  if (!dry) {
    gemv(s, S->dec_cond_w.p, g, S->dec_cond_b.p, pre_bias, S->up_init, S->gin, S->conv_pre.bd_);
    for (int f = 0; f < 4; ++f) gemv(s, S->flow[f].wn.cond_w.p, g, S->flow[f].wn.cond_b.p, gcond[f], 6 * C, S->gin, nullptr);
    gemv(s, Q.wn.cond_w.p, g, Q.wn.cond_b.p, gcond_q, 2 * C * Q.wn.n, S->gin, nullptr);
  }
  // ---- enc_p -> m_p, logs_p
  float* stats = enc_p_stats(S, s, A, gs, im, feat_cm, pitch, T, nullptr);
  if (!dry && taps) { tap(A, s, taps->m_p, stats, (size_t)IC * T); tap(A, s, taps->logs_p, stats + (size_t)IC * T, (size_t)IC * T); }
  // ---- enc_q -> z, m_q, logs_q
  float* stats_q = A.alloc<float>((size_t)2 * IC * T);
  float* z = A.alloc<float>((size_t)IC * T);
  float* zp = A.alloc<float>((size_t)IC * T);
  float* zf = A.alloc<float>((size_t)IC * T);
  {
    const size_t mark = A.off;
    WnBufs wb;
    wb.hw = A.alloc<float>((size_t)2 * C * T);
    wb.xin = A.alloc<float>((size_t)2 * C * T);
    wb.acts = gs ? nullptr : A.alloc<float>((size_t)C * T);
    wb.hw_s = im.hw_s; wb.acts_s = im.acts_s;
    // the operand of pre: Kp rows, the rows behind the spectrogram's zero (its weight columns there are zero too)
    float* specp = A.alloc<float>((size_t)Q.Kp * T);
    if (!dry) {
      RVC_HIP_CHECK(hipMemcpyAsync(specp, spec, (size_t)Q.spec * T * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (Q.Kp > Q.spec) RVC_HIP_CHECK(hipMemsetAsync(specp + (size_t)Q.spec * T, 0, (size_t)(Q.Kp - Q.spec) * T * sizeof(float), s));
      float* h = wb.hw; float* wo = wb.hw + (size_t)C * T;
      if (gs) {
        split_image_from_f32(s, specp, T, Q.Kp, T, im.spec_s, tp);
        ConvEpilogue Eh; Eh.ys_out = wb.hw_s; Eh.ys_tp = tp;
        conv_x3s_run(Q.pre, s, im.spec_s, tp, T, h, T, Eh);
      } else conv1d_run(Q.pre, s, specp, T, T, h, T, E0);
      wn_run(s, Q.wn, gcond_q, gs, wb, C, T);
      if (gs) conv_x3s_run(Q.proj, s, wb.hw_s + split_image_bytes(C, T), tp, T, stats_q, T, E0);
      else conv1d_run(Q.proj, s, wo, T, T, stats_q, T, E0);
      posterior_sample(s, stats_q, noise_q, z, IC, T);
      if (taps) { tap(A, s, taps->m_q, stats_q, (size_t)IC * T); tap(A, s, taps->logs_q, stats_q + (size_t)IC * T, (size_t)IC * T); tap(A, s, taps->z, z, (size_t)IC * T); }
      // ---- flow (forward): coupling 0 .. 3, each followed by Flip (reference models.py:185-192)
      RVC_HIP_CHECK(hipMemcpyAsync(zp, z, (size_t)IC * T * sizeof(float), hipMemcpyDeviceToDevice, s));
      float* cur = zp; float* oth = zf;
      if (record_flow) tape->mark(s, kFlowMark0);
      for (int f = 0; f < 4; ++f) {
        WnRecord rec;
        if (record_flow)
          for (int i = 0; i < 3; ++i) { rec.x[i] = tape->ptr(flow_name(f, "x" + std::to_string(i))); rec.a[i] = tape->ptr(flow_name(f, "a" + std::to_string(i))); }
        coupling_run(S, s, S->flow[f], gcond[f], gs, im, wb, cur, T, false, record_flow ? &rec : nullptr);
        if (record_flow && S->kept.on) {      // copies only: x0 passes through the coupling unchanged, the skip sum stays in the WaveNet's buffer until the next one
          RVC_HIP_CHECK(hipMemcpyAsync(tape->ptr(flow_name(f, "xin")), cur, (size_t)(IC / 2) * T * sizeof(float), hipMemcpyDeviceToDevice, s));
          RVC_HIP_CHECK(hipMemcpyAsync(tape->ptr(flow_name(f, "out")), wb.hw + (size_t)C * T, (size_t)C * T * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        flip_c(s, cur, oth, IC, T);
        std::swap(cur, oth);
      }
      if (record_flow) { tape->mark(s, kFlowMark0 + 1); tape->flow_fwd_marks = tape->timing ? 2 : 0; }
      if (taps) tap(A, s, taps->z_p, cur, (size_t)IC * T);
    }
    A.off = mark;
  }
  // ---- the slice as a sequence of its own through the generator
  // (with a tape the slice and the source are its first two tensors)
  const long long N = (long long)seg * S->upp;
  float* zs = tape ? tape->ptr("z") : A.alloc<float>((size_t)IC * seg);
  float* har = !S->f0 ? nullptr : (tape ? tape->ptr("har") : A.alloc<float>((size_t)N));
  if (!dry) segment_gather(s, z, IC, T, ids, seg, zs);
  if (S->f0) {
    float* pfs = A.alloc<float>((size_t)seg);
    float* rad = A.alloc<float>((size_t)seg);
    float* tmp = A.alloc<float>((size_t)seg);
    double* bsum = A.alloc<double>((size_t)((N + 1023) / 1024));
    if (!dry) {
      segment_gather(s, pitchf, 1, T, ids, seg, pfs);
      sine_source(s, pfs, noise_src, har, tape && S->kept.on ? tape->ptr("sine") : nullptr, rad, tmp, bsum, seg, S->upp, (float)S->sr, S->lin_w, S->lin_b);
    }
  }
  if (tape && S->kept.on && !dry) RVC_HIP_CHECK(hipMemcpyAsync(tape->ptr("g"), g, (size_t)S->gin * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (tape) { if (!dry) gen_tail_tape(S, s, *tape, pre_bias, out); }
  else gen_tail(S, s, A, gs, im.z_s, zs, har, pre_bias, seg, 0, seg, h2, out, nullptr);
}

// [keep0, keep1): the frames whose samples the caller keeps.  out[keep0 upp, keep1 upp) is defined, nothing else is promised: the generator (conv_pre on) runs on the
// window widened by its halo, clamped to the sequence; enc_p, the flow and the harmonic source run at full length (global attention, a running phase sum, and the
// caller's noise tensors keep their shapes).  halo < 0: synth_dec_halo_frames (anything else is for the test that shows the derived value is tight).
// The frames [g0, g1) the generator runs on for a keep window: the window widened by the halo, clamped, and its start moved down to a frame at which every
// stage's first column is a multiple of conv1d_residual_period of the pair launches planned for the whole sequence - the persistent pair kernel adds the
// residual of a tile block by block, so the order of a column's additions depends on its place in the tile (40k_v2 at 30 s: 64 frames, [89, ..) -> [64, ..)).
void synth_window_frames(const Synth* S, int T, long long keep0, long long keep1, int halo, int* og0, int* og1) {
  RVC_REQUIRE(keep0 >= 0 && keep0 < keep1 && keep1 <= T, "keep window must be a non-empty range of frames inside [0, T)");
  const int Hd = halo < 0 ? synth_dec_halo_frames(S) : halo;
  int g0 = (int)std::max<long long>(0, keep0 - Hd), g1 = (int)std::min<long long>(T, keep1 + Hd);
  // a window of a few frames would leave some launches fewer tiles than the kernel the whole sequence is planned on accepts: widened (costs microseconds)
  const int kMinWindow = 128;
  if (g1 - g0 < kMinWindow && halo < 0) { g0 = std::max(0, std::min(g0, T - kMinWindow)); g1 = std::min(T, std::max(g1, g0 + kMinWindow)); }
  const int h2 = conv_set_pair_arithmetic(-1);
  long long align = 1, pu = 1;
  for (const GenStage& st : S->stages) {
    pu *= st.u;
    const long long Tn = (long long)T * pu;
    if (Tn >= (1LL << 31)) break;
    const long long per = gen_stage_pairs(st, (int)Tn, h2).period;
    const long long need = per / gcd_ll(per, pu);                // frames whose columns at this stage are a multiple of the period
    align = align / gcd_ll(align, need) * need;
  }
  g0 -= (int)(g0 % align);
  *og0 = g0; *og1 = g1;
}

void synth_infer_window(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, int sid,
                        const float* noise_z, const float* noise_src, int T, float* out, const SynthTaps* taps, long long keep0, long long keep1, int halo) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(T >= 11, "need at least 11 frames (relative-position window)");
  RVC_REQUIRE(sid >= 0 && sid < S->n_spk, "speaker id out of range");
  int g0, g1;
  synth_window_frames(S, T, keep0, keep1, halo, &g0, &g1);
  if (taps) { g0 = 0; g1 = T; }                                  // (the generator's taps are whole tensors)
  Arena& A = S->arena;
  arena_passes(A, [&] { synth_graph(S, s, A, feat_cm_of(S, s, A, feat, feat_channel_major, T), pitch, pitchf, sid, noise_z, noise_src, T, out, taps, g0, g1); });
}
void synth_infer(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, int sid,
                 const float* noise_z, const float* noise_src, int T, float* out, const SynthTaps* taps) {
  synth_infer_window(S, s, feat, feat_channel_major, pitch, pitchf, sid, noise_z, noise_src, T, out, taps, 0, T, -1);
}

void synth_forward_tape(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, const float* spec,
                        int sid, const float* noise_q, const float* noise_src, int T, int ids, float* out, const SynthForwardTaps* taps, GenTape* tape,
                        bool record_flow) {
  RVC_REQUIRE(S->ready, "synth_finalize has not been called");
  RVC_REQUIRE(tape || !record_flow, "record_flow needs a tape");
  if (tape) { tape_check(S, tape); tape->recorded = false; tape->backward_done = false; tape->flow_recorded = false; tape->flow_backward_done = false; }
  RVC_REQUIRE(S->post_enc.built, "no posterior encoder loaded: the checkpoint had no enc_q.* tensors (an inference checkpoint)");
  RVC_REQUIRE(S->segment > 0, "segment_size is not set in the configuration");
  RVC_REQUIRE(T >= S->segment && T >= 11, "the sequence is shorter than the segment");
  RVC_REQUIRE(ids >= 0 && ids <= T - S->segment, "slice start outside [0, T - segment]");
  RVC_REQUIRE(sid >= 0 && sid < S->n_spk, "speaker id out of range");
  if (record_flow) { flow_bwd_build(S); flow_tape_layout(*tape, S, T, s); }
  Arena& A = S->arena;
  arena_passes(A, [&] {
    synth_forward_graph(S, s, A, feat_cm_of(S, s, A, feat, feat_channel_major, T), pitch, pitchf, spec, sid, noise_q, noise_src, T, ids, out, taps, tape, record_flow);
  });
  if (tape) { tape->recorded = true; tape->flow_recorded = record_flow; }
}

void synth_forward(Synth* S, hipStream_t s, const float* feat, int feat_channel_major, const long long* pitch, const float* pitchf, const float* spec, int sid,
                   const float* noise_q, const float* noise_src, int T, int ids, float* out, const SynthForwardTaps* taps) {
  synth_forward_tape(S, s, feat, feat_channel_major, pitch, pitchf, spec, sid, noise_q, noise_src, T, ids, out, taps, nullptr);
}

size_t synth_workspace(const Synth* M) { return M->arena.cap; }

}  // namespace rvc
