// HubertModelWithFinalProj.extract_features as a HIP kernel graph (reference lib/infer_pack/loaders.py:55-61 over
// transformers/models/hubert/modeling_hubert.py:45-477,878-955): 7-layer conv feature encoder (GroupNorm on layer 0),
// LayerNorm + projection, grouped k=128 positional conv, post-LN transformer layers.  Channel-major [C][T] throughout.
#include "model_encoder.h"
#include "models.h"

namespace rvc {

static const EncoderShape kHubEncoder = {768, 12, 64, 0, ACT_GELU, 3072};

struct HubertWeights {   // what hubert_finalize builds, and what the graph has learnt about it
  ZeroedBlock pos_img;   // image of the positional convolution's input: margins known to be zero (key: T)
  OwnedConvLayer conv[7];
  DevVec gn_g, gn_b, fp_g, fp_b, enc_g, enc_b;
  DevVec w0;            // conv_layers.0 raw [512][10]: the fused conv0 + GroupNorm + GELU kernels evaluate it from the audio
  OwnedConvLayer proj, pos, final_proj;
  std::vector<EncoderLayer> layers;
};
struct Hubert : HubertWeights {
  Ctx* ctx = nullptr;
  Arena arena;
  TensorStore ts;
  bool ready = false;
};

static const int kKern[7] = {10, 3, 3, 3, 3, 2, 2};
static const int kStride[7] = {5, 2, 2, 2, 2, 2, 2};

long long hubert_num_frames(long long L) {
  long long t = L;
  for (int i = 0; i < 7; ++i) { if (t < kKern[i]) return 0; t = (t - kKern[i]) / kStride[i] + 1; }
  return t;
}

Hubert* hubert_create(Ctx* ctx) { Hubert* H = new Hubert(); H->ctx = ctx; return H; }
void hubert_set_tensor(Hubert* H, const char* name, const float* d, const long long* shape, int ndim) { H->ts.set(name, d, shape, ndim); }

void hubert_destroy(Hubert* H) { delete H; }

static void linear_layer(ConvLayer& L, const TensorStore& ts, const std::string& p, int out, int in) {
  conv1d_layer_init(L, ts.get(p + ".weight", {out, in}).data.data(), ts.get(p + ".bias", {out}).data.data(), out, in, 1, 1, 0, 1, 1);
}

void hubert_finalize(Hubert* H) {
  H->ready = false; static_cast<HubertWeights&>(*H) = {};   // a finalize that throws leaves the handle not ready
  const TensorStore& ts = H->ts;
  // the k = 1 projections (feature projection, q/k, out, feed-forward, final_proj) also get a bf16x3 split weight image
  // (conv_x3.hip); strided / grouped convolutions and the activation x activation products of attention stay on the fp32 kernel
  ConvBuildScope x3scope(H->ctx->precision);
  // conv0: Conv1d(1, 512, 10, stride 5) == Linear(10 -> 512) over im2col frames
  conv1d_layer_init(H->conv[0], ts.get("feature_extractor.conv_layers.0.conv.weight", {512, 1, 10}).data.data(), nullptr, 512, 10, 1, 1, 0, 1, 1);
  H->w0.upload(ts.get("feature_extractor.conv_layers.0.conv.weight", {512, 1, 10}).data);
  for (int i = 1; i < 7; ++i)
    conv1d_layer_init(H->conv[i], ts.get("feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight", {512, 512, kKern[i]}).data.data(),
                      nullptr, 512, 512, kKern[i], kStride[i], 0, 1, 1);
  H->gn_g.upload(ts.get("feature_extractor.conv_layers.0.layer_norm.weight", {512}).data);
  H->gn_b.upload(ts.get("feature_extractor.conv_layers.0.layer_norm.bias", {512}).data);
  H->fp_g.upload(ts.get("feature_projection.layer_norm.weight", {512}).data);
  H->fp_b.upload(ts.get("feature_projection.layer_norm.bias", {512}).data);
  linear_layer(H->proj, ts, "feature_projection.projection", 768, 512);
  {
    // weight_norm(dim=2): w[:, :, k] = v[:, :, k] * g[k] / ||v[:, :, k]||   (modeling_hubert.py:61-77); both key spellings accepted
    const bool par = ts.has("encoder.pos_conv_embed.conv.parametrizations.weight.original1");
    const HostTensor& v = ts.get(par ? "encoder.pos_conv_embed.conv.parametrizations.weight.original1" : "encoder.pos_conv_embed.conv.weight_v", {768, 48, 128});
    const HostTensor& g = ts.get(par ? "encoder.pos_conv_embed.conv.parametrizations.weight.original0" : "encoder.pos_conv_embed.conv.weight_g", {1, 1, 128});
    std::vector<float> w(v.numel());
    for (int k = 0; k < 128; ++k) {
      double s = 0.0;
      for (size_t r = 0; r < (size_t)768 * 48; ++r) { const double x = v.data[r * 128 + k]; s += x * x; }
      const float sc = (float)((double)g.data[k] / std::sqrt(s));
      for (size_t r = 0; r < (size_t)768 * 48; ++r) w[r * 128 + k] = v.data[r * 128 + k] * sc;
    }
    conv1d_layer_init(H->pos, w.data(), ts.get("encoder.pos_conv_embed.conv.bias", {768}).data.data(), 768, 768, 128, 1, 64, 1, 16);
  }
  H->enc_g.upload(ts.get("encoder.layer_norm.weight", {768}).data);
  H->enc_b.upload(ts.get("encoder.layer_norm.bias", {768}).data);
  int nl = 0;
  while (ts.has("encoder.layers." + std::to_string(nl) + ".attention.q_proj.weight")) ++nl;
  RVC_REQUIRE(nl >= 11, "expected at least 11 encoder layers");
  H->layers.resize(nl);
  const float qs = 0.125f;   // head_dim^-0.5 = 64^-0.5, exact in fp32
  for (int l = 0; l < nl; ++l) {
    EncoderLayer& Y = H->layers[l];
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    const HostTensor& wq = ts.get(p + "attention.q_proj.weight", {768, 768});
    const HostTensor& wk = ts.get(p + "attention.k_proj.weight", {768, 768});
    const HostTensor& bq = ts.get(p + "attention.q_proj.bias", {768});
    const HostTensor& bk = ts.get(p + "attention.k_proj.bias", {768});
    // one 768 -> 2304 projection: q (scaled), k, v rows; v's bias is added after the attention (softmax rows sum to 1)
    const HostTensor& wv = ts.get(p + "attention.v_proj.weight", {768, 768});
    std::vector<float> w(3 * (size_t)768 * 768), b(3 * 768, 0.f);
    for (size_t i = 0; i < (size_t)768 * 768; ++i) { w[i] = wq.data[i] * qs; w[(size_t)768 * 768 + i] = wk.data[i]; w[2 * (size_t)768 * 768 + i] = wv.data[i]; }
    for (int i = 0; i < 768; ++i) { b[i] = bq.data[i] * qs; b[768 + i] = bk.data[i]; }
    conv1d_layer_init(Y.qkv, w.data(), b.data(), 2304, 768, 1, 1, 0, 1, 1);
    Y.bv.upload(ts.get(p + "attention.v_proj.bias", {768}).data);
    linear_layer(Y.o, ts, p + "attention.out_proj", 768, 768);
    linear_layer(Y.ff1, ts, p + "feed_forward.intermediate_dense", 3072, 768);
    linear_layer(Y.ff2, ts, p + "feed_forward.output_dense", 768, 3072);
    Y.g1.upload(ts.get(p + "layer_norm.weight", {768}).data); Y.b1.upload(ts.get(p + "layer_norm.bias", {768}).data);
    Y.g2.upload(ts.get(p + "final_layer_norm.weight", {768}).data); Y.b2.upload(ts.get(p + "final_layer_norm.bias", {768}).data);
  }
  linear_layer(H->final_proj, ts, "final_proj", 256, 768);
  H->ts.clear();
  H->ready = true;
}

static void hubert_graph(Hubert* H, hipStream_t s, Arena& A, const float* audio, long long L, int version, int n_layers, float* out_rm,
                         float* out_cm, const HubertTaps* taps) {
  const bool dry = A.dry;
  ConvEpilogue E0;
  int Tc[8]; Tc[0] = (int)L;
  for (int i = 0; i < 7; ++i) Tc[i + 1] = (Tc[i] - kKern[i]) / kStride[i] + 1;
  const int T = Tc[7];
  // the positional convolution (k = 128, 16 groups) reads its input as a split-resident image through row offsets -64 .. +63: the margins
  // of that image are its zero padding, so it lives in a block of its own (first allocation, never aliased) that is zeroed per (layout, T)
  const bool pos_s = conv_x3s_eligible(H->pos) && conv_x3s_eligible(H->proj);
  unsigned char* hpos_s = nullptr;
  if (pos_s) {
    const size_t img0 = A.off;
    hpos_s = A.alloc<unsigned char>(split_image_bytes(768, T));
    H->pos_img.ensure_zero(A, img0, A.off - img0, T, 0, s);
  }
  // ---- feature encoder
  // Layers 1 .. 6 (k = 3 / 2, stride 2, no padding) on the split-resident GEMM: every layer's output is written by its producer's epilogue as the bf16 hi / lo
  // image of the next one, DE-INTERLEAVED (even | odd positions), so that a stride-2 tap is a row offset and no layer converts its input per tile; the exact-erf
  // GELU sits in the epilogue (the pipelined kernel ran it as a second pass over the tensor).  Without bf16x3 images: the fp32 path on conv_x3p_kernel / conv_x3_kernel.
  bool s2 = true;
  for (int i = 1; i < 7 && s2; ++i) s2 = conv_x3s_s2_eligible(H->conv[i]) && Tc[i + 1] >= 1;
  float* feat = nullptr;
  if (s2) {
    unsigned char* imgA = A.alloc<unsigned char>(split_s2_bytes(512, Tc[1]));
    unsigned char* imgB = A.alloc<unsigned char>(split_s2_bytes(512, Tc[2]));
    double* c0part = A.alloc<double>(hubert_conv0_scratch_doubles(512, Tc[1]));
    float* c0stat = A.alloc<float>(1024);
    feat = A.alloc<float>((size_t)512 * Tc[7]);
    if (!dry) {
      hubert_conv0_gn_gelu_img(s, audio, L, H->w0.p, H->gn_g.p, H->gn_b.p, 512, Tc[1], 1e-5f, imgA, split_s2_tp(Tc[1]), kSplitMargin, split_s2_h(Tc[1]), c0part, c0stat);
      unsigned char* in_s = imgA; unsigned char* out_s = imgB;
      for (int i = 1; i < 7; ++i) {
        const SplitGeom g = split_geom_s2(kKern[i], Tc[i]);
        ConvEpilogue Eg; Eg.act = ACT_GELU;
        if (i < 6) { Eg.ys_out = out_s; Eg.ys_tp = split_s2_tp(Tc[i + 1]); Eg.ys_deint_h = split_s2_h(Tc[i + 1]); }
        conv_x3s_run(H->conv[i], s, in_s, split_s2_tp(Tc[i]), Tc[i + 1], i < 6 ? nullptr : feat, Tc[i + 1], Eg, &g);
        std::swap(in_s, out_s);      // ping-pong inside the two largest images (each layer's output is half its input)
      }
    }
  } else {
  float* c0 = A.alloc<float>((size_t)512 * Tc[1]);
  float* c1 = A.alloc<float>((size_t)512 * Tc[2]);
  double* c0part = A.alloc<double>(hubert_conv0_scratch_doubles(512, Tc[1]));
  float* c0stat = A.alloc<float>(1024);
  if (!dry) hubert_conv0_gn_gelu(s, audio, L, H->w0.p, H->gn_g.p, H->gn_b.p, 512, Tc[1], 1e-5f, c0, Tc[1], c0part, c0stat);
  float* in = c0; float* outb = c1;
  for (int i = 1; i < 7; ++i) {
    if (!dry) { ConvEpilogue Eg; Eg.act = ACT_GELU; conv1d_run(H->conv[i], s, in, Tc[i], Tc[i], outb, Tc[i + 1], Eg); }
    std::swap(in, outb);      // ping-pong inside the two largest buffers (each layer's output is smaller than its input)
  }
  feat = in;
  }
  // feat: [512][T]
  if (taps) tap(A, s, taps->conv_stack, feat, (size_t)512 * T);
  // Split-resident GEMM path (conv_x3s.hip): the activations that feed a k = 1 projection live as the bf16 hi / lo image the kernel stages,
  // written by their producers (LayerNorm, the attention's epilogue, FFN1's GELU epilogue); the fp32 copy is kept only where a residual or
  // the attention reads it.  Needs the bf16x3 weight images (context precision 1 / 2); without them the fp32-input kernels run.
  int need = version == 1 ? 8 : 11;
  if (n_layers > 0) need = n_layers;
  RVC_REQUIRE(need <= (int)H->layers.size(), "not enough encoder layers loaded");
  bool gs = conv_x3s_eligible(H->proj) && (version != 1 || conv_x3s_eligible(H->final_proj));
  for (int l = 0; l < need && gs; ++l) {
    const EncoderLayer& Y = H->layers[l];
    gs = conv_x3s_eligible(Y.qkv) && conv_x3s_eligible(Y.o) && conv_x3s_eligible(Y.ff1) && conv_x3s_eligible(Y.ff2);
  }
  const long long tp = split_image_tp(T);
  float* ln = gs ? nullptr : A.alloc<float>((size_t)512 * T);
  unsigned char* ln_s = gs ? A.alloc<unsigned char>(split_image_bytes(512, T)) : nullptr;
  unsigned char* hs = gs ? A.alloc<unsigned char>(split_image_bytes(768, T)) : nullptr;
  float* h = A.alloc<float>((size_t)768 * T);
  float* hb = A.alloc<float>((size_t)768 * T);
  if (!dry) {
    if (gs) {
      layernorm_c_split(s, feat, H->fp_g.p, H->fp_b.p, nullptr, ln_s, tp, kSplitMargin, 512, T, T, 1e-5f);
      ConvEpilogue Epj; if (pos_s) { Epj.ys_out = hpos_s; Epj.ys_tp = tp; }
      conv_x3s_run(H->proj, s, ln_s, tp, T, h, T, Epj);
    } else {
      layernorm_c(s, feat, nullptr, H->fp_g.p, H->fp_b.p, ln, 512, T, T, 1e-5f);
      conv1d_run(H->proj, s, ln, T, T, h, T, E0);
    }
    if (taps && taps->pos_conv) { ConvEpilogue Ep; Ep.act = ACT_GELU; Ep.tout_limit = T; conv1d_run(H->pos, s, h, T, T, taps->pos_conv, T, Ep); }
    ConvEpilogue Ep; Ep.act = ACT_GELU; Ep.act_before_res = 1; Ep.R = h; Ep.ldR = T; Ep.tout_limit = T;
    if (gs && pos_s) { Ep.tout_limit = 0; conv_x3s_run(H->pos, s, hpos_s, tp, T, hb, T, Ep); }      // 16 groups x one 64-row tile, 384 (chunk, tap) units
    else conv1d_run(H->pos, s, h, T, T, hb, T, Ep);
    if (gs) layernorm_c_split(s, hb, H->enc_g.p, H->enc_b.p, h, hs, tp, kSplitMargin, 768, T, T, 1e-5f);
    else layernorm_c(s, hb, nullptr, H->enc_g.p, H->enc_b.p, h, 768, T, T, 1e-5f);
  }
  {
    const size_t mark = A.off;
    // attention on split-resident operands (attention_dma.hip): q / k as one image, V^T written by the same launch; without them fp32 q / k / v
    float* qk = gs ? nullptr : A.alloc<float>((size_t)2304 * T);
    float* vr = gs ? nullptr : A.alloc<float>((size_t)T * 768);
    unsigned char* qk_s = gs ? A.alloc<unsigned char>(split_image_bytes(1536, T)) : nullptr;
    unsigned char* vt_s = gs ? A.alloc<unsigned char>(attention_vt_bytes(768, T)) : nullptr;
    float* attn = gs ? nullptr : A.alloc<float>((size_t)768 * T);
    float* ff = gs ? nullptr : A.alloc<float>((size_t)3072 * T);
    unsigned char* attn_s = gs ? A.alloc<unsigned char>(split_image_bytes(768, T)) : nullptr;
    unsigned char* ff_s = gs ? A.alloc<unsigned char>(split_image_bytes(3072, T)) : nullptr;
    if (!dry) {
      if (gs) attention_vt_clear_tail(s, vt_s, 768, T);
      const EncoderSplitBufs sb = {h, hb, hs, qk_s, vt_s, attn_s, ff_s};
      const EncoderPlainBufs pb = {h, hb, qk, vr, attn, ff};
      for (int l = 0; l < need; ++l) {
        if (taps && l == 0) tap(A, s, taps->hidden_0, h, (size_t)768 * T);
        if (taps && l == 8) tap(A, s, taps->hidden_8, h, (size_t)768 * T);
        if (gs) encoder_layer_run_split(s, H->layers[l], kHubEncoder, sb, T);
        else encoder_layer_run_plain(s, H->layers[l], kHubEncoder, pb, T);
      }
      if (taps && need == 8) tap(A, s, taps->hidden_8, h, (size_t)768 * T);
    }
    A.off = mark;
  }
  const float* res = h; int D = 768;
  if (version == 1) {
    float* fp = A.alloc<float>((size_t)256 * T);
    if (!dry) { if (gs) conv_x3s_run(H->final_proj, s, hs, tp, T, fp, T, E0); else conv1d_run(H->final_proj, s, h, T, T, fp, T, E0); }
    res = fp; D = 256;
  }
  if (!dry) {
    if (out_cm) RVC_HIP_CHECK(hipMemcpyAsync(out_cm, res, (size_t)D * T * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (out_rm) transpose(s, res, out_rm, D, T, T, D, 1, 0, 0);
  }
}

void hubert_forward(Hubert* H, hipStream_t s, const float* audio, long long L, int version, int n_layers, float* out_rm, float* out_cm,
                    const HubertTaps* taps) {
  RVC_REQUIRE(H->ready, "hubert_finalize has not been called");
  RVC_REQUIRE(version == 1 || version == 2, "version must be 1 or 2");
  RVC_REQUIRE(hubert_num_frames(L) >= 2, "audio too short");
  arena_passes(H->arena, [&] { hubert_graph(H, s, H->arena, audio, L, version, n_layers, out_rm, out_cm, taps); });
}

size_t hubert_workspace(const Hubert* M) { return M->arena.cap; }

}  // namespace rvc
