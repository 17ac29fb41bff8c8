// The trainer's discriminators (reference lib/infer_pack/models.py:1024-1145: MultiPeriodDiscriminator = DiscriminatorS + DiscriminatorP for periods
// 2, 3, 5, 7, 11, 17; MultiPeriodDiscriminatorV2 adds 23 and 37), forward only, and the segmented reductions of the three GAN losses
// (lib/train/losses.py:564-593).  Weight norm (dim 0) is folded at finalize; spectral norm is not supported (no shipped configuration uses it).
// All S = 2 B signals (y first, then y_hat) run through every layer in ONE launch per layer, in the reference's own layout [S][C][H][p]: the
// post-activation output of a layer is the feature map the caller asked for and the next layer's input, so the graph owns no activation memory.
//   DiscriminatorP(p): reflect pad to a multiple of p + view [H][p] + Conv2d(1, 32, (5, 1), stride 3) in disc_first_kernel; 32 -> 128 -> 512 -> 1024
//                      (stride 3) -> 1024 (stride 1) on the bf16x3 GEMM (conv_x3d.hip); Conv2d(1024, 1, (3, 1)) in disc_post_kernel.   6 launches
//   DiscriminatorS:    Conv1d(1, 16, 15) in disc_first_kernel (p = 1, nothing to pad); the four grouped k = 41 stride-4 layers (4 input channels per
//                      group) in disc_group_kernel; Conv1d(1024, 1024, 5) on the GEMM with p = 1; Conv1d(1024, 1, 3) in disc_post_kernel.        7 launches
// The forward is PLANNED (disc_plan: pure, no stream) and the plan is launched; disc_launch_count is the size of that plan.
// The input-gradient pass (disc_input_grad: the vector-Jacobian product from cotangents on the taps to the signals) walks the same layers backwards on
// the feature maps the forward wrote - one launch per layer again, planned the same way; see "input gradient" below.
// The weight-gradient pass (disc_weight_grad: dL / d(weight_g, weight_v, bias) from the same feature maps and the deltas the input-gradient pass left) is two
// launches per layer - gradient, finish -, opt-in through disc_keep_parameters; see "weight gradient" below.
// The optimizer step (AdamW on the kept parameters, then the folded weights and the images below re-derived on the device) is disc_optim.hip.
#include "disc_model.h"
#include "signal_dev.h"

namespace rvc {

constexpr float kDiscSlope = 0.1f;    // modules.LRELU_SLOPE

// ---------------------------------------------------------------------------------------------- kernels
// First layer from the raw signal: x[h][w] = sig[h p + w] for h p + w < T, the reflection sig[2 (T - 1) - (h p + w)] behind it (F.pad "reflect" on the
// right, models.py:1131-1135), zero rows outside [0, H);  y[s][c][h'][w] = lrelu(b[c] + sum_j W[c][j] x[stride h' + j - pad][w]).  One thread per (h', w).
struct DiscFirstArgs { const float* sig; const float* W; const float* bias; float* Y; int T, H, Hout, p, Co, stride, pad; float slope; };
template <int K>
__global__ __launch_bounds__(256) void disc_first_kernel(const DiscFirstArgs a) {
  __shared__ float ws[32 * K + 32];
  for (int i = threadIdx.x; i < a.Co * K; i += 256) ws[i] = a.W[i];
  for (int i = threadIdx.x; i < a.Co; i += 256) ws[32 * K + i] = a.bias[i];
  __syncthreads();
  const int N = a.Hout * a.p, n = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (n >= N) return;
  const int h = n / a.p, w = n - h * a.p;
  const float* sig = a.sig + (long long)s * a.T;
  float x[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int r = a.stride * h + j - a.pad;
    int t = r * a.p + w;
    if (t >= a.T) t = 2 * (a.T - 1) - t;
    x[j] = (r >= 0 && r < a.H) ? sig[t] : 0.f;
  }
  float* Y = a.Y + (long long)s * a.Co * N + n;
  for (int c = 0; c < a.Co; ++c) {
    float v = ws[32 * K + c];
#pragma unroll
    for (int j = 0; j < K; ++j) v = fmaf(ws[c * K + j], x[j], v);
    Y[(long long)c * N] = fmaxf(v, v * a.slope);
  }
}

// DiscriminatorS's grouped layers: Conv1d(Ci, Co, 41, stride 4, padding 20, groups = Ci / 4).  A workgroup = (64 outputs, one group, one signal): the
// group's 4 input rows (4 * 64 + 37 columns) and its weights in LDS; thread = (output t, quarter of the group's output channels), NPT channels each.
struct DiscGroupArgs { const float* X; const float* W; const float* bias; float* Y; int Ci, Co, opg, Tin, Tout; float slope; };
constexpr int kGrpK = 41, kGrpStride = 4, kGrpPad = 20, kGrpCin = 4, kGrpTT = 64, kGrpSpan = kGrpStride * (kGrpTT - 1) + kGrpK;
template <int NPT>
__global__ __launch_bounds__(256) void disc_group_kernel(const DiscGroupArgs a) {
  __shared__ float xs[kGrpCin][kGrpSpan];
  __shared__ float ws[4 * NPT * kGrpCin * kGrpK];
  const int t0 = blockIdx.x * kGrpTT, g = blockIdx.y, s = blockIdx.z;
  const float* X = a.X + ((long long)s * a.Ci + g * kGrpCin) * a.Tin;
  for (int i = threadIdx.x; i < kGrpCin * kGrpSpan; i += 256) {
    const int ci = i / kGrpSpan, o = i - ci * kGrpSpan;
    const int t = kGrpStride * t0 + o - kGrpPad;
    xs[ci][o] = (t >= 0 && t < a.Tin) ? X[(long long)ci * a.Tin + t] : 0.f;
  }
  const float* W = a.W + (long long)g * a.opg * (kGrpCin * kGrpK);
  for (int i = threadIdx.x; i < a.opg * kGrpCin * kGrpK; i += 256) ws[i] = W[i];
  __syncthreads();
  const int tl = threadIdx.x & 63, q = threadIdx.x >> 6, t = t0 + tl;
  float v[NPT];
#pragma unroll
  for (int i = 0; i < NPT; ++i) v[i] = a.bias[g * a.opg + q * NPT + i];
  for (int ci = 0; ci < kGrpCin; ++ci)
    for (int j = 0; j < kGrpK; ++j) {
      const float xv = xs[ci][kGrpStride * tl + j];
#pragma unroll
      for (int i = 0; i < NPT; ++i) v[i] = fmaf(ws[((q * NPT + i) * kGrpCin + ci) * kGrpK + j], xv, v[i]);
    }
  if (t < a.Tout) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) a.Y[((long long)s * a.Co + g * a.opg + q * NPT + i) * a.Tout + t] = fmaxf(v[i], v[i] * a.slope);
  }
}

// conv_post: Conv2d(Ci, 1, (3, 1), padding (1, 0)) / Conv1d(Ci, 1, 3, padding 1), no activation.  Thread = (one of 32 outputs, one eighth of the channels);
// the eight partial sums are added in index order.
struct DiscPostArgs { const float* X; const float* W; const float* bias; float* Y; int Ci, H, p; };
__global__ __launch_bounds__(256) void disc_post_kernel(const DiscPostArgs a) {
  __shared__ float red[8][32];
  const int N = a.H * a.p, nl = threadIdx.x & 31, cq = threadIdx.x >> 5, n = blockIdx.x * 32 + nl, s = blockIdx.y;
  float v = 0.f;
  if (n < N) {
    const int h = n / a.p;
    const bool up = h > 0, down = h + 1 < a.H;
    const int cn = a.Ci / 8;
    const float* X = a.X + ((long long)s * a.Ci + cq * cn) * N + n;
    const float* W = a.W + cq * cn * 3;
    for (int c = 0; c < cn; ++c, X += N, W += 3) {
      if (up) v = fmaf(W[0], X[-a.p], v);
      v = fmaf(W[1], X[0], v);
      if (down) v = fmaf(W[2], X[a.p], v);
    }
  }
  red[cq][nl] = v;
  __syncthreads();
  if (cq == 0 && n < N) {
    float t = a.bias[0];
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][nl];
    a.Y[(long long)s * N + n] = t;
  }
}

// ---------------------------------------------------------------------------------------------- model
Disc* disc_create(Ctx* ctx, int version) {
  RVC_REQUIRE(version == 1 || version == 2, "discriminator version must be 1 (MultiPeriodDiscriminator) or 2 (MultiPeriodDiscriminatorV2)");
  Disc* D = new Disc(); D->ctx = ctx; D->version = version;
  return D;
}
void disc_destroy(Disc* D) { delete D; }
void disc_set_tensor(Disc* D, const char* name, const float* d, const long long* shape, int ndim) { D->ts.set(name, d, shape, ndim); }

static std::vector<int> disc_periods(int version) {
  std::vector<int> p = {0, 2, 3, 5, 7, 11, 17};
  if (version == 2) { p.push_back(23); p.push_back(37); }
  return p;
}

// The transposed, phase-grouped images of a dense layer's data gradient (conv_x3d_bwd.hip).  Input row h = stride h' + j - pad: stride 1 is one product,
// tap t (row h + t - pad of the gradient) carrying W[.][.][k - 1 - t]; stride 3 (k 5, pad 2) is one product per phase r = h mod 3, tap 0 (row j) carrying
// W[.][.][r + 2] and - r > 0 - tap 1 (row j + 1) carrying W[.][.][r - 1].
// Returns the number of phases (= stride) and fills img[r] and nt[r], the taps of phase r; rows Ci padded to a multiple of 128.
int disc_bwd_weight_images(const float* w, int Co, int Ci, int k, int stride, int pad, std::vector<uint16_t> (&img)[3], int (&nt)[3]) {
  RVC_REQUIRE(k == 5 && pad == 2 && (stride == 1 || stride == 3), "dense discriminator layer: k 5, pad 2, stride 1 or 3");
  RVC_REQUIRE(Ci >= 1 && Co >= 16 && Co % 16 == 0, "dense discriminator layer: output channels a multiple of 16");
  const int CiPx = (Ci + 127) & ~127;
  for (int r = 0; r < stride; ++r) {
    std::vector<int> taps;
    if (stride == 1) taps = {4, 3, 2, 1, 0};
    else if (r == 0) taps = {2};
    else taps = {r + 2, r - 1};
    nt[r] = (int)taps.size();
    std::vector<float> wt((size_t)Ci * Co * nt[r]);
    for (int co = 0; co < Co; ++co)
      for (int ci = 0; ci < Ci; ++ci)
        for (int t = 0; t < nt[r]; ++t) wt[((size_t)ci * Co + co) * nt[r] + t] = w[((size_t)co * Ci + ci) * k + taps[t]];
    x3_weight_image(wt.data(), Ci, Co, nt[r], CiPx, img[r]);
  }
  return stride;
}
// the geometry of that launch for a layer (Ci -> Co, k 5, pad 2, stride 1 or 3) whose input has H rows and whose output gradient has Hd: everything of the
// arguments but the pointers
void disc_bwd_geometry(ConvX3dBwdArgs& a, int Ci, int Co, int k, int stride, int pad, int H, int Hd, int p, int S, float slope) {
  a.R = Ci; a.RPx = (Ci + 127) & ~127; a.Ck = Co; a.Hd = Hd; a.H = H; a.p = p; a.ostride = stride; a.off0 = stride == 1 ? -pad : 0; a.nph = stride;
  for (int r = 0; r < stride && r < 3; ++r) a.nt[r] = stride == 1 ? k : (r == 0 ? 1 : 2);
  a.S = S; a.slope = slope;
}
static void disc_bwd_images(DiscLayer& L, const std::vector<float>& w) {
  std::vector<uint16_t> img[3]; int nt[3];
  const int nph = disc_bwd_weight_images(w.data(), L.Co, L.Ci, L.k, L.stride, L.pad, img, nt);
  L.CiPx = (L.Ci + 127) & ~127;
  for (int r = 0; r < nph; ++r) L.wxb[r].upload(img[r]);
}

void disc_keep_parameters(Disc* D, bool on) {
  RVC_REQUIRE(!D->ready, "disc_keep_parameters: set the switch before finalize");
  D->keep = on;
}
void disc_finalize(Disc* D) {
  D->ready = false; static_cast<DiscWeights&>(*D) = {};   // a finalize that throws leaves the handle not ready
  D->params.clear(); D->kept = false; D->optim.reset();
  const TensorStore& ts = D->ts;
  const std::vector<int> periods = disc_periods(D->version);
  struct Spec { int Ci, Co, k, stride, pad, groups; };
  static const Spec kS[7] = {{1, 16, 15, 1, 7, 1}, {16, 64, 41, 4, 20, 4}, {64, 256, 41, 4, 20, 16}, {256, 1024, 41, 4, 20, 64},
                             {1024, 1024, 41, 4, 20, 256}, {1024, 1024, 5, 1, 2, 1}, {1024, 1, 3, 1, 1, 1}};
  static const Spec kP[6] = {{1, 32, 5, 3, 2, 1}, {32, 128, 5, 3, 2, 1}, {128, 512, 5, 3, 2, 1}, {512, 1024, 5, 3, 2, 1}, {1024, 1024, 5, 1, 2, 1},
                             {1024, 1, 3, 1, 1, 1}};
  for (size_t i = 0; i < periods.size(); ++i) {
    DiscNet net; net.period = periods[i];
    const Spec* sp = net.period ? kP : kS; const int nl = net.period ? 6 : 7;
    for (int l = 0; l < nl; ++l) {
      const std::string n = "discriminators." + std::to_string(i) + (l + 1 < nl ? ".convs." + std::to_string(l) : std::string(".conv_post"));
      const Spec& c = sp[l];
      const long long numel = (long long)c.Co * (c.Ci / c.groups) * c.k;
      std::vector<float> w;
      RVC_REQUIRE(!ts.has(n + ".weight_u") && !ts.has(n + ".weight_orig"), n + ": spectral norm is not supported");
      if (ts.has(n + ".weight_v")) {
        const HostTensor& v = ts.get(n + ".weight_v"); const HostTensor& g = ts.get(n + ".weight_g");
        RVC_REQUIRE((long long)v.numel() == numel && v.shape[0] == c.Co && (long long)g.numel() == c.Co, "shape of " + n + ".weight_v / weight_g");
        w = weight_norm0(v, g);
      } else {
        const HostTensor& t = ts.get(n + ".weight");
        RVC_REQUIRE((long long)t.numel() == numel && t.shape[0] == c.Co, "shape of " + n + ".weight");
        w = t.data;
      }
      const HostTensor& b = ts.get(n + ".bias", {c.Co});
      DiscLayer L; L.Ci = c.Ci; L.Co = c.Co; L.k = c.k; L.stride = c.stride; L.pad = c.pad; L.groups = c.groups;
      L.b.upload(b.data);
      if (ts.has(n + ".weight_v")) {
        const HostTensor& v = ts.get(n + ".weight_v"); const HostTensor& g = ts.get(n + ".weight_g");
        L.gi_b = (int)D->params.size(); D->params.push_back({n + ".bias", b.shape});
        L.gi_g = (int)D->params.size(); D->params.push_back({n + ".weight_g", g.shape});
        L.gi_w = (int)D->params.size(); D->params.push_back({n + ".weight_v", v.shape});
        if (D->keep) { L.pv.upload(v.data); L.pg.upload(g.data); }
      } else {
        L.gi_w = (int)D->params.size(); D->params.push_back({n + ".weight", ts.get(n + ".weight").shape});
        L.gi_b = (int)D->params.size(); D->params.push_back({n + ".bias", b.shape});
        if (D->keep && c.groups == 1 && c.Ci % 16 == 0 && c.Co > 1) L.pv.upload(w);   // a GEMM layer keeps only images: the optimizer's fp32 master copy
      }
      if (disc_layer_is_gemm(L)) {
        L.CoPx = (c.Co + 127) & ~127;
        std::vector<uint16_t> img;
        x3_weight_image(w.data(), c.Co, c.Ci, c.k, L.CoPx, img);
        L.wx.upload(img);
        disc_bwd_images(L, w);
      } else {
        L.w.upload(w);
      }
      net.L.push_back(std::move(L));
    }
    D->nets.push_back(std::move(net));
  }
  D->ts.clear();
  D->kept = D->keep;
  D->ready = true;
}
int disc_param_count(const Disc* D) { RVC_REQUIRE(D->ready, "finalize first"); return (int)D->params.size(); }
void disc_param_info(const Disc* D, int k, std::string& name, std::vector<long long>& shape) {
  RVC_REQUIRE(D->ready, "finalize first");
  RVC_REQUIRE(k >= 0 && k < (int)D->params.size(), "no such parameter");
  name = D->params[k].name; shape = D->params[k].shape;
}

int disc_count(const Disc* D) { return (int)disc_periods(D->version).size(); }
int disc_num_taps(const Disc* D, int i) {
  RVC_REQUIRE(i >= 0 && i < disc_count(D), "no such sub-discriminator");
  return i == 0 ? 7 : 6;
}
// the pad a period needs must be shorter than the signal (torch's reflect pad refuses the rest)
static void disc_check_T(const Disc* D, long long T) {
  RVC_REQUIRE(T >= 1 && T <= (1LL << 24), "signal length out of range");
  for (int p : disc_periods(D->version))
    if (p) { const long long pad = (p - T % p) % p; RVC_REQUIRE(pad < T, "signal of " + std::to_string(T) + " samples is too short for the reflect pad of period " + std::to_string(p)); }
}
static int conv_out(int H, int k, int stride, int pad) { return (H + 2 * pad - k) / stride + 1; }
void disc_tap_shape(const Disc* D, int i, int tap, long long T, int* C, int* H, int* p) {
  RVC_REQUIRE(D->ready, "finalize first");
  RVC_REQUIRE(tap >= 0 && tap < disc_num_taps(D, i), "no such tap");
  disc_check_T(D, T);
  const DiscNet& net = D->nets[i];
  const int per = net.period ? net.period : 1;
  int h = (int)((T + per - 1) / per);
  for (int l = 0; l <= tap; ++l) h = conv_out(h, net.L[l].k, net.L[l].stride, net.L[l].pad);
  RVC_REQUIRE(h >= 1, "signal too short");
  *C = net.L[tap].Co; *H = h; *p = per;
}

// ---------------------------------------------------------------------------------------------- plan, then launch
struct DiscLaunch {
  int kind = 0;                       // 0: first layer, 1: grouped, 2: GEMM, 3: conv_post
  dim3 grid;
  int K = 0;                          // kind 0: taps; kind 1: channels per thread
  DiscFirstArgs f; DiscGroupArgs g; ConvX3dPlan x; DiscPostArgs q;
};
// pure: no stream, no launch, no allocation.  fmaps (may be null: counting only): one pointer per tap, discriminator-major.
static void disc_plan(const Disc* D, const float* signals, int S, long long T, float* const* fmaps, std::vector<DiscLaunch>& plan) {
  RVC_REQUIRE(D->ready, "finalize first");
  RVC_REQUIRE(S >= 1 && S <= 65535, "1 <= S <= 65535 signals");
  disc_check_T(D, T);
  plan.clear();
  int tap0 = 0;
  for (size_t i = 0; i < D->nets.size(); ++i) {
    const DiscNet& net = D->nets[i];
    const int per = net.period ? net.period : 1;
    int H = (int)((T + per - 1) / per);
    const float* x = signals;
    for (size_t l = 0; l < net.L.size(); ++l) {
      const DiscLayer& L = net.L[l];
      const int Ho = conv_out(H, L.k, L.stride, L.pad);
      RVC_REQUIRE(Ho >= 1, "signal too short");
      float* y = fmaps ? fmaps[tap0 + l] : nullptr;
      RVC_REQUIRE(!fmaps || y, "null feature-map pointer");
      const long long N = (long long)Ho * per;
      DiscLaunch d;
      if (l == 0) {
        d.kind = 0; d.K = L.k;
        d.f = DiscFirstArgs{x, L.w.p, L.b.p, y, (int)T, H, Ho, per, L.Co, L.stride, L.pad, kDiscSlope};
        d.grid = dim3((unsigned)((N + 255) / 256), (unsigned)S);
      } else if (l + 1 == net.L.size()) {
        d.kind = 3;
        d.q = DiscPostArgs{x, L.w.p, L.b.p, y, L.Ci, H, per};
        d.grid = dim3((unsigned)((N + 31) / 32), (unsigned)S);
      } else if (disc_layer_is_gemm(L)) {
        d.kind = 2;
        const ConvX3dArgs a{x, reinterpret_cast<const unsigned char*>(L.wx.p), L.b.p, y, L.Ci, L.Co, L.CoPx, H, Ho, per, L.k, L.stride, L.pad, S, kDiscSlope};
        RVC_REQUIRE(conv_x3d_plan(a, d.x), "discriminator layer does not fit the GEMM kernel");
      } else {
        RVC_REQUIRE(L.k == kGrpK && L.stride == kGrpStride && L.pad == kGrpPad && L.Ci / L.groups == kGrpCin && per == 1, "grouped layer geometry");
        d.kind = 1; d.K = L.Co / L.groups / 4;
        RVC_REQUIRE(d.K == 1 || d.K == 4, "grouped layer: 4 or 16 output channels per group");
        d.g = DiscGroupArgs{x, L.w.p, L.b.p, y, L.Ci, L.Co, L.Co / L.groups, H, Ho, kDiscSlope};
        d.grid = dim3((unsigned)((Ho + kGrpTT - 1) / kGrpTT), (unsigned)L.groups, (unsigned)S);
      }
      plan.push_back(d);
      x = y; H = Ho;
    }
    tap0 += (int)net.L.size();
  }
}
int disc_launch_count(const Disc* D, int S, long long T) {
  std::vector<DiscLaunch> plan;
  disc_plan(D, nullptr, S, T, nullptr, plan);
  return (int)plan.size();
}
void disc_forward(Disc* D, hipStream_t s, const float* signals, int S, long long T, float* const* scores, float* const* fmaps) {
  RVC_REQUIRE(signals && fmaps, "null argument");
  std::vector<DiscLaunch> plan;
  disc_plan(D, signals, S, T, fmaps, plan);
  for (const DiscLaunch& d : plan) {
    switch (d.kind) {
      case 0:
        if (d.K == 5) hipLaunchKernelGGL(disc_first_kernel<5>, d.grid, dim3(256), 0, s, d.f);
        else if (d.K == 15) hipLaunchKernelGGL(disc_first_kernel<15>, d.grid, dim3(256), 0, s, d.f);
        else throw Error("first layer: 5 or 15 taps");
        break;
      case 1:
        if (d.K == 4) hipLaunchKernelGGL(disc_group_kernel<4>, d.grid, dim3(256), 0, s, d.g);
        else hipLaunchKernelGGL(disc_group_kernel<1>, d.grid, dim3(256), 0, s, d.g);
        break;
      case 2: conv_x3d_launch(d.x, s); break;
      default: hipLaunchKernelGGL(disc_post_kernel, d.grid, dim3(256), 0, s, d.q); break;
    }
  }
  if (scores) {      // a score is the flattened last tap (models.py:1105-1107,:1141-1143): a copy for callers that want it apart
    int tap0 = 0;
    for (size_t i = 0; i < D->nets.size(); ++i) {
      tap0 += (int)D->nets[i].L.size();
      if (!scores[i] || scores[i] == fmaps[tap0 - 1]) continue;
      int C, H, p; disc_tap_shape(D, (int)i, (int)D->nets[i].L.size() - 1, T, &C, &H, &p);
      RVC_HIP_CHECK(hipMemcpyAsync(scores[i], fmaps[tap0 - 1], (size_t)S * H * p * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  }
}

// ---------------------------------------------------------------------------------------------- losses
// K segments in one launch pair: kSegParts workgroups per segment each sum a contiguous chunk in float64 (thread-strided, then block_sum), then one
// workgroup per segment adds its partials in index order.  No atomics: two calls give the same bits.
constexpr int kSegMax = 64, kSegParts = 32;
struct SqSegs { const float* x[kSegMax]; long long n[kSegMax]; float c[kSegMax]; };
struct L1Segs { const float* a[kSegMax]; const float* b[kSegMax]; long long n[kSegMax]; };
__device__ __forceinline__ double seg_term(const SqSegs& g, int k, long long j) { const float d = g.c[k] - g.x[k][j]; return (double)d * (double)d; }
__device__ __forceinline__ double seg_term(const L1Segs& g, int k, long long j) { return (double)fabsf(g.a[k][j] - g.b[k][j]); }
template <class Segs>
__global__ __launch_bounds__(256) void seg_partial_kernel(const Segs g, double* part) {
  __shared__ double red[4];
  const int k = blockIdx.y;
  const long long n = g.n[k], chunk = (n + kSegParts - 1) / kSegParts;
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  double acc = 0.0;
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) acc += seg_term(g, k, j);
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) part[k * kSegParts + blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void seg_final_kernel(const double* __restrict__ part, double* out) {
  __shared__ double red[4];
  const double t = block_sum(threadIdx.x < kSegParts ? part[blockIdx.x * kSegParts + threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}
template <class Segs>
static void seg_sums(hipStream_t s, const Segs& g, int K, double* out) {
  double* part = (double*)stream_scratch(s, 21, (size_t)kSegMax * kSegParts * sizeof(double));
  hipLaunchKernelGGL(seg_partial_kernel<Segs>, dim3(kSegParts, K), dim3(256), 0, s, g, part);
  hipLaunchKernelGGL(seg_final_kernel, dim3(K), dim3(256), 0, s, part, out);
}
void sqerr_sums(hipStream_t s, const float* const* x, const long long* n, const float* c, int K, double* out) {
  RVC_REQUIRE(x && n && c && out && K >= 1 && K <= kSegMax, "sqerr_sums: 1 <= K <= 64 segments");
  SqSegs g{};
  for (int k = 0; k < K; ++k) { RVC_REQUIRE(x[k] && n[k] > 0, "sqerr_sums: empty segment"); g.x[k] = x[k]; g.n[k] = n[k]; g.c[k] = c[k]; }
  seg_sums(s, g, K, out);
}
void l1_sums(hipStream_t s, const float* const* a, const float* const* b, const long long* n, int K, double* out) {
  RVC_REQUIRE(a && b && n && out && K >= 1 && K <= kSegMax, "l1_sums: 1 <= K <= 64 segments");
  L1Segs g{};
  for (int k = 0; k < K; ++k) { RVC_REQUIRE(a[k] && b[k] && n[k] > 0, "l1_sums: empty segment"); g.a[k] = a[k]; g.b[k] = b[k]; g.n[k] = n[k]; }
  seg_sums(s, g, K, out);
}

// ---------------------------------------------------------------------------------------------- input gradient
// tap[l] = a_{l+1} = lrelu(z_l), the last tap the score z_last.  With cotangents c_l on the taps (null: zero) and delta_l = dL / dz_l:
//   delta_last = c_last;   delta_l = (convT_{l+1}(delta_{l+1}) + c_l) * (tap[l] > 0 ? 1 : slope);   dA_0 = convT_0(delta_0), folded back onto the signal.
// The mask comes from the saved post-activation (a > 0 <=> z > 0; torch's leaky_relu backward takes the slope at exactly 0), so given the forward's own
// feature maps the pass is linear: the exact VJP of what the forward computed.  Every kernel is a gather (no atomics): two calls give the same bits.

// conv_post transposed, fused with the mask of the layer below: Y[s][c][h][w] = (sum_j W[c][j] ds[s][h + 1 - j][w] + Cot) * mask(A).  One thread per element.
struct DiscPostBwdArgs { const float* dS; const float* W; const float* Cot; const float* A; float* Y; int Ci, H, p; float slope; };
__global__ __launch_bounds__(256) void disc_post_bwd_kernel(const DiscPostBwdArgs a) {
  const long long N = (long long)a.H * a.p, i = (long long)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (i >= a.Ci * N) return;
  const int c = (int)(i / N), n = (int)(i - c * N), h = n / a.p;
  float v = 0.f;
  if (a.dS) {
    const float* dS = a.dS + s * N + n;
    const float* W = a.W + c * 3;
    if (h + 1 < a.H) v = fmaf(W[0], dS[a.p], v);
    v = fmaf(W[1], dS[0], v);
    if (h > 0) v = fmaf(W[2], dS[-a.p], v);
  }
  const long long idx = s * a.Ci * N + i;
  if (a.Cot) v += a.Cot[idx];
  a.Y[idx] = a.A[idx] > 0.f ? v : v * a.slope;
}

// DiscriminatorS's grouped layers transposed: input sample u of channel g 4 + ci gathers, from the opg output channels of its group, the taps
// j = (u & 3) + 4 m <= 40 at output t = (u >> 2) + 5 - m (4 t + j - 20 = u): 10 or 11 taps.  One thread per input element.
struct DiscGroupBwdArgs { const float* D; const float* W; const float* Cot; const float* A; float* Y; int Ci, Co, opg, Tin, Tout; float slope; };
__global__ __launch_bounds__(256) void disc_group_bwd_kernel(const DiscGroupBwdArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (i >= (long long)a.Ci * a.Tin) return;
  const int cin = (int)(i / a.Tin), u = (int)(i - (long long)cin * a.Tin), g = cin / kGrpCin, ci = cin - g * kGrpCin;
  const float* D = a.D + (s * a.Co + (long long)g * a.opg) * a.Tout;
  const float* W = a.W + ((long long)g * a.opg * kGrpCin + ci) * kGrpK;
  float v = 0.f;
  for (int m = 0; (u & 3) + 4 * m < kGrpK; ++m) {
    const int j = (u & 3) + 4 * m, t = (u >> 2) + kGrpPad / kGrpStride - m;
    if (t < 0 || t >= a.Tout) continue;
    for (int o = 0; o < a.opg; ++o) v = fmaf(W[(long long)o * kGrpCin * kGrpK + j], D[(long long)o * a.Tout + t], v);
  }
  const long long idx = s * a.Ci * a.Tin + i;
  if (a.Cot) v += a.Cot[idx];
  a.Y[idx] = a.A[idx] > 0.f ? v : v * a.slope;
}

// First layer transposed, fused with the un-fold and the reflect fold-back.  One thread per signal sample t: it gathers dA_0 at its own position t and, where
// 2 (T - 1) - t lies in the reflect pad [T, H p), at that mirror position too (disc_first_kernel reads sig[2 (T - 1) - q] for q >= T).  dA_0[h][w] =
// sum_c sum_j W[c][j] D[c][h'][w] over stride h' + j - pad = h.  add: the sub-discriminators add into dsig one after the other on the stream, in index order.
struct DiscFirstBwdArgs { const float* D; const float* W; float* dsig; int T, H, Hout, p, Co, stride, pad, add; };
template <int K>
__global__ __launch_bounds__(256) void disc_first_bwd_kernel(const DiscFirstBwdArgs a) {
  __shared__ float ws[32 * K];
  for (int i = threadIdx.x; i < a.Co * K; i += 256) ws[i] = a.W[i];
  __syncthreads();
  const int t = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (t >= a.T) return;
  const long long N = (long long)a.Hout * a.p;
  const float* D = a.D + (long long)s * a.Co * N;
  float v = 0.f;
  for (int side = 0; side < 2; ++side) {
    const long long q = side ? 2LL * (a.T - 1) - t : t;
    if (side && (q < a.T || q >= (long long)a.H * a.p)) break;
    const int h = (int)(q / a.p), w = (int)(q - (long long)h * a.p);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int hh = h + a.pad - j;
      if (hh < 0 || hh % a.stride != 0 || hh / a.stride >= a.Hout) continue;
      const float* d = D + (long long)(hh / a.stride) * a.p + w;
      for (int c = 0; c < a.Co; ++c) v = fmaf(ws[c * K + j], d[(long long)c * N], v);
    }
  }
  float* o = a.dsig + (long long)s * a.T + t;
  *o = a.add ? *o + v : v;
}

struct DiscBwdLaunch {
  int kind = 0;                       // 0: first layer, 1: grouped, 2: GEMM, 3: conv_post
  dim3 grid;
  int K = 0;                          // kind 0: taps
  DiscFirstBwdArgs f; DiscGroupBwdArgs g; ConvX3dBwdPlan x; DiscPostBwdArgs q;
};
// pure: no stream, no launch, no allocation.  fmaps / dtaps / work (all may be null: counting only): one pointer per tap, discriminator-major; launch `l` of
// a sub-discriminator is layer l transposed: it reads delta_l (work[l]; the given cotangent of the score for the last layer) and writes delta_{l-1} (work[l-1]).
static void disc_bwd_plan(const Disc* D, int S, long long T, const float* const* fmaps, const float* const* dtaps, float* const* work, float* dsignals,
                          std::vector<DiscBwdLaunch>& plan) {
  RVC_REQUIRE(D->ready, "finalize first");
  RVC_REQUIRE(S >= 1 && S <= 65535, "1 <= S <= 65535 signals");
  disc_check_T(D, T);
  plan.clear();
  const bool real = fmaps != nullptr;
  int tap0 = 0;
  for (size_t i = 0; i < D->nets.size(); ++i) {
    const DiscNet& net = D->nets[i];
    const int per = net.period ? net.period : 1, nl = (int)net.L.size();
    std::vector<int> Hs(nl + 1);
    Hs[0] = (int)((T + per - 1) / per);
    for (int l = 0; l < nl; ++l) { Hs[l + 1] = conv_out(Hs[l], net.L[l].k, net.L[l].stride, net.L[l].pad); RVC_REQUIRE(Hs[l + 1] >= 1, "signal too short"); }
    if (real) for (int l = 0; l < nl; ++l) RVC_REQUIRE(fmaps[tap0 + l] && work[tap0 + l], "null feature-map or work pointer");
    for (int l = nl - 1; l >= 0; --l) {
      const DiscLayer& L = net.L[l];
      const int H = Hs[l], Ho = Hs[l + 1];
      const float* delta = real ? (l + 1 == nl ? dtaps[tap0 + l] : work[tap0 + l]) : nullptr;     // conv_post reads the score's cotangent where it was given
      const float* cot = real && l > 0 ? dtaps[tap0 + l - 1] : nullptr;
      const float* act = real && l > 0 ? fmaps[tap0 + l - 1] : nullptr;
      float* y = real && l > 0 ? work[tap0 + l - 1] : nullptr;
      DiscBwdLaunch d;
      if (l == 0) {
        d.kind = 0; d.K = L.k;
        d.f = DiscFirstBwdArgs{delta, L.w.p, dsignals, (int)T, H, Ho, per, L.Co, L.stride, L.pad, i > 0 ? 1 : 0};
        d.grid = dim3((unsigned)((T + 255) / 256), (unsigned)S);
      } else if (l + 1 == nl) {
        d.kind = 3;
        d.q = DiscPostBwdArgs{delta, L.w.p, cot, act, y, L.Ci, H, per, kDiscSlope};
        d.grid = dim3((unsigned)(((long long)L.Ci * H * per + 255) / 256), (unsigned)S);
      } else if (disc_layer_is_gemm(L)) {
        d.kind = 2;
        ConvX3dBwdArgs a{};
        a.D = delta; a.Cot = cot; a.A = act; a.Y = y;
        for (int r = 0; r < L.stride; ++r) a.Wx[r] = reinterpret_cast<const unsigned char*>(L.wxb[r].p);
        disc_bwd_geometry(a, L.Ci, L.Co, L.k, L.stride, L.pad, H, Ho, per, S, kDiscSlope);
        RVC_REQUIRE(conv_x3d_bwd_plan(a, d.x), "discriminator layer does not fit the data-gradient kernel");
      } else {
        RVC_REQUIRE(L.k == kGrpK && L.stride == kGrpStride && L.pad == kGrpPad && L.Ci / L.groups == kGrpCin && per == 1, "grouped layer geometry");
        d.kind = 1;
        d.g = DiscGroupBwdArgs{delta, L.w.p, cot, act, y, L.Ci, L.Co, L.Co / L.groups, H, Ho, kDiscSlope};
        d.grid = dim3((unsigned)(((long long)L.Ci * H + 255) / 256), (unsigned)S);
      }
      plan.push_back(d);
    }
    tap0 += nl;
  }
}
int disc_input_grad_launch_count(const Disc* D, int S, long long T) {
  std::vector<DiscBwdLaunch> plan;
  disc_bwd_plan(D, S, T, nullptr, nullptr, nullptr, nullptr, plan);
  return (int)plan.size();
}
void disc_input_grad(Disc* D, hipStream_t s, int S, long long T, const float* const* fmaps, const float* const* dtaps, float* const* work, float* dsignals) {
  RVC_REQUIRE(fmaps && dtaps && work && dsignals, "null argument");
  std::vector<DiscBwdLaunch> plan;
  disc_bwd_plan(D, S, T, fmaps, dtaps, work, dsignals, plan);
  int tap0 = 0;                       // delta of the last tap is its cotangent: work receives a copy (zeros where none was given)
  for (size_t i = 0; i < D->nets.size(); ++i) {
    const int last = tap0 + (int)D->nets[i].L.size() - 1;
    int C, H, p; disc_tap_shape(D, (int)i, (int)D->nets[i].L.size() - 1, T, &C, &H, &p);
    const size_t bytes = (size_t)S * C * H * p * sizeof(float);
    if (!dtaps[last]) RVC_HIP_CHECK(hipMemsetAsync(work[last], 0, bytes, s));
    else if (dtaps[last] != work[last]) RVC_HIP_CHECK(hipMemcpyAsync(work[last], dtaps[last], bytes, hipMemcpyDeviceToDevice, s));
    tap0 = last + 1;
  }
  for (const DiscBwdLaunch& d : plan) {
    switch (d.kind) {
      case 0:
        if (d.K == 5) hipLaunchKernelGGL(disc_first_bwd_kernel<5>, d.grid, dim3(256), 0, s, d.f);
        else if (d.K == 15) hipLaunchKernelGGL(disc_first_bwd_kernel<15>, d.grid, dim3(256), 0, s, d.f);
        else throw Error("first layer: 5 or 15 taps");
        break;
      case 1: hipLaunchKernelGGL(disc_group_bwd_kernel, d.grid, dim3(256), 0, s, d.g); break;
      case 2: conv_x3d_bwd_launch(d.x, s); break;
      default: hipLaunchKernelGGL(disc_post_bwd_kernel, d.grid, dim3(256), 0, s, d.q); break;
    }
  }
}

// The element-wise ends of the pass.  Cotangents of the trainer's losses, K tensors in one launch:
//   kind 0: out = scale a              (d mean(s^2) / ds = 2 s / N: discriminator_loss on generated scores)
//   kind 1: out = -scale (1 - a)       (d mean((1 - s)^2) / ds: generator_loss; discriminator_loss on real scores)
//   kind 2: out = scale sign(a - b)    (d mean |r - g| / dg with a = g, b = r: feature_loss; sign(0) = 0)
struct CotSegs { const float* a[kSegMax]; const float* b[kSegMax]; float* out[kSegMax]; long long n[kSegMax]; float scale[kSegMax]; };
__global__ __launch_bounds__(256) void cotangent_kernel(const CotSegs g, int kind) {
  const int k = blockIdx.y;
  const long long n = g.n[k];
  const float sc = g.scale[k];
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
    const float a = g.a[k][j];
    float v;
    if (kind == 0) v = sc * a;
    else if (kind == 1) v = -sc * (1.f - a);
    else { const float d = a - g.b[k][j]; v = d > 0.f ? sc : (d < 0.f ? -sc : 0.f); }
    g.out[k][j] = v;
  }
}
void loss_cotangents(hipStream_t s, int kind, const float* const* a, const float* const* b, const long long* n, const float* scale, int K, float* const* out) {
  RVC_REQUIRE(a && n && scale && out && K >= 1 && K <= kSegMax && kind >= 0 && kind <= 2 && (kind != 2 || b), "loss_cotangents: 1 <= K <= 64 tensors, kind 0, 1 or 2");
  CotSegs g{};
  long long longest = 0;
  for (int k = 0; k < K; ++k) {
    RVC_REQUIRE(a[k] && out[k] && n[k] > 0 && (kind != 2 || b[k]), "loss_cotangents: empty tensor");
    g.a[k] = a[k]; g.b[k] = kind == 2 ? b[k] : nullptr; g.out[k] = out[k]; g.n[k] = n[k]; g.scale[k] = scale[k];
    longest = std::max(longest, n[k]);
  }
  const unsigned blocks = (unsigned)std::min<long long>((longest + 255) / 256, 1024);
  hipLaunchKernelGGL(cotangent_kernel, dim3(blocks, K), dim3(256), 0, s, g, kind);
}
// gradient_norm_loss's interpolation, out[b][t] = alpha[b] y[b][t] + (1 - alpha[b]) y_hat[b][t], with the reference's roundings: 1 - alpha, the two products
// and the sum are each rounded to float32 (no contraction into an fma)
__global__ __launch_bounds__(256) void interpolate_kernel(const float* __restrict__ alpha, const float* __restrict__ y, const float* __restrict__ y_hat, long long T,
                                                          float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const float al = alpha[b];
  out[b * T + t] = __fadd_rn(__fmul_rn(al, y[b * T + t]), __fmul_rn(__fsub_rn(1.f, al), y_hat[b * T + t]));
}
void interpolate_rows(hipStream_t s, const float* alpha, const float* y, const float* y_hat, int B, long long T, float* out) {
  RVC_REQUIRE(alpha && y && y_hat && out && B >= 1 && B <= 65535 && T >= 1, "interpolate_rows: bad argument");
  hipLaunchKernelGGL(interpolate_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, s, alpha, y, y_hat, T, out);
}

// ---------------------------------------------------------------------------------------------- weight gradient
// With delta_l = dL / dz_l (work[l] of the input-gradient pass) and X_l the layer's input (the signal through the reflect rule for l = 0, tap[l - 1] otherwise):
//   dW_l[m][c][j] = sum_s sum_n delta_l[s][m][n] X_l[s][c][stride h' + j - pad][w]  (n = h' p + w; rows outside [0, H) are zero),   db_l[m] = sum_s sum_n delta_l[s][m][n]
// and through weight norm (dim 0), with n_m = |v_m| and d_m = <dW[m], v[m]>:  grad_g[m] = d_m / n_m,  grad_v[m] = (g_m / n_m) (dW[m] - (d_m / n_m^2) v[m]).
// Two launches per layer whatever S and T: the gradient kernel writes `splits` partial images (each split owns a contiguous piece of the reduction), the
// finishing kernel adds them in index order, forms db in float64 and applies the chain in one pass over a row.  No atomics: two calls give the same bits.
// The dense k = 5 layers run on the matrix cores (conv_x3d_wgrad.hip); the first layer, the grouped layers and conv_post are direct gathers.

// One thread per weight element (m, ci, j) and split: the sum over every signal and the split's run of n, in float64.  T > 0: X is the signal [S][T] seen
// through disc_first_kernel's reflect rule; T = 0: X is a tap [S][Ci][H][p] and channel ci of group m / opg is row (m / opg) cig + ci.
struct DiscWgradDirectArgs { const float* D; const float* X; float* part; int S, Ci, Co, cig, opg, k, stride, pad, H, Hout, p, T, chunk; };
__global__ __launch_bounds__(256) void disc_wgrad_direct_kernel(const DiscWgradDirectArgs a) {
  const int L = a.cig * a.k, total = a.Co * L, o = blockIdx.x * 256 + threadIdx.x, split = blockIdx.y;
  if (o >= total) return;
  const int m = o / L, r = o - m * L, ci = r / a.k, j = r - ci * a.k, c = (m / a.opg) * a.cig + ci;
  const int N = a.Hout * a.p, n0 = split * a.chunk, n1 = min(n0 + a.chunk, N);
  const long long HP = (long long)a.H * a.p;
  double acc = 0.0;
  for (int s = 0; s < a.S; ++s) {
    const float* D = a.D + ((long long)s * a.Co + m) * N;
    const float* X = a.T ? a.X + (long long)s * a.T : a.X + ((long long)s * a.Ci + c) * HP;
    int h = n0 / a.p, w = n0 - h * a.p;
    for (int n = n0; n < n1; ++n) {
      const int row = a.stride * h + j - a.pad;
      if (row >= 0 && row < a.H) {
        long long t = (long long)row * a.p + w;
        if (a.T && t >= a.T) t = 2LL * (a.T - 1) - t;
        acc = fma((double)D[n], (double)X[t], acc);
      }
      if (++w == a.p) { w = 0; ++h; }
    }
  }
  a.part[(long long)split * total + o] = (float)acc;
}

// One workgroup per output channel m: db[m] (float64, thread-strided then block_sum: a fixed order), dW[m] = the partials added in index order, and the
// weight-norm chain where v is given (gw receives dW itself otherwise).  gw doubles as the row's store between the two passes: a thread re-reads only what
// it wrote itself.
__global__ __launch_bounds__(256) void disc_wgrad_finish_kernel(const DiscWgradFinishArgs a) {
  __shared__ double red[4];
  const int m = blockIdx.x;
  double bs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < a.S; ++s) {
    const float* D = a.D + ((long long)s * a.Co + m) * a.N;
    for (int n = threadIdx.x; n < a.N; n += 1024) {
#pragma unroll
      for (int u = 0; u < 4; ++u) bs[u] += n + 256 * u < a.N ? (double)D[n + 256 * u] : 0.0;
    }
  }
  const double b = block_sum((bs[0] + bs[1]) + (bs[2] + bs[3]), red);
  if (threadIdx.x == 0) a.gb[m] = (float)b;
  const float* P = a.part + (long long)m * a.L;
  const float* v = a.v ? a.v + (long long)m * a.L : nullptr;
  float* gw = a.gw + (long long)m * a.L;
  double d = 0.0, vv = 0.0;
  for (int q = threadIdx.x; q < a.L; q += 256) {
    double w = 0.0;
    for (int z = 0; z < a.splits; ++z) w += (double)P[(long long)z * a.pstride + q];
    gw[q] = (float)w;
    if (v) { const double x = (double)v[q]; d = fma((double)(float)w, x, d); vv = fma(x, x, vv); }
  }
  if (!v) return;                               // uniform: a plain weight's gradient is dW
  d = block_sum(d, red);
  vv = block_sum(vv, red);
  const double nrm = sqrt(vv), coef = d / vv, sc = (double)a.g[m] / nrm;
  if (threadIdx.x == 0) a.gg[m] = (float)(d / nrm);
  for (int q = threadIdx.x; q < a.L; q += 256) gw[q] = (float)(sc * ((double)gw[q] - coef * (double)v[q]));
}
void disc_wgrad_finish(hipStream_t s, const DiscWgradFinishArgs& a) {
  hipLaunchKernelGGL(disc_wgrad_finish_kernel, dim3((unsigned)a.Co), dim3(256), 0, s, a);
}

struct DiscWgradLaunch {
  bool gemm = false;
  ConvX3dWgradPlan x; DiscWgradDirectArgs d; dim3 dgrid; DiscWgradFinishArgs f;
  size_t part_floats = 0;
};
// pure: no stream, no launch, no allocation.  signals / fmaps / deltas / grads (all may be null: counting only).  The partial images' pointer is set by the
// caller once the largest part_floats of the plan is known.
static void disc_wgrad_plan(const Disc* D, const float* signals, int S, long long T, const float* const* fmaps, const float* const* deltas, float* const* grads,
                            std::vector<DiscWgradLaunch>& plan) {
  RVC_REQUIRE(D->ready, "finalize first");
  RVC_REQUIRE(D->kept, "weight_grad needs the parameters on the device: call rvc_disc_keep_parameters(d, 1) before finalize (trainable=True)");
  RVC_REQUIRE(S >= 1 && S <= 65535, "1 <= S <= 65535 signals");
  disc_check_T(D, T);
  plan.clear();
  const bool real = fmaps != nullptr;
  if (real) for (size_t k = 0; k < D->params.size(); ++k) RVC_REQUIRE(grads[k], "null gradient pointer");
  int tap0 = 0;
  for (size_t i = 0; i < D->nets.size(); ++i) {
    const DiscNet& net = D->nets[i];
    const int per = net.period ? net.period : 1;
    int H = (int)((T + per - 1) / per);
    for (size_t l = 0; l < net.L.size(); ++l) {
      const DiscLayer& L = net.L[l];
      const int Ho = conv_out(H, L.k, L.stride, L.pad);
      RVC_REQUIRE(Ho >= 1, "signal too short");
      if (real) RVC_REQUIRE(fmaps[tap0 + l] && deltas[tap0 + l], "null feature-map or delta pointer");
      const float* x = real ? (l == 0 ? signals : fmaps[tap0 + l - 1]) : nullptr;
      const float* delta = real ? deltas[tap0 + l] : nullptr;
      const long long N = (long long)Ho * per;
      const int cig = L.Ci / L.groups, Lrow = cig * L.k;
      RVC_REQUIRE((long long)L.Co * Lrow < (1LL << 31) && N < (1LL << 31), "layer too large");
      DiscWgradLaunch d;
      if (l > 0 && l + 1 < net.L.size() && disc_layer_is_gemm(L)) {
        d.gemm = true;
        const ConvX3dWgradArgs a{delta, x, nullptr, L.Ci, L.Co, H, Ho, per, L.k, L.stride, L.pad, S, 0, 0, 0};
        RVC_REQUIRE(conv_x3d_wgrad_plan(a, d.x), "discriminator layer does not fit the weight-gradient kernel");
        d.f.splits = d.x.splits; d.part_floats = d.x.part_floats;
      } else {
        const int blocks = (L.Co * Lrow + 255) / 256;
        const long long most = std::min<long long>(64, (N + 15) / 16);                    // a split sums at least 16 columns of every signal
        const long long splits0 = std::max<long long>(1, std::min<long long>((2048 + blocks - 1) / blocks, most));
        const int chunk = (int)((N + splits0 - 1) / splits0), splits = (int)((N + chunk - 1) / chunk);
        d.d = DiscWgradDirectArgs{delta, x, nullptr, S, L.Ci, L.Co, cig, L.Co / L.groups, L.k, L.stride, L.pad, H, Ho, per, l == 0 ? (int)T : 0, chunk};
        d.dgrid = dim3((unsigned)blocks, (unsigned)splits);
        d.f.splits = splits; d.part_floats = (size_t)splits * L.Co * Lrow;
      }
      d.f.part = nullptr; d.f.D = delta; d.f.v = L.gi_g >= 0 ? L.pv.p : nullptr; d.f.g = L.gi_g >= 0 ? L.pg.p : nullptr;
      d.f.gw = real ? grads[L.gi_w] : nullptr; d.f.gg = real && L.gi_g >= 0 ? grads[L.gi_g] : nullptr; d.f.gb = real ? grads[L.gi_b] : nullptr;
      d.f.pstride = (long long)L.Co * Lrow; d.f.S = S; d.f.Co = L.Co; d.f.N = (int)N; d.f.L = Lrow;
      plan.push_back(d);
      H = Ho;
    }
    tap0 += (int)net.L.size();
  }
}
int disc_weight_grad_launch_count(const Disc* D, int S, long long T) {
  std::vector<DiscWgradLaunch> plan;
  disc_wgrad_plan(D, nullptr, S, T, nullptr, nullptr, nullptr, plan);
  return 2 * (int)plan.size();
}
void disc_weight_grad(Disc* D, hipStream_t s, const float* signals, int S, long long T, const float* const* fmaps, const float* const* deltas, float* const* grads) {
  RVC_REQUIRE(signals && fmaps && deltas && grads, "null argument");
  std::vector<DiscWgradLaunch> plan;
  disc_wgrad_plan(D, signals, S, T, fmaps, deltas, grads, plan);
  size_t most = 0;
  for (const DiscWgradLaunch& d : plan) most = std::max(most, d.part_floats);
  float* part = (float*)stream_scratch(s, 24, most * sizeof(float));       // every layer's partial images in turn: the stream orders their uses
  for (DiscWgradLaunch& d : plan) {
    d.f.part = part;
    if (d.gemm) { d.x.a.part = part; conv_x3d_wgrad_launch(d.x, s); }
    else { d.d.part = part; hipLaunchKernelGGL(disc_wgrad_direct_kernel, d.dgrid, dim3(256), 0, s, d.d); }
    disc_wgrad_finish(s, d.f);
  }
}

}  // namespace rvc
