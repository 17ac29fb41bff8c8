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
#include "model_common.h"
#include "models.h"
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
struct DiscLayer {
  int Ci = 0, Co = 0, k = 0, stride = 1, pad = 0, groups = 1, CoPx = 0;
  DevVec w, b;                       // folded fp32 weights [Co][Ci / groups][k] (the VALU layers) and bias
  DevBuf<uint16_t> wx;               // bf16x3 image (the GEMM layers)
};
struct DiscNet { int period = 0; std::vector<DiscLayer> L; };   // period 0: DiscriminatorS; L.back() is conv_post
struct DiscWeights { std::vector<DiscNet> nets; };
struct Disc : DiscWeights {
  Ctx* ctx = nullptr;
  int version = 2;
  TensorStore ts;
  bool ready = false;
};

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
static bool disc_layer_is_gemm(const DiscLayer& l) { return l.groups == 1 && l.Ci % 16 == 0 && l.Co > 1; }

void disc_finalize(Disc* D) {
  D->ready = false; static_cast<DiscWeights&>(*D) = {};   // a finalize that throws leaves the handle not ready
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
      if (disc_layer_is_gemm(L)) {
        L.CoPx = (c.Co + 127) & ~127;
        std::vector<uint16_t> img;
        x3_weight_image(w.data(), c.Co, c.Ci, c.k, L.CoPx, img);
        L.wx.upload(img);
      } else {
        L.w.upload(w);
      }
      net.L.push_back(std::move(L));
    }
    D->nets.push_back(std::move(net));
  }
  D->ts.clear();
  D->ready = true;
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

}  // namespace rvc
