// The decoder's weight-gradient pass (model_synth.hip::synth_dec_weight_grad): the weight gradient of its dense 1-D convolutions - every ResBlock convolution,
// every up-sampler, conv_pre - as ONE bf16x3 GEMM kernel over the items of a batch, and the direct kernels around it (finish with the weight-norm chain, the
// noise convolutions, conv_post, the conditioning's outer product, m_source).
//
// conv_gen_wgrad_kernel:  out[r][c k + t] = sum_item sum_n a_P(P[item][r][n]) a_G(G[item][c][cstride n + tstep t + off0]),  a_X(v) = max(v, slope_X v) (slope 1: none)
//   Conv1d(C, R, k, dilation d, pad): P = the layer's delta [R][N], G = the layer's input [C][N] (a pre-activation: the leaky ReLU is applied here, no activated
//                                     copy exists), (cstride, tstep, off0) = (1, d, -pad): the output is the weight [R][C][k]
//   ConvTranspose1d(R, C, k, u, pad): P = the layer's input [R][N], G = the layer's delta [C][u N], (u, 1, -pad): the output is the weight [R][C][k]
//   rows     r: WM * AM * 32 per workgroup (128, 64 or 32; the 32-row tile runs over 128 columns, as in conv_gen_bwd.hip)
//   columns  q = c k + t in the weight's own order, (4 / WM) * 32 per workgroup; a last tile may be ragged
//   K        the reduction over (item, n): stages of ONE item and 128 consecutive n, the pair loop of conv_x3gather_dev.h.  An item's last stage is ragged
//            (n >= N reads as zero): a stage never straddles two items.
// Every item is its own allocation with the same layout (a tape): the kernel receives one base pointer per item and operand.  A load instruction fetches ONE
// row of P or ONE column (c, t) of G for 64 lanes through a descriptor of exactly that (item, channel) row; an element outside [0, Tg) and every n >= N is given
// kOOB and reads as zero.  BOTH operands are fp32 and are split in the loop after the activation.
// The reduction is SPLIT without atomics: blockIdx.z owns a contiguous run of stages and writes its own partial image [R][C k]; gen_wgrad_finish_kernel adds the
// partials in index order, so two calls give the same bits.
#include "conv_x3gather_dev.h"
#include "signal_dev.h"

namespace rvc {

namespace {
constexpr int kKB = kGatherKB;

template <int WM, int AM>
__global__ __launch_bounds__(256) void conv_gen_wgrad_kernel(const ConvGenWgradArgs p) {
  constexpr int WN = 4 / WM, BM = WM * AM * 32, BN = WN * 32;
  constexpr int kARows = BM / 4, kBCols = BN / 4;          // rows of P and columns of G one wave fetches per stage
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_gw[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave % WM, wn = wave / WM;
  const int c0 = blockIdx.x * BN, r0 = blockIdx.y * BM, split = blockIdx.z;
  const int ncols = p.C * p.k;
  const int g0 = split * p.per, g1 = min(g0 + p.per, p.total);
  // this wave's first column of G: (channel, tap); the following ones by counting
  const int q0 = c0 + wave * kBCols, qc0 = q0 / p.k, qt0 = q0 - qc0 * p.k;

  auto load = [&](int g, float (&ar)[kARows][2], float (&br)[kBCols][2]) {
    const int s = g / p.cps, nc = (g - s * p.cps) * kKB;
    const int n = nc + 2 * lane;
    const bool ok0 = n < p.N, ok1 = n + 1 < p.N;
    const float* Pw = p.P[s] + (long long)(r0 + wave * kARows) * p.ldP;
#pragma unroll
    for (int i = 0; i < kARows; ++i) {
      const bool row = r0 + wave * kARows + i < p.R;      // a 16-row layer on the 32-row tile: the rows behind it get an empty descriptor
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(row ? Pw + (long long)i * p.ldP : p.P[s], row ? (unsigned)p.N * 4u : 0u);
      ar[i][0] = buf_load(rs, ok0 ? (unsigned)n * 4u : kOOB);
      ar[i][1] = buf_load(rs, ok1 ? (unsigned)n * 4u + 4u : kOOB);
    }
    const float* Gs = p.G[s];
    const int e = p.cstride * n + p.off0;
    int c = qc0, t = qt0;
#pragma unroll
    for (int i = 0; i < kBCols; ++i) {
      const bool col = q0 + i < ncols;
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(Gs + (long long)(col ? c : 0) * p.ldG, col ? (unsigned)p.Tg * 4u : 0u);
      const int e0 = e + t * p.tstep, e1 = e0 + p.cstride;
      br[i][0] = buf_load(rs, (ok0 && e0 >= 0 && e0 < p.Tg) ? (unsigned)e0 * 4u : kOOB);
      br[i][1] = buf_load(rs, (ok1 && e1 >= 0 && e1 < p.Tg) ? (unsigned)e1 * 4u : kOOB);
      if (++t == p.k) { t = 0; ++c; }
    }
  };
  f32x16 acc[AM];
  gather_pair_loop<BM, BN, AM>(smem_gw, g0, g1, wave, lane, wm, wn, acc, load, GatherLrelu{p.slopeP}, GatherLrelu{p.slopeG});

  // the split's partial image, in the weight's layout
  const int q = c0 + wn * 32 + li;
  if (q < ncols) {
    const int row0 = r0 + wm * (AM * 32) + acc_row32(0, lh);
    float* O = p.part + ((long long)split * p.R + row0) * ncols + q;
#pragma unroll
    for (int am = 0; am < AM; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int dr = am * 32 + acc_row32(r, 0);
        if (row0 + dr < p.R) O[(long long)dr * ncols] = acc[am][r];
      }
  }
}

template <int WM, int AM> void gen_wgrad_launch_t(const ConvGenWgradPlan& p, hipStream_t s) {
  RVC_ALLOW_BIG_LDS((conv_gen_wgrad_kernel<WM, AM>));
  hipLaunchKernelGGL((conv_gen_wgrad_kernel<WM, AM>), p.grid, dim3(256), p.lds, s, p.a);
}
}  // namespace

// pure: no stream, no launch, no allocation.  The tile follows the rows (128, 64, 32); the split count follows the reduction length B ceil(N / 128): enough
// workgroups for the device where the output is small and the reduction long (32 x 352 outputs over B seg upp columns), one split where the output tiles fill it
// by themselves, never more partial images than kGenWgradPartFloats holds.
bool conv_gen_wgrad_plan(const ConvGenWgradArgs& a0, ConvGenWgradPlan& p) {
  ConvGenWgradArgs a = a0;
  if (a.B < 1 || a.B > kGenWgradMaxItems || a.R < 16 || a.R % 16 != 0 || a.C < 1 || a.k < 1 || a.k > 16 || a.N < 1 || a.Tg < 1) return false;
  if (a.ldP < a.N || a.ldG < a.Tg || a.cstride < 1 || a.tstep < 1 || a.off0 > 4096 || a.off0 < -4096) return false;
  if (!(a.slopeP >= 0.f && a.slopeP <= 1.f && a.slopeG >= 0.f && a.slopeG <= 1.f)) return false;      // max(v, slope v) is the leaky ReLU for these slopes only
  const long long ncols = (long long)a.C * a.k;
  // 32-bit element and byte offsets inside one row of G (a stage of columns and the taps past its end) and inside one row of P
  if (((long long)a.cstride * ((long long)a.N + kKB) + (long long)a.tstep * a.k + 4096) * 4 >= (1LL << 31) || (long long)a.Tg * 4 >= (1LL << 31)) return false;
  if (((long long)a.N + kKB) * 4 >= (1LL << 31) || ncols + 128 >= (1LL << 31)) return false;
  if ((long long)a.R * ncols > (long long)kGenWgradPartFloats) return false;
  const int bm = a.R % 128 == 0 ? 128 : (a.R % 64 == 0 ? 64 : 32), bn = bm == 32 ? 128 : 64;
  a.cps = (int)(((long long)a.N + kKB - 1) / kKB);
  if ((long long)a.B * a.cps >= (1LL << 30)) return false;
  a.total = a.B * a.cps;
  const int rtiles = (a.R + bm - 1) / bm;                     // (a 16- or 48-row layer leaves the last 32-row tile half empty)
  const long long tiles = ((ncols + bn - 1) / bn) * rtiles;
  constexpr long long kTarget = 1024, kMaxSplits = 32;       // about four workgroups per compute unit; a bound on the finishing pass's reads
  const long long fit = (long long)kGenWgradPartFloats / ((long long)a.R * ncols);      // partial images the buffer holds: >= 1 (checked above)
  const int splits = gather_splits(tiles, a.total, kTarget, std::min(kMaxSplits, fit), a.per);
  p.a = a;
  p.bm = bm;
  p.splits = splits;
  p.lds = gather_pair_lds(bm, bn);
  p.part_floats = (size_t)splits * a.R * ncols;
  p.grid = dim3((unsigned)((ncols + bn - 1) / bn), (unsigned)rtiles, (unsigned)splits);
  p.flops = 2.0 * a.B * (double)a.N * a.R * (double)ncols;
  return true;
}
void conv_gen_wgrad_launch(const ConvGenWgradPlan& p, hipStream_t s) {
  if (p.bm == 128) gen_wgrad_launch_t<2, 2>(p, s);
  else if (p.bm == 64) gen_wgrad_launch_t<2, 1>(p, s);
  else gen_wgrad_launch_t<1, 1>(p, s);
}

// ------------------------------------------------------------------------------------------------ the direct kernels
namespace {
// One workgroup per row m of the weight: dW[m] = the partials added in index order; the weight-norm chain (dim 0) where v is given, with n = |v[m]| and
// d = <dW[m], v[m]>: grad_g[m] = d / n, grad_v[m] = (g[m] / n) (dW[m] - (d / n^2) v[m]) (the formulas of disc_wgrad_finish_kernel); gw receives dW itself
// otherwise.  Rows m < brows also form a bias gradient: the float64 sum of row m of D over the items (thread-strided, then block_sum: a fixed order).
// gw doubles as the row's store between the two passes: a thread re-reads only what it wrote itself.
__global__ __launch_bounds__(256) void gen_wgrad_finish_kernel(const GenWgradFinishArgs a) {
  __shared__ double red[4];
  const int m = blockIdx.x;
  if (a.gb && m < a.brows) {                       // uniform
    double bs = 0.0;
    for (int b = 0; b < a.B; ++b) {
      const float* D = a.D.p[b] + (long long)m * a.N;
      for (long long n = threadIdx.x; n < a.N; n += 256) bs += (double)D[n];
    }
    bs = block_sum(bs, red);
    if (threadIdx.x == 0) a.gb[m] = (float)bs;
  }
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
  if (!v) return;                                  // uniform: a plain weight's gradient is dW
  d = block_sum(d, red);
  vv = block_sum(vv, red);
  const double nrm = sqrt(vv), coef = d / vv, sc = (double)a.g[m] / nrm;
  if (threadIdx.x == 0) a.gg[m] = (float)(d / nrm);
  for (int q = threadIdx.x; q < a.L; q += 256) gw[q] = (float)(sc * ((double)gw[q] - coef * (double)v[q]));
}

// noise_convs.i, Conv1d(1, C, k, stride s, pad) on the harmonic source: one workgroup per channel c,
//   dW[c][t] = sum_item sum_n D[c][n] har[s n + t - pad] (outside [0, Nh): zero),  db[c] = sum_item sum_n D[c][n],  float64, fixed order
__global__ __launch_bounds__(256) void gen_wgrad_noise_kernel(const GenItems D, const GenItems H, int B, long long T, long long Nh, int k, int s, int pad, float* gw, float* gb) {
  __shared__ double red[4];
  const int c = blockIdx.x;
  for (int t = 0; t <= k; ++t) {                   // t = k: the bias
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
      const float* d = D.p[b] + (long long)c * T;
      const float* h = H.p[b];
      for (long long n = threadIdx.x; n < T; n += 256) {
        if (t == k) { acc += (double)d[n]; continue; }
        const long long e = (long long)s * n + t - pad;
        if (e >= 0 && e < Nh) acc = fma((double)d[n], (double)h[e], acc);
      }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) { if (t == k) gb[c] = (float)acc; else gw[(long long)c * k + t] = (float)acc; }
  }
}

// conv_post, Conv1d(C, 1, k, pad) without a bias behind a leaky ReLU of slope `slope`: one workgroup per (c, t),
//   dW[0][c][t] = sum_item sum_n d[n] lrelu(x[c][n + t - pad])
__global__ __launch_bounds__(256) void gen_wgrad_post_kernel(const GenItems D, const GenItems X, int B, long long T, int k, int pad, float slope, float* gw) {
  __shared__ double red[4];
  const int c = blockIdx.x, t = blockIdx.y;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* d = D.p[b];
    const float* x = X.p[b] + (long long)c * T;
    for (long long n = threadIdx.x; n < T; n += 256) {
      const long long e = n + t - pad;
      if (e >= 0 && e < T) { const float v = x[e]; acc = fma((double)d[n], (double)(v > 0.f ? v : v * slope), acc); }
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) gw[(long long)c * k + t] = (float)acc;
}

// cond, Conv1d(gin, C, 1) on the item's speaker row: one workgroup per channel c,  dW[c][g] = sum_item dcond[item][c] g[item][g],  db[c] = sum_item dcond[item][c]
// (written twice: cond.bias and conv_pre.bias receive the same cotangent), float64, items in index order
__global__ __launch_bounds__(256) void gen_wgrad_cond_kernel(const GenItems DC, const GenItems Gv, int B, int G, float* gw, float* gb, float* gb2) {
  const int c = blockIdx.x;
  for (int g = threadIdx.x; g < G; g += 256) {
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc = fma((double)DC.p[b][c], (double)Gv.p[b][g], acc);
    gw[(long long)c * G + g] = (float)acc;
  }
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += (double)DC.p[b][c];
    gb[c] = (float)acc; gb2[c] = (float)acc;
  }
}

// m_source.l_linear (har = tanh(w sine + b)): e[n] = d.har[n] (1 - har[n]^2);  dw = sum e sine, db = sum e, float64; one workgroup
__global__ __launch_bounds__(256) void gen_wgrad_msource_kernel(const GenItems DH, const GenItems H, const GenItems Sn, int B, long long N, float* gw, float* gb) {
  __shared__ double red[4];
  double aw = 0.0, ab = 0.0;
  for (int b = 0; b < B; ++b) {
    const float *dh = DH.p[b], *h = H.p[b], *sn = Sn.p[b];
    for (long long n = threadIdx.x; n < N; n += 256) {
      const double hv = (double)h[n], e = (double)dh[n] * (1.0 - hv * hv);
      aw = fma(e, (double)sn[n], aw); ab += e;
    }
  }
  aw = block_sum(aw, red);
  ab = block_sum(ab, red);
  if (threadIdx.x == 0) { gw[0] = (float)aw; gb[0] = (float)ab; }
}
}  // namespace

void gen_wgrad_finish(hipStream_t s, const GenWgradFinishArgs& a) {
  hipLaunchKernelGGL(gen_wgrad_finish_kernel, dim3((unsigned)a.R), dim3(256), 0, s, a);
}
void gen_wgrad_noise(hipStream_t s, const GenItems& D, const GenItems& H, int B, int C, long long T, long long Nh, int k, int stride, int pad, float* gw, float* gb) {
  hipLaunchKernelGGL(gen_wgrad_noise_kernel, dim3((unsigned)C), dim3(256), 0, s, D, H, B, T, Nh, k, stride, pad, gw, gb);
}
void gen_wgrad_post(hipStream_t s, const GenItems& D, const GenItems& X, int B, int C, long long T, int k, int pad, float slope, float* gw) {
  hipLaunchKernelGGL(gen_wgrad_post_kernel, dim3((unsigned)C, (unsigned)k), dim3(256), 0, s, D, X, B, T, k, pad, slope, gw);
}
void gen_wgrad_cond(hipStream_t s, const GenItems& DC, const GenItems& Gv, int B, int C, int G, float* gw, float* gb, float* gb2) {
  hipLaunchKernelGGL(gen_wgrad_cond_kernel, dim3((unsigned)C), dim3(256), 0, s, DC, Gv, B, G, gw, gb, gb2);
}
void gen_wgrad_msource(hipStream_t s, const GenItems& DH, const GenItems& H, const GenItems& Sn, int B, long long N, float* gw, float* gb) {
  hipLaunchKernelGGL(gen_wgrad_msource_kernel, dim3(1), dim3(256), 0, s, DH, H, Sn, B, N, gw, gb);
}

}  // namespace rvc
