// The flow's weight-gradient pass (model_synth.hip::flow_wgrad): the weight gradient of a ResidualCouplingLayer's convolutions - pre, WN's k = 5 in_layers, its
// 1x1 res_skip layers, post - as ONE bf16x3 GEMM kernel over the items of a batch, EACH AT ITS OWN LENGTH, and the finishing kernel behind it (partials, weight
// norm, the bias sums, cond_layer's outer product).
//
// conv_flow_wgrad_kernel:  out[r][c k + t] = sum_item sum_{n < N[item]} P[item][r][n] act(G[item])[c][n + t + off0]
//   gate 0: act(G)[c] = G[c];  gate 1: G has 2 C rows and act(G)[c] = tanh(G[c]) sigmoid(G[C + c]) - WN's gate, which no forward stores: the recording forward
//           keeps only the pre-gate rows.  A wave fetches both rows of an element (two loads in flight while the previous stage is multiplied) and forms the
//           gate when the stage's loads have landed, just before the split, through the hardware's exp2 and reciprocal as conv_flow_bwd.hip does.
//   rows     r: WM * AM * 32 per workgroup (128, 64 or 32; the 32-row tile runs over 128 columns), as conv_gen_wgrad.hip.  Rows [0, R0) come from P, rows
//            [R0, R) from a second base pointer P2 (a res_skip layer's output cotangent is the pair [d x | d skip], two tensors of the tape).
//   columns  q = c k + t in the weight's own order; a last tile may be ragged
//   K        the reduction over (item, n), RAGGED: item b owns the stages [first[b], first[b + 1]) of 128 consecutive n, its last one ragged (n >= N[b] reads as
//            zero, of P and of G - the gate of two zeros is zero); a stage never straddles two items, and every descriptor has the item's own length.
// The loop is the pair loop of conv_x3gather_dev.h written out around gather_mfma3_unit, the B operand holding NV = 1 or 2 fetched values per element: the LDS
// layout, the three-MFMA unit and the order of the additions are gather_pair_loop's.  A change to that loop is made here as well.
// The reduction is SPLIT without atomics: blockIdx.z owns a contiguous run of the concatenated stages (a split may start inside an item) and writes its own
// partial image [R][C k]; flow_wgrad_finish_kernel adds the partials in index order, so two calls give the same bits.
#include "conv_x3gather_dev.h"
#include "signal_dev.h"

namespace rvc {

namespace {
constexpr int kKB = kGatherKB;

__device__ __forceinline__ float fw_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504f * x)); }
// tanh(x) = 2 sigmoid(2 x) - 1: exactly 0 at x = 0, so an element outside an item's length contributes nothing
__device__ __forceinline__ float fw_gate(float at, float as) { return (2.f * fw_sigmoid(2.f * at) - 1.f) * fw_sigmoid(as); }

template <int WM, int AM, bool GATE>
__global__ __launch_bounds__(256) void conv_flow_wgrad_kernel(const ConvFlowWgradArgs p) {
  constexpr int WN = 4 / WM, BM = WM * AM * 32, BN = WN * 32, NV = GATE ? 2 : 1;
  constexpr int kKU = kGatherKU, kARows = BM / 4, kBCols = BN / 4;          // rows of P and columns of G one wave fetches per stage
  constexpr int kABlock = gather_pair_block(BM), kBBlock = gather_pair_block(BN);
  constexpr int kAPlane = 2 * kKU * kABlock, kBPlane = 2 * kKU * kBBlock;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_fw[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave % WM, wn = wave / WM;
  const int c0 = blockIdx.x * BN, r0 = blockIdx.y * BM, split = blockIdx.z;
  const int ncols = p.C * p.k;
  const int g0 = split * p.per, g1 = min(g0 + p.per, p.total);
  // this wave's first column of G: (channel, tap); the following ones by counting
  const int q0 = c0 + wave * kBCols, qc0 = q0 / p.k, qt0 = q0 - qc0 * p.k;

  float ar[kARows][2], br[kBCols][NV][2];
  auto load = [&](int g) {
    int s = 0;
    while (s + 1 < p.B && g >= p.first[s + 1]) ++s;        // the stage's item (uniform; B <= 16)
    const int Ns = p.N[s];
    const unsigned rowbytes = (unsigned)Ns * 4u;
    const int n = (g - p.first[s]) * kKB + 2 * lane;
    const bool ok0 = n < Ns, ok1 = n + 1 < Ns;
#pragma unroll
    for (int i = 0; i < kARows; ++i) {
      const int r = r0 + wave * kARows + i;
      const bool row = r < p.R;                            // a 16-row layer on the 32-row tile: the rows behind it get an empty descriptor
      const float* base = !row ? p.P[s] : (r < p.R0 ? p.P[s] + (long long)r * Ns : p.P2[s] + (long long)(r - p.R0) * Ns);
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, row ? rowbytes : 0u);
      ar[i][0] = buf_load(rs, ok0 ? (unsigned)n * 4u : kOOB);
      ar[i][1] = buf_load(rs, ok1 ? (unsigned)n * 4u + 4u : kOOB);
    }
    const float* Gs = p.G[s];
    const int e = n + p.off0;
    int c = qc0, t = qt0;
#pragma unroll
    for (int i = 0; i < kBCols; ++i) {
      const bool col = q0 + i < ncols;
      const int e0 = e + t, e1 = e0 + 1;
      const unsigned o0 = (ok0 && e0 >= 0 && e0 < Ns) ? (unsigned)e0 * 4u : kOOB;
      const unsigned o1 = (ok1 && e1 >= 0 && e1 < Ns) ? (unsigned)e1 * 4u : kOOB;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(Gs + (long long)(col ? c + v * p.C : 0) * Ns, col ? rowbytes : 0u);
        br[i][v][0] = buf_load(rs, o0);
        br[i][v][1] = buf_load(rs, o1);
      }
      if (++t == p.k) { t = 0; ++c; }
    }
  };
  // lane l's pair is k = 2 l, 2 l + 1 of the stage: unit l >> 3, half (l >> 2) & 1, bytes 4 (l & 3) .. of the row's 16
  const int soff = (lane & 3) * 4;
  auto store = [&]() {
    unsigned char* a = smem_fw + (lane >> 2) * kABlock + (wave * kARows) * 16 + soff;
#pragma unroll
    for (int i = 0; i < kARows; ++i) {
      unsigned hi, lo;
      split2(ar[i][0], ar[i][1], hi, lo);
      *reinterpret_cast<unsigned*>(a + i * 16) = hi;
      *reinterpret_cast<unsigned*>(a + i * 16 + kAPlane) = lo;
    }
    unsigned char* b = smem_fw + 2 * kAPlane + (lane >> 2) * kBBlock + (wave * kBCols) * 16 + soff;
#pragma unroll
    for (int i = 0; i < kBCols; ++i) {
      float x0, x1;
      if constexpr (GATE) { x0 = fw_gate(br[i][0][0], br[i][1][0]); x1 = fw_gate(br[i][0][1], br[i][1][1]); }
      else { x0 = br[i][0][0]; x1 = br[i][0][1]; }
      unsigned hi, lo;
      split2(x0, x1, hi, lo);
      *reinterpret_cast<unsigned*>(b + i * 16) = hi;
      *reinterpret_cast<unsigned*>(b + i * 16 + kBPlane) = lo;
    }
  };

  f32x16 acc[AM];
#pragma unroll
  for (int am = 0; am < AM; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[am][r] = 0.f;

  const int aoff = lh * kABlock + (wm * (AM * 32) + li) * 16;
  const int boff = 2 * kAPlane + lh * kBBlock + (wn * 32 + li) * 16;
  if (g0 < g1) load(g0);
  for (int g = g0; g < g1; ++g) {
    __syncthreads();                               // the previous stage's operands have been read
    store();
    __syncthreads();
    if (g + 1 < g1) load(g + 1);                   // in flight while this stage is multiplied
#pragma unroll
    for (int ku = 0; ku < kKU; ++ku) gather_mfma3_unit<AM>(acc, smem_fw + aoff + ku * 2 * kABlock, kAPlane, smem_fw + boff + ku * 2 * kBBlock, kBPlane);
  }

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

template <int WM, int AM> void flow_wgrad_launch_t(const ConvFlowWgradPlan& p, hipStream_t s) {
  if (p.a.gate) {
    RVC_ALLOW_BIG_LDS((conv_flow_wgrad_kernel<WM, AM, true>));
    hipLaunchKernelGGL((conv_flow_wgrad_kernel<WM, AM, true>), p.grid, dim3(256), p.lds, s, p.a);
  } else {
    RVC_ALLOW_BIG_LDS((conv_flow_wgrad_kernel<WM, AM, false>));
    hipLaunchKernelGGL((conv_flow_wgrad_kernel<WM, AM, false>), p.grid, dim3(256), p.lds, s, p.a);
  }
}
}  // namespace

// pure: no stream, no launch, no allocation.  The tile follows the rows (128, 64, 32) as conv_gen_wgrad_plan chooses it; the stages are the items' own, item b
// owning ceil(N[b] / 128) of them from first[b]; the split count follows their total.
bool conv_flow_wgrad_plan(const ConvFlowWgradArgs& a0, ConvFlowWgradPlan& p) {
  ConvFlowWgradArgs a = a0;
  if (a.B < 1 || a.B > kGenWgradMaxItems || a.R < 16 || a.R % 16 != 0 || a.R0 < 1 || a.R0 > a.R || a.C < 1 || a.k < 1 || a.k > 16) return false;
  if (a.off0 > 4096 || a.off0 < -4096 || (a.gate != 0 && a.gate != 1)) return false;
  const long long ncols = (long long)a.C * a.k;
  if (ncols + 128 >= (1LL << 31) || (long long)a.R * ncols > (long long)kGenWgradPartFloats) return false;
  long long total = 0;
  for (int b = 0; b < a.B; ++b) {
    const long long n = a.N[b];
    if (n < 1) return false;
    // 32-bit element and byte offsets inside one row: a stage of columns, the taps past its end, the offset
    if ((n + kKB + a.k + 4096) * 4 >= (1LL << 31)) return false;
    a.first[b] = (int)total;
    total += (n + kKB - 1) / kKB;
    if (total >= (1LL << 30)) return false;
  }
  for (int b = a.B; b <= kGenWgradMaxItems; ++b) a.first[b] = (int)total;
  for (int b = a.B; b < kGenWgradMaxItems; ++b) a.N[b] = 0;
  a.total = (int)total;
  const int bm = a.R % 128 == 0 ? 128 : (a.R % 64 == 0 ? 64 : 32), bn = bm == 32 ? 128 : 64;
  const int rtiles = (a.R + bm - 1) / bm;                     // (a 16- or 48-row layer leaves the last 32-row tile half empty)
  const long long tiles = ((ncols + bn - 1) / bn) * rtiles;
  constexpr long long kTarget = 1024, kMaxSplits = 32;       // as conv_gen_wgrad_plan: about four workgroups per compute unit, a bound on the finishing pass's reads
  const long long fit = (long long)kGenWgradPartFloats / ((long long)a.R * ncols);      // partial images the buffer holds: >= 1 (checked above)
  const int splits = gather_splits(tiles, a.total, kTarget, std::min(kMaxSplits, fit), a.per);
  p.a = a;
  p.bm = bm;
  p.splits = splits;
  p.lds = gather_pair_lds(bm, bn);
  p.part_floats = (size_t)splits * a.R * ncols;
  p.grid = dim3((unsigned)((ncols + bn - 1) / bn), (unsigned)rtiles, (unsigned)splits);
  return true;
}
void conv_flow_wgrad_launch(const ConvFlowWgradPlan& p, hipStream_t s) {
  if (p.bm == 128) flow_wgrad_launch_t<2, 2>(p, s);
  else if (p.bm == 64) flow_wgrad_launch_t<2, 1>(p, s);
  else flow_wgrad_launch_t<1, 1>(p, s);
}

// ------------------------------------------------------------------------------------------------ the finishing kernel
namespace {
// gen_wgrad_finish_kernel for ragged items.  One workgroup per row m of the weight: dW[m] = the partials added in index order - or, outer = 1 (cond_layer), the
// float64 outer product sum_item V[item][m] Gv[item][q], items in index order - then the weight-norm chain (dim 0) where v is given, with n = |v[m]| and
// d = <dW[m], v[m]>: grad_g[m] = d / n, grad_v[m] = (g[m] / n) (dW[m] - (d / n^2) v[m]).  The bias gradient gb[m]: bias 1, the float64 sum of row m of the pair
// [D | D2] over every item's own N[item] columns (thread-strided, then block_sum: a fixed order); bias 2, the float64 sum over the items of V[item][m] (row sums
// the data pass has already formed).  gw doubles as the row's store between the two passes: a thread re-reads only what it wrote itself.
__global__ __launch_bounds__(256) void flow_wgrad_finish_kernel(const FlowWgradFinishArgs a) {
  __shared__ double red[4];
  const int m = blockIdx.x;
  if (a.bias == 1) {                               // uniform
    double bs = 0.0;
    for (int b = 0; b < a.B; ++b) {
      const long long N = a.N[b];
      const float* D = m < a.R0 ? a.D.p[b] + (long long)m * N : a.D2.p[b] + (long long)(m - a.R0) * N;
      for (long long n = threadIdx.x; n < N; n += 256) bs += (double)D[n];
    }
    bs = block_sum(bs, red);
    if (threadIdx.x == 0) a.gb[m] = (float)bs;
  } else if (a.bias == 2 && threadIdx.x == 0) {
    double bs = 0.0;
    for (int b = 0; b < a.B; ++b) bs += (double)a.V.p[b][m];
    a.gb[m] = (float)bs;
  }
  const float* P = a.part + (long long)m * a.L;
  const float* v = a.v ? a.v + (long long)m * a.L : nullptr;
  float* gw = a.gw + (long long)m * a.L;
  double d = 0.0, vv = 0.0;
  for (int q = threadIdx.x; q < a.L; q += 256) {
    double w = 0.0;
    if (a.outer) { for (int b = 0; b < a.B; ++b) w = fma((double)a.V.p[b][m], (double)a.Gv.p[b][q], w); }
    else { for (int z = 0; z < a.splits; ++z) w += (double)P[(long long)z * a.pstride + q]; }
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
}  // namespace

void flow_wgrad_finish(hipStream_t s, const FlowWgradFinishArgs& a) {
  hipLaunchKernelGGL(flow_wgrad_finish_kernel, dim3((unsigned)a.R), dim3(256), 0, s, a);
}

}  // namespace rvc
