// Weight gradient of conv_x3d.hip's strided k-tap convolution along H (the discriminators' dense layers) as ONE bf16x3 GEMM launch in the same layout
// [S][C][H][p]:  dW[m][c][j] = sum_s sum_n D[s][m][n] X[s][c][stride n - (stride - 1) w + (j - pad) p]  with n = h' p + w over the Hout p outputs.
//   rows     m: output channels, 128 per workgroup (4 waves as 2 x 2, each 64 rows x 32 columns = two 32 x 32 accumulators)
//   columns  q = c k + j in the weight's own order [Ci][k], 64 per workgroup: the partial image is the weight's layout; a last tile may be ragged
//   K        the reduction over (signal, n): stages of ONE signal and 128 consecutive n, 8 units of three v_mfma_f32_32x32x16_bf16 per accumulator
//            (hi lo, lo hi, hi hi).  A signal's last stage is ragged (n >= N reads as zero), so any S N >= 1 is right - a plane of one row included.
// BOTH operands are fp32 activations and are split (split2) inside the kernel.  A load instruction fetches ONE row of D or ONE column (c, j) of X for
// 64 lanes, through a buffer descriptor of exactly that (signal, channel) plane: lane l holds the neighbours n = 2 l and 2 l + 1 of the stage (two
// loads), so a split2 gives one packed bf16 pair per plane and the operand tiles [hi | lo][unit][half][row][8 k] are written with 32-bit LDS stores.
// A tap above row 0 or below row H - 1, and every n >= N, is outside the descriptor's range (or is given kOOB) and reads as zero: no tap can reach
// another channel's or another signal's rows.  X is gathered with the forward's element formula.
// The reduction is SPLIT without atomics: blockIdx.z = split owns a contiguous run of stages and writes its own partial image [Co][Ci k]; the
// finishing kernel (discriminator.hip) adds the partials in index order, so two calls give the same bits.  Registers hold the next stage's loads
// while the current one is multiplied.
// This is the pair loop of conv_x3gather_dev.h written out: through the shared loop the compiler schedules the 160 loads of a stage differently and the pass
// measured 1.8 % slower (profiles/x3g_dedup_timing.txt), so the kernel keeps its own copy; the planner shares the header's arithmetic.
#include "conv_x3gather_dev.h"

namespace rvc {

namespace {
constexpr int kBM = 128, kBN = 64, kKB = 128, kKU = kKB / 16;
// one (unit, half) block of rows is padded by one 16-B row: the 16 groups of 4 lanes of a store land in 16 different bank quads
constexpr int kABlock = kBM * 16 + 16, kBBlock = kBN * 16 + 16;
constexpr int kAPlane = 2 * kKU * kABlock, kBPlane = 2 * kKU * kBBlock;
constexpr int kLds = 2 * kAPlane + 2 * kBPlane;
constexpr int kARows = kBM / 4, kBCols = kBN / 4;        // rows of D and columns of X one wave fetches per stage

__global__ __launch_bounds__(256) void conv_x3d_wgrad_kernel(const ConvX3dWgradArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_x3w[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int c0 = blockIdx.x * kBN, r0 = blockIdx.y * kBM, split = blockIdx.z;
  const int HP = p.H * p.p, N = p.Hout * p.p, ncols = p.Ci * p.k;
  const int g0 = split * p.per, g1 = min(g0 + p.per, p.total);

  // this wave's share of a stage: rows r0 + 32 wave + i of D and columns c0 + 16 wave + i of X (a column past the end gets an empty descriptor)
  float ar[kARows][2], br[kBCols][2];
  auto load = [&](int g) {
    const int s = g / p.cps, nc = (g - s * p.cps) * kKB;
    const int n = nc + 2 * lane;
    const int w0 = n % p.p, w1 = w0 + 1 == p.p ? 0 : w0 + 1;
    const int e0 = p.stride * n - (p.stride - 1) * w0, e1 = p.stride * (n + 1) - (p.stride - 1) * w1;
    const bool ok0 = n < N, ok1 = n + 1 < N;
    const float* Dw = p.D + ((long long)s * p.Co + r0 + wave * kARows) * N;
#pragma unroll
    for (int i = 0; i < kARows; ++i) {
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(Dw + (long long)i * N, (unsigned)N * 4u);
      ar[i][0] = buf_load(rs, (unsigned)n * 4u);
      ar[i][1] = buf_load(rs, (unsigned)n * 4u + 4u);
    }
    const float* Xs = p.X + (long long)s * p.Ci * HP;
#pragma unroll
    for (int i = 0; i < kBCols; ++i) {
      const int q = c0 + wave * kBCols + i;
      const int c = q / p.k, j = q - c * p.k;
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(Xs + (long long)(q < ncols ? c : 0) * HP, q < ncols ? (unsigned)HP * 4u : 0u);
      const int t = (j - p.pad) * p.p;
      br[i][0] = buf_load(rs, ok0 ? (unsigned)(e0 + t) * 4u : kOOB);
      br[i][1] = buf_load(rs, ok1 ? (unsigned)(e1 + t) * 4u : kOOB);
    }
  };
  // lane l's pair is k = 2 l, 2 l + 1 of the stage: unit l >> 3, half (l >> 2) & 1, bytes 4 (l & 3) .. of the row's 16
  const int soff = (lane & 3) * 4;
  auto store = [&]() {
    unsigned char* a = smem_x3w + (lane >> 2) * kABlock + (wave * kARows) * 16 + soff;
#pragma unroll
    for (int i = 0; i < kARows; ++i) {
      unsigned hi, lo;
      split2(ar[i][0], ar[i][1], hi, lo);
      *reinterpret_cast<unsigned*>(a + i * 16) = hi;
      *reinterpret_cast<unsigned*>(a + i * 16 + kAPlane) = lo;
    }
    unsigned char* b = smem_x3w + 2 * kAPlane + (lane >> 2) * kBBlock + (wave * kBCols) * 16 + soff;
#pragma unroll
    for (int i = 0; i < kBCols; ++i) {
      unsigned hi, lo;
      split2(br[i][0], br[i][1], hi, lo);
      *reinterpret_cast<unsigned*>(b + i * 16) = hi;
      *reinterpret_cast<unsigned*>(b + i * 16 + kBPlane) = lo;
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[am][r] = 0.f;

  const int aoff = lh * kABlock + (wm * 64 + li) * 16;
  const int boff = 2 * kAPlane + lh * kBBlock + (wn * 32 + li) * 16;
  if (g0 < g1) load(g0);
  for (int g = g0; g < g1; ++g) {
    __syncthreads();                               // the previous stage's operands have been read
    store();
    __syncthreads();
    if (g + 1 < g1) load(g + 1);                   // in flight while this stage is multiplied
#pragma unroll
    for (int ku = 0; ku < kKU; ++ku) gather_mfma3_unit<2>(acc, smem_x3w + aoff + ku * 2 * kABlock, kAPlane, smem_x3w + boff + ku * 2 * kBBlock, kBPlane);
  }

  // the split's partial image, in the weight's layout
  const int q = c0 + wn * 32 + li;
  if (q < ncols) {
    float* P = p.part + ((long long)split * p.Co + r0 + wm * 64 + acc_row32(0, lh)) * ncols + q;
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) P[(long long)(am * 32 + acc_row32(r, 0)) * ncols] = acc[am][r];
  }
}
}  // namespace

// pure: no stream, no launch, no allocation.  Chooses the split count: enough workgroups for the device where the output is small and the reduction
// long (128 x 160 outputs over up to ~35 000 columns), one split where the output tiles fill it by themselves.
bool conv_x3d_wgrad_plan(const ConvX3dWgradArgs& a0, ConvX3dWgradPlan& p) {
  ConvX3dWgradArgs a = a0;
  if (a.Ci <= 0 || a.Co <= 0 || a.Co % kBM != 0 || a.k < 1 || a.k > 16 || a.stride < 1 || a.pad < 0 || a.p < 1 || a.S < 1 || a.S > 65535) return false;
  if (a.H < 1 || a.Hout != (a.H + 2 * a.pad - a.k) / a.stride + 1 || a.Hout < 1) return false;
  const long long HP = (long long)a.H * a.p, N = (long long)a.Hout * a.p, ncols = (long long)a.Ci * a.k;
  // 32-bit byte offsets inside one plane of X (and one stage of columns and the taps past its end) and inside one row of D
  if ((HP + (long long)a.stride * (N + kKB) + (long long)a.k * a.p) * 4 >= (1LL << 31) || (N + kKB) * 4 >= (1LL << 31)) return false;
  a.cps = (int)((N + kKB - 1) / kKB);
  if ((long long)a.S * a.cps >= (1LL << 30)) return false;
  a.total = a.S * a.cps;
  const long long tiles = ((ncols + kBN - 1) / kBN) * (a.Co / kBM);
  constexpr long long kTarget = 1024, kMaxSplits = 64;       // about four workgroups per compute unit; a bound on the partial images
  const int splits = gather_splits(tiles, a.total, kTarget, kMaxSplits, a.per);
  p.a = a;
  p.splits = splits;
  p.lds = kLds;
  static_assert(kLds == gather_pair_lds(kBM, kBN), "the kernel's tiles are the pair loop's");
  p.part_floats = (size_t)splits * a.Co * ncols;
  p.grid = dim3((unsigned)((ncols + kBN - 1) / kBN), (unsigned)(a.Co / kBM), (unsigned)splits);
  p.flops = 2.0 * a.S * (double)N * a.Co * a.Ci * a.k;
  return true;
}
void conv_x3d_wgrad_launch(const ConvX3dWgradPlan& p, hipStream_t s) {
  RVC_ALLOW_BIG_LDS(conv_x3d_wgrad_kernel);
  hipLaunchKernelGGL(conv_x3d_wgrad_kernel, p.grid, dim3(256), p.lds, s, p.a);
}

}  // namespace rvc
