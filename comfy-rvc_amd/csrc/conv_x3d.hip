// Strided k-tap convolution along H over a batch of [Ci][H][p] tensors as ONE bf16x3 GEMM launch (the discriminators of the trainer:
// reference lib/infer_pack/models.py:1111-1145 DiscriminatorP's Conv2d((5, 1), stride (3, 1)) layers, and with p = 1 DiscriminatorS's dense
// Conv1d(1024, 1024, 5), :1093).  Y[s][m][h'][w] = lrelu(b[m] + sum_c sum_j W[m][c][j] X[s][c][stride h' + j - pad][w]).
//   rows     m: output channels, 128 per workgroup (4 waves as 2 x 2, each 64 rows x 32 columns = two 32 x 32 accumulators)
//   columns  n = h' p + w of ONE signal, 64 per workgroup; blockIdx.z = signal, so one launch covers every signal and every column of the
//            period and the weight image is streamed once per layer (the column tiles of all signals share it through L2)
//   K        units of (16-channel chunk, tap), tap fastest; three v_mfma_f32_32x32x16_bf16 per unit and accumulator (hi lo, lo hi, hi hi)
// Input and output stay in the reference's layout [S][C][H][p]: the post-activation output is the feature map the caller gets AND the next
// layer's input - nothing is transposed or copied.  im2col by address: column n, tap j reads flat element stride n - (stride - 1) w +
// (j - pad) p of the (signal, channel) plane through a buffer descriptor of exactly that plane (H p floats), so a tap above row 0 or below
// row H - 1 is out of the descriptor's range and reads as zero (conv_kernels.h, kOOB) - no branch, and no tap can reach another channel's
// or another signal's rows.  Each wave gathers 4 channels of the chunk (wave-uniform descriptors), splits them (split2) and writes its
// quarter of the [hi | lo][half][64 columns][8 ch] operand; the weights come by LDS-DMA from the image conv1d's bf16x3 layers use
// ([chunk][tap][hi | lo][half][CoPx rows][8 ch]).  Two slots of U units each in LDS: stage st + 1 is fetched while stage st is multiplied.
#include "conv_x3_dev.h"

namespace rvc {

namespace {
constexpr int kBM = 128, kBN = 64;
constexpr int kASlot = kBM * 64;               // bytes of [hi | lo][half][kBM rows][16 B]
constexpr int kBSlot = kBN * 64;               // bytes of [hi | lo][half][kBN columns][16 B]
constexpr int kUSlot = kASlot + kBSlot;

// U: units per stage.  A stage is what one barrier publishes: its U weight units and U operand quarters are in flight together, so the latency of
// the fetch is paid once per U units (the grids of the deep layers are below one workgroup per CU: nothing else hides it).
template <int U>
__global__ __launch_bounds__(256) void conv_x3d_kernel(const ConvX3dArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_x3d[];      // 2 slots of U units
  constexpr int kSlot = U * kUSlot;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int n0 = blockIdx.x * kBN, co0 = blockIdx.y * kBM, sig = blockIdx.z;
  const int HP = p.H * p.p, N = p.Hout * p.p;
  const int nunits = (p.Ci >> 4) * p.k, nstages = nunits / U;                     // the planner chose U as a divisor of the units

  // weights: the unit's four (plane, half) row blocks of 128 rows are eight 1-KiB pieces; this wave fetches the two of block `wave`
  const __amdgpu_buffer_rsrc_t ars = make_rsrc(p.Wx, (unsigned)nunits * (unsigned)p.CoPx * 64u);
  const int avoff = (wave * p.CoPx + co0 + lane) * 16;
  const int astep = p.CoPx * 64;                                    // bytes of one unit of the image
  // input: channels 4 wave .. 4 wave + 3 of the chunk at column n0 + lane
  const int n = n0 + lane;
  const int w = n % p.p;
  const int e0 = p.stride * n - (p.stride - 1) * w - p.pad * p.p;   // element of tap 0 in the plane (negative: above row 0)
  const float* Xw = p.X + ((long long)sig * p.Ci + wave * 4) * HP;

  float xr[U][4];
  int chunk_n = 0, tap_n = 0, asoff = 0;                            // (chunk, tap) and image offset of the next unit to be issued
  auto issue = [&](int slot) {
#pragma unroll
    for (int q = 0; q < U; ++q) {
      unsigned char* base = smem_x3d + slot * kSlot + q * kUSlot;
      buf_dma(ars, base + wave * (kBM * 16), avoff, asoff);
      buf_dma(ars, base + wave * (kBM * 16) + 1024, avoff + 1024, asoff);
      asoff += astep;
      const unsigned voff = (unsigned)(e0 + tap_n * p.p) * 4u;
      const float* cb = Xw + (long long)chunk_n * 16 * HP;
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[q][i] = buf_load(make_rsrc(cb + (long long)i * HP, (unsigned)HP * 4u), voff);
      if (++tap_n == p.k) { tap_n = 0; ++chunk_n; }
    }
  };
  auto store_b = [&](int slot) {
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < U; ++q) {
      unsigned h0, l0, h1, l1;
      split2(xr[q][0], xr[q][1], h0, l0);
      split2(xr[q][2], xr[q][3], h1, l1);
      const u32x2_t hi = {h0, h1}, lo = {l0, l1};
      unsigned char* b = smem_x3d + slot * kSlot + q * kUSlot + kASlot + ((wave >> 1) * kBN + lane) * 16 + (wave & 1) * 8;
      *reinterpret_cast<u32x2_t*>(b) = hi;
      *reinterpret_cast<u32x2_t*>(b + kBN * 32) = lo;
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[am][r] = 0.f;

  issue(0);
  wait_vmcnt<0>();
  store_b(0);
  __syncthreads();

  const int aoff = (lh * kBM + wm * 64 + li) * 16;
  const int boff = kASlot + (lh * kBN + wn * 32 + li) * 16;
  for (int st = 0; st < nstages; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < nstages;
    if (more) issue(cur ^ 1);                    // slot cur ^ 1 was last read before the barrier that ended stage st - 1
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const unsigned char* wa = smem_x3d + cur * kSlot + q * kUSlot + aoff;
      const unsigned char* xa = smem_x3d + cur * kSlot + q * kUSlot + boff;
      u32x4 ah[2], al[2];
#pragma unroll
      for (int am = 0; am < 2; ++am) {
        ah[am] = *reinterpret_cast<const u32x4*>(wa + am * 512);
        al[am] = *reinterpret_cast<const u32x4*>(wa + kBM * 32 + am * 512);
      }
      const u32x4 bh = *reinterpret_cast<const u32x4*>(xa), bl = *reinterpret_cast<const u32x4*>(xa + kBN * 32);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        acc[am] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[am]), __builtin_bit_cast(bf16x8, bl), acc[am], 0, 0, 0);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        acc[am] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al[am]), __builtin_bit_cast(bf16x8, bh), acc[am], 0, 0, 0);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        acc[am] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[am]), __builtin_bit_cast(bf16x8, bh), acc[am], 0, 0, 0);
    }
    if (more) {
      wait_vmcnt<0>();                           // this wave's 2 U weight pieces have landed in LDS, its 4 U input values in registers
      store_b(cur ^ 1);
    }
    __syncthreads();
  }

  // epilogue: bias, leaky ReLU as max(v, slope v) (slope 1: none); 32 x 32 accumulator layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int nn = n0 + wn * 32 + li;
  float bv[2][16];
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[am][r] = p.bias[co0 + (wm * 2 + am) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];     // Co is a multiple of the row tile
  if (nn < N) {
    float* Y = p.Y + ((long long)sig * p.Co + co0 + wm * 64 + 4 * lh) * N + nn;
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[am][r] + bv[am][r];
        Y[(long long)(am * 32 + (r & 3) + 8 * (r >> 2)) * N] = fmaxf(v, v * p.slope);
      }
  }
}
}  // namespace

// pure: no stream, no launch, no allocation.  The geometry has one kernel; what is decided here is whether the layer fits it, and the grid.
bool conv_x3d_plan(const ConvX3dArgs& a, ConvX3dPlan& p) {
  if (a.Ci <= 0 || a.Ci % 16 != 0 || a.Co <= 0 || a.Co % kBM != 0 || a.CoPx != a.Co || !a.bias) return false;
  if (a.k < 1 || a.k > 16 || a.stride < 1 || a.pad < 0 || a.p < 1 || a.S < 1 || a.S > 65535) return false;
  if (a.H < 1 || a.Hout != (a.H + 2 * a.pad - a.k) / a.stride + 1 || a.Hout < 1) return false;
  const long long HP = (long long)a.H * a.p, N = (long long)a.Hout * a.p;
  // 32-bit byte offsets inside one plane (and one row block of tile columns past its end), and inside the weight image
  if ((HP + (long long)a.stride * kBN + (long long)a.k * a.p) * 4 >= (1LL << 31) || (long long)(a.Ci / 16) * a.k * a.CoPx * 64 >= (1LL << 31)) return false;
  const int nunits = (a.Ci / 16) * a.k;
  p.a = a;
  p.units = nunits % 4 == 0 ? 4 : (nunits % 2 == 0 ? 2 : 1);
  p.lds = (size_t)2 * p.units * kUSlot;
  p.grid = dim3((unsigned)((N + kBN - 1) / kBN), (unsigned)(a.CoPx / kBM), (unsigned)a.S);
  p.flops = 2.0 * a.S * (double)N * a.Co * a.Ci * a.k;
  return true;
}
template <int U> static void conv_x3d_launch_u(const ConvX3dPlan& p, hipStream_t s) {
  RVC_ALLOW_BIG_LDS(conv_x3d_kernel<U>);
  hipLaunchKernelGGL(conv_x3d_kernel<U>, p.grid, dim3(256), p.lds, s, p.a);
}
void conv_x3d_launch(const ConvX3dPlan& p, hipStream_t s) {
  if (p.units == 4) conv_x3d_launch_u<4>(p, s);
  else if (p.units == 2) conv_x3d_launch_u<2>(p, s);
  else conv_x3d_launch_u<1>(p, s);
}

}  // namespace rvc
