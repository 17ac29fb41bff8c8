// Strided k-tap convolution along H over a batch of [Ci][H][p] tensors as ONE bf16x3 GEMM launch (the discriminators of the trainer:
// reference lib/infer_pack/models.py:1111-1145 DiscriminatorP's Conv2d((5, 1), stride (3, 1)) layers, and with p = 1 DiscriminatorS's dense
// Conv1d(1024, 1024, 5), :1093).  Y[s][m][h'][w] = lrelu(b[m] + sum_c sum_j W[m][c][j] X[s][c][stride h' + j - pad][w]).
//   rows     m: output channels, 128 per workgroup (4 waves as 2 x 2, each 64 rows x 32 columns = two 32 x 32 accumulators)
//   columns  n = h' p + w of ONE signal, 64 per workgroup; blockIdx.z = signal, so one launch covers every signal and every column of the
//            period and the weight image is streamed once per layer (the column tiles of all signals share it through L2)
//   K        units of (16-channel chunk, tap), tap fastest: the image loop of conv_x3gather_dev.h over the image conv1d's bf16x3 layers use
//            ([chunk][tap][hi | lo][half][CoPx rows][8 ch])
// Input and output stay in the reference's layout [S][C][H][p]: the post-activation output is the feature map the caller gets AND the next
// layer's input - nothing is transposed or copied.  im2col by address: column n, tap j reads flat element stride n - (stride - 1) w +
// (j - pad) p of the (signal, channel) plane through a buffer descriptor of exactly that plane (H p floats), so a tap above row 0 or below
// row H - 1 is out of the descriptor's range and reads as zero (conv_kernels.h, kOOB) - no branch, and no tap can reach another channel's
// or another signal's rows.
#include "conv_x3gather_dev.h"

namespace rvc {

namespace {
constexpr int kBM = 128, kBN = 64;

template <int U>
__global__ __launch_bounds__(256) void conv_x3d_kernel(const ConvX3dArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_x3d[];      // 2 slots of U units
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int n0 = blockIdx.x * kBN, co0 = blockIdx.y * kBM, sig = blockIdx.z;
  const int HP = p.H * p.p, N = p.Hout * p.p;
  const int nunits = (p.Ci >> 4) * p.k, nstages = nunits / U;                     // the planner chose U as a divisor of the units

  const __amdgpu_buffer_rsrc_t ars = make_rsrc(p.Wx, (unsigned)nunits * (unsigned)p.CoPx * 64u);
  const int avoff = (wave * p.CoPx + co0 + lane) * 16;
  const int astep = p.CoPx * 64;                                    // bytes of one unit of the image
  // input: channels 4 wave .. 4 wave + 3 of the chunk at column n0 + lane
  const int n = n0 + lane;
  const int w = n % p.p;
  const int e0 = p.stride * n - (p.stride - 1) * w - p.pad * p.p;   // element of tap 0 in the plane (negative: above row 0)
  const float* Xw = p.X + ((long long)sig * p.Ci + wave * 4) * HP;

  int chunk_n = 0, tap_n = 0;                                       // (chunk, tap) of the next unit to be gathered
  auto gather = [&](int, float (&x)[4]) {
    const unsigned voff = (unsigned)(e0 + tap_n * p.p) * 4u;
    const float* cb = Xw + (long long)chunk_n * 16 * HP;
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = buf_load(make_rsrc(cb + (long long)i * HP, (unsigned)HP * 4u), voff);
    if (++tap_n == p.k) { tap_n = 0; ++chunk_n; }
  };
  f32x16 acc[2];
  gather_image_loop<kBM, kBN, 2, U>(smem_x3d, ars, avoff, astep, nstages, wave, lane, wm, wn, acc, gather);

  // epilogue: bias, leaky ReLU as max(v, slope v) (slope 1: none)
  const int nn = n0 + wn * 32 + li;
  float bv[2][16];
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[am][r] = p.bias[co0 + (wm * 2 + am) * 32 + acc_row32(r, lh)];     // Co is a multiple of the row tile
  if (nn < N) {
    float* Y = p.Y + ((long long)sig * p.Co + co0 + wm * 64 + acc_row32(0, lh)) * N + nn;
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[am][r] + bv[am][r];
        Y[(long long)(am * 32 + acc_row32(r, 0)) * N] = fmaxf(v, v * p.slope);
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
  p.a = a;
  p.units = gather_units((a.Ci / 16) * a.k);
  p.lds = gather_image_lds(kBM, kBN, p.units);
  p.grid = dim3((unsigned)((N + kBN - 1) / kBN), (unsigned)(a.CoPx / kBM), (unsigned)a.S);
  p.flops = 2.0 * a.S * (double)N * a.Co * a.Ci * a.k;
  return true;
}
void conv_x3d_launch(const ConvX3dPlan& p, hipStream_t s) {
  gather_dispatch_units(p.units, [&](auto u) {
    constexpr int U = decltype(u)::value;
    RVC_ALLOW_BIG_LDS(conv_x3d_kernel<U>);
    hipLaunchKernelGGL(conv_x3d_kernel<U>, p.grid, dim3(256), p.lds, s, p.a);
  });
}

}  // namespace rvc
