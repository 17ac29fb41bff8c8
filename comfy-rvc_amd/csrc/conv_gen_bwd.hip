// The generator's backward data pass (model_synth.hip::synth_dec_input_grad): the data gradient of its 1-D convolutions as ONE bf16x3 GEMM kernel, and the
// few direct kernels around it (tanh / conv_post, the noise branch, the conditioning's row sums).
//
// conv_gen_bwd_kernel:  Y[r][n] = acc[r][n] * (A[r][n] > 0 ? scale : scale * slope) + R[r][n] (+ Y[r][n]),  acc[r][n] = sum_c sum_t W'[r][c][t] D[c][e(n, t)]
// with e(n, t) = cstride n + off0 + tstep t and zero outside [0, Td):
//   rows     r: the forward's INPUT channels; WM * AM * 32 per workgroup (128, 64 or 32: a 16- or 32-channel stage runs the 32-row tile over 128 columns)
//   columns  n: the positions of the forward's input, (4 / WM) * 32 per workgroup
//   K        units of (16-channel chunk of the forward's OUTPUT channels, tap), tap fastest; the weight image (x3_weight_image of W', rows padded to RPx) comes by
//            LDS-DMA, the gradient operand is gathered through one descriptor per channel row (out of range reads as zero), split in the kernel and stored to LDS;
//            two slots of U units
// A stride-1 dilated Conv1d(C, C, k) is cstride 1, tstep dil, off0 = pad - (k - 1) dil over the transposed, tap-flipped image W'[ci][co][t] = W[co][ci][k - 1 - t];
// a ConvTranspose1d(Cin, Cout, k, u, pad) is cstride u, tstep 1, off0 = -pad over its own weight [ci][co][t].  A: the recorded pre-activation (null: no mask),
// R: the residual cotangent (null: none), accumulate: the output's previous value is added last (the three ResBlocks' sum, in launch order).
// The kernel writes the image loop of conv_x3gather_dev.h out: through the shared loop the compiler orders the address arithmetic differently and the 32-channel stage of the decoder's backward pass measured 1.2 % slower
// (profiles/x3g_dedup_timing.txt), so it keeps its own copy; the planner and the launcher share the header's arithmetic.
#include "conv_x3gather_dev.h"

namespace rvc {

namespace {
template <int WM, int AM, int U>
__global__ __launch_bounds__(256) void conv_gen_bwd_kernel(const ConvGenBwdArgs p) {
  constexpr int WN = 4 / WM, BM = WM * AM * 32, BN = WN * 32, AR = BM < 64 ? 64 : BM, CN = BN / 64;
  constexpr int kASlot = AR * 64;              // bytes of [hi | lo][half][AR rows][16 B]
  constexpr int kBSlot = BN * 64;              // bytes of [hi | lo][half][BN columns][16 B]
  constexpr int kUSlot = kASlot + kBSlot, kSlot = U * kUSlot;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_gb[];      // 2 slots of U units
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave % WM, wn = wave / WM;
  const int n0 = blockIdx.x * BN, r0 = blockIdx.y * BM;
  const int nunits = (p.Ck >> 4) * p.nt, nstages = nunits / U;                    // the planner chose U as a divisor of the units

  const __amdgpu_buffer_rsrc_t ars = make_rsrc(p.Wx, (unsigned)nunits * (unsigned)p.RPx * 64u);
  const int avoff = (wave * p.RPx + r0 + lane) * 16;                // wave = plane (hi | lo, half) of the unit
  const int astep = p.RPx * 64;                                     // bytes of one unit of the image
  // gradient: channels 4 wave .. 4 wave + 3 of the chunk at columns n0 + lane (+ 64)
  const float* Dw = p.D + (long long)(wave * 4) * p.ldD;
  const unsigned dbytes = (unsigned)p.Td * 4u;

  float xr[U][CN][4];
  int chunk_n = 0, tap_n = 0, asoff = 0;
  auto issue = [&](int slot) {
#pragma unroll
    for (int q = 0; q < U; ++q) {
      unsigned char* base = smem_gb + slot * kSlot + q * kUSlot;
#pragma unroll
      for (int h = 0; h < AR / 64; ++h) buf_dma(ars, base + wave * (AR * 16) + h * 1024, avoff + h * 1024, asoff);
      asoff += astep;
      const float* cb = Dw + (long long)chunk_n * 16 * p.ldD;
#pragma unroll
      for (int c = 0; c < CN; ++c) {
        const unsigned voff = (unsigned)((n0 + lane + c * 64) * p.cstride + p.off0 + tap_n * p.tstep) * 4u;      // negative: far beyond the extent
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[q][c][i] = buf_load(make_rsrc(cb + (long long)i * p.ldD, dbytes), voff);
      }
      if (++tap_n == p.nt) { tap_n = 0; ++chunk_n; }
    }
  };
  auto store_b = [&](int slot) {
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < U; ++q)
#pragma unroll
      for (int c = 0; c < CN; ++c) {
        unsigned h0, l0, h1, l1;
        split2(xr[q][c][0], xr[q][c][1], h0, l0);
        split2(xr[q][c][2], xr[q][c][3], h1, l1);
        const u32x2_t hi = {h0, h1}, lo = {l0, l1};
        unsigned char* b = smem_gb + slot * kSlot + q * kUSlot + kASlot + ((wave >> 1) * BN + c * 64 + lane) * 16 + (wave & 1) * 8;
        *reinterpret_cast<u32x2_t*>(b) = hi;
        *reinterpret_cast<u32x2_t*>(b + BN * 32) = lo;
      }
  };

  f32x16 acc[AM];
#pragma unroll
  for (int am = 0; am < AM; ++am)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[am][r] = 0.f;

  issue(0);
  wait_vmcnt<0>();
  store_b(0);
  __syncthreads();

  const int aoff = (lh * AR + wm * (AM * 32) + li) * 16;
  const int boff = kASlot + (lh * BN + wn * 32 + li) * 16;
  for (int st = 0; st < nstages; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < nstages;
    if (more) issue(cur ^ 1);                    // slot cur ^ 1 was last read before the barrier that ended stage st - 1
#pragma unroll
    for (int q = 0; q < U; ++q) gather_mfma3_unit<AM>(acc, smem_gb + cur * kSlot + q * kUSlot + aoff, AR * 32, smem_gb + cur * kSlot + q * kUSlot + boff, BN * 32);
    if (more) {
      wait_vmcnt<0>();                           // this wave's weight pieces have landed in LDS, its gradient values in registers
      store_b(cur ^ 1);
    }
    __syncthreads();
  }

  const int nn = n0 + wn * 32 + li;
  if (nn < p.N) {
    const int row0 = r0 + wm * (AM * 32) + 4 * lh;
    const float s1 = p.scale, s0 = p.scale * p.slope;
#pragma unroll
    for (int am = 0; am < AM; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + am * 32 + (r & 3) + 8 * (r >> 2);      // acc_row32(r, 0) written out: with the helper's parentheses the compiler folds the sum another way and the kernel changes
        if (row < p.R) {
          const long long idx = (long long)row * p.ldY + nn;
          float v = acc[am][r];
          v *= (!p.A || p.A[idx] > 0.f) ? s1 : s0;
          if (p.Res) v += p.Res[idx];
          if (p.accumulate) v += p.Y[idx];
          p.Y[idx] = v;
        }
      }
  }
}

template <int WM, int AM> void gen_bwd_launch_u(const ConvGenBwdPlan& p, hipStream_t s) {
  gather_dispatch_units(p.units, [&](auto u) {
    constexpr int U = decltype(u)::value;
    RVC_ALLOW_BIG_LDS((conv_gen_bwd_kernel<WM, AM, U>));
    hipLaunchKernelGGL((conv_gen_bwd_kernel<WM, AM, U>), p.grid, dim3(256), p.lds, s, p.a);
  });
}
}  // namespace

// pure: no stream, no launch, no allocation.  The tile follows the rows: 128 where they fill it, 64 otherwise, 32 rows x 128 columns for the 16- / 32-channel stages
bool conv_gen_bwd_plan(const ConvGenBwdArgs& a, ConvGenBwdPlan& p) {
  if (!a.D || !a.Wx || !a.Y || a.R <= 0 || a.RPx % 128 != 0 || a.RPx < a.R || a.Ck <= 0 || a.Ck % 16 != 0) return false;
  if (a.N < 1 || a.Td < 1 || a.ldD < a.Td || a.ldY < a.N || a.nt < 1 || a.nt > 16 || a.cstride < 1 || a.tstep < 1 || a.off0 > 0 || a.off0 < -4096) return false;
  const int bm = a.R <= 32 ? 32 : (a.R % 128 == 0 ? 128 : 64), bn = bm == 32 ? 128 : 64;
  // 32-bit byte offsets: the furthest element a column of the last tile reads, the output plane, the image
  const long long ncols = ((long long)a.N + bn - 1) / bn * bn;
  if ((ncols * a.cstride + (long long)a.nt * a.tstep) * 4 >= (1LL << 31) || (long long)a.Td * 4 >= (1LL << 31)) return false;
  const long long nunits = (long long)(a.Ck / 16) * a.nt;
  if (nunits * a.RPx * 64 >= (1LL << 31)) return false;
  p.a = a;
  p.bm = bm;
  p.units = gather_units(nunits);
  p.lds = gather_image_lds(std::max(bm, 64), bn, p.units);
  p.grid = dim3((unsigned)(ncols / bn), (unsigned)((a.R + bm - 1) / bm), 1);
  p.flops = 2.0 * a.N * a.R * a.Ck * a.nt;
  return true;
}
void conv_gen_bwd_launch(const ConvGenBwdPlan& p, hipStream_t s) {
  if (p.bm == 128) gen_bwd_launch_u<2, 2>(p, s);
  else if (p.bm == 64) gen_bwd_launch_u<2, 1>(p, s);
  else gen_bwd_launch_u<1, 1>(p, s);
}

// ------------------------------------------------------------------------------------------------ the direct kernels
namespace {
// d[n] = dy[n] (1 - y[n]^2): the cotangent at conv_post's output
__global__ void gen_tanh_bwd_kernel(const float* dy, const float* y, float* d, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const float v = y[i]; d[i] = dy[i] * (1.f - v * v); }
}
// conv_post (C -> 1, k taps, no bias) transposed, times the mask of its input at `slope`, times scale:  dx[c][t] = scale m(x[c][t]) sum_j w[c][j] d[t + pad - j]
__global__ void gen_post_bwd_kernel(const float* d, const float* w, const float* x, float* dx, int k, int pad, long long T, float slope, float scale) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (t >= T) return;
  float acc = 0.f;
  for (int j = 0; j < k; ++j) {
    const long long q = t + pad - j;
    if (q >= 0 && q < T) acc = fmaf(w[c * k + j], d[q], acc);
  }
  const long long idx = (long long)c * T + t;
  dx[idx] = acc * (x[idx] > 0.f ? scale : scale * slope);
}
// the noise convolution Conv1d(1, C, k, stride s, pad) transposed onto the harmonic source:  dhar[n] (+)= sum_c sum_j w[c][j] D[c][(n + pad - j) / s] over the
// taps j = (n + pad) mod s, + s, .. for which the position lies in [0, T); out2 (or null): a second copy of the running sum
__global__ void gen_noise_bwd_kernel(const float* D, const float* w, float* dhar, float* out2, int C, int k, int s, int pad, long long T, long long N, int accumulate) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  const int j0 = (int)((n + pad) % s);
  for (int c = 0; c < C; ++c)
    for (int j = j0; j < k; j += s) {
      const long long t = (n + pad - j) / s;
      if (n + pad - j >= 0 && t < T) acc = fmaf(w[c * k + j], D[(long long)c * T + t], acc);
    }
  const float v = accumulate ? dhar[n] + acc : acc;
  dhar[n] = v; if (out2) out2[n] = v;
}
// out[c] = sum_t D[c][t] in float64: one workgroup per row, each thread its strided share in index order, then the tree over the 256 partials
__global__ __launch_bounds__(256) void gen_row_sums_kernel(const float* D, long long T, float* out, float* out2) {
  __shared__ double part[256];
  const float* row = D + (long long)blockIdx.x * T;
  double a = 0.0;
  for (long long t = threadIdx.x; t < T; t += 256) a += (double)row[t];
  part[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[blockIdx.x] = (float)part[0]; if (out2) out2[blockIdx.x] = (float)part[0]; }
}
// dg[g] = sum_c W[c][g] dcond[c] in float64, c in index order
__global__ void gen_cond_bwd_kernel(const float* W, const float* dcond, int C, int G, float* out, float* out2) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double a = 0.0;
  for (int c = 0; c < C; ++c) a += (double)W[(long long)c * G + g] * (double)dcond[c];
  out[g] = (float)a; if (out2) out2[g] = (float)a;
}
}  // namespace

void gen_tanh_bwd(hipStream_t s, const float* dy, const float* y, float* d, long long n) {
  hipLaunchKernelGGL(gen_tanh_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, y, d, n);
}
void gen_post_bwd(hipStream_t s, const float* d, const float* w, const float* x, float* dx, int C, int k, int pad, long long T, float slope, float scale) {
  hipLaunchKernelGGL(gen_post_bwd_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)C), dim3(256), 0, s, d, w, x, dx, k, pad, T, slope, scale);
}
void gen_noise_bwd(hipStream_t s, const float* D, const float* w, float* dhar, float* out2, int C, int k, int stride, int pad, long long T, long long N, int accumulate) {
  hipLaunchKernelGGL(gen_noise_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, D, w, dhar, out2, C, k, stride, pad, T, N, accumulate);
}
void gen_row_sums(hipStream_t s, const float* D, int C, long long T, float* out, float* out2) {
  hipLaunchKernelGGL(gen_row_sums_kernel, dim3((unsigned)C), dim3(256), 0, s, D, T, out, out2);
}
void gen_cond_bwd(hipStream_t s, const float* W, const float* dcond, int C, int G, float* out, float* out2) {
  hipLaunchKernelGGL(gen_cond_bwd_kernel, dim3((unsigned)((G + 63) / 64)), dim3(64), 0, s, W, dcond, C, G, out, out2);
}

}  // namespace rvc
