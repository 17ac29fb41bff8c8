// Data gradient of conv_x3d.hip's strided k = 5 convolution along H (the discriminators' dense layers), as bf16x3 GEMM launches in the same
// layout [S][C][H][p]:  dX[s][c][h][w] = sum_m sum_j W[m][c][j] D[s][m][h'][w] over the (h', j) with stride h' + j - pad = h, then the epilogue
// of the backward chain:  Y = (dX + Cot) * (A > 0 ? 1 : slope)  with Cot (may be null) and A read at the output's own address.
//   rows     c: the forward's INPUT channels, 128 per workgroup (the 32-row gradient into DiscriminatorP's first layer runs with zero rows
//            32 .. 127 of its image: the epilogue stores rows < R only)
//   columns  n = j p + w over the output rows h = ostride j + phase of ONE signal, 64 per workgroup; blockIdx.z = signal; the phases' column
//            tiles lie behind one another in blockIdx.x, so a layer is ONE launch whatever H is (a phase without rows has no tile)
//   K        units of (16-channel chunk of the forward's OUTPUT channels, tap), tap fastest; tap t reads flat element n + (off0 + t) p of the
//            (signal, channel) plane of D through a descriptor of exactly that plane (Hd p floats): a row above 0 or below Hd - 1 reads as zero
// Stride 1 (pad 2) is ONE product of five taps: off0 = -2, tap t carries W[.][.][4 - t].  Stride 3 (pad 2) is THREE products, one per phase
// r = h mod 3, of the rows h = 3 j + r:  r = 0: W[2] D[j];  r = 1: W[3] D[j], W[0] D[j + 1];  r = 2: W[4] D[j], W[1] D[j + 1]  - off0 = 0, one or
// two taps, and the store goes to row 3 j + r (element 3 n - 2 w + r p).  The host regroups the weights per product (discriminator.hip) and
// x3_weight_image makes the image, so the kernel is conv_x3d_kernel's pipeline with another gather and another epilogue.
// The kernel writes the image loop of conv_x3gather_dev.h out: through the shared loop the compiler orders the address arithmetic differently and the input-gradient pass measured 0.6 % slower
// (profiles/x3g_dedup_timing.txt), so it keeps its own copy; the planner and the launcher share the header's arithmetic.
#include "conv_x3gather_dev.h"

namespace rvc {

namespace {
constexpr int kBM = 128, kBN = 64;
constexpr int kASlot = kBM * 64;               // bytes of [hi | lo][half][kBM rows][16 B]
constexpr int kBSlot = kBN * 64;               // bytes of [hi | lo][half][kBN columns][16 B]
constexpr int kUSlot = kASlot + kBSlot;

template <int U>
__global__ __launch_bounds__(256) void conv_x3d_bwd_kernel(const ConvX3dBwdArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_x3b[];      // 2 slots of U units
  constexpr int kSlot = U * kUSlot;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  int ph = 0;                                                                     // the phase whose run of column tiles holds this workgroup
  while (ph + 1 < p.nph && (int)blockIdx.x >= p.tile0[ph + 1]) ++ph;
  const int n0 = ((int)blockIdx.x - p.tile0[ph]) * kBN, r0 = blockIdx.y * kBM, sig = blockIdx.z;
  const int DP = p.Hd * p.p, HP = p.H * p.p, N = p.Hj[ph] * p.p, nt = p.nt[ph];
  const int nunits = (p.Ck >> 4) * nt, nstages = nunits / U;                      // the planner chose U as a divisor of every phase's units

  const __amdgpu_buffer_rsrc_t ars = make_rsrc(p.Wx[ph], (unsigned)nunits * (unsigned)p.RPx * 64u);
  const int avoff = (wave * p.RPx + r0 + lane) * 16;
  const int astep = p.RPx * 64;                                     // bytes of one unit of the image
  // gradient: channels 4 wave .. 4 wave + 3 of the chunk at column n0 + lane
  const int e0 = n0 + lane + p.off0 * p.p;                          // element of tap 0 in the plane (negative: above row 0)
  const float* Dw = p.D + ((long long)sig * p.Ck + wave * 4) * DP;

  float xr[U][4];
  int chunk_n = 0, tap_n = 0, asoff = 0;
  auto issue = [&](int slot) {
#pragma unroll
    for (int q = 0; q < U; ++q) {
      unsigned char* base = smem_x3b + slot * kSlot + q * kUSlot;
      buf_dma(ars, base + wave * (kBM * 16), avoff, asoff);
      buf_dma(ars, base + wave * (kBM * 16) + 1024, avoff + 1024, asoff);
      asoff += astep;
      const unsigned voff = (unsigned)(e0 + tap_n * p.p) * 4u;
      const float* cb = Dw + (long long)chunk_n * 16 * DP;
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[q][i] = buf_load(make_rsrc(cb + (long long)i * DP, (unsigned)DP * 4u), voff);
      if (++tap_n == nt) { tap_n = 0; ++chunk_n; }
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
      unsigned char* b = smem_x3b + slot * kSlot + q * kUSlot + kASlot + ((wave >> 1) * kBN + lane) * 16 + (wave & 1) * 8;
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
    for (int q = 0; q < U; ++q) gather_mfma3_unit<2>(acc, smem_x3b + cur * kSlot + q * kUSlot + aoff, kBM * 32, smem_x3b + cur * kSlot + q * kUSlot + boff, kBN * 32);
    if (more) {
      wait_vmcnt<0>();                           // this wave's 2 U weight pieces have landed in LDS, its 4 U gradient values in registers
      store_b(cur ^ 1);
    }
    __syncthreads();
  }

  // epilogue: column nn of phase ph is element ostride nn - (ostride - 1) w + ph p of the output plane (row ostride j + ph); cotangent, mask.
  const int nn = n0 + wn * 32 + li;
  if (nn < N) {
    const int w = nn % p.p;
    const long long e = (long long)p.ostride * nn - (long long)(p.ostride - 1) * w + (long long)ph * p.p;
    const int row0 = r0 + wm * 64 + acc_row32(0, lh);
    const long long base = ((long long)sig * p.R + row0) * HP + e;
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int dr = am * 32 + acc_row32(r, 0);
        if (row0 + dr < p.R) {
          const long long idx = base + (long long)dr * HP;
          float v = acc[am][r];
          if (p.Cot) v += p.Cot[idx];
          p.Y[idx] = p.A[idx] > 0.f ? v : v * p.slope;
        }
      }
  }
}
}  // namespace

// pure: no stream, no launch, no allocation.  Fills tile0 (the phases' runs of column tiles; a phase without rows has none) and the grid.
bool conv_x3d_bwd_plan(const ConvX3dBwdArgs& a0, ConvX3dBwdPlan& p) {
  ConvX3dBwdArgs a = a0;
  if (a.R <= 0 || a.RPx % kBM != 0 || a.RPx < a.R || a.Ck <= 0 || a.Ck % 16 != 0) return false;
  if (a.p < 1 || a.S < 1 || a.S > 65535 || a.Hd < 1 || a.H < 1 || a.off0 > 0 || a.off0 < -16) return false;
  if (a.ostride < 1 || a.nph != a.ostride || a.nph > 3) return false;                    // one phase per residue of the output row
  const long long DP = (long long)a.Hd * a.p, HP = (long long)a.H * a.p;
  // 32-bit byte offsets inside one plane of D (and one tile of columns and the taps past its end), inside the output plane and inside the images
  if ((DP + HP + kBN + 32LL * a.p) * 4 >= (1LL << 31)) return false;
  int units = 4, tiles = 0;
  p.flops = 0.0;
  for (int ph = 0; ph < a.nph; ++ph) {
    if (!a.Wx[ph] || a.nt[ph] < 1 || a.nt[ph] > 16) return false;
    if ((long long)(a.Ck / 16) * a.nt[ph] * a.RPx * 64 >= (1LL << 31)) return false;
    a.Hj[ph] = a.H > ph ? (a.H - ph + a.ostride - 1) / a.ostride : 0;                    // rows h = ostride j + ph below H
    if (a.Hj[ph] > a.Hd) return false;                                                  // tap 0 of every column lies in the plane of D
    units = std::min(units, gather_units((a.Ck / 16) * a.nt[ph]));
    a.tile0[ph] = tiles;
    tiles += (int)(((long long)a.Hj[ph] * a.p + kBN - 1) / kBN);
    p.flops += 2.0 * a.S * (double)a.Hj[ph] * a.p * a.R * a.Ck * a.nt[ph];
  }
  a.tile0[a.nph] = tiles;
  if (tiles < 1) return false;
  p.a = a;
  p.units = units;
  p.lds = gather_image_lds(kBM, kBN, p.units);
  p.grid = dim3((unsigned)tiles, (unsigned)(a.RPx / kBM), (unsigned)a.S);
  return true;
}
void conv_x3d_bwd_launch(const ConvX3dBwdPlan& p, hipStream_t s) {
  gather_dispatch_units(p.units, [&](auto u) {
    constexpr int U = decltype(u)::value;
    RVC_ALLOW_BIG_LDS(conv_x3d_bwd_kernel<U>);
    hipLaunchKernelGGL(conv_x3d_bwd_kernel<U>, p.grid, dim3(256), p.lds, s, p.a);
  });
}

}  // namespace rvc
