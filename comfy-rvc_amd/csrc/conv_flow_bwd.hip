// The flow's backward data pass (model_synth.hip::flow_backward): the transposed products of a ResidualCouplingLayer - WN's k = 5 in_layers (2 H rows of d a ->
// H), its 1x1 res_skip layers, post and pre - as ONE bf16x3 gather GEMM kernel on the image loop of conv_x3gather_dev.h, and the direct kernels around it (Flip
// and the x1 half, the gate's derivative as a tensor with its float64 row sums, cond_layer transposed, the recording gate of the forward).
//
// conv_flow_bwd_kernel:  Y[r][n] = n < len ? acc[r][n] + Res[r][n] : 0,  acc[r][n] = sum_c sum_t W'[r][c][t] G[c][n + off0 + t], G zero outside [0, Td)
//   rows     r: the forward's INPUT channels, 64 per workgroup
//   columns  n: one item's frames, 64 per workgroup.  An item has a few hundred frames, so the pass is a chain of latency-bound launches: the smallest tile the
//            image loop offers (four waves, one 32 x 32 accumulator each) gives the most workgroups, 15 for 192 rows x 300 frames
//   K        units of (16-channel chunk of the forward's OUTPUT channels, tap), tap fastest; the weight image (gen_bwd_conv_image: transposed, taps flipped) comes
//            by LDS-DMA, the gradient operand is gathered through one descriptor per channel row, split in the kernel and stored to LDS; two slots of U units
// GATED: the operand is WN's gate read backwards.  A wave fetches, per element, d acts[c] and the two taped pre-gate rows a[c], a[H + c] (three loads in flight
// while the previous stage is multiplied) and forms d a[c] or d a[H + c] when the loads have landed, just before the split - as conv_gen_wgrad applies the
// leaky ReLU at its load.  A 16-channel chunk lies in one half of the 2 H rows (H % 16 == 0), so the choice is uniform over the workgroup.
#include "conv_x3gather_dev.h"

namespace rvc {

namespace {
// d acts times the gate's derivative: rows [0, H) of d a take the tanh side, rows [H, 2 H) the sigmoid side
// Both gates through the hardware's exp2 and reciprocal (about 1 ulp each; tanh(x) = 2 sigmoid(2 x) - 1, absolute error about 1e-7): the kernel forms this per
// element, tap and row block, and tanhf / expf with their range branches cost it several times the product itself.
__device__ __forceinline__ float flow_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504f * x)); }
__device__ __forceinline__ float flow_gate_grad(float d, float at, float as, bool sig_side) {
  const float t = 2.f * flow_sigmoid(2.f * at) - 1.f, g = flow_sigmoid(as);
  return sig_side ? d * t * (g * (1.f - g)) : d * g * (1.f - t * t);
}

template <int U, bool GATED>
__global__ __launch_bounds__(256) void conv_flow_bwd_kernel(const ConvFlowBwdArgs p) {
  constexpr int WM = 2, WN = 2, AM = 1, BM = WM * AM * 32, BN = WN * 32, NV = GATED ? 3 : 1;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_fb[];      // 2 slots of U units
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, lh = lane >> 5, wm = wave % WM, wn = wave / WM;
  const int n0 = blockIdx.x * BN, r0 = blockIdx.y * BM;
  const int nunits = (p.Ck >> 4) * p.nt, nstages = nunits / U;                    // the planner chose U as a divisor of the units

  const __amdgpu_buffer_rsrc_t ars = make_rsrc(p.Wx, (unsigned)nunits * (unsigned)p.RPx * 64u);
  const int avoff = (wave * p.RPx + r0 + lane) * 16;                // wave = plane (hi | lo, half) of the unit
  const unsigned dbytes = (unsigned)p.Td * 4u;

  // the closures walk the units in the same order, gather at issue and finish at the store: each keeps its own (chunk, tap)
  int chunk_g = 0, tap_g = 0, chunk_f = 0, tap_f = 0;
  auto gather = [&](int c, float (&raw)[NV][4]) {
    const unsigned voff = (unsigned)(n0 + lane + c * 64 + p.off0 + tap_g) * 4u;      // negative: far beyond the extent
    const int ch = chunk_g * 16 + wave * 4;                          // this wave's first channel of the unit
    if constexpr (GATED) {
      const int r = ch >= p.H ? ch - p.H : ch;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        raw[0][i] = buf_load(make_rsrc(p.D + (long long)(r + i) * p.ldD, dbytes), voff);
        raw[1][i] = buf_load(make_rsrc(p.A + (long long)(r + i) * p.ldD, dbytes), voff);
        raw[2][i] = buf_load(make_rsrc(p.A + (long long)(p.H + r + i) * p.ldD, dbytes), voff);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[0][i] = buf_load(make_rsrc(p.D + (long long)(ch + i) * p.ldD, dbytes), voff);
    }
    if (c == BN / 64 - 1 && ++tap_g == p.nt) { tap_g = 0; ++chunk_g; }
  };
  auto finish = [&](int c, const float (&raw)[NV][4], float (&x)[4]) {
    if constexpr (GATED) {
      const bool sig_side = chunk_f * 16 >= p.H;
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = flow_gate_grad(raw[0][i], raw[1][i], raw[2][i], sig_side);      // out of range: d acts reads as zero
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = raw[0][i];
    }
    if (c == BN / 64 - 1 && ++tap_f == p.nt) { tap_f = 0; ++chunk_f; }
  };

  f32x16 acc[AM];
  gather_image_loop_act<BM, BN, AM, U, NV>(smem_fb, ars, avoff, p.RPx * 64, nstages, wave, lane, wm, wn, acc, gather, finish);

  // the epilogue adds the running x-chain cotangent (or x0's) and applies the item's mask
  const int nn = n0 + wn * 32 + li;
  if (nn < p.N) {
    const bool live = nn < p.len;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + wm * 32 + acc_row32(r, lh);
      if (row < p.R) {
        const long long idx = (long long)row * p.ldY + nn;
        float v = acc[0][r];
        if (p.Res) v += p.Res[idx];
        p.Y[idx] = live ? v : 0.f;
      }
    }
  }
}

template <bool GATED> void flow_bwd_launch_u(const ConvFlowBwdPlan& p, hipStream_t s) {
  gather_dispatch_units(p.units, [&](auto u) {
    constexpr int U = decltype(u)::value;
    RVC_ALLOW_BIG_LDS((conv_flow_bwd_kernel<U, GATED>));
    hipLaunchKernelGGL((conv_flow_bwd_kernel<U, GATED>), p.grid, dim3(256), p.lds, s, p.a);
  });
}
}  // namespace

// pure: no stream, no launch, no allocation
bool conv_flow_bwd_plan(const ConvFlowBwdArgs& a, ConvFlowBwdPlan& p) {
  if (!a.D || !a.Wx || !a.Y || a.R <= 0 || a.RPx % 128 != 0 || a.RPx < a.R || a.Ck <= 0 || a.Ck % 16 != 0) return false;
  if (a.N < 1 || a.Td < 1 || a.ldD < a.Td || a.ldY < a.N || a.nt < 1 || a.nt > 16 || a.off0 > 0 || a.off0 < -4096 || a.len < 0 || a.len > a.N) return false;
  if (a.A && (a.H < 16 || a.H % 16 != 0 || a.Ck != 2 * a.H)) return false;
  // 32-bit byte offsets: the furthest element a column of the last tile reads, the image
  const long long ncols = ((long long)a.N + 63) / 64 * 64;
  if ((ncols + a.nt) * 4 >= (1LL << 31) || (long long)a.Td * 4 >= (1LL << 31)) return false;
  const long long nunits = (long long)(a.Ck / 16) * a.nt;
  if (nunits * a.RPx * 64 >= (1LL << 31)) return false;
  p.a = a;
  p.units = gather_units(nunits);
  p.lds = gather_image_lds(64, 64, p.units);
  p.grid = dim3((unsigned)(ncols / 64), (unsigned)((a.R + 63) / 64), 1);
  return true;
}
void conv_flow_bwd_launch(const ConvFlowBwdPlan& p, hipStream_t s) {
  if (p.a.A) flow_bwd_launch_u<true>(p, s); else flow_bwd_launch_u<false>(p, s);
}

// ------------------------------------------------------------------------------------------------ the direct kernels
namespace {
__global__ void flow_unflip_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ dm, int C, int T, int len) {
  const long long n = (long long)C * T;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i / T), t = (int)(i - (long long)c * T);
  const float v = t < len ? x[(long long)(C - 1 - c) * T + t] : 0.f;
  y[i] = v;
  if (c >= C / 2) dm[(long long)(c - C / 2) * T + t] = v;
}
// one workgroup per row of d a: each thread its strided share in index order, the float64 partials added by the tree
__global__ __launch_bounds__(256) void flow_gate_bwd_kernel(const float* __restrict__ dacts, const float* __restrict__ a, float* __restrict__ da, float* __restrict__ dgc,
                                                            int H, int T, int len) {
  __shared__ double part[256];
  const int row = blockIdx.x, c = row >= H ? row - H : row;
  const float* d = dacts + (long long)c * T;
  const float* at = a + (long long)c * T;
  const float* as = a + (long long)(H + c) * T;
  float* o = da + (long long)row * T;
  double acc = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) {
    const float v = t < len ? flow_gate_grad(d[t], at[t], as[t], row >= H) : 0.f;
    o[t] = v;
    acc += (double)v;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) dgc[row] = (float)part[0];
}
struct FlowCondArgs { const float* W[4]; const float* dgc[4]; };
// 64 columns g x 16 row slices per workgroup: slice q sums its quarter of coupling q / 4's rows in index order, thread q = 0 adds the 16 partials in slice order
__global__ __launch_bounds__(1024) void flow_cond_bwd_kernel(const FlowCondArgs p, int C, int G, float* out, float* out2) {
  __shared__ double part[16][64];
  const int gi = threadIdx.x & 63, q = threadIdx.x >> 6, g = blockIdx.x * 64 + gi;
  const int f = q >> 2, per = (C + 3) / 4, c0 = (q & 3) * per, c1 = min(C, c0 + per);
  double acc = 0.0;
  if (g < G)
    for (int c = c0; c < c1; ++c) acc += (double)p.W[f][(long long)c * G + g] * (double)p.dgc[f][c];
  part[q][gi] = acc;
  __syncthreads();
  if (q == 0 && g < G) {
    for (int k = 1; k < 16; ++k) acc += part[k][gi];
    out[g] = (float)acc; if (out2) out2[g] = (float)acc;
  }
}
// ops.hip's wn_gate_kernel / wn_gate_split_kernel with the summed pre-gate activation stored back: one thread = 8 channels of one frame
__global__ __launch_bounds__(256) void wn_gate_record_kernel(float* __restrict__ a, const float* __restrict__ g, float* __restrict__ out, unsigned char* __restrict__ img,
                                                             long long tp, int margin, int H, int T) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int grp = blockIdx.y;
  if (t >= T) return;
  const long long n = (long long)H * T;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = grp * 8 + j;
    if (c >= H) { v[j] = 0.f; continue; }
    const long long i = (long long)c * T + t;
    const float ta = a[i] + g[c], sa = a[i + n] + g[c + H];
    a[i] = ta; a[i + n] = sa;
    v[j] = tanhf(ta) * (1.f / (1.f + expf(-sa)));
    if (out) out[i] = v[j];
  }
  if (!img) return;
  u32x4 hi, lo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const __bf16 ah = (__bf16)v[2 * j], bh = (__bf16)v[2 * j + 1];
    const __bf16 al = (__bf16)(v[2 * j] - (float)ah), bl = (__bf16)(v[2 * j + 1] - (float)bh);
    hi[j] = bf16_bits(ah) | (bf16_bits(bh) << 16);
    lo[j] = bf16_bits(al) | (bf16_bits(bl) << 16);
  }
  unsigned char* row = img + (((long long)(grp >> 1) * 4 + (grp & 1)) * tp + margin + t) * 16;
  *reinterpret_cast<u32x4*>(row) = hi;
  *reinterpret_cast<u32x4*>(row + tp * 32) = lo;
}
}  // namespace

void flow_unflip(hipStream_t s, const float* x, float* y, float* dm, int C, int T, int len) {
  const long long n = (long long)C * T;
  hipLaunchKernelGGL(flow_unflip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, dm, C, T, len);
}
void flow_gate_bwd(hipStream_t s, const float* dacts, const float* a, float* da, float* dgc, int H, int T, int len) {
  hipLaunchKernelGGL(flow_gate_bwd_kernel, dim3((unsigned)(2 * H)), dim3(256), 0, s, dacts, a, da, dgc, H, T, len);
}
void flow_cond_bwd(hipStream_t s, const float* const (&W)[4], const float* const (&dgc)[4], int C, int G, float* out, float* out2) {
  FlowCondArgs p;
  for (int f = 0; f < 4; ++f) { p.W[f] = W[f]; p.dgc[f] = dgc[f]; }
  hipLaunchKernelGGL(flow_cond_bwd_kernel, dim3((unsigned)((G + 63) / 64)), dim3(1024), 0, s, p, C, G, out, out2);
}
void wn_gate_record(hipStream_t s, float* a, const float* g, float* out, unsigned char* img, long long tp, int margin, int H, int T) {
  RVC_REQUIRE(!img || (H & 15) == 0, "wn_gate_record: hidden channels must be a multiple of 16 for the split image");
  hipLaunchKernelGGL(wn_gate_record_kernel, dim3((T + 255) / 256, (H + 7) / 8), dim3(256), 0, s, a, g, out, img, tp, margin, H, T);
}

}  // namespace rvc
