// The optimizer step on the device: torch.optim.AdamW (amsgrad off, maximize off) per element in float32, and the discriminators' step built on it
// (reference training_cli.py:562-563: clip_grad_value_, optim_d.step()), which then re-derives on the same stream what the three passes read - the folded
// fp32 weights of the VALU layers and the bf16x3 images of the dense k = 5 layers - bit for bit as disc_finalize builds them on the host.
//   launch 1  disc_adamw_kernel   every parameter tensor, driven by a chunk table in device memory (165 tensors exceed a kernel-argument table)
//   launch 2  disc_fold_kernel    weight norm: sc[co] = (float)(g / sqrt(sum v^2)), the sum in float64 in the host's order (sequential along the row), and
//                                 w = v * sc of the VALU layers.  Not launched for a plain-weight net
//   launch 3  disc_image_kernel   the dense layers: a tile of 16 output channels x (a slab of <= 64 input channels) x 5 taps of w = v * sc through LDS, written
//                                 as whole 16-byte pieces of the forward image and of the transposed phase images.  Zero padding rows are never touched
// Every multiply and add of the update is its own rounding, sqrtf and the divisions are IEEE: the file is compiled with contraction off (the pragma below; the
// _rn intrinsics of the HIP headers are plain operators compiled with contraction allowed, so a product and a sum written with them still fuse).
// No atomics and a fixed order everywhere: two steps from the same state give the same bits.
#include "disc_model.h"

#pragma clang fp contract(off)

namespace rvc {

// ---------------------------------------------------------------------------------------------- AdamW
struct AdamwK { float decay, omb1, beta2, omb2, step_size, sbc2, eps, clip; int has_clip; };   // 1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2)
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamwK& k) {
  if (k.has_clip) g = g < -k.clip ? -k.clip : (g > k.clip ? k.clip : g);      // clamp on read (a NaN stays a NaN, as torch's clamp_)
  p = p * k.decay;
  m = m + (g - m) * k.omb1;
  v = v * k.beta2 + k.omb2 * (g * g);
  const float denom = sqrtf(v) / k.sbc2 + k.eps;
  p = p - k.step_size * (m / denom);
}
// n elements by the threads of one workgroup.  Where the four pointers share their offset from 16-byte alignment: scalar head, float4 body, scalar tail;
// otherwise one element per thread and pass (coalesced dwords).  g is only read.
__device__ __forceinline__ void adamw_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n,
                                           const AdamwK& k) {
  const unsigned a = (unsigned)((uintptr_t)p & 15);
  const bool same = ((uintptr_t)g & 15) == a && ((uintptr_t)m & 15) == a && ((uintptr_t)v & 15) == a;
  long long head = same ? min(n, (long long)(((16 - a) & 15) >> 2)) : n, nvec = (n - head) >> 2;
  for (long long i = threadIdx.x; i < head; i += blockDim.x) adamw_elem(p[i], g[i], m[i], v[i], k);
  float4* p4 = reinterpret_cast<float4*>(p + head); const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = reinterpret_cast<float4*>(m + head); float4* v4 = reinterpret_cast<float4*>(v + head);
  for (long long i = threadIdx.x; i < nvec; i += blockDim.x) {
    float4 pp = p4[i], mm = m4[i], vv = v4[i]; const float4 gg = g4[i];
    adamw_elem(pp.x, gg.x, mm.x, vv.x, k); adamw_elem(pp.y, gg.y, mm.y, vv.y, k); adamw_elem(pp.z, gg.z, mm.z, vv.z, k); adamw_elem(pp.w, gg.w, mm.w, vv.w, k);
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
  }
  for (long long i = head + 4 * nvec + threadIdx.x; i < n; i += blockDim.x) adamw_elem(p[i], g[i], m[i], v[i], k);
}

constexpr int kAdamwMax = 64;
struct AdamwSegs { float* p[kAdamwMax]; const float* g[kAdamwMax]; float* m[kAdamwMax]; float* v[kAdamwMax]; long long n[kAdamwMax]; };
// grid (x, K): workgroup x of tensor k owns one contiguous run of it (a multiple of 4 long, so the runs keep the tensor's alignment)
__global__ __launch_bounds__(256) void adamw_kernel(const AdamwSegs s, const AdamwK k) {
  const int t = blockIdx.y;
  const long long n = s.n[t], per = (((n + gridDim.x - 1) / gridDim.x) + 3) & ~3LL, b0 = (long long)blockIdx.x * per;
  if (b0 >= n) return;
  adamw_span(s.p[t] + b0, s.g[t] + b0, s.m[t] + b0, s.v[t] + b0, min(per, n - b0), k);
}

static AdamwK adamw_scalars(const rvc_adamw_hyper& h) {
  RVC_REQUIRE(h.step >= 1, "adamw: step is the step being taken, >= 1");
  RVC_REQUIRE(std::isfinite(h.lr) && h.lr >= 0.0 && h.beta1 >= 0.0 && h.beta1 < 1.0 && h.beta2 >= 0.0 && h.beta2 < 1.0 && h.eps >= 0.0 && h.weight_decay >= 0.0,
              "adamw: lr >= 0, 0 <= beta < 1, eps >= 0, weight_decay >= 0");
  RVC_REQUIRE(!h.has_clip || h.clip_value >= 0.0, "adamw: clip_value >= 0");
  const double bc1 = 1.0 - std::pow(h.beta1, (double)h.step), bc2 = 1.0 - std::pow(h.beta2, (double)h.step);
  AdamwK k;
  k.decay = (float)(1.0 - h.lr * h.weight_decay); k.omb1 = (float)(1.0 - h.beta1); k.beta2 = (float)h.beta2; k.omb2 = (float)(1.0 - h.beta2);
  k.step_size = (float)(h.lr / bc1); k.sbc2 = (float)std::sqrt(bc2); k.eps = (float)h.eps;
  k.has_clip = h.has_clip ? 1 : 0; k.clip = h.has_clip ? (float)h.clip_value : 0.f;
  return k;
}

void adamw_step(hipStream_t s, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* n, int K, const rvc_adamw_hyper& h) {
  RVC_REQUIRE(p && g && m && v && n && K >= 1 && K <= kAdamwMax, "adamw_step: 1 <= K <= 64 tensors");
  const AdamwK k = adamw_scalars(h);
  AdamwSegs segs{};
  long long longest = 0;
  for (int i = 0; i < K; ++i) {
    RVC_REQUIRE(p[i] && g[i] && m[i] && v[i] && n[i] > 0, "adamw_step: empty tensor");
    RVC_REQUIRE((((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 3) == 0, "adamw_step: pointers must be 4-byte aligned");
    segs.p[i] = p[i]; segs.g[i] = g[i]; segs.m[i] = m[i]; segs.v[i] = v[i]; segs.n[i] = n[i];
    longest = std::max(longest, n[i]);
  }
  const unsigned blocks = (unsigned)std::min<long long>((longest + 4095) / 4096, 1024);
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks, (unsigned)K), dim3(256), 0, s, segs, k);
}

// ---------------------------------------------------------------------------------------------- the discriminators' step
constexpr int kChunk = 8192;                                    // elements of one workgroup of the update
struct AdamwChunk { float* p; long long off; int n; int pad; };  // n elements of a parameter tensor at p; off: their place in the flat buffers
__global__ __launch_bounds__(256) void disc_adamw_kernel(const AdamwChunk* __restrict__ tab, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const AdamwK k) {
  const AdamwChunk c = tab[blockIdx.x];
  adamw_span(c.p, g + c.off, m + c.off, v + c.off, c.n, k);
}

// Weight norm (dim 0) of up to kFoldRows rows of one layer, weight_norm0 of model_common.h restated: thread r owns row r and adds its squares in float64 in
// index order (the host's order: a square of a float is exact in float64, so only the order of the additions matters); the rows reach it through LDS tiles
// that the whole workgroup loads with coalesced reads.  w (VALU layers; null for the GEMM layers, whose images disc_image_kernel writes) = v * sc.
constexpr int kFoldRows = 64, kFoldCols = 64;
struct FoldBlock { const float* v; const float* g; float* sc; float* w; int rows, L; };    // pointers at the block's first row
__global__ __launch_bounds__(256) void disc_fold_kernel(const FoldBlock* __restrict__ tab) {
  __shared__ float tile[kFoldRows][kFoldCols + 1];
  __shared__ float scs[kFoldRows];
  const FoldBlock b = tab[blockIdx.x];
  double s = 0.0;
  for (int c0 = 0; c0 < b.L; c0 += kFoldCols) {
    const int nc = min(kFoldCols, b.L - c0);
    for (int i = threadIdx.x; i < kFoldRows * kFoldCols; i += 256) {
      const int r = i / kFoldCols, c = i - r * kFoldCols;
      tile[r][c] = (r < b.rows && c < nc) ? b.v[(long long)r * b.L + c0 + c] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < kFoldRows)
      for (int c = 0; c < nc; ++c) { const double x = (double)tile[threadIdx.x][c]; s += x * x; }
    __syncthreads();
  }
  if (threadIdx.x < b.rows) {
    const float sc = (float)((double)b.g[threadIdx.x] / sqrt(s));
    b.sc[threadIdx.x] = sc; scs[threadIdx.x] = sc;
  }
  __syncthreads();
  if (b.w)
    for (int i = threadIdx.x; i < b.rows * b.L; i += 256) b.w[i] = b.v[i] * scs[i / b.L];
}

// x3_weight_image (conv_mfma.hip) restated: w = hi + lo, both bf16, round-to-nearest-even
__device__ __forceinline__ unsigned bf16_rne_dev(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ void bf16_split(float w, unsigned& hi, unsigned& lo) {
  hi = bf16_rne_dev(w);
  lo = bf16_rne_dev(w - __uint_as_float(hi << 16));
}
// The images of a dense k = 5 layer.  A 16-byte piece of the forward image holds 8 consecutive input channels of one (output channel, tap); a piece of a
// transposed phase image holds 8 consecutive OUTPUT channels of one (input channel, tap) - hence the tile through LDS.  The transposed images are those of
// disc_bwd_images (discriminator.hip): stride 1 is one image of 5 taps, tap t carrying W[.][.][4 - t]; stride 3 is one image per phase r of the input row,
// r = 0 one tap (W[.][.][2]), r > 0 two taps (W[.][.][r + 2], W[.][.][r - 1]).
constexpr int kImgCo = 16, kImgSlab = 64, kImgK = 5;
struct ImgLayer { const float* v; const float* sc; uint4* wx; uint4* wxb[3]; int Ci, Co, CoPx, CiPx, stride, slab, first, nblocks; };   // sc null: v is the weight
__global__ __launch_bounds__(256) void disc_image_kernel(const ImgLayer* __restrict__ tab, int nlayers) {
  __shared__ float wl[kImgCo][kImgSlab * kImgK + 1];
  int li = 0;
  while (li + 1 < nlayers && (int)blockIdx.x >= tab[li].first + tab[li].nblocks) ++li;
  const ImgLayer L = tab[li];
  const int local = (int)blockIdx.x - L.first, nslab = L.Ci / L.slab, co0 = (local / nslab) * kImgCo, ci0 = (local % nslab) * L.slab, span = L.slab * kImgK;
  for (int i = threadIdx.x; i < kImgCo * span; i += 256) {
    const int r = i / span, c = i - r * span;
    const float x = L.v[((long long)(co0 + r) * L.Ci + ci0) * kImgK + c];
    wl[r][c] = L.sc ? x * L.sc[co0 + r] : x;
  }
  __syncthreads();
  // forward image [chunk][tap][hi | lo][half][CoPx rows][8 ch]
  for (int q = threadIdx.x; q < kImgCo * kImgK * (L.slab / 8); q += 256) {
    const int col = q & (kImgCo - 1), rest = q / kImgCo, u = rest % kImgK, grp = rest / kImgK, ci = ci0 + grp * 8;
    unsigned hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bf16_split(wl[col][(grp * 8 + e) * kImgK + u], hi[e], lo[e]);
    const long long base = ((long long)((ci >> 4) * kImgK + u) * 4 + ((ci & 15) >> 3)) * L.CoPx + co0 + col;
    L.wx[base] = make_uint4(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16, hi[4] | hi[5] << 16, hi[6] | hi[7] << 16);
    L.wx[base + 2LL * L.CoPx] = make_uint4(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16, lo[4] | lo[5] << 16, lo[6] | lo[7] << 16);
  }
  // transposed phase images [chunk of 16 co][tap][hi | lo][half][CiPx rows][8 co]: five (phase, tap) slots in all for either stride
  for (int q = threadIdx.x; q < L.slab * 2 * kImgK; q += 256) {
    const int cil = q % L.slab, h = (q / L.slab) & 1, slot = q / (2 * L.slab);
    int r, nt, t, src;
    if (L.stride == 1) { r = 0; nt = 5; t = slot; src = 4 - slot; }
    else if (slot == 0) { r = 0; nt = 1; t = 0; src = 2; }
    else { r = (slot + 1) >> 1; nt = 2; t = (slot + 1) & 1; src = t == 0 ? r + 2 : r - 1; }
    unsigned hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bf16_split(wl[h * 8 + e][cil * kImgK + src], hi[e], lo[e]);
    const long long base = ((long long)((co0 >> 4) * nt + t) * 4 + h) * L.CiPx + ci0 + cil;
    uint4* W = L.wxb[r];
    W[base] = make_uint4(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16, hi[4] | hi[5] << 16, hi[6] | hi[7] << 16);
    W[base + 2LL * L.CiPx] = make_uint4(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16, lo[4] | lo[5] << 16, lo[6] | lo[7] << 16);
  }
}

// The device tables of one finalized handle: made by the first call that needs them, dropped by finalize.
struct DiscOptimTables {
  DevBuf<AdamwChunk> chunks; DevBuf<FoldBlock> folds; DevBuf<ImgLayer> imgs;
  DevVec sc;                                        // sc[co] of every weight-normed layer, layer after layer
  std::vector<float*> ptr; std::vector<long long> off, n;   // per parameter tensor: where the handle holds it, its place in the flat buffers, its length
  long long total = 0;
  int img_blocks = 0, img_layers = 0;
};
static float* disc_param_ptr(const DiscLayer& L, int which) {     // 0: bias, 1: weight_g, 2: weight_v or the plain weight
  if (which == 0) return L.b.p;
  if (which == 1) return L.pg.p;
  if (L.gi_g >= 0) return L.pv.p;
  return disc_layer_is_gemm(L) ? L.pv.p : L.w.p;
}
static DiscOptimTables& disc_optim_tables(Disc* D, const char* who) {
  RVC_REQUIRE(D->ready, "finalize first");
  RVC_REQUIRE(D->kept, std::string(who) + " needs the parameters on the device: call rvc_disc_keep_parameters(d, 1) before finalize (trainable=True)");
  if (D->optim) return *D->optim;
  auto T = std::make_shared<DiscOptimTables>();
  const size_t np = D->params.size();
  T->ptr.assign(np, nullptr); T->off.assign(np, 0); T->n.assign(np, 0);
  for (size_t k = 0; k < np; ++k) {
    long long n = 1; for (long long d : D->params[k].shape) n *= d;
    T->n[k] = n; T->off[k] = T->total; T->total += n;
  }
  size_t rows = 0;
  for (DiscNet& net : D->nets)
    for (DiscLayer& L : net.L) {
      T->ptr[L.gi_b] = disc_param_ptr(L, 0); T->ptr[L.gi_w] = disc_param_ptr(L, 2);
      if (L.gi_g >= 0) { T->ptr[L.gi_g] = disc_param_ptr(L, 1); rows += (size_t)L.Co; }
    }
  for (size_t k = 0; k < np; ++k) RVC_REQUIRE(T->ptr[k], "parameter " + D->params[k].name + " is not on the device");
  if (rows) T->sc.alloc(rows);
  std::vector<AdamwChunk> chunks;
  for (size_t k = 0; k < np; ++k)
    for (long long o = 0; o < T->n[k]; o += kChunk) chunks.push_back(AdamwChunk{T->ptr[k] + o, T->off[k] + o, (int)std::min<long long>(kChunk, T->n[k] - o), 0});
  std::vector<FoldBlock> folds; std::vector<ImgLayer> imgs;
  size_t row0 = 0;
  for (DiscNet& net : D->nets)
    for (DiscLayer& L : net.L) {
      const bool gemm = disc_layer_is_gemm(L), wn = L.gi_g >= 0;
      const int Lrow = (L.Ci / L.groups) * L.k;
      float* sc = wn ? T->sc.p + row0 : nullptr;
      if (wn) {
        for (int r = 0; r < L.Co; r += kFoldRows)
          folds.push_back(FoldBlock{L.pv.p + (long long)r * Lrow, L.pg.p + r, sc + r, gemm ? nullptr : L.w.p + (long long)r * Lrow, std::min(kFoldRows, L.Co - r), Lrow});
        row0 += (size_t)L.Co;
      }
      if (gemm) {
        RVC_REQUIRE(L.k == kImgK && (L.stride == 1 || L.stride == 3) && L.Co % kImgCo == 0 && L.Ci % 16 == 0 && L.pv.p && L.wx.p, "dense discriminator layer: k 5, stride 1 or 3");
        ImgLayer I{};
        I.v = L.pv.p; I.sc = sc; I.wx = reinterpret_cast<uint4*>(L.wx.p);
        for (int r = 0; r < L.stride; ++r) { RVC_REQUIRE(L.wxb[r].p, "missing phase image"); I.wxb[r] = reinterpret_cast<uint4*>(L.wxb[r].p); }
        I.Ci = L.Ci; I.Co = L.Co; I.CoPx = L.CoPx; I.CiPx = L.CiPx; I.stride = L.stride;
        I.slab = L.Ci % kImgSlab == 0 ? kImgSlab : (L.Ci % 32 == 0 ? 32 : 16);
        I.first = T->img_blocks; I.nblocks = (L.Co / kImgCo) * (L.Ci / I.slab);
        T->img_blocks += I.nblocks;
        imgs.push_back(I);
      }
    }
  T->chunks.upload(chunks);
  if (!folds.empty()) T->folds.upload(folds);
  if (!imgs.empty()) T->imgs.upload(imgs);
  T->img_layers = (int)imgs.size();
  D->optim = T;
  return *T;
}
static void disc_refold(DiscOptimTables& T, hipStream_t s) {
  if (T.folds.n) hipLaunchKernelGGL(disc_fold_kernel, dim3((unsigned)T.folds.n), dim3(256), 0, s, T.folds.p);
  if (T.img_blocks) hipLaunchKernelGGL(disc_image_kernel, dim3((unsigned)T.img_blocks), dim3(256), 0, s, T.imgs.p, T.img_layers);
}
int disc_adamw_step_launch_count(Disc* D) {
  const DiscOptimTables& T = disc_optim_tables(D, "the optimizer step");
  return 1 + (T.folds.n ? 1 : 0) + (T.img_blocks ? 1 : 0);
}
void disc_adamw_step(Disc* D, hipStream_t s, const float* grads, float* exp_avg, float* exp_avg_sq, const rvc_adamw_hyper& h) {
  RVC_REQUIRE(grads && exp_avg && exp_avg_sq, "null argument");
  RVC_REQUIRE((((uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3) == 0, "disc_adamw_step: pointers must be 4-byte aligned");
  DiscOptimTables& T = disc_optim_tables(D, "the optimizer step");
  const AdamwK k = adamw_scalars(h);
  hipLaunchKernelGGL(disc_adamw_kernel, dim3((unsigned)T.chunks.n), dim3(256), 0, s, T.chunks.p, grads, exp_avg, exp_avg_sq, k);
  disc_refold(T, s);
}
long long disc_param_total(Disc* D) { return disc_optim_tables(D, "parameter I/O").total; }
void disc_get_parameters(Disc* D, hipStream_t s, float* flat) {
  RVC_REQUIRE(flat, "null argument");
  const DiscOptimTables& T = disc_optim_tables(D, "get_parameters");
  for (size_t k = 0; k < T.ptr.size(); ++k)
    RVC_HIP_CHECK(hipMemcpyAsync(flat + T.off[k], T.ptr[k], (size_t)T.n[k] * sizeof(float), hipMemcpyDeviceToDevice, s));
}
void disc_set_parameters(Disc* D, hipStream_t s, const float* flat) {
  RVC_REQUIRE(flat, "null argument");
  DiscOptimTables& T = disc_optim_tables(D, "set_parameters");
  for (size_t k = 0; k < T.ptr.size(); ++k)
    RVC_HIP_CHECK(hipMemcpyAsync(T.ptr[k], flat + T.off[k], (size_t)T.n[k] * sizeof(float), hipMemcpyDeviceToDevice, s));
  disc_refold(T, s);
}

}  // namespace rvc
