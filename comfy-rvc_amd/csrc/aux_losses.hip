// The trainer's auxiliary generator losses on log-mel spectrograms [B][F][T] (reference lib/train/losses.py:235-277 compute_tsi_loss / compute_envelope,
// :324-342 compute_harmonics, :376-390 of combined_aux_loss; lib/infer_pack/commons.py:71-108), forward only.  gfx950, plain HIP.
//
// HPSS (librosa.decompose.hpss with margin 1, power 2 on S = |mag|, kernel sizes 3, 7, 13, 19, 29): a workgroup stages a 32 x 32 tile of S with a
// 14-element halo on all four sides in LDS (60 x 60 values; the halo is read through scipy's "reflect" index, so the filters see the boundary
// already folded in) and produces all five kernel sizes and both directions from that one load.  The windows are nested and centred, so a thread
// grows ONE sorted list per direction (sorted_insert, signal_dev.h; the lists live in LDS, interleaved by thread) from 1 to 29 values and reads the
// median off it at 3, 7, 13, 19 and 29 values: the median of an odd window is one of its inputs and comes out exact.  The soft masks are fp32 step by step as numpy forms them (explicit _rn
// intrinsics: no contraction).  hpss_kernel<MODE>: 0 writes the raw harmonic / percussive parts [B][F][5 T] (compute_harmonics), 1 reduces the
// min / max of the four tensors of a (original, generated) pair, 2 reduces |scaled generated - scaled original| with those min / max; neither
// 1 nor 2 writes a 5 T tensor.  The L1 sums are float64 in a fixed order (thread: its elements in order; block_sum; f64_segment_sums over the
// workgroups in index order); min / max are order-free.
//
// TSI: one workgroup per (item, dim) forms both envelopes (L2 norm along dim, max over t - 1 .. t + 1, sum along dim; sums in float64, one thread per
// kept index walking the summed axis in order) and their Pearson correlation with the reference's eps placement.
#include <cfloat>
#include "rvc_internal.h"
#include "models.h"
#include "signal_dev.h"

namespace rvc {

// ------------------------------------------------------------------------------------------------ fixed-order float64 sums of segments
struct SegSumArgs { const double* x; long long b[kSegSumMax + 1]; double* out; };
__global__ __launch_bounds__(256) void f64_segment_sums_kernel(SegSumArgs a) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long j = a.b[blockIdx.x] + threadIdx.x; j < a.b[blockIdx.x + 1]; j += 256) acc += a.x[j];
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) a.out[blockIdx.x] = t;
}
void f64_segment_sums(hipStream_t s, const double* x, const long long* bounds, int K, double* out) {
  RVC_REQUIRE(K >= 1 && K <= kSegSumMax, "f64_segment_sums: 1 <= K <= 16 segments");
  SegSumArgs a;
  a.x = x; a.out = out;
  for (int k = 0; k <= K; ++k) a.b[k] = bounds[k];
  for (int k = 0; k < K; ++k) RVC_REQUIRE(a.b[k] <= a.b[k + 1], "f64_segment_sums: bounds must ascend");
  hipLaunchKernelGGL(f64_segment_sums_kernel, dim3(K), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------ HPSS
constexpr int kHpTile = 32, kHpHalo = 14, kHpW = kHpTile + 2 * kHpHalo, kHpPitch = kHpW + 1, kHpSizes = 5, kHpMaxK = 2 * kHpHalo + 1;
__device__ __constant__ int kHpHalf[kHpSizes] = {1, 3, 6, 9, 14};      // kernel sizes 3, 7, 13, 19, 29

struct HpssArgs {
  const float* x[2];                 // [B][F][T]: the original (or only) tensor, the generated one
  int B, F, T, tiles_t, tiles_f;
  float* h; float* p;                // MODE 0: [B][F][5 T]
  int medians;                       // MODE 0: h, p take the medians themselves (along time, along mel) instead of S * mask
  const float* mm;                   // MODE 2: (min, max) of original harmonic, original percussive, generated harmonic, generated percussive
  float eps;
  float* mm_part;                    // MODE 1: [blocks][8]
  double* l1_part;                   // MODE 2: [2][blocks]
  long long blocks;
};

// numpy's softmask(X, X_ref, power=2, split_zeros=True) of one element, in float32
__device__ __forceinline__ float softmask2(float x, float r) {
  const float z = fmaxf(x, r);
  if (z < FLT_MIN) return 0.5f;
  float a = __fdiv_rn(x, z), b = __fdiv_rn(r, z);
  a = __fmul_rn(a, a); b = __fmul_rn(b, b);
  return __fdiv_rn(a, __fadd_rn(a, b));
}

// medians of the five nested windows around c[0] along `step`; w: the thread's sorted list in LDS, element i at w[256 i] (conflict-free)
__device__ __forceinline__ void nested_medians(const float* c, int step, float* w, float (&med)[kHpSizes]) {
  w[0] = c[0];
  int n = 1, r = 0;
  for (int q = 0; q < kHpSizes; ++q) {
    const int h = kHpHalf[q];
    while (r < h) { ++r; sorted_insert<256>(w, n++, c[-r * step]); sorted_insert<256>(w, n++, c[r * step]); }
    med[q] = w[h * 256];
  }
}

__device__ __forceinline__ void hpss_point(const float* c, float* w, bool medians, float (&H)[kHpSizes], float (&P)[kHpSizes]) {
  float mt[kHpSizes], mf[kHpSizes];
  nested_medians(c, 1, w, mt);                  // along time: harmonic
  nested_medians(c, kHpPitch, w, mf);           // along mel: percussive
  const float S = c[0];
#pragma unroll
  for (int q = 0; q < kHpSizes; ++q) {
    H[q] = medians ? mt[q] : __fmul_rn(S, softmask2(mt[q], mf[q]));
    P[q] = medians ? mf[q] : __fmul_rn(S, softmask2(mf[q], mt[q]));
  }
}

__device__ __forceinline__ float scale_fix(float v, float mn, float den, float eps) {      // minmax_scale(...).nan_to_num(eps)
  const float y = __fdiv_rn(__fsub_rn(v, mn), den);
  return y != y ? eps : fminf(fmaxf(y, -FLT_MAX), FLT_MAX);
}

template <int MODE>
__global__ __launch_bounds__(256) void hpss_kernel(HpssArgs a) {
  constexpr int NIMG = MODE == 0 ? 1 : 2;
  __shared__ float tile[NIMG][kHpW * kHpPitch];
  __shared__ float sorted[kHpMaxK * 256];
  __shared__ double red[4];
  __shared__ float mred[4][8];
  const int tid = threadIdx.x;
  const int bt = blockIdx.x % a.tiles_t, bf = (blockIdx.x / a.tiles_t) % a.tiles_f, item = blockIdx.x / (a.tiles_t * a.tiles_f);
  const int t0 = bt * kHpTile, f0 = bf * kHpTile;
  for (int g = 0; g < NIMG; ++g) {
    const float* x = a.x[g] + (long long)item * a.F * a.T;
    for (int i = tid; i < kHpW * kHpW; i += 256) {
      const int y = i / kHpW, xx = i - y * kHpW;
      long long f = reflect_index(f0 - kHpHalo + y, a.F), t = reflect_index(t0 - kHpHalo + xx, a.T);
      f = f < 0 ? 0 : (f >= a.F ? a.F - 1 : f);          // positions beyond the halo of the last tile: never used, kept inside the tensor
      t = t < 0 ? 0 : (t >= a.T ? a.T - 1 : t);
      tile[g][y * kHpPitch + xx] = fabsf(x[f * a.T + t]);
    }
  }
  __syncthreads();
  float mn[8], mx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { mn[k] = FLT_MAX; mx[k] = -FLT_MAX; }
  double acc_h = 0.0, acc_p = 0.0;
  float den[4] = {1.f, 1.f, 1.f, 1.f};
  if (MODE == 2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) den[k] = __fadd_rn(__fsub_rn(a.mm[2 * k + 1], a.mm[2 * k]), a.eps);
  }
  for (int e = tid; e < kHpTile * kHpTile; e += 256) {
    const int y = e / kHpTile, xx = e - y * kHpTile;
    const int f = f0 + y, t = t0 + xx;
    if (f >= a.F || t >= a.T) continue;
    float H[NIMG][kHpSizes], P[NIMG][kHpSizes];
    for (int g = 0; g < NIMG; ++g) hpss_point(&tile[g][(y + kHpHalo) * kHpPitch + xx + kHpHalo], sorted + tid, MODE == 0 && a.medians, H[g], P[g]);
    if (MODE == 0) {
      const long long o = ((long long)item * a.F + f) * (5LL * a.T) + t;
#pragma unroll
      for (int q = 0; q < kHpSizes; ++q) { a.h[o + (long long)q * a.T] = H[0][q]; a.p[o + (long long)q * a.T] = P[0][q]; }
    } else if (MODE == 1) {
      for (int g = 0; g < NIMG; ++g)
#pragma unroll
        for (int q = 0; q < kHpSizes; ++q) {
          mn[2 * g] = fminf(mn[2 * g], H[g][q]); mx[2 * g] = fmaxf(mx[2 * g], H[g][q]);
          mn[2 * g + 1] = fminf(mn[2 * g + 1], P[g][q]); mx[2 * g + 1] = fmaxf(mx[2 * g + 1], P[g][q]);
        }
    } else {
#pragma unroll
      for (int q = 0; q < kHpSizes; ++q) {
        const float ho = scale_fix(H[0][q], a.mm[0], den[0], a.eps), po = scale_fix(P[0][q], a.mm[2], den[1], a.eps);
        const float hg = scale_fix(H[NIMG - 1][q], a.mm[4], den[2], a.eps), pg = scale_fix(P[NIMG - 1][q], a.mm[6], den[3], a.eps);
        acc_h += (double)fabsf(__fsub_rn(hg, ho)); acc_p += (double)fabsf(__fsub_rn(pg, po));
      }
    }
  }
  if (MODE == 1) {                     // slots: k = 2 * tensor + (0 min, 1 max); tensor = original harmonic, original percussive, generated harmonic, generated percussive
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = mn[k]; v[2 * k + 1] = mx[k]; }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      for (int o = 32; o > 0; o >>= 1) { const float u = __shfl_xor(v[k], o); v[k] = (k & 1) ? fmaxf(v[k], u) : fminf(v[k], u); }
    if ((tid & 63) == 0)
#pragma unroll
      for (int k = 0; k < 8; ++k) mred[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < 8) {
      float u = mred[0][tid];
      for (int wv = 1; wv < 4; ++wv) u = (tid & 1) ? fmaxf(u, mred[wv][tid]) : fminf(u, mred[wv][tid]);
      a.mm_part[(long long)blockIdx.x * 8 + tid] = u;
    }
  }
  if (MODE == 2) {
    const double th = block_sum(acc_h, red);
    const double tp = block_sum(acc_p, red);
    if (tid == 0) { a.l1_part[blockIdx.x] = th; a.l1_part[a.blocks + blockIdx.x] = tp; }
  }
}

__global__ __launch_bounds__(256) void minmax_final_kernel(const float* __restrict__ part, long long blocks, float* out) {
  __shared__ float mred[4][8];
  const int tid = threadIdx.x;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = (k & 1) ? -FLT_MAX : FLT_MAX;
  for (long long b = tid; b < blocks; b += 256)
#pragma unroll
    for (int k = 0; k < 8; ++k) { const float u = part[b * 8 + k]; v[k] = (k & 1) ? fmaxf(v[k], u) : fminf(v[k], u); }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    for (int o = 32; o > 0; o >>= 1) { const float u = __shfl_xor(v[k], o); v[k] = (k & 1) ? fmaxf(v[k], u) : fminf(v[k], u); }
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < 8; ++k) mred[tid >> 6][k] = v[k];
  __syncthreads();
  if (tid < 8) {
    float u = mred[0][tid];
    for (int wv = 1; wv < 4; ++wv) u = (tid & 1) ? fmaxf(u, mred[wv][tid]) : fminf(u, mred[wv][tid]);
    out[tid] = u;
  }
}

static HpssArgs hpss_args(const float* x0, const float* x1, int B, int F, int T) {
  RVC_REQUIRE(x0 && x1 && B >= 1 && F > kHpHalo && T > kHpHalo, "hpss: both spectrogram axes must be longer than 14");
  HpssArgs a{};
  a.x[0] = x0; a.x[1] = x1; a.B = B; a.F = F; a.T = T;
  a.tiles_t = (T + kHpTile - 1) / kHpTile; a.tiles_f = (F + kHpTile - 1) / kHpTile;
  a.blocks = (long long)B * a.tiles_t * a.tiles_f;
  RVC_REQUIRE(a.blocks < (1LL << 31) && (long long)B * F * T * 5 < (1LL << 40), "hpss: tensor too large");
  return a;
}

// launches: 1.  h, p [B][F][5 T]: S * mask of kernel size 3 | 7 | 13 | 19 | 29 side by side along the last axis, before the min-max scaling
// (medians != 0: the two medians themselves, for the exactness test)
void hpss_parts(hipStream_t s, const float* x, int B, int F, int T, float* h, float* p, int medians) {
  HpssArgs a = hpss_args(x, x, B, F, T);
  RVC_REQUIRE(h && p, "hpss: null output");
  a.h = h; a.p = p; a.medians = medians != 0;
  hipLaunchKernelGGL(hpss_kernel<0>, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
}

// launches: 4 (min / max partials, min / max, L1 partials, the two sums).  out2 = (sum |gen_h - org_h|, sum |gen_p - org_p|) over the B F 5 T scaled values
void hpss_l1(hipStream_t s, const float* org, const float* gen, int B, int F, int T, float eps, double* out2) {
  HpssArgs a = hpss_args(org, gen, B, F, T);
  RVC_REQUIRE(out2 && eps >= 0.f, "hpss: bad argument");
  char* scr = (char*)stream_scratch(s, 23, (size_t)a.blocks * (8 * sizeof(float) + 2 * sizeof(double)) + 64);
  a.l1_part = (double*)scr;
  a.mm_part = (float*)(scr + (size_t)a.blocks * 2 * sizeof(double));
  float* mm = a.mm_part + a.blocks * 8;
  a.mm = mm; a.eps = eps;
  hipLaunchKernelGGL(hpss_kernel<1>, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(256), 0, s, a.mm_part, a.blocks, mm);
  hipLaunchKernelGGL(hpss_kernel<2>, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
  const long long bounds[3] = {0, a.blocks, 2 * a.blocks};
  f64_segment_sums(s, a.l1_part, bounds, 2, out2);
}

// ------------------------------------------------------------------------------------------------ TSI
struct TsiArgs { const float* x[2]; int B, F, T; float eps; double* out; };

// block (item, dim): dim 0 = the reference's dim=-1 (normalise and sum along time, correlate along mel), dim 1 = dim=-2.  LDS: env [2][L] | norm [2][T]
__global__ __launch_bounds__(256) void tsi_kernel(TsiArgs a) {
  extern __shared__ float tsi_lds[];
  __shared__ double red[4];
  const int tid = threadIdx.x, item = blockIdx.x >> 1, dim = blockIdx.x & 1;
  const int F = a.F, T = a.T, L = dim == 0 ? F : T;
  float* env = tsi_lds;               // [2][L]
  float* nrm = tsi_lds + 2 * L;       // [2][T] (dim 1)
  for (int g = 0; g < 2; ++g) {
    const float* x = a.x[g] + (long long)item * F * T;
    if (dim == 0) {
      for (int f = tid; f < F; f += 256) {
        const float* r = x + (long long)f * T;
        double ss = 0.0;
        for (int t = 0; t < T; ++t) ss += (double)r[t] * (double)r[t];
        const float d = fmaxf((float)sqrt(ss), a.eps);
        double e = 0.0;
        for (int t = 0; t < T; ++t) {
          float m = __fdiv_rn(r[t], d);
          if (t > 0) m = fmaxf(m, __fdiv_rn(r[t - 1], d));
          if (t + 1 < T) m = fmaxf(m, __fdiv_rn(r[t + 1], d));
          e += (double)(m != m ? a.eps : m);
        }
        env[g * L + f] = (float)e;
      }
    } else {
      for (int t = tid; t < T; t += 256) {
        double ss = 0.0;
        for (int f = 0; f < F; ++f) { const float v = x[(long long)f * T + t]; ss += (double)v * (double)v; }
        nrm[g * T + t] = fmaxf((float)sqrt(ss), a.eps);
      }
      __syncthreads();
      for (int t = tid; t < T; t += 256) {
        double e = 0.0;
        for (int f = 0; f < F; ++f) {
          const float* r = x + (long long)f * T;
          float m = __fdiv_rn(r[t], nrm[g * T + t]);
          if (t > 0) m = fmaxf(m, __fdiv_rn(r[t - 1], nrm[g * T + t - 1]));
          if (t + 1 < T) m = fmaxf(m, __fdiv_rn(r[t + 1], nrm[g * T + t + 1]));
          e += (double)(m != m ? a.eps : m);
        }
        env[g * L + t] = (float)e;
      }
    }
  }
  __syncthreads();
  // compute_correlation(x = original envelope, y = generated envelope) along the L kept values
  double sx = 0.0, sy = 0.0;
  for (int i = tid; i < L; i += 256) { sx += (double)env[i]; sy += (double)env[L + i]; }
  const float mx = (float)(block_sum(sx, red) / (double)L);
  const float my = (float)(block_sum(sy, red) / (double)L);
  double cxy = 0.0, cxx = 0.0, cyy = 0.0;
  for (int i = tid; i < L; i += 256) {
    const float dx = __fsub_rn(env[i], mx), dy = __fsub_rn(env[L + i], my);
    cxy += (double)dx * (double)dy; cxx += (double)dx * (double)dx; cyy += (double)dy * (double)dy;
  }
  const float cov = (float)block_sum(cxy, red);
  const float vx = (float)block_sum(cxx, red);
  const float vy = (float)block_sum(cyy, red);
  if (tid == 0) {
    float sdx = __fsqrt_rn(__fadd_rn(vx, a.eps)), sdy = __fsqrt_rn(__fadd_rn(vy, a.eps));
    if (sdx != sdx) sdx = a.eps;
    if (sdy != sdy) sdy = a.eps;
    float c = __fdiv_rn(cov, __fadd_rn(__fmul_rn(sdx, sdy), a.eps));
    if (c != c) c = a.eps;
    a.out[(long long)dim * a.B + item] = (double)__fsub_rn(1.0f, c);
  }
}

// launches: 1.  out [2][B] = 1 - correlation per item for dim=-1 (row 0) and dim=-2 (row 1)
void tsi_terms(hipStream_t s, const float* org, const float* gen, int B, int F, int T, float eps, double* out) {
  RVC_REQUIRE(org && gen && out && B >= 1 && F >= 1 && T >= 1 && eps >= 0.f, "tsi: bad argument");
  const size_t lds = ((size_t)2 * std::max(F, T) + 2 * (size_t)T) * sizeof(float);
  RVC_REQUIRE(lds <= 48 * 1024, "tsi: 2 max(F, T) + 2 T values must fit 48 KB of LDS");
  TsiArgs a;
  a.x[0] = org; a.x[1] = gen; a.B = B; a.F = F; a.T = T; a.eps = eps; a.out = out;
  hipLaunchKernelGGL(tsi_kernel, dim3(2 * B), dim3(256), lds, s, a);
}

}  // namespace rvc
