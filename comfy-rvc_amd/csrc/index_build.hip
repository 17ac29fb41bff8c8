// Building the retrieval index on the device: the k-means that RVCTrainModelNode.train_index (reference custom_nodes/rvc_nodes.py:500-554) leaves to
// faiss (IndexIVFFlat::train: Lloyd iterations over the level-1 quantiser's centroids, then add = one assignment against the final centroids).
//   assign: label_i = argmin_j |x_i - c_j|^2 = argmax_j (c_j . x_i - |c_j|^2 / 2), the arithmetic of the search (index.hip): bf16 hi / lo split of
//           both operands, hi*lo + lo*hi + hi*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Unlike the search the [K][N] scores never reach
//           memory: a workgroup owns 128 rows, walks its share of the 128-centroid tiles and keeps the running best of every row in registers; the
//           K range is split over blockIdx.y when the row tiles alone do not fill the chip, and a merge kernel picks the best of the splits (ties:
//           smallest index, everywhere).  The distance of the winner is then evaluated directly, sum_d (x_d - c_d)^2 in fp64: no cancellation, so
//           a row that IS a centroid gets 0 and the inertia is good to fp32 rounding.
//   update: counting sort of the row ids by label (stable: ids ascending inside a cluster, so the order of every sum is fixed), segmented fp64 sum,
//           one rounding to fp32; empty clusters by faiss's split rule (Clustering.cpp::split_clusters) with the most populated cluster as the donor.
//           Integer atomics only (histogram); bit-identical from run to run.
#include "conv_x3_dev.h"
#include "models.h"
#include <climits>

namespace rvc {

namespace {

constexpr int kAT = 128;             // tile edge: centroids (MFMA rows) and data rows (MFMA columns) per workgroup
constexpr int kAK = 32;              // reduction depth of one stage = two MFMA steps
constexpr int kPlane = kAT * 16;     // bytes of one [row][8 ch] half-plane (conv_x3.hip's LDS row format)

// ------------------------------------------------------------------------------------------------ assign
// -|c_j|^2 / 2, one wave per centroid, fp64 sum rounded once
__global__ __launch_bounds__(256) void kmeans_nhalf_kernel(const float* __restrict__ cent, int K, int D, float* __restrict__ nhalf) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= K) return;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) { const double v = cent[(long long)j * D + d]; s += v * v; }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) nhalf[j] = (float)(-0.5 * s);
}

// grid (row tiles, K splits), 256 threads = 2 x 2 waves of 2 x 2 MFMA blocks.  LDS per operand: [k step][hi | lo][8-channel half][128 rows][8 ch] bf16.
// A staging unit is 8 consecutive floats of one row; thread t takes units t, t + 256, t + 512 (centroids), t + 768 ... (data rows), fetched one
// stage ahead into registers and split while they are written to LDS.  Rows past N / K and channels past D are zeros (and never win).
__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(const float* __restrict__ rows, long long N, int D, const float* __restrict__ cent, int K,
                                                               const float* __restrict__ nhalf, int tps, float* __restrict__ pbest,
                                                               int* __restrict__ pidx) {
  __shared__ __attribute__((aligned(16))) unsigned char As[8 * kPlane];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[8 * kPlane];
  __shared__ float s_nh[kAT];
  __shared__ float s_v[kAT];
  __shared__ int s_i[kAT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  const long long n0 = (long long)blockIdx.x * kAT;
  const int ktiles = (K + kAT - 1) / kAT;
  const int kt0 = blockIdx.y * tps, kt1 = min(ktiles, kt0 + tps);
  const int nch = (D + kAK - 1) / kAK;

  float4 ra[4][2];
  auto load = [&](int m0, int c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w = (tid + 256 * j) & 511, row = w >> 2, k = c * kAK + (w & 3) * 8;
      const float* src = nullptr;
      if (j < 2) { const int m = m0 + row; if (m < K && k < D) src = cent + (long long)m * D + k; }
      else { const long long n = n0 + row; if (n < N && k < D) src = rows + n * D + k; }
      if (src) { ra[j][0] = *reinterpret_cast<const float4*>(src); ra[j][1] = *reinterpret_cast<const float4*>(src + 4); }
      else { ra[j][0] = make_float4(0.f, 0.f, 0.f, 0.f); ra[j][1] = ra[j][0]; }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w = (tid + 256 * j) & 511, row = w >> 2, g = w & 3;
      unsigned char* dst = (j < 2 ? As : Bs) + ((g >> 1) * 4 + (g & 1)) * kPlane + row * 16;
      unsigned h[4], l[4];
      split2(ra[j][0].x, ra[j][0].y, h[0], l[0]); split2(ra[j][0].z, ra[j][0].w, h[1], l[1]);
      split2(ra[j][1].x, ra[j][1].y, h[2], l[2]); split2(ra[j][1].z, ra[j][1].w, h[3], l[3]);
      *reinterpret_cast<u32x4*>(dst) = u32x4{h[0], h[1], h[2], h[3]};
      *reinterpret_cast<u32x4*>(dst + 2 * kPlane) = u32x4{l[0], l[1], l[2], l[3]};
    }
  };

  float bv[2] = {-INFINITY, -INFINITY};
  int bi[2] = {INT_MAX, INT_MAX};
  for (int kt = kt0; kt < kt1; ++kt) {
    const int m0 = kt * kAT;
    f32x16 acc[2][2];
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int an = 0; an < 2; ++an)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[am][an][r] = 0.f;
    if (tid < kAT) s_nh[tid] = m0 + tid < K ? nhalf[m0 + tid] : -INFINITY;
    load(m0, 0);
    for (int c = 0; c < nch; ++c) {
      __syncthreads();                                   // every wave is done reading the previous stage
      store();
      if (c + 1 < nch) load(m0, c + 1);
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const unsigned char* ap = As + (kk * 4 + lh) * kPlane + ((wm * 2) * 32 + li) * 16;
        const unsigned char* bp = Bs + (kk * 4 + lh) * kPlane + ((wn * 2) * 32 + li) * 16;
        u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          ah[a] = *reinterpret_cast<const u32x4*>(ap + a * 512); al[a] = *reinterpret_cast<const u32x4*>(ap + a * 512 + 2 * kPlane);
          bh[a] = *reinterpret_cast<const u32x4*>(bp + a * 512); bl[a] = *reinterpret_cast<const u32x4*>(bp + a * 512 + 2 * kPlane);
        }
#pragma unroll
        for (int am = 0; am < 2; ++am)
#pragma unroll
          for (int an = 0; an < 2; ++an)
            acc[am][an] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al[am]), __builtin_bit_cast(bf16x8, bh[an]), acc[am][an], 0, 0, 0);
#pragma unroll
        for (int am = 0; am < 2; ++am)
#pragma unroll
          for (int an = 0; an < 2; ++an)
            acc[am][an] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[am]), __builtin_bit_cast(bf16x8, bl[an]), acc[am][an], 0, 0, 0);
#pragma unroll
        for (int am = 0; am < 2; ++am)
#pragma unroll
          for (int an = 0; an < 2; ++an)
            acc[am][an] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[am]), __builtin_bit_cast(bf16x8, bh[an]), acc[am][an], 0, 0, 0);
      }
    }
    // per-tile best: a lane sees its centroids in increasing order (tiles, am, r), so "strictly greater" keeps the smallest index
#pragma unroll
    for (int am = 0; am < 2; ++am)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = (wm * 2 + am) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float nh = s_nh[ml];
#pragma unroll
        for (int an = 0; an < 2; ++an) {
          const float v = acc[am][an][r] + nh;
          if (m0 + ml < K && v > bv[an]) { bv[an] = v; bi[an] = m0 + ml; }
        }
      }
    __syncthreads();                                     // s_nh is rewritten by the next tile
  }
  // the other half of the wave holds the other rows of the same columns, the other wave row (wm) the other 64 centroids of every tile
#pragma unroll
  for (int an = 0; an < 2; ++an) {
    const float ov = __shfl_xor(bv[an], 32);
    const int oi = __shfl_xor(bi[an], 32);
    if (ov > bv[an] || (ov == bv[an] && oi < bi[an])) { bv[an] = ov; bi[an] = oi; }
  }
  if (wm == 1 && lh == 0)
#pragma unroll
    for (int an = 0; an < 2; ++an) { const int col = (wn * 2 + an) * 32 + li; s_v[col] = bv[an]; s_i[col] = bi[an]; }
  __syncthreads();
  if (wm == 0 && lh == 0)
#pragma unroll
    for (int an = 0; an < 2; ++an) {
      const int col = (wn * 2 + an) * 32 + li;
      const float ov = s_v[col]; const int oi = s_i[col];
      if (ov > bv[an] || (ov == bv[an] && oi < bi[an])) { bv[an] = ov; bi[an] = oi; }
      const long long n = n0 + col;
      if (n < N) { pbest[(long long)blockIdx.y * N + n] = bv[an]; pidx[(long long)blockIdx.y * N + n] = bi[an]; }
    }
}

// One wave per row: the best of the S splits (every lane, broadcast loads), then the winner's squared distance evaluated directly.
__global__ __launch_bounds__(256) void kmeans_merge_kernel(const float* __restrict__ pbest, const int* __restrict__ pidx, int S, long long N,
                                                           const float* __restrict__ rows, const float* __restrict__ cent, int D, int K,
                                                           int* __restrict__ label, float* __restrict__ dist) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  float bv = pbest[n]; int bi = pidx[n];
  for (int s = 1; s < S; ++s) {
    const float v = pbest[(long long)s * N + n]; const int i = pidx[(long long)s * N + n];
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
  }
  if (bi < 0 || bi >= K) bi = 0;                         // a row of NaN scores compares false everywhere
  if (lane == 0) label[n] = bi;
  if (!dist) return;
  double s = 0.0;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 x = *reinterpret_cast<const float4*>(rows + n * D + d);
    const float4 c = *reinterpret_cast<const float4*>(cent + (long long)bi * D + d);
    const double a = (double)x.x - (double)c.x, b = (double)x.y - (double)c.y, e = (double)x.z - (double)c.z, f = (double)x.w - (double)c.w;
    s += a * a; s += b * b; s += e * e; s += f * f;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) dist[n] = (float)s;
}

// sum of dist in fp64, fixed order: thread t adds elements t, t + 1024, ..., then a tree over the threads
__global__ __launch_bounds__(1024) void kmeans_inertia_kernel(const float* __restrict__ dist, long long N, double* __restrict__ out) {
  __shared__ double s_s[1024];
  double s = 0.0;
  for (long long i = threadIdx.x; i < N; i += 1024) s += (double)dist[i];
  s_s[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if ((int)threadIdx.x < o) s_s[threadIdx.x] += s_s[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) *out = s_s[0];
}

// ------------------------------------------------------------------------------------------------ update
// Stable counting sort of the row ids by label.  The rows are cut into B contiguous blocks of R; hist[b][k] = rows of block b with label k,
// turned into "rows with label k in the blocks before b" by the scan; block b then places its rows chunk by chunk in row order.
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int* __restrict__ label, long long N, int K, long long R, int* __restrict__ hist) {
  const long long i0 = (long long)blockIdx.x * R, i1 = min(N, i0 + R);
  int* mine = hist + (long long)blockIdx.x * K;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) { const int l = label[i]; if (l >= 0 && l < K) atomicAdd(&mine[l], 1); }
}
__global__ __launch_bounds__(256) void kmeans_scan_blocks_kernel(int* __restrict__ hist, int B, int K, int* __restrict__ count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  int run = 0;
  for (int b = 0; b < B; ++b) { const int t = hist[(long long)b * K + k]; hist[(long long)b * K + k] = run; run += t; }
  count[k] = run;
}
// seg_off[k] = rows with a label below k (k = 0 .. K): thread t owns a contiguous run of clusters
__global__ __launch_bounds__(1024) void kmeans_scan_clusters_kernel(const int* __restrict__ count, int K, int* __restrict__ seg_off) {
  __shared__ int s_s[1024];
  const int per = (K + 1023) / 1024, k0 = min(K, (int)threadIdx.x * per), k1 = min(K, k0 + per);
  int s = 0;
  for (int k = k0; k < k1; ++k) s += count[k];
  s_s[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) { int run = 0; for (int t = 0; t < 1024; ++t) { const int v = s_s[t]; s_s[t] = run; run += v; } seg_off[K] = run; }
  __syncthreads();
  int run = s_s[threadIdx.x];
  for (int k = k0; k < k1; ++k) { seg_off[k] = run; run += count[k]; }
}
__global__ __launch_bounds__(256) void kmeans_place_kernel(const int* __restrict__ label, long long N, int K, long long R, int* base,
                                                           const int* __restrict__ seg_off, int* __restrict__ ids) {
  __shared__ int s_l[256];
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * R, i1 = min(N, i0 + R);
  int* mine = base + (long long)blockIdx.x * K;
  for (long long c0 = i0; c0 < i1; c0 += 256) {
    const long long i = c0 + tid;
    int l = i < i1 ? label[i] : -1;
    if (l >= K) l = -1;
    s_l[tid] = l;
    __syncthreads();                                     // (also: the previous chunk's update of `mine` is visible)
    int before = 0, after = 0;
    if (l >= 0) {
      for (int t = 0; t < 256; ++t) { const int same = s_l[t] == l; before += same & (t < tid); after += same & (t > tid); }
      ids[seg_off[l] + mine[l] + before] = (int)i;
    }
    __syncthreads();                                     // everybody has read `mine` and s_l
    if (l >= 0 && after == 0) mine[l] += before + 1;      // the chunk's last row of a label moves that label's cursor
  }
}
// grid (K, ceil(D / 256)): the rows of cluster k in id order, one channel per thread
__global__ __launch_bounds__(256) void kmeans_mean_kernel(const float* __restrict__ rows, const int* __restrict__ ids, const int* __restrict__ seg_off,
                                                          int D, float* __restrict__ cent) {
  const int k = blockIdx.x, d = blockIdx.y * 256 + threadIdx.x;
  const int a = seg_off[k], b = seg_off[k + 1];
  if (d >= D || b == a) return;                          // an empty cluster keeps its centroid until the split rule replaces it
  double s = 0.0;
  for (int i = a; i < b; ++i) s += (double)rows[(long long)ids[i] * D + d];
  cent[(long long)k * D + d] = (float)(s / (double)(b - a));
}
// faiss Clustering.cpp::split_clusters with a deterministic donor: empty clusters in increasing order; the donor is the most populated cluster at
// that moment (smallest index on ties); both get the donor's centroid, perturbed by 1 +- 1/1024 with alternating signs, and share its count.
__global__ __launch_bounds__(1024) void kmeans_split_kernel(float* __restrict__ cent, int* __restrict__ count, int K, int D) {
  __shared__ int s_a[1024], s_b[1024];
  const int tid = threadIdx.x;
  const float up = 1.f + 1.f / 1024.f, dn = 1.f - 1.f / 1024.f;
  for (int cursor = 0;;) {
    int e = INT_MAX;
    for (int k = cursor + tid; k < K; k += 1024) if (count[k] == 0) { e = k; break; }
    s_a[tid] = e;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) { if (tid < o) s_a[tid] = min(s_a[tid], s_a[tid + o]); __syncthreads(); }
    const int j = s_a[0];
    __syncthreads();
    if (j == INT_MAX) return;
    int bc = -1, bk = INT_MAX;
    for (int k = tid; k < K; k += 1024) { const int c = count[k]; if (c > bc) { bc = c; bk = k; } }
    s_a[tid] = bc; s_b[tid] = bk;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if (tid < o) {
        const int c = s_a[tid + o], k = s_b[tid + o];
        if (c > s_a[tid] || (c == s_a[tid] && k < s_b[tid])) { s_a[tid] = c; s_b[tid] = k; }
      }
      __syncthreads();
    }
    const int donor = s_b[0], dc = s_a[0];
    __syncthreads();
    if (dc <= 0) return;
    for (int d = tid; d < D; d += 1024) {
      const float v = cent[(long long)donor * D + d];
      cent[(long long)j * D + d] = v * ((d & 1) ? dn : up);
      cent[(long long)donor * D + d] = v * ((d & 1) ? up : dn);
    }
    if (tid == 0) { const int h = dc / 2; count[j] = h; count[donor] = dc - h; }
    cursor = j + 1;
    __syncthreads();
  }
}

__global__ void kmeans_gather_kernel(const float* __restrict__ rows, const long long* __restrict__ init, int D, float* __restrict__ cent) {
  const long long r = init[blockIdx.x];
  for (int d = threadIdx.x; d < D; d += blockDim.x) cent[(long long)blockIdx.x * D + d] = rows[r * D + d];
}

void check_shape(long long N, int D, int K) {
  RVC_REQUIRE(N > 0 && N <= INT_MAX, "k-means: 1 .. 2^31 - 1 rows");
  RVC_REQUIRE(D > 0 && D % 8 == 0 && D <= 4096, "k-means: feature dimension must be a multiple of 8, at most 4096");
  RVC_REQUIRE(K > 0 && K <= (1 << 22), "k-means: 1 .. 2^22 centroids");
}
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

void kmeans_assign(Ctx* ctx, hipStream_t s, const float* rows, long long N, int D, const float* cent, int K, int* label, float* dist) {
  (void)ctx;
  check_shape(N, D, K);
  const int ktiles = (K + kAT - 1) / kAT;
  const long long ntiles = (N + kAT - 1) / kAT;
  // K splits only while the row tiles alone leave compute units idle (256 CUs x 2 workgroups)
  int S = ntiles >= 512 ? 1 : (int)std::min<long long>(ktiles, (512 + ntiles - 1) / ntiles);
  const int tps = (ktiles + S - 1) / S;
  S = (ktiles + tps - 1) / tps;
  const size_t nh_b = up256((size_t)K * sizeof(float)), pb_b = up256((size_t)S * N * sizeof(float));
  char* scr = (char*)stream_scratch(s, 13, nh_b + 2 * pb_b);
  float* nhalf = (float*)scr; float* pbest = (float*)(scr + nh_b); int* pidx = (int*)(scr + nh_b + pb_b);
  hipLaunchKernelGGL(kmeans_nhalf_kernel, dim3((K + 3) / 4), dim3(256), 0, s, cent, K, D, nhalf);
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)ntiles, (unsigned)S), dim3(256), 0, s, rows, N, D, cent, K, nhalf, tps, pbest, pidx);
  hipLaunchKernelGGL(kmeans_merge_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, pbest, pidx, S, N, rows, cent, D, K, label, dist);
}

void kmeans_update(hipStream_t s, const float* rows, const int* label, long long N, int D, int K, float* cent, int* count) {
  check_shape(N, D, K);
  // row blocks of the counting sort: about 1024 rows each, at most 2^22 histogram cells in all
  const long long bmax = std::max<long long>(1, (1LL << 22) / K);
  const long long B = std::min<long long>(bmax, (N + 1023) / 1024);
  const long long R = (N + B - 1) / B;
  const size_t h_b = up256((size_t)B * K * sizeof(int)), o_b = up256((size_t)(K + 1) * sizeof(int));
  char* scr = (char*)stream_scratch(s, 14, h_b + o_b + up256((size_t)N * sizeof(int)));
  int* hist = (int*)scr; int* seg_off = (int*)(scr + h_b); int* ids = (int*)(scr + h_b + o_b);
  RVC_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)B * K * sizeof(int), s));
  hipLaunchKernelGGL(kmeans_hist_kernel, dim3((unsigned)B), dim3(256), 0, s, label, N, K, R, hist);
  hipLaunchKernelGGL(kmeans_scan_blocks_kernel, dim3((K + 255) / 256), dim3(256), 0, s, hist, (int)B, K, count);
  hipLaunchKernelGGL(kmeans_scan_clusters_kernel, dim3(1), dim3(1024), 0, s, count, K, seg_off);
  hipLaunchKernelGGL(kmeans_place_kernel, dim3((unsigned)B), dim3(256), 0, s, label, N, K, R, hist, seg_off, ids);
  hipLaunchKernelGGL(kmeans_mean_kernel, dim3((unsigned)K, (unsigned)((D + 255) / 256)), dim3(256), 0, s, rows, ids, seg_off, D, cent);
  hipLaunchKernelGGL(kmeans_split_kernel, dim3(1), dim3(1024), 0, s, cent, count, K, D);
}

void index_train(Ctx* ctx, hipStream_t s, const float* rows, long long N, int D, const long long* init_rows, int K, int niter, float* cent, int* label,
                 double* inertia) {
  check_shape(N, D, K);
  RVC_REQUIRE(init_rows && niter >= 0 && niter <= 1000, "k-means: initial rows and 0 .. 1000 iterations expected");
  for (int k = 0; k < K; ++k) RVC_REQUIRE(init_rows[k] >= 0 && init_rows[k] < N, "k-means: initial row out of range");
  const size_t i_b = up256((size_t)K * sizeof(long long)), d_b = up256((size_t)N * sizeof(float)), c_b = up256((size_t)K * sizeof(int));
  char* scr = (char*)stream_scratch(s, 15, i_b + d_b + c_b + up256((size_t)(niter + 1) * sizeof(double)));
  long long* init = (long long*)scr; float* dist = (float*)(scr + i_b); int* count = (int*)(scr + i_b + d_b);
  double* inert = (double*)(scr + i_b + d_b + c_b);
  RVC_HIP_CHECK(hipMemcpyAsync(init, init_rows, (size_t)K * sizeof(long long), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(kmeans_gather_kernel, dim3((unsigned)K), dim3(256), 0, s, rows, init, D, cent);
  for (int it = 0; it <= niter; ++it) {
    kmeans_assign(ctx, s, rows, N, D, cent, K, label, inertia ? dist : nullptr);
    if (inertia) hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(1), dim3(1024), 0, s, dist, N, inert + it);
    if (it < niter) kmeans_update(s, rows, label, N, D, K, cent, count);     // (the last pass is faiss's add: labels against the final centroids)
  }
  if (inertia) RVC_HIP_CHECK(hipMemcpyAsync(inertia, inert, (size_t)(niter + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
  RVC_HIP_CHECK(hipStreamSynchronize(s));                 // init_rows / inertia are host buffers of the caller
}

}  // namespace rvc
