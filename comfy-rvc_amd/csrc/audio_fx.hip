// Audio nodes on the device (reference lib/karafan/audio_utils.py::Silent / Normalize, lib/audio.py::AudioProcessor, custom_nodes/audio_nodes.py::
// MergeAudioNode / AudioBatchValueNode): the silence gate, click removal, peak normalisation, the per-sample merge of up to four tracks and the
// int64 energy of np.array_split segments.  The reference runs these over whole songs with scipy / librosa / numpy on the host; here every entry
// point is a fixed number of launches whatever the number of samples.  Prefix sums and index scans are block-propagated like the filter of
// dataset_prep.hip: every block reduces its tile, ONE block chains the tile totals through LDS, every block scans its tile again from its true offset.
#include "rvc_internal.h"
#include "ops.h"
#include "signal_dev.h"

namespace rvc {

constexpr int kFxThreads = 256, kFxItems = 8, kFxTile = kFxThreads * kFxItems;      // samples per block of a scan
constexpr int kFxParts = 512;                                                        // blocks of a reduction (grid-stride over the samples)

// ================================================================================================ block-propagated scans
// An Op has: T (value type), identity(), combine(a, b) (associative; a precedes b) and load(i) for element i of the scan order.
// Inclusive scan of one value per thread over the block; returns the scanned value, *total = combine of all 256.
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(const Op& op, typename Op::T v, typename Op::T* lds /*[5]*/, typename Op::T* total) {
  using T = typename Op::T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o);
    if (lane >= o) v = op.combine(u, v);
  }
  __syncthreads();                                   // lds may still be read by the previous call
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  T pre = op.identity();
  for (int w = 0; w < wave; ++w) pre = op.combine(pre, lds[w]);
  T all = op.identity();
#pragma unroll
  for (int w = 0; w < kFxThreads / 64; ++w) all = op.combine(all, lds[w]);
  *total = all;
  return op.combine(pre, v);
}

// pass 1: part[b] = combine of tile b
template <class Op>
__global__ __launch_bounds__(kFxThreads) void scan_reduce_kernel(const Op op, long long n, typename Op::T* part) {
  using T = typename Op::T;
  __shared__ T lds[kFxThreads / 64];
  const long long base = (long long)blockIdx.x * kFxTile + (long long)threadIdx.x * kFxItems;
  T a = op.identity();
#pragma unroll
  for (int k = 0; k < kFxItems; ++k) if (base + k < n) a = op.combine(a, op.load(base + k));
  T total;
  block_scan(op, a, lds, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}
// pass 2: part[b] -> combine of the tiles before b (exclusive), 256 tiles at a time, the carry through a register of every thread
template <class Op>
__global__ __launch_bounds__(kFxThreads) void scan_chain_kernel(const Op op, long long nb, typename Op::T* part) {
  using T = typename Op::T;
  __shared__ T lds[kFxThreads / 64];
  T carry = op.identity();
  for (long long base = 0; base < nb; base += kFxThreads) {
    const long long b = base + threadIdx.x;
    const T v = b < nb ? part[b] : op.identity();
    T total;
    const T inc = block_scan(op, v, lds, &total);
    // exclusive = carry (+) everything before this thread: the inclusive value of the left neighbour
    T ex = __shfl_up(inc, 1);
    __shared__ T edge[kFxThreads / 64];
    __syncthreads();
    if ((threadIdx.x & 63) == 63) edge[threadIdx.x >> 6] = inc;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ex = threadIdx.x == 0 ? op.identity() : edge[(threadIdx.x >> 6) - 1];
    if (b < nb) part[b] = op.combine(carry, ex);
    carry = op.combine(carry, total);
  }
}
// pass 3: out(i) = inclusive scan at element i
template <class Op, class Out>
__global__ __launch_bounds__(kFxThreads) void scan_write_kernel(const Op op, long long n, const typename Op::T* part, const Out out) {
  using T = typename Op::T;
  __shared__ T lds[kFxThreads / 64];
  const long long base = (long long)blockIdx.x * kFxTile + (long long)threadIdx.x * kFxItems;
  T v[kFxItems];
  T a = op.identity();
#pragma unroll
  for (int k = 0; k < kFxItems; ++k) {
    v[k] = base + k < n ? op.load(base + k) : op.identity();
    a = op.combine(a, v[k]);
  }
  T total;
  const T inc = block_scan(op, a, lds, &total);
  // the offset of this thread: tiles before (part) and threads before (inclusive minus own)
  __shared__ T edge[kFxThreads];
  edge[threadIdx.x] = inc;
  __syncthreads();
  T run = part[blockIdx.x];
  if (threadIdx.x > 0) run = op.combine(run, edge[threadIdx.x - 1]);
#pragma unroll
  for (int k = 0; k < kFxItems; ++k) {
    run = op.combine(run, v[k]);
    if (base + k < n) out(base + k, run);
  }
}
static long long scan_tiles(long long n) { return (n + kFxTile - 1) / kFxTile; }
template <class Op, class Out>
static void scan_launch(hipStream_t s, const Op& op, long long n, typename Op::T* part, const Out& out) {
  const long long nb = scan_tiles(n);
  RVC_REQUIRE(nb < (1LL << 31), "too many samples for one call");
  hipLaunchKernelGGL((scan_reduce_kernel<Op>), dim3((unsigned)nb), dim3(kFxThreads), 0, s, op, n, part);
  hipLaunchKernelGGL((scan_chain_kernel<Op>), dim3(1), dim3(kFxThreads), 0, s, op, nb, part);
  hipLaunchKernelGGL((scan_write_kernel<Op, Out>), dim3((unsigned)nb), dim3(kFxThreads), 0, s, op, n, part, out);
}

// sum of the float32-rounded squares in float64 (np.square of a float32 array, then scipy's float64 line buffer)
struct SqSumOp {
  using T = double;
  const float* x;
  __device__ __forceinline__ T identity() const { return 0.0; }
  __device__ __forceinline__ T combine(T a, T b) const { return a + b; }
  __device__ __forceinline__ T load(long long i) const { const float v = x[i]; return (double)__fmul_rn(v, v); }
};
// nearest non-click index at or before i (-1: none) / at or after i (n: none; scanned from the end: element r of the order is sample n - 1 - r)
struct PrevOp {
  using T = long long;
  const unsigned char* mask;
  __device__ __forceinline__ T identity() const { return -1; }
  __device__ __forceinline__ T combine(T a, T b) const { return a > b ? a : b; }
  __device__ __forceinline__ T load(long long i) const { return mask[i] ? -1 : i; }
};
struct NextOp {
  using T = long long;
  const unsigned char* mask; long long n;
  __device__ __forceinline__ T identity() const { return n; }
  __device__ __forceinline__ T combine(T a, T b) const { return a < b ? a : b; }
  __device__ __forceinline__ T load(long long r) const { const long long i = n - 1 - r; return mask[i] ? n : i; }
};
struct StoreP { double* p; __device__ __forceinline__ void operator()(long long i, double v) const { p[i + 1] = v; } };          // P[i + 1] = sum of [0, i]
struct StoreFwd { long long* p; __device__ __forceinline__ void operator()(long long i, long long v) const { p[i] = v; } };
struct StoreRev { long long* p; long long n; __device__ __forceinline__ void operator()(long long r, long long v) const { p[n - 1 - r] = v; } };

// ================================================================================================ click removal
// scipy.ndimage "reflect" (d c b a | a b c d | d c b a), one reflection: valid for -n <= j < 2 n

struct ClickArgs {
  const float* x; long long n;
  const double* P;                 // [n + 1] prefix sums of the squares, P[0] = 0 is never stored: read through psum()
  int size; float multiplier;
  int method, ksize, detect;       // method 0 median, 1 interpolation; detect 0: the mask is the caller's
  unsigned char* mask; float* y;
  const long long* prev; const long long* next;
};
__device__ __forceinline__ double psum(const ClickArgs& p, long long i) { return i <= 0 ? 0.0 : p.P[i]; }      // sum of squares of [0, i)

// mask[i] = |x[i]| > multiplier * sqrt(uniform_filter1d(x^2, size)[i]); the window is [i - size / 2, i - size / 2 + size) (scipy's placement for even
// and odd sizes), reflected at both ends.  Median method: y is written here as well (the median of the UNMODIFIED input at click positions).
__global__ __launch_bounds__(256) void click_mask_kernel(const ClickArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const float v = p.x[i];
  bool click;
  if (p.detect) {
    const long long a = i - p.size / 2, b = a + p.size;               // n >= size: a >= -n and b <= 2 n
    const long long a0 = a < 0 ? 0 : a, b0 = b > p.n ? p.n : b;
    double sum = psum(p, b0) - psum(p, a0);
    if (a < 0) sum += psum(p, -a);                                   // samples -1 .. a are samples 0 .. -a - 1
    if (b > p.n) sum += psum(p, p.n) - psum(p, 2 * p.n - b);          // samples n .. b - 1 are samples n - 1 .. 2 n - b
    const float mean = (float)(sum / (double)p.size);
    const float thr = __fmul_rn(p.multiplier, __fsqrt_rn(mean));
    click = fabsf(v) > thr;
    p.mask[i] = click ? 1 : 0;
  } else {
    click = p.mask[i] != 0;
  }
  if (p.method != 0) return;
  float out = v;
  if (click) {
    float w[kMaxClickKernel];
    const int k = p.ksize, h = k / 2;
    for (int j = 0; j < k; ++j) sorted_insert(w, j, p.x[reflect_index(i - h + j, p.n)]);      // insertion sort of the k neighbours
    out = w[h];
  }
  p.y[i] = out;
}
// interpolation method: a click between two non-click samples lies on their chord; before the first / behind the last non-click sample on the
// line through the two outermost ones (interp1d(..., fill_value="extrapolate")).  The difference of the two samples is taken in float32 as
// interp1d takes it, slope and value in float64.  Fewer than two non-click samples: nothing to interpolate from, clicks are left as they are.
__global__ __launch_bounds__(256) void click_interp_kernel(const ClickArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  float out = p.x[i];
  if (p.mask[i]) {
    long long l = p.prev[i], r = p.next[i];
    if (l < 0 && r < p.n) { l = r; r = l + 1 < p.n ? p.next[l + 1] : p.n; }
    else if (r >= p.n && l >= 0) { r = l; l = r - 1 >= 0 ? p.prev[r - 1] : -1; }
    if (l >= 0 && r < p.n) {
      const float yl = p.x[l], yr = p.x[r];
      const double slope = __ddiv_rn((double)__fsub_rn(yr, yl), (double)(r - l));
      out = (float)__dadd_rn(__dmul_rn(slope, (double)(i - l)), (double)yl);
    }
  }
  p.y[i] = out;
}

// launches: 3 (prefix sums) + 1 (mask, median fill); interpolation: + 3 + 3 (index scans) + 1 (fill) = 11; a caller's mask saves the first 3 (4)
void declick(hipStream_t s, const float* x, long long n, int size, float multiplier, int method, int ksize, int detect, float* y, unsigned char* mask) {
  ClickArgs p{};
  p.x = x; p.n = n; p.size = size; p.multiplier = multiplier; p.method = method; p.ksize = ksize; p.detect = detect; p.mask = mask; p.y = y;
  const long long nb = scan_tiles(n);
  RVC_REQUIRE((n + 255) / 256 < (1LL << 31), "too many samples for one call");
  const size_t pbytes = ((size_t)(n + 1) * sizeof(double) + 255) & ~(size_t)255, tbytes = ((size_t)nb * sizeof(double) + 255) & ~(size_t)255;
  const size_t ibytes = method ? (((size_t)n * sizeof(long long) + 255) & ~(size_t)255) : 0;
  char* scr = (char*)stream_scratch(s, 18, pbytes + tbytes + 2 * ibytes);
  double* P = (double*)scr;
  void* part = scr + pbytes;
  p.P = P;
  if (detect) scan_launch(s, SqSumOp{x}, n, (double*)part, StoreP{P});
  const dim3 g((unsigned)((n + 255) / 256));
  if (detect || method == 0) hipLaunchKernelGGL(click_mask_kernel, g, dim3(256), 0, s, p);
  if (method == 0) return;
  long long* prev = (long long*)(scr + pbytes + tbytes);
  long long* next = (long long*)(scr + pbytes + tbytes + ibytes);
  p.prev = prev; p.next = next;
  scan_launch(s, PrevOp{mask}, n, (long long*)part, StoreFwd{prev});
  scan_launch(s, NextOp{mask, n}, n, (long long*)part, StoreRev{next, n});
  hipLaunchKernelGGL(click_interp_kernel, g, dim3(256), 0, s, p);
}

// ================================================================================================ silence gate
// ss[w][f] = sum of squares (float64) of frame f = 0, 1 of window w: the frames of a centred, zero-padded framing with frame = hop = win of the
// window's samples alone, i.e. samples [f win - win / 2, f win - win / 2 + win) of the window clipped to its length (the last window may be short).
__global__ __launch_bounds__(256) void gate_levels_kernel(const float* __restrict__ x, long long n, int win, double* ss) {
  __shared__ double red[256 / 64];
  const long long w0 = (long long)blockIdx.x * win;
  const long long len = min((long long)win, n - w0);
  const int f = blockIdx.y;
  long long a = (long long)f * win - win / 2, b = a + win;
  if (a < 0) a = 0;
  if (b > len) b = len;
  double acc = 0.0;
  for (long long j = a + threadIdx.x; j < b; j += 256) { const double v = (double)x[w0 + j]; acc = fma(v, v, acc); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ss[(long long)blockIdx.x * 2 + f] = (red[0] + red[1]) + (red[2] + red[3]);
}
void gate_levels(hipStream_t s, const float* x, long long n, int win, double* ss, long long n_windows) {
  hipLaunchKernelGGL(gate_levels_kernel, dim3((unsigned)n_windows, 2), dim3(256), 0, s, x, n, win, ss);
}

// The reference's loop over the window levels (dB), with its start / end bookkeeping: a stretch of windows below the threshold that is longer
// than min_size is faded out over `fade` samples from `start` (the beginning of the last loud window) when start > fade, faded in up to `end`
// (the end of the last quiet window) when end < n - fade, and zero in between.  A quiet LAST window closes the stretch itself and zeroes up to n.
long long gate_ranges(const double* level, long long nw, long long n, long long win, long long min_size, long long fade, double threshold,
                      long long* ranges, long long cap) {
  long long nr = 0, start = 0, end = 0;
  auto push = [&](long long b, long long e, long long kind) {
    if (e <= b) return;
    RVC_REQUIRE(nr < cap, "range buffer too small");
    ranges[3 * nr] = b; ranges[3 * nr + 1] = e; ranges[3 * nr + 2] = kind; ++nr;
  };
  for (long long k = 0; k < nw; ++k) {
    const long long i = k * win;
    if (level[k] < threshold) {
      end = i + win;
      if (i >= n - win) {
        if (end - start > min_size) {
          if (start > fade) { push(start, start + fade, 0); start += fade; }
          push(start, n, 1);
          break;
        }
      }
    } else {
      if (end - start > min_size) {
        if (start > fade) { push(start, start + fade, 0); start += fade; }
        long long e = end;
        const bool fade_in = end < n - fade;
        if (fade_in) e -= fade;
        push(start, e, 1);
        if (fade_in) push(e, end, 2);
        end = e;
      }
      start = i;
    }
  }
  return nr;
}

// x[i] for i in range (b, e, kind): kind 0 *= linspace(1, 0, fade)[i - b], 1 = 0, 2 *= linspace(0, 1, fade)[i - b] - float64 ramps as numpy builds
// them (k * step + start, the last element the end point itself), the product rounded to float32.  Ranges are sorted and disjoint.
__global__ __launch_bounds__(256) void gate_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long long n,
                                                         const long long* __restrict__ ranges, int nr, long long fade) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = x[i];
  int lo = 0, hi = nr;                                 // first range whose end is beyond i
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (ranges[3 * mid + 1] <= i) lo = mid + 1; else hi = mid; }
  if (lo < nr && ranges[3 * lo] <= i) {
    const long long kind = ranges[3 * lo + 2], k = i - ranges[3 * lo];
    if (kind == 1) v = 0.f;
    else {
      const double div = (double)(fade - 1);
      double g;
      if (kind == 0) g = k == fade - 1 ? 0.0 : __dadd_rn(__dmul_rn((double)k, __ddiv_rn(-1.0, div)), 1.0);
      else g = k == fade - 1 ? 1.0 : __dadd_rn(__dmul_rn((double)k, __ddiv_rn(1.0, div)), 0.0);
      v = (float)__dmul_rn((double)v, g);
    }
  }
  y[i] = v;
}
void gate_apply(hipStream_t s, const float* x, float* y, long long n, const long long* ranges, int nr, long long fade) {
  RVC_REQUIRE((n + 255) / 256 < (1LL << 31), "too many samples for one call");
  hipLaunchKernelGGL(gate_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n, ranges, nr, fade);
}

// ================================================================================================ reductions: normalise, peak limit
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
// every block takes the samples [blockIdx.x * chunk, (blockIdx.x + 1) * chunk): a fixed order of additions for a given n
__global__ __launch_bounds__(256) void norm_sum_kernel(const float* __restrict__ x, long long n, long long chunk, double* psum_) {
  __shared__ double red[4];
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  double acc = 0.0;
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) acc += (double)x[j];
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) psum_[blockIdx.x] = t;
}
// the mean as float32 from the kFxParts partial sums (every block adds them in the same order)
__device__ __forceinline__ float norm_mean(const double* psum_, long long n, double* red) {
  double acc = 0.0;
  for (int j = threadIdx.x; j < kFxParts; j += 256) acc += psum_[j];
  return (float)(block_sum(acc, red) / (double)n);
}
__global__ __launch_bounds__(256) void norm_peak_kernel(const float* __restrict__ x, long long n, long long chunk, const double* psum_, float* pmax) {
  __shared__ double red[4];
  __shared__ float redf[4];
  const float m = norm_mean(psum_, n, red);
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  float a = 0.f;
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) a = fmaxf(a, fabsf(__fsub_rn(x[j], m)));
  const float t = block_max(a, redf);
  if (threadIdx.x == 0) pmax[blockIdx.x] = t;
}
// y = ((x - mean) / peak) * gain in float32 steps (audio -= mean; audio /= max_peak; audio *= max_db); peak 0: y = x - mean
__global__ __launch_bounds__(256) void norm_scale_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, long long chunk, const double* psum_,
                                                         const float* pmax, float gain) {
  __shared__ double red[4];
  __shared__ float redf[4];
  const float m = norm_mean(psum_, n, red);
  float a = 0.f;
  for (int j = threadIdx.x; j < kFxParts; j += 256) a = fmaxf(a, pmax[j]);
  const float peak = block_max(a, redf);
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) {
    float v = __fsub_rn(x[j], m);
    if (peak > 0.f) v = __fmul_rn(__fdiv_rn(v, peak), gain);
    y[j] = v;
  }
}
void peak_normalize(hipStream_t s, const float* x, long long n, float gain, float* y) {
  char* scr = (char*)stream_scratch(s, 19, kFxParts * (sizeof(double) + sizeof(float)));
  double* ps = (double*)scr;
  float* pm = (float*)(scr + kFxParts * sizeof(double));
  const long long chunk = (n + kFxParts - 1) / kFxParts;
  hipLaunchKernelGGL(norm_sum_kernel, dim3(kFxParts), dim3(256), 0, s, x, n, chunk, ps);
  hipLaunchKernelGGL(norm_peak_kernel, dim3(kFxParts), dim3(256), 0, s, x, n, chunk, ps, pm);
  hipLaunchKernelGGL(norm_scale_kernel, dim3(kFxParts), dim3(256), 0, s, x, y, n, chunk, ps, pm, gain);
}

// remix_audio's limiter: m = max|x| / max_volume (float32); m > 1: x / m
__global__ __launch_bounds__(256) void limit_peak_kernel(const float* __restrict__ x, long long n, long long chunk, float* pmax) {
  __shared__ float redf[4];
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  float a = 0.f;
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) a = fmaxf(a, fabsf(x[j]));
  const float t = block_max(a, redf);
  if (threadIdx.x == 0) pmax[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void limit_scale_kernel(float* __restrict__ x, long long n, long long chunk, const float* pmax, float max_volume) {
  __shared__ float redf[4];
  float a = 0.f;
  for (int j = threadIdx.x; j < kFxParts; j += 256) a = fmaxf(a, pmax[j]);
  const float m = __fdiv_rn(block_max(a, redf), max_volume);
  if (!(m > 1.f)) return;
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) x[j] = __fdiv_rn(x[j], m);
}
void peak_limit(hipStream_t s, float* x, long long n, float max_volume) {
  float* pm = (float*)stream_scratch(s, 19, kFxParts * (sizeof(double) + sizeof(float)));
  const long long chunk = (n + kFxParts - 1) / kFxParts;
  hipLaunchKernelGGL(limit_peak_kernel, dim3(kFxParts), dim3(256), 0, s, x, n, chunk, pm);
  hipLaunchKernelGGL(limit_scale_kernel, dim3(kFxParts), dim3(256), 0, s, x, n, chunk, pm, max_volume);
}

// ================================================================================================ track merge
// out[i] = nanmean / nanmedian / nanmin / nanmax over the tracks, each zero-extended to n_out (pad_audio).  NaN-free input gives numpy's float32
// result: the mean adds in track order (NaN counted as 0, as nanmean replaces it) and divides once by the number of non-NaN values; the median
// of an even count is (a + b) / 2 of the middle pair of the sorted non-NaN values, of an odd count (h + h) / 2 as numpy.ma forms it.
struct MergeArgs { const float* t[4]; long long len[4]; int k, mode; float* out; long long n; };
__global__ __launch_bounds__(256) void merge_kernel(const MergeArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  float v[4]; int c = 0; float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < p.k) {
      const float u = i < p.len[j] ? p.t[j][i] : 0.f;
      const bool nan = u != u;
      sum = __fadd_rn(sum, nan ? 0.f : u);
      if (!nan) v[c++] = u;
    }
  }
  float r = __builtin_nanf("");
  if (c > 0) {
    if (p.mode == 0) r = __fdiv_rn(sum, (float)c);
    else if (p.mode == 2) { r = v[0]; for (int j = 1; j < c; ++j) r = fminf(r, v[j]); }
    else if (p.mode == 3) { r = v[0]; for (int j = 1; j < c; ++j) r = fmaxf(r, v[j]); }
    else {
      for (int a = 1; a < c; ++a) { const float u = v[a]; int q = a; while (q > 0 && v[q - 1] > u) { v[q] = v[q - 1]; --q; } v[q] = u; }
      const float hi = v[c / 2], lo = (c & 1) ? hi : v[c / 2 - 1];
      r = __fmul_rn(__fadd_rn(lo, hi), 0.5f);
    }
  }
  p.out[i] = r;
}
void merge_tracks(hipStream_t s, const float* const* tracks, const long long* lens, int k, int mode, float* out, long long n_out) {
  MergeArgs p{};
  for (int j = 0; j < k; ++j) { p.t[j] = tracks[j]; p.len[j] = lens[j]; }
  p.k = k; p.mode = mode; p.out = out; p.n = n_out;
  RVC_REQUIRE((n_out + 255) / 256 < (1LL << 31), "too many samples for one call");
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, p);
}

// ================================================================================================ segment energy
// np.array_split(x, k): the first n % k segments hold n / k + 1 samples, the others n / k.  One block per segment, exact int64 sums of squares.
__global__ __launch_bounds__(1024) void segment_energy_kernel(const short* __restrict__ x, long long n, int k, long long* out) {
  __shared__ long long red[1024 / 64];
  const long long q = n / k, r = n % k, sidx = blockIdx.x;
  const long long b0 = sidx * q + (sidx < r ? sidx : r), b1 = b0 + q + (sidx < r ? 1 : 0);
  long long acc = 0;
#pragma unroll 8
  for (long long j = b0 + threadIdx.x; j < b1; j += 1024) { const long long v = x[j]; acc += v * v; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { long long t = 0; for (int w = 0; w < 1024 / 64; ++w) t += red[w]; out[sidx] = t; }
}
void segment_energy(hipStream_t s, const short* x, long long n, int k, long long* out) {
  hipLaunchKernelGGL(segment_energy_kernel, dim3((unsigned)k), dim3(1024), 0, s, x, n, k, out);
}

}  // namespace rvc
