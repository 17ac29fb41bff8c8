// Training-set preparation on the device (reference preprocessing_utils.py:13-100 -> lib/slicer2.py): the slicer's forward high-pass, its framed
// RMS, the silence scan (host: a sequential state machine over ~67 frames per second of audio) and the cut of the filtered recording into the
// training windows - every window as float32 and, resampled to 16 kHz and peak-limited, as the HuBERT / pitch input.  A recording costs a fixed
// number of launches however many windows it yields (the per-window route is one rvc_resample launch per window).
#include "rvc_internal.h"
#include "ops.h"
#include "signal_dev.h"

namespace rvc {

// ================================================================================================ forward high-pass (scipy.signal.lfilter)
// y = lfilter(b, a, x) from a zero state, evaluated as the cascade of the filter's second-order sections and block-propagated like the zero-phase
// filter of the conversion path (ops.hip, iir_block_kernel: why the sections form, and the LDS tiles):
//   pass 1  every lane runs one block of kLfBlock samples from a ZERO state -> its final state Z0_c
//   pass 2  z_{c+1} = Z0_c + M z_c over all blocks, M = the state transition over one block.  Blocks are taken in groups of kLfGroup: a lane
//           chains its group from zero (a), ONE lane chains the groups with Mg = M^kLfGroup through LDS (b), every lane chains its group again
//           from the group's true state and leaves each block's initial state where Z0_c was (c).  The length of (b) is n / 65536 steps.
//   pass 3  every lane runs its block again from its true initial state and writes the outputs.
// 5 launches for any n.  The states of block c live at lf_slot(c): lanes of pass 2 (a, c) that walk neighbouring groups read neighbouring rows.
constexpr int kLfBlock = 256, kLfTile = 32, kLfGroup = 256, kLfChain = 1024;
struct LfArgs {
  double sos[3][6];
  double M[kSosN * kSosN], Mg[kSosN * kSosN];
  const void* x; int is64;
  long long n, nb, ng;            // samples, blocks, groups
  double* y;
  double* Z;                      // [kLfGroup][ng][6]
  double* V;                      // [ng][6]
};
__device__ __forceinline__ long long lf_slot(const LfArgs& p, long long c) { return ((c % kLfGroup) * p.ng + c / kLfGroup) * kSosN; }

template <bool OUT>
__global__ __launch_bounds__(64) void lf_block_kernel(const LfArgs p) {
  __shared__ double tile[2][64][kLfTile + 1];
  __shared__ double ytile[OUT ? 64 : 1][kLfTile + 1];
  const int lane = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * 64, c = c0 + lane;
  double z[kSosN];
#pragma unroll
  for (int i = 0; i < kSosN; ++i) z[i] = (OUT && c < p.nb) ? p.Z[lf_slot(p, c) + i] : 0.0;
  const int lr = lane >> 5, lc = lane & 31;              // loader: two rows of 32 samples per pass (256-byte rows, coalesced)
  auto load_tile = [&](int t, double (&v)[32]) {
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const long long j = (c0 + 2 * k + lr) * kLfBlock + t * kLfTile + lc;
      v[k] = j < p.n ? (p.is64 ? ((const double*)p.x)[j] : (double)((const float*)p.x)[j]) : 0.0;       // zero input behind the end
    }
  };
  double v[32];
  load_tile(0, v);
  constexpr int ntile = kLfBlock / kLfTile;
  for (int t = 0; t < ntile; ++t) {
    double (*tl)[kLfTile + 1] = tile[t & 1];
#pragma unroll
    for (int k = 0; k < 32; ++k) tl[2 * k + lr][lc] = v[k];
    if (t + 1 < ntile) load_tile(t + 1, v);                // in flight under this tile's recurrence
    __syncthreads();
#pragma unroll 8
    for (int sidx = 0; sidx < kLfTile; ++sidx) {
      const double y = sos_cascade_step(p.sos, z, tl[lane][sidx]);
      if (OUT) ytile[lane][sidx] = y;
    }
    if (OUT) {
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < 32; ++k) {
        const int row = 2 * k + lr;
        const long long j = (c0 + row) * kLfBlock + t * kLfTile + lc;
        if (j < p.n) p.y[j] = ytile[row][lc];
      }
      __syncthreads();
    }
  }
  if (!OUT && c < p.nb) {
#pragma unroll
    for (int i = 0; i < kSosN; ++i) p.Z[lf_slot(p, c) + i] = z[i];
  }
}

__device__ __forceinline__ void lf_advance(double (&z)[kSosN], const double (&z0)[kSosN], const double (&Mx)[kSosN * kSosN]) {
  double zn[kSosN];
#pragma unroll
  for (int i = 0; i < kSosN; ++i) {
    double a = z0[i];
#pragma unroll
    for (int j = 0; j < kSosN; ++j) a = fma(Mx[i * kSosN + j], z[j], a);
    zn[i] = a;
  }
#pragma unroll
  for (int i = 0; i < kSosN; ++i) z[i] = zn[i];
}
// pass 2 (a) / (c): one lane per group.  FINAL false: from zero, the group's final state -> V;  true: from V, each block's initial state -> Z
template <bool FINAL>
__global__ __launch_bounds__(256) void lf_group_kernel(const LfArgs p) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= p.ng) return;
  double Mr[kSosN * kSosN], z[kSosN];
#pragma unroll
  for (int i = 0; i < kSosN * kSosN; ++i) Mr[i] = p.M[i];
#pragma unroll
  for (int i = 0; i < kSosN; ++i) z[i] = FINAL ? p.V[g * kSosN + i] : 0.0;
  for (int i = 0; i < kLfGroup; ++i) {
    if (g * kLfGroup + i >= p.nb) break;
    double* q = p.Z + ((long long)i * p.ng + g) * kSosN;
    double z0[kSosN];
#pragma unroll
    for (int k = 0; k < kSosN; ++k) { z0[k] = q[k]; if (FINAL) q[k] = z[k]; }
    lf_advance(z, z0, Mr);
  }
  if (!FINAL) {
#pragma unroll
    for (int i = 0; i < kSosN; ++i) p.V[g * kSosN + i] = z[i];
  }
}
// pass 2 (b): V_g (final state of group g from zero) -> the true initial state of group g; kLfChain groups at a time through LDS
__global__ __launch_bounds__(256) void lf_chain_kernel(const LfArgs p) {
  __shared__ double v[kLfChain * kSosN];
  __shared__ double carry[kSosN];
  const int tid = threadIdx.x;
  if (tid < kSosN) carry[tid] = 0.0;
  for (long long base = 0; base < p.ng; base += kLfChain) {
    const int cnt = (int)min((long long)kLfChain, p.ng - base);
    for (int i = tid; i < cnt * kSosN; i += 256) v[i] = p.V[base * kSosN + i];
    __syncthreads();
    if (tid == 0) {
      double Mr[kSosN * kSosN], z[kSosN];
#pragma unroll
      for (int i = 0; i < kSosN * kSosN; ++i) Mr[i] = p.Mg[i];
#pragma unroll
      for (int i = 0; i < kSosN; ++i) z[i] = carry[i];
      for (int l = 0; l < cnt; ++l) {
        double z0[kSosN];
#pragma unroll
        for (int k = 0; k < kSosN; ++k) { z0[k] = v[l * kSosN + k]; v[l * kSosN + k] = z[k]; }
        lf_advance(z, z0, Mr);
      }
#pragma unroll
      for (int i = 0; i < kSosN; ++i) carry[i] = z[i];
    }
    __syncthreads();
    for (int i = tid; i < cnt * kSosN; i += 256) p.V[base * kSosN + i] = v[i];
    __syncthreads();
  }
}

void lfilter_sos(hipStream_t s, const void* x, int is64, long long n, const double* sos18, double* y) {
  LfArgs p{};
  for (int k = 0; k < 3; ++k) {
    RVC_REQUIRE(sos18[k * 6 + 3] == 1.0, "sos sections must be normalised (a0 = 1)");
    for (int i = 0; i < 6; ++i) p.sos[k][i] = sos18[k * 6 + i];
  }
  p.x = x; p.is64 = is64; p.n = n; p.y = y;
  p.nb = (n + kLfBlock - 1) / kLfBlock;
  p.ng = (p.nb + kLfGroup - 1) / kLfGroup;
  RVC_REQUIRE((p.nb + 63) / 64 < (1LL << 31), "recording too long");
  sos_transition(p.sos, kLfBlock, p.M);
  // Mg = M^kLfGroup by squaring (entries stay O(1): the sections form again)
  static_assert(kLfGroup == 256, "eight squarings");
  double a[kSosN * kSosN], b[kSosN * kSosN];
  for (int i = 0; i < kSosN * kSosN; ++i) a[i] = p.M[i];
  for (int q = 0; q < 8; ++q) {
    for (int i = 0; i < kSosN; ++i)
      for (int j = 0; j < kSosN; ++j) {
        double acc = 0.0;
        for (int k = 0; k < kSosN; ++k) acc = std::fma(a[i * kSosN + k], a[k * kSosN + j], acc);
        b[i * kSosN + j] = acc;
      }
    for (int i = 0; i < kSosN * kSosN; ++i) a[i] = b[i];
  }
  for (int i = 0; i < kSosN * kSosN; ++i) p.Mg[i] = a[i];
  double* st = (double*)stream_scratch(s, 16, (size_t)(p.ng * kLfGroup + p.ng) * kSosN * sizeof(double));
  p.Z = st; p.V = st + (size_t)p.ng * kLfGroup * kSosN;
  const dim3 gb((unsigned)((p.nb + 63) / 64)), gg((unsigned)((p.ng + 255) / 256));
  hipLaunchKernelGGL((lf_block_kernel<false>), gb, dim3(64), 0, s, p);
  hipLaunchKernelGGL((lf_group_kernel<false>), gg, dim3(256), 0, s, p);
  hipLaunchKernelGGL(lf_chain_kernel, dim3(1), dim3(256), 0, s, p);
  hipLaunchKernelGGL((lf_group_kernel<true>), gg, dim3(256), 0, s, p);
  hipLaunchKernelGGL((lf_block_kernel<true>), gb, dim3(64), 0, s, p);
}

// ================================================================================================ silence scan (host)
// Which stretches of the recording the slicer drops, as (begin, end) frame pairs over the RMS list.  A frame below the threshold is silent.  When
// a silent run [s, i) ends at the first loud frame i it is cut if it is the LEADING silence and i > max_sil_kept, or if it lasted >= min_interval
// frames and the clip since the last cut is >= min_length frames.  Where it is cut depends on its length: up to max_sil_kept frames at its
// quietest frame (nothing dropped); up to 2 max_sil_kept between the quietest frame of its first and of its last max_sil_kept frames, widened to
// the quietest frame of the middle range; longer, between those two alone.  A trailing silence of >= min_interval frames is dropped from the
// quietest of its first max_sil_kept frames on, tagged (pos, total + 1).  n_samples <= min_length (a sample count against a frame count, as
// the reference compares them) means no scan: the whole recording is one clip.
static long long argmin_range(const double* v, long long a, long long b, long long n) {      // first smallest of v[a:b] clipped to [0, n)
  if (b > n) b = n;
  long long best = a;
  for (long long i = a + 1; i < b; ++i) if (v[i] < v[best]) best = i;
  return best;
}
long long slice_tags(const double* rms, long long nf, long long n_samples, double threshold, long long min_length, long long min_interval,
                     long long max_sil_kept, long long* tags, long long cap) {
  if (n_samples <= min_length) return 0;
  long long nt = 0, sil = -1, clip = 0;
  auto push = [&](long long b, long long e) {
    RVC_REQUIRE(nt < cap, "tag buffer too small");
    tags[2 * nt] = b; tags[2 * nt + 1] = e; ++nt;
  };
  for (long long i = 0; i < nf; ++i) {
    if (rms[i] < threshold) { if (sil < 0) sil = i; continue; }
    if (sil < 0) continue;
    const bool leading = sil == 0 && i > max_sil_kept;
    const bool middle = i - sil >= min_interval && i - clip >= min_length;
    if (leading || middle) {
      const long long run = i - sil;
      if (run <= max_sil_kept) {
        const long long pos = argmin_range(rms, sil, i + 1, nf);
        push(sil == 0 ? 0 : pos, pos);
        clip = pos;
      } else {
        const long long pos_l = argmin_range(rms, sil, sil + max_sil_kept + 1, nf);
        const long long pos_r = argmin_range(rms, i - max_sil_kept, i + 1, nf);
        long long lo = pos_l, hi = pos_r;
        if (run <= 2 * max_sil_kept) {
          const long long pos = argmin_range(rms, i - max_sil_kept, sil + max_sil_kept + 1, nf);
          lo = pos_l < pos ? pos_l : pos;
          hi = pos_r > pos ? pos_r : pos;
        }
        if (sil == 0) { push(0, pos_r); clip = pos_r; }
        else { push(lo, hi); clip = hi; }
      }
    }
    sil = -1;
  }
  if (sil >= 0 && nf - sil >= min_interval) {
    const long long end = nf < sil + max_sil_kept ? nf : sil + max_sil_kept;
    push(argmin_range(rms, sil, end + 1, nf), nf + 1);
  }
  return nt;
}

// ================================================================================================ windows
// filt [n] float64 and a table of (start, length) windows -> gt: the windows as float32, packed; y16: every window resampled to `target` Hz
// by the polyphase definition of rvc_resample (zero extension at the WINDOW's edges, output length ceil(length * target / sr)), packed, then
// divided by m = max|y| / max_volume where m > 1 (lib/audio.py::remix_audio, float32 arithmetic).  Four launches: packed offsets, cast,
// resample + per-window peak, scale.  Reads outside [0, n) give zero and writes stop at the caller's totals, whatever the table holds.
struct CutArgs {
  const double* filt; long long n;
  const long long* win; int nw;
  long long* off_gt; long long* off_16;     // [nw + 1] each
  unsigned* peak;                           // [nw] bits of max|y16| (non-negative floats order like their bits)
  const double* h; int half, U, D; double ratio_num, ratio_den;
  float* gt; float* y16; long long total_gt, total_16;
  float max_volume;
};
__device__ __forceinline__ long long cut_len16(const CutArgs& p, long long len) { return (long long)ceil((double)len * p.ratio_num / p.ratio_den); }

__global__ __launch_bounds__(256) void cut_offsets_kernel(const CutArgs p) {
  __shared__ long long sg[257], s16[257];
  const int tid = threadIdx.x, per = (p.nw + 255) / 256;
  const int w0 = min(tid * per, p.nw), w1 = min(w0 + per, p.nw);
  long long ag = 0, a16 = 0;
  for (int w = w0; w < w1; ++w) { const long long len = max(p.win[2 * w + 1], 0LL); ag += len; a16 += cut_len16(p, len); }
  sg[tid + 1] = ag; s16[tid + 1] = a16;
  __syncthreads();
  if (tid == 0) { sg[0] = 0; s16[0] = 0; for (int i = 1; i <= 256; ++i) { sg[i] += sg[i - 1]; s16[i] += s16[i - 1]; } }
  __syncthreads();
  ag = sg[tid]; a16 = s16[tid];
  for (int w = w0; w < w1; ++w) {
    p.off_gt[w] = ag; p.off_16[w] = a16; p.peak[w] = 0u;
    const long long len = max(p.win[2 * w + 1], 0LL);
    ag += len; a16 += cut_len16(p, len);
  }
  if (tid == 255) { p.off_gt[p.nw] = sg[256]; p.off_16[p.nw] = s16[256]; }
}
// the window that packed element i belongs to: off[w] <= i < off[w + 1] (empty windows are stepped over); -1 behind the last
__device__ __forceinline__ int cut_find(const long long* __restrict__ off, int nw, long long i) {
  if (i >= off[nw]) return -1;
  int lo = 0, hi = nw;                       // off[lo] <= i < off[hi]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
  return lo;
}
__global__ __launch_bounds__(256) void cut_gt_kernel(const CutArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total_gt) return;
  const int w = cut_find(p.off_gt, p.nw, i);
  if (w < 0) return;
  const long long j = p.win[2 * w] + (i - p.off_gt[w]);
  p.gt[i] = (j >= 0 && j < p.n) ? (float)p.filt[j] : 0.f;
}
__global__ __launch_bounds__(256) void cut_resample_kernel(const CutArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int w = i < p.total_16 ? cut_find(p.off_16, p.nw, i) : -1;
  float a = 0.f;
  if (w >= 0) {
    const long long start = p.win[2 * w], len = p.win[2 * w + 1];
    const double* __restrict__ f = p.filt; const long long n = p.n;
    const double acc = polyphase_sum([&](long long m) { const long long j = start + m; return (j >= 0 && j < n) ? (float)f[j] : 0.f; },
                                     len, p.h, p.half, p.U, p.D, i - p.off_16[w]);
    const float y = (float)acc;
    p.y16[i] = y;
    a = fabsf(y);
  }
  // one atomic per wave where the whole wave lies in one window (almost always), else one per lane
  const int w_first = __shfl(w, 0);
  if (__all(w == w_first)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    if ((threadIdx.x & 63) == 0 && w >= 0) atomicMax(p.peak + w, __float_as_uint(a));
  } else if (w >= 0) {
    atomicMax(p.peak + w, __float_as_uint(a));
  }
}
__global__ __launch_bounds__(256) void cut_limit_kernel(const CutArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total_16) return;
  const int w = cut_find(p.off_16, p.nw, i);
  if (w < 0) return;
  const float m = __fdiv_rn(__uint_as_float(p.peak[w]), p.max_volume);
  if (m > 1.f) p.y16[i] = __fdiv_rn(p.y16[i], m);
}

void cut_windows(hipStream_t s, const double* filt, long long n, const long long* win, int nw, int sr, int target, const double* taps, int half,
                 int up, int down, float max_volume, float* gt, long long total_gt, float* y16, long long total_16) {
  if (nw <= 0) return;
  CutArgs p{};
  p.filt = filt; p.n = n; p.win = win; p.nw = nw;
  char* scr = (char*)stream_scratch(s, 17, (size_t)(2 * (nw + 1)) * sizeof(long long) + (size_t)nw * sizeof(unsigned));
  p.off_gt = (long long*)scr; p.off_16 = p.off_gt + (nw + 1); p.peak = (unsigned*)(p.off_16 + (nw + 1));
  p.h = taps; p.half = half; p.U = up; p.D = down; p.ratio_num = (double)target; p.ratio_den = (double)sr;
  p.gt = gt; p.y16 = y16; p.total_gt = total_gt; p.total_16 = total_16; p.max_volume = max_volume;
  RVC_REQUIRE((total_gt + 255) / 256 < (1LL << 31) && (total_16 + 255) / 256 < (1LL << 31), "too many samples for one call");
  hipLaunchKernelGGL(cut_offsets_kernel, dim3(1), dim3(256), 0, s, p);
  if (total_gt > 0) hipLaunchKernelGGL(cut_gt_kernel, dim3((unsigned)((total_gt + 255) / 256)), dim3(256), 0, s, p);
  if (total_16 > 0) {
    const dim3 g((unsigned)((total_16 + 255) / 256));
    hipLaunchKernelGGL(cut_resample_kernel, g, dim3(256), 0, s, p);
    hipLaunchKernelGGL(cut_limit_kernel, g, dim3(256), 0, s, p);
  }
}

}  // namespace rvc
