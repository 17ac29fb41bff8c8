// Device helpers with ONE definition.  Arithmetic shared by the input high-pass of the conversion path (ops.hip: filtfilt) and the dataset preparation (dataset_prep.hip: lfilter,
// windowed resampling): ONE definition each of the second-order-section step, of the state transition of a block and of the polyphase tap
// sum, so the two users cannot drift apart (the dataset path is tested bit for bit against rvc_resample).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace rvc {

// float64 sum over a 256-thread block in a fixed order (red: 4 doubles of LDS): the block-partial reductions of audio_fx.hip and train_forward.hip
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// scipy.ndimage's "reflect" boundary (d c b a | a b c d | d c b a): the edge sample is repeated.  One reflection: -n <= j < 2 n
__host__ __device__ __forceinline__ long long reflect_index(long long j, long long n) { return j < 0 ? -j - 1 : (j >= n ? 2 * n - 1 - j : j); }

// w[0 .. j) ascending: u is inserted in order (step j of an insertion sort).  After k steps w[k / 2] is the median of the k values of an odd window -
// one of its inputs, so the median filters of audio_fx.hip (declick) and aux_losses.hip (HPSS) are exact whatever the order of insertion.
// STRIDE: elements between neighbours of the list (a per-thread list interleaved with the other threads' in LDS).
template <int STRIDE = 1>
__device__ __forceinline__ void sorted_insert(float* w, int j, float u) {
  int q = j;
  while (q > 0 && w[(q - 1) * STRIDE] > u) { w[q * STRIDE] = w[(q - 1) * STRIDE]; --q; }
  w[q * STRIDE] = u;
}

constexpr int kSosN = 6;      // states of the cascade: 2 per section, 3 sections (a 5th-order filter: the last section is first order, b2 = a2 = 0)

// one sample through the cascade sos[k] = {b0, b1, b2, 1, a1, a2} (direct form II transposed per section, float64)
__host__ __device__ __forceinline__ double sos_cascade_step(const double (&sos)[3][6], double (&z)[kSosN], double x) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double y = fma(sos[k][0], x, z[2 * k]);
    z[2 * k] = fma(-sos[k][4], y, fma(sos[k][1], x, z[2 * k + 1]));
    z[2 * k + 1] = fma(-sos[k][5], y, sos[k][2] * x);
    x = y;
  }
  return x;
}

// M [6][6]: column j = the cascade's state after `steps` zero-input samples from the unit state e_j (the recurrence itself: O(1) entries)
inline void sos_transition(const double (&sos)[3][6], long long steps, double* M) {
  for (int j = 0; j < kSosN; ++j) {
    double z[kSosN] = {0, 0, 0, 0, 0, 0};
    z[j] = 1.0;
    for (long long t = 0; t < steps; ++t) sos_cascade_step(sos, z, 0.0);
    for (int i = 0; i < kSosN; ++i) M[i * kSosN + j] = z[i];
  }
}

// output n of the rational resampler (ops.hip: resample_kernel): sum_m x(m) h[m U - n D + half] over the taps that meet [0, n_in), ascending m,
// float64 accumulation; x(m) returns sample m as float32
template <class X>
__device__ __forceinline__ double polyphase_sum(X x, long long n_in, const double* __restrict__ h, int half, int U, int D, long long n) {
  const long long c = n * D;                       // position of output n on the up-sampled grid
  long long lo = c - half, hi = c + half;
  long long m0 = lo <= 0 ? 0 : (lo + U - 1) / U;   // ceil(lo / U), clamped to the signal
  long long m1 = hi / U;                           // floor (hi >= 0)
  if (m1 > n_in - 1) m1 = n_in - 1;
  double acc = 0.0;
  for (long long m = m0; m <= m1; ++m) acc += (double)x(m) * h[m * U - c + half];
  return acc;
}

}  // namespace rvc
