// Element-wise kernels and reductions of the training forward (model_synth.hip::synth_forward) and of the two reconstruction losses:
//   posterior sampling  z = m_q + noise exp(logs_q)                  (reference lib/infer_pack/models.py:235-237, full mask: one item at its own length)
//   segment gather      columns [ids, ids + seg) of a [C][T] tensor  (lib/infer_pack/commons.py:150-166 slice_segments / slice_segments2)
//   kl_loss             sum of logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p) over the unmasked columns (lib/train/losses.py:596-611)
//   l1 sum              sum |a - b|                                  (F.l1_loss, training_cli.py:570)
//   kl_loss backward    the four cotangents of that sum, element-wise (what loss_gen_all.backward() sends into z_p, logs_q, m_p, logs_p)
// The reductions accumulate in float64 in a fixed order: kLossParts blocks each sum a contiguous chunk (thread-strided, then block_sum), ONE block adds
// the partials in index order.  No floating-point atomics: two calls give the same bits.
#include "rvc_internal.h"
#include "models.h"
#include "signal_dev.h"

namespace rvc {

constexpr int kLossParts = 256;      // blocks of a reduction

__global__ __launch_bounds__(256) void posterior_sample_kernel(const float* __restrict__ stats, const float* __restrict__ noise, float* __restrict__ z, long long n) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long st = (long long)gridDim.x * 256;
  for (; i < n; i += st) z[i] = stats[i] + noise[i] * expf(stats[n + i]);
}
void posterior_sample(hipStream_t s, const float* stats, const float* noise, float* z, int C, int T) {
  const long long n = (long long)C * T;
  const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(posterior_sample_kernel, dim3(blocks), dim3(256), 0, s, stats, noise, z, n);
}

__global__ __launch_bounds__(256) void segment_gather_kernel(const float* __restrict__ x, int T, int ids, int seg, float* __restrict__ y, long long n) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long st = (long long)gridDim.x * 256;
  for (; i < n; i += st) { const long long c = i / seg; const int t = (int)(i - c * seg); y[i] = x[c * T + ids + t]; }
}
void segment_gather(hipStream_t s, const float* x, int C, int T, int ids, int seg, float* y) {
  RVC_REQUIRE(ids >= 0 && seg > 0 && ids + seg <= T, "segment outside the sequence");
  const long long n = (long long)C * seg;
  const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(segment_gather_kernel, dim3(blocks), dim3(256), 0, s, x, T, ids, seg, y, n);
}

struct KlTerm {
  const float* z_p; const float* logs_q; const float* m_p; const float* logs_p; long long ldT, len;
  // element j of the C x len unmasked block, in fp32 steps like the reference's tensor expression
  __device__ __forceinline__ double operator()(long long j) const {
    const long long c = j / len, i = c * ldT + (j - c * len);
    const float lp = logs_p[i], d = z_p[i] - m_p[i];
    const float kl = (lp - logs_q[i]) - 0.5f;
    return (double)(kl + (0.5f * (d * d)) * expf(-2.0f * lp));
  }
};
struct L1Term {
  const float* a; const float* b;
  __device__ __forceinline__ double operator()(long long j) const { return (double)fabsf(a[j] - b[j]); }
};
template <class Term>
__global__ __launch_bounds__(256) void loss_partial_kernel(Term term, long long n, long long chunk, double* part) {
  __shared__ double red[4];
  const long long b0 = (long long)blockIdx.x * chunk, b1 = min(b0 + chunk, n);
  double acc = 0.0;
  for (long long j = b0 + threadIdx.x; j < b1; j += 256) acc += term(j);
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ part, double* out, double count, int has_count) {
  __shared__ double red[4];
  const double t = block_sum(threadIdx.x < kLossParts ? part[threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) { out[0] = t; if (has_count) out[1] = count; }
}
static_assert(kLossParts <= 256, "one block adds the partials");

template <class Term>
static void loss_sum(hipStream_t s, const Term& term, long long n, double* out, double count, int has_count) {
  double* part = (double*)stream_scratch(s, 20, kLossParts * sizeof(double));
  const long long chunk = (n + kLossParts - 1) / kLossParts;
  hipLaunchKernelGGL(loss_partial_kernel<Term>, dim3(kLossParts), dim3(256), 0, s, term, n, chunk, part);
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, part, out, count, has_count);
}
void kl_loss_sum(hipStream_t s, const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, int C, long long ldT, long long len, double* out2) {
  RVC_REQUIRE(C > 0 && len > 0 && len <= ldT, "kl_loss: 0 < len <= T_pitch expected");
  loss_sum(s, KlTerm{z_p, logs_q, m_p, logs_p, ldT, len}, (long long)C * len, out2, (double)len, 1);
}
// kl_loss's backward for one item: with r = (z_p - m_p) exp(-2 logs_p), d z_p = scale r, d m_p = -scale r, d logs_q = -scale,
// d logs_p = scale (1 - (z_p - m_p) r) for t < len and exactly 0 behind; float64 from the float32 inputs, rounded once.
__global__ __launch_bounds__(256) void kl_loss_grad_kernel(const float* __restrict__ z_p, const float* __restrict__ m_p, const float* __restrict__ logs_p, long long ldT,
                                                           long long len, long long n, double scale, float* __restrict__ dz_p, float* __restrict__ dlogs_q,
                                                           float* __restrict__ dm_p, float* __restrict__ dlogs_p) {
  const long long st = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) {
    float gz = 0.f, gq = 0.f, gm = 0.f, gp = 0.f;
    if (i % ldT < len) {
      const double d = (double)z_p[i] - (double)m_p[i], r = d * exp(-2.0 * (double)logs_p[i]);
      gz = (float)(scale * r); gm = (float)(-(scale * r)); gq = (float)(-scale); gp = (float)(scale * (1.0 - d * r));
    }
    dz_p[i] = gz; dlogs_q[i] = gq; dm_p[i] = gm; dlogs_p[i] = gp;
  }
}
void kl_loss_grad(hipStream_t s, const float* z_p, const float* m_p, const float* logs_p, int C, long long ldT, long long len, float scale, float* dz_p,
                  float* dlogs_q, float* dm_p, float* dlogs_p) {
  RVC_REQUIRE(C > 0 && ldT > 0 && len >= 0 && len <= ldT, "kl_loss_grad: 0 <= len <= T_pitch expected");
  const long long n = (long long)C * ldT;
  const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(kl_loss_grad_kernel, dim3(blocks), dim3(256), 0, s, z_p, m_p, logs_p, ldT, len, n, (double)scale, dz_p, dlogs_q, dm_p, dlogs_p);
}
void l1_sum(hipStream_t s, const float* a, const float* b, long long n, double* out1) {
  RVC_REQUIRE(n > 0, "l1_sum: n > 0 expected");
  loss_sum(s, L1Term{a, b}, n, out1, 0.0, 0);
}

}  // namespace rvc
