// Launch wrappers of the non-GEMM device ops (ops.hip), and the two GELU evaluations every kernel file shares.
#pragma once
#include <hip/hip_runtime.h>

namespace rvc {

// exact-erf GELU (torch F.gelu default) through the library's erff: two divergent paths per element - for kernels that are not bound by it
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }
// exact-erf GELU (torch F.gelu default), branch-free: erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7 absolute, i.e. ~1e-7 of the
// activation - far inside the fp32 noise of the 768-term sums that feed it; ocml's erff takes two divergent paths per element).  What
// conv_x3s.hip's epilogue, HuBERT's fused layer 0 (ops.hip) and the image producers of model_mdx23.hip evaluate: those run at HBM rate
// only if the activation stays under ~20 VALU instructions per value.
__device__ __forceinline__ float gelu_bf(float v) {
  const float x = v * 0.70710678118654752440f, ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * x * x);
  return 0.5f * v * (1.f + copysignf(fmaf(-poly, e, 1.f), x));
}

// LayerNorm over channels that ALSO writes y as the split-resident image of conv_x3s.hip (y may be null: image only); margin = kSplitMargin
void wn_gate_split(hipStream_t s, const float* a, const float* g, unsigned char* img, long long tp, int margin, int H, int T);   // WN gate -> split image only
// HuBERT feature-encoder layer 0 fused: Conv1d(1, C, 10, stride 5) -> GroupNorm(C, C) -> GELU from the raw audio (the convolution is
// evaluated twice instead of being stored: ops.hip).  partial: hubert_conv0_scratch_doubles(C, T1) doubles, stat: 2 C floats.
void hubert_conv0_gn_gelu(hipStream_t s, const float* audio, long long L, const float* w, const float* gamma, const float* beta, int C, int T1, float eps,
                          float* out, long long ld, double* partial, float* stat);
// the same, the result written only as the DE-INTERLEAVED bf16 hi / lo image a stride-2 layer on the split-resident GEMM reads (split_geom_s2; H = split_s2_h(T1), tp = split_s2_tp(T1))
void hubert_conv0_gn_gelu_img(hipStream_t s, const float* audio, long long L, const float* w, const float* gamma, const float* beta, int C, int T1, float eps,
                              unsigned char* img, long long tp, int margin, int H, double* partial, float* stat);
size_t hubert_conv0_scratch_doubles(int C, int T1);
void layernorm_c_split(hipStream_t s, const float* x, const float* gamma, const float* beta, float* y, unsigned char* img, long long tp, int margin,
                       int C, int T, long long ld, float eps);
void layernorm_c(hipStream_t s, const float* x, const float* r, const float* gamma, const float* beta, float* y, int C, int T,
                 long long ld, float eps);
void groupnorm_t_gelu(hipStream_t s, float* x, const float* gamma, const float* beta, int C, int T, long long ld, float eps);
void fill(hipStream_t s, float* p, float v, long long n);
void wn_gate(hipStream_t s, const float* a, const float* g, float* out, int H, int T);
void gemv(hipStream_t s, const float* W, const float* x, const float* b, float* y, int N, int K, const float* add);
void zp_sample(hipStream_t s, const float* stats, const float* noise, float* zp, int C, int T);
void flip_c(hipStream_t s, const float* x, float* y, int C, int T);
void encp_embed(hipStream_t s, float* x, const float* emb, const long long* pitch, int C, int T);
// returns the kernel that ran: 1 = four outputs per thread (k = 7, pad = 3, 16-byte aligned rows), 0 = one output per thread
int conv_to1(hipStream_t s, const float* x, long long ldx, const float* w /*[Ci][K]*/, int Ci, int K, int pad, int T, float pre_slope,
             int act_tanh, float* y);
void resample(hipStream_t s, const float* x, long long n_in, const double* h, int half, int U, int D, float* y, long long n_out);
void transpose(hipStream_t s, const float* in, float* out, int R, int C, long long ldin, long long ldout, int batch, long long bin,
               long long bout);
void feats_prepare(hipStream_t s, const float* f, const float* f0, const float* pitchf, float* out, int D, int Th, int T, float protect,
                   int do_protect);
// x[c][t] += b[c] + sum_j w[c][j] src[t stride + j - pad] for k = 1 / 4 / 8 taps of one source channel (16-byte rows); false: not its shape
bool noise_add(hipStream_t s, float* x, long long ld, int C, int T, const float* src, long long L, int k, int stride, int pad, const float* w, const float* b);
void f0_post(hipStream_t s, const double* f0, long long n, double factor, double mel_min, double mel_max, int bins, long long* pitch, float* pitchf);
void frames(hipStream_t s, const float* src, float* out, int L, int k, int stride, int pad, int Tout, int reflect);
void magnitude(hipStream_t s, const float* ft, float* mag, int F, int T);
void mel_to_unet(hipStream_t s, const float* mel, float* x, int n, int Tr, float a, float b);
void avgpool2(hipStream_t s, const float* x, float* y, int C, int H, int W, long long ldx);
void gru_scan(hipStream_t s, const float* gi, const float* b_ih, const float* w_hh, const float* w_hh_t /* k-major copy for the repair kernel */, const float* b_hh, float* out,
              unsigned long long* xbuf, int* err, int T, unsigned spin_limit = 0, int fault = 0);
void rmvpe_decode(hipStream_t s, const float* sal, double* f0, int n, long long ld, float thred, const int* err = nullptr);
void sine_source(hipStream_t s, const float* f0, const float* noise, float* har, float* sine_out, float* rad, float* tmp, double* bsum,
                 int T, int upp, float sr, float lw, float lb, float* phase_out = nullptr);

size_t preprocess_scratch_doubles(long long n, bool have_sos);   // doubles of scratch preprocess() needs for an input of n samples
void preprocess(hipStream_t s, const void* x, int is64, long long n, const double* b, const double* a, const double* zi, int t_pad,
                double* filt, float* padded, double* rms1, int n1, int frame, int hop, double* scratch, const double* sos = nullptr,
                const double* sos_zi = nullptr);      // sos [3][6] + sosfilt_zi [3][2]: block-propagated cascade evaluation (ops.hip)
void postprocess(hipStream_t s, float* x, long long N, const double* rms1, int n1, int sr2, float rate, short* out, float* rms2, unsigned* maxbits);
// librosa-style centred framed RMS of a float64 signal (zero padding of frame / 2 on both sides): rms [n_frames], one block per frame
void rms_frames_f64(hipStream_t s, const double* x, long long n, int frame, int hop, double* rms, long long n_frames);

// training-set preparation (dataset_prep.hip)
// y = scipy.signal.lfilter(b, a, x) from a zero state for the filter given as three normalised second-order sections (host [3][6]); 5 launches
void lfilter_sos(hipStream_t s, const void* x, int is64, long long n, const double* sos18, double* y);
// the slicer's silence scan over a HOST RMS list: writes (begin, end) frame pairs to tags [cap][2], returns their number
long long slice_tags(const double* rms, long long nf, long long n_samples, double threshold, long long min_length, long long min_interval,
                     long long max_sil_kept, long long* tags, long long cap);
// windows (start, length) [nw][2] (device) of filt -> gt: float32 casts, packed; y16: resampled by up / down (taps: design of rvc_resample) and
// peak-limited to max_volume per window, packed; 4 launches
void cut_windows(hipStream_t s, const double* filt, long long n, const long long* win, int nw, int sr, int target, const double* taps, int half,
                 int up, int down, float max_volume, float* gt, long long total_gt, float* y16, long long total_16);

// audio nodes (audio_fx.hip)
constexpr int kMaxClickKernel = 31;      // largest median window of declick
// ss [n_windows][2]: float64 sums of squares of the (at most two) centred frames of every window of `win` samples; 1 launch
void gate_levels(hipStream_t s, const float* x, long long n, int win, double* ss, long long n_windows);
// the silence gate's scan over HOST window levels (dB): (begin, end, kind) ranges -> ranges [cap][3], kind 0 fade-out, 1 zero, 2 fade-in; returns their number
long long gate_ranges(const double* level, long long nw, long long n, long long win, long long min_size, long long fade, double threshold,
                      long long* ranges, long long cap);
// y = x with the ranges (device [nr][3], sorted, disjoint) applied: float64 linspace ramps of `fade` samples, zeros; 1 launch
void gate_apply(hipStream_t s, const float* x, float* y, long long n, const long long* ranges, int nr, long long fade);
// click mask (|x| > multiplier * local RMS over `size` samples, reflect boundary) -> mask [n]; clicks replaced by the median of ksize neighbours
// (method 0, 4 launches) or by linear interpolation between the nearest non-click samples (method 1, 11 launches) -> y [n]; detect 0: mask is an input
void declick(hipStream_t s, const float* x, long long n, int size, float multiplier, int method, int ksize, int detect, float* y, unsigned char* mask);
// y = (x - mean(x)) / max|x - mean| * gain in float32 steps, mean and peak by float64 / exact device reductions; 3 launches
void peak_normalize(hipStream_t s, const float* x, long long n, float gain, float* y);
// x /= max|x| / max_volume where that exceeds 1 (remix_audio's limiter); 2 launches
void peak_limit(hipStream_t s, float* x, long long n, float max_volume);
// out [n_out] = NaN-ignoring mean (mode 0) / median (1) / min (2) / max (3) over k <= 4 zero-extended tracks; 1 launch
void merge_tracks(hipStream_t s, const float* const* tracks, const long long* lens, int k, int mode, float* out, long long n_out);
// out [k] = exact int64 sum of squares of every np.array_split segment of the int16 samples; 1 launch
void segment_energy(hipStream_t s, const short* x, long long n, int k, long long* out);

// padded 2-D split-resident images (split2d.hip): level changes of RMVPE's U-Net in the layout conv_x3s.hip convolves
void pool2_pad_split(hipStream_t s, const float* x, long long ldx, bool x_padded, int C, int H, int W, float* y, long long ldy, unsigned char* img,
                     long long tp, int margin);
void interleave2_pad_split(hipStream_t s, const float* ph, long long ldp, int Co, int H, int W, float* y, long long ldy, bool y_padded, unsigned char* img,
                           long long tp, int margin);
void pad2d_split(hipStream_t s, const float* x, long long ldx, int C, int H, int W, float* y, long long ldy, unsigned char* img, long long tp, int margin);
void unpad2d(hipStream_t s, const float* x, long long ldx, int C, int H, int W, float* y, long long ldy);

}  // namespace rvc
