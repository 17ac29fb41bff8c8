// Training inputs (reference lib/train/mel_processing.py): the linear magnitude spectrogram of a ragged batch of clips by an LDS FFT, the log-mel
// projection of such a batch through a banded filterbank, the per-scale term of the multi-scale mel loss (lib/train/losses.py:430-561), and the backward
// of the first two with respect to the audio (the log-mel vector-Jacobian product and the mel losses' cotangents; their header is further down).  gfx950,
// plain HIP.
//
// stft_mag_kernel<LOGM, TL, FR>: a workgroup owns FR consecutive frames of one clip, a team of TL lanes per frame.  A real frame of n_fft samples
// (reflect-padded - or, for hop > n_fft, cropped: the frame starts (hop - n_fft) / 2 samples into its hop and nothing is reflected -, clamped,
// Hann-windowed) is packed as M = n_fft / 2 = 2^LOGM complex values (even samples real, odd samples imaginary) in LDS, transformed by an M-point
// radix-4 Stockham FFT (one radix-2 stage when log2 M is odd) and unpacked by the real-input split to bins 0 .. M.  Every stage reads its inputs into
// registers, crosses a barrier and writes the autosorted outputs back into the same LDS rows, so one buffer per frame suffices; the magnitude pass
// then walks [bin][frame] so that the FR frames of a bin leave as one 4 FR-byte store.  The complex spectrum never reaches HBM.  Twiddles and window are
// float64 on the host, rounded once to fp32 and uploaded once per (context, n_fft); the kernel calls no sinf / cosf and no fast-math intrinsic.
//
// Shapes (n_fft: TL lanes per frame x FR frames = threads, LDS):
//   1024, 2048: 64 x 16 = 1024 threads, one wave per frame, 16 frames = one 64-byte store per bin; 72 / 143 KB.  (rvc_spectrogram_batch; unchanged.)
//   256, 512:   16 x 16 =  256 threads, FOUR frames per wave: a 128- / 256-point FFT has 32 / 64 radix-4 butterflies per stage, so one wave per frame
//               would idle half its lanes at 256 and give every lane one butterfly per barrier at 512; a team of 16 lanes does 2 / 4.  17 / 34 KB.
//   4096:       128 x 8 = 1024 threads, EIGHT frames per workgroup, two waves per frame.  Sixteen rows of 2048 complex values would be 262 KB; eight rows
//               (131,200 B with the row pad) plus the 3073 twiddles (24,584 B) are 155,784 B of the CU's 163,840 B - one workgroup per CU either way
//               (four rows + twiddles = 90 KB would not fit twice), so the choice is the largest power of two that fits, and the team is widened to
//               two waves so that the one resident workgroup still brings 16 waves (4 per SIMD) to hide the LDS round trips of 4 butterflies per lane.
//               The magnitude pass's store becomes 8 frames x 4 B = 32 bytes per bin (a wave writes eight such segments).
#include "models.h"
#include "signal_dev.h"

namespace rvc {

constexpr int kSpecFrames = 16;       // frames per workgroup (8 at n_fft 4096, see above): 16 x 4 B = one 64-byte store per bin
constexpr int kSpecRowPad = 2;        // complex values between the frames' LDS rows: frame stride = 4 dwords mod 64, so the magnitude pass's 16 frames x 2 bins
                                      // per half-wave fall on 32 distinct even banks
constexpr int kMelCols = 64;          // frames per workgroup of mel_project_kernel

struct SpecTables { DevBuf<float2> tw; DevBuf<float> win; };                     // tw [3 n_fft / 4 + 1] = exp(-2 pi i t / n_fft), win [n_fft]
struct MelBank {
  int n_fft = 0, n_mels = 0;
  DevBuf<int> rows; DevBuf<float> w;   // rows [n_mels][3] = (first bin, count, offset into w)
  DevBuf<int> cols;                    // the transpose's index, [n_fft / 2 + 1][2] = (first, one past the last) of the rows whose band holds the bin
};
struct SpecState {
  std::mutex mu;
  std::map<int, SpecTables> tables;
  std::map<std::pair<int, int>, MelBank> banks;
};

static SpecState* spec_state(Ctx* ctx) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (!ctx->spec) ctx->spec = new SpecState();
  return ctx->spec;
}
void spec_state_free(Ctx* ctx) { delete ctx->spec; ctx->spec = nullptr; }

static const SpecTables& spec_tables(Ctx* ctx, int n_fft) {   // (std::map nodes are address-stable and a table is never replaced)
  SpecState* st = spec_state(ctx);
  std::lock_guard<std::mutex> lk(st->mu);
  auto it = st->tables.find(n_fft);
  if (it != st->tables.end()) return it->second;
  const int nt = 3 * n_fft / 4 + 1;
  std::vector<float> tw(2 * (size_t)nt), win(n_fft);
  for (int t = 0; t < nt; ++t) {
    double c, s;
    if (t == 0) { c = 1.0; s = 0.0; }
    else if (4 * t == n_fft) { c = 0.0; s = 1.0; }        // the quarter turns exactly, not cos(pi / 2) = 6e-17
    else if (2 * t == n_fft) { c = -1.0; s = 0.0; }
    else if (4 * t == 3 * n_fft) { c = 0.0; s = -1.0; }
    else { const double a = 2.0 * M_PI * (double)t / (double)n_fft; c = std::cos(a); s = std::sin(a); }
    tw[2 * t] = (float)c; tw[2 * t + 1] = (float)(-s);
  }
  for (int n = 0; n < n_fft; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)n_fft));   // torch.hann_window(n_fft), periodic
  SpecTables T;
  T.tw.upload(reinterpret_cast<const float2*>(tw.data()), (size_t)nt);
  T.win.upload(win);
  return st->tables[n_fft] = std::move(T);
}

// Clip tables in device memory, int64 [n_clips][4]: (sample offset, samples, first output column, first workgroup of the clip).  The workgroup finds
// its clip by bisection over the last column.
struct SpecArgs {
  const float* audio; const long long* clips; int n_clips;
  int hop, pad; float eps; int clamp;
  const float2* tw; const float* win;
  float* out; long long pitch;
};

__device__ __forceinline__ int clip_of_block(const long long* clips, int n_clips, long long block) {
  int lo = 0, hi = n_clips - 1;                     // largest c with clips[c][3] <= block (clips[0][3] = 0)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (clips[4 * (long long)mid + 3] <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// frame fr of the clip at x (ns samples) into the team's row: samples through the reflect index, clamp, window, packed pairs
template <int LOGM, int TL>
__device__ __forceinline__ void load_frame(const SpecArgs& a, float2* z, const float* x, long long ns, long long fr, bool live, int lane) {
  constexpr int M = 1 << LOGM;
  for (int m = lane; m < M; m += TL) {
    float2 v = make_float2(0.f, 0.f);
    if (live) {
      long long s0 = fr * a.hop + 2 * m - a.pad, s1 = s0 + 1;
      if (s0 < 0) s0 = -s0;
      if (s0 >= ns) s0 = 2 * (ns - 1) - s0;
      if (s1 < 0) s1 = -s1;
      if (s1 >= ns) s1 = 2 * (ns - 1) - s1;
      float x0 = x[s0], x1 = x[s1];
      if (a.clamp) { x0 = fminf(fmaxf(x0, -1.05f), 1.05f); x1 = fminf(fmaxf(x1, -1.05f), 1.05f); }
      v.x = x0 * a.win[2 * m]; v.y = x1 * a.win[2 * m + 1];
    }
    z[m] = v;
  }
}

// M-point forward FFT of the team's row (every thread of the workgroup calls it: the stages cross workgroup barriers): Stockham autosort, inputs
// j + r M / R, outputs (j / Ns) Ns R + j % Ns + r Ns.  The rows are complete behind the caller's barrier and again behind the last one here.
template <int LOGM, int TL>
__device__ __forceinline__ void fft_row(float2* z, const float2* tw, int lane) {
  constexpr int M = 1 << LOGM, Q = M / 4, PER4 = Q / TL;
#pragma unroll
  for (int st = 0; st < LOGM / 2; ++st) {
    const int Ns = 1 << (2 * st);
    float2 v[PER4][4];
#pragma unroll
    for (int i = 0; i < PER4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i][r] = z[lane + TL * i + r * Q];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER4; ++i) {
      const int j = lane + TL * i, k = j & (Ns - 1);
      float2 v0 = v[i][0], v1 = v[i][1], v2 = v[i][2], v3 = v[i][3];
      if (st > 0) {
        const int step = (M / (4 * Ns)) * 2 * k;          // exp(-2 pi i k r / (4 Ns)) in units of the n_fft-th root
        v1 = cmul(v1, tw[step]); v2 = cmul(v2, tw[2 * step]); v3 = cmul(v3, tw[3 * step]);
      }
      const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
      const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y), a3 = make_float2(v1.y - v3.y, v3.x - v1.x);      // -i (v1 - v3)
      const int o = ((j - k) << 2) + k;
      z[o] = make_float2(a0.x + a2.x, a0.y + a2.y);
      z[o + Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
      z[o + 2 * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
      z[o + 3 * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
    }
    __syncthreads();
  }
  if (LOGM & 1) {                                         // the last stage in radix 2: Ns = M / 2, so j % Ns = j
    constexpr int H = M / 2, PER2 = H / TL;
    float2 v[PER2][2];
#pragma unroll
    for (int i = 0; i < PER2; ++i) { v[i][0] = z[lane + TL * i]; v[i][1] = z[lane + TL * i + H]; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER2; ++i) {
      const int j = lane + TL * i;
      const float2 v0 = v[i][0], v1 = cmul(v[i][1], tw[2 * j]);
      z[j] = make_float2(v0.x + v1.x, v0.y + v1.y);
      z[j + H] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
    __syncthreads();
  }
}

// real-input split: X[b] = (Z[b] + conj Z[M - b]) / 2 - (i / 2) e^{-2 pi i b / n_fft} (Z[b] - conj Z[M - b]) with zk = Z[b mod M], zc = Z[(M - b) mod M], t = tw[b]
__device__ __forceinline__ float2 split_bin(float2 zk, float2 zc, float2 t) {
  const float er = 0.5f * (zk.x + zc.x), ei = 0.5f * (zk.y - zc.y);
  const float dr = zk.x - zc.x, di = zk.y + zc.y;
  const float p = t.x * dr - t.y * di, q = t.x * di + t.y * dr;
  return make_float2(er + 0.5f * q, ei - 0.5f * p);
}
// the reference's roundings: spec.pow(2).sum(-1) + eps
__device__ __forceinline__ float bin_mag(float2 X, float eps) { return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(X.x, X.x), __fmul_rn(X.y, X.y)), eps)); }

template <int LOGM, int TL, int FR>
__global__ __launch_bounds__(FR * TL) void stft_mag_kernel(SpecArgs a) {
  constexpr int M = 1 << LOGM, Q = M / 4, S = M + kSpecRowPad, NT = 3 * M / 2 + 1;
  static_assert(Q % TL == 0 && (FR & (FR - 1)) == 0 && FR * TL <= 1024, "a team divides the butterflies of a stage; the magnitude pass masks the frame");
  extern __shared__ float2 spec_lds[];
  float2* Z = spec_lds;                 // [FR][S]
  float2* tw = spec_lds + FR * S;   // [NT]
  const int tid = threadIdx.x, lane = tid % TL, wave = tid / TL;      // lane within the team, team = frame

  const int c = clip_of_block(a.clips, a.n_clips, blockIdx.x);
  const long long* d = a.clips + 4 * (long long)c;
  const long long soff = d[0], ns = d[1], ooff = d[2];
  const long long nf = ns / a.hop;
  const long long f0 = ((long long)blockIdx.x - d[3]) * FR;
  if (f0 >= nf) return;                 // (whole workgroup; cannot happen with the host's prefix: a clip without frames owns no workgroup and loses the bisection)

  for (int t = tid; t < NT; t += FR * TL) tw[t] = a.tw[t];
  float2* z = Z + wave * S;
  load_frame<LOGM, TL>(a, z, a.audio + soff, ns, f0 + wave, f0 + wave < nf, lane);
  __syncthreads();
  fft_row<LOGM, TL>(z, tw, lane);

  // ---- real-input split and magnitude, [bin][frame]
  const int f = tid & (FR - 1);
  const float2* zf = Z + f * S;
  const bool store = f0 + f < nf;
  float* out = a.out + ooff + f0 + f;
  for (int b = tid / FR; b <= M; b += TL) {
    const float mag = bin_mag(split_bin(zf[b & (M - 1)], zf[(M - b) & (M - 1)], tw[b]), a.eps);
    if (store) out[(long long)b * a.pitch] = mag;
  }
}

// host side of both batch calls: the caller's clip list -> the device table (slot of the stream's scratch) with the workgroup prefix
static long long upload_clips(hipStream_t s, int slot, const std::vector<long long>& rows4, int n_clips, const long long** dev) {
  static thread_local std::vector<long long> keep;      // stays alive behind the asynchronous copy
  keep = rows4;
  long long* p = (long long*)stream_scratch(s, slot, (size_t)n_clips * 4 * sizeof(long long));
  RVC_HIP_CHECK(hipMemcpyAsync(p, keep.data(), (size_t)n_clips * 4 * sizeof(long long), hipMemcpyHostToDevice, s));
  *dev = p;
  return 0;
}

template <int LOGM, int TL, int FR>
static void stft_launch(hipStream_t s, long long blocks, const SpecArgs& a) {
  constexpr int M = 1 << LOGM;
  constexpr size_t lds = ((size_t)FR * (M + kSpecRowPad) + 3 * M / 2 + 1) * sizeof(float2);
  static_assert(lds <= 160 * 1024, "the CU has 160 KB of LDS");
  auto kern = stft_mag_kernel<LOGM, TL, FR>;
  RVC_ALLOW_BIG_LDS(kern);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(FR * TL), lds, s, a);
}

// both entries: the checks (nothing is launched or written when one fails), the clip table, the launch.  wide: the multi-scale entry's geometries.
static void stft_batch(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                       int clamp, float* out, long long pitch, bool wide) {
  if (wide) {
    RVC_REQUIRE(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096, "n_fft must be 256, 512, 1024, 2048 or 4096");
    RVC_REQUIRE(hop > 0 && hop <= (1 << 24) && ((n_fft - hop) & 1) == 0, "hop must be positive with n_fft - hop even");
  } else {
    RVC_REQUIRE(n_fft == 1024 || n_fft == 2048, "n_fft must be 1024 or 2048");
    RVC_REQUIRE(hop > 0 && hop <= n_fft && ((n_fft - hop) & 1) == 0, "hop must be in (0, n_fft] with n_fft - hop even");
  }
  RVC_REQUIRE(eps >= 0.f && n_clips >= 0 && pitch >= 0 && n_audio >= 0, "bad argument");
  const int pad = (n_fft - hop) / 2;                  // negative for hop > n_fft: the frame starts -pad samples into its hop, nothing is reflected
  const int frames = n_fft == 4096 ? 8 : kSpecFrames;
  std::vector<long long> rows((size_t)n_clips * 4);
  long long blocks = 0;
  for (int c = 0; c < n_clips; ++c) {
    const long long off = clips[3 * c], n = clips[3 * c + 1], col = clips[3 * c + 2];
    if (pad >= 0) RVC_REQUIRE(n > pad, "a clip must be longer than (n_fft - hop) / 2 samples (reflect padding)");
    else RVC_REQUIRE(n >= hop, "a clip must hold one frame (hop samples when hop > n_fft)");
    RVC_REQUIRE(off >= 0 && off + n <= n_audio, "a clip lies outside the audio buffer");
    RVC_REQUIRE(col >= 0 && col + n / hop <= pitch, "a clip's frames lie outside the output row");
    rows[4 * c] = off; rows[4 * c + 1] = n; rows[4 * c + 2] = col; rows[4 * c + 3] = blocks;
    blocks += (n / hop + frames - 1) / frames;
  }
  RVC_REQUIRE(blocks < (1LL << 31), "too many frames for one call");
  if (blocks == 0) return;
  const SpecTables& T = spec_tables(ctx, n_fft);
  SpecArgs a;
  a.audio = audio; a.n_clips = n_clips; a.hop = hop; a.pad = pad; a.eps = eps; a.clamp = clamp; a.tw = T.tw.p; a.win = T.win.p; a.out = out; a.pitch = pitch;
  upload_clips(s, 20, rows, n_clips, &a.clips);
  switch (n_fft) {
    case 256: stft_launch<7, 16, kSpecFrames>(s, blocks, a); break;
    case 512: stft_launch<8, 16, kSpecFrames>(s, blocks, a); break;
    case 1024: stft_launch<9, 64, kSpecFrames>(s, blocks, a); break;
    case 2048: stft_launch<10, 64, kSpecFrames>(s, blocks, a); break;
    default: stft_launch<11, 128, 8>(s, blocks, a); break;
  }
}

void spectrogram_batch(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                       int clamp, float* out, long long pitch) {
  stft_batch(ctx, s, audio, n_audio, clips, n_clips, n_fft, hop, eps, clamp, out, pitch, false);
}
void spectrogram_batch_ms(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                          int clamp, float* out, long long pitch) {
  stft_batch(ctx, s, audio, n_audio, clips, n_clips, n_fft, hop, eps, clamp, out, pitch, true);
}

// ------------------------------------------------------------------------------------------------ mel
void mel_filterbank_set(Ctx* ctx, int n_fft, int n_mels, const int* first, const int* count, const float* weights) {
  RVC_REQUIRE(n_fft > 0 && (n_fft & 1) == 0 && n_mels > 0 && first && count && weights, "bad argument");
  std::vector<int> rows((size_t)n_mels * 3);
  long long total = 0;
  for (int m = 0; m < n_mels; ++m) {
    RVC_REQUIRE(first[m] >= 0 && count[m] >= 0 && first[m] + count[m] <= n_fft / 2 + 1, "a filter's band lies outside bins 0 .. n_fft / 2");
    rows[3 * m] = first[m]; rows[3 * m + 1] = count[m]; rows[3 * m + 2] = (int)total;
    total += count[m];
  }
  RVC_REQUIRE(total < (1LL << 30), "bad argument");
  std::vector<int> cols((size_t)(n_fft / 2 + 1) * 2, 0);
  for (int m = n_mels - 1; m >= 0; --m)
    for (int b = first[m]; b < first[m] + count[m]; ++b) { cols[2 * b] = m; if (cols[2 * b + 1] == 0) cols[2 * b + 1] = m + 1; }
  SpecState* st = spec_state(ctx);
  std::lock_guard<std::mutex> lk(st->mu);
  MelBank& B = st->banks[std::make_pair(n_fft, n_mels)];
  if (B.rows.p) RVC_HIP_CHECK(hipDeviceSynchronize());      // a replaced bank may still be read by an earlier call
  B.rows.reset(); B.w.reset(); B.cols.reset();
  B.n_fft = n_fft; B.n_mels = n_mels;
  B.rows.upload(rows);
  B.cols.upload(cols);
  B.w.upload(weights, (size_t)total);
}

struct MelArgs {
  const float* spec; long long spec_pitch; const long long* clips; int n_clips;
  const int* rows; const float* w; int n_mels;
  float* mel; long long mel_pitch;
};

// mel[m][t] = log(max(sum_b W[m][b] spec[b][t], 1e-5)): a workgroup owns kMelCols frames of one clip, wave g the rows g, g + 4, ...: the weights are
// wave-uniform, the spectrogram reads run along the frames.  fp32 fma chain over the band in ascending bin order; the logarithm is taken in float64 and
// rounded once, so the floor comes out as the correctly rounded log(1e-5f).
__global__ __launch_bounds__(256) void mel_project_kernel(MelArgs a) {
  const int c = clip_of_block(a.clips, a.n_clips, blockIdx.x);
  const long long* d = a.clips + 4 * (long long)c;
  const long long col0 = d[0], nf = d[1];
  const long long t = ((long long)blockIdx.x - d[3]) * kMelCols + (threadIdx.x & 63);
  if (t >= nf) return;
  const float* sp = a.spec + col0 + t;
  for (int m = threadIdx.x >> 6; m < a.n_mels; m += 4) {
    const int first = a.rows[3 * m], cnt = a.rows[3 * m + 1];
    const float* w = a.w + a.rows[3 * m + 2];
    float acc = 0.f;
    for (int i = 0; i < cnt; ++i) acc = fmaf(w[i], sp[(long long)(first + i) * a.spec_pitch], acc);
    a.mel[(long long)m * a.mel_pitch + col0 + t] = (float)log((double)fmaxf(acc, 1e-5f));
  }
}

void spec_to_mel_batch(Ctx* ctx, hipStream_t s, const float* spec, long long spec_pitch, const long long* clips, int n_clips, int n_fft, int n_mels,
                       float* mel, long long mel_pitch) {
  RVC_REQUIRE(n_clips >= 0 && spec_pitch >= 0 && mel_pitch >= 0, "bad argument");
  SpecState* st = spec_state(ctx);
  const int* bank_rows; const float* bank_w;
  {
    std::lock_guard<std::mutex> lk(st->mu);
    auto it = st->banks.find(std::make_pair(n_fft, n_mels));
    RVC_REQUIRE(it != st->banks.end(), "no filterbank was set for this (n_fft, n_mels)");
    bank_rows = it->second.rows.p; bank_w = it->second.w.p;
  }
  std::vector<long long> rows((size_t)n_clips * 4);
  long long blocks = 0;
  for (int c = 0; c < n_clips; ++c) {
    const long long col = clips[2 * c], nf = clips[2 * c + 1];
    RVC_REQUIRE(col >= 0 && nf >= 0 && col + nf <= spec_pitch && col + nf <= mel_pitch, "a clip's frames lie outside a row");
    rows[4 * c] = col; rows[4 * c + 1] = nf; rows[4 * c + 2] = 0; rows[4 * c + 3] = blocks;
    blocks += (nf + kMelCols - 1) / kMelCols;
  }
  RVC_REQUIRE(blocks < (1LL << 31), "too many frames for one call");
  if (blocks == 0) return;
  MelArgs a;
  a.spec = spec; a.spec_pitch = spec_pitch; a.n_clips = n_clips; a.rows = bank_rows; a.w = bank_w; a.n_mels = n_mels; a.mel = mel; a.mel_pitch = mel_pitch;
  upload_clips(s, 21, rows, n_clips, &a.clips);
  hipLaunchKernelGGL(mel_project_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------ log-mel vector-Jacobian product
// d_audio = J^T cot for J = d(log-mel) / d(audio) of stft_mag_kernel followed by mel_project_kernel.  Two launches.
//
// mel_vjp_frames_kernel<LOGM, TL, FR>: the forward's workgroup (FR frames, a team of TL lanes per frame, same load and same FFT, so the spectrum it differentiates
// is bit for bit the forward's) with four more passes over the rows it holds in LDS:
//   1. [bin][frame]   mag[b] = sqrt(|X[b]|^2 + eps) into LDS, as the forward stores it to HBM;
//   2. [mel][frame]   S[m] by mel_project_kernel's fma chain, cS[m] = cot[m] / S[m] where S[m] >= 1e-5 (the clamp's backward passes at equality), else 0;
//   3. [pair][frame]  the bins k and M - k share Z[k] and Z[M - k] and nothing else: c[b] = sum_m W[m][b] cS[m] over the rows the bank's transpose index lists
//                     (ascending m), G[b] = c[b] X[b] / mag[b] (0 where mag[b] is 0: a silent frame with eps 0), and the packed input of the inverse
//                     transform, P[k] = (Y[k] + conj Y[M - k]) + i e^{+2 pi i k / n_fft} (Y[k] - conj Y[M - k]) with Y = G / 2 inside and Re G at bins 0 and M
//                     (each one-sided bin enters the loss once, so the interior bins are halved against irfft), written back CONJUGATED over Z[k], Z[M - k];
//   4. the forward FFT again: conj(FFT(conj P)) is the inverse Stockham transform with the conjugated twiddles, read from the one uploaded table.  Its
//      output is the frame's real gradient, packed (even samples real, odd samples minus the imaginary part); times the window it goes to the stream's
//      scratch, frames [workgroup * FR + frame][n_fft].  Neither the spectrum nor its phase reaches HBM.
// mel_vjp_gather_kernel: one thread per sample adds, frames in index order, the entries of the <= ceil(n_fft / hop) frames that cover the sample and - hop <=
// n_fft - its mirror images in the reflect padding (position -k lands on sample k, N - 1 + k on N - 1 - k); a sample the frames do not reach (hop > n_fft,
// or the tail behind the last frame) and a sample the clamp cut off (|x| > 1.05) get 0.  No atomics: two calls give the same bits.
//
// Shapes (n_fft: TL x FR = threads; LDS = rows + twiddles + mag + cS at n_mels 256, the largest the multi-scale loss uses; cS is 4 FR n_mels bytes):
//   256:   16 x 16 = 256 threads;  16,640 +  1,544 +  8,256 + 16,384 =  42,824 B
//   512:   16 x 16 = 256 threads;  33,024 +  3,080 + 16,448 + 16,384 =  68,936 B
//   1024:  64 x 8  = 512 threads;  32,896 +  6,152 + 16,416 +  8,192 =  63,656 B (two workgroups per CU)
//   2048:  64 x 8  = 512 threads;  65,664 + 12,296 + 32,800 +  8,192 = 118,952 B
//   4096:  128 x 4 = 512 threads;  65,600 + 24,584 + 32,784 +  4,096 = 127,064 B.  Eight rows as in the forward leave 8,056 B, and mag alone is 8,196 B per frame; six
//          is no power of two (the [bin][frame] passes mask the frame), so four rows, and the workgroup is 8 waves on its CU.
constexpr int kVjpBlock = 256;        // samples per workgroup of the gather

struct VjpArgs {
  SpecArgs s;                           // s.out is unused; s.pitch is the cotangent's row pitch
  const float* cot; const int* rows; const float* w; const int* cols; int n_mels;
  float* frames;                        // [workgroups * FR][n_fft]
};

// Y[b] of pass 3 for bin b of frame-local cS: the bank's transpose, the magnitude's backward, the one-sided weight
__device__ __forceinline__ float2 bin_cotangent(const VjpArgs& a, const float* cS, float2 X, float mag, int b, int M) {
  float c = 0.f;
  for (int m = a.cols[2 * b]; m < a.cols[2 * b + 1]; ++m) {
    const int i = b - a.rows[3 * m];
    if (i >= 0 && i < a.rows[3 * m + 1]) c = fmaf(a.w[a.rows[3 * m + 2] + i], cS[m], c);
  }
  if (mag == 0.f) return make_float2(0.f, 0.f);
  const float g = c / mag;
  if (b == 0 || b == M) return make_float2(g * X.x, 0.f);
  return make_float2(0.5f * (g * X.x), 0.5f * (g * X.y));
}

// conj of P[k] = (A + conj B) + i w (A - conj B) with A = Y[k], B = Y[M - k], w = conj t = e^{+2 pi i k / n_fft}
__device__ __forceinline__ float2 packed_inverse_input(float2 A, float2 B, float2 t) {
  const float2 E = make_float2(A.x + B.x, A.y - B.y), D = make_float2(A.x - B.x, A.y + B.y);
  const float2 O = cmul(D, make_float2(t.x, -t.y));
  return make_float2(E.x - O.y, -(E.y + O.x));
}

template <int LOGM, int TL, int FR>
__global__ __launch_bounds__(FR * TL) void mel_vjp_frames_kernel(VjpArgs a) {
  constexpr int M = 1 << LOGM, Q = M / 4, S = M + kSpecRowPad, NT = 3 * M / 2 + 1, MS = M + 1;
  static_assert(Q % TL == 0 && (FR & (FR - 1)) == 0 && FR * TL <= 1024, "a team divides the butterflies of a stage; the [bin][frame] passes mask the frame");
  extern __shared__ float2 spec_lds[];
  float2* Z = spec_lds;                 // [FR][S]
  float2* tw = spec_lds + FR * S;       // [NT]
  float* mag = reinterpret_cast<float*>(tw + NT);      // [FR][MS]: an odd row stride, the FR frames of a bin on FR banks
  float* cS = mag + FR * MS;            // [FR][n_mels]
  const int tid = threadIdx.x, lane = tid % TL, wave = tid / TL;

  const int c = clip_of_block(a.s.clips, a.s.n_clips, blockIdx.x);
  const long long* d = a.s.clips + 4 * (long long)c;
  const long long soff = d[0], ns = d[1], ooff = d[2];
  const long long nf = ns / a.s.hop;
  const long long f0 = ((long long)blockIdx.x - d[3]) * FR;
  if (f0 >= nf) return;

  for (int t = tid; t < NT; t += FR * TL) tw[t] = a.s.tw[t];
  float2* z = Z + wave * S;
  const bool live = f0 + wave < nf;
  load_frame<LOGM, TL>(a.s, z, a.s.audio + soff, ns, f0 + wave, live, lane);
  __syncthreads();
  fft_row<LOGM, TL>(z, tw, lane);

  const int f = tid & (FR - 1);
  float2* zf = Z + f * S;
  float* magf = mag + f * MS;
  float* cSf = cS + f * a.n_mels;
  for (int b = tid / FR; b <= M; b += TL) magf[b] = bin_mag(split_bin(zf[b & (M - 1)], zf[(M - b) & (M - 1)], tw[b]), a.s.eps);
  __syncthreads();

  const bool flive = f0 + f < nf;       // a row behind the clip's last frame holds zeros and has no cotangent column
  for (int m = tid / FR; m < a.n_mels; m += TL) {
    float v = 0.f;
    if (flive) {
      const int first = a.rows[3 * m], cnt = a.rows[3 * m + 1];
      const float* w = a.w + a.rows[3 * m + 2];
      float acc = 0.f;
      for (int i = 0; i < cnt; ++i) acc = fmaf(w[i], magf[first + i], acc);
      if (acc >= 1e-5f) v = a.cot[(long long)m * a.s.pitch + ooff + f0 + f] / acc;
    }
    cSf[m] = v;
  }
  __syncthreads();

  for (int k = tid / FR; k <= M / 2; k += TL) {
    const int k2 = M - k;
    const float2 zk = zf[k], zc = zf[k2 & (M - 1)], t1 = tw[k], t2 = tw[k2];
    const float2 Y1 = bin_cotangent(a, cSf, split_bin(zk, zc, t1), magf[k], k, M);
    const float2 Y2 = bin_cotangent(a, cSf, split_bin(zc, zk, t2), magf[k2], k2, M);
    zf[k] = packed_inverse_input(Y1, Y2, t1);
    if (k != 0 && k2 != k) zf[k2] = packed_inverse_input(Y2, Y1, t2);
  }
  __syncthreads();
  fft_row<LOGM, TL>(z, tw, lane);

  if (live) {
    float2* g = reinterpret_cast<float2*>(a.frames + ((long long)blockIdx.x * FR + wave) * (2 * M));
    for (int m = lane; m < M; m += TL) g[m] = make_float2(a.s.win[2 * m] * z[m].x, -(a.s.win[2 * m + 1] * z[m].y));
  }
}

struct GatherArgs {
  const float* audio; const long long* clips; int n_clips;      // clips [n_clips][4] = (sample offset, samples, first row of frames, first workgroup)
  int n_fft, hop, pad, clamp;
  const float* frames; float* out;
};

__global__ __launch_bounds__(kVjpBlock) void mel_vjp_gather_kernel(GatherArgs a) {
  const int c = clip_of_block(a.clips, a.n_clips, blockIdx.x);
  const long long* d = a.clips + 4 * (long long)c;
  const long long soff = d[0], ns = d[1], row0 = d[2];
  const long long i = ((long long)blockIdx.x - d[3]) * kVjpBlock + threadIdx.x;
  if (i >= ns) return;
  const long long nf = ns / a.hop;
  float acc = 0.f;
  if (!(a.clamp && fabsf(a.audio[soff + i]) > 1.05f)) {
    long long q[3], lo[3], hi[3];       // padded positions that read sample i, and the frames that cover each
    int np = 0;
    q[np++] = i + a.pad;
    if (i >= 1 && i <= a.pad) q[np++] = a.pad - i;
    if (ns - 1 - i >= 1 && ns - 1 - i <= a.pad) q[np++] = 2 * (ns - 1) - i + a.pad;
    long long F0 = nf, F1 = -1;
    for (int j = 0; j < np; ++j) {
      lo[j] = q[j] < a.n_fft ? 0 : (q[j] - a.n_fft + a.hop) / a.hop;
      hi[j] = q[j] < 0 ? -1 : min(q[j] / a.hop, nf - 1);
      F0 = min(F0, lo[j]); F1 = max(F1, hi[j]);
    }
    for (long long fr = F0; fr <= F1; ++fr)
      for (int j = 0; j < np; ++j)
        if (fr >= lo[j] && fr <= hi[j]) acc = __fadd_rn(acc, a.frames[(row0 + fr) * a.n_fft + (q[j] - fr * a.hop)]);
  }
  a.out[soff + i] = acc;
}

template <int LOGM, int TL, int FR>
static void vjp_launch(hipStream_t s, long long blocks, const VjpArgs& a) {
  constexpr int M = 1 << LOGM;
  const size_t lds = ((size_t)FR * (M + kSpecRowPad) + 3 * M / 2 + 1) * sizeof(float2) + (size_t)FR * (M + 1 + a.n_mels) * sizeof(float);
  RVC_REQUIRE(lds <= 160 * 1024, "mel_spectrogram_vjp: too many mel rows for the workgroup's LDS");
  auto kern = mel_vjp_frames_kernel<LOGM, TL, FR>;
  RVC_ALLOW_BIG_LDS(kern);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(FR * TL), lds, s, a);
}

static int vjp_frames_per_block(int n_fft) { return n_fft <= 512 ? 16 : n_fft <= 2048 ? 8 : 4; }

void mel_spectrogram_vjp(Ctx* ctx, hipStream_t s, const float* audio, long long n_audio, const long long* clips, int n_clips, int n_fft, int hop, float eps,
                         int clamp, int n_mels, const float* cot, long long pitch, float* d_audio) {
  RVC_REQUIRE(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096, "n_fft must be 256, 512, 1024, 2048 or 4096");
  RVC_REQUIRE(hop > 0 && hop <= (1 << 24) && ((n_fft - hop) & 1) == 0, "hop must be positive with n_fft - hop even");
  RVC_REQUIRE(eps >= 0.f && n_clips >= 0 && pitch >= 0 && n_audio >= 0, "bad argument");
  SpecState* st = spec_state(ctx);
  VjpArgs a;
  {
    std::lock_guard<std::mutex> lk(st->mu);
    auto it = st->banks.find(std::make_pair(n_fft, n_mels));
    RVC_REQUIRE(it != st->banks.end(), "no filterbank was set for this (n_fft, n_mels)");
    a.rows = it->second.rows.p; a.w = it->second.w.p; a.cols = it->second.cols.p; a.n_mels = n_mels;
  }
  const int pad = (n_fft - hop) / 2, frames = vjp_frames_per_block(n_fft);
  std::vector<long long> rows((size_t)n_clips * 4), grows((size_t)n_clips * 4);
  long long blocks = 0, gblocks = 0;
  for (int c = 0; c < n_clips; ++c) {
    const long long off = clips[3 * c], n = clips[3 * c + 1], col = clips[3 * c + 2];
    if (pad >= 0) RVC_REQUIRE(n > pad, "a clip must be longer than (n_fft - hop) / 2 samples (reflect padding)");
    else RVC_REQUIRE(n >= hop, "a clip must hold one frame (hop samples when hop > n_fft)");
    RVC_REQUIRE(off >= 0 && off + n <= n_audio, "a clip lies outside the audio buffer");
    RVC_REQUIRE(col >= 0 && col + n / hop <= pitch, "a clip's frames lie outside the cotangent's row");
    rows[4 * c] = off; rows[4 * c + 1] = n; rows[4 * c + 2] = col; rows[4 * c + 3] = blocks;
    grows[4 * c] = off; grows[4 * c + 1] = n; grows[4 * c + 2] = blocks * frames; grows[4 * c + 3] = gblocks;
    blocks += (n / hop + frames - 1) / frames;
    gblocks += (n + kVjpBlock - 1) / kVjpBlock;
  }
  RVC_REQUIRE(blocks < (1LL << 31) && gblocks < (1LL << 31), "too many frames or samples for one call");
  if (gblocks == 0) return;
  const SpecTables& T = spec_tables(ctx, n_fft);
  a.s.audio = audio; a.s.n_clips = n_clips; a.s.hop = hop; a.s.pad = pad; a.s.eps = eps; a.s.clamp = clamp; a.s.tw = T.tw.p; a.s.win = T.win.p;
  a.s.out = nullptr; a.s.pitch = pitch;
  a.cot = cot;
  a.frames = (float*)stream_scratch(s, 25, (size_t)std::max<long long>(blocks, 1) * frames * n_fft * sizeof(float));
  long long* tab = (long long*)stream_scratch(s, 26, (size_t)n_clips * 8 * sizeof(long long));      // both clip tables behind one copy
  static thread_local std::vector<long long> keep;      // stays alive behind the asynchronous copy
  keep = rows; keep.insert(keep.end(), grows.begin(), grows.end());
  RVC_HIP_CHECK(hipMemcpyAsync(tab, keep.data(), keep.size() * sizeof(long long), hipMemcpyHostToDevice, s));
  a.s.clips = tab;
  if (blocks > 0) switch (n_fft) {
    case 256: vjp_launch<7, 16, 16>(s, blocks, a); break;
    case 512: vjp_launch<8, 16, 16>(s, blocks, a); break;
    case 1024: vjp_launch<9, 64, 8>(s, blocks, a); break;
    case 2048: vjp_launch<10, 64, 8>(s, blocks, a); break;
    default: vjp_launch<11, 128, 4>(s, blocks, a); break;
  }
  GatherArgs g;
  g.audio = audio; g.clips = tab + (size_t)n_clips * 4; g.n_clips = n_clips; g.n_fft = n_fft; g.hop = hop; g.pad = pad; g.clamp = clamp; g.frames = a.frames; g.out = d_audio;
  hipLaunchKernelGGL(mel_vjp_gather_kernel, dim3((unsigned)gblocks), dim3(kVjpBlock), 0, s, g);
}

// ------------------------------------------------------------------------------------------------ multi-scale mel loss
// One scale of MultiScaleMelSpectrogramLoss.forward: spec holds 2 B rows of nf frames (row r at column r * row_stride; rows 0 .. B - 1 the first signal,
// B .. 2 B - 1 the second).  A workgroup owns kMelCols frames of one item, wave g the mels g, g + 4, ...: both log-mels of an element are formed as
// mel_project_kernel forms them (same fma chain, same float64 logarithm), the pointwise loss of the pair in fp32 as the reference's loss_fn sees
// it, and the sums over the workgroup's elements in float64 (thread: ascending mel; block_sum).  The log-mels never reach HBM.  part[blk] takes the
// log term, part[blocks + blk] the term on exp(log-mel) (zero unless want_mag); f64_segment_sums adds the partials in index order.
struct MelLossArgs {
  const float* spec; long long pitch, row_stride, nf; int B, tiles;
  const int* rows; const float* w; int n_mels;
  int loss, want_mag;                   // loss 0 l1, 1 l2, 2 smoothl1 (beta 1)
  double* part; long long blocks;
};

__device__ __forceinline__ float pointwise_loss(int kind, float a, float b) {
  const float d = __fsub_rn(a, b), m = fabsf(d);
  if (kind == 0) return m;
  if (kind == 1) return __fmul_rn(d, d);
  return m < 1.0f ? __fmul_rn(__fmul_rn(0.5f, d), d) : __fsub_rn(m, 0.5f);
}

__global__ __launch_bounds__(256) void mel_scale_loss_kernel(MelLossArgs a) {
  __shared__ double red[4];
  const int item = blockIdx.x / a.tiles, tile = blockIdx.x - item * a.tiles;
  const long long t = (long long)tile * kMelCols + (threadIdx.x & 63);
  double acc_log = 0.0, acc_mag = 0.0;
  if (t < a.nf) {
    const float* sx = a.spec + (long long)item * a.row_stride + t;
    const float* sy = sx + (long long)a.B * a.row_stride;
    for (int m = threadIdx.x >> 6; m < a.n_mels; m += 4) {
      const int first = a.rows[3 * m], cnt = a.rows[3 * m + 1];
      const float* w = a.w + a.rows[3 * m + 2];
      float ax = 0.f, ay = 0.f;
      for (int i = 0; i < cnt; ++i) {
        const long long o = (long long)(first + i) * a.pitch;
        ax = fmaf(w[i], sx[o], ax); ay = fmaf(w[i], sy[o], ay);
      }
      const float lx = (float)log((double)fmaxf(ax, 1e-5f)), ly = (float)log((double)fmaxf(ay, 1e-5f));
      acc_log += (double)pointwise_loss(a.loss, lx, ly);
      if (a.want_mag) acc_mag += (double)pointwise_loss(a.loss, (float)exp((double)lx), (float)exp((double)ly));
    }
  }
  const double tl = block_sum(acc_log, red);
  const double tm = block_sum(acc_mag, red);
  if (threadIdx.x == 0) { a.part[blockIdx.x] = tl; a.part[a.blocks + blockIdx.x] = tm; }
}

// launches: K (one per scale) + 1 (the 2 K sums).  out [K][2] = (sum of the log term, sum of the mag term); the caller divides by B n_mels nf.
void multiscale_mel_loss(Ctx* ctx, hipStream_t s, int K, const float* const* spec, const long long* pitch, const long long* row_stride, int B, long long nf,
                         const int* n_fft, const int* n_mels, int loss, int want_mag, double* out) {
  RVC_REQUIRE(K >= 1 && K <= kSegSumMax / 2 && B >= 1 && nf >= 1 && loss >= 0 && loss <= 2, "multiscale_mel_loss: 1 <= K <= 8 scales, B, frames >= 1, loss 0 .. 2");
  const long long tiles = (nf + kMelCols - 1) / kMelCols, blocks = (long long)B * tiles;
  RVC_REQUIRE(blocks < (1LL << 24), "too many frames for one call");
  SpecState* st = spec_state(ctx);
  MelLossArgs a[kSegSumMax / 2];
  {
    std::lock_guard<std::mutex> lk(st->mu);
    for (int k = 0; k < K; ++k) {
      auto it = st->banks.find(std::make_pair(n_fft[k], n_mels[k]));
      RVC_REQUIRE(it != st->banks.end(), "no filterbank was set for this (n_fft, n_mels)");
      RVC_REQUIRE(spec[k] && row_stride[k] >= nf && 2LL * B * row_stride[k] - (row_stride[k] - nf) <= pitch[k], "the 2 B rows lie outside the spectrogram's row");
      a[k].rows = it->second.rows.p; a[k].w = it->second.w.p;
    }
  }
  double* part = (double*)stream_scratch(s, 22, (size_t)K * 2 * blocks * sizeof(double));
  long long bounds[kSegSumMax + 1];
  for (int k = 0; k < K; ++k) {
    a[k].spec = spec[k]; a[k].pitch = pitch[k]; a[k].row_stride = row_stride[k]; a[k].nf = nf; a[k].B = B; a[k].tiles = (int)tiles;
    a[k].n_mels = n_mels[k]; a[k].loss = loss; a[k].want_mag = want_mag; a[k].part = part + (long long)k * 2 * blocks; a[k].blocks = blocks;
    bounds[2 * k] = (long long)k * 2 * blocks; bounds[2 * k + 1] = bounds[2 * k] + blocks;
    hipLaunchKernelGGL(mel_scale_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a[k]);
  }
  bounds[2 * K] = (long long)K * 2 * blocks;
  f64_segment_sums(s, part, bounds, 2 * K, out);
}

// The cotangent on the generated log-mel a of log_weight mean loss(a, b) + mag_weight mean loss(exp a, exp b), times scale[k], for K <= 8 scales in one
// launch (blockIdx.y = scale): loss'(d) = sign d (0 at 0) | 2 d | d inside (-1, 1), sign d outside.  Every element is formed in float64 from the float32
// log-mels and rounded once; a term whose weight is not positive is left out, as the forward leaves it out.
struct MelCotArgs { const float* a[kSegSumMax / 2]; const float* b[kSegSumMax / 2]; float* out[kSegSumMax / 2]; long long n[kSegSumMax / 2]; double scale[kSegSumMax / 2];
                    int loss; double log_weight, mag_weight; };
__device__ __forceinline__ double pointwise_loss_slope(int kind, double d) {
  const double sg = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
  if (kind == 0) return sg;
  if (kind == 1) return 2.0 * d;
  return fabs(d) < 1.0 ? d : sg;
}
__global__ __launch_bounds__(256) void mel_loss_cotangents_kernel(MelCotArgs p) {
  const int k = blockIdx.y;
  const float* a = p.a[k]; const float* b = p.b[k]; float* out = p.out[k];
  const long long n = p.n[k], st = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) {
    const double x = (double)a[i], y = (double)b[i];
    double g = 0.0;
    if (p.log_weight > 0.0) g = p.log_weight * pointwise_loss_slope(p.loss, x - y);
    if (p.mag_weight > 0.0) { const double ex = exp(x); g += p.mag_weight * pointwise_loss_slope(p.loss, ex - exp(y)) * ex; }
    out[i] = (float)(p.scale[k] * g);
  }
}
void mel_loss_cotangents(hipStream_t s, int K, const float* const* a, const float* const* b, const long long* n, int loss, float log_weight, float mag_weight,
                         const float* scale, float* const* out) {
  RVC_REQUIRE(a && b && n && scale && out && K >= 1 && K <= kSegSumMax / 2 && loss >= 0 && loss <= 2, "mel_loss_cotangents: 1 <= K <= 8 scales, loss 0 .. 2");
  MelCotArgs p;
  long long most = 0;
  for (int k = 0; k < K; ++k) {
    RVC_REQUIRE(a[k] && b[k] && out[k] && n[k] > 0, "mel_loss_cotangents: empty tensor");
    p.a[k] = a[k]; p.b[k] = b[k]; p.out[k] = out[k]; p.n[k] = n[k]; p.scale[k] = (double)scale[k];
    most = std::max(most, n[k]);
  }
  p.loss = loss; p.log_weight = (double)log_weight; p.mag_weight = (double)mag_weight;
  hipLaunchKernelGGL(mel_loss_cotangents_kernel, dim3((unsigned)std::min<long long>((most + 255) / 256, 1024), K), dim3(256), 0, s, p);
}

}  // namespace rvc
