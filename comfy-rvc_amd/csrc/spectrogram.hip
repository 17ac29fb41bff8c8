// Training inputs (reference lib/train/mel_processing.py): the linear magnitude spectrogram of a ragged batch of clips by an LDS FFT, the log-mel
// projection of such a batch through a banded filterbank, and the per-scale term of the multi-scale mel loss (lib/train/losses.py:430-561).  gfx950,
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
struct MelBank { int n_fft = 0, n_mels = 0; DevBuf<int> rows; DevBuf<float> w; };   // rows [n_mels][3] = (first bin, count, offset into w)
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

  // ---- load: frame f0 + wave, samples through the reflect index, clamp, window, packed pairs
  float2* z = Z + wave * S;
  const long long fr = f0 + wave;
  const bool live = fr < nf;
  const float* x = a.audio + soff;
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
  __syncthreads();

  // ---- M-point forward FFT of the wave's row: Stockham autosort, inputs j + r M / R, outputs (j / Ns) Ns R + j % Ns + r Ns
  constexpr int PER4 = Q / TL;
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

  // ---- real-input split and magnitude, [bin][frame]: X[b] = (Z[b] + conj Z[M - b]) / 2 - (i / 2) e^{-2 pi i b / n_fft} (Z[b] - conj Z[M - b])
  const int f = tid & (FR - 1);
  const float2* zf = Z + f * S;
  const bool store = f0 + f < nf;
  float* out = a.out + ooff + f0 + f;
  for (int b = tid / FR; b <= M; b += TL) {
    const float2 zk = zf[b & (M - 1)], zc = zf[(M - b) & (M - 1)], t = tw[b];
    const float er = 0.5f * (zk.x + zc.x), ei = 0.5f * (zk.y - zc.y);
    const float dr = zk.x - zc.x, di = zk.y + zc.y;
    const float p = t.x * dr - t.y * di, q = t.x * di + t.y * dr;
    const float re = er + 0.5f * q, im = ei - 0.5f * p;
    const float mag = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), a.eps));      // the reference's roundings: spec.pow(2).sum(-1) + eps
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
  SpecState* st = spec_state(ctx);
  std::lock_guard<std::mutex> lk(st->mu);
  MelBank& B = st->banks[std::make_pair(n_fft, n_mels)];
  if (B.rows.p) RVC_HIP_CHECK(hipDeviceSynchronize());      // a replaced bank may still be read by an earlier call
  B.rows.reset(); B.w.reset();
  B.n_fft = n_fft; B.n_mels = n_mels;
  B.rows.upload(rows);
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

}  // namespace rvc
