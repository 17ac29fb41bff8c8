// Internal declarations shared by the HIP translation units of librvc_hip.so (gfx950 only).
// Public C ABI: include/rvc_hip.h.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <stdexcept>

namespace rvc {

// ----------------------------------------------------------------------------- errors
void set_error(const std::string& msg);
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

#define RVC_HIP_CHECK(expr)                                                                       \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      throw rvc::Error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + \
                       ":" + std::to_string(__LINE__) + ")");                                     \
  } while (0)

#define RVC_REQUIRE(cond, msg)                                                                    \
  do {                                                                                            \
    if (!(cond)) throw rvc::Error(std::string("requirement failed: ") + #cond + " : " + (msg));   \
  } while (0)

// ----------------------------------------------------------------------------- run-time knobs
// knob_int: a DOCUMENTED tuning / diagnosis knob of the product library (INTEGRATION.md lists every one with its test).
// exp_int: an experiment knob (tile choices, kernel selection, thresholds that a measurement once swept): compiled to its default in the product
// build - the name does not even reach the binary - and read from the environment only in -DRVC_EXPERIMENTS builds (tools/build_variant.sh).
inline int knob_int(const char* name, int def) { const char* e = getenv(name); return e ? atoi(e) : def; }
#ifdef RVC_EXPERIMENTS
inline int exp_int(const char* name, int def) { return knob_int(name, def); }
#define RVC_EXP_STR(name) getenv(name)
#else
#define exp_int(name, def) (def)
#define RVC_EXP_STR(name) ((const char*)nullptr)
#endif

// ----------------------------------------------------------------------------- activations
enum Act : int { ACT_NONE = 0, ACT_LRELU = 1, ACT_RELU = 2, ACT_GELU = 3, ACT_TANH = 4, ACT_SIGMOID = 5, ACT_LOGCLAMP = 6 };

// ----------------------------------------------------------------------------- conv (conv_mfma.hip)
// One implicit-GEMM convolution: Y[m, n] = epilogue( sum_k Wp[k, m] * Xtile[k, n] ).
// 1-D: X [Ci][Tin] (time contiguous), 2-D: X [Ci][H][Wd].  Weights are pre-packed on the host.
struct ConvArgs {
  const float* X; const float* W; const float* bias; const float* R; float* Y;
  int Ci;        // input channels (per group)
  int Co;        // GEMM rows that are stored (per group)
  int CoP;       // padded rows in the packed weights (multiple of 32)
  int Tin;       // 1-D: input length.  2-D: H
  int Tout;      // 1-D: output length. 2-D: H*Wd (output positions of the GEMM)
  int Wd;        // 2-D: width (power of two); 0 for 1-D
  int ktaps;     // taps per virtual channel (1-D: ceil(k/stride); 2-D: 9)
  int dil, stride, pad;
  int CK;        // virtual channels per chunk (even)
  int KT;        // taps per weight stage
  int nchunk;    // number of chunks
  int WROW;      // LDS row pitch in floats
  int PW, BWd, BH;  // 2-D: LDS row pitch of one image row, tile width, tile rows
  long long xBatch, wBatch, yBatch, rBatch; int bBatch;   // blockIdx.z strides (elements)
  long long ldX, ldY, ldR;                               // channel strides (elements)
  int pre_act; float pre_slope;                          // activation applied to X while staging
  int act; float act_slope;                              // epilogue activation
  int act_before_res;                                    // 1: act(v)+R   0: act(v+R)
  float out_scale; int accumulate;                       // y = [y +] out_scale * v
  int ostride, orows;                                    // 1-D interleaved store: m -> (co = m % orows, r = m / orows); addr = co*ldY + n*ostride + r
  int up2;                                               // 2-D: ConvTranspose 2x2 phase interleave
  int KH, KW, PH, PWL;                                   // 2-D window (0 = 3 x 3, pad 1): taps KH x KW, zero padding PH rows above / PWL columns left
};

// A convolution layer with its weights packed for the kernel and resident on the device.
struct ConvLayer {
  float* Wd_ = nullptr;    // packed weights (device)
  float* bd_ = nullptr;    // bias (device) or null
  float* bd4_ = nullptr;   // ConvTranspose2d on the bf16x3 path: bias repeated per output phase
  int mode = 1;            // 1: 1-D, 2: 2-D 3x3
  int Ci = 0, Co = 0, CoP = 0, groups = 1;
  int k = 1, stride = 1, dil = 1, pad = 0;
  int ktaps = 1, CK = 8, KT = 1, nchunk = 1;
  int tconv_u = 0;         // >0: ConvTranspose1d with stride u (polyphase rows), `Co` = u * co_real
  int co_real = 0;
  int up2 = 0;             // 2-D ConvTranspose (k3 s2 p1 op1) as 4 phase convs
  int conv_pad = 0;        // ConvTranspose1d: left pad of the equivalent stride-1 conv
  long long wBatch = 0;    // packed elements per group
  int kh = 3, kw = 3, ph = 1, pwl = 1;   // 2-D window (conv2d_kx_layer_init; the 3 x 3 layers keep the defaults)
  uint16_t* Wx_ = nullptr; // bf16x3 split image (conv_x3.hip), null when the layer only runs on the fp32 kernel
  int CoPx = 0; long long wxBatch = 0;
  uint16_t* Wh_ = nullptr; // fp16x2 (H2) image of a ResBlock-pair layer: ONE fp16 plane per (chunk, tap) unit, [chunk][tap][half][CoPx rows][8 ch] (conv_x3q.hip)
  int seg2_chunks = 0;     // conv_x3s only: 16-channel chunks of a SECOND input image appended to the reduction with tap offset 0 (conv_layer_append_x3:
                           // MDX23C's tfc2(x2) + shortcut(x) as one product); the caller names that image in SplitGeom::seg2_off
};

struct ConvEpilogue {
  const float* R = nullptr; long long ldR = 0;
  int pre_act = ACT_NONE; float pre_slope = 0.f;
  int act = ACT_NONE; float act_slope = 0.f;
  int act_before_res = 0;
  float out_scale = 1.f; int accumulate = 0;
  const float* bias_override = nullptr;   // per-call bias vector replacing the layer's own (speaker conditioning)
  int tout_limit = 0;                     // >0: compute only the first tout_limit output positions
  int plan_tin = 0;                       // >0: this launch is a column window of a sequence of plan_tin INPUT columns ("Planning length" below); 0: it is the whole sequence
  // split-resident activations (bf16x3 kernel only, conv_x3.hip): the tensor lives as the bf16 hi / lo image the kernel stages in LDS,
  // [16-channel chunk][hi | lo][8-channel half][kSplitMargin + t][8 ch], written by the producer's epilogue (activation `ys_slope` already applied)
  // and copied straight into LDS by the consumer (no conversion, no registers).  xs_in replaces X, ys_out replaces Y.
  const unsigned char* xs_in = nullptr; long long xs_tp = 0;
  unsigned char* ys_out = nullptr; long long ys_tp = 0; float ys_slope = 1.f;
  // conv_x3s_run only: rows [vt_row0, Co) of an image-only k = 1 projection are written TRANSPOSED as the V^T image of the attention (attention_vt_tp rows per plane) instead of
  // into ys_out - q | k | v in ONE launch (the rows below vt_row0 go to ys_out as usual); vt_row0 a multiple of 128
  unsigned char* vt_out = nullptr; long long vt_tp = 0; int vt_row0 = 0;
  // conv_x3s_run only: the WaveNet gate in the epilogue - the layer's 2 H rows packed in wn_gate_row_order (physical row p of 32-row block b = p / 32: tanh row of channel
  // 16 b + p % 32 for p % 32 < 16, sigmoid row of channel 16 b + p % 32 - 16 otherwise); ys_out receives tanh(a + g[c]) sigmoid(a' + g[H + c]) of the H channels
  int gate_h = 0; const float* gate_g = nullptr;
  int ys_deint_h = 0;                     // conv_x3s_run only: the output image is written de-interleaved for a stride-2 consumer (split_s2_h of the output length)
  // fp16x2 arithmetic (conv_x3q.hip, H2) for BOTH halves of a ResBlock pair: the intermediate image is fp16 hi / lo and each layer multiplies with its
  // one-plane fp16 weight image; only valid when conv1d_pair_h2_eligible(c1, c2, T) said so (no other kernel reads that image format)
  int h2 = 0;
};
constexpr int kSplitMargin = 64;                                                   // positions in front of t = 0 (covers every left halo)
inline long long split_image_tp(long long T) { return (T + kSplitMargin + 704 + 63) & ~63LL; }   // rows per plane: margin + T + the last tile's overhang
inline size_t split_image_bytes(int C, long long T) { return (size_t)(C / 16) * 2 * (size_t)split_image_tp(T) * 32; }
// true when this layer at this length runs on the bf16x3 kernel with a tile that has the split-resident path of its ROLE: a producer
// (writes the image: ConvEpilogue::ys_out) and a consumer (stages it: xs_in) take different branches of the tile choice, so each role
// is planned with its own geometry.  pre_lrelu: the producer's input activation (part of the real launch's arguments).
// These three questions are pure functions of their arguments.  Tin is the length the decision is made for: where the launch is a column window of a longer
// sequence, the caller passes the WHOLE sequence's length ("Planning length" below).
enum SplitRole : int { SPLIT_CONSUMER = 0, SPLIT_PRODUCER = 1 };
bool conv1d_split_eligible(const ConvLayer& L, int Tin, SplitRole role = SPLIT_CONSUMER, int h2 = 0);
// both layers of a ResBlock pair carry an fp16 image and both launches land on the persistent kernel at this length; false when the pair arithmetic is switched to bf16x3
// (h2 = 0: rvc_set_pair_arithmetic(0) / RVC_H2=0).  h2: the process-wide pair arithmetic as the caller queried it ONCE at the start of its call - a
// conversion uses the mode it saw when it started
bool conv1d_pair_h2_eligible(const ConvLayer& c1, const ConvLayer& c2, int Tin, int h2);
// Columns after which the order of the fp32 additions of this layer as the CONSUMER of a split-resident pair (c2: image in, residual added) repeats: 1 when
// every column is summed alike, the tile width where the persistent kernel adds the residual block by block.  A launch over a column window computes what the
// launch over the whole sequence computes only if the window starts at a multiple of it (synth_infer_window aligns its window).
int conv1d_residual_period(const ConvLayer& L, int Tin, int h2);
int conv_set_pair_arithmetic(int mode);   // process-wide: 1 = fp16x2 on eligible ResBlock pairs (default), 0 = bf16x3 everywhere; < 0 queries; returns the previous mode

// Planning length: the output columns of the WHOLE sequence that a launch is a column window of (the generator behind synth_infer's keep window).  Such a launch
// must compute, column for column, what the launch over the whole sequence computes, so DECISIONS READ THE PLANNING LENGTH (kernel, tile, arithmetic, K split,
// fall-back thresholds) and SIZES READ THE REAL ONE (grids, ldP, buffers, image rows).  It is an argument like the pair arithmetic h2: ConvEpilogue::plan_tin
// for the *_run functions (0 = the launch is the whole sequence), a parameter of the planners (conv_kernels.h), the length itself for the three questions
// above.  It lives in host-side types only: no kernel-argument struct holds it, so no kernel can see it.

// host-side packing + upload (weights in PyTorch layouts)
void conv1d_layer_init(ConvLayer& L, const float* w /*[Co][Ci/groups][k]*/, const float* bias, int Co, int Ci, int k,
                       int stride, int pad, int dil, int groups);
void tconv1d_layer_init(ConvLayer& L, const float* w /*[Ci][Co][k]*/, const float* bias, int Ci, int Co, int k, int u, int pad);
void conv2d3x3_layer_init(ConvLayer& L, const float* w /*[Co][Ci][3][3]*/, const float* bias, int Co, int Ci);
void conv2d1x1_layer_init(ConvLayer& L, const float* w /*[Co][Ci]*/, const float* bias, int Co, int Ci);
void tconv2d_layer_init(ConvLayer& L, const float* w /*[Ci][Co][3][3]*/, const float* bias, int Ci, int Co);
// general KH x KW window with asymmetric zero padding, bf16x3 image only (no fp32 twin): the layers run on conv_x3s_run
void conv2d_kx_layer_init(ConvLayer& L, const float* w /*[Co][Ci][KH][KW]*/, const float* bias, int Co, int Ci, int KH, int KW, int PH, int PWL);
// Layers initialised while this is on also get a bf16x3 split weight image and run on conv_x3_kernel when eligible
// (stride 1, groups 1, Ci % 16 == 0): 3 bf16 MFMAs per fp32 product, fp32 accumulate, ~1e-5 relative error.
// Both switches are THREAD-LOCAL (a model is built by the thread that calls *_finalize; two threads building models at the same time
// cannot see each other's scopes).  Models take their mode from their context (Ctx::precision) through ConvBuildScope.
bool conv_x3_set_default(bool on);   // returns the previous value
int conv_set_precision(int mode);    // 0: fp32 only, 1: layers initialised under conv_x3_set_default(true), 2: every eligible layer; returns the previous mode
struct ConvBuildScope {              // RAII: layers initialised inside get bf16x3 images according to `precision`
  int prev_mode; bool prev_default;
  explicit ConvBuildScope(int precision) : prev_mode(conv_set_precision(-1)), prev_default(conv_x3_set_default(true)) {   // < 0: keep the thread's mode
    if (precision >= 0) conv_set_precision(precision);
  }
  ~ConvBuildScope() { conv_x3_set_default(prev_default); conv_set_precision(prev_mode); }
  ConvBuildScope(const ConvBuildScope&) = delete; ConvBuildScope& operator=(const ConvBuildScope&) = delete;
};

// launches.  1-D: X [Ci][Tin] with channel stride ldX, Y [Co][Tout] with channel stride ldY.
int conv1d_out_len(const ConvLayer& L, int Tin);
void conv1d_run(const ConvLayer& L, hipStream_t s, const float* X, long long ldX, int Tin, float* Y, long long ldY,
                const ConvEpilogue& e);
// GEMM with an activation tensor as the "weight" operand: Y[z][m][n] = sum_k A[z][k][m] * B[z][k][n]  (k = channel)
void gemm_tn_run(hipStream_t s, const float* A, long long ldA, long long aBatch, const float* B, long long ldB, long long bBatch,
                 float* Y, long long ldY, long long yBatch, int M, int N, int K, int batch, const float* bias, int biasBatch,
                 const ConvEpilogue& e);
// 2-D: X [Ci][H][Wd], Y [Co][H][Wd] (or [Co][2H][2Wd] for up2).
void conv2d_run(const ConvLayer& L, hipStream_t s, const float* X, long long ldX, int H, int Wd, float* Y, long long ldY,
                const ConvEpilogue& e);

// bf16x3 GEMM of a k = 1 layer on a SPLIT-RESIDENT activation (conv_x3s.hip): both operand tiles by LDS-DMA, K split reduced inside the
// launch.  Xs: image of the [Ci][T] input (split_image_tp(T) rows per plane); Y (fp32 [Co][ldY]) and / or e.ys_out (image of the output, the
// activation e.act - identity, (leaky) ReLU, exact GELU - applied before the split).  e.R: residual, e.bias_override as in conv1d_run.
// Layers with taps run on the same kernel: a unit of the reduction is (16-channel chunk, tap) and a tap is a row offset into the image
// (im2col by address).  1-D "same" convolutions need nothing else (rows in front of position 0 / behind position T - 1 are the zero padding:
// producers keep the margins zero).  2-D convolutions run over PADDED images: row pitch W + 2 with a zero column on either side, position
// p = h (W + 2) + w + 1, T = H (W + 2); the kernel writes zeros into the pad columns of its outputs (SplitGeom from split_geom_2d).
struct SplitGeom { int ktaps = 1; int toff[16] = {0}; int padw = 0; int margin = kSplitMargin;
                   long long seg2_off = 0;      // byte offset (from the first image, < 2 GiB, same rows per plane and margin) of the second image of a layer with seg2_chunks
                   int s2_h = 0; };             // > 0: stride-2 "valid" convolution over a DE-INTERLEAVED image (split_geom_s2): even positions at rows margin + p, odd ones at margin + s2_h + p
// dst (a conv_x3s-eligible layer) += the k = 1 layer `extra` over a second input: the weight image of `extra` is appended as further units of dst's reduction
void conv_layer_append_x3(ConvLayer& dst, const ConvLayer& extra);
SplitGeom split_geom_2d(int Wd, int KH = 3, int KW = 3, int PH = 1, int PWL = 1);
// Stride-2 convolutions without padding (HuBERT's feature encoder, modeling_hubert.py conv_layers 1 .. 6: k = 3 / 2) on the split-resident GEMM: the producer writes the
// input image de-interleaved (ConvEpilogue::ys_deint_h / hubert_conv0_gn_gelu), so tap t of output p - input position 2 p + t - is row p + (t >> 1) of plane t & 1: a row
// offset like every other tap.  H = rows between the two planes (split_s2_h(T_in)); the image has split_s2_tp(T_in) rows per plane.
inline int split_s2_h(long long Tin) { return (int)(((Tin + 1) / 2 + 64 + 63) & ~63LL); }
inline long long split_s2_tp(long long Tin) { return (kSplitMargin + 2LL * split_s2_h(Tin) + 704 + 63) & ~63LL; }
inline size_t split_s2_bytes(int C, long long Tin) { return (size_t)(C / 16) * 2 * (size_t)split_s2_tp(Tin) * 32; }
SplitGeom split_geom_s2(int k, long long Tin);
bool conv_x3s_s2_eligible(const ConvLayer& L);
inline int wn_gate_row_order(int p, int H) { const int b = p >> 5, q = p & 31; return q < 16 ? 16 * b + q : H + 16 * b + (q - 16); }      // physical row -> row of the reference's [tanh H | sigmoid H] layer
void split_image_deint_from_f32(hipStream_t s, const float* X, long long ldX, int C, int T, unsigned char* img, long long tp, int H);      // (tests: in the models the producers' epilogues write the image)
void split_image_deint_to_f32(hipStream_t s, const unsigned char* img, long long tp, int H, int C, int T, float* Y, long long ldY);
bool conv_x3s_eligible(const ConvLayer& L);
void conv_x3s_run(const ConvLayer& L, hipStream_t s, const unsigned char* Xs, long long xsTp, int T, float* Y, long long ldY, const ConvEpilogue& e,
                  const SplitGeom* geom = nullptr);
// the swapped product: out[t][j] = sum_c X[c][t] W[row0 + j][c], written as the image of the transposed tensor (V^T for attention_split)
void conv_x3s_run_swapped(const ConvLayer& L, int row0, int rows, hipStream_t s, const unsigned char* Xs, long long xsTp, int T, unsigned char* Ys, long long ysTp,
                          float* Yrm = nullptr, long long ldYrm = 0,      // Yrm: also / instead fp32 out[t][j] with pitch ldYrm
                          const float* Rrm = nullptr, long long ldRrm = 0);  // Rrm: residual added to the product, laid out like Yrm (MDX23C's x + tdf(x))
void split_image_from_tm(hipStream_t s, const float* x, int C, int T, int M, unsigned char* img, long long tp);      // x [C][T][M] -> image of the (C M) x T tensor
void conv_x3s_force(int ksplit, int am, int an);      // tests / benchmarks: K split and tile of the calling thread's next launches (0 = automatic)
// the bf16x3 weight image of a dense layer on the host: P[chunk][tap][hi | lo][half][CoPx rows][8 ch] from w [Co][Ci][k], Ci % 16 == 0, rows Co .. CoPx - 1 zero (conv_mfma.hip)
void x3_weight_image(const float* w, int Co, int Ci, int k, int CoPx, std::vector<uint16_t>& P);
// Strided k-tap convolution along H over S tensors [Ci][H][p] -> [Co][Hout][p] (both [S][C][H][p], contiguous) in one bf16x3 GEMM launch, bias and
// leaky ReLU (slope 1: none) in the epilogue (conv_x3d.hip: the discriminators' dense layers).  Planned, then launched, like the split-MFMA family
// (conv_kernels.h); the plan is pure and its launch count - one - does not depend on S.  Wx: x3_weight_image of the layer.
struct ConvX3dArgs {
  const float* X; const unsigned char* Wx; const float* bias; float* Y;
  int Ci, Co, CoPx, H, Hout, p, k, stride, pad, S; float slope;
};
struct ConvX3dPlan { ConvX3dArgs a; dim3 grid; int units = 1; size_t lds = 0; double flops = 0.0; };   // units: (chunk, tap) units per pipeline stage (1, 2 or 4)
bool conv_x3d_plan(const ConvX3dArgs& a, ConvX3dPlan& p);   // false: the layer does not fit the kernel (Ci % 16, Co % 128 with CoPx = Co, a bias, k <= 16, 32-bit offsets)
void conv_x3d_launch(const ConvX3dPlan& p, hipStream_t s);
// The data gradient of that convolution with the backward chain's epilogue (conv_x3d_bwd.hip):  Y = (convT(D) + Cot) * (A > 0 ? 1 : slope), Y / Cot / A
// [S][R][H][p] (R = the forward's input channels), D [S][Ck][Hd][p] (Ck = the forward's output channels).  The output rows h = ostride j + ph form
// nph = ostride phases; phase ph is a stride-1 product of nt[ph] taps, tap t reading row j + off0 + t of D, with its own x3_weight_image Wx[ph]
// (rows R padded to RPx, channels Ck, nt[ph] taps).  Hj and tile0 are filled by the planner.  One launch for every phase and every signal.
struct ConvX3dBwdArgs {
  const float* D; const unsigned char* Wx[3]; const float* Cot; const float* A; float* Y;
  int R, RPx, Ck, Hd, H, p, ostride, off0, nph, S; int nt[3]; int Hj[3]; int tile0[4]; float slope;
};
struct ConvX3dBwdPlan { ConvX3dBwdArgs a; dim3 grid; int units = 1; size_t lds = 0; double flops = 0.0; };
bool conv_x3d_bwd_plan(const ConvX3dBwdArgs& a, ConvX3dBwdPlan& p);   // false: the layer does not fit the kernel
void conv_x3d_bwd_launch(const ConvX3dBwdPlan& p, hipStream_t s);
// the host side of that launch for a dense layer w [Co][Ci][5] (pad 2, stride 1 or 3), shared by the net and the raw entry (discriminator.hip): the transposed,
// phase-grouped images (returns the number of phases) and every field of the arguments but the pointers
int disc_bwd_weight_images(const float* w, int Co, int Ci, int k, int stride, int pad, std::vector<uint16_t> (&img)[3], int (&nt)[3]);
void disc_bwd_geometry(ConvX3dBwdArgs& a, int Ci, int Co, int k, int stride, int pad, int H, int Hd, int p, int S, float slope);
// The data gradient of the generator's 1-D convolutions with the backward chain's epilogue (conv_gen_bwd.hip):
//   Y[r][n] = (sum_c sum_t W'[r][c][t] D[c][cstride n + off0 + tstep t]) * (A[r][n] > 0 ? scale : scale slope) + Res[r][n] (+ Y[r][n]),   r < R, n < N
// D [Ck][ldD] with Td valid columns (zero outside), Wx = x3_weight_image of W' [R][Ck][nt] with its rows padded to RPx (a multiple of 128); A (null: no mask),
// Res (null) and Y share the pitch ldY.  One launch; planned, then launched, like the split-MFMA family.
struct ConvGenBwdArgs {
  const float* D; long long ldD; int Td; const unsigned char* Wx; const float* A; const float* Res; float* Y; long long ldY;
  int R, RPx, Ck, N, nt, cstride, tstep, off0; float slope, scale; int accumulate;
};
struct ConvGenBwdPlan { ConvGenBwdArgs a; dim3 grid; int bm = 128, units = 1; size_t lds = 0; double flops = 0.0; };   // bm: rows per workgroup (128, 64, 32)
bool conv_gen_bwd_plan(const ConvGenBwdArgs& a, ConvGenBwdPlan& p);   // false: the layer does not fit the kernel (Ck % 16, k <= 16, 32-bit offsets)
void conv_gen_bwd_launch(const ConvGenBwdPlan& p, hipStream_t s);
// the images of that launch, shared by the net and the raw entry (model_synth.hip): of a Conv1d w [Co][Ci][k] (transposed, taps flipped) and of a
// ConvTranspose1d w [Cin][Cout][k] (its own weight); rows padded to a multiple of 128
void gen_bwd_conv_image(const float* w, int Co, int Ci, int k, std::vector<uint16_t>& P);
void gen_bwd_up_image(const float* w, int Cin, int Cout, int k, std::vector<uint16_t>& P);
// the direct kernels of that pass: d = dy (1 - y^2); conv_post transposed with its input's mask; a noise convolution transposed onto the source (accumulate: added
// to dhar; out2: a second copy of the sum so far, or null); float64 row sums and the conditioning's transposed product (out2: a second copy or null)
void gen_tanh_bwd(hipStream_t s, const float* dy, const float* y, float* d, long long n);
void gen_post_bwd(hipStream_t s, const float* d, const float* w, const float* x, float* dx, int C, int k, int pad, long long T, float slope, float scale);
void gen_noise_bwd(hipStream_t s, const float* D, const float* w, float* dhar, float* out2, int C, int k, int stride, int pad, long long T, long long N, int accumulate);
void gen_row_sums(hipStream_t s, const float* D, int C, long long T, float* out, float* out2);
void gen_cond_bwd(hipStream_t s, const float* W, const float* dcond, int C, int G, float* out, float* out2);
// The transposed products of the flow's backward data pass (conv_flow_bwd.hip; model_synth.hip::flow_backward), one item per launch:
//   Y[r][n] = n < len ? sum_c sum_t W'[r][c][t] G[c][n + off0 + t] + Res[r][n] : 0,   r < R, n < N
// Wx = x3_weight_image of W' [R][Ck][nt] (gen_bwd_conv_image of the forward's layer), rows padded to RPx.  A null: G = D [Ck][ldD] with Td valid columns (zero
// outside).  A = the taped pre-gate activation [2 H][ldD] (Ck = 2 H): D holds d acts [H][ldD] and G is WN's gate read backwards, formed where the operand is
// gathered and split:  G[c] = D[c] sigmoid(A[H + c]) (1 - tanh^2(A[c])),  G[H + c] = D[c] tanh(A[c]) sigmoid'(A[H + c]),  c < H.  Res (null: none) and Y share ldY.
struct ConvFlowBwdArgs {
  const float* D; long long ldD; int Td; const float* A; int H; const unsigned char* Wx; const float* Res; float* Y; long long ldY;
  int R, RPx, Ck, N, nt, off0, len;
};
struct ConvFlowBwdPlan { ConvFlowBwdArgs a; dim3 grid; int units = 1; size_t lds = 0; };
bool conv_flow_bwd_plan(const ConvFlowBwdArgs& a, ConvFlowBwdPlan& p);   // pure; false: the layer does not fit the kernel (Ck % 16, H % 16, nt <= 16, 32-bit offsets)
void conv_flow_bwd_launch(const ConvFlowBwdPlan& p, hipStream_t s);
// the direct kernels of that pass.  flow_unflip: y[c][t] = t < len ? x[C - 1 - c][t] : 0 (Flip read backwards, with the mask), rows C / 2 .. also to dm.
// flow_gate_bwd: da = the gate's derivative above as a tensor [2 H][T] (zero behind len) and dgc[r] = its row sums in float64, rounded once.
// flow_cond_bwd: dg[g] = sum_f sum_c W_f[c][g] dgc_f[c] over the four couplings in float64, rounded once (out2: a second copy or null).
// wn_gate_record: WN's gate as wn_gate / wn_gate_split compute it (img null: acts as fp32 [H][T] in out), a += g left in place: the recorded pre-gate activation.
void flow_unflip(hipStream_t s, const float* x, float* y, float* dm, int C, int T, int len);
void flow_gate_bwd(hipStream_t s, const float* dacts, const float* a, float* da, float* dgc, int H, int T, int len);
void flow_cond_bwd(hipStream_t s, const float* const (&W)[4], const float* const (&dgc)[4], int C, int G, float* out, float* out2);
void wn_gate_record(hipStream_t s, float* a, const float* g, float* out, unsigned char* img, long long tp, int margin, int H, int T);
// The weight gradient of that convolution (conv_x3d_wgrad.hip): dW[m][c][j] = sum_s sum_n D[s][m][n] X[s][c][stride n - (stride - 1) w + (j - pad) p], both
// operands fp32 and split in the kernel, the reduction over (signal, n) cut into `splits` runs of stages (one signal, 128 columns each): split z writes the
// partial image part[z][Co][Ci k]; the caller provides part_floats floats and adds the partials in index order.  cps / per / total: filled by the planner.
struct ConvX3dWgradArgs {
  const float* D; const float* X; float* part;
  int Ci, Co, H, Hout, p, k, stride, pad, S; int cps, per, total;
};
struct ConvX3dWgradPlan { ConvX3dWgradArgs a; dim3 grid; int splits = 1; size_t lds = 0, part_floats = 0; double flops = 0.0; };
bool conv_x3d_wgrad_plan(const ConvX3dWgradArgs& a, ConvX3dWgradPlan& p);   // false: the layer does not fit the kernel (Co % 128, k <= 16, 32-bit offsets)
void conv_x3d_wgrad_launch(const ConvX3dWgradPlan& p, hipStream_t s);
// The finishing step (discriminator.hip), one workgroup per output channel m: gb[m] = the float64 sum of row m of D [S][Co][N], gw[m] (L floats) = the `splits`
// partials (pstride floats apart) added in index order, through the weight-norm chain where v / g are given (gg receives grad_g)
struct DiscWgradFinishArgs { const float* part; const float* D; const float* v; const float* g; float* gw; float* gg; float* gb; long long pstride; int splits, S, Co, N, L; };
void disc_wgrad_finish(hipStream_t s, const DiscWgradFinishArgs& a);
// The weight gradient of the generator's dense 1-D convolutions over the B items of a batch (conv_gen_wgrad.hip):
//   out[r][c k + t] = sum_item sum_n a_P(P[item][r][n]) a_G(G[item][c][cstride n + tstep t + off0]),  r < R, c < C, t < k, n < N;  a_X(v) = max(v, slope_X v), slope 1: none
// P [R][ldP] with N valid columns and G [C][ldG] with Tg valid columns (zero outside) per item, each item its own allocation: one base pointer per item.  Both
// operands fp32 and split in the kernel.  The reduction over (item, n) is cut into `splits` runs of stages (one item, 128 columns each): split z writes the partial
// image part[z][R][C k]; the caller provides part_floats (<= kGenWgradPartFloats) floats and adds the partials in index order (gen_wgrad_finish).  cps / per /
// total: filled by the planner.  R % 16 == 0.
constexpr int kGenWgradMaxItems = 16;                          // items of one pass (the kernels receive their base pointers as arguments)
constexpr size_t kGenWgradPartFloats = (size_t)16 << 20;       // bound on the partial images of one launch: 64 MiB
struct GenItems { const float* p[kGenWgradMaxItems]; };
struct ConvGenWgradArgs {
  const float* P[kGenWgradMaxItems]; const float* G[kGenWgradMaxItems]; float* part;
  int B, R, C, k, N; long long ldP, ldG; int Tg, cstride, tstep, off0; float slopeP, slopeG; int cps, per, total;
};
struct ConvGenWgradPlan { ConvGenWgradArgs a; dim3 grid; int bm = 128, splits = 1; size_t lds = 0, part_floats = 0; double flops = 0.0; };   // bm: rows per workgroup (128, 64, 32)
bool conv_gen_wgrad_plan(const ConvGenWgradArgs& a, ConvGenWgradPlan& p);   // false: the layer does not fit the kernel (R % 16, k <= 16, B <= 16, 32-bit offsets, the partial bound)
void conv_gen_wgrad_launch(const ConvGenWgradPlan& p, hipStream_t s);
// The finishing step, one workgroup per row: gw[m] = the `splits` partials (pstride floats apart) added in index order, through the weight-norm chain where v / g
// are given (gg receives grad_g); rows m < brows also write gb[m] = the float64 sum of row m (N columns) of D over the B items (gb null: no bias)
struct GenWgradFinishArgs { const float* part; long long pstride; int splits, R, L; const float* v; const float* g; float* gw; float* gg; float* gb; GenItems D; int B, brows; long long N; };
void gen_wgrad_finish(hipStream_t s, const GenWgradFinishArgs& a);
// the direct kernels of the pass (float64 sums in a fixed order): a noise convolution's weight and bias from d.up [C][T] and the source [Nh]; conv_post's weight
// from d.post [T] and lrelu_slope(x [C][T]); cond's weight [C][G] and the bias sum (written to gb and gb2) from d.cond [C] and the items' g [G]; m_source.l_linear
void gen_wgrad_noise(hipStream_t s, const GenItems& D, const GenItems& H, int B, int C, long long T, long long Nh, int k, int stride, int pad, float* gw, float* gb);
void gen_wgrad_post(hipStream_t s, const GenItems& D, const GenItems& X, int B, int C, long long T, int k, int pad, float slope, float* gw);
void gen_wgrad_cond(hipStream_t s, const GenItems& DC, const GenItems& Gv, int B, int C, int G, float* gw, float* gb, float* gb2);
void gen_wgrad_msource(hipStream_t s, const GenItems& DH, const GenItems& H, const GenItems& Sn, int B, long long N, float* gw, float* gb);
// The weight gradient of the flow's convolutions over the B items of a batch, each at its own length (conv_flow_wgrad.hip):
//   out[r][c k + t] = sum_item sum_{n < N[item]} P[item][r][n] act(G[item])[c][n + t + off0],  r < R, c < C, t < k
// P [R0][N[item]] and, for rows [R0, R), P2 [R - R0][N[item]] (R0 == R: no second tensor); gate 0: G [C][N[item]], act = identity; gate 1: G [2 C][N[item]] and
// act(G)[c] = tanh(G[c]) sigmoid(G[C + c]), formed in the kernel.  Zero outside [0, N[item]).  Both operands fp32 and split in the kernel.  The ragged reduction
// is cut into stages of one item and 128 columns (first[b]: item b's first stage, filled by the planner with per / total) and into `splits` runs of them: split z
// writes the partial image part[z][R][C k]; the caller provides part_floats (<= kGenWgradPartFloats) floats and adds them in index order (flow_wgrad_finish).
struct ConvFlowWgradArgs {
  const float* P[kGenWgradMaxItems]; const float* P2[kGenWgradMaxItems]; const float* G[kGenWgradMaxItems]; float* part;
  int N[kGenWgradMaxItems]; int first[kGenWgradMaxItems + 1];
  int B, R, R0, C, k, off0, gate; int per, total;
};
struct ConvFlowWgradPlan { ConvFlowWgradArgs a; dim3 grid; int bm = 128, splits = 1; size_t lds = 0, part_floats = 0; };   // bm: rows per workgroup (128, 64, 32)
// pure; false: R % 16, k > 16, B outside 1 .. 16, an N[item] < 1, offsets outside 32 bits, a partial image beyond kGenWgradPartFloats
bool conv_flow_wgrad_plan(const ConvFlowWgradArgs& a, ConvFlowWgradPlan& p);
void conv_flow_wgrad_launch(const ConvFlowWgradPlan& p, hipStream_t s);
// The finishing step for ragged items, one workgroup per row m: gw[m] (L floats) = the `splits` partials (pstride floats apart) added in index order - or, outer
// = 1, sum_item V[item][m] Gv[item][q] in float64 (cond_layer) - through the weight-norm chain where v / g are given (gg receives grad_g).  bias 0: none; 1: gb[m]
// = the float64 sum of row m of the pair [D (R0 rows) | D2] over every item's N[item] columns; 2: gb[m] = the float64 sum over the items of V[item][m].
struct FlowWgradFinishArgs {
  const float* part; long long pstride; int splits, R, L; const float* v; const float* g; float* gw; float* gg; float* gb;
  int bias, outer, B, R0; GenItems D, D2, V, Gv; int N[kGenWgradMaxItems];
};
void flow_wgrad_finish(hipStream_t s, const FlowWgradFinishArgs& a);
// one ConvBlockRes of 16 or 32 channels (3 x 3, 3 x 3, + x) in one launch (conv_cbr2.hip): x, out fp32 [C][H W], distinct
bool cbr2_small_eligible(const ConvLayer& c1, const ConvLayer& c2);
void cbr2_small_run(const ConvLayer& c1, const ConvLayer& c2, hipStream_t s, const float* x, int H, int W, float* out);
// one 3 x 3 convolution of 16 / 32 input and <= 64 output channels on the same structure: rows below relu_rows get the ReLU, rows >= split_row go to Y2, R added to Y's rows
bool conv3_small_eligible(const ConvLayer& L);
void conv3_small_run(const ConvLayer& L, hipStream_t s, const float* x, int H, int W, float* Y, float* Y2, int split_row, int relu_rows, const float* R);
void split_image_from_f32(hipStream_t s, const float* X, long long ldX, int C, int T, unsigned char* img, long long tp);
void split_image_to_f32(hipStream_t s, const unsigned char* img, long long tp, int C, int T, float* Y, long long ldY);

// fused multi-head attention (attention.hip): Q, K channel-major [heads*64][T], V row-major [T][heads*64], out channel-major
// out (fp32, channel-major) and / or out_img (the split-resident image of conv_x3s.hip, img_tp rows per plane) receive the result
void attention_fused(hipStream_t s, const float* Q, const float* K, long long ldqk, const float* V, long long ldv, const float* bv,
                     float* out, long long ldo, int heads, int dhead, int T, unsigned char* out_img = nullptr, long long img_tp = 0);

// ek / ev: emb_rel_k / emb_rel_v [2 win + 1][dhead] (shared by the heads): the relative-position projections are then computed inside the
// kernel (rel / pb may be null); without them rel holds Q . E_k and pb returns the band for a separate value-side projection
// attention on split-resident operands (attention_dma.hip): q / k channels in one image (head h's chunks at q_chunk0 / k_chunk0 + 4 h), V^T image
// [16-key chunk][plane][attention_vt_tp rows][16 B] (conv_x3s_run_swapped; key chunks past T zeroed by attention_vt_clear_tail)
long long attention_vt_tp(int channels);
size_t attention_vt_bytes(int channels, int T);
void attention_vt_clear_tail(hipStream_t s, unsigned char* vt_img, int channels, int T);
void attention_split(hipStream_t s, const unsigned char* qk_img, long long qk_tp, int qk_channels, int q_chunk0, int k_chunk0, const unsigned char* vt_img,
                     int heads, int dhead, int T, float scale, const float* bv, float* out, long long ldo, unsigned char* out_img, long long img_tp,
                     int win = 0, const unsigned char* ek_img = nullptr, const unsigned char* evt_img = nullptr);
void attention_split_force_kz(int kz);
// the synthesizer's text encoder (head dimension 96, window 10): emb_rel_k / emb_rel_v [2 win + 1][D] (host) -> the operand images attention_split takes
void attention_rel_images(const float* ek, const float* ev, int D, int win, std::vector<uint16_t>& ek_img, std::vector<uint16_t>& evt_img);
void attention_rel_fused(hipStream_t s, const float* Q, const float* K, long long ldqk, const float* V, long long ldv, const float* bv,
                         const float* rel, float* pb, int win, float* out, long long ldo, int heads, int dhead, int T, const float* ek = nullptr,
                         const float* ev = nullptr);

// per-launch HIP-event profiling of the conv kernels (bench.py's roofline leg)
void conv_prof_enable(bool on);
int conv_prof_collect(double* ms, double* flops, long long* launches);   // arrays of RVC_PROF_CFGS (tile configuration x {fp32 1-D, fp32 2-D, bf16x3})
const char* conv_prof_cfg_name(int i);
void conv_timing_read(unsigned long long* out8, bool reset);   // debug builds (-DRVC_CONV_TIMING): per-phase cycle sums

// ----------------------------------------------------------------------------- device memory
// Ownership: every device allocation has exactly one owner whose destructor frees it - DevBuf (a vector), OwnedConvLayer (a layer's weight images), Arena (a model's
// activation block), Mdx23::Lane (stream, event, accumulator).  Owners are move-only members of heap objects (models, indices, plans) or locals; none has static
// storage duration, so no destructor runs after the HIP runtime has shut down.  The per-stream scratch pool is the one process-wide holder: raw pointers, released
// by stream_scratch_release.  DevBuf and OwnedConvLayer reach the device only through dev_alloc / dev_upload / dev_free (a host-only program may define its own).
void* dev_alloc(size_t bytes);
void* dev_upload(const void* host, size_t bytes);   // dev_alloc + blocking copy (at least one byte is allocated: the result is never null)
template <typename T> T* dev_upload(const T* host, size_t n) { return static_cast<T*>(dev_upload(static_cast<const void*>(host), n * sizeof(T))); }
void dev_free(void* p);                             // null is a no-op
void* stream_scratch(hipStream_t s, int slot, size_t bytes);   // persistent per-(device, stream) scratch (grows on demand)
void* stream_scratch_zeroed(hipStream_t s, int slot, size_t bytes, bool* fresh = nullptr);   // zero-filled when (re)allocated; users leave it zero
void stream_scratch_release(int device);                        // frees the scratch of one device (last context of the device destroyed)

// move-only owner of one device allocation of n elements; .p / .n are read by the graphs (never written from outside)
template <typename T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  DevBuf() = default;
  ~DevBuf() { dev_free(p); }
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { dev_free(p); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  T* get() const { return p; }
  void reset() { dev_free(p); p = nullptr; n = 0; }
  void alloc(size_t cnt) { reset(); p = static_cast<T*>(dev_alloc(cnt * sizeof(T))); n = cnt; }   // uninitialised
  void upload(const T* h, size_t cnt) { reset(); p = dev_upload(h, cnt); n = cnt; }
  void upload(const std::vector<T>& h) { upload(h.data(), h.size()); }
};

// A layer that owns its five weight allocations.  Planners, eligibility questions and *_run take the plain `const ConvLayer&` it converts to; a non-owning VIEW
// is an explicit copy of that base (`ConvLayer v = owner;`), valid while the owner lives and never freed.
struct OwnedConvLayer : ConvLayer {
  OwnedConvLayer() = default;
  ~OwnedConvLayer() { free_weights(); }
  OwnedConvLayer(OwnedConvLayer&& o) noexcept : ConvLayer(o) { o.disown(); }
  OwnedConvLayer& operator=(OwnedConvLayer&& o) noexcept { if (this != &o) { free_weights(); ConvLayer::operator=(o); o.disown(); } return *this; }
  OwnedConvLayer(const OwnedConvLayer&) = delete; OwnedConvLayer& operator=(const OwnedConvLayer&) = delete;
  OwnedConvLayer(const ConvLayer&) = delete; OwnedConvLayer& operator=(const ConvLayer&) = delete;
 private:
  void disown() { Wd_ = bd_ = bd4_ = nullptr; Wx_ = Wh_ = nullptr; }
  void free_weights() { dev_free(Wd_); dev_free(bd_); dev_free(bd4_); dev_free(Wx_); dev_free(Wh_); }
};

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a device's copy of the kernel: set it once per (call site = kernel instantiation, device),
// not once per process - rvc_ctx_create takes a device id, and a second GPU driven from the same process would otherwise launch with the default
// 64 KiB limit (advisor, round 3).  Two threads racing on the first launch both set it: harmless.
#define RVC_ALLOW_BIG_LDS(kern)                                                                                                              \
  do {                                                                                                                                       \
    static std::atomic<unsigned long long> rvc_lds_mask_[4];                                                                                 \
    int rvc_dev_ = 0; (void)hipGetDevice(&rvc_dev_);                                                                                         \
    const unsigned long long rvc_bit_ = 1ull << (rvc_dev_ & 63);                                                                             \
    std::atomic<unsigned long long>& rvc_m_ = rvc_lds_mask_[(rvc_dev_ >> 6) & 3];                                                            \
    if (!(rvc_m_.load(std::memory_order_acquire) & rvc_bit_)) {                                                                              \
      RVC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));      \
      rvc_m_.fetch_or(rvc_bit_, std::memory_order_release);                                                                                  \
    }                                                                                                                                        \
  } while (0)

struct Arena {
  char* base = nullptr; size_t cap = 0, off = 0, peak = 0; bool dry = false;
  unsigned gen = 0;   // bumped whenever the block is (re)allocated or released: a cached "these bytes are known to be zero" must not survive that
  void reset() { off = 0; }
  template <typename T> T* alloc(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
    size_t o = off; off += bytes; if (off > peak) peak = off;
    if (dry) return reinterpret_cast<T*>(uintptr_t(0x1000) + o);   // never dereferenced
    RVC_REQUIRE(off <= cap, "arena overflow");
    return reinterpret_cast<T*>(base + o);
  }
  void ensure(size_t bytes);
  void release();
  Arena() = default;
  ~Arena() { release(); }
  Arena(const Arena&) = delete; Arena& operator=(const Arena&) = delete;
};

// The two passes of a model graph over its arena: a dry pass that only measures (alloc hands out addresses nobody dereferences, the graph launches nothing),
// ensure(peak), then the real pass.  `dry` is false again on every exit, a throw from either pass included.
template <typename F> void arena_passes(Arena& A, F&& graph) {
  struct Restore { Arena& a; ~Restore() { a.dry = false; } } restore{A};
  A.dry = true; A.reset(); A.peak = 0;
  graph();
  A.ensure(A.peak);
  A.dry = false; A.reset();
  graph();
}

// A block of an arena that a graph needs zero wherever no kernel writes: the margins of split-resident images are the zero padding of the convolutions that
// read them through row offsets.  The block is a graph's first allocation (nothing else ever occupies it) and is cleared only when it is not the block
// remembered as cleared: another place, another arena generation, another size, or another layout inside it - up to two integer keys, the lengths the images
// were laid out for (a shorter sequence in the same bytes leaves the longer one's rows behind its end).
struct ZeroedBlock {
  const void* base = nullptr; unsigned gen = 0; size_t bytes = 0; int key0 = -1, key1 = -1;
  bool stale(const void* b, unsigned g, size_t n, int k0, int k1) const { return base != b || gen != g || bytes != n || key0 != k0 || key1 != k1; }
  void remember(const void* b, unsigned g, size_t n, int k0, int k1) { base = b; gen = g; bytes = n; key0 = k0; key1 = k1; }
  void reset() { base = nullptr; }
  // real pass only: [start, start + n) of the arena is zero-filled on stream s when stale() says so
  void ensure_zero(const Arena& A, size_t start, size_t n, int k0, int k1, hipStream_t s) {
    if (A.dry || !stale(A.base + start, A.gen, n, k0, k1)) return;
    RVC_HIP_CHECK(hipMemsetAsync(A.base + start, 0, n, s));
    remember(A.base + start, A.gen, n, k0, k1);
  }
};

}  // namespace rvc
