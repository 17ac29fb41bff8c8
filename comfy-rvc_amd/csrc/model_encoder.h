// One post-LN transformer encoder layer, shared by HuBERT's encoder (modeling_hubert.py:340-477) and the synthesizer's text encoder (reference
// lib/infer_pack/attentions.py:13-70):  q | k | v -> attention -> out-projection + residual -> LayerNorm -> FFN1 (activation) -> FFN2 + residual -> LayerNorm.
// The two differ in their EncoderShape only; the FFN's taps (1 / 3) are part of its layers.  Host code: no kernel lives here.
#pragma once
#include "model_common.h"

namespace rvc {

struct EncoderLayer {
  OwnedConvLayer qkv;      // q (pre-scaled by head_dim^-0.5), k and v projections as one layer: C -> 3 C (the v rows carry no bias)
  DevVec bv;               // v's bias, added after P.V (softmax rows sum to 1)
  OwnedConvLayer o, ff1, ff2;
  DevVec g1, b1, g2, b2;   // LayerNorm behind the attention / behind the FFN
  // relative-position attention (window > 0) only:
  DevVec ek, ev;           // emb_rel_k / emb_rel_v [2 window + 1][head_dim]: the fused attention kernel does both projections itself
  DevVec rel_img;          // the same tables as the MFMA operand images of attention_split: E_k image, then E_v^T image (bf16 hi / lo)
  size_t evt_off = 0;      // byte offset of the E_v^T image
};

struct EncoderShape { int C, heads, dhead, window; int ffn_act; int filt; };   // channels, heads, head dimension, relative-position window (0: none), FFN activation, FFN rows

// The callers allocate (their arena offsets are theirs): h = the residual stream [C][T], in and out; hb [C][T] scratch.
struct EncoderSplitBufs { float *h, *hb; unsigned char *h_s, *qk_s, *vt_s, *attn_s, *ff_s; };   // h_s: image of h, in and out; q | k image (2 C), V^T image, attention and FFN images
struct EncoderPlainBufs { float *h, *hb, *qkv, *vr, *attn, *ff; };                              // qkv [3 C][T], vr [T][C], attn [C][T], ff [filt][T]

// Split-resident path (conv_x3s.hip, attention_dma.hip): every projection reads the image its producer wrote; fp32 copies only where a residual reads them.
inline void encoder_layer_run_split(hipStream_t s, const EncoderLayer& Y, const EncoderShape& sh, const EncoderSplitBufs& b, int T) {
  const int C = sh.C;
  const long long tp = split_image_tp(T);
  if (((2 * C) & 127) == 0) {
    // q | k | v in ONE launch: the q and k rows go to their image, the v rows through the transposing epilogue into the V^T image (v's bias after the attention)
    ConvEpilogue Eqk; Eqk.ys_out = b.qk_s; Eqk.ys_tp = tp; Eqk.vt_out = b.vt_s; Eqk.vt_tp = attention_vt_tp(C); Eqk.vt_row0 = 2 * C;
    conv_x3s_run(Y.qkv, s, b.h_s, tp, T, nullptr, T, Eqk);
  } else {
    ConvLayer qkL = Y.qkv; qkL.Co = 2 * C;                                  // a VIEW (explicit copy of the owner's base, frees nothing): the q and k rows of the 3 C-row projection -> image only
    ConvEpilogue Eqk; Eqk.ys_out = b.qk_s; Eqk.ys_tp = tp;
    conv_x3s_run(qkL, s, b.h_s, tp, T, nullptr, T, Eqk);
    conv_x3s_run_swapped(Y.qkv, 2 * C, C, s, b.h_s, tp, T, b.vt_s, attention_vt_tp(C));
  }
  // softmax(K^T Q [+ banded rel-k bias]) V + bv [+ banded P . E_v], written as the image the out-projection stages
  const unsigned char* ri = sh.window ? reinterpret_cast<const unsigned char*>(Y.rel_img.p) : nullptr;
  attention_split(s, b.qk_s, tp, 2 * C, 0, C / 16, b.vt_s, sh.heads, sh.dhead, T, 1.f, Y.bv.p, nullptr, T, b.attn_s, tp, sh.window, ri, ri ? ri + Y.evt_off : nullptr);
  ConvEpilogue Er; Er.R = b.h; Er.ldR = T;
  conv_x3s_run(Y.o, s, b.attn_s, tp, T, b.hb, T, Er);
  layernorm_c_split(s, b.hb, Y.g1.p, Y.b1.p, b.h, b.h_s, tp, kSplitMargin, C, T, T, 1e-5f);
  ConvEpilogue Ef; Ef.act = sh.ffn_act; Ef.ys_out = b.ff_s; Ef.ys_tp = tp;
  conv_x3s_run(Y.ff1, s, b.h_s, tp, T, nullptr, T, Ef);                     // activation in the epilogue, the filt-channel tensor exists only as the image (k = 3: taps are row offsets into it)
  conv_x3s_run(Y.ff2, s, b.ff_s, tp, T, b.hb, T, Er);
  layernorm_c_split(s, b.hb, Y.g2.p, Y.b2.p, b.h, b.h_s, tp, kSplitMargin, C, T, T, 1e-5f);
}

// Plain path: fp32 tensors throughout, the attention without materialising the [heads][T][T] scores (attention.hip).
inline void encoder_layer_run_plain(hipStream_t s, const EncoderLayer& Y, const EncoderShape& sh, const EncoderPlainBufs& b, int T) {
  const int C = sh.C;
  ConvEpilogue E0;
  conv1d_run(Y.qkv, s, b.h, T, T, b.qkv, T, E0);
  transpose(s, b.qkv + (size_t)2 * C * T, b.vr, C, T, T, C, 1, 0, 0);       // V row-major [T][C] (bias later)
  if (sh.window)   // both relative-position projections inside the kernel
    attention_rel_fused(s, b.qkv, b.qkv + (size_t)C * T, T, b.vr, C, Y.bv.p, nullptr, nullptr, sh.window, b.attn, T, sh.heads, sh.dhead, T, Y.ek.p, Y.ev.p);
  else
    attention_fused(s, b.qkv, b.qkv + (size_t)C * T, T, b.vr, C, Y.bv.p, b.attn, T, sh.heads, sh.dhead, T);
  ConvEpilogue Er; Er.R = b.h; Er.ldR = T;
  conv1d_run(Y.o, s, b.attn, T, T, b.hb, T, Er);
  layernorm_c(s, b.hb, nullptr, Y.g1.p, Y.b1.p, b.h, C, T, T, 1e-5f);
  ConvEpilogue Ef; Ef.act = sh.ffn_act;
  conv1d_run(Y.ff1, s, b.h, T, T, b.ff, T, Ef);
  conv1d_run(Y.ff2, s, b.ff, T, T, b.hb, T, Er);
  layernorm_c(s, b.hb, nullptr, Y.g2.p, Y.b2.p, b.h, C, T, T, 1e-5f);
}

}  // namespace rvc
