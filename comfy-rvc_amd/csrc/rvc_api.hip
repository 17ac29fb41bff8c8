// extern "C" layer of librvc_hip.so (see include/rvc_hip.h).  Every entry point converts C++ exceptions into a status code
// plus a thread-local message; nothing here has a CPU fallback.
#include "models.h"
#include "conv_kernels.h"

namespace rvc {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace rvc

using namespace rvc;

struct rvc_ctx { Ctx c; };
static std::mutex g_ctx_mu;
static std::map<int, int> g_ctx_count;       // live contexts per device (the per-stream scratch is released with the last one)
struct rvc_hubert { Hubert* m; rvc_ctx* ctx; };
struct rvc_rmvpe { Rmvpe* m; rvc_ctx* ctx; };
struct rvc_synth { Synth* m; rvc_ctx* ctx; };
struct rvc_conv1d_plan { OwnedConvLayer L; };

#define RVC_TRY try {
#define RVC_CATCH                                                            \
  return 0;                                                                  \
  }                                                                          \
  catch (const std::exception& e) { rvc::set_error(e.what()); return 1; }    \
  catch (...) { rvc::set_error("unknown error"); return 2; }

// tests / benchmarks: the forced K split / tile (conv_x3s_force) and key split (attention_split_force_kz) of the calling thread last for one scope
struct X3sForceScope {
  X3sForceScope(int ksplit, int am, int an) { conv_x3s_force(ksplit, am, an); }
  ~X3sForceScope() { conv_x3s_force(0, 0, 0); }
  X3sForceScope(const X3sForceScope&) = delete; X3sForceScope& operator=(const X3sForceScope&) = delete;
};
struct AttentionKzScope {
  explicit AttentionKzScope(int kz) { attention_split_force_kz(kz); }
  ~AttentionKzScope() { attention_split_force_kz(0); }
  AttentionKzScope(const AttentionKzScope&) = delete; AttentionKzScope& operator=(const AttentionKzScope&) = delete;
};
typedef DevBuf<unsigned char> DevBytes;
// the split-resident image of x [C][T] for a single-op entry point: every byte `fill` (0: zero margins, the taps' zero padding; 0xff: NaN patterns wherever x does not
// land, which must not reach a stored value), then x written into it - all on s
static DevBytes image_from_f32(hipStream_t s, const float* x, int C, int T, int fill) {
  DevBytes img;
  img.alloc(split_image_bytes(C, T));
  RVC_HIP_CHECK(hipMemsetAsync(img.p, fill, split_image_bytes(C, T), s));
  split_image_from_f32(s, x, T, C, T, img.p, split_image_tp(T));
  return img;
}

// the operand images of attention_split from fp32 q, k, v [C][T]: q | k in one image, V^T through a transposed fp32 copy (vtf); rows past T hold NaN patterns (masked
// keys must not leak) except the V^T tail, which attention_vt_clear_tail zeroes
static void attention_operand_images(hipStream_t s, const float* q, const float* k, const float* v, int C, int T, DevBytes& qk, DevBuf<float>& vtf, DevBytes& vt) {
  const long long tp = split_image_tp(T), vtp = attention_vt_tp(C);
  qk.alloc(split_image_bytes(2 * C, T));
  RVC_HIP_CHECK(hipMemsetAsync(qk.p, 0xff, split_image_bytes(2 * C, T), s));
  split_image_from_f32(s, q, T, C, T, qk.p, tp);
  split_image_from_f32(s, k, T, C, T, qk.p + split_image_bytes(C, T), tp);
  vtf.alloc((size_t)T * C);
  transpose(s, v, vtf.p, C, T, T, C, 1, 0, 0);
  vt.alloc(attention_vt_bytes(C, T));
  RVC_HIP_CHECK(hipMemsetAsync(vt.p, 0xff, attention_vt_bytes(C, T), s));
  split_image_from_f32(s, vtf.p, C, T, C, vt.p, vtp);                            // "channels" = keys, "positions" = model channels
  attention_vt_clear_tail(s, vt.p, C, T);
}

static void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw Error(std::string("kernel launch failed: ") + hipGetErrorString(e));
}

extern "C" {

const char* rvc_last_error(void) { return g_err.c_str(); }
const char* rvc_version(void) { return "rvc_hip 0.1.0 (gfx950, fp32 MFMA)"; }

int rvc_ctx_create(int device_id, rvc_ctx** out) {
  RVC_TRY
  int n = 0;
  RVC_HIP_CHECK(hipGetDeviceCount(&n));
  RVC_REQUIRE(n > 0 && device_id >= 0 && device_id < n, "no such HIP device (this library has no CPU path)");
  RVC_HIP_CHECK(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  RVC_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
  RVC_REQUIRE(std::string(prop.gcnArchName).find("gfx950") != std::string::npos,
              std::string("kernels are built for gfx950 only, found ") + prop.gcnArchName);
  rvc_ctx* c = new rvc_ctx();
  c->c.device = device_id;
  { std::lock_guard<std::mutex> lk(g_ctx_mu); ++g_ctx_count[device_id]; }
  *out = c;
  RVC_CATCH
}
// Destroying the LAST context of a device frees that device's per-stream scratch: the caller must not have calls in flight on that device
// from other threads at that moment (include/rvc_hip.h says so at rvc_ctx_destroy; handles of a destroyed context are dead anyway).
int rvc_ctx_destroy(rvc_ctx* ctx) {
  if (!ctx) return 0;
  bool last;
  { std::lock_guard<std::mutex> lk(g_ctx_mu); last = --g_ctx_count[ctx->c.device] <= 0; }
  if (last) { (void)hipSetDevice(ctx->c.device); stream_scratch_release(ctx->c.device); }   // per-stream scratch goes with the last context of a device
  spec_state_free(&ctx->c);
  delete ctx;
  return 0;
}
int rvc_ctx_set_conv_precision(rvc_ctx* ctx, int mode) {
  RVC_TRY
  RVC_REQUIRE(ctx && mode >= -1 && mode <= 2, "precision mode must be -1 (thread default), 0, 1 or 2");
  ctx->c.precision = mode;
  RVC_CATCH
}
int64_t rvc_ctx_workspace_bytes(rvc_ctx* ctx) { return ctx ? (int64_t)ctx->c.workspace_bytes : 0; }

// ------------------------------------------------------------------------------------------------ hubert
int rvc_hubert_create(rvc_ctx* ctx, rvc_hubert** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && out, "null argument");
  rvc_hubert* h = new rvc_hubert(); h->ctx = ctx; h->m = hubert_create(&ctx->c); *out = h;
  RVC_CATCH
}
int rvc_hubert_set_tensor(rvc_hubert* h, const char* name, const float* d, const int64_t* shape, int ndim) {
  RVC_TRY
  RVC_REQUIRE(h && name && d && ndim <= 8, "bad argument");
  long long sh[8]; for (int i = 0; i < ndim; ++i) sh[i] = shape[i];
  hubert_set_tensor(h->m, name, d, sh, ndim);
  RVC_CATCH
}
int rvc_hubert_finalize(rvc_hubert* h) { RVC_TRY RVC_REQUIRE(h, "null argument"); RVC_HIP_CHECK(hipSetDevice(h->ctx->c.device)); hubert_finalize(h->m); RVC_CATCH }
int rvc_hubert_destroy(rvc_hubert* h) { if (h) { hubert_destroy(h->m); delete h; } return 0; }
int64_t rvc_hubert_num_frames(int64_t L) { return hubert_num_frames(L); }
int rvc_hubert_forward(rvc_hubert* h, void* stream, const float* audio, int64_t L, int version, int n_layers, float* out_rm, float* out_cm,
                       const rvc_hubert_taps* taps) {
  RVC_TRY
  RVC_REQUIRE(h && audio, "null argument");
  hubert_forward(h->m, (hipStream_t)stream, audio, L, version, n_layers, out_rm, out_cm, taps);
  check_launch();
  h->ctx->c.workspace_bytes = hubert_workspace(h->m);
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ rmvpe
int rvc_rmvpe_create(rvc_ctx* ctx, rvc_rmvpe** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && out, "null argument");
  rvc_rmvpe* r = new rvc_rmvpe(); r->ctx = ctx; r->m = rmvpe_create(&ctx->c); *out = r;
  RVC_CATCH
}
int rvc_rmvpe_set_tensor(rvc_rmvpe* r, const char* name, const float* d, const int64_t* shape, int ndim) {
  RVC_TRY
  RVC_REQUIRE(r && name && d && ndim <= 8, "bad argument");
  long long sh[8]; for (int i = 0; i < ndim; ++i) sh[i] = shape[i];
  rmvpe_set_tensor(r->m, name, d, sh, ndim);
  RVC_CATCH
}
int rvc_rmvpe_finalize(rvc_rmvpe* r) { RVC_TRY RVC_REQUIRE(r, "null argument"); RVC_HIP_CHECK(hipSetDevice(r->ctx->c.device)); rmvpe_finalize(r->m); RVC_CATCH }
int rvc_rmvpe_destroy(rvc_rmvpe* r) { if (r) { rmvpe_destroy(r->m); delete r; } return 0; }
int rvc_rmvpe_forward(rvc_rmvpe* r, void* stream, const float* audio, int64_t L, float thred, float* mel, float* sal, double* f0,
                      const rvc_rmvpe_taps* taps) {
  RVC_TRY
  RVC_REQUIRE(r && audio, "null argument");
  rmvpe_forward(r->m, (hipStream_t)stream, audio, L, thred, mel, sal, f0, taps);
  check_launch();
  RVC_CATCH
}
int rvc_rmvpe_status(rvc_rmvpe* r, void* stream) {
  RVC_TRY
  RVC_REQUIRE(r, "null argument");
  // (2 = the hand-off timed out and the serial kernel behind the scan repaired it: the forward is valid; rvc_rmvpe_repaired tells)
  RVC_REQUIRE(rmvpe_status(r->m, (hipStream_t)stream) != 1,
              "RMVPE: the GRU scan's workgroups timed out waiting for each other (they need to be co-resident) and the repair pass did not run; the f0 of the last forward is invalid (NaN)");
  RVC_CATCH
}
int rvc_rmvpe_repaired(rvc_rmvpe* r, void* stream) { return (r && r->m && rmvpe_status(r->m, (hipStream_t)stream) == 2) ? 1 : 0; }
int rvc_rmvpe_debug_fault(rvc_rmvpe* r, int fault, unsigned spin_limit) { RVC_TRY RVC_REQUIRE(r, "null argument"); rmvpe_debug_fault(r->m, fault, spin_limit); RVC_CATCH }
int rvc_rmvpe_decode(rvc_rmvpe* r, void* stream, const float* sal, int64_t n, float thred, double* f0) {
  RVC_TRY
  RVC_REQUIRE(r && sal && f0 && n > 0, "bad argument");
  rmvpe_decode_rm(r->m, (hipStream_t)stream, sal, n, thred, f0);
  check_launch();
  RVC_CATCH
}
int rvc_f0_post(void* stream, const double* f0, int64_t n, double factor, double mel_min, double mel_max, int bins, int64_t* pitch, float* pitchf) {
  RVC_TRY
  RVC_REQUIRE(f0 && pitch && pitchf && n > 0 && bins > 2 && mel_max > mel_min, "bad argument");
  f0_post((hipStream_t)stream, f0, n, factor, mel_min, mel_max, bins, reinterpret_cast<long long*>(pitch), pitchf);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ crepe
struct rvc_crepe { Crepe* m; rvc_ctx* ctx; };
int rvc_crepe_create(rvc_ctx* ctx, int tiny, rvc_crepe** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && out, "null argument");
  std::unique_ptr<rvc_crepe> c(new rvc_crepe()); c->ctx = ctx; c->m = crepe_create(&ctx->c, tiny);
  *out = c.release();
  RVC_CATCH
}
int rvc_crepe_set_tensor(rvc_crepe* c, const char* name, const float* d, const int64_t* shape, int ndim) {
  RVC_TRY
  RVC_REQUIRE(c && name && d && ndim <= 8, "bad argument");
  long long sh[8]; for (int i = 0; i < ndim; ++i) sh[i] = shape[i];
  crepe_set_tensor(c->m, name, d, sh, ndim);
  RVC_CATCH
}
int rvc_crepe_finalize(rvc_crepe* c) { RVC_TRY RVC_REQUIRE(c, "null argument"); RVC_HIP_CHECK(hipSetDevice(c->ctx->c.device)); crepe_finalize(c->m); RVC_CATCH }
int rvc_crepe_destroy(rvc_crepe* c) { if (c) { crepe_destroy(c->m); delete c; } return 0; }
int64_t rvc_crepe_num_frames(int64_t L, int hop, int pad) { return crepe_num_frames(L, hop, pad); }
int rvc_crepe_forward(rvc_crepe* c, void* stream, const float* audio, int64_t L, int hop, int pad, float* probs, const rvc_crepe_taps* taps) {
  RVC_TRY
  RVC_REQUIRE(c && audio && probs && hop > 0, "bad argument");
  crepe_forward(c->m, (hipStream_t)stream, audio, L, hop, pad, probs, taps);
  check_launch();
  RVC_CATCH
}

int rvc_crepe_viterbi(void* stream, const float* probs, int64_t n, int min_bin, int max_bin, int32_t* bins, float* periodicity) {
  RVC_TRY
  RVC_REQUIRE(probs && bins && periodicity && n > 0 && n < (1 << 24) && min_bin >= 0 && max_bin <= 360 && min_bin < max_bin, "bad argument");
  crepe_viterbi((hipStream_t)stream, probs, (int)n, min_bin, max_bin, bins, periodicity);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ mdx23c
struct rvc_mdx23 { Mdx23* m; rvc_ctx* ctx; };
int rvc_mdx23_create(rvc_ctx* ctx, const rvc_mdx23_config* cfg, rvc_mdx23** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && cfg && out, "null argument");
  std::unique_ptr<rvc_mdx23> h(new rvc_mdx23()); h->ctx = ctx; h->m = mdx23_create(&ctx->c, *cfg);
  *out = h.release();
  RVC_CATCH
}
int rvc_mdx23_set_tensor(rvc_mdx23* m, const char* name, const float* d, const int64_t* shape, int ndim) {
  RVC_TRY
  RVC_REQUIRE(m && name && d && ndim <= 8, "bad argument");
  long long sh[8]; for (int i = 0; i < ndim; ++i) sh[i] = shape[i];
  mdx23_set_tensor(m->m, name, d, sh, ndim);
  RVC_CATCH
}
int rvc_mdx23_finalize(rvc_mdx23* m) { RVC_TRY RVC_REQUIRE(m, "null argument"); RVC_HIP_CHECK(hipSetDevice(m->ctx->c.device)); mdx23_finalize(m->m); RVC_CATCH }
int rvc_mdx23_destroy(rvc_mdx23* m) { if (m) { mdx23_destroy(m->m); delete m; } return 0; }
int rvc_mdx23_forward(rvc_mdx23* m, void* stream, const float* chunk, int64_t L, float* out) {
  RVC_TRY
  RVC_REQUIRE(m && chunk && out, "null argument");
  mdx23_forward(m->m, (hipStream_t)stream, chunk, L, out);
  check_launch();
  RVC_CATCH
}
int rvc_mdx23_set_streams(rvc_mdx23* m, int k) { RVC_TRY RVC_REQUIRE(m, "null argument"); mdx23_set_streams(m->m, k); RVC_CATCH }
int rvc_mdx23_demix(rvc_mdx23* m, void* stream, const float* mix, int64_t Lp, int64_t step, int64_t n_chunks, float overlap, float* acc) {
  RVC_TRY
  RVC_REQUIRE(m && mix && acc, "null argument");
  mdx23_demix(m->m, (hipStream_t)stream, mix, Lp, step, n_chunks, overlap, acc);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ synth
int rvc_synth_create(rvc_ctx* ctx, const rvc_synth_config* cfg, rvc_synth** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && cfg && out, "null argument");
  std::unique_ptr<rvc_synth> s(new rvc_synth()); s->ctx = ctx; s->m = synth_create(&ctx->c, *cfg);
  *out = s.release();
  RVC_CATCH
}
int rvc_synth_set_tensor(rvc_synth* s, const char* name, const float* d, const int64_t* shape, int ndim) {
  RVC_TRY
  RVC_REQUIRE(s && name && d && ndim <= 8, "bad argument");
  long long sh[8]; for (int i = 0; i < ndim; ++i) sh[i] = shape[i];
  synth_set_tensor(s->m, name, d, sh, ndim);
  RVC_CATCH
}
int rvc_synth_finalize(rvc_synth* s) { RVC_TRY RVC_REQUIRE(s, "null argument"); RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device)); synth_finalize(s->m); RVC_CATCH }
int rvc_synth_destroy(rvc_synth* s) { if (s) { synth_destroy(s->m); delete s; } return 0; }
int rvc_synth_upp(rvc_synth* s) { return s ? synth_upp(s->m) : 0; }
int rvc_synth_has_f0(rvc_synth* s) { return (s && synth_has_f0(s->m)) ? 1 : 0; }
// pitch / pitchf / noise_src belong to the f0 family only: a no-f0 model takes (and must be given) NULL for all three
static void check_pitch_args(rvc_synth* s, const void* pitch, const void* pitchf, const void* noise_src, int do_protect) {
  if (synth_has_f0(s->m)) {
    RVC_REQUIRE(pitch && pitchf && noise_src, "this model was trained with f0: pitch, pitchf and the source noise are required");
  } else {
    RVC_REQUIRE(!pitch && !pitchf && !noise_src && !do_protect, "no-f0 model: pitch, pitchf, source noise must be NULL and protect off");
  }
}
int rvc_synth_has_posterior(rvc_synth* s) { return (s && synth_has_posterior(s->m)) ? 1 : 0; }
int rvc_synth_forward(rvc_synth* s, void* stream, const float* phone, int phone_cm, const int64_t* pitch, const float* pitchf, const float* spec, int sid,
                      const float* noise_q, const float* noise_src, int64_t T, int64_t ids, float* out, const rvc_synth_forward_taps* taps) {
  RVC_TRY
  RVC_REQUIRE(s && phone && spec && noise_q && out, "null argument");
  RVC_REQUIRE(T > 0 && T < (1LL << 24), "bad sequence length");
  check_pitch_args(s, pitch, pitchf, noise_src, 0);
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_forward(s->m, (hipStream_t)stream, phone, phone_cm, (const long long*)pitch, pitchf, spec, sid, noise_q, noise_src, (int)T,
                (int)std::max<int64_t>(-1, std::min<int64_t>(ids, T)), out, taps);
  check_launch();
  RVC_CATCH
}
struct rvc_gen_tape { rvc_synth* s; GenTape* t; };
int rvc_gen_tape_create(rvc_synth* s, rvc_gen_tape** out) {
  RVC_TRY
  RVC_REQUIRE(s && out, "null argument");
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  std::unique_ptr<rvc_gen_tape> t(new rvc_gen_tape{s, nullptr});
  t->t = gen_tape_create(s->m);
  *out = t.release();
  RVC_CATCH
}
int rvc_gen_tape_release(rvc_gen_tape* t) { if (t) { gen_tape_destroy(t->t); delete t; } return 0; }
int64_t rvc_gen_tape_bytes(rvc_gen_tape* t) { return t ? (int64_t)gen_tape_bytes(t->t) : 0; }
int rvc_gen_tape_timing(rvc_gen_tape* t, int on) { RVC_TRY RVC_REQUIRE(t, "null argument"); gen_tape_timing(t->t, on != 0); RVC_CATCH }
int rvc_gen_tape_times(rvc_gen_tape* t, float* ms_host, int cap) {
  try { RVC_REQUIRE(t && ms_host && cap > 0, "bad argument"); return gen_tape_times(t->t, ms_host, cap); }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_gen_tape_tensor(rvc_gen_tape* t, const char* name, float** ptr, int* rows, int64_t* cols) {
  RVC_TRY
  RVC_REQUIRE(t && name && ptr && rows && cols, "null argument");
  long long c = 0;
  RVC_REQUIRE(gen_tape_tensor(t->t, name, ptr, rows, &c), std::string("the tape holds no tensor '") + name + "'");
  *cols = c;
  RVC_CATCH
}
int rvc_synth_forward_tape(rvc_synth* s, void* stream, const float* phone, int phone_cm, const int64_t* pitch, const float* pitchf, const float* spec, int sid,
                           const float* noise_q, const float* noise_src, int64_t T, int64_t ids, float* out, const rvc_synth_forward_taps* taps,
                           rvc_gen_tape* tape) {
  RVC_TRY
  RVC_REQUIRE(s && phone && spec && noise_q && out && tape, "null argument");
  RVC_REQUIRE(T > 0 && T < (1LL << 24), "bad sequence length");
  check_pitch_args(s, pitch, pitchf, noise_src, 0);
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_forward_tape(s->m, (hipStream_t)stream, phone, phone_cm, (const long long*)pitch, pitchf, spec, sid, noise_q, noise_src, (int)T,
                     (int)std::max<int64_t>(-1, std::min<int64_t>(ids, T)), out, taps, tape->t);
  check_launch();
  RVC_CATCH
}
int rvc_synth_forward_tape_flow(rvc_synth* s, void* stream, const float* phone, int phone_cm, const int64_t* pitch, const float* pitchf, const float* spec, int sid,
                                const float* noise_q, const float* noise_src, int64_t T, int64_t ids, float* out, const rvc_synth_forward_taps* taps,
                                rvc_gen_tape* tape, int record_flow) {
  RVC_TRY
  RVC_REQUIRE(s && phone && spec && noise_q && out && tape, "null argument");
  RVC_REQUIRE(T > 0 && T < (1LL << 24), "bad sequence length");
  check_pitch_args(s, pitch, pitchf, noise_src, 0);
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_forward_tape(s->m, (hipStream_t)stream, phone, phone_cm, (const long long*)pitch, pitchf, spec, sid, noise_q, noise_src, (int)T,
                     (int)std::max<int64_t>(-1, std::min<int64_t>(ids, T)), out, taps, tape->t, record_flow != 0);
  check_launch();
  RVC_CATCH
}
int rvc_synth_flow_input_grad(rvc_synth* s, void* stream, rvc_gen_tape* tape, const float* dz_p, int64_t T, float* dz, float* dg) {
  RVC_TRY
  RVC_REQUIRE(s && tape && dz_p && dz, "null argument");
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_flow_input_grad(s->m, (hipStream_t)stream, tape->t, dz_p, T, dz, dg);
  check_launch();
  RVC_CATCH
}
int rvc_synth_flow_input_grad_launch_count(rvc_synth* s) {
  try { return s ? synth_flow_input_grad_launch_count(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_gen_tape_flow_times(rvc_gen_tape* t, float* ms_host, int cap) {
  try { RVC_REQUIRE(t && ms_host && cap >= 2, "bad argument"); return gen_tape_flow_times(t->t, ms_host, cap); }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_synth_dec_input_grad(rvc_synth* s, void* stream, rvc_gen_tape* tape, const float* dy_hat, float* dz, float* dcond, float* dg, float* dhar) {
  RVC_TRY
  RVC_REQUIRE(s && tape && dy_hat && dz, "null argument");
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_dec_input_grad(s->m, (hipStream_t)stream, tape->t, dy_hat, dz, dcond, dg, dhar);
  check_launch();
  RVC_CATCH
}
int rvc_synth_dec_input_grad_launch_count(rvc_synth* s) {
  try { return s ? synth_dec_input_grad_launch_count(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_synth_keep_parameters(rvc_synth* s, int on) { RVC_TRY RVC_REQUIRE(s, "null argument"); synth_keep_parameters(s->m, on != 0); RVC_CATCH }
int rvc_synth_dec_param_count(rvc_synth* s) {
  try { return s ? synth_dec_param_count(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_synth_dec_param_info(rvc_synth* s, int k, char* name, int name_cap, int64_t* shape, int* ndim) {
  RVC_TRY
  RVC_REQUIRE(s && name && name_cap > 0 && shape && ndim, "null argument");
  std::string n; std::vector<long long> sh;
  synth_dec_param_info(s->m, k, n, sh);
  RVC_REQUIRE((int)n.size() < name_cap && sh.size() <= 8, "name buffer too small");
  std::copy(n.begin(), n.end(), name); name[n.size()] = 0;
  for (size_t i = 0; i < sh.size(); ++i) shape[i] = sh[i];
  *ndim = (int)sh.size();
  RVC_CATCH
}
int64_t rvc_synth_dec_param_total(rvc_synth* s) {
  try { return s ? (int64_t)synth_dec_param_total(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_synth_dec_weight_grad(rvc_synth* s, void* stream, rvc_gen_tape* const* tapes, int B, float* const* grads_dev) {
  RVC_TRY
  RVC_REQUIRE(s && tapes && grads_dev, "null argument");
  RVC_REQUIRE(B >= 1 && B <= kGenWgradMaxItems, "1 <= B <= " + std::to_string(kGenWgradMaxItems) + " tapes per weight-gradient pass");
  GenTape* t[kGenWgradMaxItems];
  for (int b = 0; b < B; ++b) { RVC_REQUIRE(tapes[b], "null tape"); t[b] = tapes[b]->t; }
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_dec_weight_grad(s->m, (hipStream_t)stream, t, B, grads_dev);
  check_launch();
  RVC_CATCH
}
int rvc_synth_dec_weight_grad_launch_count(rvc_synth* s) {
  try { return s ? synth_dec_weight_grad_launch_count(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_gen_tape_wgrad_times(rvc_gen_tape* t, float* ms_host, int cap) {
  try { RVC_REQUIRE(t && ms_host && cap > 0, "bad argument"); return gen_tape_wgrad_times(t->t, ms_host, cap); }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
// what the pure *_plan queries report (include/rvc_hip.h, single ops): units, rows per workgroup, splits, the grid, stages, stages per split
static void plan_info(int* info, int units, int bm, int splits, dim3 grid, int stages, int per) {
  if (!info) return;
  const int v[8] = {units, bm, splits, (int)grid.x, (int)grid.y, (int)grid.z, stages, per};
  std::copy(v, v + 8, info);
}
static ConvGenWgradArgs conv1d_wgrad_args(int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride, int tstep, int off0, float slope_p, float slope_g) {
  RVC_REQUIRE(N >= 1 && N < (1LL << 31) && Tg >= 1 && Tg < (1LL << 31), "bad length");
  ConvGenWgradArgs a{};
  a.B = B; a.R = R; a.C = C; a.k = k; a.N = (int)N; a.ldP = N; a.ldG = Tg; a.Tg = (int)Tg; a.cstride = cstride; a.tstep = tstep; a.off0 = off0; a.slopeP = slope_p; a.slopeG = slope_g;
  return a;
}
int rvc_conv1d_weight_grad_plan(int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride, int tstep, int off0, int* info) {
  try {
    ConvGenWgradPlan p;
    RVC_REQUIRE(conv_gen_wgrad_plan(conv1d_wgrad_args(B, R, C, k, N, Tg, cstride, tstep, off0, 1.f, 1.f), p), "the shape does not fit the weight-gradient kernel");
    plan_info(info, 8, p.bm, p.splits, p.grid, p.a.total, p.a.per);
    return p.splits;
  } catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_conv1d_weight_grad_splits(int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride, int tstep, int off0) {
  return rvc_conv1d_weight_grad_plan(B, R, C, k, N, Tg, cstride, tstep, off0, nullptr);
}
int rvc_conv1d_weight_grad(void* stream, const float* const* p_dev, const float* const* g_dev, int B, int R, int C, int k, int64_t N, int64_t Tg, int cstride,
                           int tstep, int off0, float slope_p, float slope_g, float* out_dev) {
  RVC_TRY
  RVC_REQUIRE(p_dev && g_dev && out_dev, "null argument");
  ConvGenWgradArgs a = conv1d_wgrad_args(B, R, C, k, N, Tg, cstride, tstep, off0, slope_p, slope_g);
  ConvGenWgradPlan p;
  RVC_REQUIRE(conv_gen_wgrad_plan(a, p), "the shape does not fit the weight-gradient kernel");
  for (int b = 0; b < B; ++b) { RVC_REQUIRE(p_dev[b] && g_dev[b], "null operand pointer"); p.a.P[b] = p_dev[b]; p.a.G[b] = g_dev[b]; }
  hipStream_t st = (hipStream_t)stream;
  p.a.part = (float*)stream_scratch(st, 25, p.part_floats * sizeof(float));
  conv_gen_wgrad_launch(p, st);
  GenWgradFinishArgs f{};
  f.part = p.a.part; f.pstride = (long long)R * C * k; f.splits = p.splits; f.R = R; f.L = C * k; f.gw = out_dev;
  gen_wgrad_finish(st, f);
  check_launch();
  RVC_CATCH
}
// ---- the flow's parameter gradients
int rvc_synth_flow_param_count(rvc_synth* s) {
  try { return s ? synth_flow_param_count(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_synth_flow_param_info(rvc_synth* s, int k, char* name, int name_cap, int64_t* shape, int* ndim) {
  RVC_TRY
  RVC_REQUIRE(s && name && name_cap > 0 && shape && ndim, "null argument");
  std::string n; std::vector<long long> sh;
  synth_flow_param_info(s->m, k, n, sh);
  RVC_REQUIRE((int)n.size() < name_cap && sh.size() <= 8, "name buffer too small");
  std::copy(n.begin(), n.end(), name); name[n.size()] = 0;
  for (size_t i = 0; i < sh.size(); ++i) shape[i] = sh[i];
  *ndim = (int)sh.size();
  RVC_CATCH
}
int64_t rvc_synth_flow_param_total(rvc_synth* s) {
  try { return s ? (int64_t)synth_flow_param_total(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_synth_flow_weight_grad(rvc_synth* s, void* stream, rvc_gen_tape* const* tapes, int B, float* const* grads_dev) {
  RVC_TRY
  RVC_REQUIRE(s && tapes && grads_dev, "null argument");
  RVC_REQUIRE(B >= 1 && B <= kGenWgradMaxItems, "1 <= B <= " + std::to_string(kGenWgradMaxItems) + " tapes per weight-gradient pass");
  GenTape* t[kGenWgradMaxItems];
  for (int b = 0; b < B; ++b) { RVC_REQUIRE(tapes[b], "null tape"); t[b] = tapes[b]->t; }
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));
  synth_flow_weight_grad(s->m, (hipStream_t)stream, t, B, grads_dev);
  check_launch();
  RVC_CATCH
}
int rvc_synth_flow_weight_grad_launch_count(rvc_synth* s) {
  try { return s ? synth_flow_weight_grad_launch_count(s->m) : -1; }
  catch (const std::exception& e) { set_error(e.what()); return -1; }
}
// the raw GEMM of that pass: one pointer per item, item b's operands laid out for its own length n_host[b]
static ConvFlowWgradArgs gated_wgrad_args(int B, int R, int C, int k, const int64_t* n_host, int off0, int gate) {
  RVC_REQUIRE(n_host, "null argument");
  RVC_REQUIRE(B >= 1 && B <= kGenWgradMaxItems, "1 <= B <= " + std::to_string(kGenWgradMaxItems) + " items");
  ConvFlowWgradArgs a{};
  for (int b = 0; b < B; ++b) { RVC_REQUIRE(n_host[b] >= 1 && n_host[b] < (1LL << 31), "bad length"); a.N[b] = (int)n_host[b]; }
  a.B = B; a.R = R; a.R0 = R; a.C = C; a.k = k; a.off0 = off0; a.gate = gate;
  return a;
}
int rvc_gated_conv1d_weight_grad_plan(int B, int R, int C, int k, const int64_t* n_host, int off0, int gate, int* info) {
  try {
    ConvFlowWgradPlan p;
    RVC_REQUIRE(conv_flow_wgrad_plan(gated_wgrad_args(B, R, C, k, n_host, off0, gate), p), "the shape does not fit the weight-gradient kernel");
    plan_info(info, 8, p.bm, p.splits, p.grid, p.a.total, p.a.per);
    return p.splits;
  } catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_gated_conv1d_weight_grad(void* stream, const float* const* p_dev, const float* const* g_dev, int B, int R, int C, int k, const int64_t* n_host, int off0,
                                 int gate, float* out_dev) {
  RVC_TRY
  RVC_REQUIRE(p_dev && g_dev && out_dev, "null argument");
  ConvFlowWgradPlan p;
  RVC_REQUIRE(conv_flow_wgrad_plan(gated_wgrad_args(B, R, C, k, n_host, off0, gate), p), "the shape does not fit the weight-gradient kernel");
  for (int b = 0; b < B; ++b) { RVC_REQUIRE(p_dev[b] && g_dev[b], "null operand pointer"); p.a.P[b] = p.a.P2[b] = p_dev[b]; p.a.G[b] = g_dev[b]; }
  hipStream_t st = (hipStream_t)stream;
  p.a.part = (float*)stream_scratch(st, 25, p.part_floats * sizeof(float));
  conv_flow_wgrad_launch(p, st);
  FlowWgradFinishArgs f{};
  f.part = p.a.part; f.pstride = (long long)R * C * k; f.splits = p.splits; f.R = R; f.L = C * k; f.gw = out_dev; f.B = B; f.R0 = R;
  flow_wgrad_finish(st, f);
  check_launch();
  RVC_CATCH
}
// ---- raw entries of the other four bf16x3 gather GEMMs (conv_x3d*.hip, conv_gen_bwd.hip), stated as the forward operation: the weights come from the host in
// the module's layout and go through the regrouping the nets use.  info (8 ints, may be null): units, bm, splits, grid x / y / z, stages, stages per split
static const float kNoDevice = 0.f;      // a non-null pointer for the planners' pure queries: nothing dereferences it
static ConvX3dArgs disc_conv_args(int S, int Ci, int Co, int H, int p, int k, int stride, int pad, float slope) {
  RVC_REQUIRE(H >= 1 && k >= 1 && stride >= 1 && pad >= 0 && H + 2 * pad >= k, "bad geometry");
  ConvX3dArgs a{};
  a.X = &kNoDevice; a.Wx = reinterpret_cast<const unsigned char*>(&kNoDevice); a.bias = &kNoDevice;
  a.Ci = Ci; a.Co = Co; a.CoPx = Co; a.H = H; a.Hout = (H + 2 * pad - k) / stride + 1; a.p = p; a.k = k; a.stride = stride; a.pad = pad; a.S = S; a.slope = slope;
  return a;
}
int rvc_op_disc_conv_plan(int S, int Ci, int Co, int H, int p, int k, int stride, int pad, int* info) {
  try {
    ConvX3dPlan pl;
    RVC_REQUIRE(conv_x3d_plan(disc_conv_args(S, Ci, Co, H, p, k, stride, pad, 1.f), pl), "the shape does not fit the GEMM kernel");
    plan_info(info, pl.units, 128, 1, pl.grid, (Ci / 16) * k / pl.units, 0);
    return pl.units;
  } catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_op_disc_conv(void* stream, const float* x, const float* w, const float* bias, float* y, int S, int Ci, int Co, int H, int p, int k, int stride, int pad,
                     float slope, int* units) {
  RVC_TRY
  RVC_REQUIRE(x && w && bias && y, "null argument");
  RVC_REQUIRE(slope >= 0.f && slope <= 1.f, "0 <= slope <= 1");
  ConvX3dArgs a = disc_conv_args(S, Ci, Co, H, p, k, stride, pad, slope);
  ConvX3dPlan pl;
  RVC_REQUIRE(conv_x3d_plan(a, pl), "the shape does not fit the GEMM kernel");
  std::vector<uint16_t> img;
  x3_weight_image(w, Co, Ci, k, Co, img);
  DevBuf<uint16_t> wx; wx.upload(img);
  DevBuf<float> b; b.upload(bias, (size_t)Co);
  pl.a.X = x; pl.a.Wx = reinterpret_cast<const unsigned char*>(wx.p); pl.a.bias = b.p; pl.a.Y = y;
  hipStream_t st = (hipStream_t)stream;
  conv_x3d_launch(pl, st);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(st));
  if (units) *units = pl.units;
  RVC_CATCH
}
static ConvX3dBwdArgs disc_conv_bwd_args(int S, int Ci, int Co, int H, int Hd, int p, int stride, float slope) {
  RVC_REQUIRE(stride == 1 || stride == 3, "stride 1 or 3");
  RVC_REQUIRE(Ci >= 1 && Co >= 16 && Co % 16 == 0, "output channels a multiple of 16");
  ConvX3dBwdArgs a{};
  for (int r = 0; r < stride; ++r) a.Wx[r] = reinterpret_cast<const unsigned char*>(&kNoDevice);
  disc_bwd_geometry(a, Ci, Co, 5, stride, 2, H, Hd, p, S, slope);
  return a;
}
static int bwd_min_stages(const ConvX3dBwdPlan& pl) {
  int stages = 1 << 30;
  for (int r = 0; r < pl.a.nph; ++r) if (pl.a.Hj[r] > 0) stages = std::min(stages, (pl.a.Ck / 16) * pl.a.nt[r] / pl.units);
  return stages;
}
int rvc_op_disc_conv_input_grad_plan(int S, int Ci, int Co, int H, int Hd, int p, int stride, int* info) {
  try {
    ConvX3dBwdPlan pl;
    RVC_REQUIRE(conv_x3d_bwd_plan(disc_conv_bwd_args(S, Ci, Co, H, Hd, p, stride, 1.f), pl), "the shape does not fit the data-gradient kernel");
    plan_info(info, pl.units, 128, 1, pl.grid, bwd_min_stages(pl), 0);
    return pl.units;
  } catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_op_disc_conv_input_grad(void* stream, const float* d, const float* w, const float* cot, const float* act, float* y, int S, int Ci, int Co, int H, int Hd,
                                int p, int stride, float slope, int* units) {
  RVC_TRY
  RVC_REQUIRE(d && w && act && y, "null argument");
  ConvX3dBwdArgs a = disc_conv_bwd_args(S, Ci, Co, H, Hd, p, stride, slope);
  std::vector<uint16_t> img[3]; int nt[3];
  const int nph = disc_bwd_weight_images(w, Co, Ci, 5, stride, 2, img, nt);
  DevBuf<uint16_t> wx[3];
  for (int r = 0; r < nph; ++r) { RVC_REQUIRE(nt[r] == a.nt[r], "phase taps"); wx[r].upload(img[r]); a.Wx[r] = reinterpret_cast<const unsigned char*>(wx[r].p); }
  a.D = d; a.Cot = cot; a.A = act; a.Y = y;
  ConvX3dBwdPlan pl;
  RVC_REQUIRE(conv_x3d_bwd_plan(a, pl), "the shape does not fit the data-gradient kernel");
  hipStream_t st = (hipStream_t)stream;
  conv_x3d_bwd_launch(pl, st);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(st));
  if (units) *units = pl.units;
  RVC_CATCH
}
static ConvX3dWgradArgs disc_conv_wgrad_args(int S, int Ci, int Co, int H, int p, int k, int stride, int pad) {
  RVC_REQUIRE(H >= 1 && k >= 1 && stride >= 1 && pad >= 0 && H + 2 * pad >= k, "bad geometry");
  return ConvX3dWgradArgs{nullptr, nullptr, nullptr, Ci, Co, H, (H + 2 * pad - k) / stride + 1, p, k, stride, pad, S, 0, 0, 0};
}
int rvc_op_disc_conv_weight_grad_plan(int S, int Ci, int Co, int H, int p, int k, int stride, int pad, int* info) {
  try {
    ConvX3dWgradPlan pl;
    RVC_REQUIRE(conv_x3d_wgrad_plan(disc_conv_wgrad_args(S, Ci, Co, H, p, k, stride, pad), pl), "the shape does not fit the weight-gradient kernel");
    plan_info(info, 8, 128, pl.splits, pl.grid, pl.a.total, pl.a.per);
    return pl.splits;
  } catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_op_disc_conv_weight_grad(void* stream, const float* d, const float* x, float* dw, int S, int Ci, int Co, int H, int p, int k, int stride, int pad, int* splits) {
  RVC_TRY
  RVC_REQUIRE(d && x && dw, "null argument");
  ConvX3dWgradPlan pl;
  RVC_REQUIRE(conv_x3d_wgrad_plan(disc_conv_wgrad_args(S, Ci, Co, H, p, k, stride, pad), pl), "the shape does not fit the weight-gradient kernel");
  RVC_REQUIRE((long long)Co * Ci * k < (1LL << 31) && (long long)pl.a.Hout * p < (1LL << 31), "layer too large");
  hipStream_t st = (hipStream_t)stream;
  DevBuf<float> part, gb;
  part.alloc(pl.part_floats); gb.alloc((size_t)Co);
  pl.a.D = d; pl.a.X = x; pl.a.part = part.p;
  conv_x3d_wgrad_launch(pl, st);
  DiscWgradFinishArgs f{};
  f.part = part.p; f.D = d; f.gw = dw; f.gb = gb.p; f.pstride = (long long)Co * Ci * k; f.splits = pl.splits; f.S = S; f.Co = Co; f.N = pl.a.Hout * p; f.L = Ci * k;
  disc_wgrad_finish(st, f);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(st));
  if (splits) *splits = pl.splits;
  RVC_CATCH
}
static ConvGenBwdArgs conv1d_bwd_args(int transposed, int Ci, int Co, int k, int step, int pad, int64_t N, int64_t Td, int64_t ldD, int64_t ldY, float slope,
                                      float scale, int accumulate) {
  RVC_REQUIRE(N >= 1 && N < (1LL << 31) && Td >= 1 && Td < (1LL << 31) && k >= 1 && step >= 1 && pad >= 0, "bad geometry");
  ConvGenBwdArgs a{};
  a.D = &kNoDevice; a.Wx = reinterpret_cast<const unsigned char*>(&kNoDevice); a.Y = const_cast<float*>(&kNoDevice);
  a.ldD = ldD; a.Td = (int)Td; a.ldY = ldY; a.R = Ci; a.RPx = (Ci + 127) & ~127; a.Ck = Co; a.N = (int)N; a.nt = k;
  if (transposed) { a.cstride = step; a.tstep = 1; a.off0 = -pad; }                       // ConvTranspose1d(Ci, Co, k, stride = step, pad)
  else { a.cstride = 1; a.tstep = step; a.off0 = pad - (k - 1) * step; }                    // Conv1d(Ci, Co, k, dilation = step, pad)
  a.slope = slope; a.scale = scale; a.accumulate = accumulate;
  return a;
}
int rvc_op_conv1d_input_grad_plan(int transposed, int Ci, int Co, int k, int step, int pad, int64_t N, int64_t Td, int* info) {
  try {
    ConvGenBwdPlan pl;
    RVC_REQUIRE(conv_gen_bwd_plan(conv1d_bwd_args(transposed, Ci, Co, k, step, pad, N, Td, Td, N, 1.f, 1.f, 0), pl), "the shape does not fit the data-gradient kernel");
    plan_info(info, pl.units, pl.bm, 1, pl.grid, (Co / 16) * k / pl.units, 0);
    return pl.units;
  } catch (const std::exception& e) { set_error(e.what()); return -1; }
}
int rvc_op_conv1d_input_grad(void* stream, const float* d, const float* w, const float* act, const float* res, float* y, int transposed, int Ci, int Co, int k,
                             int step, int pad, int64_t N, int64_t Td, int64_t ldD, int64_t ldY, float slope, float scale, int accumulate, int* bm, int* units) {
  RVC_TRY
  RVC_REQUIRE(d && w && y, "null argument");
  ConvGenBwdArgs a = conv1d_bwd_args(transposed, Ci, Co, k, step, pad, N, Td, ldD, ldY, slope, scale, accumulate);
  std::vector<uint16_t> img;
  if (transposed) gen_bwd_up_image(w, Ci, Co, k, img); else gen_bwd_conv_image(w, Co, Ci, k, img);
  DevBuf<uint16_t> wx; wx.upload(img);
  a.D = d; a.Wx = reinterpret_cast<const unsigned char*>(wx.p); a.A = act; a.Res = res; a.Y = y;
  ConvGenBwdPlan pl;
  RVC_REQUIRE(conv_gen_bwd_plan(a, pl), "the shape does not fit the data-gradient kernel");
  hipStream_t st = (hipStream_t)stream;
  conv_gen_bwd_launch(pl, st);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(st));
  if (bm) *bm = pl.bm;
  if (units) *units = pl.units;
  RVC_CATCH
}
int rvc_kl_loss_grad(void* stream, const float* z_p, const float* m_p, const float* logs_p, int C, int64_t T_pitch, int64_t len, float scale, float* dz_p,
                     float* dlogs_q, float* dm_p, float* dlogs_p) {
  RVC_TRY
  RVC_REQUIRE(z_p && m_p && logs_p && dz_p && dlogs_q && dm_p && dlogs_p, "null argument");
  kl_loss_grad((hipStream_t)stream, z_p, m_p, logs_p, C, T_pitch, len, scale, dz_p, dlogs_q, dm_p, dlogs_p);
  check_launch();
  RVC_CATCH
}
int rvc_kl_loss(void* stream, const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, int C, int64_t T_pitch, int64_t len, double* sum) {
  RVC_TRY
  RVC_REQUIRE(z_p && logs_q && m_p && logs_p && sum, "null argument");
  kl_loss_sum((hipStream_t)stream, z_p, logs_q, m_p, logs_p, C, T_pitch, len, sum);
  check_launch();
  RVC_CATCH
}
int rvc_l1_sum(void* stream, const float* a, const float* b, int64_t n, double* sum) {
  RVC_TRY
  RVC_REQUIRE(a && b && sum, "null argument");
  l1_sum((hipStream_t)stream, a, b, n, sum);
  check_launch();
  RVC_CATCH
}
// ------------------------------------------------------------------------------------------------ discriminators
struct rvc_disc { Disc* m; rvc_ctx* ctx; };
int rvc_disc_create(rvc_ctx* ctx, int version, rvc_disc** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && out, "null argument");
  std::unique_ptr<rvc_disc> d(new rvc_disc()); d->ctx = ctx; d->m = disc_create(&ctx->c, version);
  *out = d.release();
  RVC_CATCH
}
int rvc_disc_set_tensor(rvc_disc* d, const char* name, const float* data, const int64_t* shape, int ndim) {
  RVC_TRY
  RVC_REQUIRE(d && name && data && ndim <= 8, "bad argument");
  long long sh[8]; for (int i = 0; i < ndim; ++i) sh[i] = shape[i];
  disc_set_tensor(d->m, name, data, sh, ndim);
  RVC_CATCH
}
int rvc_disc_finalize(rvc_disc* d) { RVC_TRY RVC_REQUIRE(d, "null argument"); RVC_HIP_CHECK(hipSetDevice(d->ctx->c.device)); disc_finalize(d->m); RVC_CATCH }
int rvc_disc_release(rvc_disc* d) { if (d) { disc_destroy(d->m); delete d; } return 0; }
int rvc_disc_count(rvc_disc* d) { return d ? disc_count(d->m) : 0; }
int rvc_disc_num_taps(rvc_disc* d, int i) { return d && i >= 0 && i < disc_count(d->m) ? disc_num_taps(d->m, i) : 0; }
int rvc_disc_tap_shape(rvc_disc* d, int i, int tap, int64_t T, int* C, int* H, int* p) {
  RVC_TRY
  RVC_REQUIRE(d && C && H && p, "null argument");
  disc_tap_shape(d->m, i, tap, T, C, H, p);
  RVC_CATCH
}
int rvc_disc_launch_count(rvc_disc* d, int S, int64_t T) {
  try { RVC_REQUIRE(d, "null argument"); return disc_launch_count(d->m, S, T); }
  catch (const std::exception& e) { rvc::set_error(e.what()); return -1; }
}
int rvc_disc_forward(rvc_disc* d, void* stream, const float* signals, int S, int64_t T, float* const* scores, float* const* fmaps) {
  RVC_TRY
  RVC_REQUIRE(d && signals && fmaps, "null argument");
  disc_forward(d->m, (hipStream_t)stream, signals, S, T, scores, fmaps);
  check_launch();
  RVC_CATCH
}
int rvc_sqerr_sums(void* stream, const float* const* x, const int64_t* n, const float* c, int K, double* sums) {
  RVC_TRY
  RVC_REQUIRE(x && n && c && sums && K >= 1 && K <= 64, "1 <= K <= 64 segments, no null argument");
  long long nn[64]; for (int k = 0; k < K; ++k) nn[k] = n[k];
  sqerr_sums((hipStream_t)stream, x, nn, c, K, sums);
  check_launch();
  RVC_CATCH
}
int rvc_l1_sums(void* stream, const float* const* a, const float* const* b, const int64_t* n, int K, double* sums) {
  RVC_TRY
  RVC_REQUIRE(a && b && n && sums && K >= 1 && K <= 64, "1 <= K <= 64 segments, no null argument");
  long long nn[64]; for (int k = 0; k < K; ++k) nn[k] = n[k];
  l1_sums((hipStream_t)stream, a, b, nn, K, sums);
  check_launch();
  RVC_CATCH
}
int rvc_disc_input_grad_launch_count(rvc_disc* d, int S, int64_t T) {
  try { RVC_REQUIRE(d, "null argument"); return disc_input_grad_launch_count(d->m, S, T); }
  catch (const std::exception& e) { rvc::set_error(e.what()); return -1; }
}
int rvc_disc_input_grad(rvc_disc* d, void* stream, int S, int64_t T, const float* const* fmaps, const float* const* dtaps, float* const* work, float* dsignals) {
  RVC_TRY
  RVC_REQUIRE(d && fmaps && dtaps && work && dsignals, "null argument");
  disc_input_grad(d->m, (hipStream_t)stream, S, T, fmaps, dtaps, work, dsignals);
  check_launch();
  RVC_CATCH
}
int rvc_disc_keep_parameters(rvc_disc* d, int on) { RVC_TRY RVC_REQUIRE(d, "null argument"); disc_keep_parameters(d->m, on != 0); RVC_CATCH }
int rvc_disc_param_count(rvc_disc* d) {
  try { RVC_REQUIRE(d, "null argument"); return disc_param_count(d->m); }
  catch (const std::exception& e) { rvc::set_error(e.what()); return -1; }
}
int rvc_disc_param_info(rvc_disc* d, int k, char* name, int name_cap, int64_t* shape, int* ndim) {
  RVC_TRY
  RVC_REQUIRE(d && name && name_cap > 0 && shape && ndim, "null argument");
  std::string n; std::vector<long long> sh;
  disc_param_info(d->m, k, n, sh);
  RVC_REQUIRE((int)n.size() < name_cap && sh.size() <= 8, "name buffer too small");
  std::memcpy(name, n.c_str(), n.size() + 1);
  for (size_t i = 0; i < sh.size(); ++i) shape[i] = sh[i];
  *ndim = (int)sh.size();
  RVC_CATCH
}
int rvc_disc_weight_grad_launch_count(rvc_disc* d, int S, int64_t T) {
  try { RVC_REQUIRE(d, "null argument"); return disc_weight_grad_launch_count(d->m, S, T); }
  catch (const std::exception& e) { rvc::set_error(e.what()); return -1; }
}
int rvc_disc_weight_grad(rvc_disc* d, void* stream, const float* signals, int S, int64_t T, const float* const* fmaps, const float* const* deltas,
                         float* const* grads) {
  RVC_TRY
  RVC_REQUIRE(d && signals && fmaps && deltas && grads, "null argument");
  disc_weight_grad(d->m, (hipStream_t)stream, signals, S, T, fmaps, deltas, grads);
  check_launch();
  RVC_CATCH
}
int rvc_adamw_step(void* stream, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int K, const rvc_adamw_hyper* hyper) {
  RVC_TRY
  RVC_REQUIRE(p && g && m && v && n && hyper && K >= 1 && K <= 64, "1 <= K <= 64 tensors, no null argument");
  long long nn[64]; for (int k = 0; k < K; ++k) nn[k] = n[k];
  adamw_step((hipStream_t)stream, p, g, m, v, nn, K, *hyper);
  check_launch();
  RVC_CATCH
}
int rvc_disc_adamw_step(rvc_disc* d, void* stream, const float* grads, float* exp_avg, float* exp_avg_sq, const rvc_adamw_hyper* hyper) {
  RVC_TRY
  RVC_REQUIRE(d && grads && exp_avg && exp_avg_sq && hyper, "null argument");
  RVC_HIP_CHECK(hipSetDevice(d->ctx->c.device));
  disc_adamw_step(d->m, (hipStream_t)stream, grads, exp_avg, exp_avg_sq, *hyper);
  check_launch();
  RVC_CATCH
}
int rvc_disc_adamw_step_launch_count(rvc_disc* d) {
  try { RVC_REQUIRE(d, "null argument"); RVC_HIP_CHECK(hipSetDevice(d->ctx->c.device)); return disc_adamw_step_launch_count(d->m); }
  catch (const std::exception& e) { rvc::set_error(e.what()); return -1; }
}
int64_t rvc_disc_param_total(rvc_disc* d) {
  try { RVC_REQUIRE(d, "null argument"); RVC_HIP_CHECK(hipSetDevice(d->ctx->c.device)); return disc_param_total(d->m); }
  catch (const std::exception& e) { rvc::set_error(e.what()); return -1; }
}
int rvc_disc_get_parameters(rvc_disc* d, void* stream, float* flat) {
  RVC_TRY
  RVC_REQUIRE(d && flat, "null argument");
  RVC_HIP_CHECK(hipSetDevice(d->ctx->c.device));
  disc_get_parameters(d->m, (hipStream_t)stream, flat);
  RVC_CATCH
}
int rvc_disc_set_parameters(rvc_disc* d, void* stream, const float* flat) {
  RVC_TRY
  RVC_REQUIRE(d && flat, "null argument");
  RVC_HIP_CHECK(hipSetDevice(d->ctx->c.device));
  disc_set_parameters(d->m, (hipStream_t)stream, flat);
  check_launch();
  RVC_CATCH
}
int rvc_loss_cotangents(void* stream, int kind, const float* const* a, const float* const* b, const int64_t* n, const float* scale, int K, float* const* out) {
  RVC_TRY
  RVC_REQUIRE(a && n && scale && out && K >= 1 && K <= 64, "1 <= K <= 64 tensors, no null argument");
  long long nn[64]; for (int k = 0; k < K; ++k) nn[k] = n[k];
  loss_cotangents((hipStream_t)stream, kind, a, b, nn, scale, K, out);
  check_launch();
  RVC_CATCH
}
int rvc_interpolate(void* stream, const float* alpha, const float* y, const float* y_hat, int B, int64_t T, float* out) {
  RVC_TRY
  interpolate_rows((hipStream_t)stream, alpha, y, y_hat, B, T, out);
  check_launch();
  RVC_CATCH
}
int rvc_synth_dec_halo(rvc_synth* s) { return s ? synth_dec_halo_frames(s->m) : 0; }
int rvc_synth_window_frames(rvc_synth* s, int64_t T, int64_t keep0, int64_t keep1, int64_t* g0, int64_t* g1) {
  RVC_TRY
  RVC_REQUIRE(s && g0 && g1 && T > 0 && T < (1LL << 30), "bad argument");
  RVC_HIP_CHECK(hipSetDevice(s->ctx->c.device));                  // (the plans that decide the alignment ask for the device's CU count)
  int a, b;
  synth_window_frames(s->m, (int)T, keep0, keep1, -1, &a, &b);
  *g0 = a; *g1 = b;
  RVC_CATCH
}
int rvc_synth_infer_window_halo(rvc_synth* s, void* stream, const float* phone, int phone_cm, const int64_t* pitch, const float* pitchf, int sid,
                                const float* noise_z, const float* noise_src, int64_t T, float* out, const rvc_synth_taps* taps, int64_t keep0, int64_t keep1,
                                int halo) {
  RVC_TRY
  RVC_REQUIRE(s && phone && noise_z && out, "null argument");
  check_pitch_args(s, pitch, pitchf, noise_src, 0);
  synth_infer_window(s->m, (hipStream_t)stream, phone, phone_cm, (const long long*)pitch, pitchf, sid, noise_z, noise_src, (int)T, out, taps, keep0, keep1, halo);
  check_launch();
  RVC_CATCH
}
int rvc_synth_infer_window(rvc_synth* s, void* stream, const float* phone, int phone_cm, const int64_t* pitch, const float* pitchf, int sid,
                           const float* noise_z, const float* noise_src, int64_t T, float* out, const rvc_synth_taps* taps, int64_t keep0, int64_t keep1) {
  return rvc_synth_infer_window_halo(s, stream, phone, phone_cm, pitch, pitchf, sid, noise_z, noise_src, T, out, taps, keep0, keep1, -1);
}
int rvc_synth_infer(rvc_synth* s, void* stream, const float* phone, int phone_cm, const int64_t* pitch, const float* pitchf, int sid,
                    const float* noise_z, const float* noise_src, int64_t T, float* out, const rvc_synth_taps* taps) {
  return rvc_synth_infer_window(s, stream, phone, phone_cm, pitch, pitchf, sid, noise_z, noise_src, T, out, taps, 0, T);
}

int rvc_vc_segment_window(rvc_hubert* h, rvc_synth* s, void* stream, const float* audio, int64_t L, int version, const int64_t* pitch,
                          const float* pitchf, int sid, float protect, int do_protect, const float* noise_z, const float* noise_src, float* out,
                          int64_t keep0, int64_t keep1) {
  RVC_TRY
  RVC_REQUIRE(h && s && audio && noise_z && out, "null argument");
  check_pitch_args(s, pitch, pitchf, noise_src, do_protect);
  hipStream_t st = (hipStream_t)stream;
  const long long Th = hubert_num_frames(L);
  const int D = version == 1 ? 256 : 768;
  RVC_REQUIRE(version == 1 || version == 2, "version must be 1 (256-d) or 2 (768-d)");
  RVC_REQUIRE(D == synth_feat_dim(s->m), "feature width of `version` does not match the synthesizer (v1 models take 256-d, v2 models 768-d features)");
  RVC_REQUIRE(Th > 0 && 2 * Th < (1LL << 30), "segment length out of range");
  const int T = (int)(2 * Th);
  if (keep1 < 0) keep1 = T;                                      // (the un-windowed entry point: the sequence length is only known here)
  // scratch for the channel-major features lives in two small allocations owned by this call's stream order
  float* fcm = (float*)stream_scratch(st, 1, (size_t)D * Th * sizeof(float));
  float* fup = (float*)stream_scratch(st, 2, (size_t)D * T * sizeof(float));
  hubert_forward(h->m, st, audio, L, version, 0, nullptr, fcm, nullptr);
  feats_prepare(st, fcm, nullptr, pitchf, fup, D, (int)Th, T, protect, do_protect);
  synth_infer_window(s->m, st, fup, 1, (const long long*)pitch, pitchf, sid, noise_z, noise_src, T, out, nullptr, keep0, keep1, -1);
  check_launch();
  RVC_CATCH
}
int rvc_vc_segment(rvc_hubert* h, rvc_synth* s, void* stream, const float* audio, int64_t L, int version, const int64_t* pitch,
                   const float* pitchf, int sid, float protect, int do_protect, const float* noise_z, const float* noise_src, float* out) {
  return rvc_vc_segment_window(h, s, stream, audio, L, version, pitch, pitchf, sid, protect, do_protect, noise_z, noise_src, out, 0, -1);
}

int rvc_vc_segment_feats_window(rvc_synth* s, void* stream, const float* feats_cm, const float* feats0_cm, int64_t Th, int feat_dim, const int64_t* pitch,
                                const float* pitchf, int sid, float protect, int do_protect, const float* noise_z, const float* noise_src, float* out,
                                int64_t keep0, int64_t keep1) {
  RVC_TRY
  RVC_REQUIRE(s && feats_cm && noise_z && out, "null argument");
  check_pitch_args(s, pitch, pitchf, noise_src, do_protect);
  hipStream_t st = (hipStream_t)stream;
  RVC_REQUIRE(feat_dim == synth_feat_dim(s->m), "feat_dim does not match the synthesizer (v1 models take 256-d, v2 models 768-d features)");
  RVC_REQUIRE(Th > 0 && 2 * Th < (1LL << 30), "segment length out of range");
  const int T = (int)(2 * Th);
  float* fup = (float*)stream_scratch(st, 2, (size_t)feat_dim * T * sizeof(float));
  feats_prepare(st, feats_cm, feats0_cm, pitchf, fup, feat_dim, (int)Th, T, protect, do_protect);
  synth_infer_window(s->m, st, fup, 1, (const long long*)pitch, pitchf, sid, noise_z, noise_src, T, out, nullptr, keep0, keep1, -1);
  check_launch();
  RVC_CATCH
}
int rvc_vc_segment_feats(rvc_synth* s, void* stream, const float* feats_cm, const float* feats0_cm, int64_t Th, int feat_dim, const int64_t* pitch,
                         const float* pitchf, int sid, float protect, int do_protect, const float* noise_z, const float* noise_src, float* out) {
  return rvc_vc_segment_feats_window(s, stream, feats_cm, feats0_cm, Th, feat_dim, pitch, pitchf, sid, protect, do_protect, noise_z, noise_src, out, 0, 2 * Th);
}

int rvc_resample(void* stream, const float* x, int64_t n_in, const double* taps, int half, int up, int down, float* y, int64_t n_out) {
  RVC_TRY
  RVC_REQUIRE(x && taps && y && n_in > 0 && half >= 0 && up > 0 && down > 0, "bad argument");
  resample((hipStream_t)stream, x, n_in, taps, half, up, down, y, n_out);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ feature retrieval
struct rvc_index { FeatIndex* m; };
int rvc_index_create(rvc_ctx* ctx, const float* big_npy, int64_t N, int D, rvc_index** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && out, "null argument");
  std::unique_ptr<rvc_index> h(new rvc_index()); h->m = index_create(&ctx->c, big_npy, N, D);
  *out = h.release();
  RVC_CATCH
}
int rvc_index_destroy(rvc_index* h) { if (h) { index_destroy(h->m); delete h; } return 0; }
int64_t rvc_index_ntotal(const rvc_index* h) { return h ? index_size(h->m) : 0; }
int rvc_index_create_ivf(rvc_ctx* ctx, const float* big_npy, int64_t N, int D, const float* centroids, int nlist, const int32_t* list_of, int nprobe,
                         rvc_index** out) {
  RVC_TRY
  RVC_REQUIRE(ctx && out, "null argument");
  std::unique_ptr<rvc_index> h(new rvc_index()); h->m = index_create_ivf(&ctx->c, big_npy, N, D, centroids, nlist, (const int*)list_of, nprobe);
  *out = h.release();
  RVC_CATCH
}
int rvc_index_nprobe(const rvc_index* h) { return h && h->m ? index_nprobe(h->m) : 0; }
int rvc_index_search(rvc_index* h, void* stream, const float* feats_cm, int64_t T, int64_t* idx, float* score) {
  RVC_TRY
  RVC_REQUIRE(h && feats_cm && idx && T > 0, "bad argument");
  index_search(h->m, (hipStream_t)stream, feats_cm, (int)T, (long long*)idx, score);
  check_launch();
  RVC_CATCH
}
int rvc_index_blend(rvc_index* h, void* stream, const float* feats_cm, const int64_t* idx, int64_t T, float index_rate, float* out_cm) {
  RVC_TRY
  RVC_REQUIRE(h && feats_cm && idx && out_cm && T > 0, "bad argument");
  index_blend(h->m, (hipStream_t)stream, feats_cm, (const long long*)idx, (int)T, index_rate, out_cm);
  check_launch();
  RVC_CATCH
}
// building the index: k-means on the device (index_build.hip)
int rvc_kmeans_assign(rvc_ctx* ctx, void* stream, const float* rows, int64_t N, int D, const float* cent, int K, int32_t* label, float* dist) {
  RVC_TRY
  RVC_REQUIRE(ctx && rows && cent && label, "null argument");
  kmeans_assign(&ctx->c, (hipStream_t)stream, rows, N, D, cent, K, (int*)label, dist);
  check_launch();
  RVC_CATCH
}
int rvc_kmeans_update(void* stream, const float* rows, const int32_t* label, int64_t N, int D, int K, float* cent, int32_t* count) {
  RVC_TRY
  RVC_REQUIRE(rows && label && cent && count, "null argument");
  kmeans_update((hipStream_t)stream, rows, (const int*)label, N, D, K, cent, (int*)count);
  check_launch();
  RVC_CATCH
}
int rvc_index_train(rvc_ctx* ctx, void* stream, const float* rows, int64_t N, int D, const int64_t* init_rows, int K, int niter, float* cent,
                    int32_t* label, double* inertia) {
  RVC_TRY
  RVC_REQUIRE(ctx && rows && init_rows && cent && label, "null argument");
  index_train(&ctx->c, (hipStream_t)stream, rows, N, D, (const long long*)init_rows, K, niter, cent, (int*)label, inertia);
  check_launch();
  RVC_CATCH
}

int rvc_preprocess(void* stream, const void* audio, int is_f64, int64_t n, const double* b6, const double* a6, const double* zi5, int t_pad,
                   double* filt, float* padded, double* rms1, int n1, const double* sos18, const double* sos_zi6) {
  RVC_TRY
  RVC_REQUIRE(audio && b6 && a6 && zi5 && filt && n > 3 * 6 + 1 && t_pad >= 0, "bad argument");
  RVC_REQUIRE(a6[0] != 0.0, "a[0] must be non-zero");
  RVC_REQUIRE(rms1 == nullptr || n1 == (int)(n / 8000) + 1, "rms1 must hold n / 8000 + 1 frames");
  hipStream_t st = (hipStream_t)stream;
  RVC_REQUIRE((sos18 == nullptr) == (sos_zi6 == nullptr), "sos and its initial state come together");
  double* scratch = (double*)stream_scratch(st, 2, preprocess_scratch_doubles(n, sos18 != nullptr) * sizeof(double));      // ext | yr, each rounded up to whole blocks
  preprocess(st, audio, is_f64, n, b6, a6, zi5, t_pad, filt, padded, rms1, n1, 16000, 8000, scratch, sos18, sos_zi6);
  check_launch();
  RVC_CATCH
}
int rvc_postprocess(void* stream, float* wav, int64_t N, const double* rms1, int n1, int sr2, float rms_mix_rate, int16_t* out_i16) {
  RVC_TRY
  RVC_REQUIRE(wav && out_i16 && N > 0 && sr2 > 0, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int n2 = (int)(N / (sr2 / 2)) + 1;
  float* scratch = (float*)stream_scratch(st, 1, (size_t)(n2 + 4) * sizeof(float));
  postprocess(st, wav, N, rms1, n1, sr2, rms_mix_rate, (short*)out_i16, scratch + 4, (unsigned*)scratch);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ training-set preparation (dataset_prep.hip)
int rvc_lfilter_hp(void* stream, const void* x, int is_f64, int64_t n, const double* sos18, double* y) {
  RVC_TRY
  RVC_REQUIRE(x && sos18 && y && n > 0, "bad argument");
  lfilter_sos((hipStream_t)stream, x, is_f64, n, sos18, y);
  check_launch();
  RVC_CATCH
}
int rvc_frame_rms(void* stream, const double* x, int64_t n, int win, int hop, double* rms, int64_t n_frames) {
  RVC_TRY
  RVC_REQUIRE(x && rms && n > 0 && win > 0 && hop > 0, "bad argument");
  RVC_REQUIRE(n_frames == (n + 2 * (int64_t)(win / 2) - win) / hop + 1 && n_frames < (1LL << 31), "rms must hold (n + 2 (win / 2) - win) / hop + 1 frames");
  rms_frames_f64((hipStream_t)stream, x, n, win, hop, rms, n_frames);
  check_launch();
  RVC_CATCH
}
int rvc_slice_tags(const double* rms, int64_t n_frames, int64_t n_samples, double threshold, int64_t min_length, int64_t min_interval,
                   int64_t max_sil_kept, int64_t* tags, int64_t cap, int64_t* n_tags) {
  RVC_TRY
  RVC_REQUIRE((rms || n_frames == 0) && tags && n_tags && n_frames >= 0 && cap >= 0, "bad argument");
  RVC_REQUIRE(min_interval >= 1 && max_sil_kept >= 1 && min_length >= min_interval, "min_length >= min_interval >= 1 and max_sil_kept >= 1 frames");
  *n_tags = slice_tags(rms, n_frames, n_samples, threshold, min_length, min_interval, max_sil_kept, (long long*)tags, cap);
  RVC_CATCH
}
int rvc_cut_windows(void* stream, const double* filt, int64_t n, const int64_t* windows, int n_windows, int sr, int target_sr, const double* taps,
                    int half, int up, int down, float max_volume, float* gt, int64_t total_gt, float* y16, int64_t total_16) {
  RVC_TRY
  RVC_REQUIRE(filt && windows && taps && n > 0 && n_windows >= 0 && half >= 0 && up > 0 && down > 0, "bad argument");
  RVC_REQUIRE(sr > 0 && target_sr > 0 && (int64_t)sr * up == (int64_t)target_sr * down, "up / down must be target_sr / sr");
  RVC_REQUIRE(max_volume > 0.f && total_gt >= 0 && total_16 >= 0 && (gt || total_gt == 0) && (y16 || total_16 == 0), "bad argument");
  cut_windows((hipStream_t)stream, filt, n, (const long long*)windows, n_windows, sr, target_sr, taps, half, up, down, max_volume, gt, total_gt,
              y16, total_16);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ audio nodes (audio_fx.hip)
int rvc_gate_levels(void* stream, const float* x, int64_t n, int win, double* ss, int64_t n_windows) {
  RVC_TRY
  RVC_REQUIRE(x && ss && n > 0 && win > 0, "bad argument");
  RVC_REQUIRE(n_windows == (n + win - 1) / win && n_windows < (1LL << 31), "ss must hold ceil(n / win) windows");
  gate_levels((hipStream_t)stream, x, n, win, ss, n_windows);
  check_launch();
  RVC_CATCH
}
int rvc_gate_ranges(const double* level, int64_t n_windows, int64_t n, int64_t win, int64_t min_size, int64_t fade, double threshold_db,
                    int64_t* ranges, int64_t cap, int64_t* n_ranges) {
  RVC_TRY
  RVC_REQUIRE(level && ranges && n_ranges && n > 0 && win > 0 && cap >= 0, "bad argument");
  RVC_REQUIRE(n_windows == (n + win - 1) / win, "level must hold ceil(n / win) windows");
  RVC_REQUIRE(fade >= 2 && min_size >= 2 * fade, "fade >= 2 samples and min_size >= 2 fade");
  *n_ranges = gate_ranges(level, n_windows, n, win, min_size, fade, threshold_db, (long long*)ranges, cap);
  RVC_CATCH
}
int rvc_gate_apply(void* stream, const float* x, float* y, int64_t n, const int64_t* ranges, int n_ranges, int64_t fade) {
  RVC_TRY
  RVC_REQUIRE(x && y && n > 0 && n_ranges >= 0 && (ranges || n_ranges == 0) && fade >= 2, "bad argument");
  gate_apply((hipStream_t)stream, x, y, n, (const long long*)ranges, n_ranges, fade);
  check_launch();
  RVC_CATCH
}
int rvc_declick(void* stream, const float* x, int64_t n, int size, float multiplier, int method, int kernel_size, int detect, float* y, uint8_t* mask) {
  RVC_TRY
  if (!detect) size = 1;
  RVC_REQUIRE(x && y && mask && n > 0 && size > 0 && (method == 0 || method == 1) && multiplier >= 0.f, "bad argument");
  RVC_REQUIRE(kernel_size >= 1 && (kernel_size & 1) && kernel_size <= kMaxClickKernel, "kernel_size must be odd and at most 31");
  RVC_REQUIRE(n >= size && n >= kernel_size, "the signal must be at least as long as the RMS window and the median window");
  RVC_REQUIRE(x != y, "declick reads the unmodified input: y must not be x");
  declick((hipStream_t)stream, x, n, size, multiplier, method, kernel_size, detect != 0, y, mask);
  check_launch();
  RVC_CATCH
}
int rvc_peak_normalize(void* stream, const float* x, int64_t n, float gain, float* y) {
  RVC_TRY
  RVC_REQUIRE(x && y && n > 0 && gain > 0.f, "bad argument");
  peak_normalize((hipStream_t)stream, x, n, gain, y);
  check_launch();
  RVC_CATCH
}
int rvc_peak_limit(void* stream, float* x, int64_t n, float max_volume) {
  RVC_TRY
  RVC_REQUIRE(x && n > 0 && max_volume > 0.f, "bad argument");
  peak_limit((hipStream_t)stream, x, n, max_volume);
  check_launch();
  RVC_CATCH
}
int rvc_merge_tracks(void* stream, const float* const* tracks, const int64_t* lens, int k, int mode, float* out, int64_t n_out) {
  RVC_TRY
  RVC_REQUIRE(tracks && lens && out && k >= 2 && k <= 4 && mode >= 0 && mode <= 3 && n_out > 0, "bad argument");
  long long l[4];
  for (int j = 0; j < k; ++j) {
    RVC_REQUIRE(lens[j] >= 0 && lens[j] <= n_out && (tracks[j] || lens[j] == 0), "every track must fit the output");
    l[j] = lens[j];
  }
  merge_tracks((hipStream_t)stream, tracks, l, k, mode, out, n_out);
  check_launch();
  RVC_CATCH
}
int rvc_segment_energy(void* stream, const int16_t* x, int64_t n, int k, int64_t* out) {
  RVC_TRY
  RVC_REQUIRE(x && out && k >= 1 && n >= k, "bad argument");
  segment_energy((hipStream_t)stream, x, n, k, (long long*)out);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ training inputs (spectrogram.hip)
int rvc_spectrogram_batch(rvc_ctx* ctx, void* stream, const float* audio, int64_t n_audio, const int64_t* clips, int n_clips, int n_fft, int hop, float eps,
                          int clamp, float* out, int64_t pitch) {
  RVC_TRY
  RVC_REQUIRE(ctx && audio && out && (clips || n_clips == 0), "null argument");
  spectrogram_batch(&ctx->c, (hipStream_t)stream, audio, n_audio, (const long long*)clips, n_clips, n_fft, hop, eps, clamp, out, pitch);
  check_launch();
  RVC_CATCH
}
int rvc_mel_filterbank_set(rvc_ctx* ctx, int n_fft, int n_mels, const int32_t* first, const int32_t* count, const float* weights) {
  RVC_TRY
  RVC_REQUIRE(ctx, "null argument");
  RVC_HIP_CHECK(hipSetDevice(ctx->c.device));
  mel_filterbank_set(&ctx->c, n_fft, n_mels, (const int*)first, (const int*)count, weights);
  RVC_CATCH
}
int rvc_spec_to_mel_batch(rvc_ctx* ctx, void* stream, const float* spec, int64_t spec_pitch, const int64_t* clips, int n_clips, int n_fft, int n_mels,
                          float* mel, int64_t mel_pitch) {
  RVC_TRY
  RVC_REQUIRE(ctx && spec && mel && (clips || n_clips == 0), "null argument");
  spec_to_mel_batch(&ctx->c, (hipStream_t)stream, spec, spec_pitch, (const long long*)clips, n_clips, n_fft, n_mels, mel, mel_pitch);
  check_launch();
  RVC_CATCH
}
int rvc_spectrogram_batch_ms(rvc_ctx* ctx, void* stream, const float* audio, int64_t n_audio, const int64_t* clips, int n_clips, int n_fft, int hop, float eps,
                             int clamp, float* out, int64_t pitch) {
  RVC_TRY
  RVC_REQUIRE(ctx && audio && out && (clips || n_clips == 0), "null argument");
  spectrogram_batch_ms(&ctx->c, (hipStream_t)stream, audio, n_audio, (const long long*)clips, n_clips, n_fft, hop, eps, clamp, out, pitch);
  check_launch();
  RVC_CATCH
}
int rvc_mel_spectrogram_vjp(rvc_ctx* ctx, void* stream, const float* audio, int64_t n_audio, const int64_t* clips, int n_clips, int n_fft, int hop, float eps,
                            int clamp, int n_mels, const float* cot_mel, int64_t pitch, float* d_audio) {
  RVC_TRY
  RVC_REQUIRE(ctx && audio && cot_mel && d_audio && (clips || n_clips == 0), "null argument");
  mel_spectrogram_vjp(&ctx->c, (hipStream_t)stream, audio, n_audio, (const long long*)clips, n_clips, n_fft, hop, eps, clamp, n_mels, cot_mel, pitch, d_audio);
  check_launch();
  RVC_CATCH
}
int rvc_mel_spectrogram_vjp_launch_count(void) { return kMelVjpLaunches; }
int rvc_mel_loss_cotangents(void* stream, int K, const float* const* a, const float* const* b, const int64_t* n, int loss, float log_weight, float mag_weight,
                            const float* scale, float* const* out) {
  RVC_TRY
  mel_loss_cotangents((hipStream_t)stream, K, a, b, (const long long*)n, loss, log_weight, mag_weight, scale, out);
  check_launch();
  RVC_CATCH
}
int rvc_multiscale_mel_loss(rvc_ctx* ctx, void* stream, int K, const float* const* spec, const int64_t* pitch, const int64_t* row_stride, int B, int64_t nf,
                            const int32_t* n_fft, const int32_t* n_mels, int loss, int want_mag, double* out) {
  RVC_TRY
  RVC_REQUIRE(ctx && spec && pitch && row_stride && n_fft && n_mels && out, "null argument");
  multiscale_mel_loss(&ctx->c, (hipStream_t)stream, K, spec, (const long long*)pitch, (const long long*)row_stride, B, nf, (const int*)n_fft, (const int*)n_mels,
                      loss, want_mag, out);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ auxiliary losses (aux_losses.hip)
int rvc_hpss(void* stream, const float* x, int B, int F, int T, float* h, float* p, int medians) {
  RVC_TRY
  hpss_parts((hipStream_t)stream, x, B, F, T, h, p, medians);
  check_launch();
  RVC_CATCH
}
int rvc_hpss_l1(void* stream, const float* org, const float* gen, int B, int F, int T, float eps, double* sums) {
  RVC_TRY
  hpss_l1((hipStream_t)stream, org, gen, B, F, T, eps, sums);
  check_launch();
  RVC_CATCH
}
int rvc_tsi_terms(void* stream, const float* org, const float* gen, int B, int F, int T, float eps, double* out) {
  RVC_TRY
  tsi_terms((hipStream_t)stream, org, gen, B, F, T, eps, out);
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ single ops
int rvc_op_conv1d(void* stream, const float* x, const float* w, const float* bias, const float* res, float* y, int Ci, int Co, int Tin, int k,
                  int stride, int pad, int dil, int groups, int pre_act, float pre_slope, int act, float act_slope, int act_before_res,
                  float out_scale, int accumulate) {
  RVC_TRY
  OwnedConvLayer L;
  conv1d_layer_init(L, w, bias, Co, Ci, k, stride, pad, dil, groups);
  ConvEpilogue e; e.pre_act = pre_act; e.pre_slope = pre_slope; e.act = act; e.act_slope = act_slope; e.act_before_res = act_before_res;
  e.out_scale = out_scale; e.accumulate = accumulate;
  const int Tout = conv1d_out_len(L, Tin);
  e.R = res; e.ldR = Tout;
  conv1d_run(L, (hipStream_t)stream, x, Tin, Tin, y, Tout, e);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  RVC_CATCH
}
int rvc_op_gemm_split(void* stream, const float* x, const float* w, const float* bias, const float* res, float* y, float* ysplit_f32, int Ci, int Co,
                      int T, int act, float act_slope, int act_before_res, float out_scale, int ksplit, int am, int an, int k, int dil) {
  RVC_TRY
  RVC_REQUIRE(x && w && (y || ysplit_f32) && Ci > 0 && Co > 0 && T > 0 && k >= 1 && (k & 1) == 1 && dil >= 1, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, w, bias, Co, Ci, k, 1, (k - 1) / 2 * dil, dil, 1); }
  RVC_REQUIRE(conv_x3s_eligible(L), "layer not eligible for the split-resident GEMM (Ci % 16 == 0, Ci k >= 64, Co >= 32, pad <= 64)");
  const long long tp = split_image_tp(T);
  DevBytes xs = image_from_f32(s, x, Ci, T, 0), ys;
  ConvEpilogue e; e.act = act; e.act_slope = act_slope; e.act_before_res = act_before_res; e.out_scale = out_scale; e.R = res; e.ldR = T;
  if (ysplit_f32) { ys.alloc(split_image_bytes(Co, T)); e.ys_out = ys.p; e.ys_tp = tp; }
  { X3sForceScope force(ksplit, am, an); conv_x3s_run(L, s, xs.p, tp, T, y, T, e); }
  if (ysplit_f32) split_image_to_f32(s, ys.p, tp, Co, T, ysplit_f32, T);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_gemm_split_swapped(void* stream, const float* x, const float* w, float* yt, int Ci, int Co, int T, int row0, int rows) {
  RVC_TRY
  RVC_REQUIRE(x && w && yt && Ci > 0 && Co > 0 && T > 0 && rows > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, w, nullptr, Co, Ci, 1, 1, 0, 1, 1); }
  const long long tp = split_image_tp(T), vtp = attention_vt_tp(rows);
  const size_t vbytes = attention_vt_bytes(rows, T);
  DevBytes xs = image_from_f32(s, x, Ci, T, 0xff), ys;                          // NaN patterns past T: the tail rows must come out as zeros regardless
  ys.alloc(vbytes);
  RVC_HIP_CHECK(hipMemsetAsync(ys.p, 0xff, vbytes, s));
  conv_x3s_run_swapped(L, row0, rows, s, xs.p, tp, T, ys.p, vtp);
  attention_vt_clear_tail(s, ys.p, rows, T);
  split_image_to_f32(s, ys.p, vtp, (T + 63) / 64 * 64, rows, yt, rows);          // yt [ceil64(T)][rows]
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_wn_in_gate_split(void* stream, const float* x, const float* w, const float* bias, const float* g_dev, float* y, int Ci, int H, int T, int k) {
  RVC_TRY
  RVC_REQUIRE(x && w && y && Ci > 0 && H > 0 && (H & 15) == 0 && T > 0 && k >= 1 && (k & 1) == 1, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  // the 2 H rows in the order the gate epilogue wants (wn_gate_row_order)
  std::vector<float> wp((size_t)2 * H * Ci * k), bp((size_t)2 * H, 0.f);
  for (int r = 0; r < 2 * H; ++r) {
    const int src = wn_gate_row_order(r, H);
    std::copy(w + (size_t)src * Ci * k, w + (size_t)(src + 1) * Ci * k, wp.begin() + (size_t)r * Ci * k);
    if (bias) bp[r] = bias[src];
  }
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, wp.data(), bp.data(), 2 * H, Ci, k, 1, (k - 1) / 2, 1, 1); }
  RVC_REQUIRE(conv_x3s_eligible(L), "layer not eligible for the split-resident kernel");
  const long long tp = split_image_tp(T);
  DevBytes xs = image_from_f32(s, x, Ci, T, 0), ys;
  ys.alloc(split_image_bytes(H, T));
  ConvEpilogue e; e.ys_out = ys.p; e.ys_tp = tp; e.gate_h = H; e.gate_g = g_dev;
  conv_x3s_run(L, s, xs.p, tp, T, nullptr, T, e);
  split_image_to_f32(s, ys.p, tp, H, T, y, T);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_gemm_split_qkv(void* stream, const float* x, const float* w, const float* bias, float* y_img_f32, float* yt, int Ci, int Co, int T, int vt_row0) {
  RVC_TRY
  RVC_REQUIRE(x && w && y_img_f32 && yt && Ci > 0 && Co > 0 && T > 0 && vt_row0 > 0 && vt_row0 < Co, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, w, bias, Co, Ci, 1, 1, 0, 1, 1); }
  const int rows = Co - vt_row0;
  RVC_REQUIRE(conv_x3s_eligible(L), "layer not eligible for the split-resident kernel");
  const long long tp = split_image_tp(T), vtp = attention_vt_tp(rows);
  const size_t vbytes = attention_vt_bytes(rows, T);
  DevBytes xs = image_from_f32(s, x, Ci, T, 0xff), ys, vt;                      // NaN patterns past T: the transposed rows past T must come out as zeros regardless
  ys.alloc(split_image_bytes(vt_row0, T));
  vt.alloc(vbytes);
  RVC_HIP_CHECK(hipMemsetAsync(vt.p, 0xff, vbytes, s));
  ConvEpilogue e; e.ys_out = ys.p; e.ys_tp = tp; e.vt_out = vt.p; e.vt_tp = vtp; e.vt_row0 = vt_row0;
  conv_x3s_run(L, s, xs.p, tp, T, nullptr, T, e);
  attention_vt_clear_tail(s, vt.p, rows, T);
  split_image_to_f32(s, ys.p, tp, vt_row0, T, y_img_f32, T);                    // y_img_f32 [vt_row0][T]: the rows below vt_row0, from their image
  split_image_to_f32(s, vt.p, vtp, (T + 63) / 64 * 64, rows, yt, rows);          // yt [ceil64(T)][rows]: the rows from vt_row0 on, transposed
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv2d3x3_plus_1x1(void* stream, const float* x1, const float* w1, const float* x2, const float* w2, float* y, float* y_img_f32, int Ci1, int Ci2, int Co, int H, int W,
                              int ksplit) {
  RVC_TRY
  RVC_REQUIRE(x1 && w1 && x2 && w2 && y && Ci1 > 0 && Ci2 > 0 && Co > 0 && H > 0 && W > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L1, L2;
  { ConvBuildScope scope(2); conv2d3x3_layer_init(L1, w1, nullptr, Co, Ci1); conv1d_layer_init(L2, w2, nullptr, Co, Ci2, 1, 1, 0, 1, 1); }
  RVC_REQUIRE(conv_x3s_eligible(L1) && conv_x3s_eligible(L2), "layers not eligible for the split-resident GEMM (channels % 16, Co >= 32)");
  conv_layer_append_x3(L1, L2);
  SplitGeom g = split_geom_2d(W);
  const long long TP = (long long)H * (W + 2), tp = ((long long)g.margin + TP + std::max(704, g.margin) + 63) & ~63LL;
  const size_t b1 = (size_t)(Ci1 / 16) * 4 * (size_t)tp * 16, b2 = (size_t)(Ci2 / 16) * 4 * (size_t)tp * 16, bo = (size_t)((Co + 15) / 16) * 4 * (size_t)tp * 16;
  DevBytes img, yimg; DevBuf<float> yp;
  img.alloc(b1 + b2); RVC_HIP_CHECK(hipMemsetAsync(img.p, 0, b1 + b2, s));      // zero margins: the vertical zero padding
  yp.alloc((size_t)Co * TP);
  if (y_img_f32) { yimg.alloc(bo); RVC_HIP_CHECK(hipMemsetAsync(yimg.p, 0xff, bo, s)); }
  pad2d_split(s, x1, (long long)H * W, Ci1, H, W, nullptr, 0, img.p, tp, g.margin);
  pad2d_split(s, x2, (long long)H * W, Ci2, H, W, nullptr, 0, img.p + b1, tp, g.margin);
  g.seg2_off = (long long)b1;
  ConvEpilogue e;
  if (yimg.p) { e.ys_out = yimg.p; e.ys_tp = tp; }
  { X3sForceScope force(ksplit, 0, 0); conv_x3s_run(L1, s, img.p, tp, (int)TP, yp.p, TP, e, &g); }
  unpad2d(s, yp.p, TP, Co, H, W, y, (long long)H * W);
  if (yimg.p) {                                               // the raw image of the output, read back through the padded layout
    split_image_to_f32(s, yimg.p + (size_t)(g.margin - kSplitMargin) * 16, tp, Co, (int)TP, yp.p, TP);
    unpad2d(s, yp.p, TP, Co, H, W, y_img_f32, (long long)H * W);
  }
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_gemm_split_swapped_res(void* stream, const float* x, const float* w, const float* res, float* y, int Ci, int Co, int T, int ld, int off) {
  RVC_TRY
  RVC_REQUIRE(x && w && res && y && Ci > 0 && Co > 0 && T > 0 && ld >= Co + off && off >= 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, w, nullptr, Co, Ci, 1, 1, 0, 1, 1); }
  DevBytes xs = image_from_f32(s, x, Ci, T, 0);
  conv_x3s_run_swapped(L, 0, Co, s, xs.p, split_image_tp(T), T, nullptr, 0, y + off, ld, res + off, ld);      // y[t][off + j] = sum_c x[c][t] w[j][c] + res[t][off + j]
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_attention_split(void* stream, const float* q, const float* k, const float* v, const float* bv, float* out, float* out_img_f32, int heads, int T) {
  RVC_TRY
  RVC_REQUIRE(q && k && v && (out || out_img_f32) && heads > 0 && T > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int C = heads * 64;
  DevBytes qk, vt, oi; DevBuf<float> vtf;
  const long long tp = split_image_tp(T);
  attention_operand_images(s, q, k, v, C, T, qk, vtf, vt);
  if (out_img_f32) oi.alloc(split_image_bytes(C, T));
  attention_split(s, qk.p, tp, 2 * C, 0, C / 16, vt.p, heads, 64, T, 1.f, bv, out, T, oi.p, tp);
  if (out_img_f32) split_image_to_f32(s, oi.p, tp, C, T, out_img_f32, T);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_attention_split_rel(void* stream, const float* q, const float* k, const float* v, const float* bv, const float* ek_host, const float* ev_host,
                               float* out, float* out_img_f32, int heads, int T, int kz) {
  RVC_TRY
  RVC_REQUIRE(q && k && v && ek_host && ev_host && (out || out_img_f32) && heads > 0 && T > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int C = heads * 96;
  DevBytes qk, vt, oi, tab; DevBuf<float> vtf;
  std::vector<uint16_t> eki, evi;
  attention_rel_images(ek_host, ev_host, 96, 10, eki, evi);
  const size_t evt_off = eki.size() * 2;                                         // E_k image, then E_v^T image
  tab.alloc(evt_off + evi.size() * 2);
  RVC_HIP_CHECK(hipMemcpy(tab.p, eki.data(), evt_off, hipMemcpyHostToDevice));
  RVC_HIP_CHECK(hipMemcpy(tab.p + evt_off, evi.data(), evi.size() * 2, hipMemcpyHostToDevice));
  const long long tp = split_image_tp(T);
  attention_operand_images(s, q, k, v, C, T, qk, vtf, vt);
  if (out_img_f32) oi.alloc(split_image_bytes(C, T));
  { AttentionKzScope force(kz); attention_split(s, qk.p, tp, 2 * C, 0, C / 16, vt.p, heads, 96, T, 1.f, bv, out, T, oi.p, tp, 10, tab.p, tab.p + evt_off); }
  if (out_img_f32) split_image_to_f32(s, oi.p, tp, C, T, out_img_f32, T);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_cbr2_small(void* stream, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, int C, int H, int W) {
  RVC_TRY
  RVC_REQUIRE(x && w1 && b1 && w2 && b2 && y && (C == 16 || C == 32) && H > 0 && W > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer c1, c2;
  { ConvBuildScope scope(2); conv2d3x3_layer_init(c1, w1, b1, C, C); conv2d3x3_layer_init(c2, w2, b2, C, C); }
  cbr2_small_run(c1, c2, s, x, H, W, y);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv3_small(void* stream, const float* x, const float* w, const float* b, const float* res, float* y, float* y2, int Ci, int Co, int H, int W, int split_row,
                       int relu_rows) {
  RVC_TRY
  RVC_REQUIRE(x && w && b && y && Ci > 0 && Co > 0 && H > 0 && W > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv2d3x3_layer_init(L, w, b, Co, Ci); }
  conv3_small_run(L, s, x, H, W, y, y2, split_row, relu_rows, res);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv1d_split(void* stream, const float* x, const float* w, const float* bias, const float* res, float* y, int Ci, int Co, int T, int k, int pad,
                        int dil, int groups, int act, int act_before_res) {
  RVC_TRY
  RVC_REQUIRE(x && w && y && Ci > 0 && Co > 0 && T > 0 && k >= 1 && groups >= 1, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, w, bias, Co, Ci, k, 1, pad, dil, groups); }
  RVC_REQUIRE(conv_x3s_eligible(L), "layer not eligible for the split-resident kernel");
  DevBytes xs = image_from_f32(s, x, Ci, T, 0);
  ConvEpilogue e; e.act = act; e.act_slope = 0.1f; e.act_before_res = act_before_res; e.R = res; e.ldR = T;
  conv_x3s_run(L, s, xs.p, split_image_tp(T), T, y, T, e);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv1d_s2_split(void* stream, const float* x, const float* w, const float* bias, float* y, float* y_img_f32, int Ci, int Co, int T, int k, int act) {
  RVC_TRY
  RVC_REQUIRE(x && w && y && Ci > 0 && Co > 0 && k >= 2 && T >= k, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv1d_layer_init(L, w, bias, Co, Ci, k, 2, 0, 1, 1); }
  RVC_REQUIRE(conv_x3s_s2_eligible(L), "layer not eligible for the stride-2 path of the split-resident kernel (Ci, Co multiples of 16)");
  const int Tout = (T - k) / 2 + 1;
  const SplitGeom g = split_geom_s2(k, T);
  DevBytes xs, ys;
  xs.alloc(split_s2_bytes(Ci, T));
  RVC_HIP_CHECK(hipMemsetAsync(xs.p, 0xff, split_s2_bytes(Ci, T), s));      // (NaN patterns wherever the producer does not write: what a consumer reads there must not reach a stored column)
  split_image_deint_from_f32(s, x, T, Ci, T, xs.p, split_s2_tp(T), g.s2_h);
  ConvEpilogue e; e.act = act; e.act_slope = 0.1f;
  if (y_img_f32) {
    ys.alloc(split_s2_bytes(Co, Tout));
    e.ys_out = ys.p; e.ys_tp = split_s2_tp(Tout); e.ys_deint_h = split_s2_h(Tout);
  }
  conv_x3s_run(L, s, xs.p, split_s2_tp(T), Tout, y, Tout, e, &g);
  if (y_img_f32) split_image_deint_to_f32(s, ys.p, split_s2_tp(Tout), split_s2_h(Tout), Co, Tout, y_img_f32, Tout);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv2d_split(void* stream, const float* x, const float* w, const float* bias, const float* res, float* y, float* ysplit_f32, int Ci, int Co,
                        int H, int W, int act, int act_before_res, int ksplit, int am, int an) {
  RVC_TRY
  RVC_REQUIRE(x && w && y && Ci > 0 && Co > 0 && H > 0 && W >= 2 && (W & 1) == 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  OwnedConvLayer L;
  { ConvBuildScope scope(2); conv2d3x3_layer_init(L, w, bias, Co, Ci); }
  RVC_REQUIRE(conv_x3s_eligible(L), "layer not eligible for the split-resident kernel (Ci % 16 == 0)");
  const SplitGeom g = split_geom_2d(W);
  const int T = H * (W + 2);
  const long long tp = g.margin + T + 704 + 64;
  const size_t ib = (size_t)(Ci / 16) * 4 * tp * 16, ob = (size_t)((Co + 15) / 16) * 4 * tp * 16;
  DevBytes xs, ys; DevBuf<float> rp, yp, t;
  xs.alloc(ib); RVC_HIP_CHECK(hipMemsetAsync(xs.p, 0, ib, s));
  yp.alloc((size_t)Co * T);
  pad2d_split(s, x, (long long)H * W, Ci, H, W, nullptr, 0, xs.p, tp, g.margin);
  ConvEpilogue e; e.act = act; e.act_slope = 0.1f; e.act_before_res = act_before_res;
  if (res) { rp.alloc((size_t)Co * T); pad2d_split(s, res, (long long)H * W, Co, H, W, rp.p, T, nullptr, 0, 0); e.R = rp.p; e.ldR = T; }
  if (ysplit_f32) { ys.alloc(ob); RVC_HIP_CHECK(hipMemsetAsync(ys.p, 0, ob, s)); e.ys_out = ys.p; e.ys_tp = tp; }
  { X3sForceScope force(ksplit, am, an); conv_x3s_run(L, s, xs.p, tp, T, yp.p, T, e, &g); }
  unpad2d(s, yp.p, T, Co, H, W, y, (long long)H * W);
  if (ysplit_f32) {
    RVC_REQUIRE((Co & 15) == 0, "split output needs Co % 16 == 0");
    t.alloc((size_t)Co * T);
    // (the image's rows start at its own margin: hand the reader the plane origin shifted so that its fixed 64-row margin lands on position 0)
    split_image_to_f32(s, ys.p + (size_t)(g.margin - kSplitMargin) * 16, tp, Co, T, t.p, T);
    unpad2d(s, t.p, T, Co, H, W, ysplit_f32, (long long)H * W);
  }
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv_transpose1d(void* stream, const float* x, const float* w, const float* bias, float* y, int Ci, int Co, int Tin, int k, int u,
                            int pad, int pre_act, float pre_slope, int accumulate) {
  RVC_TRY
  OwnedConvLayer L;
  tconv1d_layer_init(L, w, bias, Ci, Co, k, u, pad);
  ConvEpilogue e; e.pre_act = pre_act; e.pre_slope = pre_slope; e.accumulate = accumulate;
  const int Tout = conv1d_out_len(L, Tin);
  conv1d_run(L, (hipStream_t)stream, x, Tin, Tin, y, Tout, e);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  RVC_CATCH
}
int rvc_op_conv2d3x3(void* stream, const float* x, const float* w, const float* bias, const float* res, float* y, int Ci, int Co, int H, int W,
                     int relu) {
  RVC_TRY
  OwnedConvLayer L;
  conv2d3x3_layer_init(L, w, bias, Co, Ci);
  ConvEpilogue e; e.act = relu ? ACT_RELU : ACT_NONE; e.act_before_res = 1; e.R = res; e.ldR = (long long)H * W;
  conv2d_run(L, (hipStream_t)stream, x, (long long)H * W, H, W, y, (long long)H * W, e);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  RVC_CATCH
}
int rvc_op_conv_transpose2d(void* stream, const float* x, const float* w, const float* bias, float* y, int Ci, int Co, int H, int W, int relu) {
  RVC_TRY
  OwnedConvLayer L;
  tconv2d_layer_init(L, w, bias, Ci, Co);
  ConvEpilogue e; e.act = relu ? ACT_RELU : ACT_NONE;
  conv2d_run(L, (hipStream_t)stream, x, (long long)H * W, H, W, y, 4LL * H * W, e);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  RVC_CATCH
}
int rvc_op_gemm_tn(void* stream, const float* a, const float* b, float* y, int M, int N, int K, int batch) {
  RVC_TRY
  ConvEpilogue e;
  gemm_tn_run((hipStream_t)stream, a, M, (long long)K * M, b, N, (long long)K * N, y, N, (long long)M * N, M, N, K, batch, nullptr, 0, e);
  check_launch();
  RVC_CATCH
}
int rvc_conv1d_plan_create(const float* w, const float* bias, int Ci, int Co, int k, int stride, int pad, int dil, int groups,
                           rvc_conv1d_plan** out) {
  RVC_TRY
  std::unique_ptr<rvc_conv1d_plan> p(new rvc_conv1d_plan());
  conv1d_layer_init(p->L, w, bias, Co, Ci, k, stride, pad, dil, groups);
  *out = p.release();
  RVC_CATCH
}
int rvc_conv1d_plan_run(rvc_conv1d_plan* p, void* stream, const float* x, int Tin, const float* res, float* y, int pre_act, float pre_slope,
                        int act, float act_slope) {
  RVC_TRY
  RVC_REQUIRE(p, "null argument");
  ConvEpilogue e; e.pre_act = pre_act; e.pre_slope = pre_slope; e.act = act; e.act_slope = act_slope;
  const int Tout = conv1d_out_len(p->L, Tin);
  e.R = res; e.ldR = Tout;
  conv1d_run(p->L, (hipStream_t)stream, x, Tin, Tin, y, Tout, e);
  check_launch();
  RVC_CATCH
}
int rvc_conv1d_plan_pair_run(rvc_conv1d_plan* c1, rvc_conv1d_plan* c2, void* stream, const float* x, int T, float* y, float out_scale,
                             int accumulate) {
  RVC_TRY
  RVC_REQUIRE(c1 && c2 && x && y, "null argument");
  ConvEpilogue e; e.pre_act = ACT_LRELU; e.pre_slope = 0.1f; e.R = x; e.ldR = T; e.out_scale = out_scale; e.accumulate = accumulate;
  ConvPlan p;
  RVC_REQUIRE(conv_x3_pair_plan(c1->L, c2->L, x, T, T, T, y, T, e, conv_set_pair_arithmetic(-1), p),
              "this pair of layers is not eligible for the fused ResBlock kernel (needs bf16x3 images, C = 32, equal odd k, long T)");
  conv_plan_launch(p, (hipStream_t)stream);
  check_launch();
  RVC_CATCH
}
int rvc_conv1d_plan_resblock_run(rvc_conv1d_plan* const* plans6, void* stream, const float* x, int T, float* y, float out_scale, int accumulate,
                                 int* ran_out, const float* noise_src, const float* noise_w, const float* noise_b) {
  RVC_TRY
  RVC_REQUIRE(plans6 && x && y && ran_out, "null argument");
  const ConvLayer* c1[3]; const ConvLayer* c2[3];
  for (int i = 0; i < 3; ++i) {
    RVC_REQUIRE(plans6[2 * i] && plans6[2 * i + 1], "null plan");
    c1[i] = &plans6[2 * i]->L; c2[i] = &plans6[2 * i + 1]->L;
  }
  Rb3Plan p;
  *ran_out = conv_rb3_plan(c1, c2, x, T, T, T, y, T, 0.1f, out_scale, accumulate, conv_set_pair_arithmetic(-1), noise_src, noise_w, noise_b, p) ? 1 : 0;
  if (*ran_out) conv_rb3_launch(p, (hipStream_t)stream);
  check_launch();
  RVC_CATCH
}
int rvc_conv1d_plan_pair_split_run(rvc_conv1d_plan* c1, rvc_conv1d_plan* c2, void* stream, const float* x, int T, float* y, float out_scale,
                                   int accumulate) {
  RVC_TRY
  RVC_REQUIRE(c1 && c2 && x && y, "null argument");
  RVC_REQUIRE(conv1d_split_eligible(c1->L, T, SPLIT_PRODUCER) && conv1d_split_eligible(c2->L, T, SPLIT_CONSUMER), "layers not eligible for split-resident tensors at this length");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* img = (unsigned char*)stream_scratch(s, 5, split_image_bytes(c1->L.Co, T));
  ConvEpilogue E1; E1.pre_act = ACT_LRELU; E1.pre_slope = 0.1f; E1.ys_out = img; E1.ys_tp = split_image_tp(T); E1.ys_slope = 0.1f;
  // the arithmetic the generator would use for this pair at this length: fp16x2 on the persistent kernel where eligible (rvc_set_pair_arithmetic), else bf16x3
  E1.h2 = conv1d_pair_h2_eligible(c1->L, c2->L, T, conv_set_pair_arithmetic(-1)) ? 1 : 0;
  conv1d_run(c1->L, s, x, T, T, nullptr, T, E1);
  ConvEpilogue E2; E2.R = x; E2.ldR = T; E2.out_scale = out_scale; E2.accumulate = accumulate; E2.xs_in = img; E2.xs_tp = E1.ys_tp; E2.h2 = E1.h2;
  conv1d_run(c2->L, s, nullptr, T, T, y, T, E2);
  check_launch();
  RVC_CATCH
}
int rvc_conv1d_plan_pair_arithmetic(rvc_conv1d_plan* c1, rvc_conv1d_plan* c2, int T) {
  if (!c1 || !c2) return -1;
  try {
    const int h2 = conv_set_pair_arithmetic(-1);
    if (conv1d_pair_h2_eligible(c1->L, c2->L, T, h2)) return 1;
    // the fused pair of the narrow stages: which kernel family the plan chose (planning needs no tensors: x = residual = null)
    ConvEpilogue e; e.pre_act = ACT_LRELU; e.pre_slope = 0.1f; e.ldR = T;
    ConvPlan p;
    return conv_x3_pair_plan(c1->L, c2->L, nullptr, T, T, T, nullptr, T, e, h2, p) && p.a.h2 ? 1 : 0;
  } catch (...) { return -1; }
}
int rvc_conv1d_plan_destroy(rvc_conv1d_plan* p) { delete p; return 0; }
int rvc_op_attention(void* stream, const float* q, const float* k, const float* v_rm, const float* bv, float* out, int heads, int T) {
  RVC_TRY
  attention_fused((hipStream_t)stream, q, k, T, v_rm, (long long)heads * 64, bv, out, T, heads, 64, T);
  check_launch();
  RVC_CATCH
}
int rvc_op_attention_rel(void* stream, const float* q, const float* k, const float* v_rm, const float* bv, const float* rel, float* pb,
                         float* out, int heads, int T, const float* ek, const float* ev) {
  RVC_TRY
  attention_rel_fused((hipStream_t)stream, q, k, T, v_rm, (long long)heads * 96, bv, rel, pb, 10, out, T, heads, 96, T, ek, ev);
  check_launch();
  RVC_CATCH
}
int rvc_op_layernorm_c(void* stream, const float* x, const float* res, const float* gamma, const float* beta, float* y, int C, int T) {
  RVC_TRY
  layernorm_c((hipStream_t)stream, x, res, gamma, beta, y, C, T, T, 1e-5f);
  check_launch();
  RVC_CATCH
}
int rvc_op_layernorm_c_split(void* stream, const float* x, const float* gamma, const float* beta, float* y, float* y_img_f32, int C, int T) {
  RVC_TRY
  RVC_REQUIRE(x && gamma && beta && y_img_f32 && C > 0 && (C & 15) == 0 && T > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  DevBytes img;
  const long long tp = split_image_tp(T);
  img.alloc(split_image_bytes(C, T));
  layernorm_c_split(s, x, gamma, beta, y, img.p, tp, kSplitMargin, C, T, T, 1e-5f);
  split_image_to_f32(s, img.p, tp, C, T, y_img_f32, T);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_sine_source(void* stream, const float* f0, const float* noise, float* har, float* sine, int T, int upp, float sr, float lw, float lb,
                       float* rad_out, float* tmp_out, float* phase_out) {
  RVC_TRY
  hipStream_t st = (hipStream_t)stream;
  const long long N = (long long)T * upp;
  RVC_REQUIRE(T > 0 && upp > 0, "bad argument");
  const size_t nb = (size_t)((N + 1023) / 1024);
  const size_t tb = ((size_t)T * sizeof(float) + 255) & ~size_t(255);
  char* scr = (char*)stream_scratch(st, 2, 2 * tb + nb * sizeof(double));        // temporaries from the stream's scratch: nothing to leak on failure
  float* rad = (float*)scr; float* tmp = (float*)(scr + tb); double* bsum = (double*)(scr + 2 * tb);
  sine_source(st, f0, noise, har, sine, rad, tmp, bsum, T, upp, sr, lw, lb, phase_out);
  if (rad_out) RVC_HIP_CHECK(hipMemcpyAsync(rad_out, rad, T * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (tmp_out) RVC_HIP_CHECK(hipMemcpyAsync(tmp_out, tmp, T * sizeof(float), hipMemcpyDeviceToDevice, st));
  RVC_HIP_CHECK(hipStreamSynchronize(st));
  check_launch();
  RVC_CATCH
}

// ------------------------------------------------------------------------------------------------ single-op entry points of the model-glue kernels (ops.hip, split2d.hip)
// The image of a padded 2-D level as RMVPE's U-Net holds it: margin of split_geom_2d(W), every byte 0xff first (NaN patterns wherever the producer does not
// write), read back as fp32 [C][ld] over the P = H (W + 2) positions.
struct Image2d { DevBytes b; long long tp = 0; int margin = 0; };
static Image2d image2d_alloc(hipStream_t s, int C, int H, int W) {
  Image2d im;
  im.margin = split_geom_2d(W).margin;
  im.tp = im.margin + (long long)H * (W + 2) + 704 + 64;
  const size_t bytes = (size_t)(C / 16) * 4 * im.tp * 16;
  im.b.alloc(bytes);
  RVC_HIP_CHECK(hipMemsetAsync(im.b.p, 0xff, bytes, s));
  return im;
}
static void image2d_to_f32(hipStream_t s, const Image2d& im, int C, long long P, float* y, long long ld) {
  // (the reader's margin is fixed at 64 rows: hand it the plane origin shifted so that position 0 lands there)
  split_image_to_f32(s, im.b.p + (size_t)(im.margin - kSplitMargin) * 16, im.tp, C, (int)P, y, ld);
}

int rvc_op_hubert_conv0(void* stream, const float* audio, int64_t L, const float* w, const float* gamma, const float* beta, int C, int T1, float* out, float* out_img_f32,
                        int64_t ld) {
  RVC_TRY
  RVC_REQUIRE(audio && w && gamma && beta && (out || out_img_f32) && C > 0 && T1 > 0 && L > 0 && ld >= T1, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  DevBuf<double> partial; DevBuf<float> stat; DevBytes img;
  partial.alloc(hubert_conv0_scratch_doubles(C, T1)); stat.alloc((size_t)2 * C);
  if (out) hubert_conv0_gn_gelu(s, audio, L, w, gamma, beta, C, T1, 1e-5f, out, ld, partial.p, stat.p);
  if (out_img_f32) {
    RVC_REQUIRE((C & 15) == 0, "the image needs C % 16 == 0");
    const long long tp = split_s2_tp(T1); const int H = split_s2_h(T1);
    img.alloc(split_s2_bytes(C, T1));
    RVC_HIP_CHECK(hipMemsetAsync(img.p, 0xff, split_s2_bytes(C, T1), s));
    hubert_conv0_gn_gelu_img(s, audio, L, w, gamma, beta, C, T1, 1e-5f, img.p, tp, kSplitMargin, H, partial.p, stat.p);
    split_image_deint_to_f32(s, img.p, tp, H, C, T1, out_img_f32, ld);
  }
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_conv_to1(void* stream, const float* x, int64_t ldx, const float* w, int Ci, int K, int pad, int T, float pre_slope, int act_tanh, float* y, int* kernel_out) {
  RVC_TRY
  RVC_REQUIRE(x && w && y && kernel_out && Ci > 0 && K > 0 && pad >= 0 && T > 0 && ldx >= T, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  *kernel_out = conv_to1(s, x, ldx, w, Ci, K, pad, T, pre_slope, act_tanh, y);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_noise_add(void* stream, float* x, int64_t ld, int C, int T, const float* src, int64_t L, int k, int stride, int pad, const float* w, const float* b, int* ran_out) {
  RVC_TRY
  RVC_REQUIRE(x && src && w && b && ran_out && C > 0 && T > 0 && L > 0 && k > 0 && stride > 0 && pad >= 0 && ld >= T, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  *ran_out = noise_add(s, x, ld, C, T, src, L, k, stride, pad, w, b) ? 1 : 0;
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_transpose(void* stream, const float* in, float* out, int R, int C, int64_t ldin, int64_t ldout, int batch, int64_t bin, int64_t bout) {
  RVC_TRY
  RVC_REQUIRE(in && out && R > 0 && C > 0 && batch > 0 && ldin >= C && ldout >= R, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  transpose(s, in, out, R, C, ldin, ldout, batch, bin, bout);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_frames(void* stream, const float* src, float* out, int L, int k, int stride, int pad, int Tout, int reflect) {
  RVC_TRY
  RVC_REQUIRE(src && out && L > 0 && k > 0 && stride > 0 && pad >= 0 && Tout > 0, "bad argument");
  RVC_REQUIRE(!reflect || (pad < L && (long long)(Tout - 1) * stride + k - 1 - pad <= 2LL * (L - 1)), "a reflected index must land inside the signal");
  hipStream_t s = (hipStream_t)stream;
  frames(s, src, out, L, k, stride, pad, Tout, reflect);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_mel_to_unet(void* stream, const float* mel, float* x, int n, int Tr, float a, float b) {
  RVC_TRY
  RVC_REQUIRE(mel && x && n > 0 && Tr >= n && Tr <= 2 * n - 1, "bad argument (the right reflection must land inside the n frames)");
  hipStream_t s = (hipStream_t)stream;
  mel_to_unet(s, mel, x, n, Tr, a, b);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_feats_prepare(void* stream, const float* f, const float* f0, const float* pitchf, float* out, int D, int Th, int T, float protect, int do_protect) {
  RVC_TRY
  RVC_REQUIRE(f && out && (pitchf || !do_protect) && D > 0 && Th > 0 && T > 0 && T <= 2 * Th, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  feats_prepare(s, f, f0, pitchf, out, D, Th, T, protect, do_protect);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_wn_gate(void* stream, const float* a, const float* g, float* out, float* out_img_f32, int H, int T) {
  RVC_TRY
  RVC_REQUIRE(a && g && (out || out_img_f32) && H > 0 && T > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  DevBytes img;
  if (out) wn_gate(s, a, g, out, H, T);
  if (out_img_f32) {
    const long long tp = split_image_tp(T);
    img.alloc(split_image_bytes(H, T));
    RVC_HIP_CHECK(hipMemsetAsync(img.p, 0xff, split_image_bytes(H, T), s));
    wn_gate_split(s, a, g, img.p, tp, kSplitMargin, H, T);
    split_image_to_f32(s, img.p, tp, H, T, out_img_f32, T);
  }
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_pool2_pad(void* stream, const float* x, int64_t ldx, int x_padded, int C, int H, int W, float* y, float* y_img_f32, int64_t ldy) {
  RVC_TRY
  RVC_REQUIRE(x && (y || y_img_f32) && C > 0 && H >= 2 && W >= 2, "bad argument");
  const int Ho = H / 2, Wo = W / 2; const long long P = (long long)Ho * (Wo + 2);
  RVC_REQUIRE(ldx >= (long long)H * (x_padded ? W + 2 : W) && ldy >= P, "bad pitch");
  hipStream_t s = (hipStream_t)stream;
  Image2d im;
  if (y_img_f32) im = image2d_alloc(s, C, Ho, Wo);
  pool2_pad_split(s, x, ldx, x_padded != 0, C, H, W, y, ldy, im.b.p, im.tp, im.margin);
  if (y_img_f32) image2d_to_f32(s, im, C, P, y_img_f32, ldy);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_interleave2_pad(void* stream, const float* ph, int64_t ldp, int Co, int H, int W, float* y, int y_padded, float* y_img_f32, int64_t ldy) {
  RVC_TRY
  RVC_REQUIRE(ph && (y || y_img_f32) && Co > 0 && H > 0 && W > 0 && ldp >= (long long)H * (W + 2), "bad argument");
  const long long P = (long long)(2 * H) * (2 * W + 2);      // the image (and its read-back) is always the padded level
  RVC_REQUIRE(ldy >= ((y_padded || y_img_f32) ? P : (long long)(2 * H) * (2 * W)), "bad pitch");
  hipStream_t s = (hipStream_t)stream;
  Image2d im;
  if (y_img_f32) im = image2d_alloc(s, Co, 2 * H, 2 * W);
  interleave2_pad_split(s, ph, ldp, Co, H, W, y, ldy, y_padded != 0, im.b.p, im.tp, im.margin);
  if (y_img_f32) image2d_to_f32(s, im, Co, P, y_img_f32, ldy);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_pad2d(void* stream, const float* x, int64_t ldx, int C, int H, int W, float* y, float* y_img_f32, int64_t ldy) {
  RVC_TRY
  const long long P = (long long)H * (W + 2);
  RVC_REQUIRE(x && (y || y_img_f32) && C > 0 && H > 0 && W > 0 && ldx >= (long long)H * W && ldy >= P, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  Image2d im;
  if (y_img_f32) im = image2d_alloc(s, C, H, W);
  pad2d_split(s, x, ldx, C, H, W, y, ldy, im.b.p, im.tp, im.margin);
  if (y_img_f32) image2d_to_f32(s, im, C, P, y_img_f32, ldy);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_unpad2d(void* stream, const float* x, int64_t ldx, int C, int H, int W, float* y, int64_t ldy) {
  RVC_TRY
  RVC_REQUIRE(x && y && C > 0 && H > 0 && W > 0 && ldx >= (long long)H * (W + 2) && ldy >= (long long)H * W, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  unpad2d(s, x, ldx, C, H, W, y, ldy);
  check_launch();
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  RVC_CATCH
}
int rvc_op_gru_scan(void* stream, const float* gi, const float* b_ih, const float* w_hh, const float* b_hh, float* out, int T, int* err_out) {
  RVC_TRY
  RVC_REQUIRE(gi && b_ih && w_hh && b_hh && out && err_out && T > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  DevBuf<unsigned long long> xbuf; DevBuf<int> err;
  xbuf.alloc((size_t)2 * 2 * 256); err.alloc(2);
  gru_scan(s, gi, b_ih, w_hh, nullptr, b_hh, out, xbuf.p, err.p, T);      // no repair kernel; the product's default spin limit
  check_launch();
  int e[2] = {0, 0};
  RVC_HIP_CHECK(hipMemcpyAsync(e, err.p, sizeof(e), hipMemcpyDeviceToHost, s));
  RVC_HIP_CHECK(hipStreamSynchronize(s));
  *err_out = e[0];
  RVC_CATCH
}

int rvc_prof_enable(int on) { RVC_TRY conv_prof_enable(on != 0); RVC_CATCH }
int rvc_set_conv_precision(int mode) {
  RVC_TRY
  RVC_REQUIRE(mode >= 0 && mode <= 2, "precision mode must be 0, 1 or 2");
  conv_set_precision(mode);
  RVC_CATCH
}
int rvc_set_pair_arithmetic(int mode) {
  RVC_TRY
  RVC_REQUIRE(mode == 0 || mode == 1, "pair arithmetic must be 0 (bf16x3) or 1 (fp16x2)");
  conv_set_pair_arithmetic(mode);
  RVC_CATCH
}
int rvc_get_pair_arithmetic(void) { return conv_set_pair_arithmetic(-1); }
int rvc_prof_collect(double* ms, double* flops, int64_t* launches) {
  RVC_TRY
  static_assert(RVC_PROF_CFGS == kProfCfgs, "profiling table size");
  long long l[RVC_PROF_CFGS];
  conv_prof_collect(ms, flops, l);
  for (int i = 0; i < RVC_PROF_CFGS; ++i) launches[i] = l[i];
  RVC_CATCH
}
int rvc_prof_collect_ex(double* out, double ridge_fp32, double ridge_x3) { RVC_TRY conv_prof_collect_ex(out, ridge_fp32, ridge_x3); RVC_CATCH }
const char* rvc_prof_cfg_name(int i) { return conv_prof_cfg_name(i); }
int rvc_prof_dump_csv(const char* path) { RVC_TRY RVC_REQUIRE(path && conv_prof_dump_csv(path) >= 0, "cannot write the launch table"); RVC_CATCH }
#ifdef RVC_EXPERIMENTS
int rvc_debug_read_scratch(void* stream, int slot, void* host_dst, size_t bytes) {
  RVC_TRY
  void* p = stream_scratch((hipStream_t)stream, slot, bytes);
  RVC_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  RVC_HIP_CHECK(hipMemcpy(host_dst, p, bytes, hipMemcpyDeviceToHost));
  RVC_CATCH
}
int rvc_debug_conv_timing(uint64_t* out8, int reset) { RVC_TRY conv_timing_read((unsigned long long*)out8, reset != 0); RVC_CATCH }
int rvc_debug_x3p_check(void) { return conv_x3p_check_read(); }
int rvc_debug_gemm_split_bench(void* stream, int Ci, int Co, int T, int ksplit, int am, int an, int split_out, int reps, float* us_out, int w2d, int nlayers) {
  RVC_TRY
  RVC_REQUIRE(us_out && reps > 0 && Ci > 0 && Co > 0 && T > 0 && nlayers >= 1 && nlayers <= 64, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int kt = w2d > 0 ? 9 : 1;
  std::vector<float> w((size_t)Co * Ci * kt), b((size_t)Co, 0.01f);
  uint32_t st = 12345u;
  std::vector<OwnedConvLayer> Ls((size_t)nlayers);
  DevBuf<float> x, r, y; DevBytes xs, ys;
  struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } e0, e1;
  for (auto& L : Ls) {      // distinct weights per layer: cycled through, they come from HBM like a model's layers do
    for (auto& v : w) { st = st * 1664525u + 1013904223u; v = ((float)(st >> 8) / 8388608.f - 1.f) * 0.05f; }
    ConvBuildScope scope(2);
    if (w2d > 0) conv2d3x3_layer_init(L, w.data(), b.data(), Co, Ci); else conv1d_layer_init(L, w.data(), b.data(), Co, Ci, 1, 1, 0, 1, 1);
  }
  SplitGeom g; if (w2d > 0) g = split_geom_2d(w2d);
  const long long tp = ((long long)g.margin + T + 704 + 63) & ~63LL;
  std::vector<float> hx((size_t)Ci * T);
  for (auto& v : hx) { st = st * 1664525u + 1013904223u; v = (float)(st >> 8) / 8388608.f - 1.f; }
  x.upload(hx);
  r.alloc((size_t)Co * T); RVC_HIP_CHECK(hipMemset(r.p, 0, (size_t)Co * T * 4));
  y.alloc((size_t)Co * T);
  const size_t ib = (size_t)(Ci / 16) * 4 * tp * 16, ob = (size_t)((Co + 15) / 16) * 4 * tp * 16;
  xs.alloc(ib); RVC_HIP_CHECK(hipMemset(xs.p, 0, ib)); ys.alloc(ob); RVC_HIP_CHECK(hipMemset(ys.p, 0, ob));
  split_image_from_f32(s, x.p, T, Ci, T, xs.p + (size_t)(g.margin - kSplitMargin) * 16, tp);
  ConvEpilogue e;
  if (split_out) { e.act = ACT_GELU; e.ys_out = ys.p; e.ys_tp = tp; } else { e.R = r.p; e.ldR = T; }
  X3sForceScope force(ksplit, am, an);
  for (auto& L : Ls) conv_x3s_run(L, s, xs.p, tp, T, split_out ? nullptr : y.p, T, e, w2d > 0 ? &g : nullptr);
  RVC_HIP_CHECK(hipEventCreate(&e0.e)); RVC_HIP_CHECK(hipEventCreate(&e1.e));
  RVC_HIP_CHECK(hipEventRecord(e0.e, s));
  for (int i = 0; i < reps; ++i) conv_x3s_run(Ls[(size_t)(i % nlayers)], s, xs.p, tp, T, split_out ? nullptr : y.p, T, e, w2d > 0 ? &g : nullptr);
  RVC_HIP_CHECK(hipEventRecord(e1.e, s));
  RVC_HIP_CHECK(hipEventSynchronize(e1.e));
  float ms = 0.f; RVC_HIP_CHECK(hipEventElapsedTime(&ms, e0.e, e1.e));
  *us_out = ms * 1e3f / (float)reps;
  RVC_CATCH
}

#endif  // RVC_EXPERIMENTS

}  // extern "C"
