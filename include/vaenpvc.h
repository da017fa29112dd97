/*
 * vaenpvc.h -- C-ABI of the MI355X-native ConvVAE hot path (libvaenpvc_hip.so).
 *
 * The reference (JeremyCCHsu/vae-npvc) has NO foreign-function interface: its hot
 * path is a TensorFlow-1 graph executed by `sess.run`.  This header is therefore the
 * boundary a maintainer would bind instead of building that graph; each entry point
 * cites the reference code whose arithmetic it replaces (paths relative to the
 * reference repository root).  See INTEGRATION.md for the ctypes stub.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller, contiguous,
 *     16-byte aligned; no device memory is allocated or freed behind the ABI;
 *   - all work is enqueued on the caller's `hipStream_t` (passed as void*) and is ordered
 *     with it; nothing synchronises the host (exceptions, stated at the function:
 *     vaenpvc_timer_read, vaenpvc_validate_ids).  ONE internal helper stream per context:
 *     the backward pass forks the weight-gradient kernels onto it (event fork after the
 *     gradient tensor they read is complete, event join before the call returns its work
 *     to the caller's stream), so the caller observes plain stream order.  The stream and
 *     its events are created lazily on the device that is current at the context's first
 *     launch and destroyed by vaenpvc_ctx_destroy; VAENPVC_SIDE_STREAM=0 (read at context
 *     creation) or backward-mask bit 30 cleared keeps everything on the caller's stream
 *     (the library itself does so for two-term operands from 16 384 frames per call on,
 *     where the fork measured slower; VAENPVC_SIDE_STREAM=1 forces the fork everywhere);
 *   - no mutable state outside the context: masks, precision, timer and the helper stream
 *     belong to the `vaenpvc_ctx`; entry points that take a context lock it for the
 *     duration of the call, so different contexts may be driven from different host
 *     threads (and devices) concurrently, and one context from several threads serially;
 *   - return value: 0 = ok, <0 = error (see VAENPVC_E_*); `vaenpvc_last_error()`
 *     returns a thread-local message; no C++ exception crosses the ABI;
 *   - frames are rows: x is [F, H] float32 (the reference's [F,1,H,1] NCHW tensor,
 *     analyzer.py:116-122), y is int64 [F] (analyzer.py:127), H = 513;
 *   - 1 <= F <= 262 144 (2^18) frames per call: element offsets inside the kernels are 32-bit for
 *     the largest per-frame tensor; larger batches return VAENPVC_E_ARG (split them on the host:
 *     frames are independent, gradients of the mean add with weights F_i / F).
 */
#ifndef VAENPVC_H_
#define VAENPVC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAENPVC_MAX_LAYERS 8

#define VAENPVC_OK 0
#define VAENPVC_E_ARG (-1)       /* bad argument / malformed architecture */
#define VAENPVC_E_WORKSPACE (-2) /* workspace too small */
#define VAENPVC_E_HIP (-3)       /* a HIP runtime call failed */
#define VAENPVC_E_UNSUPPORTED (-4)
#define VAENPVC_E_STATE (-5)     /* the call needs state a preceding call of the same context did not leave (vaenpvc_train_bwd_target) */

/* implementation selector (vaenpvc_set_impl) */
#define VAENPVC_IMPL_AUTO 0 /* tuned gfx950 kernels where the geometry matches, generic otherwise */
#define VAENPVC_IMPL_GENERIC 1 /* geometry-generic HIP kernels only (cross-check path) */

/* workspace modes */
#define VAENPVC_MODE_INFER 0
#define VAENPVC_MODE_TRAIN 1

/* operand precision of the GEMM-shaped kernels on the bf16 matrix cores (vaenpvc_set_precision):
 * every fp32 operand is split into this many bf16 terms; accumulation is always fp32 */
#define VAENPVC_PREC_BF16X3 3 /* 3 terms, 6 products: fp32-exact (1e-6 of max|C|) */
#define VAENPVC_PREC_BF16X2 2 /* default: 2 terms, 3 products, 16 mantissa bits per operand: activations <= 1.4e-5,
                               * gradients <= 3.0e-5 of their tensor's scale against the float64 oracle at 32 768
                               * frames (bars 1e-4 / 2e-4; DESIGN.md section 5 on how lrelu kinks are kept out of
                               * that comparison) */
#define VAENPVC_PREC_AUTO VAENPVC_PREC_BF16X2
#define VAENPVC_PREC_BF16 1   /* plain bf16 operands (BASELINE.json config 2 "bf16"; ~1e-2) */

/* Architecture description = the keys model/vae.py actually reads from
 * architecture-*.json (model/vae.py:22-23,39,74,80-81,86,95).  Kernels are [k,1],
 * strides [s,1] (W = 1 everywhere). */
typedef struct vaenpvc_arch {
  int32_t H;     /* arch["hwc"][0] : bins per frame (513) */
  int32_t z_dim; /* arch["z_dim"] ; also the speaker-embedding width (model/vae.py:21-24) */
  int32_t y_dim; /* arch["y_dim"] : number of speakers */
  int32_t n_enc;
  int32_t enc_kernel[VAENPVC_MAX_LAYERS];
  int32_t enc_stride[VAENPVC_MAX_LAYERS];
  int32_t enc_output[VAENPVC_MAX_LAYERS];
  int32_t gen_h; /* arch["generator"]["hwc"] = [h, w(=1), c] */
  int32_t gen_c;
  int32_t n_dec;
  int32_t dec_kernel[VAENPVC_MAX_LAYERS];
  int32_t dec_stride[VAENPVC_MAX_LAYERS];
  int32_t dec_output[VAENPVC_MAX_LAYERS];
} vaenpvc_arch;

typedef struct vaenpvc_ctx vaenpvc_ctx;

/* ABI version of this header; bumped on any signature change. */
int vaenpvc_abi_version(void);
const char* vaenpvc_last_error(void);

/* Replaces ConvVAE.__init__ / _sanity_check (model/vae.py:9-39): validates the
 * architecture (AssertionError analogue = VAENPVC_E_ARG) and derives the TF 'SAME'
 * shape chain. Holds no device memory. */
int vaenpvc_ctx_create(const vaenpvc_arch* arch, vaenpvc_ctx** out);
void vaenpvc_ctx_destroy(vaenpvc_ctx* ctx);
int vaenpvc_set_impl(vaenpvc_ctx* ctx, int impl);
/* Operand precision of this context (VAENPVC_PREC_*).  The reference computes in fp32
 * (tf.float32 everywhere); BF16X2 / BF16X3 meet its 1e-4 parity bar, BF16 is the reduced
 * precision training mode. */
int vaenpvc_set_precision(vaenpvc_ctx* ctx, int planes);
int vaenpvc_get_precision(const vaenpvc_ctx* ctx);
/* Weight gradients of the merge layer and decoder layer 0 on the VCC2016 geometry (no reference counterpart; same
 * result, another order of summation).  Nothing non-linear sits between the two layers, so both gradients follow from
 * dWc = z^T du0 (du0 = gradient at decoder layer 0's pre-LayerNorm output) and the per-speaker sums of du0, pushed
 * through the conv kernels as 138 pseudo-frames.  mode: 0 = never (one frame-sized GEMM per layer), 1 = from 1 024
 * frames per call on (default; environment VAENPVC_D0W_FACTOR at context creation), 2 = whenever the kernels serve the
 * shape.  May be changed between a train step and vaenpvc_train_bwd_target: the backward pass re-makes operands the
 * forward pass did not leave.  vaenpvc_get_d0w_route: the route the last layered backward pass of this context took. */
#define VAENPVC_D0W_ROUTE_FP32 0       /* exact-fp32 conv weight-gradient kernel (or the generic kernels / no layered backward pass yet) */
#define VAENPVC_D0W_ROUTE_FACTOR 1     /* the factorised route */
#define VAENPVC_D0W_ROUTE_PLANES 2     /* frame-sized plane GEMMs, operand planes of h left by the forward pass */
#define VAENPVC_D0W_ROUTE_PLANES_REDO 3 /* frame-sized plane GEMMs, operand planes of h re-made by the backward pass */
int vaenpvc_set_d0w_factor(vaenpvc_ctx* ctx, int mode);
int vaenpvc_get_d0w_route(const vaenpvc_ctx* ctx);

/* Trainable-tensor table = tf.trainable_variables() of the reference in creation
 * order (model/vae.py:20-24,72-103; util/layers.py:33-64): 44 tensors for the
 * VCC2016 architecture, stored back to back in ONE flat float32 buffer in TF layouts
 * (conv [k,1,Cin,Cout]; conv_transpose [k,1,Cout,Cin]; dense [in,out]). */
int vaenpvc_param_count(const vaenpvc_ctx* ctx);
int64_t vaenpvc_param_floats(const vaenpvc_ctx* ctx);
/* name: caller buffer of name_cap bytes; shape: int64[4]; returns 0 / VAENPVC_E_ARG */
int vaenpvc_param_info(const vaenpvc_ctx* ctx, int index, char* name, int name_cap,
                       int64_t* offset_floats, int32_t* ndim, int64_t* shape);

/* Workspace (activations kept for backward, per-frame statistics, gradient
 * scratch).  `vaenpvc_ws_find` exposes named regions (float offsets into d_ws) so
 * that tests can inspect every intermediate the reference graph would hold:
 *   enc_a<i>, enc_st<i>, z_mu, z_lv, z, eps, h, dec_a<i>, dec_st<i>, xh,
 *   kl_f, nll_f, d_enc_a<i>, d_z_mu, d_z_lv, d_z, d_h, d_dec_a<i>, d_xh
 * The forward regions are written at every batch size.  The gradient regions are the
 * hand-over buffers of the backward pass: on the tuned path at >= 1024 frames several
 * of them are never written because the gradient travels as bf16 operand planes
 * (d_h, d_z_mu / d_z_lv, d_enc_a3 / d_enc_a4, d_dec_a0; regions pl_*, cl<i>) -- select
 * the generic path (vaenpvc_set_impl) to inspect every one of them.               */
int64_t vaenpvc_workspace_bytes(const vaenpvc_ctx* ctx, int64_t F, int mode);
int vaenpvc_ws_find(const vaenpvc_ctx* ctx, int64_t F, int mode, const char* name,
                    int64_t* offset_floats, int64_t* count_floats);

/* ConvVAE.encode (model/vae.py:139-141 -> _encoder 72-82; util/layers.py:47-66):
 * d_z_mu [F,z_dim]; d_z_lv may be NULL (convert.py:85 only uses z_mu). */
int vaenpvc_encode_fwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, int64_t F,
                       float* d_z_mu, float* d_z_lv, void* d_ws, size_t ws_bytes, void* stream);

/* ConvVAE.decode / generate (model/vae.py:143-145 -> _generator 84-103, _merge 51-61;
 * util/image.py:4-5 NHWC transpose is a no-op on memory since W = 1):
 * d_z [F,z_dim], d_y int64 [F] -> d_xh [F,H]. */
int vaenpvc_decode_fwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_z,
                       const int64_t* d_y, int64_t F, float* d_xh, void* d_ws, size_t ws_bytes,
                       void* stream);

/* ConvVAE.loss (model/vae.py:106-137; util/layers.py:152-183) + the gradient half of
 * `optimizer.minimize(loss['G'])` (trainer/vae.py:19-24).
 * d_eps [F,z_dim] is the N(0,1) draw of GaussianSampleLayer, injected by the caller
 * (the reference's tf.random_normal is unseeded).
 * d_grads: flat float32 buffer, same layout as d_params, OVERWRITTEN with
 *          d loss['G'] / d params for the LOCAL mean over these F frames.
 * d_loss3: float[3] = { G, D_KL, logP } (model/vae.py:127-130). */
int vaenpvc_train_fwd_bwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_x,
                          const int64_t* d_y, const float* d_eps, int64_t F, float* d_grads,
                          float* d_loss3, void* d_ws, size_t ws_bytes, void* stream);

/* Same step with the sampler's N(0,1) draw generated on the device inside the sampler kernel
 * (util/layers.py:154 tf.random_normal): Philox4x32-10 keyed by `seed`, counter words 2-3 =
 * `offset` (pass the global step so every step draws fresh noise; with data parallelism give
 * every rank its own seed).  Element e of the [F, z_dim] draw is the (e & 3)-th Box-Muller
 * normal of Philox counter (e >> 2, offset); vaenpvc_philox_normal produces the identical
 * tensor stand-alone.  The draw is kept in workspace region "eps" for the backward pass.
 * d_offset (may be NULL): device int64 added to `offset` when the kernel RUNS, so that a
 * captured hipGraph draws fresh noise on every replay (pass the device step counter that
 * vaenpvc_adam_step_dev increments). */
int vaenpvc_train_fwd_bwd_seeded(vaenpvc_ctx* ctx, const float* d_params, const float* d_x,
                                 const int64_t* d_y, uint64_t seed, uint64_t offset,
                                 const int64_t* d_offset, int64_t F, float* d_grads,
                                 float* d_loss3, void* d_ws, size_t ws_bytes, void* stream);
int vaenpvc_philox_normal(uint64_t seed, uint64_t offset, float* d_out, int64_t n, void* stream);
/* U[0,1) from the same generator (element e = top 24 bits of word e & 3 of counter (e >> 2, offset)): the
 * per-frame interpolation coefficients of the gradient penalty (tf.random_uniform in WGAN-GP critics). */
int vaenpvc_philox_uniform(uint64_t seed, uint64_t offset, float* d_out, int64_t n, void* stream);

/* The same step with the log-density evaluated against d_target [F,H] instead of d_x (the encoder still reads
 * d_x): d G / d xh becomes (xh - target) / ((1 + 1e-6) F).  With target = x + alpha (1 + 1e-6) dD(xh)/dxh
 * (vaenpvc_disc_generator_target) the 'Generator' and 'y_emb' ranges of d_grads hold the gradient of
 * l_G = -logP + alpha W_dist of the VAWGAN trainer (trainer/vae.py:141-145); d_loss3 is then meaningless. */
int vaenpvc_train_fwd_bwd_target(vaenpvc_ctx* ctx, const float* d_params, const float* d_x,
                                 const int64_t* d_y, const float* d_eps, const float* d_target, int64_t F,
                                 float* d_grads, float* d_loss3, void* d_ws, size_t ws_bytes, void* stream);
/* Backward pass only, against d_target, on the activations a preceding vaenpvc_train_fwd_bwd / _target call
 * left in d_ws: same context, parameters, x, y, eps, F and workspace, nothing else run on that workspace in
 * between.  The backward pass reads the forward tensors and writes only gradient regions, so the second gradient
 * of the VAWGAN generator step (l_G after l_E) costs one backward instead of a whole step.  The context remembers the
 * batch size, kernel selection, precision and workspace of its last train step and returns VAENPVC_E_STATE when this call
 * does not match them (the backward pass would otherwise consume stale or unwritten operands without a sign). */
int vaenpvc_train_bwd_target(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                             const float* d_eps, const float* d_target, int64_t F, float* d_grads,
                             float* d_loss3, void* d_ws, size_t ws_bytes, void* stream);

/* Gradient buckets for data-parallel overlap (no reference counterpart: the reference is single
 * GPU).  The backward pass finishes the flat gradient buffer back to front -- decoder convs,
 * merge, heads, then embedding + encoder -- and each of those is ONE contiguous range of
 * d_grads.  When a callback is registered it is invoked ON THE CALLING HOST THREAD, during
 * vaenpvc_train_fwd_bwd*, once per range as soon as every kernel that writes it has been
 * enqueued; `ready_stream` is a stream on which those kernels are ordered before anything the
 * callback enqueues on it (record an event there / make the communication stream wait on it and
 * start the all-reduce of d_grads[offset, offset + count) while the rest of the backward pass
 * still runs).  bucket ids count up from 0 in call order; cb = NULL unregisters. */
typedef void (*vaenpvc_bucket_cb)(void* user, int32_t bucket, int64_t offset_floats,
                                  int64_t count_floats, void* ready_stream);
int vaenpvc_set_bucket_callback(vaenpvc_ctx* ctx, vaenpvc_bucket_cb cb, void* user);

/* Forward + losses only (VAETrainer._refresh_status fetch, trainer/vae.py:31-36). */
int vaenpvc_loss_fwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_x,
                     const int64_t* d_y, const float* d_eps, int64_t F, float* d_loss3,
                     void* d_ws, size_t ws_bytes, void* stream);
int vaenpvc_loss_fwd_seeded(vaenpvc_ctx* ctx, const float* d_params, const float* d_x,
                            const int64_t* d_y, uint64_t seed, uint64_t offset, int64_t F,
                            float* d_loss3, void* d_ws, size_t ws_bytes, void* stream);

/* tf.train.AdamOptimizer apply for all trainables as ONE fused pass over the flat
 * buffers (trainer/vae.py:16-24; TF-flavour: p -= lr_t * m / (sqrt(v) + eps),
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t), t = step, 1-based).  grad_scale multiplies the
 * gradient first (1/world_size after an all-reduce SUM). */
int vaenpvc_adam_step(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n,
                      int64_t step, float lr, float beta1, float beta2, float eps,
                      float grad_scale, void* stream);

/* Same update, but the step counter lives in device memory: the kernel sequence first
 * increments *d_step (int64) and derives lr_t from it on the device, so the call can be
 * captured in a hipGraph and replayed (trainer/vae.py:94-99 hot loop without host work). */
int vaenpvc_adam_step_dev(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n,
                          int64_t* d_step, float lr, float beta1, float beta2, float eps,
                          float grad_scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VAWGAN branch (trainer/vae.py:115-218, architecture-vawgan-vcc2016.json).  The reference tree holds the
 * trainer and the architecture file but not the model class (README.md:3 points at another git branch), so
 * the critic is SPECIFIED in DESIGN.md section 9 from what the tree pins down: convs of
 * arch["discriminator"] built with the tree's conv + LayerNorm + lrelu block (util/layers.py:47-66,147-149),
 * one dense unit, WGAN-GP losses
 *     W_dist = mean D(x) - mean D(xh),  gp = mean_f (|dD(xi_f)/dxi_f| - 1)^2,  xi = x + t (xh - x),
 *     l_D = -W_dist + lambda gp,  l_E = -logP + D_KL,  l_G = -logP + alpha W_dist.
 * The critic owns its own flat parameter buffer (14 tensors for the VCC2016 file, names
 * Discriminator/Conv2d-<i>/{kernel,bias,layernorm.offset,layernorm.scale}, Discriminator/dense/{kernel,bias});
 * the object holds geometry only, no device memory and no mutable state. */
typedef struct vaenpvc_disc_arch {
  int32_t H; /* arch["hwc"][0] */
  int32_t n_layers;
  int32_t kernel[VAENPVC_MAX_LAYERS]; /* arch["discriminator"]["kernel"][i][0] */
  int32_t stride[VAENPVC_MAX_LAYERS];
  int32_t output[VAENPVC_MAX_LAYERS];
} vaenpvc_disc_arch;
typedef struct vaenpvc_disc vaenpvc_disc;
int vaenpvc_disc_create(const vaenpvc_disc_arch* arch, vaenpvc_disc** out);
void vaenpvc_disc_destroy(vaenpvc_disc* disc);
int vaenpvc_disc_param_count(const vaenpvc_disc* disc);
int64_t vaenpvc_disc_param_floats(const vaenpvc_disc* disc);
int vaenpvc_disc_param_info(const vaenpvc_disc* disc, int index, char* name, int name_cap,
                            int64_t* offset_floats, int32_t* ndim, int64_t* shape);
int64_t vaenpvc_disc_workspace_bytes(const vaenpvc_disc* disc, int64_t F); /* 1 <= F <= 65536 */
/* Critic values of x and xh: d_out (may be NULL) float[2F] = D(x) | D(xh); d_loss2 (may be NULL) = {W_dist, 0}. */
int vaenpvc_disc_fwd(const vaenpvc_disc* disc, const float* d_dparams, const float* d_x, const float* d_xh,
                     int64_t F, float* d_out, float* d_loss2, void* d_ws, size_t ws_bytes, void* stream);
/* `optimizer.minimize(loss['l_D'], var_list=d_vars)` gradient half (trainer/vae.py:141): d_t float[F] are the
 * interpolation coefficients; d_dgrads (critic layout) is OVERWRITTEN with d l_D / d critic parameters
 * (first and second order terms: the penalty differentiates the critic's input gradient);
 * d_loss2 = {W_dist, gp} (the trainer's status line, trainer/vae.py:196-201). */
int vaenpvc_disc_critic_fwd_bwd(const vaenpvc_disc* disc, const float* d_dparams, const float* d_x,
                                const float* d_xh, const float* d_t, int64_t F, float lambda,
                                float* d_dgrads, float* d_loss2, void* d_ws, size_t ws_bytes, void* stream);
/* Generator side of the adversarial term: d_target [F,H] = x + alpha (1 + 1e-6) dD(xh)/dxh, to be passed to
 * vaenpvc_train_fwd_bwd_target; d_loss2 (may be NULL) = {W_dist, 0}. */
int vaenpvc_disc_generator_target(const vaenpvc_disc* disc, const float* d_dparams, const float* d_x,
                                  const float* d_xh, int64_t F, float alpha, float* d_target, float* d_loss2,
                                  void* d_ws, size_t ws_bytes, void* stream);

/* Tanhize.forward_process / backward_process (analyzer.py:82-87), per bin:
 * fwd: clip((x-xmin)/(xmax-xmin),0,1)*2-1 ; bwd: (x*.5+.5)*(xmax-xmin)+xmin.
 * d_xmin/d_xmax: float32 [H]. In-place allowed. */
int vaenpvc_tanhize_fwd(const float* d_sp, const float* d_xmin, const float* d_xmax, float* d_x,
                        int64_t F, int32_t H, void* stream);
int vaenpvc_tanhize_bwd(const float* d_x, const float* d_xmin, const float* d_xmax, float* d_sp,
                        int64_t F, int32_t H, void* stream);

/* Global-variance (GV) post-filter fused with Tanhize.backward_process (not in the reference: README.md "TODO: GV",
 * and "Global variance post-filtering was not included in this repo").  d_x [F,H] is decoder output in the Tanhize
 * domain holding n_seg utterances back to back: utterance u is rows d_offsets[u] .. d_offsets[u+1] (device int64
 * [n_seg+1], non-decreasing, [0] = 0, [n_seg] = F; NOT checked here -- the binding checks it on the host).  Per
 * utterance and bin, with c = (x*.5+.5)*(xmax-xmin)+xmin, mu_c / v_c its utterance mean / biased variance and
 * g = d_gv[bin] (the target speaker's mean utterance variance, etc/<spk>_gv.npf):
 *     d_sp = mu_c + sqrt(g / v_c) * (c - mu_c)   where v_c > 1e-8,
 *     d_sp = vaenpvc_tanhize_bwd's bytes           elsewhere (1-frame utterance, constant bin, xmax == xmin).
 * An utterance's output depends only on its own frames (bit for bit, whatever its offset or neighbours in the batch).
 * d_sp must not overlap d_x.  d_ws: >= vaenpvc_gv_workspace_bytes(F, n_seg, H) bytes, 16-byte aligned
 * (VAENPVC_E_WORKSPACE if shorter or NULL).  F >= 0, n_seg >= 1, H >= 1; F is not limited to 2^18 here. */
int64_t vaenpvc_gv_workspace_bytes(int64_t F, int32_t n_seg, int32_t H);
int vaenpvc_gv_postfilter(const float* d_x, const int64_t* d_offsets, int32_t n_seg, int64_t F, int32_t H,
                          const float* d_xmin, const float* d_xmax, const float* d_gv, float* d_sp,
                          void* d_ws, size_t ws_bytes, void* stream);

/* WORLD-style waveform synthesis (the reference's convert.py:105-114 -> analyzer.py:pw2wav -> pyworld.synthesize; pyworld
 * is a CPU C library this project does not have).  The algorithm is DESIGN.md section 14: WORLD's Synthesis() structure
 * (pulses from a float64 phase scan, minimum-phase periodic and aperiodic responses from 1024-point FFTs, overlap-add)
 * with documented deviations; sample-level equality with pyworld is not claimed.  n_seg utterances back to back:
 * utterance u is frames d_frame_offsets[u] .. [u+1] of d_f0 [F], d_sp [F,H] (log10, energy-normalised as in the .bin
 * files), d_en [F], d_ap [F,H], and samples d_sample_offsets[u] .. [u+1] of d_y [S] (float32), with
 * S_u = floor(T_u * frame_period_ms * fs / 1000) computed in float64 (pyworld's y_length).  Both offset arrays are device
 * int64 [n_seg+1], non-decreasing, [0] = 0, [n_seg] = F resp. S, every T_u >= 1; NOT checked here -- the binding checks
 * them on the host (a malformed array cannot make a kernel write outside d_y or d_ws).  The noise is the Philox draw of
 * vaenpvc_philox_normal (key `seed`, offset 0), element index counted from the utterance's first pulse.  Per-sample f0 is
 * capped at VAENPVC_SYNTH_F0_CEIL Hz, which bounds the pulses per utterance by floor(S_u * 1000 / fs) + 1; a pulse beyond
 * it is dropped.  An utterance's output depends only on its own frames and `seed` (bit for bit, whatever its offset or
 * neighbours in the batch).  H must be 513 (FFT size 1024), 8000 <= fs <= 48000, frame_period_ms finite and > 0; d_y must
 * not overlap an input.  d_ws: >= vaenpvc_synth_workspace_bytes(n_seg, S, H, fs) bytes, 16-byte aligned
 * (VAENPVC_E_WORKSPACE if shorter or NULL): about 4 KiB per pulse slot, (floor(S * 1000 / fs) + n_seg) slots. */
#define VAENPVC_SYNTH_F0_CEIL 1000
int64_t vaenpvc_synth_workspace_bytes(int32_t n_seg, int64_t S, int32_t H, int32_t fs);
int vaenpvc_synthesize(const float* d_f0, const float* d_sp, const float* d_en, const float* d_ap,
                       const int64_t* d_frame_offsets, const int64_t* d_sample_offsets, int32_t n_seg, int64_t F,
                       int64_t S, int32_t H, int32_t fs, double frame_period_ms, uint64_t seed, float* d_y, void* d_ws,
                       size_t ws_bytes, void* stream);

/* WORLD-style feature analysis (the reference's analyzer.py:25-47: librosa.load -> pyworld dio(f0_ceil = --f0_ceil) ->
 * stonemask -> cheaptrick(fft_size 1024) -> d4c, then en = sum(sp + 1e-10), sp = log10(sp / en); pyworld is a CPU C
 * library this project does not have).  The algorithm is DESIGN.md section 15 (DIO with 2 channels per octave, speed 1,
 * allowed range 0.1; StoneMask; CheapTrick q1 = -0.15; D4C threshold 0.85), restated by tests/world_analysis_ref.py;
 * sample-level equality with pyworld is not claimed.  n_seg utterances back to back: utterance u is samples
 * d_sample_offsets[u] .. [u+1] of d_x [S] (float32, librosa's int16 / 32768 scale) and frames d_frame_offsets[u] .. [u+1]
 * of the outputs, with T_u = (int)(1000 S_u / fs / frame_period_ms) + 1 computed in float64 (GetSamplesForDIO); frame i
 * is at i * frame_period_ms / 1000 s.  Both offset arrays are device int64 [n_seg+1], non-decreasing, [0] = 0,
 * [n_seg] = S resp. F, every S_u >= 1; NOT checked here -- the binding checks them on the host (a malformed array cannot
 * make a kernel write outside the outputs or d_ws).  Outputs, float32: d_f0 [F] (StoneMask's refined f0, 0 = unvoiced),
 * d_sp [F, 513] (log10(sp / en), the record form), d_ap [F, 513], d_en [F].  An utterance's outputs depend only on its own
 * samples (bit for bit, whatever its offset or neighbours in the batch).  Checked (VAENPVC_E_ARG): fs == 16000,
 * 71 <= f0_floor < f0_ceil <= 800, 1 <= frame_period_ms <= 50, n_seg >= 1, n_seg <= S <= INT32_MAX,
 * n_seg <= F <= (int)(1000 S / fs / frame_period_ms) + n_seg, no NULL pointer, no overlap of an output with an input,
 * another output or the workspace.  d_ws: >= vaenpvc_analysis_workspace_bytes(...) bytes (VAENPVC_E_WORKSPACE if
 * shorter or NULL), 256-byte aligned.  Its layout, every region starting at a 256-byte boundary in this order, with
 * nb = 1 + (int)(log2(f0_ceil / f0_floor) * 2) bands, NBS = S + n_seg band samples and NES = S / 2 + 2 n_seg edge slots:
 *   mean   double [n_seg]        mean of DIO's y = [x_u, 0] (S_u + 1 samples)
 *   taps   double [nb, 1281]     combined low-cut x band-pass filter of band b, offsets -(320 + L_b) .. (320 + L_b)
 *   band   double [nb, NBS]      band signal of utterance u at [b, soff[u] + u + i], i = 0 .. S_u
 *   edges  double [nb, 4, NES]   fine edges (negative-going, positive-going, peak, dip) of utterance u from slot
 *                                soff[u] / 2 + 2 u, in sample order
 *   ecnt   int32  [nb, 4, n_seg] the number of fine edges of each list
 *   cand   double [nb, F]        DIO candidate per band and frame (0: none)
 *   score  double [nb, F]        its score / (candidate + 1e-12)
 *   best   double [F]            the pre-fix contour (candidate of the best-scoring band)
 *   s1, s2 double [F]            FixF0Contour scratch
 *   f0d    double [F]            DIO's f0 (after FixF0Contour)
 *   f0r    double [F]            StoneMask's refined f0 (d_f0 is its float32 cast)
 *   ap0    double [F]            D4C LoveTrain's cumulative-power ratio (voiced when > 0.85)
 *   coarse double [F]            D4C's coarse aperiodicity in dB after the f0 revision (0 where D4C's body did not run)
 *   flags  int32  [F]            bit 0: StoneMask fell back to DIO's f0; bit 1: D4C's body ran */
int64_t vaenpvc_analysis_workspace_bytes(int32_t n_seg, int64_t S, int64_t F, int32_t fs, double frame_period_ms,
                                         double f0_floor, double f0_ceil);
int vaenpvc_analyze(const float* d_x, const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t n_seg,
                    int64_t S, int64_t F, int32_t fs, double frame_period_ms, double f0_floor, double f0_ceil,
                    float* d_f0, float* d_sp, float* d_ap, float* d_en, void* d_ws, size_t ws_bytes, void* stream);

/* Objective evaluation (not in the reference; evaluate.py): mel-cepstral distortion in dB between two utterances along
 * their dynamic-time-warping path, with the log-F0 error and the voicing mismatch on the same path.  The definition is
 * DESIGN.md section 16, restated by tests/mcd_ref.py.  Inputs per side are what a .bin record holds, float32: sp [F, 513]
 * = log10(sp / en), en [F] (> 0), f0 [F] (voiced when > 1).  All arithmetic is float64.
 *
 * vaenpvc_mcep_matrix (host only, no device work): fills host_W, double [(order + 1) x H] row-major, the fixed matrix with
 * mc[t] = W L[t] for the log amplitude L[t, k] = 0.5 (ln 10 sp[t, k] + ln en[t]): the one-sided real cepstrum of the
 * 1024-point symmetric extension of L, then SPTK's freqt recursion (all-pass constant alpha) from 513 coefficients to
 * order + 1, so that L(omega) ~ sum_m mc[m] cos(m w(omega)), w the all-pass phase.  VAENPVC_E_ARG unless H == 513,
 * 1 <= order <= VAENPVC_MCD_MAX_ORDER, 0 <= alpha < 1, host_W != NULL.  The caller uploads W for vaenpvc_mcd_dtw.
 *
 * vaenpvc_mcd_dtw: n_pair utterance pairs; pair p is frames d_offA[p] .. d_offA[p+1] of side A (Ta frames) and
 * d_offB[p] .. d_offB[p+1] of side B (Tb frames); both offset arrays are device int64 [n_pair + 1], non-decreasing,
 * [0] = 0, [n_pair] = Fa resp. Fb, every utterance 1 .. VAENPVC_MCD_MAX_FRAMES frames; cells = sum over pairs of
 * Ta * Tb.  The offsets are NOT checked on the host -- the binding does that; on the device a pair that breaks the
 * contract (or does not fit into `cells`) is skipped and its results are NaN, nothing is written out of bounds.
 *   local cost  d(i, j) = sqrt(sum_{m=1..order} (mcA[i, m] - mcB[j, m])^2)           (the gain mc[0] is left out)
 *   DTW         D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), D(0, 0) = d(0, 0), unit weights, no band; on
 *               equal values the predecessor is the diagonal, then (i-1, j), then (i, j-1)
 * d_results: double [n_pair, 8] = { mcd_db = (VAENPVC_MCD_DB_FACTOR * sum) / P,  P (path length),  D(Ta-1, Tb-1),
 * lf0_rmse = sqrt(mean((ln f0A - ln f0B)^2)) over the path cells where both frames are voiced (NaN if none),  the number
 * of those cells,  the number of path cells where exactly one frame is voiced,  sum = the sum of d over the path,  0 };
 * sums run in back-trace order, from (Ta-1, Tb-1) to (0, 0), one rounding per operation.
 * d_path (optional, NULL to skip): int32 [Fa + Fb, 2]; pair p's path starts at entry d_offA[p] + d_offB[p], P entries
 * (i, j) in back-trace order, first (Ta-1, Tb-1), last (0, 0); the rest of the pair's Ta + Tb entries is not written.
 * d_D (optional, NULL to skip): double [cells], the accumulated cost D in the layout of the `cost` region below.
 * A pair's results depend only on its own frames (bit for bit, whatever its place or neighbours in the call).
 * Checked (VAENPVC_E_ARG): 1 <= n_pair <= VAENPVC_MCD_MAX_PAIRS, n_pair <= Fa, Fb <= n_pair * VAENPVC_MCD_MAX_FRAMES,
 * max(Fa, Fb) <= cells <= min(Fa * Fb, n_pair * VAENPVC_MCD_MAX_FRAMES^2), 1 <= order <= VAENPVC_MCD_MAX_ORDER, no NULL
 * pointer besides the optional ones, no overlap of an output with an input, another output or the workspace.  d_ws:
 * >= vaenpvc_mcd_workspace_bytes(...) bytes (VAENPVC_E_WORKSPACE if shorter or NULL), 256-byte aligned.  Its layout,
 * every region starting at a 256-byte boundary in this order:
 *   mc     double [Fa + Fb, order + 1]  mel-cepstra, side A's frames first
 *   lf0    double [Fa + Fb]             ln f0 where f0 > 1, otherwise -1
 *   pinfo  int64  [n_pair + 1, 6]       per pair: first cell of its cost matrix, first tile, d_offA[p], d_offB[p], Ta, Tb
 *                                       (Ta = Tb = 0: skipped); row n_pair holds the totals
 *   cost   double [cells]               d, pair after pair (Ta * Tb cells each; element offsets are 64-bit); inside a pair
 *                                       anti-diagonal after anti-diagonal: s = i + j ascending, i ascending inside a
 *                                       diagonal, so the DP's lanes touch consecutive addresses.  With m = min(Ta, Tb),
 *                                       M = max(Ta, Tb) the cells before diagonal s number s (s + 1) / 2 for s <= m,
 *                                       m (m + 1) / 2 + (s - m) m for m <= s <= M, Ta Tb - r (r + 1) / 2 with
 *                                       r = Ta + Tb - 1 - s beyond; cell (i, j) follows at i - max(0, s - Tb + 1)
 *                                       (hipvae.metrics.diag_index)
 *   code   uint8  [cells]               predecessor of each cell, same layout: 0 diagonal, 1 (i-1, j), 2 (i, j-1) */
#define VAENPVC_MCD_MAX_FRAMES 4096
#define VAENPVC_MCD_MAX_ORDER 64
#define VAENPVC_MCD_MAX_PAIRS 65536
#define VAENPVC_MCD_DB_FACTOR 6.1418514637137541 /* 10 sqrt(2) / ln 10 */
int vaenpvc_mcep_matrix(int32_t order, double alpha, int32_t H, double* host_W);
int64_t vaenpvc_mcd_workspace_bytes(int32_t n_pair, int64_t Fa, int64_t Fb, int64_t cells, int32_t order);
int vaenpvc_mcd_dtw(const float* d_spA, const float* d_enA, const float* d_f0A, const int64_t* d_offA, int64_t Fa,
                    const float* d_spB, const float* d_enB, const float* d_f0B, const int64_t* d_offB, int64_t Fb,
                    int32_t n_pair, int64_t cells, const double* d_W, int32_t order, double* d_results,
                    int32_t* d_path, double* d_D, void* d_ws, size_t ws_bytes, void* stream);

/* Training-set statistics on the device (build.py --device; the host path of build.py is NumPy).  Both entries enqueue
 * on `stream`, allocate nothing, do not synchronise with the host and use no floating-point atomic (integer histogram
 * adds only): a call returns the same bytes every time.  DESIGN.md section 17; restated by tests/stats_ref.py.
 *
 * vaenpvc_column_select: exact per-column order statistics.  d_x is a float32 matrix of F rows and H columns with a row
 * stride of ld floats (ld >= H; a raw record buffer [F, 1029] is used in place with ld = 1029).  host_ranks: HOST array
 * of n_rank (1 .. VAENPVC_SELECT_MAX_RANKS) zero-based ranks in [0, F), in any order, duplicates allowed.
 * d_out[r * H + h] = np.sort(x[:, h])[host_ranks[r]]: an element of the column, no interpolation (-0.0 sorts just below
 * +0.0).  d_flag: device int32[1]; the call stores 0, then sets bit 0 if any element of the F x H window is NaN or
 * +-Inf; the outputs of such a column are then unspecified (every write stays in bounds).  Checked (VAENPVC_E_ARG): no
 * NULL pointer, 1 <= F <= 2^31 - 1 (an empty column has no order statistic), 1 <= H <= 2^21, H <= ld <= 2^24, n_rank
 * and every rank in range.  d_ws: >= vaenpvc_column_select_workspace_bytes(F, H, n_rank) bytes (VAENPVC_E_WORKSPACE if
 * shorter or NULL), 16-byte aligned.  Its layout, every region starting at a 256-byte boundary in this order:
 *   hist    uint32 [n_rank, H, 256]   digit counts of the current radix pass per (slot, column); zero on return
 *   prefix  uint32 [n_rank, H]        the selected element's order-preserving key (negative floats: every bit flipped,
 *                                     the others: the sign bit flipped)
 *   krem    uint32 [n_rank, H]        the rank among the elements that equal the selected one (0 .. ties - 1)
 *   lead    int32  [n_rank, H]        the lowest rank index that selected the same element in this column
 * The select reads d_x once for the first 8 key bits and once per further 8 bits and distinct prefix still alive:
 * between 4 and 1 + 3 n_rank passes.
 *
 * vaenpvc_speaker_stats: utterance u is rows d_offsets[u] .. d_offsets[u+1] (device int64 [n_seg+1], non-decreasing,
 * [0] = 0, [n_seg] = F) of d_sp (float32, F x H, row stride ld_sp >= H floats) and of d_f0 (float32, element stride
 * ld_f0 >= 1 floats); d_spk[u] (device int32 [n_seg]) is its speaker in [0, n_spk).  Neither array is checked here --
 * the binding does that; on the device offsets are clamped to [0, F] and an id outside [0, n_spk) belongs to no speaker,
 * so nothing is read or written out of bounds.  All arithmetic is float64, in orders that depend only on the lengths of
 * the speaker's utterances and their order:
 *   d_lf0   double [n_spk, 3]   (count, mean, population std) of ln f0 over the speaker's frames with f0 > 2 (strict);
 *                               count == 0: mean = std = NaN
 *   d_gv    double [n_spk, H]   per bin, the mean over the speaker's utterances of >= 2 frames of the utterance's
 *                               biased variance of sp (two passes); NaN where d_n_utt is 0
 *   d_n_utt int64  [n_spk]      the number of those utterances
 * A speaker's results are the same bytes wherever its utterances stand among the others'.  Checked (VAENPVC_E_ARG): no
 * NULL pointer, F >= 0, n_seg >= 1, n_spk >= 1, 1 <= H <= 2^21, H <= ld_sp <= 2^24, 1 <= ld_f0 <= 2^24.  d_ws: >=
 * vaenpvc_speaker_stats_workspace_bytes(F, n_seg, H) bytes (VAENPVC_E_WORKSPACE if shorter or NULL), 16-byte aligned:
 *   uvar    double [n_seg, H]   the utterance variances (rows of utterances under 2 frames are not written)
 *   ustat   double [n_seg, 3]   (count, mean, M2) of ln f0 per utterance */
#define VAENPVC_SELECT_MAX_RANKS 8
int64_t vaenpvc_column_select_workspace_bytes(int64_t F, int32_t H, int32_t n_rank);
int vaenpvc_column_select(const float* d_x, int64_t F, int32_t H, int64_t ld, const int64_t* host_ranks, int32_t n_rank,
                          float* d_out, int32_t* d_flag, void* d_ws, size_t ws_bytes, void* stream);
int64_t vaenpvc_speaker_stats_workspace_bytes(int64_t F, int32_t n_seg, int32_t H);
int vaenpvc_speaker_stats(const float* d_sp, int64_t ld_sp, const float* d_f0, int64_t ld_f0, const int64_t* d_offsets,
                          const int32_t* d_spk, int32_t n_seg, int32_t n_spk, int64_t F, int32_t H, double* d_lf0,
                          double* d_gv, int64_t* d_n_utt, void* d_ws, size_t ws_bytes, void* stream);

/* Band-limited resampling of the data path (analyzer.py --resample; the reference's analyzer.py:40 reads every wav with
 * librosa.load(sr=16000), which resamples; librosa is a CPU library this project does not have).  The definition is
 * DESIGN.md section 18, restated by tests/resample_ref.py; the constants are the ones resampy documents for its
 * `kaiser_best` filter, sample-level equality with librosa is not claimed.  Rates rate_in -> rate_out in Hz, g their gcd,
 * L = rate_out / g, M = rate_in / g, s = min(1, L / M), K = ceil(64 / s).  With the prototype, in input-sample time t,
 *   h(t) = s R sinc(s R t) I0(B sqrt(1 - v^2)) / I0(B),  v = s t / 64,  h = 0 where |v| >= 1,
 *   R = 0.9475937167399596, B = 14.769656459379492, sinc the normalised sinc,
 * a segment of n input samples gives (n L + M - 1) / M (integer division) output samples; output m of the segment sits
 * at u = m M / L input samples and is  y[m] = sum_{j = -K+1 .. K} x[floor(u) + j] h(frac(u) - j),  x zero outside the
 * segment, summed in float64 in ascending j and rounded once to float32.  frac(u) depends only on r = m mod L: the
 * weights are the table T, double [2K][L] row-major, T[j + K - 1][r] = h(((r M) mod L) / L - j).
 *
 * vaenpvc_resample_plan (host only, no device work): *up = L, *down = M, *half_taps = K.  VAENPVC_E_ARG unless
 * 1000 <= rate_in, rate_out <= 384000, rate_in != rate_out, no NULL pointer, the table has at most
 * VAENPVC_RESAMPLE_MAX_TABLE entries (2 K L <= 2^24) and a workgroup can stage the input window of one tile:
 * ceil(VAENPVC_RESAMPLE_TILE M / L) + 2 K <= VAENPVC_RESAMPLE_MAX_WINDOW samples.  (8000, 11025, 22050, 24000, 32000,
 * 44100, 48000 and 96000 -> 16000 are all inside.)
 *
 * vaenpvc_resample_filter (host only, no device work): fills host_table, double [2K][L], in float64; the only place the
 * weights are computed.  VAENPVC_E_ARG as for the plan, or when host_table is NULL.  The caller uploads it.
 *
 * vaenpvc_resample: n_seg segments back to back: segment u is samples d_in_offsets[u] .. [u+1] of d_x [S_in] (float32)
 * and outputs d_out_offsets[u] .. [u+1] of d_y [S_out] (float32), (n_u L + M - 1) / M of them.  Both offset arrays are
 * device int64 [n_seg+1], non-decreasing, [0] = 0, [n_seg] = S_in resp. S_out, every n_u >= 1; NOT checked here -- the
 * binding checks them on the host (on the device offsets are clamped to [0, S_in] resp. [0, S_out]: a malformed array
 * cannot make the kernel read or write out of bounds).  d_table: the device copy of T for this rate pair.  A segment's
 * outputs depend only on its own samples (bit for bit, whatever its offset or neighbours in the batch).  One workgroup
 * handles VAENPVC_RESAMPLE_TILE consecutive outputs of one segment.  Checked (VAENPVC_E_ARG): the plan's conditions, no
 * NULL pointer, 1 <= n_seg < 2^24, n_seg <= S_in <= INT32_MAX, n_seg <= S_out <= min(INT32_MAX,
 * (S_in L + M - 1) / M + n_seg), no overlap of d_y with d_x, d_table or an offset array.  No workspace: the call enqueues
 * one kernel on `stream`, allocates nothing, does not synchronise with the host and uses no atomic. */
#define VAENPVC_RESAMPLE_TILE 256
#define VAENPVC_RESAMPLE_MAX_TABLE (1 << 24)
#define VAENPVC_RESAMPLE_MAX_WINDOW 8192
int vaenpvc_resample_plan(int32_t rate_in, int32_t rate_out, int32_t* up, int32_t* down, int32_t* half_taps);
int vaenpvc_resample_filter(int32_t rate_in, int32_t rate_out, double* host_table);
int vaenpvc_resample(const float* d_x, const int64_t* d_in_offsets, const int64_t* d_out_offsets, int32_t n_seg,
                     int64_t S_in, int64_t S_out, int32_t rate_in, int32_t rate_out, const double* d_table, float* d_y,
                     void* stream);

/* analyzer.read record slicing (analyzer.py:113-127): rows of `rec_floats` float32
 * (1029) -> x = Tanhize(row[0:H]) and y = int64(row[rec_floats-1]) (bit-exact cast). */
int vaenpvc_unpack_records(const float* d_records, int64_t F, int32_t rec_floats, int32_t H,
                           const float* d_xmin, const float* d_xmax, float* d_x, int64_t* d_y,
                           void* stream);
/* The shuffle_batch dequeue of analyzer.py:128-135 fused with the slicing: output row f is
 * built from record d_index[f] (int64, 0 <= d_index[f] < n_records; checked on the host side
 * of the binding, not here) of the HBM-resident record store. */
int vaenpvc_gather_unpack_records(const float* d_records, int64_t n_records, const int64_t* d_index,
                                  int64_t F, int32_t rec_floats, int32_t H, const float* d_xmin,
                                  const float* d_xmax, float* d_x, int64_t* d_y, void* stream);

/* Speaker ids index the embedding table (model/vae.py:89): TensorFlow raises on an id outside
 * [0, y_dim) on the CPU.  Here the kernels clamp ids (no out-of-bounds access) and this check
 * reports them: synchronises `stream`, returns VAENPVC_E_ARG if any d_y[f] is out of range.
 * d_flag: int32[1] device scratch. */
int vaenpvc_validate_ids(const vaenpvc_ctx* ctx, const int64_t* d_y, int64_t F, int32_t* d_flag,
                         void* stream);

/* tf.summary.histogram payload (model/vae.py:132-136: histograms of x and xh): d_stats =
 * double[4] {min, max, sum, sum of squares}, d_counts = uint64[n_edges + 1] with bucket b
 * counting d_edges[b-1] <= v < d_edges[b] (d_edges ascending float32, n_edges <= 2048).
 * Both outputs are ACCUMULATED into: the caller initialises them ({+inf, -inf, 0, 0}, zeros). */
int vaenpvc_summary(const float* d_data, int64_t n, const float* d_edges, int32_t n_edges,
                    double* d_stats, uint64_t* d_counts, void* stream);

/* Developer hooks (per-step kernel selection masks, the single-kernel event timer) are declared in
 * vaenpvc_debug.h: they are exported by the same library but are not part of the boundary a maintainer binds. */

#ifdef __cplusplus
}
#endif
#endif /* VAENPVC_H_ */
