/*
 * vaenpvc_debug.h -- developer hooks of libvaenpvc_hip.so (no reference counterpart).
 *
 * NOT part of the drop-in boundary (include/vaenpvc.h): a maintainer binding the ConvVAE path needs none of
 * this.  The parity tests use the selection masks to pin every kernel family against the float64 oracle at
 * small batch sizes, bench.py uses the timer to report the duration of one kernel site.  The bit assignments
 * below are per-round tuning state and may change without an ABI version bump.
 */
#ifndef VAENPVC_DEBUG_H_
#define VAENPVC_DEBUG_H_

#include "vaenpvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bits of the two kernel-selection masks (vaenpvc_set_tuned_masks): one mask for the forward steps, one for the backward
 * steps, default all ones, state of THIS context.  A cleared bit moves that step of that pass off the measured default;
 * the *_MIN_FRAMES bits exist for the parity tests, which pin every kernel family at small batch sizes. */
enum vaenpvc_sel_bit {
  VAENPVC_SEL_ENC0 = 0,                 /* 0..10, one bit per step: cleared = the geometry-generic kernel instead of the tuned gfx950 one */
  VAENPVC_SEL_ENC1 = 1,
  VAENPVC_SEL_ENC2 = 2,
  VAENPVC_SEL_ENC3 = 3,
  VAENPVC_SEL_ENC4 = 4,
  VAENPVC_SEL_HEADS = 5,
  VAENPVC_SEL_MERGE = 6,
  VAENPVC_SEL_DEC0 = 7,
  VAENPVC_SEL_DEC1 = 8,
  VAENPVC_SEL_DEC2 = 9,
  VAENPVC_SEL_DEC3 = 10,
  VAENPVC_SEL_FBWD_MIN_FRAMES = 14,     /* backward: cleared = the one-kernel backward steps at any batch size (from 1 024 frames on otherwise) */
  VAENPVC_SEL_FBWD = 15,                /* backward: cleared = the thin layers' backward steps (decoder 2 and 1, encoder 1; VAENPVC_FB_LAYERS) as three
                                           kernels each instead of ONE kernel per layer (csrc/gfx950_fbwd.h) */
  VAENPVC_SEL_TN_W4 = 16,               /* backward: cleared = dense-shaped weight gradients with many tiles per row chunk (encoder layer 4) on
                                           k_gemm_tn instead of the four-wave k_gemm_tn4 */
  VAENPVC_SEL_TAP_WGRAD_W4 = 17,        /* backward: cleared = the 1025-tap layer's weight gradient on the eight-wave kernel (k_toep_wgrad_bf16_k32) at
                                           every batch size instead of the four-wave one (k_toep_wgrad_bf16_w4) from 4 096 frames on */
  VAENPVC_SEL_FRAME_SPLIT = 18,         /* backward: cleared = a small-batch train step keeps the 1025-tap layer inside the two frame kernels */
  VAENPVC_SEL_ENC0_FUSED_BWD = 19,      /* backward: cleared = encoder layer 0's LayerNorm backward and weight gradient as two passes instead of
                                           k_enc0_bwd_wave (from 1 024 frames on) */
  VAENPVC_SEL_FRAME_WGRAD = 20,         /* backward: cleared = behind the frame kernels, the layered weight-gradient kernels on two streams instead of
                                           the one-launch job list (csrc/gfx950_frame_wgrad.h) */
  VAENPVC_SEL_FRAME = 21,               /* cleared = never the small-batch frame kernels (csrc/gfx950_frame.h; selected up to VAENPVC_FRAME_MAX = 512
                                           frames per call); a train step uses them for both passes or for neither */
  VAENPVC_SEL_FCONV_R_MIN_FRAMES = 22,  /* cleared = every medium conv site on the register-weight fused kernel (csrc/gfx950_fconv_r.h) at any batch size */
  VAENPVC_SEL_ENC0_WAVE_MIN_FRAMES = 23, /* cleared = encoder layer 0 on its wave-per-frame kernels at any batch size */
  VAENPVC_SEL_FWGRAD_MIN_FRAMES = 24,   /* backward: cleared = every thin weight gradient on the fused kernel (csrc/gfx950_fwgrad.h) at any batch size */
  VAENPVC_SEL_FCONV_MIN_FRAMES = 25,    /* cleared = every thin conv site on the fused kernel (csrc/gfx950_fconv.h) at any batch size */
  VAENPVC_SEL_CV_SITE_SET = 26,         /* cleared = EVERY conv site of encoder layers 1-3 / decoder layers 0-2 on the view GEMMs instead of the
                                           measured per-precision site set */
  VAENPVC_SEL_VIEW_GEMM = 27,           /* cleared = no conv site on the view-GEMM kernels (csrc/gfx950_viewconv.h) */
  VAENPVC_SEL_PLANE_GEMM_MIN_FRAMES = 28, /* cleared = the plane GEMM and view-GEMM kernels at any batch size (from 1 024 frames on otherwise) */
  VAENPVC_SEL_PLANE_GEMM = 29,          /* cleared = heads, merge and encoder layer 4 on the exact-fp32 MFMA kernels instead of the bf16-split plane GEMMs */
  VAENPVC_SEL_TOEP_MIN_FRAMES = 30,     /* forward: cleared = the bf16-split kernels of the last decoder layer at any batch size (from 16 frames on otherwise) */
  VAENPVC_SEL_WGRAD_STREAM = 30         /* backward: cleared = the weight-gradient kernels on the caller's stream instead of the context's helper
                                           stream (serialised kernels; bench.py times single kernels this way) */
};
/* Debug/validation hook (no reference counterpart): sets both masks of a context that runs in VAENPVC_IMPL_AUTO on the
 * VCC2016 geometry.
 * vaenpvc_timer_select accepts a comma-separated LIST of site tags (a kernel group timed in one pass: bench.py's roofline.sites). */
int vaenpvc_set_tuned_masks(vaenpvc_ctx* ctx, uint32_t fwd_mask, uint32_t bwd_mask);

/* Measurement hook (no reference counterpart): brackets every launch of ONE tagged
 * kernel with a hipEvent pair on the launch stream, so bench.py can report that
 * kernel's average duration over the timed region.  Tags are the kernel-site names
 * listed in DESIGN.md (e.g. "dec3_fwd").  NULL or "" disables.  State of THIS context. */
int vaenpvc_timer_select(vaenpvc_ctx* ctx, const char* tag);
/* Synchronises the recorded events (blocks the host), returns the summed milliseconds and the
 * number of launches since the last read, and resets the accumulator. */
int vaenpvc_timer_read(vaenpvc_ctx* ctx, double* total_ms, int64_t* launches);

/* Process-wide developer switches of the small-batch path (scripts/frame_prof.py, scripts/wgrad_prof.py):
 * per-phase shader clocks of the two frame kernels (environment VAENPVC_FRAME_PROF=1 selects the instrumented
 * instantiations; copies 1024 counters, returns 0 or -1 when profiling is off); a bit set of the job-list segments of
 * the one-launch weight gradient to leave in the launch; the most frame chunks of its nine chunked jobs (NULL = defaults). */
int vaenpvc_debug_frame_prof(long long* out1024);
void vaenpvc_debug_wg_segments(unsigned mask);
void vaenpvc_debug_wg_caps(const int* caps9);

#ifdef __cplusplus
}
#endif
#endif /* VAENPVC_DEBUG_H_ */
