// kernels.h -- host-callable launchers shared between the ABI layer and the kernel
// translation units.  Everything enqueues on `stream`; nothing synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vaenpvc_debug.h"   // vaenpvc_sel_bit: names of the selection-mask bits
#include "model.h"
#include "philox.h"
#include "runtime.h"

namespace vaenpvc {

struct Ws {  // resolved workspace pointers (see workspace_layout)
  float* enc_a[VAENPVC_MAX_LAYERS];
  float* enc_st[VAENPVC_MAX_LAYERS];
  float *z_mu, *z_lv, *z, *h;
  float* eps;  // N(0,1) draw of the sampler when it is generated on the device (seeded entry points)
  float* dec_a[VAENPVC_MAX_LAYERS];
  float* dec_st[VAENPVC_MAX_LAYERS];
  float *xh, *kl_f, *nll_f;
  float* dec_y;  // lrelu(LN(dec_a[n_dec-2]))
  // train only
  float* d_xh;
  float* d_dec_a[VAENPVC_MAX_LAYERS];   // d_dec_a[0] is BORROWED from the fused loss kernel to the start of the backward pass (loss_fwd_post parks
                                        // the edge-term parts of the last layer's weight gradient there; k_sum_parts_add consumes them before
                                        // anything writes d(a0)); valid while Runtime::dxh_post_F == F
  float *d_h, *d_z, *d_e, *d_z_mu, *d_z_lv;
  float* d_enc_a[VAENPVC_MAX_LAYERS];
  float* dy_tmp;   // gradient hand-over buffer of the layered backward pass; BORROWED the same way: column 512 of the last layer's
                   // input gradient waits here from the fused loss kernel until dec3_dgrad has written the other 512 columns
  float *pl_y3, *pl_y4, *pl_z, *pl_dz, *pl_dh, *pl_da4;
  float* cl[12];  // channel-last planes of the conv view GEMMs (cl_layout.h: CL_*)
  float* toep_gp;  // bf16 planes of d_xh
  float* toep_yp;  // bf16 planes of dec_y
  float* scratch;
  int64_t scratch_floats;
  float* frame_pk;   // packed weight copies of the small-batch frame kernels (gfx950_frame.h: Pk)
  float* frame_lnp;  // per-frame channel sums of their LayerNorm backward
  float* frame_y;    // activated layer outputs [F][12000] for their weight-gradient launch (train mode)
};

// sets the thread-local message vaenpvc_last_error() returns; returns `code` (abi.hip)
int abi_error(int code, const char* msg);

// ---- single-kernel event timer (state in the context's Runtime, runtime.h) --------
#define VAENPVC_TIMED(tag, stream, ...)               \
  do {                                                \
    ::vaenpvc::Runtime& _rt = ::vaenpvc::rt();        \
    bool _tm = _rt.timer_match(tag);                  \
    if (_tm) _rt.timer_begin(stream);                 \
    __VA_ARGS__;                                      \
    if (_tm) _rt.timer_end(stream);                   \
  } while (0)

// ---- geometry-generic HIP kernels (generic_kernels.hip) -------------------------
namespace generic {
void encoder_fwd(const Model& m, const float* P, const float* x, int64_t F, const Ws& w, hipStream_t s);
// z = z_mu + eps*sqrt(exp(z_lv)) (eps may be null -> z = z_mu); also per-frame KL
// (key != nullptr: eps is drawn on the device with Philox and stored in w.eps for the backward pass)
void reparam_fwd(const Model& m, const float* eps, const PhiloxKey* key, int64_t F, const Ws& w, hipStream_t s);
// decoder from z (w.z or external) and y -> xh_out
void decoder_fwd(const Model& m, const float* P, const float* z, const int64_t* y, int64_t F, const Ws& w,
                 float* xh_out, hipStream_t s);
// per-frame log-density, optional d_xh, then {G, D_KL, logP}
void loss_fwd(const Model& m, const float* x, int64_t F, const Ws& w, bool want_grad, float* loss3, hipStream_t s);
void loss_reduce(int64_t F, const Ws& w, float* loss3, hipStream_t s);   // batch means of kl_f / nll_f -> {G, D_KL, logP}
void backward(const Model& m, const float* P, const float* x, const int64_t* y, const float* eps, int64_t F,
              const Ws& w, float* G, hipStream_t s);
// per-step entry points (the tuned path can fall back to any of them, per layer)
void enc_layer_fwd(const Model& m, const float* P, const float* x, int64_t F, const Ws& w, hipStream_t s, int i);
void heads_fwd(const Model& m, const float* P, int64_t F, const Ws& w, hipStream_t s);
void merge_fwd(const Model& m, const float* P, const float* z, const int64_t* y, int64_t F, const Ws& w, hipStream_t s);
void dec_layer_fwd(const Model& m, const float* P, int64_t F, const Ws& w, float* xh_out, hipStream_t s, int i);
void bias_grad(const float* d, float* db, int64_t F, int C, int H, hipStream_t s);
void bwd_dec_layer(const Model& m, const float* P, int64_t F, const Ws& w, float* G, hipStream_t s, int i);
void bwd_merge(const Model& m, const float* P, const int64_t* y, int64_t F, const Ws& w, float* G, hipStream_t s);
void bwd_reparam(const Model& m, const float* eps, int64_t F, const Ws& w, hipStream_t s);
void bwd_heads(const Model& m, const float* P, int64_t F, const Ws& w, float* G, hipStream_t s);
void bwd_enc_layer(const Model& m, const float* P, const float* x, int64_t F, const Ws& w, float* G, hipStream_t s, int i);
}  // namespace generic

// ---- elementwise / optimiser kernels (misc_kernels.hip) -------------------------
void launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float b1, float b2,
                 float eps, float gscale, hipStream_t s);
void launch_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, int64_t* d_step, float lr, float b1,
                     float b2, float eps, float gscale, hipStream_t s);
void launch_tanhize(const float* in, const float* xmin, const float* xmax, float* out, int64_t F, int H,
                    bool forward, hipStream_t s);
// rows gathered through `idx` (int64 record numbers) when it is not null
void launch_unpack(const float* rec, const int64_t* idx, int64_t F, int rec_floats, int H, const float* xmin,
                   const float* xmax, float* x, int64_t* y, hipStream_t s);
void launch_check_ids(const int64_t* y, int64_t F, int ny, int* flag, hipStream_t s);
void launch_philox_normal(float* out, int64_t n, PhiloxKey key, hipStream_t s);
void launch_philox_uniform(float* out, int64_t n, PhiloxKey key, hipStream_t s);
// min, max, sum, sum of squares (double[4]) and counts per bucket (uint64[n_edges + 1]; bucket b holds
// edges[b-1] <= v < edges[b]) of `n` floats; the outputs must be zeroed by the caller (stats[0..1] = +-inf)
void launch_summary(const float* d, int64_t n, const float* edges, int n_edges, double* stats, unsigned long long* counts,
                    hipStream_t s);

// ---- global-variance post-filter of the conversion path (gfx950_gv.hip) ----------
// workgroups of the per-chunk launches, and workspace bytes: (x0, mean, M2) per chunk and bin + the per-bin map per utterance
int64_t gv_chunk_grid(int64_t F, int n_seg);
int64_t gv_workspace_bytes(int64_t F, int n_seg, int H);
void launch_gv_postfilter(const float* x, const int64_t* off, int n_seg, int64_t F, int H, const float* xmin,
                          const float* xmax, const float* gv, float* out, void* ws, hipStream_t s);

// ---- WORLD-style synthesis of the conversion path (gfx950_synth.hip) -------------
// pulse slots (floor(S*1000/fs) + n_seg) and workspace bytes: counts, their prefix, per slot (sample, shift + voicing,
// 4 KiB segment)
int64_t synth_slots(int n_seg, int64_t S, int fs);
int64_t synth_workspace_bytes(int n_seg, int64_t S, int fs);
void launch_synthesize(const float* f0, const float* sp, const float* en, const float* ap, const int64_t* foff,
                       const int64_t* soff, int n_seg, int64_t F, int64_t S, int fs, double frame_period_ms,
                       uint64_t seed, float* y, void* ws, hipStream_t s);

// ---- WORLD-style feature analysis of the data path (gfx950_analysis.hip) ---------
// workspace regions (include/vaenpvc.h documents the layout, 256-byte aligned, in this order)
struct AnalysisWs {
  double* mean;     // [n_seg]
  double* taps;     // [nb, analysis_taps()]
  double* band;     // [nb, S + n_seg]
  double* edges;    // [nb, 4, S / 2 + 2 n_seg]
  int32_t* ecnt;    // [nb, 4, n_seg]
  double *cand, *score;  // [nb, F]
  double *best, *s1, *s2, *f0d, *f0r, *ap0, *coarse;  // [F]
  int32_t* flags;   // [F]
  int64_t bytes;
};
AnalysisWs analysis_carve(void* ws, int n_seg, int64_t S, int64_t F, int nb);
int analysis_taps();
int64_t analysis_workspace_bytes(int n_seg, int64_t S, int64_t F, int nb);
void launch_analyze(const float* x, const int64_t* soff, const int64_t* foff, int n_seg, int64_t S, int64_t F, int fs,
                    double frame_period_ms, double f0_floor, double f0_ceil, int nb, float* f0, float* sp, float* ap,
                    float* en, void* ws, hipStream_t s);

// ---- DTW-aligned mel-cepstral distortion (gfx950_dtw.hip) ----
constexpr int MCD_MAX_FRAMES = 4096;                     // per utterance and side (= VAENPVC_MCD_MAX_FRAMES)
constexpr double MCD_DB_FACTOR = 6.1418514637137541;     // 10 sqrt(2) / ln 10 (= VAENPVC_MCD_DB_FACTOR)
struct McdWs {      // the regions of include/vaenpvc.h, in this order, each 256-byte aligned
  double* mc;           // [Fa + Fb, order + 1]
  double* lf0;          // [Fa + Fb]
  int64_t* pinfo;       // [n_pair + 1, 6]
  double* cost;         // [cells]
  unsigned char* code;  // [cells]
  int64_t bytes;
};
McdWs mcd_carve(void* ws, int n_pair, int64_t Fa, int64_t Fb, int64_t cells, int order);
int64_t mcd_workspace_bytes(int n_pair, int64_t Fa, int64_t Fb, int64_t cells, int order);
void mcep_matrix_host(int order, double alpha, double* W);      // host only: W [(order + 1) x 513]
void launch_mcd_dtw(const float* spA, const float* enA, const float* f0A, const int64_t* offA, int64_t Fa,
                    const float* spB, const float* enB, const float* f0B, const int64_t* offB, int64_t Fb, int n_pair,
                    int64_t cells, const double* W, int order, double* results, int32_t* path, double* D, void* ws,
                    hipStream_t s);

// ---- training-set statistics of build.py --device (gfx950_stats.hip) ----
constexpr int SEL_MAX_RANKS = 8;        // = VAENPVC_SELECT_MAX_RANKS
constexpr int64_t SEL_MAX_LD = 1 << 24;  // row stride in floats: the histogram kernel's in-slice offsets stay 32-bit
constexpr int SEL_MAX_H = 1 << 21;      // 64-column groups fit the grid's y dimension
int64_t column_select_workspace_bytes(int H, int n_rank);
void launch_column_select(const float* x, int64_t F, int H, int64_t ld, const int64_t* ranks, int n_rank, float* out,
                          int32_t* flag, void* ws, hipStream_t s);
int64_t speaker_stats_workspace_bytes(int n_seg, int H);
void launch_speaker_stats(const float* sp, int64_t ld_sp, const float* f0, int64_t ld_f0, const int64_t* off,
                          const int32_t* spk, int n_seg, int n_spk, int64_t F, int H, double* lf0, double* gv,
                          int64_t* n_utt, void* ws, hipStream_t s);

// ---- band-limited resampling of analyzer.py --resample (gfx950_resample.hip) ----
// host only: L = rate_out / gcd, M = rate_in / gcd, K = ceil(64 / min(1, L / M)); false when the pair is outside the
// limits of include/vaenpvc.h
bool resample_plan_host(int rate_in, int rate_out, int* up, int* down, int* half_taps);
void resample_filter_host(int L, int M, int K, double* T);      // host only: T [2K][L]
void launch_resample(const float* x, const int64_t* ioff, const int64_t* ooff, int n_seg, int64_t S_in, int64_t S_out,
                     int L, int M, int K, const double* T, float* y, hipStream_t s);

// ---- tuned gfx950 kernels for the VCC2016 geometry (gfx950_*.hip) ----------------
namespace tuned {
// step masks: bit set = use the tuned kernel for that step, clear = generic kernel.
//   forward  bits: 0..4 encoder conv i | 5 heads | 6 merge | 7..10 decoder layer i
//   backward bits: 0..4 encoder conv i | 5 heads | 6 merge | 7..10 decoder layer i
bool available();
void encoder_fwd(const Model& m, const float* P, const float* x, int64_t F, const Ws& w, hipStream_t s);
// `weights_packed`: the packed weight copies in w.scratch are already current (the encoder of the
// same step built them); a stand-alone decode call packs them itself.
void decoder_fwd(const Model& m, const float* P, const float* z, const int64_t* y, int64_t F, const Ws& w,
                 float* xh_out, hipStream_t s, bool weights_packed = false);
void backward(const Model& m, const float* P, const float* x, const int64_t* y, const float* eps, int64_t F,
              const Ws& w, float* G, hipStream_t s);
// the loss of a train step fused with the first pass of the backward over d(xh) (planes of d(xh), column 512 of the last layer's
// input gradient, bias-gradient parts): true = done, the backward pass that follows picks the results up (Runtime::dxh_post_F);
// false = not selected at this batch size / precision / masks, the caller runs generic::loss_fwd
// sampler + KL writing z also as the planes of the merge GEMM (true = done: the decoder_fwd that follows on w.z skips its split pass,
// Runtime::plz_F; false = not selected, the caller runs generic::reparam_fwd)
bool reparam_fwd_planes(const Model& m, const float* eps, const PhiloxKey* key, int64_t F, const Ws& w, hipStream_t s);
bool loss_fwd_post(const Model& m, const float* P, const float* x, int64_t F, const Ws& w, float* loss3, hipStream_t s);
// ---- small-batch path: whole frames per workgroup (gfx950_frame.hip)
constexpr int FRAME_ENC = 1, FRAME_SAMPLE = 2, FRAME_DEC = 4, FRAME_LOSS = 8, FRAME_GRAD = 16;   // = frame::FM_*
constexpr int64_t FRAME_CAP = 1024;          // largest batch the workspace reserves its per-frame sums for
int64_t frame_pack_floats();
int64_t frame_lnp_floats(int64_t F);
bool frame_fwd_on(int64_t F);
bool frame_bwd_on(int64_t F);
// packed weight copies; G_zero / zero2 (nullable): buffers zero-filled by the same launch
void frame_pack(const Model& m, const float* P, const Ws& w, float* G_zero, float* zero2, int nzero2, hipStream_t s, bool zero_only = false);
// scratch region the small-batch backward wants zeroed before it runs (per-speaker sums of the merge backward)
float* frame_zero_region(const Ws& w, int* count);
void frame_forward(const Model& m, const float* P, const float* x, const float* target, const int64_t* y, const float* eps,
                   const PhiloxKey* key, const float* z_in, int64_t F, const Ws& w, float* xh_out, int mode, float* loss3,
                   hipStream_t s);
// input-gradient chain + LayerNorm parameter / conv-bias gradients (the weight gradients are the caller's)
// (lnp_sums: also launch the reduction of the LayerNorm parameter / conv-bias sums; false when frame_wgrad follows)
// (loss3: where the batch means go when the step's forward pass left them to the backward half -- the split train step,
//  gfx950_frame.hip: frame_split_on; null: nobody wants them)
void frame_backward(const Model& m, const float* P, const float* target, const float* eps, int64_t F, const Ws& w, float* G,
                    hipStream_t s, bool lnp_sums, float* loss3 = nullptr);
bool frame_split_on(const Ws& w, int64_t F);
// every parameter gradient in one launch (gfx950_frame_wgrad.h); G must have been zero-filled
void frame_wgrad(const Model& m, const float* P, const float* x, const int64_t* y, int64_t F, const Ws& w, float* G, hipStream_t s);
// the whole backward pass of a small batch: frame_backward + every weight gradient (gfx950_layers.hip)
// (g_zeroed: the gradient buffer and frame_zero_region were zero-filled by this step's frame_pack)
void backward_frame(const Model& m, const float* P, const float* x, const float* target, const int64_t* y, const float* eps,
                    int64_t F, const Ws& w, float* G, hipStream_t s, bool g_zeroed, float* loss3 = nullptr);
}  // namespace tuned

}  // namespace vaenpvc
