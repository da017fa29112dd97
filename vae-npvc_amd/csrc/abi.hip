// abi.hip -- the extern "C" surface declared in include/vaenpvc.h (+ the developer hooks of include/vaenpvc_debug.h).
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "../../include/vaenpvc_debug.h"
#include "kernels.h"

using namespace vaenpvc;

typedef std::pair<std::vector<Region>, int64_t> Layout;
struct vaenpvc_ctx {
  Model m;
  int impl = VAENPVC_IMPL_AUTO;
  Runtime rt;                // every piece of mutable state besides the layout cache (runtime.h)
  std::recursive_mutex mu;   // taken by every entry point that receives the context
  std::map<std::pair<int64_t, int>, std::shared_ptr<const Layout>> ws_cache;
};
// lock + bind the context's Runtime to this thread for the duration of an entry point
struct Call {
  std::lock_guard<std::recursive_mutex> lk;
  RtScope sc;
  explicit Call(vaenpvc_ctx* c, bool launches = true) : lk(c->mu), sc(&c->rt) {
    if (launches) c->rt.bind_device();
  }
};

static thread_local char g_err[512] = "";
static int fail(int code, const char* f, ...) {
  va_list ap;
  va_start(ap, f);
  vsnprintf(g_err, sizeof g_err, f, ap);
  va_end(ap);
  return code;
}

namespace vaenpvc {
int abi_error(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace vaenpvc

// shared ownership: a layout handed out stays valid even if the cache is trimmed meanwhile
static std::shared_ptr<const Layout> layout_of(vaenpvc_ctx* c, int64_t F, int mode) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  auto key = std::make_pair(F, mode);
  auto it = c->ws_cache.find(key);
  if (it == c->ws_cache.end()) {
    if (c->ws_cache.size() > 64) c->ws_cache.clear();
    int64_t total = 0;
    auto regs = workspace_layout(c->m, F, mode, &total);
    it = c->ws_cache.emplace(key, std::make_shared<const Layout>(std::move(regs), total)).first;
  }
  return it->second;
}

static int resolve(vaenpvc_ctx* c, int64_t F, int mode, void* d_ws, size_t ws_bytes, Ws* w) {
  if (F < 1) return fail(VAENPVC_E_ARG, "F must be >= 1 (got %lld)", (long long)F);
  if (F > (1LL << 18)) return fail(VAENPVC_E_ARG, "F too large (%lld > 262144 frames per call)", (long long)F);
  const auto layp = layout_of(c, F, mode);
  const Layout& lay = *layp;
  if (d_ws == nullptr || ws_bytes < (size_t)lay.second * 4)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)lay.second * 4,
                (long long)ws_bytes);
  if (((uintptr_t)d_ws & 15) != 0) return fail(VAENPVC_E_ARG, "workspace must be 16-byte aligned");
  float* base = (float*)d_ws;
  memset(w, 0, sizeof *w);
  for (const Region& r : lay.first) {
    float* p = base + r.offset;
    const std::string& n = r.name;
    auto idx = [&](size_t pre) { return atoi(n.c_str() + pre); };
    if (n.rfind("enc_a", 0) == 0) w->enc_a[idx(5)] = p;
    else if (n.rfind("enc_st", 0) == 0) w->enc_st[idx(6)] = p;
    else if (n.rfind("dec_a", 0) == 0) w->dec_a[idx(5)] = p;
    else if (n.rfind("dec_st", 0) == 0) w->dec_st[idx(6)] = p;
    else if (n.rfind("d_enc_a", 0) == 0) w->d_enc_a[idx(7)] = p;
    else if (n.rfind("d_dec_a", 0) == 0) w->d_dec_a[idx(7)] = p;
    else if (n == "z_mu") w->z_mu = p;
    else if (n == "z_lv") w->z_lv = p;
    else if (n == "z") w->z = p;
    else if (n == "eps") w->eps = p;
    else if (n == "h") w->h = p;
    else if (n == "xh") w->xh = p;
    else if (n == "dec_y") w->dec_y = p;
    else if (n == "kl_f") w->kl_f = p;
    else if (n == "nll_f") w->nll_f = p;
    else if (n == "d_xh") w->d_xh = p;
    else if (n == "d_h") w->d_h = p;
    else if (n == "d_z") w->d_z = p;
    else if (n == "d_e") w->d_e = p;
    else if (n == "d_z_mu") w->d_z_mu = p;
    else if (n == "d_z_lv") w->d_z_lv = p;
    else if (n == "dy_tmp") w->dy_tmp = p;
    else if (n == "toep_gp") w->toep_gp = p;
    else if (n.rfind("cl", 0) == 0) w->cl[idx(2)] = p;
    else if (n == "pl_y3") w->pl_y3 = p;
    else if (n == "pl_y4") w->pl_y4 = p;
    else if (n == "pl_z") w->pl_z = p;
    else if (n == "pl_dz") w->pl_dz = p;
    else if (n == "pl_dh") w->pl_dh = p;
    else if (n == "pl_da4") w->pl_da4 = p;
    else if (n == "toep_yp") w->toep_yp = p;
    else if (n == "scratch") { w->scratch = p; w->scratch_floats = r.count; }
    else if (n == "frame_pk") w->frame_pk = p;
    else if (n == "frame_lnp") w->frame_lnp = p;
    else if (n == "frame_y") w->frame_y = p;
  }
  return 0;
}

static int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(VAENPVC_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

static bool use_tuned(const vaenpvc_ctx* c) {
  return c->impl == VAENPVC_IMPL_AUTO && c->m.is_vcc2016 && tuned::available();
}

extern "C" {

int vaenpvc_set_tuned_masks(vaenpvc_ctx* ctx, uint32_t fwd_mask, uint32_t bwd_mask) {
  if (!ctx) return fail(VAENPVC_E_ARG, "null context");
  Call call(ctx, false);
  ctx->rt.fwd_mask = fwd_mask;
  ctx->rt.bwd_mask = bwd_mask;
  return 0;
}

int vaenpvc_set_precision(vaenpvc_ctx* ctx, int planes) {
  if (!ctx || planes < 1 || planes > 3) return fail(VAENPVC_E_ARG, "precision must be 1, 2 or 3 bf16 terms");
  Call call(ctx, false);
  ctx->rt.planes = planes;
  return 0;
}
int vaenpvc_get_precision(const vaenpvc_ctx* ctx) { return ctx ? ctx->rt.planes : VAENPVC_E_ARG; }

int vaenpvc_set_d0w_factor(vaenpvc_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return fail(VAENPVC_E_ARG, "d0w factor mode must be 0, 1 or 2");
  Call call(ctx, false);
  ctx->rt.d0w_factor = mode;
  return 0;
}
int vaenpvc_get_d0w_route(const vaenpvc_ctx* ctx) { return ctx ? ctx->rt.d0w_route : VAENPVC_E_ARG; }

int vaenpvc_set_bucket_callback(vaenpvc_ctx* ctx, vaenpvc_bucket_cb cb, void* user) {
  if (!ctx) return fail(VAENPVC_E_ARG, "null context");
  Call call(ctx, false);
  ctx->rt.bucket_cb = cb;
  ctx->rt.bucket_user = user;
  return 0;
}

int vaenpvc_timer_select(vaenpvc_ctx* ctx, const char* tag) {
  if (!ctx) return fail(VAENPVC_E_ARG, "null context");
  Call call(ctx, false);
  ctx->rt.tag = tag ? tag : "";
  ctx->rt.used = 0;
  return 0;
}

int vaenpvc_timer_read(vaenpvc_ctx* ctx, double* total_ms, int64_t* launches) {
  if (!ctx) return fail(VAENPVC_E_ARG, "null context");
  Call call(ctx, false);
  Runtime& r = ctx->rt;
  double tot = 0.0;
  for (size_t i = 0; i < r.used; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(r.pool[i].second) != hipSuccess) return fail(VAENPVC_E_HIP, "timer sync");
    if (hipEventElapsedTime(&ms, r.pool[i].first, r.pool[i].second) != hipSuccess) return fail(VAENPVC_E_HIP, "timer elapsed");
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (int64_t)r.used;
  r.used = 0;
  return 0;
}

int vaenpvc_abi_version(void) { return 4; }
const char* vaenpvc_last_error(void) { return g_err; }

int vaenpvc_ctx_create(const vaenpvc_arch* arch, vaenpvc_ctx** out) {
  if (!arch || !out) return fail(VAENPVC_E_ARG, "null argument");
  vaenpvc_ctx* c = new (std::nothrow) vaenpvc_ctx();
  if (!c) return fail(VAENPVC_E_ARG, "out of host memory");
  std::string err = build_model(*arch, &c->m);
  if (!err.empty()) {
    delete c;
    return fail(VAENPVC_E_ARG, "architecture: %s", err.c_str());
  }
  const char* env = getenv("VAENPVC_IMPL");
  if (env && strcmp(env, "generic") == 0) c->impl = VAENPVC_IMPL_GENERIC;
  c->rt.read_env();
  *out = c;
  return 0;
}

void vaenpvc_ctx_destroy(vaenpvc_ctx* ctx) {
  if (!ctx) return;
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int cur = -1;
    if (ctx->rt.device >= 0 && hipGetDevice(&cur) == hipSuccess) {
      if (cur != ctx->rt.device) (void)hipSetDevice(ctx->rt.device);
      ctx->rt.release();
      if (cur != ctx->rt.device) (void)hipSetDevice(cur);
    }
  }
  delete ctx;
}

int vaenpvc_set_impl(vaenpvc_ctx* ctx, int impl) {
  if (!ctx || (impl != VAENPVC_IMPL_AUTO && impl != VAENPVC_IMPL_GENERIC)) return fail(VAENPVC_E_ARG, "bad impl");
  Call call(ctx, false);
  ctx->impl = impl;
  return 0;
}

int vaenpvc_param_count(const vaenpvc_ctx* ctx) { return ctx ? (int)ctx->m.table.size() : VAENPVC_E_ARG; }
int64_t vaenpvc_param_floats(const vaenpvc_ctx* ctx) { return ctx ? ctx->m.n_params : VAENPVC_E_ARG; }

int vaenpvc_param_info(const vaenpvc_ctx* ctx, int index, char* name, int name_cap, int64_t* offset_floats,
                       int32_t* ndim, int64_t* shape) {
  if (!ctx || index < 0 || index >= (int)ctx->m.table.size()) return fail(VAENPVC_E_ARG, "bad parameter index");
  const ParamInfo& p = ctx->m.table[index];
  if (name && name_cap > 0) {
    strncpy(name, p.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (offset_floats) *offset_floats = p.offset;
  if (ndim) *ndim = p.ndim;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  return 0;
}

int64_t vaenpvc_workspace_bytes(const vaenpvc_ctx* ctx, int64_t F, int mode) {
  if (!ctx || F < 1 || (mode != VAENPVC_MODE_INFER && mode != VAENPVC_MODE_TRAIN)) return fail(VAENPVC_E_ARG, "bad argument");
  return layout_of(const_cast<vaenpvc_ctx*>(ctx), F, mode)->second * 4;
}

int vaenpvc_ws_find(const vaenpvc_ctx* ctx, int64_t F, int mode, const char* name, int64_t* offset_floats,
                    int64_t* count_floats) {
  if (!ctx || !name || F < 1) return fail(VAENPVC_E_ARG, "bad argument");
  const auto lay = layout_of(const_cast<vaenpvc_ctx*>(ctx), F, mode);
  for (const Region& r : lay->first)
    if (r.name == name) {
      if (offset_floats) *offset_floats = r.offset;
      if (count_floats) *count_floats = r.count;
      return 0;
    }
  return fail(VAENPVC_E_ARG, "no workspace region named '%s'", name);
}

int vaenpvc_encode_fwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, int64_t F, float* d_z_mu,
                       float* d_z_lv, void* d_ws, size_t ws_bytes, void* stream) {
  if (!ctx || !d_params || !d_x || !d_z_mu) return fail(VAENPVC_E_ARG, "null argument");
  Call call(ctx);
  Ws w;
  int rc = resolve(ctx, F, VAENPVC_MODE_INFER, d_ws, ws_bytes, &w);
  if (rc) return rc;
  ctx->rt.last_F = -1;   // activations / operand planes of a preceding train step may be overwritten: vaenpvc_train_bwd_target must not re-use them
  hipStream_t s = (hipStream_t)stream;
  if (use_tuned(ctx) && tuned::frame_fwd_on(F)) {
    tuned::frame_pack(ctx->m, d_params, w, nullptr, nullptr, 0, s);
    tuned::frame_forward(ctx->m, d_params, d_x, nullptr, nullptr, nullptr, nullptr, nullptr, F, w, nullptr, tuned::FRAME_ENC, nullptr, s);
  } else if (use_tuned(ctx)) tuned::encoder_fwd(ctx->m, d_params, d_x, F, w, s);
  else generic::encoder_fwd(ctx->m, d_params, d_x, F, w, s);
  size_t nb = (size_t)F * ctx->m.z * 4;
  if (hipMemcpyAsync(d_z_mu, w.z_mu, nb, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(VAENPVC_E_HIP, "copy z_mu");
  if (d_z_lv && hipMemcpyAsync(d_z_lv, w.z_lv, nb, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(VAENPVC_E_HIP, "copy z_lv");
  return check_launch("encode_fwd");
}

int vaenpvc_decode_fwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_z, const int64_t* d_y, int64_t F,
                       float* d_xh, void* d_ws, size_t ws_bytes, void* stream) {
  if (!ctx || !d_params || !d_z || !d_y || !d_xh) return fail(VAENPVC_E_ARG, "null argument");
  Call call(ctx);
  Ws w;
  int rc = resolve(ctx, F, VAENPVC_MODE_INFER, d_ws, ws_bytes, &w);
  if (rc) return rc;
  ctx->rt.last_F = -1;   // activations / operand planes of a preceding train step may be overwritten: vaenpvc_train_bwd_target must not re-use them
  hipStream_t s = (hipStream_t)stream;
  if (use_tuned(ctx) && tuned::frame_fwd_on(F)) {
    tuned::frame_pack(ctx->m, d_params, w, nullptr, nullptr, 0, s);
    tuned::frame_forward(ctx->m, d_params, nullptr, nullptr, d_y, nullptr, nullptr, d_z, F, w, d_xh, tuned::FRAME_DEC, nullptr, s);
  } else if (use_tuned(ctx)) tuned::decoder_fwd(ctx->m, d_params, d_z, d_y, F, w, d_xh, s);
  else generic::decoder_fwd(ctx->m, d_params, d_z, d_y, F, w, d_xh, s);
  return check_launch("decode_fwd");
}

static int fwd_all(vaenpvc_ctx* ctx, const float* P, const float* x, const int64_t* y, const float* eps,
                   const PhiloxKey* key, int64_t F, const Ws& w, bool want_grad, float* loss3, hipStream_t s,
                   const float* target = nullptr, bool allow_frame = true, float* zero_g = nullptr) {
  if (allow_frame && use_tuned(ctx) && tuned::frame_fwd_on(F)) {
    // small batch: one workgroup per frame carries it through the whole forward pass (gfx950_frame.h); the launch that
    // packs the weights also zero-fills what the backward pass accumulates into
    int nz2 = 0;
    float* z2 = zero_g ? tuned::frame_zero_region(w, &nz2) : nullptr;
    tuned::frame_pack(ctx->m, P, w, zero_g, z2, nz2, s);
    tuned::frame_forward(ctx->m, P, x, target, y, eps, key, nullptr, F, w, nullptr,
                         tuned::FRAME_ENC | tuned::FRAME_SAMPLE | tuned::FRAME_DEC | tuned::FRAME_LOSS | (want_grad ? tuned::FRAME_GRAD : 0),
                         loss3, s);
    return 0;
  }
  if (use_tuned(ctx)) tuned::encoder_fwd(ctx->m, P, x, F, w, s);
  else generic::encoder_fwd(ctx->m, P, x, F, w, s);
  rt().plz_F = -1;
  VAENPVC_TIMED("reparam", s, (use_tuned(ctx) && tuned::reparam_fwd_planes(ctx->m, eps, key, F, w, s)) ? (void)0 : generic::reparam_fwd(ctx->m, eps, key, F, w, s));
  if (use_tuned(ctx)) tuned::decoder_fwd(ctx->m, P, w.z, y, F, w, w.xh, s, /*weights_packed=*/true);
  else generic::decoder_fwd(ctx->m, P, w.z, y, F, w, w.xh, s);
  rt().dxh_post_F = -1;
  const bool fused_loss = want_grad && use_tuned(ctx);
  VAENPVC_TIMED("loss", s, (fused_loss && tuned::loss_fwd_post(ctx->m, P, target ? target : x, F, w, loss3, s))
                               ? (void)0 : generic::loss_fwd(ctx->m, target ? target : x, F, w, want_grad, loss3, s));   // (the density's data argument)
  return 0;
}

static PhiloxKey make_key(uint64_t seed, uint64_t offset, const int64_t* d_offset = nullptr) {
  return PhiloxKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), d_offset};
}

static int loss_impl(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y, const float* d_eps,
                     const PhiloxKey* key, int64_t F, float* d_loss3, void* d_ws, size_t ws_bytes, void* stream) {
  if (!ctx || !d_params || !d_x || !d_y || (!d_eps && !key) || !d_loss3) return fail(VAENPVC_E_ARG, "null argument");
  Call call(ctx);
  Ws w;
  int rc = resolve(ctx, F, VAENPVC_MODE_INFER, d_ws, ws_bytes, &w);
  if (rc) return rc;
  ctx->rt.last_F = -1;   // activations / operand planes of a preceding train step may be overwritten: vaenpvc_train_bwd_target must not re-use them
  fwd_all(ctx, d_params, d_x, d_y, d_eps, key, F, w, false, d_loss3, (hipStream_t)stream);
  return check_launch("loss_fwd");
}

int vaenpvc_loss_fwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                     const float* d_eps, int64_t F, float* d_loss3, void* d_ws, size_t ws_bytes, void* stream) {
  return loss_impl(ctx, d_params, d_x, d_y, d_eps, nullptr, F, d_loss3, d_ws, ws_bytes, stream);
}
int vaenpvc_loss_fwd_seeded(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                            uint64_t seed, uint64_t offset, int64_t F, float* d_loss3, void* d_ws, size_t ws_bytes,
                            void* stream) {
  PhiloxKey k = make_key(seed, offset);
  return loss_impl(ctx, d_params, d_x, d_y, nullptr, &k, F, d_loss3, d_ws, ws_bytes, stream);
}

static int train_impl(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                      const float* d_eps, const PhiloxKey* key, int64_t F, float* d_grads, float* d_loss3, void* d_ws,
                      size_t ws_bytes, void* stream, const float* d_target = nullptr) {
  if (!ctx || !d_params || !d_x || !d_y || (!d_eps && !key) || !d_grads || !d_loss3) return fail(VAENPVC_E_ARG, "null argument");
  Call call(ctx);
  Ws w;
  int rc = resolve(ctx, F, VAENPVC_MODE_TRAIN, d_ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // small batches: both passes on the whole-frame kernels, or neither (the layered backward pass reads operand copies
  // only the layered forward pass leaves behind)
  const bool frame = use_tuned(ctx) && tuned::frame_fwd_on(F) && tuned::frame_bwd_on(F);
  fwd_all(ctx, d_params, d_x, d_y, d_eps, key, F, w, true, d_loss3, s, d_target, frame, frame ? d_grads : nullptr);
  {  // what vaenpvc_train_bwd_target may re-use
    Runtime& r = ctx->rt;
    r.last_F = F;
    r.last_path = frame ? 2 : use_tuned(ctx) ? 1 : 0;
    r.last_planes = r.planes;
    r.last_fwd_mask = r.fwd_mask;
    r.last_bwd_mask = r.bwd_mask;
    r.last_ws = d_ws;
  }
  const float* eps_bwd = key ? w.eps : d_eps;   // (the seeded sampler stored its draw in the workspace)
  ctx->rt.bucket_next = 0;
  if (frame) {
    tuned::backward_frame(ctx->m, d_params, d_x, d_target, d_y, eps_bwd, F, w, d_grads, s, /*g_zeroed=*/true, d_loss3);
  } else if (use_tuned(ctx)) {
    tuned::backward(ctx->m, d_params, d_x, d_y, eps_bwd, F, w, d_grads, s);
  } else {
    generic::backward(ctx->m, d_params, d_x, d_y, eps_bwd, F, w, d_grads, s);
    if (ctx->rt.bucket_cb)  // the generic path finishes everything at once: one bucket
      ctx->rt.bucket_cb(ctx->rt.bucket_user, 0, 0, ctx->m.n_params, (void*)s);
  }
  return check_launch("train_fwd_bwd");
}

int vaenpvc_train_fwd_bwd(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                          const float* d_eps, int64_t F, float* d_grads, float* d_loss3, void* d_ws,
                          size_t ws_bytes, void* stream) {
  return train_impl(ctx, d_params, d_x, d_y, d_eps, nullptr, F, d_grads, d_loss3, d_ws, ws_bytes, stream);
}
int vaenpvc_train_fwd_bwd_seeded(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                                 uint64_t seed, uint64_t offset, const int64_t* d_offset, int64_t F, float* d_grads,
                                 float* d_loss3, void* d_ws, size_t ws_bytes, void* stream) {
  PhiloxKey k = make_key(seed, offset, d_offset);
  return train_impl(ctx, d_params, d_x, d_y, nullptr, &k, F, d_grads, d_loss3, d_ws, ws_bytes, stream);
}

int vaenpvc_train_fwd_bwd_target(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                                 const float* d_eps, const float* d_target, int64_t F, float* d_grads,
                                 float* d_loss3, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_target) return fail(VAENPVC_E_ARG, "null argument");
  return train_impl(ctx, d_params, d_x, d_y, d_eps, nullptr, F, d_grads, d_loss3, d_ws, ws_bytes, stream, d_target);
}

int vaenpvc_train_bwd_target(vaenpvc_ctx* ctx, const float* d_params, const float* d_x, const int64_t* d_y,
                             const float* d_eps, const float* d_target, int64_t F, float* d_grads, float* d_loss3,
                             void* d_ws, size_t ws_bytes, void* stream) {
  if (!ctx || !d_params || !d_x || !d_y || !d_eps || !d_target || !d_grads || !d_loss3) return fail(VAENPVC_E_ARG, "null argument");
  Call call(ctx);
  Ws w;
  int rc = resolve(ctx, F, VAENPVC_MODE_TRAIN, d_ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  {
    // the backward pass consumes what the preceding train step of THIS context left in THIS workspace (activations, packed
    // weights, operand planes): same batch size, same kernel family, same masks and precision -- anything else would read
    // stale or unwritten operands without a sign (round-3 advisor)
    const Runtime& r = ctx->rt;
    const int path = (use_tuned(ctx) && tuned::frame_fwd_on(F) && tuned::frame_bwd_on(F)) ? 2 : use_tuned(ctx) ? 1 : 0;
    if (r.last_F != F || r.last_path != path || r.last_planes != r.planes || r.last_fwd_mask != r.fwd_mask ||
        r.last_bwd_mask != r.bwd_mask || r.last_ws != d_ws)
      return fail(VAENPVC_E_STATE, "train_bwd_target: no matching train step precedes it in this context (batch size, kernel selection, precision or workspace differ)");
  }
  rt().dxh_post_F = -1;
  generic::loss_fwd(ctx->m, d_target, F, w, true, d_loss3, s);   // new d(xh) from the activations already in place
  ctx->rt.bucket_next = 0;
  if (use_tuned(ctx) && tuned::frame_fwd_on(F) && tuned::frame_bwd_on(F)) {
    int nz2 = 0;
    float* z2 = tuned::frame_zero_region(w, &nz2);
    tuned::frame_pack(ctx->m, d_params, w, d_grads, z2, nz2, s, /*zero_only=*/true);   // (the packed weights of the preceding train step are still in the workspace: parameters may not change in between, include/vaenpvc.h)
    tuned::backward_frame(ctx->m, d_params, d_x, d_target, d_y, d_eps, F, w, d_grads, s, /*g_zeroed=*/true);
  } else if (use_tuned(ctx)) {
    tuned::backward(ctx->m, d_params, d_x, d_y, d_eps, F, w, d_grads, s);
  } else {
    generic::backward(ctx->m, d_params, d_x, d_y, d_eps, F, w, d_grads, s);
    if (ctx->rt.bucket_cb) ctx->rt.bucket_cb(ctx->rt.bucket_user, 0, 0, ctx->m.n_params, (void*)s);
  }
  return check_launch("train_bwd_target");
}

int vaenpvc_philox_normal(uint64_t seed, uint64_t offset, float* d_out, int64_t n, void* stream) {
  if (!d_out || n < 1) return fail(VAENPVC_E_ARG, "bad argument");
  launch_philox_normal(d_out, n, make_key(seed, offset), (hipStream_t)stream);
  return check_launch("philox_normal");
}
int vaenpvc_philox_uniform(uint64_t seed, uint64_t offset, float* d_out, int64_t n, void* stream) {
  if (!d_out || n < 1) return fail(VAENPVC_E_ARG, "bad argument");
  launch_philox_uniform(d_out, n, make_key(seed, offset), (hipStream_t)stream);
  return check_launch("philox_uniform");
}

int vaenpvc_adam_step(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n, int64_t step,
                      float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
  if (!d_params || !d_grads || !d_m || !d_v || n < 1 || step < 1) return fail(VAENPVC_E_ARG, "bad argument");
  double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)step)) /
                (1.0 - std::pow((double)beta1, (double)step));
  launch_adam(d_params, d_grads, d_m, d_v, n, (float)lr_t, beta1, beta2, eps, grad_scale, (hipStream_t)stream);
  return check_launch("adam_step");
}

int vaenpvc_adam_step_dev(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n, int64_t* d_step,
                          float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
  if (!d_params || !d_grads || !d_m || !d_v || !d_step || n < 1) return fail(VAENPVC_E_ARG, "bad argument");
  launch_adam_dev(d_params, d_grads, d_m, d_v, n, d_step, lr, beta1, beta2, eps, grad_scale, (hipStream_t)stream);
  return check_launch("adam_step_dev");
}

int vaenpvc_tanhize_fwd(const float* d_sp, const float* d_xmin, const float* d_xmax, float* d_x, int64_t F,
                        int32_t H, void* stream) {
  if (!d_sp || !d_xmin || !d_xmax || !d_x || F < 1 || H < 1) return fail(VAENPVC_E_ARG, "bad argument");
  launch_tanhize(d_sp, d_xmin, d_xmax, d_x, F, H, true, (hipStream_t)stream);
  return check_launch("tanhize_fwd");
}

int vaenpvc_tanhize_bwd(const float* d_x, const float* d_xmin, const float* d_xmax, float* d_sp, int64_t F,
                        int32_t H, void* stream) {
  if (!d_x || !d_xmin || !d_xmax || !d_sp || F < 1 || H < 1) return fail(VAENPVC_E_ARG, "bad argument");
  launch_tanhize(d_x, d_xmin, d_xmax, d_sp, F, H, false, (hipStream_t)stream);
  return check_launch("tanhize_bwd");
}

static bool gv_shape_ok(int64_t F, int32_t n_seg, int32_t H) {
  // launch grids fit 32 bits; byte counts of x and of the workspace fit int64 with room
  return F >= 0 && n_seg > 0 && H > 0 && F <= (1LL << 56) / H && gv_chunk_grid(F, n_seg) <= INT32_MAX &&
         gv_chunk_grid(F, n_seg) * H <= (1LL << 56) && H <= (1 << 23) &&
         (int64_t)n_seg * ((H + 31) / 32) <= INT32_MAX;
}

int64_t vaenpvc_gv_workspace_bytes(int64_t F, int32_t n_seg, int32_t H) {
  if (!gv_shape_ok(F, n_seg, H)) return fail(VAENPVC_E_ARG, "bad argument (F %lld, n_seg %d, H %d)", (long long)F, n_seg, H);
  return gv_workspace_bytes(F, n_seg, H);
}

int vaenpvc_gv_postfilter(const float* d_x, const int64_t* d_offsets, int32_t n_seg, int64_t F, int32_t H,
                          const float* d_xmin, const float* d_xmax, const float* d_gv, float* d_sp, void* d_ws,
                          size_t ws_bytes, void* stream) {
  if (!d_x || !d_offsets || !d_xmin || !d_xmax || !d_gv || !d_sp) return fail(VAENPVC_E_ARG, "null argument");
  if (!gv_shape_ok(F, n_seg, H)) return fail(VAENPVC_E_ARG, "bad argument (F %lld, n_seg %d, H %d)", (long long)F, n_seg, H);
  const char *x0 = (const char*)d_x, *s0 = (const char*)d_sp;
  const int64_t nbytes = F * (int64_t)H * 4;
  if (nbytes > 0 && x0 < s0 + nbytes && s0 < x0 + nbytes) return fail(VAENPVC_E_ARG, "d_sp must not overlap d_x");
  const int64_t need = gv_workspace_bytes(F, n_seg, H);
  if (d_ws == nullptr || ws_bytes < (size_t)need)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)need, (long long)ws_bytes);
  if (((uintptr_t)d_ws & 15) != 0) return fail(VAENPVC_E_ARG, "workspace must be 16-byte aligned");
  launch_gv_postfilter(d_x, d_offsets, n_seg, F, H, d_xmin, d_xmax, d_gv, d_sp, d_ws, (hipStream_t)stream);
  return check_launch("gv_postfilter");
}

static int select_shape_check(int64_t F, int32_t H, int32_t n_rank) {
  if (F < 1 || F > INT32_MAX) return fail(VAENPVC_E_ARG, "F must be in [1, 2^31 - 1] (got %lld)", (long long)F);
  if (H < 1 || H > SEL_MAX_H) return fail(VAENPVC_E_ARG, "H must be in [1, %d] (got %d)", SEL_MAX_H, H);
  if (n_rank < 1 || n_rank > VAENPVC_SELECT_MAX_RANKS)
    return fail(VAENPVC_E_ARG, "n_rank must be in [1, %d] (got %d)", VAENPVC_SELECT_MAX_RANKS, n_rank);
  return 0;
}

int64_t vaenpvc_column_select_workspace_bytes(int64_t F, int32_t H, int32_t n_rank) {
  if (select_shape_check(F, H, n_rank) != 0) return VAENPVC_E_ARG;
  return column_select_workspace_bytes(H, n_rank);
}

int vaenpvc_column_select(const float* d_x, int64_t F, int32_t H, int64_t ld, const int64_t* host_ranks, int32_t n_rank,
                          float* d_out, int32_t* d_flag, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_x || !host_ranks || !d_out || !d_flag) return fail(VAENPVC_E_ARG, "null argument");
  if (select_shape_check(F, H, n_rank) != 0) return VAENPVC_E_ARG;
  if (ld < H || ld > SEL_MAX_LD)
    return fail(VAENPVC_E_ARG, "ld must be in [H, %lld] (got %lld, H %d)", (long long)SEL_MAX_LD, (long long)ld, H);
  for (int r = 0; r < n_rank; ++r)
    if (host_ranks[r] < 0 || host_ranks[r] >= F)
      return fail(VAENPVC_E_ARG, "rank %d is %lld, outside [0, %lld)", r, (long long)host_ranks[r], (long long)F);
  const int64_t need = column_select_workspace_bytes(H, n_rank);
  if (d_ws == nullptr || ws_bytes < (size_t)need)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)need, (long long)ws_bytes);
  if (((uintptr_t)d_ws & 15) != 0) return fail(VAENPVC_E_ARG, "workspace must be 16-byte aligned");
  launch_column_select(d_x, F, H, ld, host_ranks, n_rank, d_out, d_flag, d_ws, (hipStream_t)stream);
  return check_launch("column_select");
}

static int speaker_stats_shape_check(int64_t F, int32_t n_seg, int32_t H) {
  if (F < 0 || n_seg < 1 || H < 1 || H > SEL_MAX_H)
    return fail(VAENPVC_E_ARG, "bad argument (F %lld, n_seg %d, H %d)", (long long)F, n_seg, H);
  return 0;
}

int64_t vaenpvc_speaker_stats_workspace_bytes(int64_t F, int32_t n_seg, int32_t H) {
  if (speaker_stats_shape_check(F, n_seg, H) != 0) return VAENPVC_E_ARG;
  return speaker_stats_workspace_bytes(n_seg, H);
}

int vaenpvc_speaker_stats(const float* d_sp, int64_t ld_sp, const float* d_f0, int64_t ld_f0, const int64_t* d_offsets,
                          const int32_t* d_spk, int32_t n_seg, int32_t n_spk, int64_t F, int32_t H, double* d_lf0,
                          double* d_gv, int64_t* d_n_utt, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_sp || !d_f0 || !d_offsets || !d_spk || !d_lf0 || !d_gv || !d_n_utt) return fail(VAENPVC_E_ARG, "null argument");
  if (speaker_stats_shape_check(F, n_seg, H) != 0) return VAENPVC_E_ARG;
  if (n_spk < 1 || ld_sp < H || ld_f0 < 1 || ld_sp > SEL_MAX_LD || ld_f0 > SEL_MAX_LD)
    return fail(VAENPVC_E_ARG, "bad argument (n_spk %d, ld_sp %lld, ld_f0 %lld, H %d)", n_spk, (long long)ld_sp,
                (long long)ld_f0, H);
  const int64_t need = speaker_stats_workspace_bytes(n_seg, H);
  if (d_ws == nullptr || ws_bytes < (size_t)need)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)need, (long long)ws_bytes);
  if (((uintptr_t)d_ws & 15) != 0) return fail(VAENPVC_E_ARG, "workspace must be 16-byte aligned");
  launch_speaker_stats(d_sp, ld_sp, d_f0, ld_f0, d_offsets, d_spk, n_seg, n_spk, F, H, d_lf0, d_gv, d_n_utt, d_ws,
                       (hipStream_t)stream);
  return check_launch("speaker_stats");
}

static bool synth_shape_ok(int32_t n_seg, int64_t S, int32_t H, int32_t fs) {
  // pulse samples and slot counts fit int32, launch grids 32 bits
  return n_seg > 0 && n_seg < (1 << 24) && S >= 0 && S <= INT32_MAX && H == 513 && fs >= 8000 && fs <= 48000;
}

int64_t vaenpvc_synth_workspace_bytes(int32_t n_seg, int64_t S, int32_t H, int32_t fs) {
  if (!synth_shape_ok(n_seg, S, H, fs))
    return fail(VAENPVC_E_ARG, "bad argument (n_seg %d, S %lld, H %d, fs %d)", n_seg, (long long)S, H, fs);
  return synth_workspace_bytes(n_seg, S, fs);
}

static bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
  const char *x = (const char*)a, *y = (const char*)b;
  return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

int vaenpvc_synthesize(const float* d_f0, const float* d_sp, const float* d_en, const float* d_ap,
                       const int64_t* d_frame_offsets, const int64_t* d_sample_offsets, int32_t n_seg, int64_t F,
                       int64_t S, int32_t H, int32_t fs, double frame_period_ms, uint64_t seed, float* d_y, void* d_ws,
                       size_t ws_bytes, void* stream) {
  if (!d_f0 || !d_sp || !d_en || !d_ap || !d_frame_offsets || !d_sample_offsets || !d_y)
    return fail(VAENPVC_E_ARG, "null argument");
  if (!synth_shape_ok(n_seg, S, H, fs) || F < n_seg || F > INT32_MAX)
    return fail(VAENPVC_E_ARG, "bad argument (n_seg %d, F %lld, S %lld, H %d, fs %d)", n_seg, (long long)F,
                (long long)S, H, fs);
  if (!std::isfinite(frame_period_ms) || !(frame_period_ms > 0.0))
    return fail(VAENPVC_E_ARG, "frame period must be finite and > 0 (got %g ms)", frame_period_ms);
  const int64_t ny = S * 4, nf = F * 4, nfh = F * (int64_t)H * 4, no = ((int64_t)n_seg + 1) * 8;
  if (overlaps(d_y, ny, d_f0, nf) || overlaps(d_y, ny, d_sp, nfh) || overlaps(d_y, ny, d_en, nf) ||
      overlaps(d_y, ny, d_ap, nfh) || overlaps(d_y, ny, d_frame_offsets, no) || overlaps(d_y, ny, d_sample_offsets, no))
    return fail(VAENPVC_E_ARG, "d_y must not overlap an input");
  const int64_t need = synth_workspace_bytes(n_seg, S, fs);
  if (d_ws == nullptr || ws_bytes < (size_t)need)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)need, (long long)ws_bytes);
  if (((uintptr_t)d_ws & 15) != 0) return fail(VAENPVC_E_ARG, "workspace must be 16-byte aligned");
  if (overlaps(d_y, ny, d_ws, need)) return fail(VAENPVC_E_ARG, "d_y must not overlap the workspace");
  launch_synthesize(d_f0, d_sp, d_en, d_ap, d_frame_offsets, d_sample_offsets, n_seg, F, S, fs, frame_period_ms, seed,
                    d_y, d_ws, (hipStream_t)stream);
  return check_launch("synthesize");
}

static int analysis_bands(int32_t fs, double f0_floor, double f0_ceil) {
  // 71 <= f0_floor < f0_ceil <= 800 at 16 kHz: every FFT the stages derive stays <= 2048 points
  if (fs != 16000 || !std::isfinite(f0_floor) || !std::isfinite(f0_ceil) || !(f0_floor >= 71.0) ||
      !(f0_floor < f0_ceil) || !(f0_ceil <= 800.0))
    return -1;
  return 1 + (int)(std::log(f0_ceil / f0_floor) / std::log(2.0) * 2.0);
}

static bool analysis_shape_ok(int32_t n_seg, int64_t S, int64_t F, double frame_period_ms, int32_t fs) {
  // every utterance has >= 1 sample and >= 1 frame; F is at most the frame count the samples allow
  return n_seg > 0 && n_seg < (1 << 24) && S >= n_seg && S <= INT32_MAX && F >= n_seg &&
         std::isfinite(frame_period_ms) && frame_period_ms >= 1.0 && frame_period_ms <= 50.0 &&
         F <= (int64_t)(1000.0 * (double)S / fs / frame_period_ms) + n_seg;
}

int64_t vaenpvc_analysis_workspace_bytes(int32_t n_seg, int64_t S, int64_t F, int32_t fs, double frame_period_ms,
                                         double f0_floor, double f0_ceil) {
  const int nb = analysis_bands(fs, f0_floor, f0_ceil);
  if (nb < 1 || !analysis_shape_ok(n_seg, S, F, frame_period_ms, fs))
    return fail(VAENPVC_E_ARG, "bad argument (n_seg %d, S %lld, F %lld, fs %d, frame period %g, f0 %g .. %g)", n_seg,
                (long long)S, (long long)F, fs, frame_period_ms, f0_floor, f0_ceil);
  return analysis_workspace_bytes(n_seg, S, F, nb);
}

int vaenpvc_analyze(const float* d_x, const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t n_seg,
                    int64_t S, int64_t F, int32_t fs, double frame_period_ms, double f0_floor, double f0_ceil,
                    float* d_f0, float* d_sp, float* d_ap, float* d_en, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_x || !d_sample_offsets || !d_frame_offsets || !d_f0 || !d_sp || !d_ap || !d_en)
    return fail(VAENPVC_E_ARG, "null argument");
  const int nb = analysis_bands(fs, f0_floor, f0_ceil);
  if (nb < 1) return fail(VAENPVC_E_ARG, "fs must be 16000 and 71 <= f0_floor < f0_ceil <= 800 (got %d, %g, %g)", fs,
                          f0_floor, f0_ceil);
  if (!analysis_shape_ok(n_seg, S, F, frame_period_ms, fs))
    return fail(VAENPVC_E_ARG, "bad argument (n_seg %d, S %lld, F %lld, frame period %g)", n_seg, (long long)S,
                (long long)F, frame_period_ms);
  const int64_t nf = F * 4, nfh = F * 513 * 4, nx = S * 4, no = ((int64_t)n_seg + 1) * 8;
  const void* outs[4] = {d_f0, d_sp, d_ap, d_en};
  const int64_t outn[4] = {nf, nfh, nfh, nf};
  for (int a = 0; a < 4; ++a) {
    if (overlaps(outs[a], outn[a], d_x, nx) || overlaps(outs[a], outn[a], d_sample_offsets, no) ||
        overlaps(outs[a], outn[a], d_frame_offsets, no))
      return fail(VAENPVC_E_ARG, "outputs must not overlap an input");
    for (int b = a + 1; b < 4; ++b)
      if (overlaps(outs[a], outn[a], outs[b], outn[b])) return fail(VAENPVC_E_ARG, "outputs must not overlap");
  }
  const int64_t need = analysis_workspace_bytes(n_seg, S, F, nb);
  if (d_ws == nullptr || ws_bytes < (size_t)need)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)need,
                (long long)ws_bytes);
  if (((uintptr_t)d_ws & 255) != 0) return fail(VAENPVC_E_ARG, "workspace must be 256-byte aligned");
  for (int a = 0; a < 4; ++a)
    if (overlaps(outs[a], outn[a], d_ws, need)) return fail(VAENPVC_E_ARG, "outputs must not overlap the workspace");
  launch_analyze(d_x, d_sample_offsets, d_frame_offsets, n_seg, S, F, fs, frame_period_ms, f0_floor, f0_ceil, nb, d_f0,
                 d_sp, d_ap, d_en, d_ws, (hipStream_t)stream);
  return check_launch("analyze");
}

int vaenpvc_mcep_matrix(int32_t order, double alpha, int32_t H, double* host_W) {
  if (!host_W) return fail(VAENPVC_E_ARG, "null argument");
  if (order < 1 || order > VAENPVC_MCD_MAX_ORDER || H != 513 || !std::isfinite(alpha) || !(alpha >= 0.0) ||
      !(alpha < 1.0))
    return fail(VAENPVC_E_ARG, "need 1 <= order <= %d, 0 <= alpha < 1, H == 513 (got %d, %g, %d)",
                VAENPVC_MCD_MAX_ORDER, order, alpha, H);
  mcep_matrix_host(order, alpha, host_W);
  return 0;
}

int vaenpvc_resample_plan(int32_t rate_in, int32_t rate_out, int32_t* up, int32_t* down, int32_t* half_taps) {
  if (!up || !down || !half_taps) return fail(VAENPVC_E_ARG, "null argument");
  int L, M, K;
  if (!resample_plan_host(rate_in, rate_out, &L, &M, &K))
    return fail(VAENPVC_E_ARG,
                "cannot resample %d -> %d Hz: need distinct rates in [1000, 384000], 2K L <= %d table entries and a "
                "window ceil(%d M / L) + 2K <= %d samples",
                rate_in, rate_out, VAENPVC_RESAMPLE_MAX_TABLE, VAENPVC_RESAMPLE_TILE, VAENPVC_RESAMPLE_MAX_WINDOW);
  *up = L;
  *down = M;
  *half_taps = K;
  return 0;
}

int vaenpvc_resample_filter(int32_t rate_in, int32_t rate_out, double* host_table) {
  if (!host_table) return fail(VAENPVC_E_ARG, "null argument");
  int32_t L, M, K;
  if (vaenpvc_resample_plan(rate_in, rate_out, &L, &M, &K) != 0) return VAENPVC_E_ARG;
  resample_filter_host(L, M, K, host_table);
  return 0;
}

int vaenpvc_resample(const float* d_x, const int64_t* d_in_offsets, const int64_t* d_out_offsets, int32_t n_seg,
                     int64_t S_in, int64_t S_out, int32_t rate_in, int32_t rate_out, const double* d_table, float* d_y,
                     void* stream) {
  if (!d_x || !d_in_offsets || !d_out_offsets || !d_table || !d_y) return fail(VAENPVC_E_ARG, "null argument");
  int32_t L, M, K;
  if (vaenpvc_resample_plan(rate_in, rate_out, &L, &M, &K) != 0) return VAENPVC_E_ARG;
  // every segment has >= 1 sample and so >= 1 output; S_out is at most what the samples allow (one ceil per segment)
  if (n_seg < 1 || n_seg >= (1 << 24) || S_in < n_seg || S_in > INT32_MAX || S_out < n_seg || S_out > INT32_MAX ||
      S_out > (S_in * L + M - 1) / M + n_seg)
    return fail(VAENPVC_E_ARG, "bad argument (n_seg %d, S_in %lld, S_out %lld, %d -> %d Hz)", n_seg, (long long)S_in,
                (long long)S_out, rate_in, rate_out);
  const int64_t ny = S_out * 4, no = ((int64_t)n_seg + 1) * 8;
  if (overlaps(d_y, ny, d_x, S_in * 4) || overlaps(d_y, ny, d_table, (int64_t)2 * K * L * 8) ||
      overlaps(d_y, ny, d_in_offsets, no) || overlaps(d_y, ny, d_out_offsets, no))
    return fail(VAENPVC_E_ARG, "d_y must not overlap an input");
  launch_resample(d_x, d_in_offsets, d_out_offsets, n_seg, S_in, S_out, L, M, K, d_table, d_y, (hipStream_t)stream);
  return check_launch("resample");
}

static bool mcd_shape_ok(int32_t n_pair, int64_t Fa, int64_t Fb, int64_t cells, int32_t order) {
  // every utterance has 1 .. VAENPVC_MCD_MAX_FRAMES frames, so cells (the sum of Ta * Tb) lies between the larger side's
  // frame count and n_pair * MAX^2; the offsets themselves are device data (checked by the binding and by k_mcd_prep)
  const int64_t mx = VAENPVC_MCD_MAX_FRAMES;
  return n_pair >= 1 && n_pair <= VAENPVC_MCD_MAX_PAIRS && Fa >= n_pair && Fb >= n_pair && Fa <= n_pair * mx &&
         Fb <= n_pair * mx && cells >= (Fa > Fb ? Fa : Fb) && cells <= Fa * Fb && cells <= n_pair * mx * mx &&
         order >= 1 && order <= VAENPVC_MCD_MAX_ORDER;
}

int64_t vaenpvc_mcd_workspace_bytes(int32_t n_pair, int64_t Fa, int64_t Fb, int64_t cells, int32_t order) {
  if (!mcd_shape_ok(n_pair, Fa, Fb, cells, order))
    return fail(VAENPVC_E_ARG, "bad argument (n_pair %d, Fa %lld, Fb %lld, cells %lld, order %d)", n_pair,
                (long long)Fa, (long long)Fb, (long long)cells, order);
  return mcd_workspace_bytes(n_pair, Fa, Fb, cells, order);
}

int vaenpvc_mcd_dtw(const float* d_spA, const float* d_enA, const float* d_f0A, const int64_t* d_offA, int64_t Fa,
                    const float* d_spB, const float* d_enB, const float* d_f0B, const int64_t* d_offB, int64_t Fb,
                    int32_t n_pair, int64_t cells, const double* d_W, int32_t order, double* d_results,
                    int32_t* d_path, double* d_D, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_spA || !d_enA || !d_f0A || !d_offA || !d_spB || !d_enB || !d_f0B || !d_offB || !d_W || !d_results)
    return fail(VAENPVC_E_ARG, "null argument");
  if (!mcd_shape_ok(n_pair, Fa, Fb, cells, order))
    return fail(VAENPVC_E_ARG, "bad argument (n_pair %d, Fa %lld, Fb %lld, cells %lld, order %d)", n_pair,
                (long long)Fa, (long long)Fb, (long long)cells, order);
  const int64_t need = mcd_workspace_bytes(n_pair, Fa, Fb, cells, order);
  if (d_ws == nullptr || ws_bytes < (size_t)need)
    return fail(VAENPVC_E_WORKSPACE, "workspace too small: need %lld bytes, got %lld", (long long)need,
                (long long)ws_bytes);
  if (((uintptr_t)d_ws & 255) != 0) return fail(VAENPVC_E_ARG, "workspace must be 256-byte aligned");
  const void* outs[3] = {d_results, d_path, d_D};
  const int64_t outn[3] = {(int64_t)n_pair * 64, (Fa + Fb) * 8, cells * 8};
  const void* ins[9] = {d_spA, d_enA, d_f0A, d_offA, d_spB, d_enB, d_f0B, d_offB, d_W};
  const int64_t inn[9] = {Fa * 513 * 4, Fa * 4, Fa * 4, ((int64_t)n_pair + 1) * 8, Fb * 513 * 4, Fb * 4, Fb * 4,
                          ((int64_t)n_pair + 1) * 8, ((int64_t)order + 1) * 513 * 8};
  for (int a = 0; a < 3; ++a) {
    if (!outs[a]) continue;
    for (int b = 0; b < 9; ++b)
      if (overlaps(outs[a], outn[a], ins[b], inn[b])) return fail(VAENPVC_E_ARG, "outputs must not overlap an input");
    for (int b = a + 1; b < 3; ++b)
      if (outs[b] && overlaps(outs[a], outn[a], outs[b], outn[b]))
        return fail(VAENPVC_E_ARG, "outputs must not overlap");
    if (overlaps(outs[a], outn[a], d_ws, need)) return fail(VAENPVC_E_ARG, "outputs must not overlap the workspace");
  }
  launch_mcd_dtw(d_spA, d_enA, d_f0A, d_offA, Fa, d_spB, d_enB, d_f0B, d_offB, Fb, n_pair, cells, d_W, order, d_results,
                 d_path, d_D, d_ws, (hipStream_t)stream);
  return check_launch("mcd_dtw");
}

int vaenpvc_unpack_records(const float* d_records, int64_t F, int32_t rec_floats, int32_t H, const float* d_xmin,
                           const float* d_xmax, float* d_x, int64_t* d_y, void* stream) {
  if (!d_records || !d_xmin || !d_xmax || !d_x || !d_y || F < 1 || H < 1 || rec_floats < H + 1)
    return fail(VAENPVC_E_ARG, "bad argument");
  launch_unpack(d_records, nullptr, F, rec_floats, H, d_xmin, d_xmax, d_x, d_y, (hipStream_t)stream);
  return check_launch("unpack_records");
}

int vaenpvc_gather_unpack_records(const float* d_records, int64_t n_records, const int64_t* d_index, int64_t F,
                                  int32_t rec_floats, int32_t H, const float* d_xmin, const float* d_xmax, float* d_x,
                                  int64_t* d_y, void* stream) {
  if (!d_records || !d_index || !d_xmin || !d_xmax || !d_x || !d_y || F < 1 || n_records < 1 || H < 1 || rec_floats < H + 1)
    return fail(VAENPVC_E_ARG, "bad argument");
  launch_unpack(d_records, d_index, F, rec_floats, H, d_xmin, d_xmax, d_x, d_y, (hipStream_t)stream);
  return check_launch("gather_unpack_records");
}

int vaenpvc_validate_ids(const vaenpvc_ctx* ctx, const int64_t* d_y, int64_t F, int32_t* d_flag, void* stream) {
  if (!ctx || !d_y || !d_flag || F < 1) return fail(VAENPVC_E_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  int32_t bad = 0;
  launch_check_ids(d_y, F, ctx->m.ny, d_flag, s);
  if (hipMemcpyAsync(&bad, d_flag, sizeof bad, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(VAENPVC_E_HIP, "validate_ids: copy");
  if (bad) return fail(VAENPVC_E_ARG, "%d speaker id(s) outside [0, %d)", (int)bad, ctx->m.ny);
  return check_launch("validate_ids");
}

int vaenpvc_summary(const float* d_data, int64_t n, const float* d_edges, int32_t n_edges, double* d_stats,
                    uint64_t* d_counts, void* stream) {
  if (!d_data || !d_edges || !d_stats || !d_counts || n < 1 || n_edges < 1 || n_edges > 2048)
    return fail(VAENPVC_E_ARG, "bad argument");
  launch_summary(d_data, n, d_edges, n_edges, d_stats, reinterpret_cast<unsigned long long*>(d_counts), (hipStream_t)stream);
  return check_launch("summary");
}

}  // extern "C"
