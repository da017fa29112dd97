// gfx950_gv.hip -- global-variance (GV) post-filter of the conversion path, fused with the inverse Tanhize
// (not in the reference: its README lists GV as a TODO and as left out of the repository).
//
// x [F, H] fp32 holds n_seg utterances back to back (rows off[u] .. off[u+1]).  Per utterance and bin, with
// c = (x*.5+.5)*(xmax-xmin)+xmin (affine in x, so the statistics are taken on x and mapped):
//   out = mu_c + sqrt(g / v_c) * (c - mu_c)   where v_c > 1e-8,   out = c (the fp32 inverse Tanhize) elsewhere.
//
// Three launches, no host synchronisation, no allocation, grids sized from (F, n_seg, H) alone:
//   k_gv_partial   one workgroup per (utterance, chunk of GV_C frames, 64 bins): per bin, Welford (mean, M2) of
//                  x - x0, x0 = the chunk's first row (shifted: the mean's rounding error is relative to the spread,
//                  not to |x|); wave w takes rows w, w + 4, ..., the four waves combine in LDS in order
//   k_gv_finalize  one workgroup per (utterance, 32 bins), 32 chunk slices: the exact two-pass combination of the chunk
//                  partials (fp64 sums in a fixed order: mean, then M2 about it), writes the per-bin map
//                  out = mu_c + k ((x - mu_x.hi) - mu_x.lo), mu_x split into two floats: k reaches sqrt(g / 1e-8), so
//                  an fp32 mu_x would shift the output by k ulp(mu_x)
//   k_gv_apply     the chunk grid again: reads x, writes out
// Chunk k of utterance u is chunk-grid column floor(off[u]/GV_C) + u + k (floor(F/GV_C) + n_seg columns; a workgroup
// past its utterance's last chunk exits).  Chunks start at multiples of GV_C frames from the utterance's first frame
// and every combination order depends only on the chunk count, so an utterance's output is a function of its own
// frames: the same bytes whatever its offset in the batch or its neighbours.  No atomics.
// Rows are 4*H bytes (2 052 at H = 513, mostly not 16-byte aligned): a wave reads 64 consecutive bins of a row, one
// dword per lane (256 contiguous bytes), addressed from the chunk's first row with 32-bit offsets (GV_C * H < 2^30);
// a thread issues the loads of all its GV_C / 4 rows before it uses one.
#include "kernels.h"

namespace vaenpvc {

namespace {

constexpr int GV_C = 128;        // frames per chunk
constexpr int GV_W = 4;          // waves of the chunk kernels; 64 bins per workgroup
constexpr int GV_U = GV_C / GV_W;  // rows per thread, all loads in flight at once
constexpr int GV_FB = 32;        // bins per finalize workgroup
constexpr int GV_FS = 32;        // chunk slices per finalize workgroup (1024 threads)

// chunk-grid column b -> utterance u and its frame rows [r0, r1); false for a column past its utterance's last chunk
__device__ bool gv_chunk(const int64_t* __restrict__ off, int n_seg, int64_t F, int64_t b, int& u, int64_t& r0,
                         int64_t& r1) {
  int lo = 0, hi = n_seg - 1;  // largest u with off[u] / GV_C + u <= b (strictly increasing in u)
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (off[mid] / GV_C + mid <= b) lo = mid;
    else hi = mid - 1;
  }
  u = lo;
  const int64_t s = off[u], e = off[u + 1];
  const int64_t k = b - (s / GV_C + u);
  r0 = s + k * GV_C;
  r1 = min(min(e, r0 + GV_C), F);
  return r0 < r1;
}

}  // namespace

__global__ void __launch_bounds__(64 * GV_W) k_gv_partial(const float* __restrict__ x, const int64_t* __restrict__ off,
                                                          int n_seg, int64_t F, int H, float4* __restrict__ part) {
  __shared__ float sh[3][GV_W][64];
  const int64_t b = blockIdx.x;
  int u;
  int64_t r0, r1;
  if (!gv_chunk(off, n_seg, F, b, u, r0, r1)) return;
  const int n = (int)(r1 - r0), lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int d = blockIdx.y * 64 + lane;
  const bool on = d < H;
  const float* p = x + r0 * (int64_t)H;  // uniform
  const uint32_t od = on ? (uint32_t)d : 0u;
  const float x0 = on ? p[od] : 0.f;
  float v[GV_U];
#pragma unroll
  for (int r = 0; r < GV_U; ++r)  // unconditional loads (rows past the chunk re-read its last row): all in flight
    v[r] = p[(uint32_t)min(w + r * GV_W, n - 1) * (uint32_t)H + od];
  float mean = 0.f, m2 = 0.f;
#pragma unroll
  for (int r = 0; r < GV_U; ++r) {
    if (w + r * GV_W < n) {
      const float inv = 1.f / (float)(r + 1);
      const float y = v[r] - x0, dl = y - mean;
      mean += dl * inv;
      m2 += dl * (y - mean);
    }
  }
  sh[0][w][lane] = (float)(w < n ? (n - w + GV_W - 1) / GV_W : 0);
  sh[1][w][lane] = mean;
  sh[2][w][lane] = m2;
  __syncthreads();
  if (w != 0 || !on) return;
  double tn = 0.0, tm = 0.0, t2 = 0.0;  // Chan et al. pairwise update, waves in order
  for (int k = 0; k < GV_W; ++k) {
    const double nb = sh[0][k][lane], mb = sh[1][k][lane];
    if (nb == 0.0) continue;
    const double nn = tn + nb, dl = mb - tm;
    tm += dl * (nb / nn);
    t2 += (double)sh[2][k][lane] + dl * dl * (tn * nb / nn);
    tn = nn;
  }
  part[b * H + d] = make_float4(x0, (float)tm, (float)t2, 0.f);
}

__global__ void __launch_bounds__(GV_FB * GV_FS) k_gv_finalize(const int64_t* __restrict__ off, int64_t nb, int H,
                                                               int n_bg, const float4* __restrict__ part,
                                                               const float* __restrict__ xmin,
                                                               const float* __restrict__ xmax,
                                                               const float* __restrict__ gv, float4* __restrict__ par) {
  __shared__ double sh[GV_FS][GV_FB];
  const int u = blockIdx.x / n_bg;
  const int j = threadIdx.x % GV_FB, sl = threadIdx.x / GV_FB;
  const int d = (blockIdx.x % n_bg) * GV_FB + j;
  const int64_t s = off[u], N = off[u + 1] - s;
  if (N <= 0) return;  // uniform over the workgroup
  const int64_t base = s / GV_C + u, nch = min((N + GV_C - 1) / GV_C, nb - base);
  const bool on = d < H;
  // pass 1: sum of the chunk sums
  double acc = 0.0;
  if (on) {
#pragma unroll 4
    for (int64_t k = sl; k < nch; k += GV_FS) {
      const float4 q = part[(base + k) * H + d];
      acc += (double)min((int64_t)GV_C, N - k * GV_C) * ((double)q.x + (double)q.y);
    }
  }
  sh[sl][j] = acc;
  __syncthreads();
  double mean = 0.0;
  for (int k = 0; k < GV_FS; ++k) mean += sh[k][j];
  mean /= (double)N;
  __syncthreads();
  // pass 2: M2 = sum_k (M2_k + n_k (mean_k - mean)^2)
  acc = 0.0;
  if (on) {
#pragma unroll 4
    for (int64_t k = sl; k < nch; k += GV_FS) {
      const float4 q = part[(base + k) * H + d];
      const double dl = ((double)q.x + (double)q.y) - mean;
      acc += (double)q.z + (double)min((int64_t)GV_C, N - k * GV_C) * dl * dl;
    }
  }
  sh[sl][j] = acc;
  __syncthreads();
  if (sl != 0 || !on) return;
  double m2 = 0.0;
  for (int k = 0; k < GV_FS; ++k) m2 += sh[k][j];
  const double lo = xmin[d], sc = (double)xmax[d] - lo, a = 0.5 * sc;
  const double vc = a * a * (m2 / (double)N);  // utterance variance of c = a x + const
  float4 q = make_float4(0.f, 0.f, __builtin_nanf(""), 0.f);  // mu_c = NaN marks a pass-through bin
  if (vc > 1e-8) {
    const float hi = (float)mean;
    q = make_float4(hi, (float)(mean - (double)hi), (float)((mean * 0.5 + 0.5) * sc + lo),
                    (float)(sqrt((double)gv[d] / vc) * a));
  }
  par[(int64_t)u * H + d] = q;
}

__global__ void __launch_bounds__(64 * GV_W) k_gv_apply(const float* __restrict__ x, const int64_t* __restrict__ off,
                                                        int n_seg, int64_t F, int H, const float* __restrict__ xmin,
                                                        const float* __restrict__ xmax, const float4* __restrict__ par,
                                                        float* __restrict__ out) {
  int u;
  int64_t r0, r1;
  if (!gv_chunk(off, n_seg, F, blockIdx.x, u, r0, r1)) return;
  const int d = blockIdx.y * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  if (d >= H) return;
  const int n = (int)(r1 - r0);
  const float lo = xmin[d], sc = xmax[d] - lo;
  const float4 q = par[(int64_t)u * H + d];
  const bool pass = isnan(q.z);
  const float* p = x + r0 * (int64_t)H;  // uniform
  float* po = out + r0 * (int64_t)H;
  float v[GV_U];
#pragma unroll
  for (int r = 0; r < GV_U; ++r) {
    const int i = w + r * GV_W;
    v[r] = i < n ? p[(uint32_t)i * (uint32_t)H + (uint32_t)d] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < GV_U; ++r) {
    const int i = w + r * GV_W;
    if (i >= n) break;
    const float c = (v[r] * .5f + .5f) * sc + lo;  // k_tanhize's expression: pass-through is its bytes
    po[(uint32_t)i * (uint32_t)H + (uint32_t)d] = pass ? c : q.z + q.w * ((v[r] - q.x) - q.y);
  }
}

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

int64_t gv_chunk_grid(int64_t F, int n_seg) { return F / GV_C + n_seg; }

int64_t gv_workspace_bytes(int64_t F, int n_seg, int H) {
  return align256(gv_chunk_grid(F, n_seg) * H * (int64_t)sizeof(float4)) + align256((int64_t)n_seg * H * sizeof(float4));
}

void launch_gv_postfilter(const float* x, const int64_t* off, int n_seg, int64_t F, int H, const float* xmin,
                          const float* xmax, const float* gv, float* out, void* ws, hipStream_t s) {
  const int64_t nb = gv_chunk_grid(F, n_seg);
  float4* part = (float4*)ws;
  float4* par = (float4*)((char*)ws + align256(nb * H * (int64_t)sizeof(float4)));
  const dim3 grid((unsigned)nb, (unsigned)((H + 63) / 64));
  const int n_bg = (H + GV_FB - 1) / GV_FB;
  hipLaunchKernelGGL(k_gv_partial, grid, dim3(64 * GV_W), 0, s, x, off, n_seg, F, H, part);
  hipLaunchKernelGGL(k_gv_finalize, dim3((unsigned)((int64_t)n_seg * n_bg)), dim3(GV_FB * GV_FS), 0, s, off, nb, H,
                     n_bg, part, xmin, xmax, gv, par);
  hipLaunchKernelGGL(k_gv_apply, grid, dim3(64 * GV_W), 0, s, x, off, n_seg, F, H, xmin, xmax, par, out);
}

}  // namespace vaenpvc
