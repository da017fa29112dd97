// gfx950_synth.hip -- WORLD-style waveform synthesis of the conversion path (the reference's convert.py:105-114 hands
// each converted utterance to pyworld.synthesize; pyworld is a CPU C library and is not available to this project).
// The algorithm is stated in DESIGN.md section 14 and restated in float64 NumPy by tests/world_ref.py.
//
// n_seg utterances back to back: utterance u is frames foff[u] .. foff[u+1] and samples soff[u] .. soff[u+1].  Four
// launches on the caller's stream, no host synchronisation, no allocation, no atomics:
//   k_synth_timebase  one workgroup per utterance: per-sample f0 (float64, no FMA contraction, so that the phase is the
//                     sequential float64 sum of tests/world_ref.py bit for bit), the phase scan (one lane adds, the
//                     workgroup computes the increments and detects the wraps), pulse compaction in sample order into
//                     the utterance's fixed slots base_u = floor(soff[u]*1000/fs) + u, capacity floor(S_u*1000/fs) + 1
//   k_synth_scan      one workgroup: exclusive prefix of the per-utterance pulse counts
//   k_synth_segment   grid-strided over the pulses, one workgroup per pulse: the 1024-sample segment r of the pulse with
//                     1024-point complex FFTs in LDS (radix-4 Stockham, 256 threads, one butterfly per thread and stage);
//                     the two cepstra share one FFT, the two minimum-phase spectra share one, the noise spectrum takes
//                     one and the periodic and aperiodic responses share the last inverse
//   k_synth_ola       one thread per output sample: binary search of the utterance's sorted pulse list, the covering
//                     segments summed in pulse order
// Every per-utterance quantity is computed from the utterance's own frames and samples, so its output is the same bytes
// whatever its neighbours or offset in the batch.  Every write is bounded by the slot capacity, the workspace and S,
// whatever the input values are (NaN and inf included) and even for offsets that break the caller's contract.
#include <cfloat>

#include "kernels.h"
#include "philox.h"

namespace vaenpvc {

namespace {

constexpr int SN = 1024;          // FFT size
constexpr int SH = SN / 2 + 1;    // bins (513)
constexpr int SY_T = 256;         // threads of the workgroup kernels
constexpr int TB_CH = 1024;       // samples per chunk of the phase scan
constexpr double TWO_PI = 6.283185307179586;  // == 2 * np.pi
constexpr double PI_D = 3.141592653589793;
constexpr int64_t SEG_GRID = 2048;  // workgroups of the segment kernel at most (grid-strided over the pulses)

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct SynthWs {
  int32_t* cnt;    // [n_seg] pulses kept per utterance
  int32_t* pre;    // [n_seg + 1] exclusive prefix of cnt
  int32_t* pidx;   // [n_slots] pulse sample, relative to the utterance's first sample
  float2* pinfo;   // [n_slots] (fractional shift x, voiced 1 / unvoiced 0)
  float* seg;      // [n_slots, SN] the pulse's segment r
};

SynthWs carve(void* ws, int n_seg, int64_t n_slots) {
  SynthWs w;
  char* p = (char*)ws;
  w.cnt = (int32_t*)p;
  p += align256((int64_t)n_seg * 4);
  w.pre = (int32_t*)p;
  p += align256((int64_t)(n_seg + 1) * 4);
  w.pidx = (int32_t*)p;
  p += align256(n_slots * 4);
  w.pinfo = (float2*)p;
  p += align256(n_slots * 8);
  w.seg = (float*)p;
  return w;
}

// utterance u's frame range [fo, fo + T) and sample range [so, so + S), clamped to the batch
__device__ __forceinline__ void utt_range(const int64_t* __restrict__ foff, const int64_t* __restrict__ soff, int u,
                                          int64_t F, int64_t Stot, int64_t& fo, int64_t& T, int64_t& so, int64_t& S) {
  fo = min(max(foff[u], (int64_t)0), F);
  T = min(max(foff[u + 1], fo), F) - fo;
  so = min(max(soff[u], (int64_t)0), Stot);
  S = min(max(soff[u + 1], so), Stot) - so;
}

// slot base and capacity of utterance u, never past n_slots
__device__ __forceinline__ void utt_slots(int64_t so, int64_t S, int u, int fs, int64_t n_slots, int64_t& base,
                                          int64_t& cap) {
  base = so * 1000 / fs + u;
  cap = min(S * 1000 / fs + 1, max(n_slots - base, (int64_t)0));
}

// coarse f0 / voicing at coarse index t (0..T; T is the extrapolated point)
__device__ __forceinline__ double cf0_at(const float* __restrict__ f0, int64_t fo, int64_t T, int64_t t, double lowest) {
#pragma clang fp contract(off)
  auto clean = [&](int64_t j) -> double {
    const double v = (double)f0[fo + j];
    return (isfinite(v) && v >= lowest) ? v : 0.0;
  };
  if (t < T) return clean(t);
  if (T == 1) return clean(0);
  return 2.0 * clean(T - 1) - clean(T - 2);
}

struct Coarse {
  double f_T, v_T;  // extrapolated point
};

__device__ __forceinline__ double cvuv_of(double cf) { return cf != 0.0 ? 1.0 : 0.0; }

// per-sample f0 (after the unvoiced value and the ceiling) and voicing of sample n
__device__ __forceinline__ double sample_f0(const float* __restrict__ f0, int64_t fo, int64_t T, const Coarse& cx,
                                            int64_t n, double fsd, double Pd, double lowest, bool& vuv) {
#pragma clang fp contract(off)  // the interpolation is tests/world_ref.py's float64 arithmetic, operation for operation
  const double pos = ((double)n / fsd) / Pd;
  const int64_t k = min((int64_t)floor(pos), T - 1);
  const double frac = pos - (double)k;
  const double c0 = cf0_at(f0, fo, T, k, lowest);
  const double c1 = (k + 1 < T) ? cf0_at(f0, fo, T, k + 1, lowest) : cx.f_T;
  const double v0 = cvuv_of(c0);
  const double v1 = (k + 1 < T) ? cvuv_of(c1) : cx.v_T;
  const double fi = c0 + (c1 - c0) * frac;
  const double vi = v0 + (v1 - v0) * frac;
  vuv = vi > 0.5;
  double f = vuv ? fi : 500.0;
  f = f < (double)VAENPVC_SYNTH_F0_CEIL ? f : (double)VAENPVC_SYNTH_F0_CEIL;
  return f;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {  // a * conj(b)
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// 1024-point complex FFT (INV: positive exponent, unnormalised) of x, radix-4 Stockham, ping-pong x <-> y; all SY_T
// threads; the caller has synchronised after writing x.  Returns the buffer holding the result (y: five stages).
// tw[m] = exp(-2 pi i m / SN).
template <bool INV>
__device__ float2* fft1024(float2* x, float2* y, const float2* __restrict__ tw) {
  const int i = threadIdx.x;
#pragma unroll
  for (int p = 1; p < SN; p <<= 2) {
    const int k = i & (p - 1);
    float2 a0 = x[i], a1 = x[i + SN / 4], a2 = x[i + SN / 2], a3 = x[i + 3 * SN / 4];
    if (p > 1) {
      const int st = (SN / (4 * p)) * k;
      if (INV) {
        a1 = cmulc(a1, tw[st]);
        a2 = cmulc(a2, tw[2 * st]);
        a3 = cmulc(a3, tw[3 * st]);
      } else {
        a1 = cmul(a1, tw[st]);
        a2 = cmul(a2, tw[2 * st]);
        a3 = cmul(a3, tw[3 * st]);
      }
    }
    const float2 v0 = make_float2(a0.x + a2.x, a0.y + a2.y), v1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 v2 = make_float2(a1.x + a3.x, a1.y + a3.y);
    const float2 d = make_float2(a1.x - a3.x, a1.y - a3.y);
    const float2 v3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);  // (+i) d  /  (-i) d
    const int j = ((i - k) << 2) + k;
    y[j] = make_float2(v0.x + v2.x, v0.y + v2.y);
    y[j + p] = make_float2(v1.x + v3.x, v1.y + v3.y);
    y[j + 2 * p] = make_float2(v0.x - v2.x, v0.y - v2.y);
    y[j + 3 * p] = make_float2(v1.x - v3.x, v1.y - v3.y);
    __syncthreads();
    float2* t = x;
    x = y;
    y = t;
  }
  return x;
}

// fixed-order sum over the workgroup (every thread gets it); red: SY_T / 64 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < SY_T / 64; ++w) s += red[w];
  return s;
}

}  // namespace

__global__ void __launch_bounds__(SY_T) k_synth_timebase(const float* __restrict__ f0, const int64_t* __restrict__ foff,
                                                         const int64_t* __restrict__ soff, int64_t F, int64_t Stot,
                                                         int fs, double frame_period_ms, int64_t n_slots,
                                                         int32_t* __restrict__ cnt, int32_t* __restrict__ pidx,
                                                         float2* __restrict__ pinfo) {
#pragma clang fp contract(off)
  __shared__ double inc[TB_CH], ph[TB_CH];  // increments, phases
  __shared__ int wcount[SY_T / 64];
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t fo, T, so, S, base, cap;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  utt_slots(so, S, u, fs, n_slots, base, cap);
  if (T < 1 || S < 2 || cap <= 0) {
    if (tid == 0) cnt[u] = 0;
    return;
  }
  const double fsd = (double)fs, Pd = frame_period_ms / 1000.0, lowest = fsd / SN + 1.0;
  Coarse cx;
  cx.f_T = cf0_at(f0, fo, T, T, lowest);
  cx.v_T = (T == 1) ? cvuv_of(cx.f_T) : 2.0 * cvuv_of(cf0_at(f0, fo, T, T - 1, lowest)) -
                                            cvuv_of(cf0_at(f0, fo, T, T - 2, lowest));
  double carry = 0.0, w_prev = 0.0;
  int64_t count = 0;
  for (int64_t c0 = 0; c0 < S; c0 += TB_CH) {
    const int nc = (int)min((int64_t)TB_CH, S - c0);
    for (int l = tid; l < nc; l += SY_T) {
      bool v;
      const double f = sample_f0(f0, fo, T, cx, c0 + l, fsd, Pd, lowest, v);
      inc[l] = TWO_PI * f / fsd;
    }
    __syncthreads();
    if (tid == 0) {  // the sequential float64 sum (np.cumsum)
      double acc = carry;
      int l = 0;
      for (; l + 8 <= nc; l += 8) {
        double t[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) t[r] = inc[l + r];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          acc = acc + t[r];
          ph[l + r] = acc;
        }
      }
      for (; l < nc; ++l) {
        acc = acc + inc[l];
        ph[l] = acc;
      }
    }
    __syncthreads();
    carry = ph[nc - 1];
    for (int l0 = 0; l0 < nc; l0 += SY_T) {  // rounds in sample order: the compaction keeps pulses sorted
      const int l = l0 + tid;
      const int64_t n = c0 + l;  // a pulse at sample n - 1 when the wrapped phase jumps between n - 1 and n
      bool hit = false;
      double w0 = 0.0, w1 = 0.0;
      if (l < nc && n >= 1) {
        w1 = fmod(ph[l], TWO_PI);
        w0 = l > 0 ? fmod(ph[l - 1], TWO_PI) : w_prev;
        hit = fabs(w1 - w0) > PI_D;
      }
      const uint64_t m = __ballot(hit);
      if (lane == 0) wcount[wv] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < SY_T / 64; ++w) {
        before += w < wv ? wcount[w] : 0;
        total += wcount[w];
      }
      if (hit) {
        const int64_t slot = count + before + __popcll(m & ((1ull << lane) - 1ull));
        if (slot < cap) {
          bool v;
          sample_f0(f0, fo, T, cx, n - 1, fsd, Pd, lowest, v);
          const double x = -(w0 - TWO_PI) / (w1 - (w0 - TWO_PI));
          pidx[base + slot] = (int32_t)(n - 1);
          pinfo[base + slot] = make_float2((float)x, v ? 1.f : 0.f);
        }
      }
      count += total;
      __syncthreads();
    }
    w_prev = fmod(ph[nc - 1], TWO_PI);
    __syncthreads();
  }
  if (tid == 0) cnt[u] = (int32_t)min(count, cap);
}

__global__ void __launch_bounds__(SY_T) k_synth_scan(const int32_t* __restrict__ cnt, int n_seg,
                                                     int32_t* __restrict__ pre) {
  __shared__ int wsum[SY_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int run = 0;
  for (int b = 0; b < n_seg; b += SY_T) {
    const int v = b + tid < n_seg ? cnt[b + tid] : 0;
    int s = v;  // inclusive wave scan
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(s, o, 64);
      if (lane >= o) s += t;
    }
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SY_T / 64; ++w) {
      before += w < wv ? wsum[w] : 0;
      total += wsum[w];
    }
    if (b + tid < n_seg) pre[b + tid] = run + before + s - v;
    run += total;
    __syncthreads();
  }
  if (tid == 0) pre[n_seg] = run;
}

__global__ void __launch_bounds__(SY_T) k_synth_segment(const float* __restrict__ sp, const float* __restrict__ en,
                                                        const float* __restrict__ ap, const int64_t* __restrict__ foff,
                                                        const int64_t* __restrict__ soff, int n_seg, int64_t F,
                                                        int64_t Stot, int fs, double frame_period_ms, int64_t n_slots,
                                                        PhiloxKey key, SynthWs w) {
  __shared__ float2 bA[SN], bB[SN], tw[SN];
  __shared__ float2 sNz[SH];
  __shared__ float sE[SH], sR[SH], sQ[SH];
  __shared__ float red[SY_T / 64];
  const int tid = threadIdx.x;
  for (int m = tid; m < SN; m += SY_T) {
    float s, c;
    sincospif(-2.0f * (float)m / (float)SN, &s, &c);
    tw[m] = make_float2(c, s);
  }
  const int total = w.pre[n_seg];
  const double fsd = (double)fs, Pd = frame_period_ms / 1000.0;
  for (int g = blockIdx.x; g < total; g += gridDim.x) {
    int lo = 0, hi = n_seg - 1;  // utterance: largest u with pre[u] <= g
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (w.pre[mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    const int u = lo, p = g - w.pre[u];
    int64_t fo, T, so, S, base, cap;
    utt_range(foff, soff, u, F, Stot, fo, T, so, S);
    utt_slots(so, S, u, fs, n_slots, base, cap);
    const int64_t slot = base + p;
    float* out = w.seg + slot * SN;
    const int ncnt = w.cnt[u];
    const int ip = w.pidx[slot];
    const int ns = p + 1 < ncnt ? min(w.pidx[slot + 1] - ip, SN) : 0;
    if (ns <= 0 || T < 1) {  // the last pulse (and a degenerate list) contributes nothing
      for (int i = tid; i < SN; i += SY_T) out[i] = 0.f;
      continue;
    }
    const float2 info = w.pinfo[slot];
    const bool voiced = info.y != 0.f;
    // ---- envelope E, ratio R = c^2 and 1 - R = q (2 - q) at the pulse's frame position (q = 1 - c, exact near c = 1)
    const double q = ((double)ip / fsd) / Pd;
    const int64_t fl = min(T - 1, (int64_t)floor(q)), ce = min(T - 1, (int64_t)ceil(q));
    const float af = (float)(q - (double)fl), bf = 1.f - af;
    const int64_t rl = fo + max(fl, (int64_t)0), rc = fo + max(ce, (int64_t)0);
    const float el = en[rl], ec = en[rc];
    const float* spl = sp + rl * SH;
    const float* spc = sp + rc * SH;
    const float* apl = ap + rl * SH;
    const float* apc = ap + rc * SH;
    for (int k = tid; k < SH; k += SY_T) {
      const float s0 = fabsf(el * exp10f(spl[k])), s1 = fabsf(ec * exp10f(spc[k]));
      const float a0 = apl[k], a1 = apc[k];
      const float c = bf * fminf(fmaxf(a0, 0.001f), 1.f) + af * fminf(fmaxf(a1, 0.001f), 1.f);
      const float qq = bf * fminf(fmaxf(1.f - a0, 1e-12f), 0.999f) + af * fminf(fmaxf(1.f - a1, 1e-12f), 0.999f);
      sE[k] = bf * s0 + af * s1;
      sR[k] = c * c;
      sQ[k] = qq * (2.f - qq);
    }
    // ---- noise: philox normals (ip - i_0) + j, j < ns, mean removed, zero-padded; its spectrum -> sNz
    const int i0 = w.pidx[base];
    const uint64_t e0 = (uint64_t)(int64_t)(ip - i0);
    float z[SN / SY_T], zs = 0.f;
#pragma unroll
    for (int m = 0; m < SN / SY_T; ++m) {
      const int j = tid + m * SY_T;
      z[m] = j < ns ? philox_normal(key, e0 + (uint64_t)j) : 0.f;
      zs += z[m];
    }
    const float mean = block_sum(zs, red) / (float)ns;
#pragma unroll
    for (int m = 0; m < SN / SY_T; ++m) {
      const int j = tid + m * SY_T;
      bA[j] = make_float2(j < ns ? z[m] - mean : 0.f, 0.f);
    }
    __syncthreads();
    const float2* Z = fft1024<false>(bA, bB, tw);
    for (int k = tid; k < SH; k += SY_T) sNz[k] = Z[k];
    __syncthreads();  // sE / sR / sQ complete; Z (in bB) consumed
    const bool per_on = voiced && sR[0] <= 0.999f;
    // ---- the two log-amplitudes as one complex sequence (periodic + i aperiodic), mirrored; one FFT -> N * cepstra
    for (int k = tid; k < SH; k += SY_T) {
      const float E = sE[k], R = sR[k];
      const float lp = per_on ? 0.5f * logf(fmaxf(E * sQ[k] + 1e-12f, FLT_MIN)) : 0.f;
      const float la = 0.5f * logf(fmaxf(voiced ? E * R : E, FLT_MIN));
      bA[k] = make_float2(lp, la);
      if (k > 0 && k < SN / 2) bA[SN - k] = make_float2(lp, la);
    }
    __syncthreads();
    float2* C = fft1024<false>(bA, bB, tw);  // real even inputs: FFT = N * IFFT
    // fold (causal cepstrum) and scale by 1 / N, in place
    for (int i = tid; i < SN; i += SY_T) {
      const float s = i == 0 || i == SN / 2 ? 1.f / SN : (i < SN / 2 ? 2.f / SN : 0.f);
      C[i] = make_float2(C[i].x * s, C[i].y * s);
    }
    __syncthreads();
    float2* W = fft1024<false>(C, C == bA ? bB : bA, tw);
    float2* Y = W == bA ? bB : bA;
    // ---- split the two spectra, exponentiate, delay the periodic one, multiply the aperiodic one with the noise;
    // Y = P + i A over all N bins (Hermitian P, A; imaginary parts of bins 0 and N/2 dropped)
    for (int k = tid; k < SH; k += SY_T) {
      const float2 a = W[k], b = W[(SN - k) & (SN - 1)];
      const float2 cp = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));   // (W[k] + conj W[N-k]) / 2
      const float2 ca = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));  // (W[k] - conj W[N-k]) / 2i
      float s, c;
      float2 P = make_float2(0.f, 0.f);
      if (per_on) {
        const float mp = expf(cp.x);
        sincosf(cp.y, &s, &c);
        const float2 Mp = make_float2(mp * c, mp * s);
        sincospif(-2.f * ((float)k * info.x) / (float)SN, &s, &c);
        P = cmul(Mp, make_float2(c, s));
      }
      const float ma = expf(ca.x);
      sincosf(ca.y, &s, &c);
      float2 A = cmul(sNz[k], make_float2(ma * c, ma * s));
      if (k == 0 || k == SN / 2) {
        P.y = 0.f;
        A.y = 0.f;
      }
      Y[k] = make_float2(P.x - A.y, P.y + A.x);
      if (k > 0 && k < SN / 2) Y[SN - k] = make_float2(P.x + A.y, A.x - P.y);
    }
    __syncthreads();
    const float2* yt = fft1024<true>(Y, W, tw);  // yt[n] = (per[n], aper[n]), before the fftshift
    // ---- fftshift, DC removal of the periodic response, r = (per sqrt(ns) + aper) / N
    float dsum = 0.f;
    for (int m = tid; m < SN / 2; m += SY_T) dsum += yt[m].x;  // sum over shifted indices >= N/2
    const float d = block_sum(dsum, red);
    const float sq = sqrtf((float)ns);
    for (int i = tid; i < SN; i += SY_T) {
      const float2 v = yt[(i + SN / 2) & (SN - 1)];
      const int h = i < SN / 2 ? i : SN - 1 - i;
      const float wd = (0.5f - 0.5f * cospif(2.f * (float)(h + 1) / (float)(SN + 1))) * (1.f / 512.5f);
      float per = 0.f;
      if (per_on) per = (i < SN / 2 ? 0.f : v.x) - d * wd;
      out[i] = (per * sq + v.y) * (1.f / SN);
    }
    __syncthreads();  // LDS reused by the next pulse
  }
}

__global__ void __launch_bounds__(SY_T) k_synth_ola(const int64_t* __restrict__ foff, const int64_t* __restrict__ soff,
                                                    int n_seg, int64_t F, int64_t Stot, int fs, int64_t n_slots,
                                                    SynthWs w, float* __restrict__ y) {
  const int64_t n = (int64_t)blockIdx.x * SY_T + threadIdx.x;
  if (n >= Stot) return;
  int lo = 0, hi = n_seg - 1;  // utterance: largest u with soff[u] <= n
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (soff[mid] <= n) lo = mid;
    else hi = mid - 1;
  }
  const int u = lo;
  int64_t fo, T, so, S, base, cap;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  utt_slots(so, S, u, fs, n_slots, base, cap);
  const int64_t nl = n - so;
  float acc = 0.f;
  if (nl >= 0 && nl < S) {
    const int c = w.cnt[u];
    const int32_t* pi = w.pidx + base;
    int a = 0, b = c;  // first pulse with i_p >= nl - N/2
    while (a < b) {
      const int mid = (a + b) >> 1;
      if ((int64_t)pi[mid] < nl - SN / 2) a = mid + 1;
      else b = mid;
    }
    for (int p = a; p < c && (int64_t)pi[p] <= nl + SN / 2 - 1; ++p)
      acc += w.seg[(base + p) * SN + (nl - pi[p] + SN / 2 - 1)];
  }
  y[n] = acc;
}

int64_t synth_slots(int n_seg, int64_t S, int fs) { return S * 1000 / fs + n_seg; }

int64_t synth_workspace_bytes(int n_seg, int64_t S, int fs) {
  const int64_t ns = synth_slots(n_seg, S, fs);
  return align256((int64_t)n_seg * 4) + align256((int64_t)(n_seg + 1) * 4) + align256(ns * 4) + align256(ns * 8) +
         ns * SN * (int64_t)sizeof(float);
}

void launch_synthesize(const float* f0, const float* sp, const float* en, const float* ap, const int64_t* foff,
                       const int64_t* soff, int n_seg, int64_t F, int64_t S, int fs, double frame_period_ms,
                       uint64_t seed, float* y, void* ws, hipStream_t s) {
  const int64_t n_slots = synth_slots(n_seg, S, fs);
  const SynthWs w = carve(ws, n_seg, n_slots);
  PhiloxKey key{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u, nullptr};
  hipLaunchKernelGGL(k_synth_timebase, dim3((unsigned)n_seg), dim3(SY_T), 0, s, f0, foff, soff, F, S, fs,
                     frame_period_ms, n_slots, w.cnt, w.pidx, w.pinfo);
  hipLaunchKernelGGL(k_synth_scan, dim3(1), dim3(SY_T), 0, s, w.cnt, n_seg, w.pre);
  hipLaunchKernelGGL(k_synth_segment, dim3((unsigned)min(n_slots, SEG_GRID)), dim3(SY_T), 0, s, sp, en, ap, foff, soff,
                     n_seg, F, S, fs, frame_period_ms, n_slots, key, w);
  if (S > 0)
    hipLaunchKernelGGL(k_synth_ola, dim3((unsigned)((S + SY_T - 1) / SY_T)), dim3(SY_T), 0, s, foff, soff, n_seg, F, S,
                       fs, n_slots, w, y);
}

}  // namespace vaenpvc
