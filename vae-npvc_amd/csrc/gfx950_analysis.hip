// gfx950_analysis.hip -- WORLD-style feature analysis (the reference's analyzer.py:25-47 runs pyworld's
// dio -> stonemask -> cheaptrick -> d4c on every wav; pyworld is a CPU C library and is not available to this project).
// The algorithm is stated in DESIGN.md section 15 and restated in float64 NumPy by tests/world_analysis_ref.py.
//
// n_seg utterances back to back: utterance u is samples soff[u] .. soff[u+1] of x and frames foff[u] .. foff[u+1] of
// the outputs.  Seven launches on the caller's stream, no host synchronisation, no allocation, no atomics:
//   k_an_taps     one workgroup per band: the combined low-cut (50 Hz) x band-pass (Nuttall x cos) filter, float64
//   k_an_mean     one workgroup per utterance: the mean of DIO's y = [x, 0] (fixed-order float64 sum)
//   k_an_band     one thread per (band, band sample): the direct FIR over y - mean, float64, taps in LDS
//   k_an_events   one workgroup per (utterance, band): the four fine-edge series (negative- and positive-going zero
//                 crossings, peaks, dips) compacted in sample order by wave ballots
//   k_an_cand     one thread per frame: the four interpolated interval series, candidate and score per band, best band
//   k_an_fix      one thread per utterance: FixF0Contour (sequential over frames)
//   k_an_frame    one workgroup per frame: StoneMask, CheapTrick, D4C's LoveTrain and body, the record's sp / en, with
//                 power-of-two float64 complex FFTs (128 .. 2048 points, radix-2 Stockham) in LDS
// All arithmetic is float64 (the outputs are stored as float32).  Every decision is evaluated with the restatement's
// operations in its order (no FMA contraction), every sum has a fixed order, and every per-utterance quantity reads only
// the utterance's own samples and frames: an utterance's outputs are the same bytes alone or anywhere in a batch.
// Every write is bounded by the workspace and the output shapes whatever the input values (NaN and inf included).
#include <cfloat>

#include "kernels.h"

namespace vaenpvc {

namespace {

#pragma clang fp contract(off)

constexpr int AT = 256;           // threads of every workgroup kernel
constexpr int NMAX = 2048;        // largest FFT
constexpr int LC_C = 320;         // low-cut half length round(16000 / 50)
constexpr int TAPMAX = 2 * (LC_C + 320) + 1;  // combined filter: band-pass half length <= round(2 fs / 100.4) = 319
constexpr int SCR = 1536;         // mirrored-cumsum scratch of the linear smoothing (<= 1024 + 2 * 124 + 1 values)
constexpr int NCT = 1024;         // CheapTrick FFT size
constexpr int HB = NCT / 2 + 1;   // 513 bins
constexpr double PI = 3.141592653589793;
constexpr double SAFE = 1e-12;
constexpr double EPSD = 2.220446049250313e-16;
constexpr double MAXV = 100000.0;

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

__device__ __forceinline__ int mround(double v) { return v > 0 ? (int)(v + 0.5) : (int)(v - 0.5); }

__device__ __forceinline__ void utt_range(const int64_t* __restrict__ foff, const int64_t* __restrict__ soff, int u,
                                          int64_t F, int64_t Stot, int64_t& fo, int64_t& T, int64_t& so, int64_t& S) {
  fo = min(max(foff[u], (int64_t)0), F);
  T = min(max(foff[u + 1], fo), F) - fo;
  so = min(max(soff[u], (int64_t)0), Stot);
  S = min(max(soff[u + 1], so), Stot) - so;
}

__device__ __forceinline__ double band_f0(double f0_floor, int b) { return f0_floor * pow(2.0, (b + 1) / 2.0); }

// fixed-order sum over the workgroup (every thread gets it); red: AT / 64 doubles of LDS
__device__ __forceinline__ double bsum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < AT / 64; ++w) s += red[w];
  return s;
}

// n-point complex FFT (INV: positive exponent, unnormalised) of x, radix-2 Stockham, ping-pong x <-> y; the caller has
// synchronised after writing x.  Returns the buffer holding the result.  tw[m] = exp(-2 pi i m / NMAX), m < NMAX / 2.
template <bool INV>
__device__ double2* fftd(double2* x, double2* y, int logn, const double2* __restrict__ tw) {
  const int n = 1 << logn, half = n >> 1;
  for (int s = 0; s < logn; ++s) {
    const int ns = 1 << s;
    for (int j = threadIdx.x; j < half; j += AT) {
      const int k = j & (ns - 1);
      const double2 v0 = x[j];
      double2 v1 = x[j + half];
      const double2 w = tw[k * (NMAX / 2 / ns)];
      const double wy = INV ? -w.y : w.y;
      v1 = make_double2(v1.x * w.x - v1.y * wy, v1.x * wy + v1.y * w.x);
      const int d = ((j - k) << 1) + k;
      y[d] = make_double2(v0.x + v1.x, v0.y + v1.y);
      y[d + ns] = make_double2(v0.x - v1.x, v0.y - v1.y);
    }
    __syncthreads();
    double2* t = x;
    x = y;
    y = t;
  }
  return x;
}

// the two real spectra packed in Z = FFT(a + i b): A[k] = (Z[k] + conj Z[n-k]) / 2, B[k] = (Z[k] - conj Z[n-k]) / 2i
__device__ __forceinline__ void unpack2(const double2* Z, int n, int k, double2& A, double2& B) {
  const double2 a = Z[k], b = Z[(n - k) & (n - 1)];
  A = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
  B = make_double2(0.5 * (a.y + b.y), -0.5 * (a.x - b.x));
}

__device__ __forceinline__ double xs_at(const float* __restrict__ x, int64_t so, int64_t S, int64_t j) {
  return S > 0 ? (double)x[so + min(max(j, (int64_t)0), S - 1)] : 0.0;
}

// common.cpp GetWindowedWaveform without the randn() safeguard, written to dst[j * stride] for j < N (zero beyond the
// window).  kind 0: Hanning, 1: Blackman.  Returns 2h + 1.
__device__ int windowed(const float* __restrict__ x, int64_t so, int64_t S, double t, double f, int kind,
                        double ratio, int fs, int N, double* dst, int stride, double* red) {
  const int h = mround(ratio * fs / f / 2.0);
  const int n = min(2 * h + 1, N);
  const int64_t origin = mround(t * fs + 0.001);
  double sw = 0.0, sx = 0.0;
  for (int j = threadIdx.x; j < N; j += AT) {
    double v = 0.0;
    if (j < n) {
      const int k = j - h;
      const double pos = (2.0 * k / ratio) / fs;
      const double w = kind == 0 ? 0.5 * cos(PI * pos * f) + 0.5
                                 : 0.42 + 0.5 * cos(PI * pos * f) + 0.08 * cos(PI * pos * f * 2);
      v = xs_at(x, so, S, origin + k) * w;
      sw += w;
      sx += v;
    }
    dst[j * stride] = v;
  }
  sx = bsum(sx, red);
  sw = bsum(sw, red);
  const double coef = sx / sw;
  for (int j = threadIdx.x; j < n; j += AT) {
    const int k = j - h;
    const double pos = (2.0 * k / ratio) / fs;
    const double w = kind == 0 ? 0.5 * cos(PI * pos * f) + 0.5
                               : 0.42 + 0.5 * cos(PI * pos * f) + 0.08 * cos(PI * pos * f * 2);
    dst[j * stride] = dst[j * stride] - w * coef;
  }
  __syncthreads();
  return n;
}

// DCCorrection in place on P [N/2 + 1]
__device__ void dc_correction(double* P, double f0, int fs, int N) {
  const int ul = 2 + (int)(f0 * N / fs);
  double v = 0.0;
  const int i = threadIdx.x;
  const bool on = i < ul - 1 && i <= N / 2;
  if (on) {
    const double q = (i * (double)fs / N - f0) / (-(double)fs / N);
    const int b = min(max((int)q, 0), N / 2 - 1);
    const double dy = b < ul ? P[b + 1] - P[b] : 0.0;
    v = P[i] + (P[b] + dy * (q - b));
  }
  __syncthreads();
  if (on) P[i] = v;
  __syncthreads();
}

// LinearSmoothing of in [N/2 + 1] -> out (may alias in); scr: SCR doubles
__device__ void linear_smoothing(const double* in, double* out, double width, int fs, int N, double* scr,
                                 double* red) {
  const int bd = (int)(width * N / fs) + 1, half = N / 2;
  const int M = min(half + 2 * bd + 1, SCR);
  const double df = (double)fs / N;
  for (int i = threadIdx.x; i < M; i += AT) {
    int src;
    if (i < bd) src = bd - i;
    else if (i < half + bd) src = i - bd;
    else src = half - (i - (half + bd));
    scr[i] = in[min(max(src, 0), half)] * fs / N;
  }
  __syncthreads();
  // inclusive scan: chunks of CH consecutive values per thread, then the thread totals
  constexpr int CH = SCR / AT;
  const int c0 = threadIdx.x * CH;
  double loc[CH];
  double run = 0.0;
#pragma unroll
  for (int r = 0; r < CH; ++r) {
    const double v = c0 + r < M ? scr[c0 + r] : 0.0;
    run = r == 0 ? v : run + v;
    loc[r] = run;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double s = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  __syncthreads();
  if (lane == 63) red[wv] = s;
  __syncthreads();
  double before = s - run;
  for (int w = 0; w < wv; ++w) before += red[w];
#pragma unroll
  for (int r = 0; r < CH; ++r)
    if (c0 + r < M) scr[c0 + r] = before + loc[r];
  __syncthreads();
  const double x0 = -(bd - 0.5) * fs / N;
  double res[(NMAX / 2 + 1 + AT - 1) / AT];
  int m = 0;
  for (int i = threadIdx.x; i <= half; i += AT, ++m) {
    const double fl = (double)i / N * fs - width / 2.0;
    const double fh = fl + width;
    const double vl = (fl - x0) / df, vh = (fh - x0) / df;
    const int bl = min(max((int)vl, 0), M - 1), bh = min(max((int)vh, 0), M - 1);
    const double dl = bl + 1 < M ? scr[bl + 1] - scr[bl] : 0.0;
    const double dh = bh + 1 < M ? scr[bh + 1] - scr[bh] : 0.0;
    const double lo = scr[bl] + dl * (vl - bl), hi = scr[bh] + dh * (vh - bh);
    res[m] = (hi - lo) / width;
  }
  __syncthreads();
  m = 0;
  for (int i = threadIdx.x; i <= half; i += AT, ++m) out[i] = res[m];
  __syncthreads();
}

struct FrameLds {
  double2 bA[NMAX], bB[NMAX], tw[NMAX / 2];
  double r0[SCR], r1[SCR], r2[SCR];
  double red[AT / 64];
};

// StoneMask's FixF0 over the packed power / numerator arrays (p = r0, num = r1)
__device__ double fix_f0(const double* P, const double* num, int N, int fs, double f0, int nh) {
  double ns = 0.0, ds = 0.0;
  for (int i = 0; i < nh; ++i) {
    const int k = min(max(mround(f0 * N / fs * (i + 1)), 0), N / 2);
    const double inst = P[k] == 0.0 ? 0.0 : k * (double)fs / N + num[k] / P[k] * fs / 2.0 / PI;
    const double a = sqrt(P[k]);
    ns += a * inst;
    ds += a * (i + 1.0);
  }
  return ns / (ds + SAFE);
}

__device__ double stonemask(FrameLds& L, const float* __restrict__ x, int64_t so, int64_t S, int fs, double t,
                            double f0, bool& back) {
  back = false;
  if (!(f0 > 40.0) || f0 > fs / 12.0) return 0.0;
  const int h = (int)(1.5 * fs / f0 + 1.0);
  const int n = 2 * h + 1;
  const double wl = n / (double)fs;
  const int logn = 2 + (31 - __clz(n));
  if (logn > 11) return 0.0;  // f0 < 47 Hz: never produced by DIO (f0_floor >= 71)
  const int N = 1 << logn;
  for (int j = threadIdx.x; j < N; j += AT) {
    double a = 0.0, b = 0.0;
    if (j < n) {
      auto mw = [&](int jj) {
        const double bt = (double)(-h + jj) / fs;
        const int raw = mround((t + bt) * fs);
        const double tmp = (raw - 1.0) / fs - t;
        return 0.42 + 0.5 * cos(2.0 * PI * tmp / wl) + 0.08 * cos(4.0 * PI * tmp / wl);
      };
      const double bt = (double)(-h + j) / fs;
      const int raw = mround((t + bt) * fs);
      const double xv = xs_at(x, so, S, (int64_t)raw - 1);
      const double dw = j == 0 ? -mw(1) / 2.0 : (j == n - 1 ? mw(n - 2) / 2.0 : -(mw(j + 1) - mw(j - 1)) / 2.0);
      a = xv * mw(j);
      b = xv * dw;
    }
    L.bA[j] = make_double2(a, b);
  }
  __syncthreads();
  const double2* Z = fftd<false>(L.bA, L.bB, logn, L.tw);
  for (int k = threadIdx.x; k <= N / 2; k += AT) {
    double2 M, D;
    unpack2(Z, N, k, M, D);
    L.r1[k] = M.x * D.y - M.y * D.x;
    L.r0[k] = M.x * M.x + M.y * M.y;
  }
  __syncthreads();
  const double tent = fix_f0(L.r0, L.r1, N, fs, f0, 2);
  const double mean = (tent <= 0.0 || tent > f0 * 2) ? 0.0 : fix_f0(L.r0, L.r1, N, fs, tent, 6);
  __syncthreads();
  back = !(fabs(mean - f0) <= f0 * 0.2);
  return back ? f0 : mean;
}

// CheapTrick: linear envelope -> L.r0 [513]
__device__ void cheaptrick(FrameLds& L, const float* __restrict__ x, int64_t so, int64_t S, int fs, double t,
                           double f0) {
  const double f = f0 <= 3.0 * fs / (NCT - 3.0) ? 500.0 : f0;
  const int h = mround(1.5 * fs / f);
  const int n = min(2 * h + 1, NCT);
  const int64_t origin = mround(t * fs + 0.001);
  double ww = 0.0;
  for (int j = threadIdx.x; j < n; j += AT) {
    const double w = 0.5 * cos(PI * ((j - h) / 1.5 / fs) * f) + 0.5;
    ww += w * w;
  }
  const double nrm = sqrt(bsum(ww, L.red));
  double sw = 0.0, sx = 0.0;
  for (int j = threadIdx.x; j < NCT; j += AT) {
    double v = 0.0;
    if (j < n) {
      const double w = (0.5 * cos(PI * ((j - h) / 1.5 / fs) * f) + 0.5) / nrm;
      v = xs_at(x, so, S, origin + (j - h)) * w;
      sw += w;
      sx += v;
    }
    L.bA[j] = make_double2(v, 0.0);
  }
  sx = bsum(sx, L.red);
  sw = bsum(sw, L.red);
  const double coef = sx / sw;
  for (int j = threadIdx.x; j < n; j += AT) {
    const double w = (0.5 * cos(PI * ((j - h) / 1.5 / fs) * f) + 0.5) / nrm;
    L.bA[j].x = L.bA[j].x - w * coef;
  }
  __syncthreads();
  constexpr int LG = 10;
  const double2* X = fftd<false>(L.bA, L.bB, LG, L.tw);
  for (int k = threadIdx.x; k < HB; k += AT) L.r0[k] = X[k].x * X[k].x + X[k].y * X[k].y;
  __syncthreads();
  dc_correction(L.r0, f, fs, NCT);
  linear_smoothing(L.r0, L.r0, f * 2.0 / 3.0, fs, NCT, L.r2, L.red);
  // log, mirrored -> one FFT (real, even) -> lifters -> inverse FFT -> exp
  for (int k = threadIdx.x; k < HB; k += AT) {
    const double lg = log(L.r0[k] + EPSD);
    L.bA[k] = make_double2(lg, 0.0);
    if (k > 0 && k < NCT / 2) L.bA[NCT - k] = make_double2(lg, 0.0);
  }
  __syncthreads();
  double2* C = fftd<false>(L.bA, L.bB, LG, L.tw);
  double2* W = C == L.bA ? L.bB : L.bA;
  constexpr double Q1 = -0.15;
  for (int k = threadIdx.x; k < HB; k += AT) {
    double sl = 1.0, cl = (1.0 - 2.0 * Q1) + 2.0 * Q1;
    if (k > 0) {
      const double q = (double)k / fs;
      sl = sin(PI * f * q) / (PI * f * q);
      cl = (1.0 - 2.0 * Q1) + 2.0 * Q1 * cos(2.0 * PI * q * f);
    }
    const double v = C[k].x * sl * cl / NCT;
    W[k] = make_double2(v, 0.0);
    if (k > 0 && k < NCT / 2) W[NCT - k] = make_double2(v, 0.0);
  }
  __syncthreads();
  const double2* E = fftd<true>(W, C, LG, L.tw);
  for (int k = threadIdx.x; k < HB; k += AT) L.r1[k] = exp(E[k].x);
  __syncthreads();
  for (int k = threadIdx.x; k < HB; k += AT) L.r0[k] = L.r1[k];
  __syncthreads();
}

__device__ double lovetrain(FrameLds& L, const float* __restrict__ x, int64_t so, int64_t S, int fs, double t,
                            double f0) {
  if (f0 == 0.0) return 0.0;
  const double f = fmax(f0, 40.0);
  constexpr int LG = 11, N = 1 << LG;
  const int b0 = (int)ceil(100.0 * N / fs), b1 = (int)ceil(4000.0 * N / fs), b2 = (int)ceil(7900.0 * N / fs);
  windowed(x, so, S, t, f, 1, 3.0, fs, N, &L.bA[0].x, 2, L.red);
  for (int j = threadIdx.x; j < N; j += AT) L.bA[j].y = 0.0;
  __syncthreads();
  const double2* X = fftd<false>(L.bA, L.bB, LG, L.tw);
  double s1 = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k <= b2; k += AT) {
    const double p = k <= b0 ? 0.0 : X[k].x * X[k].x + X[k].y * X[k].y;
    s2 += p;
    if (k <= b1) s1 += p;
  }
  s1 = bsum(s1, L.red);
  s2 = bsum(s2, L.red);
  return s2 == 0.0 ? 0.0 : s1 / s2;
}

// D4C's GetCentroid at time t, accumulated into acc [N/2 + 1]
__device__ void centroid(FrameLds& L, const float* __restrict__ x, int64_t so, int64_t S, int fs, double t, double f,
                         double* acc, bool first) {
  constexpr int LG = 11, N = 1 << LG;
  const int n = windowed(x, so, S, t, f, 1, 4.0, fs, N, &L.bA[0].x, 2, L.red);
  double p = 0.0;
  for (int j = threadIdx.x; j < n; j += AT) p += L.bA[j].x * L.bA[j].x;
  p = bsum(p, L.red);
  const double sc = p > 0.0 ? sqrt(p) : 1.0;
  for (int j = threadIdx.x; j < N; j += AT) {
    const double v = p > 0.0 ? L.bA[j].x / sc : L.bA[j].x;
    L.bA[j] = make_double2(v, v * (j + 1.0));
  }
  __syncthreads();
  const double2* Z = fftd<false>(L.bA, L.bB, LG, L.tw);
  for (int k = threadIdx.x; k <= N / 2; k += AT) {
    double2 A, B;
    unpack2(Z, N, k, A, B);
    const double c = B.x * A.x + A.y * B.y;
    acc[k] = first ? c : acc[k] + c;
  }
  __syncthreads();
}

__device__ double d4c_coarse(FrameLds& L, const float* __restrict__ x, int64_t so, int64_t S, int fs, double t,
                             double f0) {
  constexpr int LG = 11, N = 1 << LG, HN = N / 2;
  const double f = fmax(47.0, f0);
  centroid(L, x, so, S, fs, t - 0.25 / f, f, L.r0, true);
  centroid(L, x, so, S, fs, t + 0.25 / f, f, L.r0, false);
  dc_correction(L.r0, f, fs, N);
  windowed(x, so, S, t, f, 0, 4.0, fs, N, &L.bA[0].x, 2, L.red);
  for (int j = threadIdx.x; j < N; j += AT) L.bA[j].y = 0.0;
  __syncthreads();
  const double2* X = fftd<false>(L.bA, L.bB, LG, L.tw);
  for (int k = threadIdx.x; k <= HN; k += AT) L.r1[k] = X[k].x * X[k].x + X[k].y * X[k].y;
  __syncthreads();
  dc_correction(L.r1, f, fs, N);
  linear_smoothing(L.r1, L.r1, f, fs, N, L.r2, L.red);
  for (int k = threadIdx.x; k <= HN; k += AT) L.r0[k] = L.r1[k] > 0.0 ? L.r0[k] / L.r1[k] : 0.0;
  __syncthreads();
  linear_smoothing(L.r0, L.r0, f / 2.0, fs, N, L.r2, L.red);
  linear_smoothing(L.r0, L.r1, f, fs, N, L.r2, L.red);
  for (int k = threadIdx.x; k <= HN; k += AT) L.r0[k] = L.r0[k] - L.r1[k];
  __syncthreads();
  // coarse aperiodicity of the one 3 kHz band
  constexpr int WL = (int)(3000.0 * N / 16000) * 2 + 1, HW = WL / 2, CEN = (int)(3000.0 * N / 16000);
  for (int j = threadIdx.x; j < N; j += AT) {
    double v = 0.0;
    if (j < WL) {
      const double tt = j / (WL - 1.0);
      const double w = 0.355768 - 0.487396 * cos(2 * PI * tt) + 0.144232 * cos(4 * PI * tt) -
                       0.012604 * cos(6 * PI * tt);
      v = L.r0[CEN - HW + j] * w;
    }
    L.bA[j] = make_double2(v, 0.0);
  }
  __syncthreads();
  const double2* Y = fftd<false>(L.bA, L.bB, LG, L.tw);
  double* srt = (double*)(Y == L.bA ? L.bB : L.bA);  // N doubles
  for (int k = threadIdx.x; k < N; k += AT) srt[k] = k <= HN ? Y[k].x * Y[k].x + Y[k].y * Y[k].y : DBL_MAX;
  __syncthreads();
  for (int kk = 2; kk <= N; kk <<= 1) {  // bitonic sort, ascending
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < N; i += AT) {
        const int p = i ^ jj;
        if (p > i) {
          const double a = srt[i], b = srt[p];
          const bool up = (i & kk) == 0;
          if (up ? a > b : a < b) {
            srt[i] = b;
            srt[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  const int bd = mround(N * 8.0 / WL);
  double sa = 0.0, st = 0.0;
  for (int k = threadIdx.x; k <= HN; k += AT) {
    st += srt[k];
    if (k <= HN - bd - 1) sa += srt[k];
  }
  sa = bsum(sa, L.red);
  st = bsum(st, L.red);
  const double coarse = st == 0.0 ? 0.0 : 10 * log10(sa / st);
  return fmin(0.0, coarse + (f - 100) / 50.0);
}

}  // namespace

__global__ void __launch_bounds__(AT) k_an_taps(int fs, double f0_floor, double* __restrict__ taps) {
  __shared__ double lcsum;
  const int b = blockIdx.x;
  const double bf = band_f0(f0_floor, b);
  const int L = mround(fs / bf * 2.0), C = LC_C, K = C + L;
  const int NL = 2 * C + 1, NB = 2 * L + 1;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 1; i <= NL; ++i) s += 0.5 - 0.5 * cos(i * 2.0 * PI / (NL + 1));
    lcsum = s;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < TAPMAX; q += AT) {
    double acc = 0.0;
    if (q <= 2 * K) {
      const int o = q - K;  // offset of the combined tap
      for (int j = max(-C, o - L); j <= min(C, o + L); ++j) {
        double lc = -(0.5 - 0.5 * cos((C + j + 1) * 2.0 * PI / (NL + 1))) / lcsum;
        if (j == 0) lc += 1.0;
        const int kb = o - j + L;  // band-pass index 0 .. 2L
        const double tt = kb / (NB - 1.0);
        const double w = 0.355768 - 0.487396 * cos(2 * PI * tt) + 0.144232 * cos(4 * PI * tt) -
                         0.012604 * cos(6 * PI * tt);
        acc += lc * (w * cos(2 * PI * bf * (kb - L) / fs));
      }
    }
    taps[b * TAPMAX + q] = acc;
  }
}

__global__ void __launch_bounds__(AT) k_an_mean(const float* __restrict__ x, const int64_t* __restrict__ foff,
                                                const int64_t* __restrict__ soff, int64_t F, int64_t Stot,
                                                double* __restrict__ mean) {
  __shared__ double red[AT / 64];
  const int u = blockIdx.x;
  int64_t fo, T, so, S;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < S; i += AT) s += (double)x[so + i];
  s = bsum(s, red);
  if (threadIdx.x == 0) mean[u] = s / (double)(S + 1);
}

__global__ void __launch_bounds__(AT) k_an_band(const float* __restrict__ x, const int64_t* __restrict__ foff,
                                                const int64_t* __restrict__ soff, int n_seg, int64_t F, int64_t Stot,
                                                int fs, double f0_floor, const double* __restrict__ taps,
                                                const double* __restrict__ mean, double* __restrict__ band) {
  __shared__ double h[TAPMAX];
  const int b = blockIdx.y;
  for (int q = threadIdx.x; q < TAPMAX; q += AT) h[q] = taps[b * TAPMAX + q];
  __syncthreads();
  const int64_t NBS = Stot + n_seg;
  const int64_t g = (int64_t)blockIdx.x * AT + threadIdx.x;
  if (g >= NBS) return;
  int lo = 0, hi = n_seg - 1;  // utterance: largest u with soff[u] + u <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (soff[mid] + mid <= g) lo = mid;
    else hi = mid - 1;
  }
  const int u = lo;
  int64_t fo, T, so, S;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  const int64_t i = g - soff[u] - u;
  double acc = 0.0;
  if (i >= 0 && i <= S) {
    const double bf = band_f0(f0_floor, b);
    const int K = LC_C + mround(fs / bf * 2.0);
    const double m = mean[u];
    const int64_t q0 = max((int64_t)0, (int64_t)K - i - 1), q1 = min((int64_t)2 * K, (int64_t)K + S - i - 1);
    for (int64_t q = q0; q <= q1; ++q) {
      const int64_t j = i + 1 + q - K;  // 0 <= j <= S
      const double y = (j < S ? (double)x[so + j] : 0.0) - m;
      acc += h[q] * y;
    }
  }
  band[(int64_t)b * NBS + g] = acc;
}

__global__ void __launch_bounds__(AT) k_an_events(const int64_t* __restrict__ foff, const int64_t* __restrict__ soff,
                                                  int n_seg, int64_t F, int64_t Stot, const double* __restrict__ band,
                                                  double* __restrict__ edges, int32_t* __restrict__ ecnt) {
  __shared__ int wcount[4][AT / 64];
  const int u = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t fo, T, so, S;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  const int64_t NBS = Stot + n_seg, NES = Stot / 2 + 2 * (int64_t)n_seg;
  const double* s = band + (int64_t)b * NBS + so + u;
  const int64_t base = so / 2 + 2 * (int64_t)u;
  const int64_t cap = min(S / 2 + 2, max(NES - base, (int64_t)0));
  const int64_t len[4] = {S + 1, S + 1, S, S};
  int64_t count[4] = {0, 0, 0, 0};
  for (int64_t c0 = 1; c0 <= S; c0 += AT) {  // candidate edges e = 1 .. len - 1
    const int64_t e = c0 + tid;
    double a[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0};
    bool hit[4] = {false, false, false, false};
    if (e <= S) {
      const double p = s[e - 1], c = s[e];
      a[0] = p;
      z[0] = c;
      a[1] = -p;
      z[1] = -c;
      if (e + 1 <= S) {
        const double dp = c - p, dc = s[e + 1] - c;
        a[2] = dp;
        z[2] = dc;
        a[3] = -dp;
        z[3] = -dc;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) hit[k] = e < len[k] && a[k] > 0.0 && z[k] <= 0.0;
    }
    uint64_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m[k] = __ballot(hit[k]);
      if (lane == 0) wcount[k][wv] = __popcll(m[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < AT / 64; ++w) {
        before += w < wv ? wcount[k][w] : 0;
        total += wcount[k][w];
      }
      if (hit[k]) {
        const int64_t slot = count[k] + before + __popcll(m[k] & ((1ull << lane) - 1ull));
        if (slot < cap) edges[(int64_t)(b * 4 + k) * NES + base + slot] = (double)e - a[k] / (z[k] - a[k]);
      }
      count[k] += total;
    }
    __syncthreads();
  }
  if (tid < 4) ecnt[(int64_t)(b * 4 + tid) * n_seg + u] = (int32_t)min(count[tid], cap);
}

namespace {
// WORLD's interp1 of the interval series of one fine-edge list at time t
__device__ double interp_series(const double* e, int n_e, double t, double fsd) {
  const int n = n_e - 1;  // intervals
  int lo = 0, hi = n;     // count of locations <= t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((e[mid] + e[mid + 1]) / 2.0 / fsd <= t) lo = mid + 1;
    else hi = mid;
  }
  const int k = min(max(lo, 1), n - 1);
  const double l0 = (e[k - 1] + e[k]) / 2.0 / fsd, l1 = (e[k] + e[k + 1]) / 2.0 / fsd;
  const double v0 = fsd / (e[k] - e[k - 1]), v1 = fsd / (e[k + 1] - e[k]);
  const double s = (t - l0) / (l1 - l0);
  return v0 + s * (v1 - v0);
}
}  // namespace

__global__ void __launch_bounds__(AT) k_an_cand(const int64_t* __restrict__ foff, const int64_t* __restrict__ soff,
                                                int n_seg, int64_t F, int64_t Stot, int fs, double frame_period_ms,
                                                double f0_floor, double f0_ceil, int nb,
                                                const double* __restrict__ edges, const int32_t* __restrict__ ecnt,
                                                double* __restrict__ cand, double* __restrict__ score,
                                                double* __restrict__ best) {
  const int64_t f = (int64_t)blockIdx.x * AT + threadIdx.x;
  if (f >= F) return;
  int lo = 0, hi = n_seg - 1;  // utterance: largest u with foff[u] <= f
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (foff[mid] <= f) lo = mid;
    else hi = mid - 1;
  }
  const int u = lo;
  int64_t fo, T, so, S;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  const int64_t i = f - foff[u];
  const double t = (double)i * frame_period_ms / 1000.0, fsd = (double)fs;
  const int64_t NES = Stot / 2 + 2 * (int64_t)n_seg;
  const int64_t base = so / 2 + 2 * (int64_t)u;
  double bc = 0.0, bs = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double bf = band_f0(f0_floor, b);
    int n[4];
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
      n[k] = ecnt[(int64_t)(b * 4 + k) * n_seg + u];
      ok = ok && n[k] - 1 >= 3;
    }
    double c = 0.0, sc = MAXV / SAFE;
    if (ok) {
      double v[4];
      for (int k = 0; k < 4; ++k) v[k] = interp_series(edges + (int64_t)(b * 4 + k) * NES + base, n[k], t, fsd);
      c = (v[0] + v[1] + v[2] + v[3]) / 4.0;
      double q = sqrt(((v[0] - c) * (v[0] - c) + (v[1] - c) * (v[1] - c) + (v[2] - c) * (v[2] - c) +
                       (v[3] - c) * (v[3] - c)) / 3.0);
      if (c > bf || c < bf / 2.0 || c > f0_ceil || c < f0_floor || !(c == c)) {
        c = 0.0;
        q = MAXV;
      }
      sc = q / (c + SAFE);
    }
    cand[(int64_t)b * F + f] = c;
    score[(int64_t)b * F + f] = sc;
    if (b == 0 || bs > sc) {
      bs = sc;
      bc = c;
    }
  }
  best[f] = bc;
}

namespace {
__device__ double select_best(double cur, double past, const double* cand, int64_t F, int nb, int64_t j) {
  const double ref = (cur * 3.0 - past) / 2.0;
  double err = fabs(ref - cand[j]), bst = cand[j];
  for (int b = 1; b < nb; ++b) {
    const double e = fabs(ref - cand[(int64_t)b * F + j]);
    if (e < err) {
      err = e;
      bst = cand[(int64_t)b * F + j];
    }
  }
  if (fabs(1.0 - bst / ref) > 0.1) return 0.0;
  return bst;
}
}  // namespace

__global__ void k_an_fix(const int64_t* __restrict__ foff, const int64_t* __restrict__ soff, int n_seg, int64_t F,
                         int64_t Stot, double frame_period_ms, double f0_floor, int nb,
                         const double* __restrict__ cand, const double* __restrict__ best, double* __restrict__ s1,
                         double* __restrict__ s2, double* __restrict__ out) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_seg) return;
  int64_t fo, T, so, S;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  const double* bc = best + fo;
  const double* cd = cand + fo;
  double *a = s1 + fo, *c = s2 + fo, *o = out + fo;
  const int64_t vrm = (int64_t)(0.5 + 1000.0 / frame_period_ms / f0_floor) * 2 + 1;
  if (T <= vrm) {
    for (int64_t i = 0; i < T; ++i) o[i] = a[i] = c[i] = 0.0;
    return;
  }
  // step 1 -> a
  for (int64_t i = 0; i < vrm; ++i) a[i] = 0.0;
  for (int64_t i = vrm; i < T; ++i) {
    const double bi = i < T - vrm ? bc[i] : 0.0, bp = (i - 1 >= vrm && i - 1 < T - vrm) ? bc[i - 1] : 0.0;
    a[i] = fabs((bi - bp) / (SAFE + bi)) < 0.1 ? bi : 0.0;
  }
  // step 2 -> c
  const int64_t cc = (vrm - 1) / 2;
  for (int64_t i = 0; i < T; ++i) {
    double v = a[i];
    if (i >= cc && i < T - cc)
      for (int64_t j = -cc; j <= cc; ++j)
        if (a[i + j] == 0) {
          v = 0.0;
          break;
        }
    c[i] = v;
  }
  // step 3: from c into a (forward over the ends of voiced sections)
  for (int64_t i = 0; i < T; ++i) a[i] = c[i];
  int64_t pend = -1;
  for (int64_t i = 1; i <= T; ++i) {
    const bool neg = i < T && c[i] == 0 && c[i - 1] != 0;
    if (!(neg || i == T) || pend < 0) {
      if (neg) pend = i - 1;
      continue;
    }
    const int64_t limit = i == T ? T - 1 : i - 1;
    for (int64_t j = pend; j < limit; ++j) {
      a[j + 1] = j >= 1 ? select_best(a[j], a[j - 1], cd, F, nb, j + 1) : 0.0;
      if (a[j + 1] == 0) break;
    }
    pend = neg ? i - 1 : -1;
  }
  // step 4: from a into o (backward over the starts of voiced sections)
  for (int64_t i = 0; i < T; ++i) o[i] = a[i];
  pend = -1;
  for (int64_t i = T - 1; i >= 0; --i) {
    const bool pos = i >= 1 && c[i - 1] == 0 && c[i] != 0;
    if (!(pos || i == 0) || pend < 0) {
      if (pos) pend = i;
      continue;
    }
    const int64_t limit = i == 0 ? 1 : i;
    for (int64_t j = pend; j > limit; --j) {
      o[j - 1] = j + 1 < T ? select_best(o[j], o[j + 1], cd, F, nb, j - 1) : 0.0;
      if (o[j - 1] == 0) break;
    }
    pend = pos ? i : -1;
  }
}

__global__ void __launch_bounds__(AT) k_an_frame(const float* __restrict__ x, const int64_t* __restrict__ foff,
                                                 const int64_t* __restrict__ soff, int n_seg, int64_t F, int64_t Stot,
                                                 int fs, double frame_period_ms, AnalysisWs w, float* __restrict__ f0o,
                                                 float* __restrict__ spo, float* __restrict__ apo,
                                                 float* __restrict__ eno) {
  __shared__ FrameLds L;
  for (int m = threadIdx.x; m < NMAX / 2; m += AT) {
    double s, c;
    sincospi(-2.0 * (double)m / (double)NMAX, &s, &c);
    L.tw[m] = make_double2(c, s);
  }
  __syncthreads();
  const int64_t f = blockIdx.x;
  int lo = 0, hi = n_seg - 1;  // utterance: largest u with foff[u] <= f
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (foff[mid] <= f) lo = mid;
    else hi = mid - 1;
  }
  const int u = lo;
  int64_t fo, T, so, S;
  utt_range(foff, soff, u, F, Stot, fo, T, so, S);
  const double t = (double)(f - foff[u]) * frame_period_ms / 1000.0;
  bool back;
  const double rf = stonemask(L, x, so, S, fs, t, w.f0d[f], back);
  cheaptrick(L, x, so, S, fs, t, rf);
  double e = 0.0;
  for (int k = threadIdx.x; k < HB; k += AT) e += L.r0[k] + 1e-10;
  e = bsum(e, L.red);
  for (int k = threadIdx.x; k < HB; k += AT) spo[f * HB + k] = (float)log10(L.r0[k] / e);
  __syncthreads();
  const double ap0 = lovetrain(L, x, so, S, fs, t, rf);
  const bool body = rf != 0.0 && ap0 > 0.85;
  const double coarse = body ? d4c_coarse(L, x, so, S, fs, t, rf) : 0.0;
  for (int k = threadIdx.x; k < HB; k += AT) {
    double a = 1.0 - SAFE;
    if (body) {  // interp1 over [0, 3000, fs/2] of [-60, coarse, -1e-12] dB
      const double fa = (double)k * fs / NCT;
      double y;
      if (fa < 3000.0) {
        const double s = (fa - 0.0) / (3000.0 - 0.0);
        y = -60.0 + s * (coarse - -60.0);
      } else {
        const double s = (fa - 3000.0) / (fs / 2.0 - 3000.0);
        y = coarse + s * (-SAFE - coarse);
      }
      a = pow(10.0, y / 20.0);
    }
    apo[f * HB + k] = (float)a;
  }
  if (threadIdx.x == 0) {
    f0o[f] = (float)rf;
    eno[f] = (float)e;
    w.f0r[f] = rf;
    w.ap0[f] = ap0;
    w.coarse[f] = coarse;
    w.flags[f] = (back ? 1 : 0) | (body ? 2 : 0);
  }
}

AnalysisWs analysis_carve(void* ws, int n_seg, int64_t S, int64_t F, int nb) {
  AnalysisWs w;
  char* base = (char*)ws;
  int64_t o = 0;
  const int64_t NBS = S + n_seg, NES = S / 2 + 2 * (int64_t)n_seg;
  auto take = [&](int64_t bytes) {
    const int64_t q = o;
    o += align256(bytes);
    return base + q;
  };
  w.mean = (double*)take(n_seg * 8LL);
  w.taps = (double*)take((int64_t)nb * TAPMAX * 8);
  w.band = (double*)take((int64_t)nb * NBS * 8);
  w.edges = (double*)take((int64_t)nb * 4 * NES * 8);
  w.ecnt = (int32_t*)take((int64_t)nb * 4 * n_seg * 4);
  w.cand = (double*)take((int64_t)nb * F * 8);
  w.score = (double*)take((int64_t)nb * F * 8);
  w.best = (double*)take(F * 8);
  w.s1 = (double*)take(F * 8);
  w.s2 = (double*)take(F * 8);
  w.f0d = (double*)take(F * 8);
  w.f0r = (double*)take(F * 8);
  w.ap0 = (double*)take(F * 8);
  w.coarse = (double*)take(F * 8);
  w.flags = (int32_t*)take(F * 4);
  w.bytes = o;
  return w;
}

int analysis_taps() { return TAPMAX; }

int64_t analysis_workspace_bytes(int n_seg, int64_t S, int64_t F, int nb) {
  static char probe;
  return analysis_carve(&probe, n_seg, S, F, nb).bytes;
}

void launch_analyze(const float* x, const int64_t* soff, const int64_t* foff, int n_seg, int64_t S, int64_t F, int fs,
                    double frame_period_ms, double f0_floor, double f0_ceil, int nb, float* f0, float* sp, float* ap,
                    float* en, void* ws, hipStream_t s) {
  const AnalysisWs w = analysis_carve(ws, n_seg, S, F, nb);
  const int64_t NBS = S + n_seg;
  hipLaunchKernelGGL(k_an_taps, dim3((unsigned)nb), dim3(AT), 0, s, fs, f0_floor, w.taps);
  hipLaunchKernelGGL(k_an_mean, dim3((unsigned)n_seg), dim3(AT), 0, s, x, foff, soff, F, S, w.mean);
  hipLaunchKernelGGL(k_an_band, dim3((unsigned)((NBS + AT - 1) / AT), (unsigned)nb), dim3(AT), 0, s, x, foff, soff,
                     n_seg, F, S, fs, f0_floor, w.taps, w.mean, w.band);
  hipLaunchKernelGGL(k_an_events, dim3((unsigned)n_seg, (unsigned)nb), dim3(AT), 0, s, foff, soff, n_seg, F, S, w.band,
                     w.edges, w.ecnt);
  hipLaunchKernelGGL(k_an_cand, dim3((unsigned)((F + AT - 1) / AT)), dim3(AT), 0, s, foff, soff, n_seg, F, S, fs,
                     frame_period_ms, f0_floor, f0_ceil, nb, w.edges, w.ecnt, w.cand, w.score, w.best);
  hipLaunchKernelGGL(k_an_fix, dim3((unsigned)((n_seg + 63) / 64)), dim3(64), 0, s, foff, soff, n_seg, F, S,
                     frame_period_ms, f0_floor, nb, w.cand, w.best, w.s1, w.s2, w.f0d);
  hipLaunchKernelGGL(k_an_frame, dim3((unsigned)F), dim3(AT), 0, s, x, foff, soff, n_seg, F, S, fs, frame_period_ms, w,
                     f0, sp, ap, en);
}

}  // namespace vaenpvc
