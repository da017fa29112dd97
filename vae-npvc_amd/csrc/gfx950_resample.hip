// gfx950_resample.hip -- band-limited resampling of the data path (analyzer.py --resample): the
// Kaiser-windowed sinc interpolation resampy documents as `kaiser_best`, the filter behind the reference's
// librosa.load(sr=16000).  Nothing here allocates, synchronises with the host or uses an atomic.
//
// Rates rate_in -> rate_out, g = gcd, L = rate_out / g, M = rate_in / g, s = min(1, L / M), K = ceil(64 / s).  Output m of a
// segment sits at u = m M / L input samples and is
//   y[m] = sum_{j = -K+1 .. K} x[floor(u) + j] h(frac(u) - j)          (x zero outside the segment)
// summed in float64 in ascending j and rounded once to float32.  frac(u) depends only on r = m mod L, so the weights are
// the host-built table T [2K][L], T[j + K - 1][r] = h(((r M) mod L) / L - j) (resample_filter_host, the only place the
// weights are computed).
//
//   k_resample   one workgroup of VAENPVC_RESAMPLE_TILE lanes per tile of that many consecutive outputs of one segment.
//                Segment u owns the tile slots floor(ooff[u] / TILE) + u .. floor(ooff[u+1] / TILE) + u (at least
//                ceil(n_out_u / TILE) of them; a slot past the segment's last tile exits at once), so a workgroup finds
//                its segment by a binary search over the out-offsets alone and the grid, floor(S_out / TILE) + n_seg, is
//                known on the host.  The workgroup stages the tile's input window, samples floor(m0 M / L) - K + 1
//                onwards, ceil(TILE M / L) + 2K of them, once in LDS as float32 with zeros outside the segment; lane i
//                then owns output m0 + i: 2K fused multiply-adds in float64, the sample from LDS, the weight from
//                T[jj][r] -- lanes with consecutive m read consecutive doubles of a table row (r wraps to 0 inside a tile
//                when L < TILE or the tile straddles a multiple of L; with L = 1 or 2 all lanes read the same one or two
//                values).  m is the index within the segment and the window is filled from the segment alone, so a
//                segment's outputs are the same bytes wherever it stands in the call.
// Offsets are clamped to [0, S_in] resp. [0, S_out] and a tile past its segment's output range writes nothing, so
// malformed arrays cannot make the kernel leave its buffers.
#include <cmath>

#include "../../include/vaenpvc.h"
#include "kernels.h"

namespace vaenpvc {

namespace {

constexpr int RS_TILE = VAENPVC_RESAMPLE_TILE;
constexpr double RS_ZEROS = 64.0;                    // zero crossings of the sinc on each side (resampy kaiser_best)
constexpr double RS_BETA = 14.769656459379492;       // Kaiser window shape
constexpr double RS_ROLLOFF = 0.9475937167399596;    // cutoff as a fraction of the lower Nyquist rate

__device__ __forceinline__ int64_t rs_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(RS_TILE) void k_resample(const float* __restrict__ x, const int64_t* __restrict__ ioff,
                                                      const int64_t* __restrict__ ooff, int n_seg, int64_t S_in,
                                                      int64_t S_out, int L, int M, int K, int win,
                                                      const double* __restrict__ T, float* __restrict__ y) {
  extern __shared__ float rs_win[];   // [win] input samples floor(m0 M / L) - K + 1 ... of the segment
  const int64_t slot = blockIdx.x;
  // the last segment whose first tile slot is <= slot
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rs_clamp(ooff[mid], S_out) / RS_TILE + mid <= slot) lo = mid; else hi = mid - 1;
  }
  const int u = lo;
  const int64_t o0 = rs_clamp(ooff[u], S_out), o1 = rs_clamp(ooff[u + 1], S_out);
  const int64_t i0 = rs_clamp(ioff[u], S_in), i1 = rs_clamp(ioff[u + 1], S_in);
  const int64_t n_in = i1 - i0, n_out = o1 - o0;     // <= 0 on a malformed array: nothing is read resp. written
  const int64_t tile = slot - (o0 / RS_TILE + u);
  if (tile < 0 || tile * RS_TILE >= n_out) return;   // (uniform over the workgroup, ahead of the barrier)
  const int64_t m0 = tile * RS_TILE;
  const int64_t t0 = m0 * (int64_t)M;                // m M < 2^31 * 2^19
  const int64_t q0 = t0 / L;
  const uint32_t r0 = (uint32_t)(t0 - q0 * L);
  const int64_t first = q0 - K + 1;                  // the segment's sample at rs_win[0]
  const float* xs = x + i0;
  for (int i = threadIdx.x; i < win; i += RS_TILE) {
    const int64_t k = first + i;
    rs_win[i] = (k >= 0 && k < n_in) ? xs[k] : 0.0f;
  }
  __syncthreads();
  const int64_t m = m0 + threadIdx.x;
  if (m >= n_out) return;
  // floor(m M / L) - q0 = floor((r0 + i M) / L): r0 < L <= 384000 and i M < 256 * 384000 stay in 32 bits
  const uint32_t dq = (r0 + (uint32_t)threadIdx.x * (uint32_t)M) / (uint32_t)L;
  const uint32_t r = (uint32_t)(m % L);
  const float* w = rs_win + dq;                      // dq + 2K - 1 <= ceil((TILE - 1) M / L) + 2K - 1 < win
  const double* t = T + r;
  double acc = 0.0;
  const int taps = 2 * K;
#pragma unroll 8
  for (int jj = 0; jj < taps; ++jj) acc = fma((double)w[jj], t[(size_t)jj * L], acc);
  y[o0 + m] = (float)acc;
}

// I0 by its power series sum ((x/2)^2)^k / (k!)^2, every term positive, to convergence
double rs_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

}  // namespace

bool resample_plan_host(int rate_in, int rate_out, int* up, int* down, int* half_taps) {
  if (rate_in < 1000 || rate_in > 384000 || rate_out < 1000 || rate_out > 384000 || rate_in == rate_out) return false;
  int a = rate_in, b = rate_out;
  while (b) { const int c = a % b; a = b; b = c; }
  const int64_t L = rate_out / a, M = rate_in / a;
  const int64_t K = M > L ? (64 * M + L - 1) / L : 64;                 // ceil(64 / s), s = min(1, L / M)
  if (2 * K * L > VAENPVC_RESAMPLE_MAX_TABLE) return false;
  if ((RS_TILE * M + L - 1) / L + 2 * K > VAENPVC_RESAMPLE_MAX_WINDOW) return false;
  *up = (int)L;
  *down = (int)M;
  *half_taps = (int)K;
  return true;
}

void resample_filter_host(int L, int M, int K, double* T) {
  const double pi = 3.14159265358979323846;
  const double s = M > L ? (double)L / (double)M : 1.0;
  const double c = s * RS_ROLLOFF, i0b = rs_i0(RS_BETA);
  for (int r = 0; r < L; ++r) {
    const double frac = (double)(((int64_t)r * M) % L) / (double)L;
    for (int j = -K + 1; j <= K; ++j) {
      const double tt = frac - (double)j;
      const double v = s * tt / RS_ZEROS;
      double h = 0.0;
      if (std::fabs(v) < 1.0) {
        const double a = pi * (c * tt);
        const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
        h = c * sinc * rs_i0(RS_BETA * std::sqrt(1.0 - v * v)) / i0b;
      }
      T[(size_t)(j + K - 1) * L + r] = h;
    }
  }
}

void launch_resample(const float* x, const int64_t* ioff, const int64_t* ooff, int n_seg, int64_t S_in, int64_t S_out,
                     int L, int M, int K, const double* T, float* y, hipStream_t s) {
  const int win = (int)(((int64_t)RS_TILE * M + L - 1) / L) + 2 * K;
  const int64_t grid = S_out / RS_TILE + n_seg;
  hipLaunchKernelGGL(k_resample, dim3((unsigned)grid), dim3(RS_TILE), (size_t)win * sizeof(float), s, x, ioff, ooff,
                     n_seg, S_in, S_out, L, M, K, win, T, y);
}

}  // namespace vaenpvc
