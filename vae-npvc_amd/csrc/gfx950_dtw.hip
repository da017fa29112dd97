// gfx950_dtw.hip -- objective evaluation of a conversion: mel-cepstral distortion (MCD) along a dynamic-time-warping
// path, with the log-F0 error and the voicing mismatch on the same path (evaluate.py; the reference has no such tool).
// The metric is stated in DESIGN.md section 16 and restated in float64 NumPy by tests/mcd_ref.py.
//
// n_pair utterance pairs: pair p is frames offA[p] .. offA[p+1] of side A and offB[p] .. offB[p+1] of side B.  Five
// launches on the caller's stream, no host synchronisation, no allocation, no atomics; all arithmetic is float64:
//   k_mcd_prep   one thread: per pair the frame counts, the 64-bit offset of its cost matrix and of its first tile; a
//                pair whose offsets break the contract (a side outside 1 .. 4096 frames, outside the inputs, or more
//                cells than the workspace holds) is marked invalid: no later kernel touches it, its results are NaN
//   k_mcd_mcep   8 frames per workgroup: L = 0.5 (ln 10 sp + ln en) in LDS, mc = W L as sequential fused multiply-adds
//                over the 513 bins (k ascending), and ln f0 of the voiced frames
//   k_mcd_cost   grid-strided over 32 x 64 tiles of every pair's cost matrix: d(i, j) = sqrt(sum_m (a_m - b_m)^2),
//                m = 1 .. M ascending, stored anti-diagonal after anti-diagonal (see diag_pre)
//   k_mcd_dp     one workgroup of 1024 threads per pair walks the Ta + Tb - 1 anti-diagonals.  A thread owns R = 1, 2 or
//                4 consecutive rows and keeps D(i, j-1) and D(i-1, j-1) of each in registers; only the last row of a
//                thread is handed to the next thread through LDS (double-buffered: one barrier per diagonal, waiting
//                for LDS only).  Costs are loaded a chunk of 16 / R diagonals ahead and the predecessor bytes (0
//                diagonal, 1 from (i-1, j), 2 from (i, j-1); on ties in that order) are stored a chunk late, so a
//                diagonal waits for memory once per chunk at most
//   k_mcd_trace  one wave per pair follows the bytes from (Ta-1, Tb-1) to (0, 0).  The wave loads an 8 x 8 window of
//                bytes, costs and ln f0 at once and walks inside it with cross-lane reads, so one memory latency is paid
//                per window and not per step.  Sums are taken in this (backward) path order without contraction
// A pair's results depend only on its own frames, bit for bit, whatever shares the call.
#include <cmath>
#include <vector>

#include "kernels.h"

// additions and multiplications below are rounded one by one (the exact stages are compared bit for bit with NumPy);
// the dot products ask for their fused multiply-adds by name
#pragma clang fp contract(off)

namespace vaenpvc {

namespace {

constexpr int MH = 513;             // bins
constexpr int MC_FR = 8;            // frames per workgroup of k_mcd_mcep
constexpr int CT_I = 32, CT_J = 64; // tile of k_mcd_cost
constexpr int CT_MS = 65;           // LDS row stride in doubles (odd: lanes of a wave fall on distinct banks)
constexpr int DP_T = 1024;          // threads of k_mcd_dp; at most 4 rows per thread: MCD_MAX_FRAMES = 4 * DP_T
static_assert(MCD_MAX_FRAMES == 4 * DP_T, "k_mcd_dp covers 4 rows per thread at most");
constexpr int PI_N = 6;             // int64 fields of a pinfo row: coff, toff, oa, ob, Ta, Tb
constexpr double LN10 = 2.302585092994046;   // == np.log(10.0)
constexpr double PI_D = 3.141592653589793;
constexpr int64_t COST_GRID = 8192;

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// The cost matrix, the predecessor bytes and D of a pair are stored anti-diagonal after anti-diagonal (s = i + j
// ascending, inside a diagonal i ascending), so that the lanes of the DP kernel, which own consecutive rows, read and
// write consecutive addresses.  diag_pre: the cells on the diagonals before s.
__device__ __forceinline__ int64_t diag_pre(int s, int Ta, int Tb) {
  const int m = Ta < Tb ? Ta : Tb, M = Ta < Tb ? Tb : Ta;
  if (s <= m) return (int64_t)s * (s + 1) / 2;
  if (s <= M) return (int64_t)m * (m + 1) / 2 + (int64_t)(s - m) * m;
  const int64_t r = Ta + Tb - 1 - s;
  return (int64_t)Ta * Tb - r * (r + 1) / 2;
}
// offset of diagonal s's (virtual) row 0: cell (i, s - i) is at diag_base(s) + i
__device__ __forceinline__ int64_t diag_base(int s, int Ta, int Tb) {
  const int ilo = s - Tb + 1 > 0 ? s - Tb + 1 : 0;
  return diag_pre(s, Ta, Tb) - ilo;
}

__global__ __launch_bounds__(64) void k_mcd_prep(const int64_t* __restrict__ offA, const int64_t* __restrict__ offB,
                                                 int n_pair, int64_t Fa, int64_t Fb, int64_t cells,
                                                 int64_t* __restrict__ pinfo) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t coff = 0, toff = 0;
  for (int p = 0; p < n_pair; ++p) {
    const int64_t oa = offA[p], ob = offB[p];
    int64_t Ta = offA[p + 1] - oa, Tb = offB[p + 1] - ob;
    const bool ok = oa >= 0 && ob >= 0 && Ta >= 1 && Tb >= 1 && Ta <= MCD_MAX_FRAMES && Tb <= MCD_MAX_FRAMES &&
                    oa + Ta <= Fa && ob + Tb <= Fb && coff + Ta * Tb <= cells;
    if (!ok) Ta = Tb = 0;
    int64_t* q = pinfo + (int64_t)p * PI_N;
    q[0] = coff;
    q[1] = toff;
    q[2] = oa;
    q[3] = ob;
    q[4] = Ta;
    q[5] = Tb;
    coff += Ta * Tb;
    toff += ((Ta + CT_I - 1) / CT_I) * ((Tb + CT_J - 1) / CT_J);
  }
  int64_t* q = pinfo + (int64_t)n_pair * PI_N;
  q[0] = coff;
  q[1] = toff;
  q[2] = q[3] = q[4] = q[5] = 0;
}

// frames g < Fa are side A, the others side B; mc [Fa + Fb, M + 1], lf0 [Fa + Fb]
__global__ __launch_bounds__(256) void k_mcd_mcep(const float* __restrict__ spA, const float* __restrict__ enA,
                                                  const float* __restrict__ f0A, int64_t Fa,
                                                  const float* __restrict__ spB, const float* __restrict__ enB,
                                                  const float* __restrict__ f0B, int64_t Fb,
                                                  const double* __restrict__ W, int M, double* __restrict__ mc,
                                                  double* __restrict__ lf0) {
  __shared__ double Ls[MC_FR * MH];
  __shared__ double len[MC_FR];
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * MC_FR, F = Fa + Fb;
  if (tid < MC_FR) {
    const int64_t g = g0 + tid;
    if (g < F) {
      const float en = g < Fa ? enA[g] : enB[g - Fa];
      const float f0 = g < Fa ? f0A[g] : f0B[g - Fa];
      len[tid] = log((double)en);
      lf0[g] = f0 > 1.0f ? log((double)f0) : -1.0;
    } else {
      len[tid] = 0.0;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < MC_FR * MH; idx += 256) {
    const int f = idx / MH, k = idx - f * MH;
    const int64_t g = g0 + f;
    double v = 0.0;
    if (g < F) {
      const float s = g < Fa ? spA[g * MH + k] : spB[(g - Fa) * MH + k];
      v = 0.5 * (LN10 * (double)s + len[f]);
    }
    Ls[idx] = v;
  }
  __syncthreads();
  const int f = tid & (MC_FR - 1);
  const int64_t g = g0 + f;
  if (g >= F) return;
  const double* l = Ls + f * MH;
  for (int m = tid >> 3; m <= M; m += 256 / MC_FR) {
    const double* w = W + (int64_t)m * MH;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < MH; ++k) acc = fma(w[k], l[k], acc);
    mc[g * (M + 1) + m] = acc;
  }
}

__global__ __launch_bounds__(256) void k_mcd_cost(const int64_t* __restrict__ pinfo, int n_pair,
                                                  const double* __restrict__ mc, int64_t Fa, int M,
                                                  double* __restrict__ cost) {
  __shared__ double As[CT_I * CT_MS];
  __shared__ double Bs[CT_J * CT_MS];
  // a thread computes 8 cells of one tile row a; at each of them the 32 lanes with a = 0 .. 31 sit on one anti-diagonal
  // of the tile (column (c - a) mod 64), so a store instruction writes runs of consecutive addresses
  const int tid = threadIdx.x, a = tid & 31, c0 = (tid >> 6) * 16 + ((tid >> 5) & 1) * 8;
  const int64_t ntiles = pinfo[(int64_t)n_pair * PI_N + 1];
  const int M1 = M + 1;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    // the pair whose tile range holds t: last p with toff[p] <= t (pairs without tiles share their successor's toff)
    int lo = 0, hi = n_pair - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pinfo[(int64_t)mid * PI_N + 1] <= t) lo = mid; else hi = mid - 1;
    }
    const int64_t* q = pinfo + (int64_t)lo * PI_N;
    const int64_t coff = q[0], oa = q[2], ob = q[3];
    const int Ta = (int)q[4], Tb = (int)q[5];
    const int ntj = (Tb + CT_J - 1) / CT_J;
    const int loc = (int)(t - q[1]);
    const int i0 = (loc / ntj) * CT_I, j0 = (loc % ntj) * CT_J;
    __syncthreads();   // the previous tile's readers are done
    for (int idx = tid; idx < CT_I * M; idx += 256) {
      const int r = idx / M, m = idx - r * M;
      As[r * CT_MS + m] = i0 + r < Ta ? mc[(oa + i0 + r) * M1 + 1 + m] : 0.0;
    }
    for (int idx = tid; idx < CT_J * M; idx += 256) {
      const int r = idx / M, m = idx - r * M;
      Bs[r * CT_MS + m] = j0 + r < Tb ? mc[(Fa + ob + j0 + r) * M1 + 1 + m] : 0.0;
    }
    __syncthreads();
    double acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.0;
    for (int m = 0; m < M; ++m) {
      const double av = As[a * CT_MS + m];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double d = av - Bs[((c0 + r - a) & (CT_J - 1)) * CT_MS + m];
        acc[r] = fma(d, d, acc[r]);
      }
    }
    const int i = i0 + a;
    if (i < Ta) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j = j0 + ((c0 + r - a) & (CT_J - 1));
        if (j < Tb) cost[coff + diag_base(i + j, Ta, Tb) + i] = sqrt(acc[r]);
      }
    }
  }
}

// workgroup barrier that waits for this wave's LDS traffic only: the cost loads and the predecessor stores in flight stay
// in flight across it (__syncthreads() would drain them on every diagonal)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// R rows per thread, C diagonals per chunk.  The costs of chunk q + 1 are requested before chunk q is walked and the
// predecessor bytes of chunk q are stored when chunk q + 1 starts, so every memory operation has a whole chunk to land.
template <int R, int C>
__device__ __forceinline__ void dp_walk(int Ta, int Tb, const double* __restrict__ c, unsigned char* __restrict__ code,
                                        double* __restrict__ Dout, double* __restrict__ d_end, double (*X)[DP_T]) {
  const int t = threadIdx.x, i0 = t * R;
  const bool mine = i0 < Ta;        // the other threads only keep the barriers company
  const double INF = INFINITY;
  const int nsteps = Ta + Tb - 1, nchunks = (nsteps + C - 1) / C;
  double val[R], dg[R], cur[C][R], nxt[C][R];
  unsigned char kk[C][R];
#pragma unroll
  for (int r = 0; r < R; ++r) val[r] = dg[r] = INF;
#pragma unroll
  for (int u = 0; u < C; ++u) {
    const int64_t base = u < nsteps ? diag_base(u, Ta, Tb) : 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r, j = u - i;
      cur[u][r] = (mine && i < Ta && j >= 0 && j < Tb) ? c[base + i] : 0.0;
      kk[u][r] = 0;
    }
  }
  for (int q = 0; q < nchunks; ++q) {
    const int s0 = q * C;
#pragma unroll
    for (int u = 0; u < C; ++u) {       // the bytes of the chunk before, then the costs of the chunk after
      const int s = s0 - C + u;
      const int64_t base = s >= 0 ? diag_base(s, Ta, Tb) : 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = i0 + r, j = s - i;
        if (mine && s >= 0 && i < Ta && j >= 0 && j < Tb) code[base + i] = kk[u][r];
      }
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int s = s0 + C + u;
      const int64_t base = s < nsteps ? diag_base(s, Ta, Tb) : 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = i0 + r, j = s - i;
        nxt[u][r] = (mine && i < Ta && j >= 0 && j < Tb) ? c[base + i] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const int s = s0 + u;
      if (s < nsteps) {               // uniform over the workgroup
        if (mine) {
          const double upx = t > 0 ? X[(s + 1) & 1][t - 1] : INF;   // D(i0 - 1, s - i0), written on diagonal s - 1
          const int64_t base = Dout ? diag_base(s, Ta, Tb) : 0;
#pragma unroll
          for (int r = R - 1; r >= 0; --r) {
            const int i = i0 + r, j = s - i;
            if (i < Ta && j >= 0 && j < Tb) {
              const double up = r == 0 ? upx : val[r > 0 ? r - 1 : 0];
              double best = dg[r];
              unsigned char k = 0;
              if (up < best) { best = up; k = 1; }
              if (val[r] < best) { best = val[r]; k = 2; }
              const double d = (i == 0 && j == 0) ? cur[u][r] : cur[u][r] + best;
              kk[u][r] = k;
              if (Dout) Dout[base + i] = d;
              if (i == Ta - 1 && j == Tb - 1) *d_end = d;
              dg[r] = up;
              val[r] = d;
            }
          }
          X[s & 1][t] = val[R - 1];
        }
        lds_barrier();
      }
    }
#pragma unroll
    for (int u = 0; u < C; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) cur[u][r] = nxt[u][r];
  }
#pragma unroll
  for (int u = 0; u < C; ++u) {         // the bytes of the last chunk
    const int s = (nchunks - 1) * C + u;
    const int64_t base = s < nsteps ? diag_base(s, Ta, Tb) : 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r, j = s - i;
      if (mine && i < Ta && j >= 0 && j < Tb) code[base + i] = kk[u][r];
    }
  }
}

__global__ __launch_bounds__(DP_T) void k_mcd_dp(const int64_t* __restrict__ pinfo, const double* __restrict__ cost,
                                                 unsigned char* __restrict__ code, double* __restrict__ Dout,
                                                 double* __restrict__ results) {
  __shared__ double X[2][DP_T];
  const int p = blockIdx.x, t = threadIdx.x;
  const int64_t* q = pinfo + (int64_t)p * PI_N;
  const int Ta = (int)q[4], Tb = (int)q[5];
  if (Ta == 0) return;
  const int64_t coff = q[0];
  X[0][t] = INFINITY;
  X[1][t] = INFINITY;
  __syncthreads();
  double* D = Dout ? Dout + coff : nullptr;
  double* d_end = results + (int64_t)p * 8 + 2;
  // thread t owns rows t R .. t R + R - 1, R = 1, 2 or 4 covering Ta rows with 1024 threads (packing the rows of a short
  // utterance into fewer waves with R = 4 measured slower: 1.28 against 1.02 ms for 54 pairs of 700 frames)
  if (Ta <= DP_T) dp_walk<1, 16>(Ta, Tb, cost + coff, code + coff, D, d_end, X);
  else if (Ta <= 2 * DP_T) dp_walk<2, 8>(Ta, Tb, cost + coff, code + coff, D, d_end, X);
  else dp_walk<4, 4>(Ta, Tb, cost + coff, code + coff, D, d_end, X);
}

// results [n_pair, 8]: mcd_db, P, D(Ta-1, Tb-1) (written by k_mcd_dp), lf0_rmse, cells with both sides voiced, cells with
// one side voiced, sum of d along the path, 0
__global__ __launch_bounds__(64) void k_mcd_trace(const int64_t* __restrict__ pinfo, const double* __restrict__ cost,
                                                  const unsigned char* __restrict__ code,
                                                  const double* __restrict__ lf0, int64_t Fa,
                                                  double* __restrict__ results, int32_t* __restrict__ path) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int64_t* q = pinfo + (int64_t)p * PI_N;
  const int Ta = (int)q[4], Tb = (int)q[5];
  double* res = results + (int64_t)p * 8;
  if (Ta == 0) {
    if (lane < 8) res[lane] = NAN;
    return;
  }
  const int64_t coff = q[0];
  const double* lfa = lf0 + q[2];
  const double* lfb = lf0 + Fa + q[3];
  int32_t* pp = path ? path + 2 * (q[2] + q[3]) : nullptr;   // Ta + Tb entries reserved, at most Ta + Tb - 1 used
  int i = Ta - 1, j = Tb - 1;
  int64_t P = 0, nboth = 0, nmis = 0;
  double sum = 0.0, sq = 0.0;
  bool done = false;
  while (!done) {
    const int wi = i, wj = j;
    const int ii = wi - (lane >> 3), jj = wj - (lane & 7);
    const bool ok = ii >= 0 && jj >= 0;
    const int64_t o = coff + (ok ? diag_base(ii + jj, Ta, Tb) + ii : 0);
    const int cd = ok ? (int)code[o] : 0;
    const double cv = ok ? cost[o] : 0.0;
    const double la = (lane < 8 && wi - lane >= 0) ? lfa[wi - lane] : -1.0;
    const double lb = (lane < 8 && wj - lane >= 0) ? lfb[wj - lane] : -1.0;
    while (wi - i < 8 && wj - j < 8) {
      const int src = (wi - i) * 8 + (wj - j);
      const double d = __shfl(cv, src);
      int k = __shfl(cd, src);
      const double a = __shfl(la, wi - i), b = __shfl(lb, wj - j);
      sum = sum + d;
      const bool va = a >= 0.0, vb = b >= 0.0;
      if (va && vb) {
        const double e = a - b;
        sq = sq + e * e;
        ++nboth;
      } else if (va != vb) {
        ++nmis;
      }
      if (pp && lane == 0) {
        pp[2 * P] = i;
        pp[2 * P + 1] = j;
      }
      ++P;
      if (i == 0 && j == 0) {
        done = true;
        break;
      }
      if (i == 0) k = 2; else if (j == 0) k = 1;   // the border has one predecessor, whatever the byte says
      if (k == 0) { --i; --j; } else if (k == 1) { --i; } else { --j; }
    }
  }
  if (lane == 0) {
    res[0] = (MCD_DB_FACTOR * sum) / (double)P;
    res[1] = (double)P;
    res[3] = nboth > 0 ? sqrt(sq / (double)nboth) : NAN;
    res[4] = (double)nboth;
    res[5] = (double)nmis;
    res[6] = sum;
    res[7] = 0.0;
  }
}

}  // namespace

McdWs mcd_carve(void* ws, int n_pair, int64_t Fa, int64_t Fb, int64_t cells, int order) {
  McdWs w;
  char* p = (char*)ws;
  const int64_t F = Fa + Fb;
  w.mc = (double*)p;
  p += align256(F * (order + 1) * 8);
  w.lf0 = (double*)p;
  p += align256(F * 8);
  w.pinfo = (int64_t*)p;
  p += align256(((int64_t)n_pair + 1) * PI_N * 8);
  w.cost = (double*)p;
  p += align256(cells * 8);
  w.code = (unsigned char*)p;
  p += align256(cells);
  w.bytes = p - (char*)ws;
  return w;
}

int64_t mcd_workspace_bytes(int n_pair, int64_t Fa, int64_t Fb, int64_t cells, int order) {
  return mcd_carve(nullptr, n_pair, Fa, Fb, cells, order).bytes;
}

void launch_mcd_dtw(const float* spA, const float* enA, const float* f0A, const int64_t* offA, int64_t Fa,
                    const float* spB, const float* enB, const float* f0B, const int64_t* offB, int64_t Fb, int n_pair,
                    int64_t cells, const double* W, int order, double* results, int32_t* path, double* D, void* ws,
                    hipStream_t s) {
  const McdWs w = mcd_carve(ws, n_pair, Fa, Fb, cells, order);
  const int64_t F = Fa + Fb;
  k_mcd_prep<<<1, 64, 0, s>>>(offA, offB, n_pair, Fa, Fb, cells, w.pinfo);
  k_mcd_mcep<<<(unsigned)((F + MC_FR - 1) / MC_FR), 256, 0, s>>>(spA, enA, f0A, Fa, spB, enB, f0B, Fb, W, order, w.mc,
                                                                 w.lf0);
  // at most cells / (32 * 64) + Fa / 32 + Fb / 64 + n_pair tiles; the kernel strides over the count k_mcd_prep left
  int64_t grid = cells / (CT_I * CT_J) + Fa / CT_I + Fb / CT_J + n_pair;
  if (grid > COST_GRID) grid = COST_GRID;
  k_mcd_cost<<<(unsigned)grid, 256, 0, s>>>(w.pinfo, n_pair, w.mc, Fa, order, w.cost);
  k_mcd_dp<<<n_pair, DP_T, 0, s>>>(w.pinfo, w.cost, w.code, D, results);
  k_mcd_trace<<<n_pair, 64, 0, s>>>(w.pinfo, w.cost, w.code, w.lf0, Fa, results, path);
}

// host: W [(order + 1) x 513] with mc = W L: the one-sided real cepstrum of the 1024-point
// symmetric extension of L, then SPTK's freqt recursion from 513 coefficients to order + 1, run here on the 513 unit
// vectors at once
void mcep_matrix_host(int order, double alpha, double* W) {
  const int M1 = order + 1, N = MH;
  std::vector<double> G((size_t)M1 * N, 0.0), tab(1024);
  const double a = alpha, b = 1.0 - alpha * alpha;
  for (int i = N - 1; i >= 0; --i) {
    for (int n = i; n < N; ++n) {       // columns n < i are still zero
      double dprev = G[n];
      G[n] = (n == i ? 1.0 : 0.0) + a * dprev;
      double d1 = G[(size_t)N + n];
      G[(size_t)N + n] = b * dprev + a * d1;
      dprev = d1;
      for (int j = 2; j < M1; ++j) {
        const double dj = G[(size_t)j * N + n];
        G[(size_t)j * N + n] = dprev + a * (dj - G[(size_t)(j - 1) * N + n]);
        dprev = dj;
      }
    }
  }
  for (int qi = 0; qi < 1024; ++qi) tab[qi] = std::cos(PI_D * (double)qi / 512.0);
  for (int m = 0; m < M1; ++m)
    for (int k = 0; k < N; ++k) {
      const double wk = (k == 0 || k == N - 1) ? 1.0 : 2.0;
      double acc = 0.0;
      for (int n = 0; n < N; ++n) {
        const double en = (n == 0 || n == N - 1) ? 1.0 : 2.0;
        acc = acc + G[(size_t)m * N + n] * (en * tab[(n * k) & 1023]);
      }
      W[(size_t)m * N + k] = acc * wk / 1024.0;
    }
}

}  // namespace vaenpvc
