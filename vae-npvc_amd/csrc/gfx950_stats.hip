// gfx950_stats.hip -- the training-set statistics of build.py --device: exact per-column order
// statistics (the 0.5 / 99.5 percentiles behind etc/xmin.npf, xmax.npf) and the per-speaker log-F0 and global-variance
// statistics.  Nothing here allocates or synchronises with the host, and there is no floating-point atomic: the only
// atomics are integer adds into histograms (LDS, then global) and one integer OR, so every call returns the same bytes.
//
// Column select.  x [F, H] fp32 with row stride ld; for each of n_rank <= 8 zero-based ranks and each column, the
// element np.sort(x[:, h])[rank].  MSB-first radix select, 8 bits per pass, on the order-preserving uint32 image of the
// float bits (negative: all bits flipped, otherwise the sign bit flipped; -0.0 sorts just below +0.0):
//   k_sel_init     clears the histograms and the flag, seeds (prefix = 0, remaining rank = rank, leader = 0)
//   k_sel_hist     pass p = 0..3: one workgroup per (row slice, 64 columns, slot); 8 waves, a wave reads 64 consecutive
//                  columns of a row (256 contiguous bytes, one dword per lane) and 16 rows are in flight per thread.  An
//                  element whose top 8 p key bits equal the slot's prefix adds 1 to the LDS histogram [digit][column] (a
//                  wave's 64 lanes are 64 columns = 64 banks: no bank conflict whatever the data).  The workgroup then
//                  adds its non-zero LDS counts to the global histogram [slot][column][256].  Pass 0 has one slot shared
//                  by every rank and sets bit 0 of the flag on a NaN or +-Inf.
//   k_sel_narrow   one workgroup per column: per rank, the scan of its 256 counts picks the digit that holds the
//                  remaining rank, extends the prefix and reduces the remaining rank.  Ranks whose prefixes are equal
//                  share one slot from then on (the leader = the lowest such rank): a (workgroup, slot) of k_sel_hist
//                  without a leading column exits before it reads a row, so the two ranks that bracket a percentile
//                  cost one pass over x, not two, for as long as they agree.  The last pass writes the values.
// Passes over x: 1 + 3 * (distinct prefixes alive), at most 1 + 3 n_rank.  Counts are uint32 (F < 2^31).
//
// Speaker statistics.  Utterance u is rows off[u] .. off[u+1] of sp / f0, speaker spk[u].
//   k_ss_utt       one workgroup per (utterance of N >= 2 frames, 64 bins): two-pass biased variance in fp64 (wave w takes
//                  rows w, w + 8, ...; the eight partial sums are added in order)
//   k_ss_f0        one workgroup per utterance: count, mean and M2 of ln f0 over f0 > 2, two passes, fixed-tree sums
//   k_ss_final     per speaker: the utterance variances summed in offset order / their number; the (count, mean, M2)
//                  triples merged in offset order (Chan et al.), std = sqrt(M2 / count)
// Every order depends only on the utterance's length resp. on the speaker's utterances in offset order: a speaker's
// results are the same bytes wherever its utterances stand among the others'.  Offsets are clamped to [0, F] and a
// speaker id outside [0, n_spk) matches no speaker, so malformed arrays cannot make a kernel leave its buffers.
#include "kernels.h"

namespace vaenpvc {

namespace {

constexpr int SEL_COLS = 64;                // columns per workgroup
constexpr int SEL_W = 8;                    // waves per histogram workgroup
constexpr int SEL_U = 16;                   // rows per thread and step, all loads in flight at once
constexpr int SEL_ROWS = SEL_W * SEL_U;     // rows per workgroup step
constexpr int SEL_MIN_ROWS = 2048;          // rows a workgroup takes at least (against the 16 K-bin clear and flush)
constexpr int SEL_MAX_SLICES = 256;         // row slices at most
constexpr int SS_W = 8;                     // waves of k_ss_utt

__device__ __forceinline__ uint32_t sel_key(uint32_t b) { return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u); }
__device__ __forceinline__ uint32_t sel_unkey(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

struct SelRanks {
  uint32_t r[SEL_MAX_RANKS];
};

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct SelWs {
  uint32_t* hist;    // [n_rank, H, 256]
  uint32_t* prefix;  // [n_rank, H]
  uint32_t* krem;    // [n_rank, H] rank among the elements that share the prefix
  int32_t* lead;     // [n_rank, H] slot whose histogram the rank reads
  int64_t bytes;
};

SelWs sel_carve(void* ws, int H, int n_rank) {
  const int64_t nh = align256((int64_t)n_rank * H * 256 * 4), ns = align256((int64_t)n_rank * H * 4);
  char* p = (char*)ws;
  SelWs w;
  w.hist = (uint32_t*)p;
  w.prefix = (uint32_t*)(p + nh);
  w.krem = (uint32_t*)(p + nh + ns);
  w.lead = (int32_t*)(p + nh + 2 * ns);
  w.bytes = nh + 3 * ns;
  return w;
}

// row slices of the histogram grid and rows per slice (a multiple of SEL_ROWS)
void sel_slices(int64_t F, int& n_slice, int64_t& rows) {
  int64_t s = (F + SEL_MIN_ROWS - 1) / SEL_MIN_ROWS;
  s = s < 1 ? 1 : (s > SEL_MAX_SLICES ? SEL_MAX_SLICES : s);
  rows = ((F + s - 1) / s + SEL_ROWS - 1) / SEL_ROWS * SEL_ROWS;
  n_slice = (int)s;
}

}  // namespace

__global__ void __launch_bounds__(256) k_sel_init(int64_t n_hist, int n_state, int H, SelRanks ranks,
                                                  uint32_t* __restrict__ hist, uint32_t* __restrict__ prefix,
                                                  uint32_t* __restrict__ krem, int32_t* __restrict__ lead,
                                                  int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_hist) hist[i] = 0u;
  if (i < n_state) {
    prefix[i] = 0u;
    krem[i] = ranks.r[i / H];
    lead[i] = 0;
  }
  if (i == 0) *flag = 0;
}

__global__ void __launch_bounds__(64 * SEL_W) k_sel_hist(const float* __restrict__ x, int64_t F, int H, uint32_t ld,
                                                         int64_t rows, int pass, const uint32_t* __restrict__ prefix,
                                                         const int32_t* __restrict__ lead, uint32_t* __restrict__ hist,
                                                         int32_t* __restrict__ flag) {
  __shared__ uint32_t sh[256 * SEL_COLS];  // [digit][column]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.z, c0 = blockIdx.y * SEL_COLS, col = c0 + lane;
  const bool on = col < H;
  const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min(F, r0 + rows);
  if (r0 >= r1) return;  // uniform
  bool act = on;
  uint32_t pfx = 0u;
  if (pass > 0) {
    act = on && lead[(int64_t)g * H + col] == g;
    pfx = on ? prefix[(int64_t)g * H + col] : 0u;
    if (__ballot(act) == 0) return;  // every wave of the workgroup holds the same 64 columns: uniform
  }
  for (int i = threadIdx.x; i < 256 * SEL_COLS; i += 64 * SEL_W) sh[i] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
  const uint32_t oc = on ? (uint32_t)col : (uint32_t)c0;
  bool bad = false;
  for (int64_t rb = r0; rb < r1; rb += SEL_ROWS) {
    const float* p = x + rb * (int64_t)ld;  // uniform; offsets below fit 32 bits: SEL_ROWS * ld <= 2^31
    const int n = (int)min((int64_t)SEL_ROWS, r1 - rb);
    uint32_t v[SEL_U];
#pragma unroll
    for (int j = 0; j < SEL_U; ++j)  // unconditional loads (rows past the slice re-read its last row): all in flight
      v[j] = __float_as_uint(p[(uint32_t)min(w + j * SEL_W, n - 1) * ld + oc]);
#pragma unroll
    for (int j = 0; j < SEL_U; ++j) {
      if (w + j * SEL_W < n && act) {
        const uint32_t k = sel_key(v[j]);
        if (pass == 0) bad |= (v[j] & 0x7f800000u) == 0x7f800000u;
        if (((k ^ pfx) & himask) == 0u) atomicAdd(&sh[((k >> shift) & 255u) * SEL_COLS + lane], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256 * SEL_COLS; i += 64 * SEL_W) {
    const uint32_t c = sh[i];
    const int cc = c0 + (i & (SEL_COLS - 1));
    if (c != 0u && cc < H) atomicAdd(&hist[((int64_t)g * H + cc) * 256 + (i / SEL_COLS)], c);
  }
  if (__ballot(bad) != 0 && lane == 0) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(256) k_sel_narrow(int pass, int H, int n_rank, uint32_t* __restrict__ hist,
                                                    uint32_t* __restrict__ prefix, uint32_t* __restrict__ krem,
                                                    int32_t* __restrict__ lead, float* __restrict__ out) {
  __shared__ uint32_t sc[256];
  __shared__ uint32_t np[SEL_MAX_RANKS];
  const int h = blockIdx.x, t = threadIdx.x;
  const int shift = 24 - 8 * pass;
  if (t < n_rank) np[t] = prefix[(int64_t)t * H + h];
  __syncthreads();
  for (int r = 0; r < n_rank; ++r) {
    const int64_t st = (int64_t)r * H + h;
    const int g = min(max(lead[st], 0), r);
    const uint32_t c = hist[((int64_t)g * H + h) * 256 + t];
    sc[t] = c;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      const uint32_t a = t >= o ? sc[t - o] : 0u;
      __syncthreads();
      sc[t] += a;
      __syncthreads();
    }
    const uint32_t incl = sc[t], excl = incl - c, k = krem[st];
    if (excl <= k && k < incl) {  // one thread at most
      const uint32_t q = np[r] | ((uint32_t)t << shift);
      np[r] = q;
      prefix[st] = q;
      krem[st] = k - excl;
    }
    __syncthreads();
  }
  if (t < n_rank) {
    int g = t;
    for (int r = t - 1; r >= 0; --r)
      if (np[r] == np[t]) g = r;
    lead[(int64_t)t * H + h] = g;
    if (pass == 3) out[(int64_t)t * H + h] = __uint_as_float(sel_unkey(np[t]));
  }
  for (int r = 0; r < n_rank; ++r) hist[((int64_t)r * H + h) * 256 + t] = 0u;  // each thread clears the bins it read
}

__global__ void __launch_bounds__(64 * SS_W) k_ss_utt(const float* __restrict__ sp, int64_t ld, const int64_t* __restrict__ off,
                                                      int64_t F, int H, double* __restrict__ uvar) {
  __shared__ double sh[SS_W][64];
  const int u = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t s = min(max(off[u], (int64_t)0), F), e = min(max(off[u + 1], s), F), N = e - s;
  if (N < 2) return;  // uniform
  const int col = blockIdx.y * 64 + lane;
  const bool on = col < H;
  const float* p = sp + s * ld + (on ? col : blockIdx.y * 64);
  double acc = 0.0;
#pragma unroll 8
  for (int64_t i = w; i < N; i += SS_W) acc += (double)p[i * ld];
  sh[w][lane] = acc;
  __syncthreads();
  double mean = 0.0;
  for (int k = 0; k < SS_W; ++k) mean += sh[k][lane];
  mean /= (double)N;
  __syncthreads();
  acc = 0.0;
#pragma unroll 8
  for (int64_t i = w; i < N; i += SS_W) {
    const double d = (double)p[i * ld] - mean;
    acc += d * d;
  }
  sh[w][lane] = acc;
  __syncthreads();
  if (w != 0 || !on) return;
  double m2 = 0.0;
  for (int k = 0; k < SS_W; ++k) m2 += sh[k][lane];
  uvar[(int64_t)u * H + col] = m2 / (double)N;
}

__global__ void __launch_bounds__(256) k_ss_f0(const float* __restrict__ f0, int64_t ld, const int64_t* __restrict__ off,
                                               int64_t F, double* __restrict__ ustat) {
  __shared__ double sh[256];
  __shared__ double shc[256];
  const int u = blockIdx.x, t = threadIdx.x;
  const int64_t s = min(max(off[u], (int64_t)0), F), e = min(max(off[u + 1], s), F), N = e - s;
  const float* p = f0 + s * ld;
  double sum = 0.0, cnt = 0.0;  // counts stay exact in fp64 (< 2^31)
  for (int64_t i = t; i < N; i += 256) {
    const float v = p[i * ld];
    if (v > 2.f) {
      sum += log((double)v);
      cnt += 1.0;
    }
  }
  sh[t] = sum;
  shc[t] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      sh[t] += sh[t + o];
      shc[t] += shc[t + o];
    }
    __syncthreads();
  }
  const double n = shc[0], mean = n > 0.0 ? sh[0] / n : 0.0;
  __syncthreads();
  double m2 = 0.0;
  for (int64_t i = t; i < N; i += 256) {
    const float v = p[i * ld];
    if (v > 2.f) {
      const double d = log((double)v) - mean;
      m2 += d * d;
    }
  }
  sh[t] = m2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) {
    ustat[(int64_t)u * 3 + 0] = n;
    ustat[(int64_t)u * 3 + 1] = mean;
    ustat[(int64_t)u * 3 + 2] = sh[0];
  }
}

__global__ void __launch_bounds__(256) k_ss_final(const int64_t* __restrict__ off, const int32_t* __restrict__ spk,
                                                  int n_seg, int64_t F, int H, const double* __restrict__ uvar,
                                                  const double* __restrict__ ustat, double* __restrict__ lf0,
                                                  double* __restrict__ gv, int64_t* __restrict__ n_utt) {
  const int sid = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
  const bool on = col < H;
  double acc = 0.0;
  int64_t nu = 0;
  for (int u = 0; u < n_seg; ++u) {
    if (spk[u] != sid) continue;  // uniform
    const int64_t s = min(max(off[u], (int64_t)0), F), e = min(max(off[u + 1], s), F);
    if (e - s < 2) continue;
    if (on) acc += uvar[(int64_t)u * H + col];
    ++nu;
  }
  if (on) gv[(int64_t)sid * H + col] = nu > 0 ? acc / (double)nu : __builtin_nan("");
  if (blockIdx.y != 0 || threadIdx.x != 0) return;
  n_utt[sid] = nu;
  double tn = 0.0, tm = 0.0, t2 = 0.0;
  for (int u = 0; u < n_seg; ++u) {
    if (spk[u] != sid) continue;
    const double nb = ustat[(int64_t)u * 3], mb = ustat[(int64_t)u * 3 + 1];
    if (!(nb > 0.0)) continue;
    const double nn = tn + nb, dl = mb - tm;
    tm += dl * (nb / nn);
    t2 += ustat[(int64_t)u * 3 + 2] + dl * dl * (tn * nb / nn);
    tn = nn;
  }
  lf0[sid * 3 + 0] = tn;
  lf0[sid * 3 + 1] = tn > 0.0 ? tm : __builtin_nan("");
  lf0[sid * 3 + 2] = tn > 0.0 ? sqrt(t2 / tn) : __builtin_nan("");
}

int64_t column_select_workspace_bytes(int H, int n_rank) { return sel_carve(nullptr, H, n_rank).bytes; }

void launch_column_select(const float* x, int64_t F, int H, int64_t ld, const int64_t* ranks, int n_rank, float* out,
                          int32_t* flag, void* ws, hipStream_t s) {
  const SelWs w = sel_carve(ws, H, n_rank);
  SelRanks rk = {};
  for (int r = 0; r < n_rank; ++r) rk.r[r] = (uint32_t)ranks[r];
  const int64_t n_hist = (int64_t)n_rank * H * 256;
  hipLaunchKernelGGL(k_sel_init, dim3((unsigned)((n_hist + 255) / 256)), dim3(256), 0, s, n_hist, n_rank * H, H, rk,
                     w.hist, w.prefix, w.krem, w.lead, flag);
  int n_slice;
  int64_t rows;
  sel_slices(F, n_slice, rows);
  const unsigned cg = (unsigned)((H + SEL_COLS - 1) / SEL_COLS);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(k_sel_hist, dim3((unsigned)n_slice, cg, pass == 0 ? 1u : (unsigned)n_rank), dim3(64 * SEL_W), 0, s,
                       x, F, H, (uint32_t)ld, rows, pass, w.prefix, w.lead, w.hist, flag);
    hipLaunchKernelGGL(k_sel_narrow, dim3((unsigned)H), dim3(256), 0, s, pass, H, n_rank, w.hist, w.prefix, w.krem,
                       w.lead, out);
  }
}

int64_t speaker_stats_workspace_bytes(int n_seg, int H) {
  return align256((int64_t)n_seg * H * 8) + align256((int64_t)n_seg * 3 * 8);
}

void launch_speaker_stats(const float* sp, int64_t ld_sp, const float* f0, int64_t ld_f0, const int64_t* off,
                          const int32_t* spk, int n_seg, int n_spk, int64_t F, int H, double* lf0, double* gv,
                          int64_t* n_utt, void* ws, hipStream_t s) {
  double* uvar = (double*)ws;
  double* ustat = (double*)((char*)ws + align256((int64_t)n_seg * H * 8));
  hipLaunchKernelGGL(k_ss_utt, dim3((unsigned)n_seg, (unsigned)((H + 63) / 64)), dim3(64 * SS_W), 0, s, sp, ld_sp, off, F, H,
                     uvar);
  hipLaunchKernelGGL(k_ss_f0, dim3((unsigned)n_seg), dim3(256), 0, s, f0, ld_f0, off, F, ustat);
  hipLaunchKernelGGL(k_ss_final, dim3((unsigned)n_spk, (unsigned)((H + 255) / 256)), dim3(256), 0, s, off, spk, n_seg, F, H,
                     uvar, ustat, lf0, gv, n_utt);
}

}  // namespace vaenpvc
