// Exact order statistics and quantiles of the stored draws (aehmc_summary_order_stats / _quantiles):
// the k-th smallest value of every coordinate of samples [R][D] by most-significant-digit radix select, without
// sorting anything.
//
// Keys.  A double maps to a 64-bit key that is monotone in its value: all bits of a negative are flipped, the sign bit
// of a non-negative is set.  -0.0 sorts just below +0.0, -inf / +inf are the smallest / largest ordinary keys, NaNs lie
// outside them (they are counted, and a coordinate that has one answers NaN for every rank).
//
// Choice of shape.  8-bit digits: 8 passes over the draws per sweep.  A tile is QUANTILE_TILE = 16 consecutive
// coordinates (a row segment of 128 contiguous bytes per draw), a sweep serves QUANTILE_RANKS = 8 ranks.  A
// workgroup's counters are [rank][coordinate][256 bins] 32-bit words in LDS, rows padded to 257 words so that the 16
// coordinates of one digit fall into 16 banks: 8 * 16 * 257 * 4 B = 131 584 B of the CU's 160 KiB (one workgroup per
// CU; fewer ranks or a narrower tile take proportionally less -- the size is dynamic).
//
// A pass.  (1) k_quantile_hist: every key is compared with the ranks' prefixes (the digits fixed so far); the ranks
// are ascending, so the ranks whose prefix a key matches are neighbours that share ONE prefix, and the key is counted
// once, under the first of them (the leader).  Several ranks therefore cost no more atomics than one -- in the first
// pass every key matches the empty prefix of all ranks and is counted once --, and the two neighbouring ranks of an
// interpolated quantile share their counters until their keys part.  Counts are integers: LDS atomics per workgroup,
// then one global atomic per non-empty bin, so the result does not depend on the order of arrival.  (2)
// k_quantile_select: per coordinate and rank, an inclusive scan of the leader's 256 bins finds the digit whose bin
// holds the rank; the digit joins the prefix, the bins below it are taken off the remaining rank.  After the last pass
// the prefix is the key of the order statistic.  Bytes read: 8 passes * R * D * 8 per sweep.
//
// Counts are 32-bit: R < 2^31.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {

constexpr int QUANTILE_THREADS = 256;
constexpr int QUANTILE_TILE = 16;     // coordinates per workgroup (narrower, a power of two, when D is smaller)
constexpr int QUANTILE_RANKS = 8;     // ranks per sweep
constexpr int QUANTILE_BINS = 256;    // 8-bit digits
constexpr int QUANTILE_PASSES = 8;
constexpr int QUANTILE_STRIDE = QUANTILE_BINS + 1;  // a counter row in LDS, padded by one bank
constexpr int QUANTILE_INFLIGHT = 4;  // draws a lane loads before it counts the first of them
constexpr int QUANTILE_MAX = 64;      // ranks of one order_stats call, probabilities of one quantiles call
constexpr int QUANTILE_MAX_STATS = 2 * QUANTILE_MAX;  // distinct ranks behind QUANTILE_MAX interpolated quantiles

__device__ inline unsigned long long quantile_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ inline double quantile_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
  return __longlong_as_double((long long)b);
}

// the caller's scratch: counters, prefixes and remaining ranks of one sweep, NaN counts, the selected order statistics
struct QuantileWork {
  unsigned *hist;              // [D][ranks of the sweep][256]; room for min(QUANTILE_RANKS, 2 M) ranks
  unsigned long long *prefix;  // [D][QUANTILE_RANKS]
  unsigned *krem;              // [D][QUANTILE_RANKS]
  unsigned *nan;               // [D]
  double *stats;               // [2 M][D]
  size_t bytes;
};
inline QuantileWork quantile_work(void *base, long long D, long long M) {
  auto up = [](size_t n) { return (n + 255) / 256 * 256; };
  char *p = (char *)base;
  QuantileWork w;
  size_t off = 0;
  w.hist = (unsigned *)(p + off);
  off += up((size_t)D * (size_t)(2 * M < QUANTILE_RANKS ? 2 * M : QUANTILE_RANKS) * QUANTILE_BINS * sizeof(unsigned));
  w.prefix = (unsigned long long *)(p + off);
  off += up((size_t)D * QUANTILE_RANKS * sizeof(unsigned long long));
  w.krem = (unsigned *)(p + off);
  off += up((size_t)D * QUANTILE_RANKS * sizeof(unsigned));
  w.nan = (unsigned *)(p + off);
  off += up((size_t)D * sizeof(unsigned));
  w.stats = (double *)(p + off);
  off += up((size_t)2 * M * D * sizeof(double));
  w.bytes = off;
  return w;
}

struct QuantileRanks {
  unsigned r[QUANTILE_RANKS];
};

// a sweep starts from empty prefixes and its ranks; the NaN counts start with the first sweep and serve them all
__global__ __launch_bounds__(QUANTILE_THREADS) void k_quantile_init(unsigned long long *__restrict__ prefix,
                                                                    unsigned *__restrict__ krem,
                                                                    unsigned *__restrict__ nan, long long D,
                                                                    QuantileRanks ranks, int first_sweep) {
  const long long i = (long long)blockIdx.x * QUANTILE_THREADS + threadIdx.x;
  if (i >= D * QUANTILE_RANKS) return;
  prefix[i] = 0;
  krem[i] = ranks.r[i % QUANTILE_RANKS];
  if (first_sweep && i < D) nan[i] = 0;
}

struct QuantileHistArgs {
  const double *x;                   // [R][D]
  const unsigned long long *prefix;  // [D][QUANTILE_RANKS]
  unsigned *hist;                    // [D][M][256], zeros
  unsigned *nan;                     // [D]
  long long R, D, rows_per_chunk;
  unsigned long long mask;           // the key bits above this pass's digit (0 in the first pass)
  int M, tw_log2, shift, count_nan;  // M ranks, tile of 1 << tw_log2 coordinates, digit = (key >> shift) & 255
};

// Workgroup (x: tile of coordinates, y: chunk of draws).  Lane (c, rl) walks the draws rl, rl + 256 / tw, ... of its
// chunk at coordinate c: the tw lanes of a draw read one contiguous row segment.  A lane's coordinate never changes,
// so it keeps the M prefixes of that coordinate in registers.
__global__ __launch_bounds__(QUANTILE_THREADS) void k_quantile_hist(QuantileHistArgs a) {
  extern __shared__ unsigned s_hist[];  // [M][tw][QUANTILE_STRIDE]
  __shared__ unsigned s_nan[QUANTILE_TILE];
  const int tid = threadIdx.x, tw = 1 << a.tw_log2, c = tid & (tw - 1), rl = tid >> a.tw_log2;
  const int rpi = QUANTILE_THREADS >> a.tw_log2;  // draws per step of the workgroup
  const long long d = (long long)blockIdx.x * tw + c;
  const bool live = d < a.D;
  const int words = a.M * tw * QUANTILE_STRIDE;
  for (int i = tid; i < words; i += QUANTILE_THREADS) s_hist[i] = 0;
  if (tid < QUANTILE_TILE) s_nan[tid] = 0;
  unsigned long long pref[QUANTILE_RANKS];
#pragma unroll
  for (int r = 0; r < QUANTILE_RANKS; ++r) pref[r] = (live && r < a.M) ? a.prefix[d * QUANTILE_RANKS + r] : 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.y * a.rows_per_chunk;
  const long long r1 = r0 + a.rows_per_chunk < a.R ? r0 + a.rows_per_chunk : a.R;
  if (live) {
    for (long long row = r0 + rl; row < r1; row += (long long)rpi * QUANTILE_INFLIGHT) {
      double v[QUANTILE_INFLIGHT];
#pragma unroll
      for (int j = 0; j < QUANTILE_INFLIGHT; ++j) {
        const long long rr = row + (long long)j * rpi;
        v[j] = rr < r1 ? a.x[rr * a.D + d] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < QUANTILE_INFLIGHT; ++j) {
        if (row + (long long)j * rpi >= r1) break;
        const unsigned long long key = quantile_key(v[j]), kp = key & a.mask;
        int lead = -1;
#pragma unroll
        for (int r = QUANTILE_RANKS - 1; r >= 0; --r)
          if (r < a.M && kp == pref[r]) lead = r;
        if (lead >= 0) atomicAdd(&s_hist[(lead * tw + c) * QUANTILE_STRIDE + (int)((key >> a.shift) & 255)], 1u);
        if (a.count_nan && v[j] != v[j]) atomicAdd(&s_nan[c], 1u);
      }
    }
  }
  __syncthreads();
  const int bins = a.M * tw * QUANTILE_BINS;
  for (int i = tid; i < bins; i += QUANTILE_THREADS) {
    const int digit = i & (QUANTILE_BINS - 1), rc = i >> 8, cc = rc & (tw - 1), r = rc >> a.tw_log2;
    const unsigned n = s_hist[rc * QUANTILE_STRIDE + digit];
    const long long dd = (long long)blockIdx.x * tw + cc;
    if (n && dd < a.D) atomicAdd(&a.hist[(dd * a.M + r) * QUANTILE_BINS + digit], n);
  }
  if (a.count_nan && tid < tw && live && s_nan[tid]) atomicAdd(&a.nan[d], s_nan[tid]);
}

// One workgroup per coordinate, one lane per bin.  Rank r reads the counters of its leader: the first rank that has
// the same prefix (the prefixes ascend with the ranks).  The prefixes and the remaining ranks are read into LDS before
// any is rewritten: no lane reads from global memory a word that another lane of the workgroup writes.
__global__ __launch_bounds__(QUANTILE_THREADS) void k_quantile_select(const unsigned *__restrict__ hist,
                                                                      unsigned long long *__restrict__ prefix,
                                                                      unsigned *__restrict__ krem, int M, int shift) {
  __shared__ unsigned long long s_pref[QUANTILE_RANKS];
  __shared__ unsigned s_k[QUANTILE_RANKS];
  __shared__ unsigned s_scan[2][QUANTILE_BINS];
  const long long d = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < M) {
    s_pref[tid] = prefix[d * QUANTILE_RANKS + tid];
    s_k[tid] = krem[d * QUANTILE_RANKS + tid];
  }
  __syncthreads();
  for (int r = 0; r < M; ++r) {
    int lead = r;
    while (lead > 0 && s_pref[lead - 1] == s_pref[r]) --lead;
    const unsigned cnt = hist[(d * M + lead) * QUANTILE_BINS + tid];
    int cur = 0;
    s_scan[0][tid] = cnt;
    __syncthreads();
    for (int off = 1; off < QUANTILE_BINS; off <<= 1) {
      const unsigned v = s_scan[cur][tid] + (tid >= off ? s_scan[cur][tid - off] : 0u);
      s_scan[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const unsigned incl = s_scan[cur][tid], excl = incl - cnt, k = s_k[r];
    if (excl <= k && k < incl) {  // (one lane: the bins of a prefix hold more keys than the rank that remains)
      prefix[d * QUANTILE_RANKS + r] = s_pref[r] | ((unsigned long long)tid << shift);
      krem[d * QUANTILE_RANKS + r] = k - excl;
    }
    __syncthreads();
  }
}

// stats[r][d] of a sweep: the value of the selected key, NaN where the coordinate has one
__global__ __launch_bounds__(QUANTILE_THREADS) void k_quantile_write(const unsigned long long *__restrict__ prefix,
                                                                     const unsigned *__restrict__ nan,
                                                                     double *__restrict__ stats, long long D, int M) {
  const long long i = (long long)blockIdx.x * QUANTILE_THREADS + threadIdx.x;
  if (i >= D * M) return;
  const long long r = i / D, d = i % D;
  stats[i] = nan[d] ? __longlong_as_double(0x7ff8000000000000LL) : quantile_unkey(prefix[d * QUANTILE_RANKS + r]);
}

struct QuantileOutArgs {
  const double *stats;  // [U][D]
  double *out;          // [n][D]
  long long D;
  int n, interpolate;
  unsigned char lo[QUANTILE_MAX], hi[QUANTILE_MAX];  // rows of stats
  double g[QUANTILE_MAX];
};

// order statistics: out = stats[lo].  Quantiles: numpy's "linear" rule (R type 7) between a = x_(lo) and b = x_(hi) at
// the fraction g -- its two-sided form, which is exact at both ends.
__global__ __launch_bounds__(QUANTILE_THREADS) void k_quantile_out(QuantileOutArgs a) {
  const long long i = (long long)blockIdx.x * QUANTILE_THREADS + threadIdx.x;
  if (i >= a.D * a.n) return;
  const long long q = i / a.D, d = i % a.D;
  const double lo = a.stats[(long long)a.lo[q] * a.D + d];
  if (!a.interpolate) {
    a.out[i] = lo;
    return;
  }
  const double hi = a.stats[(long long)a.hi[q] * a.D + d], g = a.g[q], diff = hi - lo;
  a.out[i] = g < 0.5 ? lo + diff * g : hi - diff * (1.0 - g);
}

// The U distinct ascending ranks (host array, U <= QUANTILE_MAX_STATS, each in [0, R)) of every coordinate of
// x [R][D] into w.stats [U][D]: ceil(U / QUANTILE_RANKS) sweeps of QUANTILE_PASSES passes.
inline hipError_t launch_quantile_stats(const double *x, long long R, long long D, int U, const long long *ranks,
                                        const QuantileWork &w, hipStream_t st) {
  int twl = 4;  // the tile: 16 coordinates, or the power of two that holds D
  while (twl > 0 && (1LL << (twl - 1)) >= D) --twl;
  const int tw = 1 << twl, rpi = QUANTILE_THREADS / tw;
  const long long tiles = (D + tw - 1) / tw;
  // about 1024 workgroups in all; a chunk is at least 128 steps of a workgroup, so that zeroing and flushing its
  // counters stays small beside counting
  long long chunks = (1024 + tiles - 1) / tiles;
  const long long most = (R + 128LL * rpi - 1) / (128LL * rpi);
  if (chunks > most) chunks = most;
  if (chunks > 65535) chunks = 65535;
  const long long rows_per_chunk = (R + chunks - 1) / chunks;
  chunks = (R + rows_per_chunk - 1) / rows_per_chunk;
  // up to 8 * 16 * 257 counters of dynamic LDS; asked for on every call (no state shared between threads or devices)
  if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_quantile_hist),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(QUANTILE_RANKS * QUANTILE_TILE * QUANTILE_STRIDE * sizeof(unsigned)));
      e != hipSuccess)
    return e;
  const unsigned dr_blocks = (unsigned)((D * QUANTILE_RANKS + QUANTILE_THREADS - 1) / QUANTILE_THREADS);
  for (int u0 = 0; u0 < U; u0 += QUANTILE_RANKS) {
    const int M = U - u0 < QUANTILE_RANKS ? U - u0 : QUANTILE_RANKS;
    QuantileRanks rk;
    for (int r = 0; r < QUANTILE_RANKS; ++r) rk.r[r] = r < M ? (unsigned)ranks[u0 + r] : 0u;
    hipLaunchKernelGGL(k_quantile_init, dim3(dr_blocks), dim3(QUANTILE_THREADS), 0, st, w.prefix, w.krem, w.nan, D, rk,
                       (int)(u0 == 0));
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    for (int p = 0; p < QUANTILE_PASSES; ++p) {
      if (hipError_t e = hipMemsetAsync(w.hist, 0, (size_t)D * M * QUANTILE_BINS * sizeof(unsigned), st);
          e != hipSuccess)
        return e;
      QuantileHistArgs a;
      a.x = x; a.prefix = w.prefix; a.hist = w.hist; a.nan = w.nan;
      a.R = R; a.D = D; a.rows_per_chunk = rows_per_chunk;
      a.shift = 64 - 8 * (p + 1);
      a.mask = p == 0 ? 0ULL : ~0ULL << (a.shift + 8);
      a.M = M; a.tw_log2 = twl; a.count_nan = u0 == 0 && p == 0;
      const size_t dyn = (size_t)M * tw * QUANTILE_STRIDE * sizeof(unsigned);
      hipLaunchKernelGGL(k_quantile_hist, dim3((unsigned)tiles, (unsigned)chunks), dim3(QUANTILE_THREADS), dyn, st, a);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
      hipLaunchKernelGGL(k_quantile_select, dim3((unsigned)D), dim3(QUANTILE_THREADS), 0, st,
                         (const unsigned *)w.hist, w.prefix, w.krem, M, a.shift);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_quantile_write, dim3((unsigned)((D * M + QUANTILE_THREADS - 1) / QUANTILE_THREADS)),
                       dim3(QUANTILE_THREADS), 0, st, (const unsigned long long *)w.prefix, (const unsigned *)w.nan,
                       w.stats + (long long)u0 * D, D, M);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

inline hipError_t launch_quantile_out(const QuantileOutArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_quantile_out, dim3((unsigned)((a.D * a.n + QUANTILE_THREADS - 1) / QUANTILE_THREADS)),
                     dim3(QUANTILE_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
