// Average ranks and normal scores of the stored draws (aehmc_summary_rank): for every draw of
// samples [R][D] its rank among the R draws of its coordinate, r = #{y < x} + (#{y == x} + 1) / 2 (1-based, ties share
// the mean of their places: scipy.stats.rankdata(method="average")), or the normal score z = Phi^-1((r - 3/8) /
// (R + 1/4)) that the rank-normalised split R-hat and the bulk ESS are computed from.  With a centre c [D] the ranks
// are those of the folded draws |x - c[d]|.
//
// Shape.  A tile is T consecutive coordinates (as many as the caller's scratch holds); per tile:
//  (1) k_rank_keys: row segments of the tile are read, every value maps to the monotone 64-bit key of quantile.cuh
//      (-0.0 first made +0.0, so that the zeros tie) and the keys are written transposed, as contiguous columns
//      [T][R]; 16 coordinates x 256 rows go through LDS so that reads and writes are both coalesced.  NaNs are counted
//      per coordinate (integer atomics).
//  (2) a segmented least-significant-digit radix sort of the columns, keys only, 8-bit digits: 8 passes between two
//      column buffers.  A column is cut into NB <= 1024 chunks of >= 4096 keys, one workgroup each.  Per pass:
//      k_rank_count (the chunk's 256 digit counts), k_rank_scan (per column, the exclusive scan over (digit, chunk) in
//      place), k_rank_scatter (stable: a key's place is its chunk's scanned offset + the keys of its digit before it
//      in the chunk, which wave ballots and a scan over (sub-round, wave) give).  Every position comes from counts and
//      scans, none from the order in which atomics arrive: the sorted column is the same bits on every run.
//  (3) k_rank_out: the row segments are read again, a draw's key is recomputed and its lower and upper bound are
//      searched in its sorted column: r = (lo + hi + 1) / 2, exact in fp64.  Ties need no pass of their own.  A
//      coordinate with a NaN answers NaN for every draw.
// Steps (1) and (2) are launch_rank_sort; posterior.cuh (HDI, MCSE of a quantile) reads the sorted columns it leaves.
//
// Cost of the 8-bit digit: 8 passes, each reading the keys twice and writing them once (24 R T bytes); the scatter
// holds 2 x 16 x 257 counters (32 896 B of LDS) and its 256 offsets, the count 256 counters; registers stay far below
// any occupancy limit (make resource-usage).  Counts are 32-bit: R < 2^31.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {

constexpr int RANK_THREADS = 256;
constexpr int RANK_WAVES = RANK_THREADS / 64;
constexpr int RANK_TILE = 16;                                   // coordinates per workgroup of (1) and (3)
constexpr int RANK_BINS = 256;                                  // 8-bit digits
constexpr int RANK_PASSES = 8;
constexpr int RANK_STRIDE = RANK_BINS + 1;                      // a counter row in LDS, padded by one bank
constexpr int RANK_SUB = 4;                                     // keys of a lane per round of the scatter
constexpr int RANK_ROUND = RANK_THREADS * RANK_SUB;             // keys of a workgroup per round
constexpr long long RANK_CHUNK = 4 * RANK_ROUND;                // keys of a chunk, at least
constexpr long long RANK_MAX_CHUNKS = 1024;                     // chunks of a column, at most
constexpr long long RANK_MAX_TILE = 32768;                      // coordinates of a tile, at most (a grid dimension)
constexpr size_t RANK_DEFAULT_WORK = (size_t)256 << 20;         // the default scratch stays under this, if one
                                                                // coordinate's need does

// quantile.cuh's quantile_key (restated: that header defines kernels, which belong to one translation unit): all bits
// of a negative flipped, the sign bit of a non-negative set -- monotone in the value
__device__ inline unsigned long long rank_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
// its inverse: the value whose key this is
__device__ inline double rank_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k));
}
// the value that is ranked: folded about the centre if there is one, and -0.0 made +0.0 so that the zeros tie
__device__ inline double rank_value(double v, const double *centre, long long d) {
  if (centre) v = fabs(v - centre[d]);
  return v == 0.0 ? 0.0 : v;
}

inline long long rank_chunk(long long R) {
  long long per = (R + RANK_MAX_CHUNKS - 1) / RANK_MAX_CHUNKS;
  per = (per + RANK_ROUND - 1) / RANK_ROUND * RANK_ROUND;
  return per < RANK_CHUNK ? RANK_CHUNK : per;
}
inline long long rank_chunks(long long R) { return (R + rank_chunk(R) - 1) / rank_chunk(R); }

// the caller's scratch for a tile of T coordinates
struct RankWork {
  unsigned long long *keys[2];  // [T][R] each
  unsigned *counts;             // [T][chunks][256]
  unsigned *nan;                // [T]
  size_t bytes;
};
inline RankWork rank_work(void *base, long long R, long long T) {
  auto up = [](size_t n) { return (n + 255) / 256 * 256; };
  char *p = (char *)base;
  RankWork w;
  size_t off = 0;
  for (int i = 0; i < 2; ++i) {
    w.keys[i] = (unsigned long long *)(p + off);
    off += up((size_t)T * (size_t)R * sizeof(unsigned long long));
  }
  w.counts = (unsigned *)(p + off);
  off += up((size_t)T * (size_t)rank_chunks(R) * RANK_BINS * sizeof(unsigned));
  w.nan = (unsigned *)(p + off);
  off += up((size_t)T * sizeof(unsigned));
  w.bytes = off;
  return w;
}
// the widest tile (<= D, <= RANK_MAX_TILE) whose scratch fits `bytes`; 0 if not even one coordinate's does
inline long long rank_tile(long long R, long long D, size_t bytes) {
  long long lo = 0, hi = D < RANK_MAX_TILE ? D : RANK_MAX_TILE;  // (lo fits, or is 0)
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (rank_work(nullptr, R, mid).bytes <= bytes) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct RankTileArgs {
  const double *x;       // [R][D]
  const double *centre;  // [D] or null
  long long R, D, d0, T, rows_per_chunk;  // the tile: coordinates d0 ... d0 + T - 1
  int tw_log2;           // workgroups of 1 << tw_log2 coordinates
};

// (1) Workgroup (x: 1 << tw_log2 coordinates of the tile, y: chunk of draws).  Lane (c, rl) reads the draws rl,
// rl + 256 / tw, ... of a block of 256 rows at coordinate c (the tw lanes of a draw read one contiguous row segment);
// then lane t writes key t of every column of the block.  NEG: the keys are those of -x (psis.cuh's leave-one-out ratios).
template <bool NEG>
__global__ __launch_bounds__(RANK_THREADS) void k_rank_keys(RankTileArgs a, unsigned long long *__restrict__ keys,
                                                            unsigned *__restrict__ nan) {
  __shared__ unsigned long long s_key[RANK_TILE * RANK_STRIDE];
  __shared__ unsigned s_nan[RANK_TILE];
  const int tid = threadIdx.x, tw = 1 << a.tw_log2, c = tid & (tw - 1), rl = tid >> a.tw_log2;
  const int rpi = RANK_THREADS >> a.tw_log2;
  const long long t = (long long)blockIdx.x * tw + c, d = a.d0 + t;  // column of the tile, coordinate
  const bool live = t < a.T;
  if (tid < RANK_TILE) s_nan[tid] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.y * a.rows_per_chunk;
  const long long r1 = r0 + a.rows_per_chunk < a.R ? r0 + a.rows_per_chunk : a.R;
  unsigned n_nan = 0;
  for (long long rb = r0; rb < r1; rb += RANK_THREADS) {
    if (live) {
      for (int j = 0; j < tw; ++j) {
        const int row = j * rpi + rl;
        if (rb + row < r1) {
          const double xv = a.x[(rb + row) * a.D + d];
          const double v = rank_value(NEG ? -xv : xv, a.centre, d);
          n_nan += v != v;  // (a NaN that the fold makes counts too)
          s_key[c * RANK_STRIDE + row] = rank_key(v);
        }
      }
    }
    __syncthreads();
    if (rb + tid < r1)
      for (int cc = 0; cc < tw; ++cc) {
        const long long tt = (long long)blockIdx.x * tw + cc;
        if (tt < a.T) keys[tt * a.R + rb + tid] = s_key[cc * RANK_STRIDE + tid];
      }
    __syncthreads();
  }
  if (n_nan) atomicAdd(&s_nan[c], n_nan);
  __syncthreads();
  if (tid < tw && live && s_nan[tid]) atomicAdd(&nan[t], s_nan[tid]);
}

// (2a) Workgroup (x: chunk, y: column): counts [column][chunk][digit] of the chunk's keys.  Integer LDS atomics.
__global__ __launch_bounds__(RANK_THREADS) void k_rank_count(const unsigned long long *__restrict__ keys,
                                                             unsigned *__restrict__ counts, long long R,
                                                             long long chunk, int shift) {
  __shared__ unsigned s_hist[RANK_BINS];
  const int tid = threadIdx.x;
  s_hist[tid] = 0;
  __syncthreads();
  const long long k0 = (long long)blockIdx.x * chunk, k1 = k0 + chunk < R ? k0 + chunk : R;
  const unsigned long long *col = keys + (long long)blockIdx.y * R;
  for (long long i = k0 + tid; i < k1; i += RANK_THREADS) atomicAdd(&s_hist[(int)((col[i] >> shift) & 255)], 1u);
  __syncthreads();
  counts[((long long)blockIdx.y * gridDim.x + blockIdx.x) * RANK_BINS + tid] = s_hist[tid];
}

// (2b) One workgroup per column, lane t owns digit t: the counts become, in place, the exclusive scan over
// (digit, chunk) -- where in the sorted column the chunk's first key of that digit goes.
__global__ __launch_bounds__(RANK_THREADS) void k_rank_scan(unsigned *__restrict__ counts, int chunks) {
  __shared__ unsigned s_scan[2][RANK_BINS];
  const int tid = threadIdx.x;
  unsigned *c = counts + (long long)blockIdx.x * chunks * RANK_BINS + tid;
  unsigned total = 0;
  for (int b = 0; b < chunks; ++b) total += c[(long long)b * RANK_BINS];
  int cur = 0;
  s_scan[0][tid] = total;
  __syncthreads();
  for (int off = 1; off < RANK_BINS; off <<= 1) {
    const unsigned v = s_scan[cur][tid] + (tid >= off ? s_scan[cur][tid - off] : 0u);
    s_scan[cur ^ 1][tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  unsigned run = s_scan[cur][tid] - total;
  for (int b = 0; b < chunks; ++b) {
    const unsigned n = c[(long long)b * RANK_BINS];
    c[(long long)b * RANK_BINS] = run;
    run += n;
  }
}

// (2c) Workgroup (x: chunk, y: column), stable.  A round takes RANK_ROUND keys in the order (sub-round j, lane): the
// lanes of a wave that hold the same digit find each other by 8 ballots; the first of them stores their number under
// (j, wave, digit); lane t then scans digit t over the 16 (j, wave) in order, on top of the digit's running offset;
// a key goes to that scanned value + the lanes of its digit before it in its wave.  Two counter arrays alternate, so
// that the next round's is cleared while this round's is scanned: two barriers a round.
__global__ __launch_bounds__(RANK_THREADS) void k_rank_scatter(const unsigned long long *__restrict__ src,
                                                               unsigned long long *__restrict__ dst,
                                                               const unsigned *__restrict__ offsets, long long R,
                                                               long long chunk, int shift) {
  __shared__ unsigned s_cnt[2][RANK_SUB * RANK_WAVES * RANK_STRIDE];
  __shared__ unsigned s_base[RANK_BINS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < RANK_SUB * RANK_WAVES * RANK_STRIDE; i += RANK_THREADS) s_cnt[0][i] = s_cnt[1][i] = 0;
  s_base[tid] = offsets[((long long)blockIdx.y * gridDim.x + blockIdx.x) * RANK_BINS + tid];
  __syncthreads();
  const long long k0 = (long long)blockIdx.x * chunk, k1 = k0 + chunk < R ? k0 + chunk : R;
  const unsigned long long *in = src + (long long)blockIdx.y * R;
  unsigned long long *out = dst + (long long)blockIdx.y * R;
  const unsigned long long below = (1ULL << lane) - 1ULL;
  int cur = 0;
  for (long long kb = k0; kb < k1; kb += RANK_ROUND, cur ^= 1) {
    unsigned long long key[RANK_SUB];
    int before[RANK_SUB];
#pragma unroll
    for (int j = 0; j < RANK_SUB; ++j) {
      const long long i = kb + (long long)j * RANK_THREADS + tid;
      const bool valid = i < k1;
      key[j] = valid ? in[i] : 0ULL;
      const int dg = (int)((key[j] >> shift) & 255);
      unsigned long long same = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1;
        const unsigned long long have = __ballot(valid && bit);
        same &= bit ? have : ~have;
      }
      before[j] = __popcll(same & below);
      if (valid && before[j] == 0) s_cnt[cur][(j * RANK_WAVES + wave) * RANK_STRIDE + dg] = (unsigned)__popcll(same);
    }
    __syncthreads();
    {
      unsigned run = s_base[tid];
#pragma unroll
      for (int jw = 0; jw < RANK_SUB * RANK_WAVES; ++jw) {
        const unsigned n = s_cnt[cur][jw * RANK_STRIDE + tid];
        s_cnt[cur][jw * RANK_STRIDE + tid] = run;
        run += n;
        s_cnt[cur ^ 1][jw * RANK_STRIDE + tid] = 0;
      }
      s_base[tid] = run;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RANK_SUB; ++j) {
      const long long i = kb + (long long)j * RANK_THREADS + tid;
      if (i < k1) {
        const int dg = (int)((key[j] >> shift) & 255);
        out[s_cnt[cur][(j * RANK_WAVES + wave) * RANK_STRIDE + dg] + (unsigned)before[j]] = key[j];
      }
    }
  }
}

// Phi^-1 by Wichura's algorithm AS 241 (PPND16; Appl. Statist. 37 (1988) 477-484), relative error near 1e-16: a
// rational function of 0.180625 - q^2 for |q| = |p - 1/2| <= 0.425, of sqrt(-log(min(p, 1 - p))) - 1.6 beyond.  The
// far-tail branch of the algorithm (sqrt(-log p) > 5, p < 1.4e-11) is left out: the argument (r - 3/8) / (R + 1/4) of
// a rank is never below 0.625 / 2^31 = 2.9e-10, where sqrt(-log p) = 4.69.
__host__ __device__ inline double rank_ndtri(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e3 * r + 3.3430575583588128105e4) * r + 6.7265770927008700853e4) * r +
                            4.5921953931549871457e4) * r + 1.3731693765509461125e4) * r + 1.9715909503065514427e3) * r +
                          1.3314166789178437745e2) * r + 3.3871328727963666080e0);
    const double den = (((((((5.2264952788528545610e3 * r + 2.8729085735721942674e4) * r + 3.9307895800092710610e4) * r +
                            2.1213794301586595867e4) * r + 5.3941960214247511077e3) * r + 6.8718700749205790830e2) * r +
                          4.2313330701600911252e1) * r + 1.0);
    return q * num / den;
  }
  const double r = sqrt(-log(q < 0.0 ? p : 0.5 - q)) - 1.6;
  const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                          1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
                        4.63033784615654529590e0) * r + 1.42343711074968357734e0);
  const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                          1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
                        2.05319162663775882187e0) * r + 1.0);
  const double z = num / den;
  return q < 0.0 ? -z : z;
}

// (3) Workgroup (x: 1 << tw_log2 coordinates of the tile, y: chunk of draws), lanes as in k_rank_keys.  lo = the
// sorted keys below the draw's, found by bisection; hi = those not above it, found from lo by doubling steps and a
// bisection of the last one (tie-free draws: one more load).
__global__ __launch_bounds__(RANK_THREADS) void k_rank_out(RankTileArgs a, const unsigned long long *__restrict__ sorted,
                                                           const unsigned *__restrict__ nan, int mode,
                                                           double *__restrict__ out) {
  const int tid = threadIdx.x, tw = 1 << a.tw_log2, c = tid & (tw - 1), rl = tid >> a.tw_log2;
  const int rpi = RANK_THREADS >> a.tw_log2;
  const long long t = (long long)blockIdx.x * tw + c, d = a.d0 + t;
  if (t >= a.T) return;
  const long long r0 = (long long)blockIdx.y * a.rows_per_chunk;
  const long long r1 = r0 + a.rows_per_chunk < a.R ? r0 + a.rows_per_chunk : a.R;
  const bool poisoned = nan[t] != 0;
  const unsigned long long *col = sorted + t * a.R;
  const double denom = (double)a.R + 0.25;
  for (long long row = r0 + rl; row < r1; row += rpi) {
    double res = __longlong_as_double(0x7ff8000000000000LL);
    if (!poisoned) {
      const unsigned long long key = rank_key(rank_value(a.x[row * a.D + d], a.centre, d));
      long long lo = 0, n = a.R;  // lower bound: the first sorted key that is not below `key`
      while (n > 0) {
        const long long half = n >> 1;
        if (col[lo + half] < key) {
          lo += half + 1;
          n -= half + 1;
        } else {
          n = half;
        }
      }
      // col[lo] == key (the draw is in its column).  Upper bound: hi in (good, bad], col[good] == key < col[bad]
      long long good = lo, step = 1, bad = a.R;
      while (good + step < a.R) {
        if (col[good + step] == key) {
          good += step;
          step <<= 1;
        } else {
          bad = good + step;
          break;
        }
      }
      while (bad - good > 1) {
        const long long mid = good + ((bad - good) >> 1);
        if (col[mid] == key) good = mid; else bad = mid;
      }
      res = (double)(lo + bad + 1) * 0.5;
      if (mode == 1) res = rank_ndtri((res - 0.375) / denom);
    }
    out[row * a.D + d] = res;
  }
}

// the launch geometry of a tile's row kernels (1) and (3)
struct RankTileGeom {
  RankTileArgs a;
  long long subs, rc;  // workgroups across the tile's coordinates, chunks of rows
};
inline RankTileGeom rank_tile_geom(const double *x, const double *centre, long long R, long long D, long long d0,
                                   long long Tc) {
  RankTileGeom g;
  int twl = 4;  // workgroups of 16 coordinates, or of the power of two that holds the tile
  while (twl > 0 && (1LL << (twl - 1)) >= Tc) --twl;
  const int tw = 1 << twl;
  g.subs = (Tc + tw - 1) / tw;
  // about 2048 workgroups in all, each at least one block of 256 rows
  long long rc = (2048 + g.subs - 1) / g.subs;
  const long long most = (R + RANK_THREADS - 1) / RANK_THREADS;
  if (rc > most) rc = most;
  if (rc > 65535) rc = 65535;
  long long rows_per_chunk = (R + rc - 1) / rc;
  rows_per_chunk = (rows_per_chunk + RANK_THREADS - 1) / RANK_THREADS * RANK_THREADS;
  g.rc = (R + rows_per_chunk - 1) / rows_per_chunk;
  g.a.x = x; g.a.centre = centre; g.a.R = R; g.a.D = D; g.a.d0 = d0; g.a.T = Tc; g.a.rows_per_chunk = rows_per_chunk;
  g.a.tw_log2 = twl;
  return g;
}

// Steps (1) and (2) for the tile of `g`: afterwards w.keys[RANK_PASSES & 1] (the first buffer) holds the tile's sorted
// key columns [Tc][R] and w.nan its NaN counts; w.counts and the second key buffer are free again.  Shared by
// launch_rank, posterior.cuh and psis.cuh (neg: the columns of -x).
inline hipError_t launch_rank_sort(const RankTileGeom &g, const RankWork &w, hipStream_t st, bool neg = false) {
  const long long R = g.a.R, Tc = g.a.T;
  const long long chunk = rank_chunk(R), chunks = rank_chunks(R);
  if (hipError_t e = hipMemsetAsync(w.nan, 0, (size_t)Tc * sizeof(unsigned), st); e != hipSuccess) return e;
  if (neg)
    hipLaunchKernelGGL(k_rank_keys<true>, dim3((unsigned)g.subs, (unsigned)g.rc), dim3(RANK_THREADS), 0, st, g.a,
                       w.keys[0], w.nan);
  else
    hipLaunchKernelGGL(k_rank_keys<false>, dim3((unsigned)g.subs, (unsigned)g.rc), dim3(RANK_THREADS), 0, st, g.a,
                       w.keys[0], w.nan);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const dim3 grid((unsigned)chunks, (unsigned)Tc);
  for (int p = 0; p < RANK_PASSES; ++p) {
    const unsigned long long *src = w.keys[p & 1];
    unsigned long long *dst = w.keys[(p & 1) ^ 1];
    hipLaunchKernelGGL(k_rank_count, grid, dim3(RANK_THREADS), 0, st, src, w.counts, R, chunk, 8 * p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rank_scan, dim3((unsigned)Tc), dim3(RANK_THREADS), 0, st, w.counts, (int)chunks);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rank_scatter, grid, dim3(RANK_THREADS), 0, st, src, dst, (const unsigned *)w.counts, R,
                       chunk, 8 * p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

// out [R][D] from x [R][D]: tiles of T coordinates, T >= 1 what `w` (laid out by rank_work(base, R, T)) holds
inline hipError_t launch_rank(const double *x, const double *centre, long long R, long long D, int mode, double *out,
                              void *work, long long T, hipStream_t st) {
  const RankWork w = rank_work(work, R, T);
  for (long long d0 = 0; d0 < D; d0 += T) {
    const RankTileGeom g = rank_tile_geom(x, centre, R, D, d0, D - d0 < T ? D - d0 : T);
    if (hipError_t e = launch_rank_sort(g, w, st); e != hipSuccess) return e;
    // (an even number of passes: the sorted columns are back in the first buffer)
    hipLaunchKernelGGL(k_rank_out, dim3((unsigned)g.subs, (unsigned)g.rc), dim3(RANK_THREADS), 0, st, g.a,
                       (const unsigned long long *)w.keys[RANK_PASSES & 1], (const unsigned *)w.nan, mode, out);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace aehmc
