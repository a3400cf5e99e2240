// Pareto-smoothed importance sampling of the stored draws (aehmc_summary_psis): per column of
// x [R][D] (log importance ratios) the smoothed, normalised log-weights, the Pareto shape k of the tail, and with
// v [R][D] the weighted expectation log sum_s exp(lw_s + v_s) -- PSIS-LOO when x = -v is the pointwise log-likelihood.
// Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling"; the generalised-Pareto fit is Zhang &
// Stephens' (2009) with the prior constants of ArviZ's _gpdfit.  A consumer of the sorted key columns [T][R] that
// launch_rank_sort leaves in a tile's scratch, like posterior.cuh; the second key buffer (free after the sort) holds a
// column's tail, the tile's `counts` scratch its scalars and partial sums.  Everything in fp64.
//
// Per column, with mx its largest value (a NaN, a non-finite mx, a reff that is not finite and > 0: everything NaN,
// tail_len -1), y = x - mx, s the sorted y:
//  k_psis_fit, one workgroup per column.  M = ceil(min(R / 5, 3 sqrt(R / reff))) held to [0, R - 1],
//      cut = max(s[R - M - 1], log(DBL_MIN)), the tail starts at the first place above cut (an upper-bound search among
//      the last M places; ties at the cutoff stay out), n = its length.  n <= 4: k = +inf, nothing is smoothed.
//      Otherwise t_j = exp(s_j) - exp(cut) goes to the second key buffer, and the fit runs on it: m = 30 + floor(sqrt n)
//      thetas b_i, a wave per theta and a lane per 64th tail element for k_i = mean_j log1p(-b_i t_j) (lane sums in
//      ascending j, a butterfly over the wave: a fixed shape), L_i = n (log(-b_i / k_i) - k_i - 1), then
//      w_i = 1 / sum_l exp(L_l - L_i) (a lane per i, l ascending), weights below 10 DBL_EPSILON dropped and b = sum w_i
//      b_i by one lane in ascending i, and k' = mean_j log1p(-b t_j) by the workgroup.  psis_fit_finish gives sigma and
//      k; a fit that fails (k not finite, sigma not > 0) reports k = NaN and smooths nothing.  L and w [m] live behind
//      the tail in the second key buffer (m reaches 403 at R = 2^31 and reff = 1, 20754 at a tiny reff), and in LDS
//      where a short column has no room for them: up to PSIS_LDS_THETA thetas.
//      Then place j of the tail gets min(log(sigma gpinv((j + 0.5) / n) + exp(cut)), 0), in place of t_j, and the first
//      place of every run of equal draws replaces the run's values by the log of the mean of their exp, summed in
//      ascending place: the weights are a function of the multiset of draws.
//  k_psis_lse, workgroup (x: chunk of the sort's chunk grid, y: column): the chunk's sum of exp over the sorted column,
//      smoothed places read from the tail; k_psis_norm: a lane per column adds the partials in chunk order, norm = log
//      of it, and writes pareto_k and tail_len.  Neither the row order nor the tile enters.
//  k_psis_out, workgroup (x: 16 columns, y: chunk of rows; the chunks a function of R alone): the rows are read again.
//      A draw at or below cut keeps y - norm; a tail draw searches the first place of its value in the tail and takes
//      what stands there.  log_weights is written if asked for.  With v, every lane keeps a running (max, sum) of
//      lw + v over its rows in order, the 16 lanes of a column are merged by a tree in LDS, and the pair of the row
//      chunk is stored; k_psis_final merges a column's pairs in chunk order: log_mean = max + log(sum).  The columns of
//      a workgroup are always 16 wide, whatever the tile, so that for given rows a column's terms meet in one order.
// No floating-point atomics; every output is the same bits on every run and for every tile width.  Under a permutation
// of the rows pareto_k, tail_len and every row's log-weight keep their bits (they come from the sorted column);
// log_mean is summed along the rows and is equal to rounding only.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "posterior.cuh"
#include "rank.cuh"

namespace aehmc {

constexpr double PSIS_LOG_TINY = -708.39641853226408;  // log(DBL_MIN)
constexpr int PSIS_LDS_THETA = 64;                     // thetas whose L and w are held in LDS
constexpr long long PSIS_MAX_ROW_CHUNKS = 1024;        // row chunks of the output pass, at most
constexpr int PSIS_COL_DOUBLES = 8;                    // a PsisCol in the counts scratch

// a column's scalars.  cut is +inf and smoothed 0 where the tail stays as it is; n = -1 and mx = NaN for a column
// that answers NaN
struct PsisCol {
  double mx, cut, k, sigma, norm;
  long long n, smoothed;
};
static_assert(sizeof(PsisCol) <= PSIS_COL_DOUBLES * sizeof(double), "PsisCol outgrew its place in the scratch");

// ---- the scalar pieces ----

// M, the draws that may belong to the tail
__host__ __device__ inline long long psis_tail_size(long long R, double reff) {
  const double M = ceil(fmin((double)R / 5.0, 3.0 * sqrt((double)R / reff)));
  return (long long)fmin(fmax(M, 0.0), (double)(R - 1));
}
__host__ __device__ inline int psis_thetas(long long n) { return 30 + (int)floor(sqrt((double)n)); }
// b_i, i = 1 ... m, from the tail's quartile t_q and its largest value t_n
__host__ __device__ inline double psis_theta(int i, int m, double tq, double tn) {
  return (1.0 - sqrt((double)m / ((double)i - 0.5))) / (3.0 * tq) + 1.0 / tn;
}
// the profile log-likelihood of b from k_b = mean_j log1p(-b t_j)
__host__ __device__ inline double psis_profile(long long n, double b, double kb) {
  return (double)n * (log(-b / kb) - kb - 1.0);
}
// the fit's last step: sigma and the k of the posterior mean b, shrunk towards 0.5 by ten pseudo-observations; false
// where the fit has failed
__host__ __device__ inline bool psis_fit_finish(long long n, double kb, double b, double *k, double *sigma) {
  *sigma = -kb / b;
  *k = ((double)n * kb + 5.0) / ((double)n + 10.0);
  return *k - *k == 0.0 && *sigma > 0.0;
}
// the quantile function of the generalised Pareto distribution of shape k and scale 1
__host__ __device__ inline double psis_gpinv(double p, double k) {
  const double l = log1p(-p);
  return fabs(k) < DBL_EPSILON ? -l : expm1(-k * l) / k;
}
// what place j of n takes the place of: the expected order statistic, on top of the cutoff, held to the largest ratio
__host__ __device__ inline double psis_smoothed(long long j, long long n, double k, double sigma, double ecut) {
  return fmin(log(sigma * psis_gpinv(((double)j + 0.5) / (double)n, k) + ecut), 0.0);
}

// a running log-sum-exp (m, s): the sum is s exp(m).  -inf terms count nothing, a NaN makes s NaN, a +inf makes m +inf
__device__ inline void psis_lse_add(double &m, double &s, double a) {
  if (a > m) {
    s = s * exp(m - a) + 1.0;
    m = a;
  } else if (a != -INFINITY) {
    s += a == m ? 1.0 : exp(a - m);
  }
}
__device__ inline void psis_lse_merge(double &m, double &s, double m2, double s2) {
  const double top = m2 > m ? m2 : m;
  if (top == -INFINITY) {
    s += s2;
    return;
  }
  s = s * (m == top ? 1.0 : exp(m - top)) + s2 * (m2 == top ? 1.0 : exp(m2 - top));
  m = top;
}

__device__ inline double psis_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// the sum over the workgroup of every lane's v, the same bits in every lane: butterflies in the waves, then the waves
// in order.  s_red [RANK_WAVES]; ends behind a barrier, and may be called again at once
__device__ inline double psis_block_sum(double v, double *s_red) {
  v = psis_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = s_red[0];
  for (int u = 1; u < RANK_WAVES; ++u) total += s_red[u];
  return total;
}

// where a tile's column keeps its doubles in the counts scratch: [chunks] partial sums of the normaliser, a PsisCol,
// [row chunks][2] partial (max, sum) of the weighted expectation
constexpr long long PSIS_CHUNK_DOUBLES = RANK_BINS * (long long)sizeof(unsigned) / (long long)sizeof(double);
template <class P>
__host__ __device__ inline P *psis_col_base(P *cols, long long t, long long chunks) {
  return cols + t * chunks * PSIS_CHUNK_DOUBLES;
}

// ---- the tail and its fit ----

__global__ __launch_bounds__(RANK_THREADS) void k_psis_fit(const unsigned long long *__restrict__ sorted,
                                                           double *__restrict__ aux_all,
                                                           const unsigned *__restrict__ nan,
                                                           const double *__restrict__ reff, long long R, long long d0,
                                                           long long chunks, double *__restrict__ cols) {
  __shared__ double s_L[PSIS_LDS_THETA], s_w[PSIS_LDS_THETA];
  __shared__ double s_red[RANK_WAVES];
  __shared__ double s_b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t = blockIdx.x;
  const unsigned long long *col = sorted + t * R;
  double *aux = aux_all + t * R;
  PsisCol *out = (PsisCol *)(psis_col_base(cols, t, chunks) + chunks);
  PsisCol pc;
  pc.mx = pc.k = pc.sigma = pc.norm = posterior_nan();
  pc.cut = INFINITY;
  pc.n = -1;
  pc.smoothed = 0;
  const double r = reff ? reff[d0 + t] : 1.0;
  const double mx = rank_unkey(col[R - 1]);
  // (everything up to the fit is the same in every lane: no lane leaves a barrier behind)
  if (nan[t] != 0 || !(mx - mx == 0.0) || !(r - r == 0.0) || !(r > 0.0)) {
    if (tid == 0) *out = pc;
    return;
  }
  pc.mx = mx;
  const long long M = psis_tail_size(R, r);
  double cut = rank_unkey(col[R - M - 1]) - mx;
  if (cut < PSIS_LOG_TINY) cut = PSIS_LOG_TINY;
  long long start = R - M, left = M;  // the first place whose value lies above the cutoff
  while (left > 0) {
    const long long half = left >> 1;
    if (rank_unkey(col[start + half]) - mx > cut) {
      left = half;
    } else {
      start += half + 1;
      left -= half + 1;
    }
  }
  const long long n = R - start;
  pc.n = n;
  pc.k = INFINITY;
  if (n <= 4) {
    if (tid == 0) *out = pc;
    return;
  }
  const double ecut = exp(cut);
  for (long long j = tid; j < n; j += RANK_THREADS) aux[j] = exp(rank_unkey(col[start + j]) - mx) - ecut;
  __syncthreads();
  const double tq = aux[(long long)floor((double)n / 4.0 + 0.5) - 1], tn = aux[n - 1], dn = (double)n;
  const int m = psis_thetas(n);
  // (m > PSIS_LDS_THETA = 64: n >= 35^2 and R >= 5 (n - 1), so the 2 m doubles behind the tail end before place R)
  double *L = m <= PSIS_LDS_THETA ? s_L : aux + n;
  double *w = m <= PSIS_LDS_THETA ? s_w : aux + n + m;
  for (int i = wave; i < m; i += RANK_WAVES) {
    const double b = psis_theta(i + 1, m, tq, tn);
    double acc = 0.0;
    for (long long j = lane; j < n; j += 64) acc += log1p(-b * aux[j]);
    acc = psis_wave_sum(acc);
    if (lane == 0) L[i] = psis_profile(n, b, acc / dn);
  }
  __syncthreads();
  for (int i = tid; i < m; i += RANK_THREADS) {
    const double Li = L[i];
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc += exp(L[l] - Li);
    w[i] = 1.0 / acc;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0, b = 0.0;
    for (int i = 0; i < m; ++i)
      if (w[i] >= 10.0 * DBL_EPSILON) total += w[i];
    for (int i = 0; i < m; ++i)
      if (w[i] >= 10.0 * DBL_EPSILON) b += psis_theta(i + 1, m, tq, tn) * (w[i] / total);
    s_b = b;
  }
  __syncthreads();
  const double b = s_b;
  double acc = 0.0;
  for (long long j = tid; j < n; j += RANK_THREADS) acc += log1p(-b * aux[j]);
  const double kb = psis_block_sum(acc, s_red) / dn;  // (its barriers: every t_j has been read)
  double k, sigma;
  if (!psis_fit_finish(n, kb, b, &k, &sigma)) {
    pc.k = posterior_nan();
    if (tid == 0) *out = pc;
    return;
  }
  pc.k = k;
  pc.sigma = sigma;
  pc.cut = cut;
  pc.smoothed = n;
  if (tid == 0) *out = pc;
  for (long long j = tid; j < n; j += RANK_THREADS) aux[j] = psis_smoothed(j, n, k, sigma, ecut);
  __syncthreads();
  // runs of equal draws: the lane of a run's first place reads and rewrites that run alone.  One lane walks a whole
  // run, so the pass is serial in the run's length, which is at most n <= M <= R / 5 + 1 (a tail of one value)
  for (long long j = tid; j < n; j += RANK_THREADS) {
    const double y = rank_unkey(col[start + j]) - mx;
    if (j > 0 && rank_unkey(col[start + j - 1]) - mx == y) continue;
    long long hi = j + 1;
    while (hi < n && rank_unkey(col[start + hi]) - mx == y) ++hi;
    if (hi - j < 2) continue;
    double sum = 0.0;
    for (long long q = j; q < hi; ++q) sum += exp(aux[q]);
    const double mean = log(sum / (double)(hi - j));
    for (long long q = j; q < hi; ++q) aux[q] = mean;
  }
}

// ---- the normaliser ----

// Workgroup (x: chunk, y: column): sum of exp over the chunk's places of the smoothed sorted column
__global__ __launch_bounds__(RANK_THREADS) void k_psis_lse(const unsigned long long *__restrict__ sorted,
                                                           const double *__restrict__ aux_all, long long R,
                                                           long long chunk, double *__restrict__ cols) {
  __shared__ double s_red[RANK_WAVES];
  const int tid = threadIdx.x;
  const long long t = blockIdx.y, chunks = gridDim.x;
  double *base = psis_col_base(cols, t, chunks);
  const PsisCol pc = *(const PsisCol *)(base + chunks);
  const unsigned long long *col = sorted + t * R;
  const double *aux = aux_all + t * R;
  const long long start = R - pc.smoothed;
  const long long k0 = (long long)blockIdx.x * chunk, k1 = k0 + chunk < R ? k0 + chunk : R;
  double acc = 0.0;
  for (long long p = k0 + tid; p < k1; p += RANK_THREADS)
    acc += exp(p < start ? rank_unkey(col[p]) - pc.mx : aux[p - start]);
  const double total = psis_block_sum(acc, s_red);
  if (tid == 0) base[blockIdx.x] = total;
}

// Lane per column of the tile: the partials in chunk order; pareto_k and tail_len (unless null) of the coordinate
__global__ __launch_bounds__(64) void k_psis_norm(double *__restrict__ cols, long long chunks, long long Tc, long long d0,
                                                  double *__restrict__ pareto_k, long long *__restrict__ tail_len) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Tc) return;
  double *base = psis_col_base(cols, t, chunks);
  PsisCol *pc = (PsisCol *)(base + chunks);
  double total = 0.0;
  for (long long b = 0; b < chunks; ++b) total += base[b];
  pc->norm = log(total);
  pareto_k[d0 + t] = pc->k;
  if (tail_len) tail_len[d0 + t] = pc->n;
}

// ---- the log-weights and the weighted expectation ----

struct PsisOutArgs {
  const double *x;  // [R][D]; the ratios are -x with neg
  const double *v;  // [R][D] or null
  double *lw;       // [R][D] or null
  long long R, D, d0, T, rows_per_chunk, chunks;
  int neg;
};

// Workgroup (x: RANK_TILE columns of the tile, y: chunk of rows).  Lane (c, rl) takes the rows rl, rl + 16, ... of the
// chunk at column c: the 16 lanes of a row read one contiguous segment.
__global__ __launch_bounds__(RANK_THREADS) void k_psis_out(PsisOutArgs a, const unsigned long long *__restrict__ sorted,
                                                           const double *__restrict__ aux_all,
                                                           double *__restrict__ cols) {
  __shared__ double s_m[RANK_THREADS], s_s[RANK_THREADS];
  const int tid = threadIdx.x, c = tid & (RANK_TILE - 1), rl = tid / RANK_TILE;
  constexpr int rpi = RANK_THREADS / RANK_TILE;
  const long long t = (long long)blockIdx.x * RANK_TILE + c, d = a.d0 + t;
  const bool live = t < a.T;
  double m = -INFINITY, s = 0.0;
  if (live) {
    double *base = psis_col_base(cols, t, a.chunks);
    const PsisCol pc = *(const PsisCol *)(base + a.chunks);
    const unsigned long long *col = sorted + t * a.R;
    const double *aux = aux_all + t * a.R;
    const long long start = a.R - pc.smoothed;
    const long long r0 = (long long)blockIdx.y * a.rows_per_chunk;
    const long long r1 = r0 + a.rows_per_chunk < a.R ? r0 + a.rows_per_chunk : a.R;
    for (long long row = r0 + rl; row < r1; row += rpi) {
      const double xv = a.x[row * a.D + d];
      const double y = (a.neg ? -xv : xv) - pc.mx;
      double lw = y;
      if (y > pc.cut) {
        // a tail draw (pc.smoothed > 0): the first place in [start, R) whose value is not below y
        long long lo = start, left = pc.smoothed;
        while (left > 0) {
          const long long half = left >> 1;
          if (rank_unkey(col[lo + half]) - pc.mx < y) {
            lo += half + 1;
            left -= half + 1;
          } else {
            left = half;
          }
        }
        if (lo > a.R - 1) lo = a.R - 1;  // (the draw is in its column: never taken; keeps the read inside the tail)
        lw = aux[lo - start];
      }
      lw -= pc.norm;
      if (a.lw) a.lw[row * a.D + d] = lw;
      if (a.v) psis_lse_add(m, s, lw + a.v[row * a.D + d]);
    }
  }
  if (!a.v) return;
  s_m[tid] = m;
  s_s[tid] = s;
  __syncthreads();
  for (int stride = RANK_THREADS / 2; stride >= RANK_TILE; stride >>= 1) {
    if (tid < stride) {
      psis_lse_merge(m, s, s_m[tid + stride], s_s[tid + stride]);
      s_m[tid] = m;
      s_s[tid] = s;
    }
    __syncthreads();
  }
  if (tid < RANK_TILE && live) {
    double *pair = psis_col_base(cols, t, a.chunks) + a.chunks + PSIS_COL_DOUBLES + 2 * (long long)blockIdx.y;
    pair[0] = m;
    pair[1] = s;
  }
}

// Lane per column of the tile: the row chunks' pairs in order
__global__ __launch_bounds__(64) void k_psis_final(const double *__restrict__ cols, long long chunks, long long rc,
                                                   long long Tc, long long d0, double *__restrict__ log_mean) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Tc) return;
  const double *pair = psis_col_base(cols, t, chunks) + chunks + PSIS_COL_DOUBLES;
  double m = -INFINITY, s = 0.0;
  for (long long b = 0; b < rc; ++b) psis_lse_merge(m, s, pair[2 * b], pair[2 * b + 1]);
  log_mean[d0 + t] = m + log(s);
}

// the row chunks of the output pass: a function of R alone, at most PSIS_MAX_ROW_CHUNKS of them, whole blocks of 256
inline long long psis_rows_per_chunk(long long R) {
  const long long per = (R + PSIS_MAX_ROW_CHUNKS - 1) / PSIS_MAX_ROW_CHUNKS;
  return (per + RANK_THREADS - 1) / RANK_THREADS * RANK_THREADS;
}

// pareto_k [D], tail_len [D] or null, log_weights [R][D] or null, log_mean [D] with v, from the ratios x [R][D] (neg:
// the ratios are -x); tiles as in launch_rank
inline hipError_t launch_psis(const double *x, bool neg, const double *reff, const double *v, double *log_weights,
                              double *pareto_k, long long *tail_len, double *log_mean, long long R, long long D,
                              void *work, long long T, hipStream_t st) {
  const RankWork w = rank_work(work, R, T);
  const long long chunk = rank_chunk(R), chunks = rank_chunks(R);
  const long long rows_per_chunk = psis_rows_per_chunk(R), rc = (R + rows_per_chunk - 1) / rows_per_chunk;
  // A column's doubles share the sort's counts scratch, 128 doubles per sort chunk, and have to fit it.  They do: a row
  // chunk holds at least 256 rows, so rc <= ceil(R / 256), and a sort chunk holds 4096 keys or more.  While it holds
  // 4096, ceil(R / 256) <= 16 chunks; a larger sort chunk means more than 512 chunks, and rc <= 1024.  So
  // rc <= 16 chunks either way and chunks + 8 + 2 rc <= 33 chunks + 8 <= 128 chunks.  Checked all the same:
  if (chunks + PSIS_COL_DOUBLES + 2 * rc > chunks * PSIS_CHUNK_DOUBLES) return hipErrorInvalidValue;
  const unsigned long long *sorted = w.keys[RANK_PASSES & 1];
  double *aux = (double *)w.keys[(RANK_PASSES & 1) ^ 1];
  double *cols = (double *)w.counts;
  for (long long d0 = 0; d0 < D; d0 += T) {
    const long long Tc = D - d0 < T ? D - d0 : T;
    const RankTileGeom g = rank_tile_geom(x, nullptr, R, D, d0, Tc);
    if (hipError_t e = launch_rank_sort(g, w, st, neg); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_psis_fit, dim3((unsigned)Tc), dim3(RANK_THREADS), 0, st, sorted, aux, (const unsigned *)w.nan,
                       reff, R, d0, chunks, cols);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_psis_lse, dim3((unsigned)chunks, (unsigned)Tc), dim3(RANK_THREADS), 0, st, sorted,
                       (const double *)aux, R, chunk, cols);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_psis_norm, dim3((unsigned)((Tc + 63) / 64)), dim3(64), 0, st, cols, chunks, Tc, d0, pareto_k,
                       tail_len);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (!log_weights && !v) continue;
    PsisOutArgs a;
    a.x = x; a.v = v; a.lw = log_weights; a.R = R; a.D = D; a.d0 = d0; a.T = Tc; a.rows_per_chunk = rows_per_chunk;
    a.chunks = chunks; a.neg = neg ? 1 : 0;
    hipLaunchKernelGGL(k_psis_out, dim3((unsigned)((Tc + RANK_TILE - 1) / RANK_TILE), (unsigned)rc), dim3(RANK_THREADS),
                       0, st, a, sorted, (const double *)aux, cols);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (v) {
      hipLaunchKernelGGL(k_psis_final, dim3((unsigned)((Tc + 63) / 64)), dim3(64), 0, st, (const double *)cols, chunks,
                         rc, Tc, d0, log_mean);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace aehmc
