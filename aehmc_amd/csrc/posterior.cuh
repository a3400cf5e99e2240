// Highest-density intervals and the Monte-Carlo standard error of quantiles of the stored draws (aehmc_summary_hdi,
// aehmc_summary_quantile_mcse, aehmc_beta_quantile).  Both read values at positions of the sorted pooled
// draws that differ from coordinate to coordinate, which the radix select of quantile.cuh (one host list of ranks for
// all coordinates) cannot give: they are consumers of the sorted key columns [T][R] that steps (1) and (2) of rank.cuh
// leave in a tile's scratch (launch_rank_sort), decoded by rank_unkey.  -0.0 and +0.0 come back as +0.0; a coordinate
// with a NaN answers NaN.  The kernels belong to rank.cuh's translation unit (tu_rank.hip) for that reason.
//
//  HDI.  With s_0 <= ... <= s_{R-1} a column and m = min(floor(prob R), R - 1): the windows w_i = s_{i+m} - s_i,
//      i = 0 ... R - m - 1 (a NaN width, inf - inf, counts as +inf), i* the smallest i of minimal width, lower = s_{i*},
//      upper = s_{i*+m}: ArviZ's unimodal hdi with m clamped.  k_hdi_windows: workgroup (x: chunk of the sort's chunk
//      grid, y: column) streams col[i] and col[i + m] (consecutive lanes, consecutive keys) and reduces (width, index)
//      pairs under the total order "smaller width, then smaller index" -- shuffles in the wave, LDS across waves -- to
//      one partial per chunk, kept in the tile's `counts` scratch (free after the sort; 16 of its 1024 bytes per
//      chunk).  k_hdi_final: one wave per column reduces the partials and reads the two end points.  The order is total
//      and min over it is associative and commutative: no atomics, and the result depends on neither the chunking, the
//      tile nor the run.
//  Beta quantile.  beta_ppf(p, a, b), a, b >= 1, 0 < p < 1: the x with I_x(a, b) = p, in fp64.  I_x by the continued
//      fraction (modified Lentz) on the side of the mean where it converges, I_x(a, b) = 1 - I_{1-x}(b, a) on the other;
//      its prefactor x^a (1 - x)^b / B(a, b) from lgamma while a or b is below 10, and above that from Stirling's series
//      written in differences (see beta_log_prefactor: lgamma's own rounding, half an ulp of 1.5e8 at a + b = 1e7,
//      would be 1e-8 of I_x and 1e-11 of x).  The root by Halley steps from the normal approximation, kept inside a
//      bracket by bisection; iterations of both loops are bounded.
//  Quantile MCSE (posterior::mcse_quantile, ArviZ's _mcse_quantile).  One lane per (probability q, coordinate d):
//      e = ess[q][d], a1 = beta_ppf(0.1586553, e p + 1, e (1 - p) + 1), a2 = beta_ppf(0.8413447, ...),
//      lo = max(floor(a1 R), 1) - 1, hi = min(ceil(a2 R), R) - 1, mcse = (s_hi - s_lo) / 2.  The cost is the sort.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "rank.cuh"

namespace aehmc {

constexpr int POSTERIOR_MAX_PROBS = 64;        // AEHMC_SUMMARY_QUANTILE_MAX
constexpr int BETA_CF_ITERS = 1 << 15;         // the fraction needs O(sqrt(max(a, b))) terms: 3e3 at 1e7
constexpr int BETA_PPF_ITERS = 64;
constexpr double BETA_STIRLING_MIN = 10.0;     // Stirling's series in differences from here on (see below)
constexpr long long HDI_NONE = 0x7fffffffffffffffLL;

struct HdiPartial {
  double w;
  long long i;
};
struct PosteriorProbs {
  double p[POSTERIOR_MAX_PROBS];
};

__host__ __device__ inline double posterior_nan() {
  const unsigned long long b = 0x7ff8000000000000ULL;
  double v;
  memcpy(&v, &b, sizeof v);
  return v;
}

// ---- the regularised incomplete beta function and its inverse ----

// Stirling's correction lgamma(z) - ((z - 1/2) log z - z + log(2 pi) / 2), z >= 10: the next term is 2e-14 there
__host__ __device__ inline double beta_stirling_corr(double z) {
  const double r = 1.0 / z, r2 = r * r;
  return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0 - r2 * (1.0 / 1188.0)))));
}

// log of x^a (1 - x)^b / B(a, b).  From lgamma while a or b is small.  For a, b >= 10, with n = a + b and
// t = x n - a (one rounding: fma), Stirling's series gives
//   a log1p(t / a) + b log1p(-t / b) + log(a b / n) / 2 - log(2 pi) / 2 - (corr(a) + corr(b) - corr(n)),
// in which nothing of size n log n is left to cancel: near the mean the two log1p terms are of size sqrt(n) each.
__host__ __device__ inline double beta_log_prefactor(double x, double a, double b) {
  const double n = a + b;
  if (a < BETA_STIRLING_MIN || b < BETA_STIRLING_MIN)
    return a * log(x) + b * log1p(-x) + (lgamma(n) - lgamma(a) - lgamma(b));
  const double t = fma(x, n, -a);
  const double ua = fmax(t / a, -1.0), ub = fmax(-t / b, -1.0);
  return a * log1p(ua) + b * log1p(ub) + 0.5 * log(a * b / n) - 0.91893853320467274178 -
         (beta_stirling_corr(a) + beta_stirling_corr(b) - beta_stirling_corr(n));
}

// the continued fraction of I_x(a, b) a / (x^a (1 - x)^b / B(a, b)) by the modified Lentz method; converges for
// x < (a + 1) / (a + b + 2)
__host__ __device__ inline double beta_cf(double x, double a, double b) {
  const double tiny = 1e-300, eps = 1.2e-16;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= BETA_CF_ITERS; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= eps) break;
  }
  return h;
}

// I_x(a, b), 0 < x < 1, and its derivative in x (the beta density)
__host__ __device__ inline double beta_inc(double x, double a, double b, double *pdf) {
  const double y = 1.0 - x, pref = exp(beta_log_prefactor(x, a, b));
  *pdf = pref / (x * y);
  if (x < (a + 1.0) / (a + b + 2.0)) return pref * beta_cf(x, a, b) / a;
  return 1.0 - pref * beta_cf(y, b, a) / b;
}

// the x in (0, 1) with I_x(a, b) = p; NaN unless 0 < p < 1 and 1 <= a, b < inf
__host__ __device__ inline double beta_ppf(double p, double a, double b) {
  if (!(p > 0.0 && p < 1.0 && a >= 1.0 && b >= 1.0 && a < INFINITY && b < INFINITY)) return posterior_nan();
  const double n = a + b, mu = a / n, sd = sqrt(a * b / (n * n * (n + 1.0)));
  double lo = 0.0, hi = 1.0;  // I(lo) < p < I(hi)
  double x = mu + rank_ndtri(fmin(fmax(p, 1e-10), 1.0 - 1e-10)) * sd;
  if (!(x > lo && x < hi)) x = mu;
  for (int it = 0; it < BETA_PPF_ITERS; ++it) {
    double pdf;
    const double f = beta_inc(x, a, b, &pdf) - p;
    if (f == 0.0) break;
    if (f < 0.0) lo = x; else hi = x;
    // Halley's step, its correction of Newton's held within [2/3, 2]; converged when it no longer moves x, and
    // bisection where it leaves the bracket (x itself is an end of it)
    const double u = f / pdf, g = (a - 1.0) / x - (b - 1.0) / (1.0 - x);
    double xn = x - u / (1.0 - 0.5 * fmin(1.0, fmax(-1.0, u * g)));
    if (fabs(xn - x) <= 4.4e-16 * x) break;
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    if (xn == x) break;
    x = xn;
  }
  return x;
}

__global__ void k_beta_quantile(long long n, const double *__restrict__ p, const double *__restrict__ a,
                                const double *__restrict__ b, double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = beta_ppf(p[i], a[i], b[i]);
}

inline hipError_t launch_beta_quantile(long long n, const double *p, const double *a, const double *b, double *out,
                                       hipStream_t st) {
  hipLaunchKernelGGL(k_beta_quantile, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, p, a, b, out);
  return hipGetLastError();
}

// ---- the highest-density interval ----

// the total order of the reduction: the narrower window, and of two equally narrow ones the first
__device__ inline void hdi_take(double &w, long long &i, double w2, long long i2) {
  if (w2 < w || (w2 == w && i2 < i)) {
    w = w2;
    i = i2;
  }
}
__device__ inline void hdi_wave_min(double &w, long long &i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double w2 = __shfl_xor(w, off);
    const long long i2 = __shfl_xor(i, off);
    hdi_take(w, i, w2, i2);
  }
}

// Workgroup (x: chunk, y: column of the tile): the best window that starts in the chunk, (+inf, HDI_NONE) if none does
__global__ __launch_bounds__(RANK_THREADS) void k_hdi_windows(const unsigned long long *__restrict__ sorted,
                                                              HdiPartial *__restrict__ partial, long long R,
                                                              long long m, long long chunk) {
  __shared__ double s_w[RANK_WAVES];
  __shared__ long long s_i[RANK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long nwin = R - m;
  const long long k0 = (long long)blockIdx.x * chunk, k1 = k0 + chunk < nwin ? k0 + chunk : nwin;
  const unsigned long long *col = sorted + (long long)blockIdx.y * R;
  double w = INFINITY;
  long long i = HDI_NONE;
  for (long long k = k0 + tid; k < k1; k += RANK_THREADS) {
    double wk = rank_unkey(col[k + m]) - rank_unkey(col[k]);
    if (wk != wk) wk = INFINITY;
    hdi_take(w, i, wk, k);
  }
  hdi_wave_min(w, i);
  if (lane == 0) {
    s_w[wave] = w;
    s_i[wave] = i;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < RANK_WAVES; ++v) hdi_take(w, i, s_w[v], s_i[v]);
    HdiPartial r;
    r.w = w;
    r.i = i;
    partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = r;
  }
}

// One wave per column of the tile: the best of its partials (chunk 0 always holds window 0), and the two end points
__global__ __launch_bounds__(64) void k_hdi_final(const unsigned long long *__restrict__ sorted,
                                                  const HdiPartial *__restrict__ partial,
                                                  const unsigned *__restrict__ nan, long long R, long long m,
                                                  int chunks, long long d0, double *__restrict__ lower,
                                                  double *__restrict__ upper, long long *__restrict__ index) {
  const int lane = threadIdx.x;
  const long long t = blockIdx.x;
  double w = INFINITY;
  long long i = HDI_NONE;
  for (int b = lane; b < chunks; b += 64) {
    const HdiPartial r = partial[t * chunks + b];
    hdi_take(w, i, r.w, r.i);
  }
  hdi_wave_min(w, i);
  if (lane != 0) return;
  const unsigned long long *col = sorted + t * R;
  const bool poisoned = nan[t] != 0 || i == HDI_NONE;
  lower[d0 + t] = poisoned ? posterior_nan() : rank_unkey(col[i]);
  upper[d0 + t] = poisoned ? posterior_nan() : rank_unkey(col[i + m]);
  if (index) index[d0 + t] = poisoned ? -1LL : i;
}

// lower, upper [D] (and index [D] unless null) from x [R][D], 0 <= m <= R - 1; tiles as in launch_rank
inline hipError_t launch_hdi(const double *x, long long R, long long D, long long m, double *lower, double *upper,
                             long long *index, void *work, long long T, hipStream_t st) {
  const RankWork w = rank_work(work, R, T);
  const long long chunk = rank_chunk(R), chunks = rank_chunks(R);
  HdiPartial *partial = (HdiPartial *)w.counts;  // [T][chunks]
  const unsigned long long *sorted = w.keys[RANK_PASSES & 1];
  for (long long d0 = 0; d0 < D; d0 += T) {
    const long long Tc = D - d0 < T ? D - d0 : T;
    const RankTileGeom g = rank_tile_geom(x, nullptr, R, D, d0, Tc);
    if (hipError_t e = launch_rank_sort(g, w, st); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hdi_windows, dim3((unsigned)chunks, (unsigned)Tc), dim3(RANK_THREADS), 0, st, sorted, partial,
                       R, m, chunk);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hdi_final, dim3((unsigned)Tc), dim3(64), 0, st, sorted, (const HdiPartial *)partial,
                       (const unsigned *)w.nan, R, m, (int)chunks, d0, lower, upper, index);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- the Monte-Carlo standard error of a quantile ----

// Lane per (probability, column of the tile); out [Q][D], ranks [2][Q][D] or null
__global__ __launch_bounds__(64) void k_quantile_mcse(const unsigned long long *__restrict__ sorted,
                                                      const unsigned *__restrict__ nan, PosteriorProbs probs, int Q,
                                                      const double *__restrict__ ess, long long R, long long D,
                                                      long long d0, long long Tc, double *__restrict__ out,
                                                      long long *__restrict__ ranks) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (long long)Q * Tc) return;
  const long long q = j / Tc, t = j - q * Tc, at = q * D + d0 + t;
  const double e = ess[at], p = probs.p[q];
  double res = posterior_nan();
  long long lo = -1, hi = -1;
  if (e > 0.0 && e < INFINITY && nan[t] == 0) {
    const double a = e * p + 1.0, b = e * (1.0 - p) + 1.0, S = (double)R;
    const double a1 = beta_ppf(0.1586553, a, b), a2 = beta_ppf(0.8413447, a, b);
    lo = (long long)fmax(floor(a1 * S), 1.0) - 1;
    hi = (long long)fmin(ceil(a2 * S), S) - 1;
    if (hi < 0) hi = 0;  // (a2 > 0: never taken; keeps the read inside the column whatever beta_ppf answers)
    const unsigned long long *col = sorted + t * R;
    res = (rank_unkey(col[hi]) - rank_unkey(col[lo])) / 2.0;
  }
  out[at] = res;
  if (ranks) {
    ranks[at] = lo;
    ranks[(long long)Q * D + at] = hi;
  }
}

inline hipError_t launch_quantile_mcse(const double *x, long long R, long long D, int Q, const double *probs,
                                       const double *ess, double *out, long long *ranks, void *work, long long T,
                                       hipStream_t st) {
  const RankWork w = rank_work(work, R, T);
  PosteriorProbs pp;
  for (int q = 0; q < POSTERIOR_MAX_PROBS; ++q) pp.p[q] = q < Q ? probs[q] : 0.0;
  const unsigned long long *sorted = w.keys[RANK_PASSES & 1];
  for (long long d0 = 0; d0 < D; d0 += T) {
    const long long Tc = D - d0 < T ? D - d0 : T;
    const RankTileGeom g = rank_tile_geom(x, nullptr, R, D, d0, Tc);
    if (hipError_t e = launch_rank_sort(g, w, st); e != hipSuccess) return e;
    const long long lanes = (long long)Q * Tc;
    hipLaunchKernelGGL(k_quantile_mcse, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, sorted,
                       (const unsigned *)w.nan, pp, Q, ess, R, D, d0, Tc, out, ranks);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace aehmc
