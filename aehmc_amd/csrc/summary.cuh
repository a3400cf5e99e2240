// Posterior summaries of the stored or streamed draws (aehmc_summary_update / _autocov / _final):
// per-chain running moments, the chain-averaged autocovariance and the cross-chain statistics (split R-hat, ESS, MCSE).
// Everything is fp64 and deterministic: no floating-point atomics, every sum runs in an order that depends on the
// shapes alone, so two runs on the same input -- and any chunking of the same draws -- give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {

constexpr int SUMMARY_THREADS = 256;
constexpr int SUMMARY_TILE = 256;      // draws per table of reciprocal counts
constexpr int SUMMARY_INFLIGHT = 8;    // loads a lane issues before it folds the first of them
constexpr int SUMMARY_ACOV_LAGS = 4;   // lags a lane carries per pass over its centred series
constexpr long long SUMMARY_ACOV_MAX_ROWS = 8192;  // (segment length + lags) of one coordinate: 64 KiB of LDS

// Welford in ascending t for the draws [ta, tb) of a chunk x[T][E] (E = C * D elements, d fastest: a wavefront's load
// is one contiguous 512 B line of one draw).  The draw at ta is the k0-th of its segment.  The only dependence is
// through t, so SUMMARY_INFLIGHT draws are loaded before the first is folded.  The reciprocal of the count is the same
// for every element of a draw: the workgroup forms a table of them, one division per draw and workgroup instead of one
// per element.  (mean, m2) start as zeros: the first draw then gives mean = x, m2 = 0 by the same arithmetic as every
// other, which is what makes a chunk boundary invisible.
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_update(const double *__restrict__ x, long long E,
                                                                    long long ta, long long tb, long long k0,
                                                                    double *__restrict__ mean, double *__restrict__ m2) {
  __shared__ double inv[SUMMARY_TILE];
  const long long e = (long long)blockIdx.x * SUMMARY_THREADS + threadIdx.x;
  const bool live = e < E;
  double mu = 0.0, s = 0.0;
  if (live) {
    mu = mean[e];
    s = m2[e];
  }
  for (long long tile = ta; tile < tb; tile += SUMMARY_TILE) {
    const int nt = (int)((tb - tile) < SUMMARY_TILE ? (tb - tile) : SUMMARY_TILE);
    __syncthreads();
    if ((int)threadIdx.x < nt) inv[threadIdx.x] = 1.0 / (double)(k0 + (tile - ta) + threadIdx.x);
    __syncthreads();
    if (live) {
      const double *p = x + tile * E + e;
      int i = 0;
      for (; i + SUMMARY_INFLIGHT <= nt; i += SUMMARY_INFLIGHT) {
        double v[SUMMARY_INFLIGHT];
#pragma unroll
        for (int j = 0; j < SUMMARY_INFLIGHT; ++j) v[j] = p[(long long)(i + j) * E];
#pragma unroll
        for (int j = 0; j < SUMMARY_INFLIGHT; ++j) {
          const double dl = v[j] - mu;
          mu += dl * inv[i + j];
          s += dl * (v[j] - mu);
        }
      }
      for (; i < nt; ++i) {
        const double v = p[(long long)i * E];
        const double dl = v - mu;
        mu += dl * inv[i];
        s += dl * (v - mu);
      }
    }
  }
  if (live) {
    mean[e] = mu;
    m2[e] = s;
  }
}

struct SummaryAcovArgs {
  const double *x;     // [N][C][D]
  const double *mean;  // [S][C][D]
  double *partial;     // [G][K][D]
  long long N, C, D, n, K, rows;  // n: segment length, rows = n + K
  int S, DB, G;                   // DB coordinates per workgroup (a power of two <= 8)
};

// Biased autocovariance of every split chain about its own mean.  Workgroup (x: block of DB coordinates, y: group g)
// takes the split chains g, g + G, ... in ascending order.  For each it holds the centred series of its coordinates in
// LDS as rows [t][DB], followed by K rows of zeros, so that a lane may run its lags over one common range of t: the
// products past the end of the series are +-0 and leave the sum as it is.  Lane (lag, coordinate) sums in ascending t and
// carries SUMMARY_ACOV_LAGS lags at once (one read of x_t serves them all).  Consecutive lanes read consecutive LDS
// words: no bank conflicts.  The group's partial sum lives in partial[g]: the same lane writes and re-reads an element,
// so the order over chains is fixed and nothing is shared between workgroups.
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_acov(SummaryAcovArgs a) {
  extern __shared__ double s_series[];
  const int DB = a.DB, LPB = SUMMARY_THREADS / DB;
  const int sh = __ffs(DB) - 1, tid = threadIdx.x, j = tid & (DB - 1), kl = tid >> sh;
  const long long d0 = (long long)blockIdx.x * DB, d = d0 + j;
  const int g = blockIdx.y;
  const long long m = (long long)a.S * a.C, n = a.n, K = a.K;
  const double dn = (double)n;
  bool first = true;
  for (long long mi = g; mi < m; mi += a.G) {
    const long long seg = mi / a.C, c = mi % a.C;
    const long long tstart = seg == 0 ? 0 : a.N - n;
    __syncthreads();
    for (int idx = tid; idx < (int)a.rows * DB; idx += SUMMARY_THREADS) {  // (rows * DB <= 8192; DB a power of two)
      const long long t = idx >> sh, dd = d0 + (idx & (DB - 1));
      double v = 0.0;
      if (t < n && dd < a.D) v = a.x[((tstart + t) * a.C + c) * a.D + dd] - a.mean[(seg * a.C + c) * a.D + dd];
      s_series[idx] = v;
    }
    __syncthreads();
    for (long long kb = kl; kb < K; kb += (long long)SUMMARY_ACOV_LAGS * LPB) {
      long long k[SUMMARY_ACOV_LAGS];
      bool ok[SUMMARY_ACOV_LAGS];
      double acc[SUMMARY_ACOV_LAGS];
#pragma unroll
      for (int i = 0; i < SUMMARY_ACOV_LAGS; ++i) {
        k[i] = kb + (long long)i * LPB;
        ok[i] = k[i] < K;
        if (!ok[i]) k[i] = kb;  // (computed, not stored)
        acc[i] = 0.0;
      }
      const long long tend = n - kb;  // the shortest lag of the four decides; longer ones run into the zero rows
      for (long long t = 0; t < tend; ++t) {
        const double xt = s_series[t * DB + j];
#pragma unroll
        for (int i = 0; i < SUMMARY_ACOV_LAGS; ++i) acc[i] += xt * s_series[(t + k[i]) * DB + j];
      }
      if (d < a.D) {
#pragma unroll
        for (int i = 0; i < SUMMARY_ACOV_LAGS; ++i) {
          if (!ok[i]) continue;
          double *out = a.partial + ((long long)g * K + k[i]) * a.D + d;
          const double val = acc[i] / dn;
          *out = first ? val : *out + val;
        }
      }
    }
    first = false;
  }
}

// acov[k][d] = (sum over the groups, ascending) / (number of split chains)
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_acov_reduce(const double *__restrict__ partial, int G,
                                                                         long long KD, double m,
                                                                         double *__restrict__ acov) {
  const long long i = (long long)blockIdx.x * SUMMARY_THREADS + threadIdx.x;
  if (i >= KD) return;
  double sum = 0.0;
  for (int g = 0; g < G; ++g) sum += partial[(long long)g * KD + i];
  acov[i] = sum / m;
}

struct SummaryFinalArgs {
  const double *mean, *m2;  // [S * C][D]
  const double *acov;       // [K][D] or null
  double *out;              // [7][D]: mean, sd, rhat, ess, mcse, ess_chains, mcse_chains
  int *lag_truncated;       // [D] (with acov)
  long long n, m, D, K;     // n: segment length, m = S * C split chains
  int DX;                   // coordinates per workgroup: 64, or the power of two that holds D
};

// sum over the workgroup's chain slices in a fixed tree; every lane returns the total of its coordinate
__device__ inline double summary_tree(double *red, double v, int tid, int DX) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int h = SUMMARY_THREADS / DX / 2; h >= 1; h >>= 1) {
    if (tid / DX < h) red[tid] += red[tid + h * DX];
    __syncthreads();
  }
  return red[tid % DX];
}

// Cross-chain statistics of DX coordinates per workgroup.  Lane (dx, cy) reads rows cy, cy + CY, ... of the [m][D]
// moments, coalesced in d; the CY = 256 / DX slices of a coordinate meet in LDS.  With D = 2 and 4096 chains a
// coordinate is summed by 128 lanes instead of one.  The variance of the chain means takes a second pass about their
// mean.  Lane cy = 0 then walks the coordinate's autocorrelations (Geyer's initial positive, initial monotone sequence
// of pair sums) on its own.
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_final(SummaryFinalArgs a) {
  __shared__ double red[SUMMARY_THREADS];
  const int DX = a.DX, CY = SUMMARY_THREADS / DX, tid = threadIdx.x, dx = tid % DX, cy = tid / DX;
  const long long d = (long long)blockIdx.x * DX + dx, D = a.D, m = a.m, n = a.n;
  const bool live = d < D;
  double sm = 0.0, sv = 0.0;
  if (live)
    for (long long i = cy; i < m; i += CY) {
      sm += a.mean[i * D + d];
      sv += a.m2[i * D + d];
    }
  const double dm = (double)m, dn = (double)n;
  const double gm = summary_tree(red, sm, tid, DX) / dm;
  const double W = summary_tree(red, sv, tid, DX) / (dn - 1.0) / dm;
  double sb = 0.0;
  if (live)
    for (long long i = cy; i < m; i += CY) {
      const double dl = a.mean[i * D + d] - gm;
      sb += dl * dl;
    }
  const double sbt = summary_tree(red, sb, tid, DX);
  if (!live || cy != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double Bn = m > 1 ? sbt / (dm - 1.0) : 0.0;  // B / n: variance of the chain means
  const double varp = W * (dn - 1.0) / dn + Bn;
  const double sd = sqrt(varp);
  double rhat = nan, ess = nan, mcse = 0.0, essc = nan, mcsec = m > 1 ? sqrt(Bn / dm) : nan;
  int trunc = 0;
  if (varp > 0.0) {
    rhat = sqrt(varp / W);
    if (m > 1) essc = varp / (Bn / dm);
    if (a.acov) {
      const long long K = a.K;  // >= 2 (aehmc_summary_final)
      // pair sums P_j = rho_2j + rho_2j+1, rho_0 = 1; P_0 always counts
      double prev = 1.0 + (1.0 - (W - a.acov[D + d]) / varp);
      double sum = prev, extra = 0.0;
      for (long long k = 2;; k += 2) {
        if (k + 1 >= K) {  // the sequence was still positive when the lags ran out
          trunc = 1;
          break;
        }
        const double re = 1.0 - (W - a.acov[k * D + d]) / varp;
        const double ro = 1.0 - (W - a.acov[(k + 1) * D + d]) / varp;
        double P = re + ro;
        if (!(P > 0.0)) {
          if (re > 0.0) extra = re;
          break;
        }
        if (P > prev) P = prev;
        sum += P;
        prev = P;
      }
      double tau = -1.0 + 2.0 * sum + extra;
      const double floor_tau = 1.0 / log10(dm * dn);
      if (!(tau >= floor_tau)) tau = floor_tau;
      ess = dm * dn / tau;
      mcse = sd / sqrt(ess);
    }
  }
  a.out[d] = gm;
  a.out[D + d] = sd;
  a.out[2 * D + d] = rhat;
  a.out[5 * D + d] = essc;
  a.out[6 * D + d] = mcsec;
  if (a.acov) {
    a.out[3 * D + d] = ess;
    a.out[4 * D + d] = mcse;
    a.lag_truncated[d] = trunc;
  }
}

// ---- launches (tu_summary.hip) ----
inline hipError_t launch_summary_update(const double *x, long long T, long long E, long long t0, long long N, int S,
                                        double *mean, double *m2, hipStream_t st) {
  const long long h = N / 2;
  for (int seg = 0; seg < S; ++seg) {
    const long long slo = seg == 0 ? 0 : N - h, shi = (S == 1) ? N : (seg == 0 ? h : N);
    const long long lo = t0 > slo ? t0 : slo, hi = (t0 + T) < shi ? (t0 + T) : shi;
    if (lo >= hi) continue;
    hipLaunchKernelGGL(k_summary_update, dim3((unsigned)((E + SUMMARY_THREADS - 1) / SUMMARY_THREADS)),
                       dim3(SUMMARY_THREADS), 0, st, x, E, lo - t0, hi - t0, lo - slo + 1, mean + seg * E, m2 + seg * E);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

inline hipError_t launch_summary_acov(const double *x, const double *mean, double *partial, double *acov, long long N,
                                      long long C, long long D, int S, long long K, int G, hipStream_t st) {
  SummaryAcovArgs a;
  a.x = x; a.mean = mean; a.partial = partial;
  a.N = N; a.C = C; a.D = D; a.S = S; a.K = K; a.G = G;
  a.n = S == 2 ? N / 2 : N;
  a.rows = a.n + K;
  int DB = 8;
  while (DB > 1 && (a.rows * DB > SUMMARY_ACOV_MAX_ROWS || DB / 2 >= D)) DB /= 2;
  a.DB = DB;
  const size_t dyn = (size_t)a.rows * DB * sizeof(double);
  static bool lds_opt_in = false;  // once per process: up to 64 KiB of dynamic LDS
  if (!lds_opt_in) {
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_summary_acov),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(SUMMARY_ACOV_MAX_ROWS * sizeof(double))); e != hipSuccess)
      return e;
    lds_opt_in = true;
  }
  hipLaunchKernelGGL(k_summary_acov, dim3((unsigned)((D + DB - 1) / DB), (unsigned)G), dim3(SUMMARY_THREADS), dyn, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const long long KD = K * D;
  hipLaunchKernelGGL(k_summary_acov_reduce, dim3((unsigned)((KD + SUMMARY_THREADS - 1) / SUMMARY_THREADS)),
                     dim3(SUMMARY_THREADS), 0, st, (const double *)partial, G, KD, (double)(S * C), acov);
  return hipGetLastError();
}

inline hipError_t launch_summary_final(const double *mean, const double *m2, const double *acov, double *out,
                                       int *lag_truncated, long long n, long long m, long long D, long long K,
                                       hipStream_t st) {
  SummaryFinalArgs a;
  a.mean = mean; a.m2 = m2; a.acov = acov; a.out = out; a.lag_truncated = lag_truncated;
  a.n = n; a.m = m; a.D = D; a.K = K;
  int DX = 64;
  while (DX > 1 && DX / 2 >= D) DX /= 2;
  a.DX = DX;
  hipLaunchKernelGGL(k_summary_final, dim3((unsigned)((D + DX - 1) / DX)), dim3(SUMMARY_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
