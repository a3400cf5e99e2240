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

// ---- streaming autocovariance: lagged products over a ring of the last K - 1 draws (aehmc_summary_lag_update) ----
// A split chain's draws are shifted by its first draw a (y_t = x_t - a: products of shifted draws survive an offset
// that raw products would not).  State between calls, all of it the caller's: shift [C][D] (a), sums [C][D]
// (Y = sum of y_t, ascending t), ring [K - 1][C][D] (y of segment position p in slot p mod (K - 1)), head [K - 1][C][D]
// (y of the first K - 1 positions) and prod [G][K][D]: R(k) = sum_t y_t y_{t-k}, summed over the chains of group g.
constexpr int SUMMARY_LAG_DB = 16;                                // coordinates per workgroup
constexpr int SUMMARY_LAG_LPB = SUMMARY_THREADS / SUMMARY_LAG_DB;  // lag lanes per coordinate
constexpr int SUMMARY_LAG_TB = 4;                                 // draws a lane multiplies per pass over its rows
constexpr int SUMMARY_LAG_CG_MAX = 4;                             // chains per group, a power of two
constexpr int SUMMARY_LAG_SHORT_CG = 4, SUMMARY_LAG_LONG_CG = 2;  // ... of the two variants below
constexpr int SUMMARY_LAG_SHORT = 3, SUMMARY_LAG_SHORT_TILE = 32;  // K <= 48: 3 lags per lane, tiles of 32 draws
constexpr int SUMMARY_LAG_LONG = 9, SUMMARY_LAG_LONG_TILE = 16;    // above: 9 lags per lane, tiles of 16 draws
constexpr long long SUMMARY_LAG_SHORT_K = (long long)SUMMARY_LAG_LPB * SUMMARY_LAG_SHORT;

struct SummaryLagArgs {
  const double *x;  // the chunk [.][C][D]
  double *shift, *sums, *ring, *head, *prod;
  long long C, D, K;
  long long ta, T;          // rows [ta, ta + T) of the chunk belong to the segment ...
  long long p0;             // ... as its positions p0, p0 + 1, ...
  long long base0, base1;   // p0 mod (K - 1), (p0 + T) mod (K - 1)
  int CG;                   // chains per group
};

// doubles of LDS per row of CG chains x 16 coordinates: a lag lane is LB (odd) rows from the next, and 16 doubles of
// padding put the two lag lanes of a 32-lane group of ds_read_b64 on different halves of the 64 banks
__host__ __device__ inline int summary_lag_row(int CG) {
  const int W = CG * SUMMARY_LAG_DB;
  return W % 32 == 0 ? W + 16 : W;
}
template <int LB, int TT> inline size_t summary_lag_lds(int CG, long long K) {
  const int KP = SUMMARY_LAG_LPB * LB;
  return ((size_t)(TT + KP - 1 + (K > KP ? TT : 0)) * summary_lag_row(CG) + CG * SUMMARY_LAG_DB) * sizeof(double);
}

// The fold.  Workgroup (x: block of 16 coordinates, y: group g of CG consecutive chains).  Per tile of TT draws it
// stages in LDS, shifted on load, the rows the lags of this pass reach back to (from the ring where they precede the
// chunk, zeros before the segment) and the tile itself.  Lane (lag lane kl, coordinate j) owns LB consecutive lags and
// takes SUMMARY_LAG_TB consecutive draws at a time: TB + (TB + LB - 1) LDS reads serve TB * LB FMAs, per chain.  For
// every draw the products of the group's chains are summed first, in chain order from zero, and that sum is added to the
// lane's accumulator: the additions into an accumulator are one per draw in ascending t whatever the chunking and the
// tiling, which is what keeps a chunk boundary invisible.  A pass covers 16 * LB lags; more lags, more passes.
template <int LB, int TT>
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_lag_fold(SummaryLagArgs a) {
  extern __shared__ double s_lag[];
  constexpr int DB = SUMMARY_LAG_DB, TB = SUMMARY_LAG_TB, KP = SUMMARY_LAG_LPB * LB, PR = TT + KP - 1;
  static_assert(TT % TB == 0 && LB % 2 == 1, "tile and lag blocking");
  const int CG = a.CG, W = CG * DB, wsh = __ffs(W) - 1, RS = summary_lag_row(CG);
  const int tid = threadIdx.x, j = tid & (DB - 1), kl = tid / DB;
  const long long D = a.D, E = a.C * D, K = a.K, Km1 = K - 1, T = a.T;
  const long long d0 = (long long)blockIdx.x * DB, c0 = (long long)blockIdx.y * CG;
  const int ncg = (int)((a.C - c0) < CG ? (a.C - c0) : CG);
  const bool fresh = a.p0 == 0, multi = K > KP;
  double *s_past = s_lag, *s_sep = s_lag + PR * RS, *s_a = s_lag + (PR + (multi ? TT : 0)) * RS;
  const double *xs = a.x + a.ta * E;

  // the (chain, coordinate) this thread stages: the same for every row it touches (256 is a multiple of W)
  const int e = tid & (W - 1), ecc = e / DB;
  const bool eok = ecc < ncg && d0 + (e & (DB - 1)) < D;
  const long long eoff = eok ? (c0 + ecc) * D + d0 + (e & (DB - 1)) : 0;
  double ysum = 0.0;
  if (tid < W) {
    s_a[tid] = eok ? (fresh ? xs[eoff] : a.shift[eoff]) : 0.0;
    if (eok && !fresh) ysum = a.sums[eoff];
  }
  __syncthreads();
  const double ea = s_a[e];
  const bool dlive = d0 + j < D;

  for (long long kp = 0; kp < K; kp += KP) {
    const long long kb = kp + (long long)kl * LB;
    const bool active = kb < K;
    double acc[LB];
#pragma unroll
    for (int i = 0; i < LB; ++i)
      acc[i] = (!fresh && dlive && kb + i < K) ? a.prod[((long long)blockIdx.y * K + kb + i) * D + d0 + j] : 0.0;
    const double *s_cur = kp == 0 ? s_past + (KP - 1) * RS : s_sep;
    for (long long tl = 0; tl < T; tl += TT) {
      const int nt = (int)((T - tl) < TT ? (T - tl) : TT);
      __syncthreads();
      for (int r = tid >> wsh; r < PR; r += SUMMARY_THREADS >> wsh) {
        const long long rel = tl - kp - (KP - 1) + r;  // chunk row of the segment's part; negative: before the chunk
        double v = 0.0;
        if (eok && a.p0 + rel >= 0 && rel < T) {
          if (rel >= 0) {
            v = xs[rel * E + eoff] - ea;
          } else if (-rel <= Km1) {
            long long sl = a.base0 + rel;
            if (sl < 0) sl += Km1;
            v = a.ring[sl * E + eoff];
          }
        }
        s_past[r * RS + e] = v;
      }
      if (kp > 0)
        for (int r = tid >> wsh; r < TT; r += SUMMARY_THREADS >> wsh)
          s_sep[r * RS + e] = (eok && tl + r < T) ? xs[(tl + r) * E + eoff] - ea : 0.0;
      __syncthreads();
      if (kp == 0 && tid < W)
        for (int t = 0; t < nt; ++t) ysum += s_cur[t * RS + tid];
      if (!active) continue;
      for (int tt0 = 0; tt0 < nt; tt0 += TB) {
        double s[TB][LB];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
          for (int i = 0; i < LB; ++i) s[tb][i] = 0.0;
        const double *pw = s_past + (tt0 + KP - kl * LB - LB) * RS + j;
        const double *pc = s_cur + tt0 * RS + j;
        for (int cc = 0; cc < ncg; ++cc) {
          double w[TB + LB - 1], y[TB];
#pragma unroll
          for (int q = 0; q < TB + LB - 1; ++q) w[q] = pw[q * RS + cc * DB];
#pragma unroll
          for (int tb = 0; tb < TB; ++tb) y[tb] = pc[tb * RS + cc * DB];
#pragma unroll
          for (int tb = 0; tb < TB; ++tb)
#pragma unroll
            for (int i = 0; i < LB; ++i) s[tb][i] = fma(y[tb], w[tb + LB - 1 - i], s[tb][i]);
        }
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
          if (tt0 + tb < nt) {
#pragma unroll
            for (int i = 0; i < LB; ++i) acc[i] += s[tb][i];
          }
      }
    }
    if (active && dlive) {
#pragma unroll
      for (int i = 0; i < LB; ++i)
        if (kb + i < K) a.prod[((long long)blockIdx.y * K + kb + i) * D + d0 + j] = acc[i];
    }
  }

  // carry: the last min(T, K - 1) shifted draws into their ring slots, the segment's first K - 1 into the head.  Every
  // read of the ring lies before the last barrier above, and no other workgroup touches these chains and coordinates.
  if (!eok) return;
  const long long nring = T < Km1 ? T : Km1;
  for (long long q = 1 + (tid >> wsh); q <= nring; q += SUMMARY_THREADS >> wsh) {
    long long sl = a.base1 - q;
    if (sl < 0) sl += Km1;
    a.ring[sl * E + eoff] = xs[(T - q) * E + eoff] - ea;
  }
  const long long hend = (a.p0 + T) < Km1 ? (a.p0 + T) : Km1;
  for (long long p = a.p0 + (tid >> wsh); p < hend; p += SUMMARY_THREADS >> wsh)
    a.head[p * E + eoff] = xs[(p - a.p0) * E + eoff] - ea;
  if (tid < W) {
    a.sums[eoff] = ysum;
    if (fresh) a.shift[eoff] = ea;
  }
}

struct SummaryLagEndArgs {
  const double *sums, *ring, *head;
  double *prod, *acov;
  long long C, D, K, G, n, basen;  // n: segment length, basen = n mod (K - 1)
  int CG, first, last;             // first / last segment of the run
  double m;                        // number of split chains
};

// The segment finaliser, at a segment's last draw.  With ybar = Y / n and first_k / last_k the sums of the chain's first
// and last k shifted draws (running sums over the head and the ring): n acov(k) = R(k) - ybar (2 Y - first_k - last_k)
// + (n - k) ybar^2.  Thread (group g, coordinate d) adds the corrections of its chains, in chain order, to prod[g].
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_lag_center(SummaryLagEndArgs a) {
  const long long i = (long long)blockIdx.x * SUMMARY_THREADS + threadIdx.x;
  if (i >= a.G * a.D) return;
  const long long g = i / a.D, d = i % a.D, D = a.D, E = a.C * D, Km1 = a.K - 1, c0 = g * a.CG;
  const int ncg = (int)((a.C - c0) < a.CG ? (a.C - c0) : a.CG);
  const double dn = (double)a.n;
  double Y[SUMMARY_LAG_CG_MAX], yb[SUMMARY_LAG_CG_MAX], F[SUMMARY_LAG_CG_MAX], L[SUMMARY_LAG_CG_MAX];
#pragma unroll
  for (int c = 0; c < SUMMARY_LAG_CG_MAX; ++c) {
    Y[c] = c < ncg ? a.sums[(c0 + c) * D + d] : 0.0;
    yb[c] = Y[c] / dn;
    F[c] = L[c] = 0.0;
  }
  for (long long k = 0; k < a.K; ++k) {
    long long sl = a.basen - k;
    if (sl < 0) sl += Km1;
    double corr = 0.0;
#pragma unroll
    for (int c = 0; c < SUMMARY_LAG_CG_MAX; ++c) {
      if (c >= ncg) continue;
      if (k > 0) {
        F[c] += a.head[(k - 1) * E + (c0 + c) * D + d];
        L[c] += a.ring[sl * E + (c0 + c) * D + d];
      }
      corr += (dn - (double)k) * yb[c] * yb[c] - yb[c] * (2.0 * Y[c] - F[c] - L[c]);
    }
    a.prod[(g * a.K + k) * D + d] += corr;
  }
}

// acov[k][d] (+)= (sum over the groups, ascending) / n; after the run's last segment, / (number of split chains)
__global__ __launch_bounds__(SUMMARY_THREADS) void k_summary_lag_reduce(SummaryLagEndArgs a) {
  const long long i = (long long)blockIdx.x * SUMMARY_THREADS + threadIdx.x, KD = a.K * a.D;
  if (i >= KD) return;
  double sum = 0.0;
  for (long long g = 0; g < a.G; ++g) sum += a.prod[g * KD + i];
  double v = sum / (double)a.n;
  if (!a.first) v = a.acov[i] + v;
  a.acov[i] = a.last ? v / a.m : v;
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

template <int LB, int TT>
inline hipError_t launch_summary_lag_fold(const SummaryLagArgs &a, long long G, hipStream_t st) {
  static bool lds_opt_in_dev[64] = {};  // once per device and instantiation: the most this kernel asks for
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  bool unset = false, &lds_opt_in = (dev >= 0 && dev < 64) ? lds_opt_in_dev[dev] : unset;
  if (!lds_opt_in) {
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_summary_lag_fold<LB, TT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)summary_lag_lds<LB, TT>(LB == SUMMARY_LAG_SHORT ? SUMMARY_LAG_SHORT_CG : SUMMARY_LAG_LONG_CG,
                                                                         LB == SUMMARY_LAG_SHORT ? 2 : 1 << 20));
        e != hipSuccess)
      return e;
    lds_opt_in = true;
  }
  const size_t dyn = summary_lag_lds<LB, TT>(a.CG, a.K);
  hipLaunchKernelGGL((k_summary_lag_fold<LB, TT>),
                     dim3((unsigned)((a.D + SUMMARY_LAG_DB - 1) / SUMMARY_LAG_DB), (unsigned)G), dim3(SUMMARY_THREADS),
                     dyn, st, a);
  return hipGetLastError();
}

// chains per group at K lags: what the fold's LDS holds (aehmc_summary_lag_group tells the caller, who sizes `work`)
inline int summary_lag_group(long long K) { return K <= SUMMARY_LAG_SHORT_K ? SUMMARY_LAG_SHORT_CG : SUMMARY_LAG_LONG_CG; }

// Draws t0 ... t0 + T - 1 of a run of N: the part of every segment the chunk holds is folded, and a segment whose last
// draw it holds is centred and reduced into acov (complete once the run's last draw has been folded).
inline hipError_t launch_summary_lag_update(const double *x, long long T, long long C, long long D, long long t0,
                                            long long N, int S, long long K, int CG, double *shift, double *sums,
                                            double *ring, double *head, double *prod, double *acov, hipStream_t st) {
  const long long h = N / 2, n = S == 2 ? h : N, Km1 = K - 1, G = (C + CG - 1) / CG;
  for (int seg = 0; seg < S; ++seg) {
    const long long slo = seg == 0 ? 0 : N - h, shi = (S == 1) ? N : (seg == 0 ? h : N);
    const long long lo = t0 > slo ? t0 : slo, hi = (t0 + T) < shi ? (t0 + T) : shi;
    if (lo >= hi) continue;
    SummaryLagArgs a;
    a.x = x; a.shift = shift; a.sums = sums; a.ring = ring; a.head = head; a.prod = prod;
    a.C = C; a.D = D; a.K = K; a.CG = CG;
    a.ta = lo - t0; a.T = hi - lo; a.p0 = lo - slo;
    a.base0 = a.p0 % Km1; a.base1 = (a.p0 + a.T) % Km1;
    if (hipError_t e = K <= SUMMARY_LAG_SHORT_K
                           ? launch_summary_lag_fold<SUMMARY_LAG_SHORT, SUMMARY_LAG_SHORT_TILE>(a, G, st)
                           : launch_summary_lag_fold<SUMMARY_LAG_LONG, SUMMARY_LAG_LONG_TILE>(a, G, st);
        e != hipSuccess)
      return e;
    if (hi < shi) continue;
    SummaryLagEndArgs f;
    f.sums = sums; f.ring = ring; f.head = head; f.prod = prod; f.acov = acov;
    f.C = C; f.D = D; f.K = K; f.G = G; f.n = n; f.basen = n % Km1;
    f.CG = CG; f.first = seg == 0; f.last = seg == S - 1; f.m = (double)(S * C);
    hipLaunchKernelGGL(k_summary_lag_center, dim3((unsigned)((G * D + SUMMARY_THREADS - 1) / SUMMARY_THREADS)),
                       dim3(SUMMARY_THREADS), 0, st, f);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_summary_lag_reduce, dim3((unsigned)((K * D + SUMMARY_THREADS - 1) / SUMMARY_THREADS)),
                       dim3(SUMMARY_THREADS), 0, st, f);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace aehmc
