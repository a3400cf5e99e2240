// Nested R-hat for many short chains (aehmc_nested_update): C = K M chains in K superchains of M
// consecutive chains, the draws cut into windows of w; per window and coordinate the spread of the superchain means
// against the spread inside superchains.  Two kernels per chunk at most, whatever its length and however many windows end
// in it: k_nested_window closes every window whose last draw the chunk holds, k_nested_fold carries the chains' running
// moments of the window that stays open.  fp64, no floating-point atomics, and every sum runs in an order that
// (C, D, K, M, w) alone decide: two runs on the same draws -- and any chunking of them -- give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {

constexpr int NESTED_THREADS = 256;
constexpr int NESTED_TAB = 256;     // reciprocal counts 1 / 1 ... 1 / 256 a workgroup tabulates
constexpr int NESTED_INFLIGHT = 8;  // loads a lane issues before it folds the first of them
constexpr int NESTED_CHAINS = 8;    // chains a lane walks side by side (NESTED_INFLIGHT / NESTED_CHAINS draws of each)
constexpr int NESTED_DX = 16;       // coordinates per workgroup at most: a 128-byte line of a draw per chain
constexpr int NESTED_OUT = 5;       // rows of a window: nested_rhat, between, within, mean, mcse_superchains

// 1 / k as every Welford step of this file uses it, whichever kernel and whichever table it comes from: one IEEE
// division of 1.0 by the count
__device__ inline double nested_rcp(long long k) { return 1.0 / (double)k; }
__device__ inline double nested_rcp(const double *tab, long long k) { return k <= NESTED_TAB ? tab[k - 1] : nested_rcp(k); }

// The Welford step, shared by both kernels: a window that one kernel begins and the other ends is folded by the same
// arithmetic draw for draw.  From (0, 0) the first value gives (v, 0), so a fresh window needs no special case.
__device__ inline void nested_welford(double v, double inv, double &mu, double &s) {
  const double dl = v - mu;
  mu += dl * inv;
  s += dl * (v - mu);
}

// Welford in ascending t over the chunk's draws [ta, tb) of the open window, for every element e of [C][D]; the draw at
// ta is the (k0 + 1)-th of its window.  k0 = 0: the window begins here and (mean, m2) are not read.  The shape of
// k_summary_update: the reciprocal counts of a tile of draws sit in LDS, NESTED_INFLIGHT draws are loaded before the
// first is folded.
__global__ __launch_bounds__(NESTED_THREADS) void k_nested_fold(const double *__restrict__ x, long long E, long long ta,
                                                                long long tb, long long k0, double *__restrict__ mean,
                                                                double *__restrict__ m2) {
  __shared__ double inv[NESTED_TAB];
  const long long e = (long long)blockIdx.x * NESTED_THREADS + threadIdx.x;
  const bool live = e < E;
  double mu = 0.0, s = 0.0;
  if (live && k0 > 0) {
    mu = mean[e];
    s = m2[e];
  }
  for (long long tile = ta; tile < tb; tile += NESTED_TAB) {
    const int nt = (int)((tb - tile) < NESTED_TAB ? (tb - tile) : NESTED_TAB);
    __syncthreads();
    if ((int)threadIdx.x < nt) inv[threadIdx.x] = nested_rcp(k0 + (tile - ta) + threadIdx.x + 1);
    __syncthreads();
    if (live) {
      const double *p = x + tile * E + e;
      int i = 0;
      for (; i + NESTED_INFLIGHT <= nt; i += NESTED_INFLIGHT) {
        double v[NESTED_INFLIGHT];
#pragma unroll
        for (int j = 0; j < NESTED_INFLIGHT; ++j) v[j] = p[(long long)(i + j) * E];
#pragma unroll
        for (int j = 0; j < NESTED_INFLIGHT; ++j) nested_welford(v[j], inv[i + j], mu, s);
      }
      for (; i < nt; ++i) nested_welford(p[(long long)i * E], inv[i], mu, s);
    }
  }
  if (live) {
    mean[e] = mu;
    m2[e] = s;
  }
}

struct NestedArgs {
  const double *x;          // the chunk [T][C][D]
  const double *mean, *m2;  // [C][D]: the moments of the window that was open when the chunk began (k0 > 0)
  double *out;              // [.][NESTED_OUT][D], at the first window that ends in this chunk
  long long C, D, K, M, w;  // K superchains of M chains, windows of w draws
  long long k0;             // draws of the first window that earlier chunks hold
  long long nblk;           // blocks of DX coordinates
  int DX;                   // coordinates per workgroup: NESTED_DX, or the power of two that holds D
};

// NC consecutive chains of one superchain, side by side: Welford over the rows [0, nt) at p (E doubles apart; the chains
// D doubles apart), the first of them the (k0 + 1)-th draw of the window.  NC * TU loads are in flight.
template <int NC, int TU>
__device__ inline void nested_walk(const double *p, long long E, long long D, long long nt, long long k0,
                                   const double *tab, double (&mu)[NC], double (&s)[NC]) {
  long long i = 0;
  for (; i + TU <= nt; i += TU) {
    double v[TU][NC];
#pragma unroll
    for (int r = 0; r < TU; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) v[r][c] = p[(i + r) * E + c * D];
#pragma unroll
    for (int r = 0; r < TU; ++r) {
      const double inv = nested_rcp(tab, k0 + i + r + 1);
#pragma unroll
      for (int c = 0; c < NC; ++c) nested_welford(v[r][c], inv, mu[c], s[c]);
    }
  }
  for (; i < nt; ++i) {
    const double inv = nested_rcp(tab, k0 + i + 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) nested_welford(p[i * E + c * D], inv, mu[c], s[c]);
  }
}

// One window that ends in this chunk and DX coordinates per workgroup (blockIdx.x = window * nblk + block).  Lane
// (dx, cy) of the CY = 256 / DX lanes of a coordinate owns the superchains cy, cy + CY, ... and walks each whole:
//   per chain, Welford over the window's draws in ascending t (the first window from the carried moments): a_c, s2_c;
//   over the chains of the superchain in ascending c, Welford over the a_c: abar_k and Btilde_k, and the sum of the s2_c;
//   over its superchains in ascending k, Welford over the abar_k and the sum of Btilde_k + Wtilde_k.
// The lanes of a coordinate then meet in LDS in a fixed tree, by the pairwise (Chan) combination, since they may hold
// unequal counts (none at all where K < CY); a side that holds nothing leaves the other as it is.  A wavefront's load is
// four 128-byte lines of a draw (DX = 16), one per superchain: narrow blocks, so that a chunk of three draws at 10^4
// coordinates still makes 1875 workgroups with 8 loads in flight per lane.  No value of one coordinate ever meets
// another's.
__global__ __launch_bounds__(NESTED_THREADS) void k_nested_window(NestedArgs a) {
  __shared__ double tab[NESTED_TAB];
  __shared__ double r_n[NESTED_THREADS], r_m[NESTED_THREADS], r_b[NESTED_THREADS], r_w[NESTED_THREADS];
  const int DX = a.DX, CY = NESTED_THREADS / DX, tid = threadIdx.x, dx = tid % DX, cy = tid / DX;
  const long long wi = blockIdx.x / a.nblk, blk = blockIdx.x % a.nblk;
  const long long D = a.D, E = a.C * D, M = a.M, K = a.K, w = a.w;
  const long long d = blk * DX + dx;
  const bool live = d < D;
  // rows of the chunk that belong to the window, and how many of its draws precede them
  const long long k0 = wi == 0 ? a.k0 : 0;
  const long long ra = wi == 0 ? 0 : (w - a.k0) + (wi - 1) * w;
  const long long nt = w - k0;
  tab[tid] = nested_rcp((long long)tid + 1);
  __syncthreads();

  double cnt = 0.0, gm = 0.0, gb = 0.0, wsum = 0.0;
  if (live) {
    const double dM = (double)M, dw1 = (double)(w - 1);
    long long seen = 0;
    for (long long k = cy; k < K; k += CY) {
      double am = 0.0, ab = 0.0, ws = 0.0;
      long long j = 0;
      const long long e0 = k * M * D + d;
      const double *p0 = a.x + ra * E + e0;
      for (; j + NESTED_CHAINS <= M; j += NESTED_CHAINS) {
        double mu[NESTED_CHAINS], s[NESTED_CHAINS];
#pragma unroll
        for (int c = 0; c < NESTED_CHAINS; ++c) {
          mu[c] = k0 > 0 ? a.mean[e0 + (j + c) * D] : 0.0;
          s[c] = k0 > 0 ? a.m2[e0 + (j + c) * D] : 0.0;
        }
        nested_walk<NESTED_CHAINS, NESTED_INFLIGHT / NESTED_CHAINS>(p0 + j * D, E, D, nt, k0, tab, mu, s);
#pragma unroll
        for (int c = 0; c < NESTED_CHAINS; ++c) {
          if (w > 1) ws += s[c] / dw1;
          nested_welford(mu[c], nested_rcp(tab, j + c + 1), am, ab);
        }
      }
      for (; j < M; ++j) {
        double mu[1] = {k0 > 0 ? a.mean[e0 + j * D] : 0.0}, s[1] = {k0 > 0 ? a.m2[e0 + j * D] : 0.0};
        nested_walk<1, NESTED_INFLIGHT>(p0 + j * D, E, D, nt, k0, tab, mu, s);
        if (w > 1) ws += s[0] / dw1;
        nested_welford(mu[0], nested_rcp(tab, j + 1), am, ab);
      }
      double q = ws / dM;                  // Wtilde_k
      if (M > 1) q += ab / (dM - 1.0);     // + Btilde_k
      wsum += q;
      ++seen;
      nested_welford(am, nested_rcp(tab, seen), gm, gb);
    }
    cnt = (double)seen;
  }

  r_n[tid] = cnt;
  r_m[tid] = gm;
  r_b[tid] = gb;
  r_w[tid] = wsum;
  __syncthreads();
  for (int h = CY / 2; h >= 1; h >>= 1) {
    if (cy < h) {
      const int o = tid + h * DX;
      const double na = r_n[tid], nb = r_n[o];
      if (nb > 0.0) {
        if (na > 0.0) {
          const double n = na + nb, dl = r_m[o] - r_m[tid];
          r_m[tid] += dl * (nb / n);
          r_b[tid] = r_b[tid] + r_b[o] + dl * dl * (na * nb / n);
          r_n[tid] = n;
        } else {
          r_n[tid] = nb;
          r_m[tid] = r_m[o];
          r_b[tid] = r_b[o];
        }
        r_w[tid] += r_w[o];
      }
    }
    __syncthreads();
  }
  if (!live || cy != 0) return;
  const double dK = (double)K;
  const double B = r_b[tid] / (dK - 1.0), W = r_w[tid] / dK;
  // IEEE division does the conventions: W = B = 0 -> NaN, W = 0 < B -> +inf, B = 0 < W -> exactly 1
  double *out = a.out + wi * NESTED_OUT * D + d;
  out[0] = sqrt(1.0 + B / W);
  out[D] = B;
  out[2 * D] = W;
  out[3 * D] = r_m[tid];
  out[4 * D] = sqrt(B / dK);
}

// ---- launch (tu_nested.hip) ----
// Draws t0 ... t0 + T - 1 of a run cut into windows of w.  At most two launches: the windows whose last draw the chunk
// holds, then the chains' moments of the window it leaves open (continued where no window ended, begun afresh behind
// the last that did; the window kernel has read the carried moments by then: one stream).
inline long long nested_blocks(long long D, int *DX_out) {
  int DX = NESTED_DX;
  while (DX > 1 && DX / 2 >= D) DX /= 2;
  if (DX_out) *DX_out = DX;
  return (D + DX - 1) / DX;
}
inline hipError_t launch_nested_update(const double *x, long long T, long long C, long long D, long long t0, long long w,
                                       long long M, double *mean, double *m2, double *out, hipStream_t st) {
  const long long E = C * D, k0 = t0 % w, first = t0 / w, nwin = (t0 + T) / w - first, rem = (t0 + T) % w;
  if (nwin > 0) {
    NestedArgs a;
    a.x = x; a.mean = mean; a.m2 = m2; a.out = out + first * NESTED_OUT * D;
    a.C = C; a.D = D; a.K = C / M; a.M = M; a.w = w; a.k0 = k0;
    a.nblk = nested_blocks(D, &a.DX);
    hipLaunchKernelGGL(k_nested_window, dim3((unsigned)(nwin * a.nblk)), dim3(NESTED_THREADS), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (rem > 0) {
    const long long ta = nwin > 0 ? T - rem : 0;
    hipLaunchKernelGGL(k_nested_fold, dim3((unsigned)((E + NESTED_THREADS - 1) / NESTED_THREADS)), dim3(NESTED_THREADS),
                       0, st, x, E, ta, T, nwin > 0 ? 0LL : k0, mean, m2);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace aehmc
