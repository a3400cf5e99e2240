// Pooled window adaptation: ONE dual-averaging state, ONE Welford state and ONE step size / inverse mass matrix adapted
// from all chains together (window_adaptation.run(..., pooled=True); the per-chain kernels are in engine.cuh).
//
// One warm-up step, positions X [C, D] and acceptance probabilities a [C] after the transition:
//   abar = (sum_c a_c) / C                               -> adapt_da_update (engine.cuh), the per-chain arithmetic
//   slow stage, batch Welford (Chan) with b = (sum_c X_c) / C:
//     n' = n + C, d = b - mean, mean' = mean + d (C / n'),
//     m2' = m2 + sum_c (X_c - b)(X_c - b)^T + (n C / n') d d^T      (diagonal metric: its diagonal only)
//   window end: cov = m2 / (n - 1), imm = (n / (n + 5)) cov + 1e-3 (5 / (n + 5)) [diagonal only when dense],
//     sqrt_mass, Welford state zeroed, dual averaging restarted (adapt_da_restart)
//   after the last step the step size is exp(x_avg).
//
// Launches of one update, all on the caller's stream:
//   k_pool_colsum        partial column sums of X (and of a, as column D) over P contiguous parts of the chains
//   k_pool_mean          parts added in ascending order: b, d, mean'            (slow stage)
//   diagonal: k_pool_colsum<true> (squares about b, the one further pass over X) and k_pool_sq (m2', window end)
//   dense:    the symmetric rank-C update (syrk_f64.cuh), at a window end k_pool_imm and the factorisation (engine.hip)
//   k_pool_scalars       abar, dual averaging, sample count, the step size into all C entries of step_size
// Every sum runs in an order fixed by (C, D): P and the rows of a part come from pool_parts; no atomics.  The sample
// count is written by the last kernel only, so the others read the count the update started with.
#pragma once
#include "engine.cuh"

namespace aehmc {

struct PoolArgs {
  long long C, D;
  int stage, window_end, last;
  double target, gamma, t0, kappa;
  const double *p_accept, *position;
  aehmc_pooled_adapt_state s;
  int P;               // parts of the chain range
  long long rows_per;  // chains per part
  double *part;        // [P][D + 1] partial sums (column D: acceptance probability)
  double *b, *delta;   // [D] batch mean, b - mean
  double *sc;          // [1]: n C / n', the weight of the rank-one term
};

// parts of the chain range for the column sums: about 1024 workgroups over the 64-column blocks, at least 64 chains a part
inline void pool_parts(long long C, long long D, int &P, long long &rows_per) {
  const long long colblocks = (D + 1 + 63) / 64;
  long long want = (1024 + colblocks - 1) / colblocks;
  const long long most = (C + 63) / 64;
  if (want > most) want = most;
  if (want < 1) want = 1;
  rows_per = (C + want - 1) / want;
  P = (int)((C + rows_per - 1) / rows_per);
}
inline size_t pool_work_doubles(long long C, long long D) {
  int P;
  long long rows_per;
  pool_parts(C, D, P, rows_per);
  return (size_t)P * (D + 1) + 2 * (size_t)D + 8;
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_pool_init(PoolArgs a, double initial_step_size) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = a.s.full ? a.D * a.D : a.D;
  if (e < per) {  // mass_matrix.py:37-61: identity
    const double one = (!a.s.full || e / a.D == e % a.D) ? 1.0 : 0.0;
    a.s.wc_m2[e] = 0.0;
    a.s.imm[e] = one;
    a.s.sqrt_mass[e] = one;
  }
  if (e < a.D) a.s.wc_mean[e] = 0.0;
  if (e < a.C) a.s.step_size[e] = exp(0.0);
  if (e == 0) {  // algorithms.py:56-76, window_adaptation.py:139-140
    a.s.da_step[0] = 1;
    a.s.da_x[0] = 0.0;
    a.s.da_x_avg[0] = 0.0;
    a.s.da_g_avg[0] = 0.0;
    a.s.da_mu[0] = initial_step_size;
    a.s.wc_n[0] = 0;
  }
}

// grid (column blocks of 64 from `col0`, P); 64 columns x 4 chain phases per workgroup.  Phase s adds the chains
// lo + s, lo + s + 4, ... of its part in ascending order, then the four phases are added in order.
// SQ: squares about the batch mean b instead of the values (columns < D only)
template <bool SQ>
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_pool_colsum(PoolArgs a, long long col0) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const long long j = col0 + (long long)blockIdx.x * 64 + lane;
  const long long p = blockIdx.y;
  const long long lo = p * a.rows_per, hi = lo + a.rows_per < a.C ? lo + a.rows_per : a.C;
  const bool is_x = j < a.D, is_a = !SQ && j == a.D;
  double s = 0.0;
  if (is_x) {
    const double bj = SQ ? a.b[j] : 0.0;
    const double *x = a.position + j;
#pragma unroll 4
    for (long long c = lo + ph; c < hi; c += 4) {
      const double v = x[c * a.D];
      if (SQ) {
        const double d = v - bj;
        s = s + d * d;
      } else {
        s = s + v;
      }
    }
  } else if (is_a) {
    for (long long c = lo + ph; c < hi; c += 4) s = s + a.p_accept[c];
  }
  red[ph][lane] = s;
  __syncthreads();
  if (ph == 0 && (is_x || is_a)) a.part[p * (a.D + 1) + j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// slow stage: b = (sum of the parts) / C, d = b - mean, mean' = mean + d (C / n'); sc[0] = n C / n'
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_pool_mean(PoolArgs a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = a.s.wc_n[0], n1 = n + a.C;
  if (j == 0) a.sc[0] = ((double)n * (double)a.C) / (double)n1;
  if (j >= a.D) return;
  double s = a.part[j];
  for (int p = 1; p < a.P; p++) s = s + a.part[(long long)p * (a.D + 1) + j];
  const double b = s / (double)a.C;
  const double mean = a.s.wc_mean[j];
  const double d = b - mean;
  a.s.wc_mean[j] = mean + d * ((double)a.C / (double)n1);
  a.b[j] = b;
  a.delta[j] = d;
}

// diagonal metric, slow stage: m2' = m2 + (sum of the parts) + (n C / n') d^2; at a window end the new metric
// (adapt_window_end_elem: the per-chain expressions with the pooled count)
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_pool_sq(PoolArgs a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.D) return;
  const long long n1 = a.s.wc_n[0] + a.C;
  double s = a.part[j];
  for (int p = 1; p < a.P; p++) s = s + a.part[(long long)p * (a.D + 1) + j];
  const double d = a.delta[j];
  double m2 = (a.s.wc_m2[j] + s) + (a.sc[0] * d) * d;
  if (a.window_end) {
    double mean = 0.0, imm, sqrt_mass;
    adapt_window_end_elem(n1, mean, m2, imm, sqrt_mass);
    a.s.imm[j] = imm;
    a.s.sqrt_mass[j] = sqrt_mass;
    a.s.wc_mean[j] = mean;
  }
  a.s.wc_m2[j] = m2;
}

// dense metric, window end: imm from the LOWER triangle of m2, both triangles written from the same value (imm is
// bitwise symmetric); m2 and mean zeroed.  grid (nb, nb) blocks of 32 x 32, block (32, 8); blocks above the diagonal idle
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_pool_imm(PoolArgs a) {
  __shared__ double tile[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const long long D = a.D;
  const long long n1 = a.s.wc_n[0] + a.C;
  const double nn = (double)n1;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    const long long i = (long long)bi * 32 + r, j = (long long)bj * 32 + threadIdx.x;
    double v = 0.0;
    if (i < D && j <= i) {  // the expressions of k_adapt_update's full branch
      const double cov = a.s.wc_m2[i * D + j] / (double)(n1 - 1);
      v = (nn / (nn + 5)) * cov;
      if (i == j) v = v + 1e-3 * (5 / (nn + 5));
    }
    tile[r][threadIdx.x] = v;
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    const int cc = threadIdx.x;
    const long long i = (long long)bi * 32 + r, j = (long long)bj * 32 + cc;
    if (i < D && j < D) {
      if (bi != bj || cc <= r) {
        a.s.imm[i * D + j] = tile[r][cc];
        a.s.wc_m2[i * D + j] = 0.0;
      } else {  // diagonal block, above the diagonal: the mirrored element
        a.s.imm[i * D + j] = tile[cc][r];
        a.s.wc_m2[i * D + j] = 0.0;
      }
    }
    if (bi != bj) {  // the mirrored block
      const long long it = (long long)bj * 32 + r, jt = (long long)bi * 32 + cc;
      if (it < D && jt < D) {
        a.s.imm[it * D + jt] = tile[cc][r];
        a.s.wc_m2[it * D + jt] = 0.0;
      }
    }
  }
  if (bi == bj && threadIdx.y == 0) {
    const long long i = (long long)bi * 32 + threadIdx.x;
    if (i < D) a.s.wc_mean[i] = 0.0;
  }
}

// the scalars, last kernel of an update: abar, dual averaging (adapt_da_update: with C = 1 the per-chain kernel's
// bits), the sample count, restart at a window end, exp(x_avg) after the last step; the step size goes into all C
// entries of step_size, the array the step calls read through aehmc_set_step_sizes
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_pool_scalars(PoolArgs a) {
  __shared__ double s_eps;
  if (threadIdx.x == 0) {
    double s = a.part[a.D];
    for (int p = 1; p < a.P; p++) s = s + a.part[(long long)p * (a.D + 1) + a.D];
    const double abar = s / (double)a.C;
    DualAvg da = {a.s.da_step[0], a.s.da_x[0], a.s.da_x_avg[0], a.s.da_g_avg[0], a.s.da_mu[0]};
    double step_size = adapt_da_update(da, a.target, abar, a.gamma, a.t0, a.kappa);
    long long n = a.s.wc_n[0];
    if (a.stage != 0) n += a.C;
    if (a.window_end) {
      n = 0;
      adapt_da_restart(da, step_size);
    }
    if (a.last) step_size = exp(da.x_avg);  // window_adaptation.py:184-190
    a.s.da_step[0] = da.step;
    a.s.da_x[0] = da.x;
    a.s.da_x_avg[0] = da.x_avg;
    a.s.da_g_avg[0] = da.g_avg;
    a.s.da_mu[0] = da.mu;
    a.s.wc_n[0] = n;
    s_eps = step_size;
  }
  __syncthreads();
  const double eps = s_eps;
  for (long long c = threadIdx.x; c < a.C; c += blockDim.x) a.s.step_size[c] = eps;
}

inline hipError_t launch_pool_init(const PoolArgs &a, double initial_step_size, hipStream_t st) {
  const long long per = a.s.full ? a.D * a.D : a.D;
  const long long n = per > a.C ? per : a.C;
  hipLaunchKernelGGL(k_pool_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, initial_step_size);
  return hipGetLastError();
}
// everything of an update before the dense rank-C update: the column sums and, in a slow stage, the means (and the
// whole diagonal Welford update with its window end)
inline hipError_t launch_pool_sums(const PoolArgs &a, hipStream_t st) {
  const bool slow = a.stage != 0;
  const long long col0 = slow ? 0 : a.D;  // (a fast stage needs the acceptance column only)
  const unsigned colblocks = (unsigned)((a.D + 1 - col0 + 63) / 64);
  hipLaunchKernelGGL(k_pool_colsum<false>, dim3(colblocks, (unsigned)a.P), dim3(256), 0, st, a, col0);
  if (slow) {
    const dim3 grid((unsigned)((a.D + 255) / 256));
    hipLaunchKernelGGL(k_pool_mean, grid, dim3(256), 0, st, a);
    if (!a.s.full) {
      hipLaunchKernelGGL(k_pool_colsum<true>, dim3((unsigned)((a.D + 63) / 64), (unsigned)a.P), dim3(256), 0, st, a, 0LL);
      hipLaunchKernelGGL(k_pool_sq, grid, dim3(256), 0, st, a);
    }
  }
  return hipGetLastError();
}
inline hipError_t launch_pool_imm(const PoolArgs &a, hipStream_t st) {
  const unsigned nb = (unsigned)((a.D + 31) / 32);
  hipLaunchKernelGGL(k_pool_imm, dim3(nb, nb), dim3(32, 8), 0, st, a);
  return hipGetLastError();
}
inline hipError_t launch_pool_scalars(const PoolArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_pool_scalars, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
