// ChEES warm-up for static HMC (Hoffman, Radul, Sountsov, AISTATS 2021): ONE trajectory length T and ONE step size
// adapted from all chains together (chees.run; the pooled step-size / metric adaptation is in pooled_adapt.cuh).
//
// The HMC kernels export the state a transition returns, its acceptance probability and the accept flag, not the
// proposal.  Since E[1{accept} f(proposal)] = E[alpha f(proposal)], the accept flag weights the returned state: on
// accept that state IS the proposal with the momentum flipped (hmc.py:185), so the end velocity is v = -M^-1 momentum.
//
// One update, positions q0 / q1 [C, D] before / after the transition, momentum [C, D], accept flags and acceptance
// probabilities [C]; n = step, T = exp(log_T), h the Halton weight the transition ran with:
//   m0, m1 = column means of q0, q1 over ALL chains
//   s_c = (|q1_c - m1|^2 - |q0_c - m0|^2) <q1_c - m1, v_c>,  v_c = -imm o momentum_c  (imm: [D], or a scalar)
//   A = sum_c accepted_c,  S = sum_c (accepted_c ? s_c : 0)   (a select: a rejected chain's rows are not even read)
//   G = h T S / max(A, 1); 0 when A = 0 or G is not finite
//   Adam ascent on log_T (beta 0.9 / 0.999, 1e-8, bias corrected with n)
//   abar = (sum_c a_c) / C -> adapt_da_update (engine.cuh) with gamma 0.05, t0 10, kappa 0.75 -> eps, all C entries
//   log_T clamped to [log eps, log(max_num_steps eps)];  log_T_avg = w log_T + (1 - w) log_T_avg, w = n^-kappa
//   last: eps = exp(x_avg), log_T = log_T_avg
//   step = n + 1, h = base-2 radical inverse of n + 1, num_steps = max(1, ceil(h T / eps)) capped at max_num_steps
//
// Launches of one update, all on the caller's stream:
//   k_chees_colsum   partial column sums of q0 (columns < D), q1 (D .. 2D - 1), a (2D) and the accept flags (2D + 1)
//                    over P contiguous parts of the chains: the (P, rows_per) of pool_parts, the four phases of
//                    k_pool_colsum
//   k_chees_mean     parts added in ascending order: m0, m1
//   k_chees_chain    one wavefront per chain: the three dot products lane-strided over D (one 8-byte load per lane and
//                    array, 512 contiguous bytes per wavefront), each lane in ascending order, wave_sum; s_c to scratch
//   k_chees_scalars  one workgroup: s_c added in a fixed order (thread t: c = t, t + 256, ... ascending; then the 256
//                    partial sums ascending), then the scalar arithmetic above
// Every sum runs in an order fixed by (C, D); no atomics: two calls are bit-equal.  Five reads of [C, D] per update.
#pragma once
#include "pooled_adapt.cuh"

namespace aehmc {

struct CheesArgs {
  long long C, D;
  int last;
  double target, lr;
  long long max_steps;
  const double *q0, *q1, *mom, *imm;  // imm: [D] or nullptr (then imm_scalar)
  double imm_scalar;
  const int *accepted;
  const double *p_accept;
  aehmc_chees_state s;
  int P;               // parts of the chain range
  long long rows_per;  // chains per part
  double *part;        // [P][2 D + 2] partial sums
  double *m0, *m1;     // [D] column means
  double *sc;          // [C] per-chain criterion
};

inline void chees_parts(long long C, long long D, int &P, long long &rows_per) { pool_parts(C, 2 * D + 1, P, rows_per); }
inline size_t chees_work_doubles(long long C, long long D) {
  int P;
  long long rows_per;
  chees_parts(C, D, P, rows_per);
  return (size_t)P * (2 * D + 2) + 2 * (size_t)D + (size_t)C;
}

// base-2 radical inverse: 1/2, 1/4, 3/4, 1/8, ... (exact: a sum of distinct powers of two)
__device__ __forceinline__ double chees_halton(long long n) {
  double h = 0.0, f = 0.5;
  for (; n > 0; n >>= 1, f = f * 0.5)
    if (n & 1) h = h + f;
  return h;
}
// L of the next transition: max(1, ceil(h T / eps)) capped at `most` (a quotient that is not a number gives 1)
__device__ __forceinline__ long long chees_num_steps(double h, double T, double eps, long long most) {
  const double r = ceil((h * T) / eps);
  if (!(r >= 1.0)) return 1;
  return r < (double)most ? (long long)r : most;
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_chees_init(CheesArgs a, double initial_step_size,
                                                                   double initial_trajectory_length) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const double eps = exp(0.0);  // dual averaging as k_pool_init starts it: x = 0, the shrinkage point as given
  if (e < a.C) a.s.step_size[e] = eps;
  if (e == 0) {
    a.s.da_step[0] = 1;
    a.s.da_x[0] = 0.0;
    a.s.da_x_avg[0] = 0.0;
    a.s.da_g_avg[0] = 0.0;
    a.s.da_mu[0] = initial_step_size;
    const double log_T = log(initial_trajectory_length);
    a.s.step[0] = 1;
    a.s.log_T[0] = log_T;
    a.s.log_T_avg[0] = log_T;
    a.s.adam_m[0] = 0.0;
    a.s.adam_v[0] = 0.0;
    a.s.h[0] = 0.5;
    a.s.num_steps[0] = chees_num_steps(0.5, exp(log_T), eps, a.max_steps);
  }
}

// grid (column blocks of 64, P); 64 columns x 4 chain phases per workgroup, as k_pool_colsum: phase s adds the chains
// lo + s, lo + s + 4, ... of its part in ascending order, then the four phases are added in order
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_chees_colsum(CheesArgs a) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const long long j = (long long)blockIdx.x * 64 + lane;
  const long long p = blockIdx.y;
  const long long lo = p * a.rows_per, hi = lo + a.rows_per < a.C ? lo + a.rows_per : a.C;
  const long long W = 2 * a.D + 2;
  double s = 0.0;
  if (j < 2 * a.D) {
    const double *x = j < a.D ? a.q0 + j : a.q1 + (j - a.D);
#pragma unroll 4
    for (long long c = lo + ph; c < hi; c += 4) s = s + x[c * a.D];
  } else if (j == 2 * a.D) {
    for (long long c = lo + ph; c < hi; c += 4) s = s + a.p_accept[c];
  } else if (j == 2 * a.D + 1) {
    for (long long c = lo + ph; c < hi; c += 4) s = s + (a.accepted[c] ? 1.0 : 0.0);
  }
  red[ph][lane] = s;
  __syncthreads();
  if (ph == 0 && j < W) a.part[p * W + j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_chees_mean(CheesArgs a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * a.D) return;
  const long long W = 2 * a.D + 2;
  double s = a.part[j];
  for (int p = 1; p < a.P; p++) s = s + a.part[(long long)p * W + j];
  const double m = s / (double)a.C;
  if (j < a.D) a.m0[j] = m;
  else a.m1[j - a.D] = m;
}

// one wavefront per chain, four chains a workgroup
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_chees_chain(CheesArgs a) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.C) return;
  double n0 = 0.0, n1 = 0.0, dot = 0.0;
  if (a.accepted[c]) {  // (wave-uniform)
    const double *q0 = a.q0 + c * a.D, *q1 = a.q1 + c * a.D, *mom = a.mom + c * a.D;
    const double sc = a.imm_scalar;
#pragma unroll 2
    for (long long i = lane; i < a.D; i += 64) {
      const double d0 = q0[i] - a.m0[i];
      const double d1 = q1[i] - a.m1[i];
      const double v = -((a.imm ? a.imm[i] : sc) * mom[i]);
      n0 = n0 + d0 * d0;
      n1 = n1 + d1 * d1;
      dot = dot + d1 * v;
    }
  }
  n0 = wave_sum(n0);
  n1 = wave_sum(n1);
  dot = wave_sum(dot);
  if (lane == 0) a.sc[c] = (n1 - n0) * dot;
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_chees_scalars(CheesArgs a) {
  __shared__ double red[256];
  __shared__ double s_eps;
  const int t = threadIdx.x;
  double s = 0.0;
  for (long long c = t; c < a.C; c += 256) s = s + (a.accepted[c] ? a.sc[c] : 0.0);
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    const long long W = 2 * a.D + 2;
    double S = red[0];
    for (int i = 1; i < 256; i++) S = S + red[i];
    double sa = a.part[2 * a.D], A = a.part[2 * a.D + 1];
    for (int p = 1; p < a.P; p++) {
      sa = sa + a.part[(long long)p * W + 2 * a.D];
      A = A + a.part[(long long)p * W + 2 * a.D + 1];
    }
    const double abar = sa / (double)a.C;
    if (a.s.sums) {
      a.s.sums[0] = S;
      a.s.sums[1] = A;
      a.s.sums[2] = abar;
    }
    const long long n = a.s.step[0];
    const double nn = (double)n;
    const double h = a.s.h[0];
    double log_T = a.s.log_T[0];
    double G = ((h * exp(log_T)) * S) / (A > 1.0 ? A : 1.0);
    if (A == 0.0 || !isfinite(G)) G = 0.0;
    const double m = 0.9 * a.s.adam_m[0] + 0.1 * G;
    const double v = 0.999 * a.s.adam_v[0] + 0.001 * (G * G);
    const double mhat = m / (1.0 - pow(0.9, nn)), vhat = v / (1.0 - pow(0.999, nn));
    log_T = log_T + a.lr * (mhat / (sqrt(vhat) + 1e-8));
    DualAvg da = {a.s.da_step[0], a.s.da_x[0], a.s.da_x_avg[0], a.s.da_g_avg[0], a.s.da_mu[0]};
    double eps = adapt_da_update(da, a.target, abar, 0.05, 10.0, 0.75);  // step_size.py:9-14
    const double lo = log(eps), hi = log((double)a.max_steps * eps);
    log_T = log_T < lo ? lo : (log_T > hi ? hi : log_T);
    const double w = pow(nn, -0.75);
    const double log_T_avg = w * log_T + (1.0 - w) * a.s.log_T_avg[0];
    if (a.last) {
      eps = exp(da.x_avg);
      log_T = log_T_avg;
    }
    const double h1 = chees_halton(n + 1);
    a.s.step[0] = n + 1;
    a.s.log_T[0] = log_T;
    a.s.log_T_avg[0] = log_T_avg;
    a.s.adam_m[0] = m;
    a.s.adam_v[0] = v;
    a.s.h[0] = h1;
    a.s.num_steps[0] = chees_num_steps(h1, exp(log_T), eps, a.max_steps);
    a.s.da_step[0] = da.step;
    a.s.da_x[0] = da.x;
    a.s.da_x_avg[0] = da.x_avg;
    a.s.da_g_avg[0] = da.g_avg;
    a.s.da_mu[0] = da.mu;
    s_eps = eps;
  }
  __syncthreads();
  const double eps = s_eps;
  for (long long c = t; c < a.C; c += 256) a.s.step_size[c] = eps;
  if (a.s.sums)  // (m0 and m1 are adjacent in the scratch)
    for (long long j = t; j < 2 * a.D; j += 256) a.s.sums[3 + j] = a.m0[j];
}

inline hipError_t launch_chees_init(const CheesArgs &a, double initial_step_size, double initial_trajectory_length,
                                    hipStream_t st) {
  hipLaunchKernelGGL(k_chees_init, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, st, a, initial_step_size,
                     initial_trajectory_length);
  return hipGetLastError();
}
inline hipError_t launch_chees_update(const CheesArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_chees_colsum, dim3((unsigned)((2 * a.D + 2 + 63) / 64), (unsigned)a.P), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_chees_mean, dim3((unsigned)((2 * a.D + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_chees_chain, dim3((unsigned)((a.C + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_chees_scalars, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
