// MEADS (Hoffman & Sountsov, "Tuning-Free Generalized Hamiltonian Monte Carlo", AISTATS 2022), the all-chains variant:
// step size, diagonal preconditioner, momentum damping and slice drift of generalised HMC (ghmc_fused.cuh) from
// closed-form cross-chain statistics of the current positions Q [C, D] and potential gradients G [C, D], C >= 2.
//
//   m = column means of Q;  var_i = (1 / C) sum_c (Q_ci - m_i)^2;  sd = sqrt(var);  Z = (Q - m) / sd;  Gs = G sd
//   lam(X), X [n, d] with Gram matrix S = X X^T:  [(sum_ab S_ab^2 - sum_a S_aa^2) / (n (n - 1))] / [sum_a S_aa / n]
//   eps = min(1, multiplier / sqrt(lam(Gs)));  gamma = max(1 / sqrt(lam(Z)), 1 / ((count + 1)^slowdown eps))
//   alpha = 1 - exp(-2 eps gamma);  delta = alpha / 2;  scale = sd;  count += 1
//   guard: eps, alpha, delta or some sd_i not finite, eps <= 0, or some sd_i = 0: parameters stay, skipped += 1
//
// The C x C matrix is never formed: sum_ab S_ab^2 = |X^T X|_F^2 and S_aa = |x_a|^2.  X^T X of Z is the CENTRED symmetric
// rank-C product of Q (syrk_f64.cuh) scaled entrywise by 1 / (sd_i sd_j), that of Gs the uncentred product of G scaled by
// sd_i sd_j; only the lower triangles exist, and var is the first one's diagonal over C.
//
// Launches of one update, all on the caller's stream (the two products between k_meads_mean and k_meads_sd are
// engine.hip's):
//   k_meads_colsum   partial column sums of Q over P contiguous parts of the chains (pool_parts; the four phases of
//                    k_pool_colsum, which itself also reads an acceptance column this update does not have)
//   k_meads_mean     parts added in ascending order: m
//   k_meads_sd       sd_i = sqrt(S_ii / C)
//   k_meads_rows     one wavefront per chain: |z_c|^2 and |gs_c|^2, lane-strided, each lane ascending, wave_sum
//   k_meads_frob     one workgroup per matrix row i: sum_{j <= i} of the scaled squares of both matrices (diag + 2 below)
//   k_meads_scalars  one workgroup: the per-chain and per-row numbers added in a fixed order, the formulas, the guard
// Every sum runs in an order fixed by (C, D); no atomics: two calls are bit-equal.
#pragma once
#include "pooled_adapt.cuh"

namespace aehmc {

struct MeadsArgs {
  long long C, D;
  double multiplier, slowdown;
  const double *Q, *G;
  aehmc_meads_state s;
  int P;               // parts of the chain range
  long long rows_per;  // chains per part
  double *part;        // [P][D] partial column sums
  double *m, *sd;      // [D]
  double *nz, *ng;     // [C] squared norms of the rows of Z and Gs
  double *fro;         // [2][D] per-row sums of the scaled squares
  double *Sz, *Sg;     // [D, D] lower triangles: centred Q^T Q, G^T G
};
constexpr int MEADS_SUMS = 8;  // scalars in front of m [D] and sd [D] in aehmc_meads_state.sums

inline size_t meads_work_doubles(long long C, long long D) {
  int P;
  long long rows_per;
  pool_parts(C, D, P, rows_per);
  return (size_t)P * D + 4 * (size_t)D + 2 * (size_t)C + 2 * (size_t)D * D;
}

// the parameters a call was handed as host numbers, into their device cell
AEHMC_TU_LOCAL __global__ void k_meads_set3(double *cell, double a, double b, double c) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    cell[0] = a;
    cell[1] = b;
    cell[2] = c;
  }
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_meads_colsum(MeadsArgs a) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const long long j = (long long)blockIdx.x * 64 + lane;
  const long long p = blockIdx.y;
  const long long lo = p * a.rows_per, hi = lo + a.rows_per < a.C ? lo + a.rows_per : a.C;
  double s = 0.0;
  if (j < a.D) {
    const double *x = a.Q + j;
#pragma unroll 4
    for (long long c = lo + ph; c < hi; c += 4) s = s + x[c * a.D];
  }
  red[ph][lane] = s;
  __syncthreads();
  if (ph == 0 && j < a.D) a.part[p * a.D + j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_meads_mean(MeadsArgs a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.D) return;
  double s = a.part[j];
  for (int p = 1; p < a.P; p++) s = s + a.part[(long long)p * a.D + j];
  a.m[j] = s / (double)a.C;
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_meads_sd(MeadsArgs a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < a.D) a.sd[j] = sqrt(a.Sz[j * a.D + j] / (double)a.C);
}

// one wavefront per chain, four chains a workgroup
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_meads_rows(MeadsArgs a) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.C) return;
  const double *q = a.Q + c * a.D, *g = a.G + c * a.D;
  double nz = 0.0, ng = 0.0;
#pragma unroll 2
  for (long long i = lane; i < a.D; i += 64) {
    const double sd = a.sd[i];
    const double z = (q[i] - a.m[i]) / sd;
    const double gs = g[i] * sd;
    nz = nz + z * z;
    ng = ng + gs * gs;
  }
  nz = wave_sum(nz);
  ng = wave_sum(ng);
  if (lane == 0) {
    a.nz[c] = nz;
    a.ng[c] = ng;
  }
}

// the 256 numbers of a workgroup, thread t's in x, added ascending by thread 0 (the same value to every thread)
__device__ __forceinline__ double meads_block_sum(double x, double *red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = x;
  __syncthreads();
  double s = red[0];
  if (t == 0)
    for (int i = 1; i < 256; i++) s = s + red[i];
  __syncthreads();
  if (t == 0) red[0] = s;
  __syncthreads();
  return red[0];
}

// row i of both lower triangles: (S_ij / (sd_i sd_j))^2 and (S_ij sd_i sd_j)^2 over j <= i, the diagonal once, the rest twice
AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_meads_frob(MeadsArgs a) {
  __shared__ double red[256];
  const long long i = blockIdx.x;
  const int t = threadIdx.x;
  const double sdi = a.sd[i];
  const double *rz = a.Sz + i * a.D, *rg = a.Sg + i * a.D;
  double fz = 0.0, fg = 0.0;
  for (long long j = t; j < i; j += 256) {
    const double w = sdi * a.sd[j];
    const double xz = rz[j] / w, xg = rg[j] * w;
    fz = fz + xz * xz;
    fg = fg + xg * xg;
  }
  fz = meads_block_sum(fz, red);
  fg = meads_block_sum(fg, red);
  if (t == 0) {
    const double w = sdi * sdi;
    const double dz = rz[i] / w, dg = rg[i] * w;
    a.fro[i] = dz * dz + 2.0 * fz;
    a.fro[a.D + i] = dg * dg + 2.0 * fg;
  }
}

// thread t adds x[t], x[t + 256], ... ascending (squared when SQ), then the 256 partial sums ascending
template <bool SQ>
__device__ __forceinline__ double meads_strided_sum(const double *x, long long n, double *red) {
  double s = 0.0;
  for (long long k = threadIdx.x; k < n; k += 256) s = s + (SQ ? x[k] * x[k] : x[k]);
  return meads_block_sum(s, red);
}

AEHMC_TU_LOCAL __global__ __launch_bounds__(256) void k_meads_scalars(MeadsArgs a) {
  __shared__ double red[256];
  __shared__ int s_ok;
  const int t = threadIdx.x;
  const double z4 = meads_strided_sum<true>(a.nz, a.C, red), z2 = meads_strided_sum<false>(a.nz, a.C, red);
  const double g4 = meads_strided_sum<true>(a.ng, a.C, red), g2 = meads_strided_sum<false>(a.ng, a.C, red);
  const double Fz = meads_strided_sum<false>(a.fro, a.D, red), Fg = meads_strided_sum<false>(a.fro + a.D, a.D, red);
  double bad = 0.0;  // some sd_i zero or not finite
  for (long long j = t; j < a.D; j += 256) {
    const double sd = a.sd[j];
    if (!isfinite(sd) || sd == 0.0) bad = 1.0;
  }
  bad = meads_block_sum(bad, red);
  if (t == 0) {
    const double n = (double)a.C;
    const double lam_z = ((Fz - z4) / (n * (n - 1.0))) / (z2 / n);
    const double lam_g = ((Fg - g4) / (n * (n - 1.0))) / (g2 / n);
    const long long count = a.s.count[0];
    double eps = a.multiplier / sqrt(lam_g);
    if (eps > 1.0) eps = 1.0;
    const double g_lam = 1.0 / sqrt(lam_z), g_slow = 1.0 / (pow((double)(count + 1), a.slowdown) * eps);
    const double gamma = g_lam > g_slow ? g_lam : g_slow;
    const double alpha = 1.0 - exp(-2.0 * (eps * gamma));
    const double delta = alpha / 2.0;
    const int ok = isfinite(eps) && isfinite(alpha) && isfinite(delta) && eps > 0.0 && bad == 0.0;
    if (ok) {
      a.s.params[0] = eps;
      a.s.params[1] = alpha;
      a.s.params[2] = delta;
    } else {
      a.s.skipped[0] = a.s.skipped[0] + 1;
    }
    a.s.count[0] = count + 1;
    if (a.s.sums) {
      a.s.sums[0] = z4; a.s.sums[1] = z2; a.s.sums[2] = g4; a.s.sums[3] = g2;
      a.s.sums[4] = Fz; a.s.sums[5] = Fg; a.s.sums[6] = lam_z; a.s.sums[7] = lam_g;
    }
    s_ok = ok;
  }
  __syncthreads();
  if (s_ok)
    for (long long j = t; j < a.D; j += 256) a.s.scale[j] = a.sd[j];
  if (a.s.sums)  // (m and sd are adjacent in the scratch)
    for (long long j = t; j < 2 * a.D; j += 256) a.s.sums[MEADS_SUMS + j] = a.m[j];
}

inline hipError_t launch_meads_set3(double *cell, double x, double y, double z, hipStream_t st) {
  hipLaunchKernelGGL(k_meads_set3, dim3(1), dim3(64), 0, st, cell, x, y, z);
  return hipGetLastError();
}
// before the two rank-C products: the column means
inline hipError_t launch_meads_means(const MeadsArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_meads_colsum, dim3((unsigned)((a.D + 63) / 64), (unsigned)a.P), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_meads_mean, dim3((unsigned)((a.D + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
// behind them
inline hipError_t launch_meads_finish(const MeadsArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_meads_sd, dim3((unsigned)((a.D + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_meads_rows, dim3((unsigned)((a.C + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_meads_frob, dim3((unsigned)a.D), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_meads_scalars, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
