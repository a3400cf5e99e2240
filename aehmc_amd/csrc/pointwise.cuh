// Pointwise log-likelihoods of traced models and streaming WAIC (aehmc_set_pointwise / aehmc_pointwise_eval /
// aehmc_pointwise_waic_fold / aehmc_waic_fold / aehmc_waic_merge / aehmc_waic_final; aehmc_amd/summary.py).
//
// A pointwise program (aehmc_amd/tracing.py: trace_pointwise) is a vector function of one chain's position:
//   template <class V> __device__ void aehmc_pointwise_head(const V &q, const double *const *prm, double *h);
//   template <class V> __device__ double aehmc_pointwise(const V &q, const double *h, long long j, const double *const *prm);
// entry j of the vector from the row q and the row's n_head head values (what does not depend on j: log(sigma)).
//
// k_pointwise<FOLD, STAGE>, compiled at run time against such a source (define AEHMC_POINTWISE_TARGET first).
//   Geometry.  One thread owns one entry j.  A workgroup of PW_TILE threads owns a tile of PW_TILE consecutive j
//   (blockIdx.y) and ONE PART of the rows (blockIdx.x): rows [part PW_PART, (part + 1) PW_PART), cut by the row count alone.
//   Batches.  The part's rows are served `batch` at a time.  STAGE: the batch's rows are copied to LDS (contiguous in
//   memory: coalesced), threads 0 ... rows-1 run aehmc_pointwise_head for one row each into LDS, and every thread walks
//   the batch's rows in ascending order; a row read is one LDS address for all lanes (a broadcast).  !STAGE (a row too
//   long for a useful batch): the rows are read from global memory, again one address for all lanes; only the head values
//   go through LDS.  pw_plan states the rule.
//   FOLD = false: out[r][j] is written; a row's PW_TILE entries are consecutive doubles.
//   FOLD = true: nothing the size of the output exists.  The thread folds its entry's values over the part's rows into
//   (m, s, mean, M2) -- running maximum, sum of exp(l - m) rescaled when m grows, Welford's mean and sum of squared
//   deviations -- and writes the four numbers to the workspace [parts][4][n_out].
// k_waic_fold_stored: the same body with a loader that reads a stored block x[r][j]; precompiled (tu_pointwise.hip).
// k_waic_merge: one thread per observation adds the parts, in ascending order, to the state [4][n_obs] that holds what was
//   folded before: max-rescaling for (m, s), the pairwise update of Chan, Golub & LeVeque (1983) for (mean, M2).  The
//   number of draws behind the state lives on the host.
// k_waic_final: lppd_i = m + log(s) - log(S), p_i = M2 / (S - 1).
//
// Arithmetic (every operation rounded on its own: -ffp-contract=off), draw l as the k-th of its part (k = 1, 2, ...):
//   l != -inf:  l > m:  s = s exp(m - l) + 1, m = l;   else  s = s + (l == m ? 1 : exp(l - m))
//   d = l - mean;  mean = mean + d / k;  M2 = M2 + d (l - mean)
// part B (nB draws) onto state A (nA draws), n = nA + nB; nA == 0: A = B; else
//   mB > mA:  sA = sA exp(mA - mB) + sB, mA = mB;   else  sA = sA + sB (mB == mA ? 1 : exp(mB - mA))
//   d = meanB - meanA;  mean = meanA + d (nB / n);  M2 = (M2A + M2B) + (d d) (nA nB / n)
// Non-finite draws behave as in summary.waic on the stored array: a -inf draw adds nothing to s (also as the first draw
// of its observation: exp(-inf - -inf) is never formed) and makes M2, so p_i, NaN; a NaN makes s, mean and M2 NaN.  An
// observation's numbers come from its own column alone.  No atomics: two identical calls give the same bits.
#pragma once
#ifndef __HIPCC_RTC__ /* (hipRTC supplies the runtime, the math functions and the fixed-width integers itself) */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#endif

namespace aehmc {

constexpr int PW_TILE = 256;          // entries per workgroup, one per thread (four wavefronts of 64)
constexpr int PW_PART = 256;          // rows per part: the fold's partition, a function of the row count alone
constexpr int PW_BATCH_MAX = 32;      // rows per batch at most (the head runs on one thread per row of the batch)
constexpr int PW_STAGE_MIN_ROWS = 4;  // rows are staged in LDS only if at least this many fit
constexpr int PW_LDS_BYTES = 65536;   // LDS of a workgroup at most: two workgroups per CU (160 KiB)

struct PwArgs {
  const double *x;           // the rows: positions [R][D], or a stored block [R][n_out] (k_waic_fold_stored)
  double *out;               // FOLD = false: [R][n_out]; FOLD = true: the workspace [parts][4][n_out]
  const double *const *prm;  // the program's parameter arrays (device)
  long long R, D, n_out;
  int n_head, batch;
};

struct PwFold {
  double m, s, mean, m2;
};

__device__ inline double pw_neg_inf() { return -__builtin_huge_val(); }

__device__ inline void pw_fold_draw(PwFold &f, double l, double k) {
  if (l != pw_neg_inf()) {  // (a NaN passes and poisons s)
    if (l > f.m) {
      f.s = f.s * exp(f.m - l) + 1.0;
      f.m = l;
    } else {
      f.s = f.s + (l == f.m ? 1.0 : exp(l - f.m));
    }
  }
  const double d = l - f.mean;
  f.mean = f.mean + d / k;
  f.m2 = f.m2 + d * (l - f.mean);
}

__device__ inline void pw_fold_merge(PwFold &a, double na, const PwFold &b, double nb) {
  if (na == 0.0) {
    a = b;
    return;
  }
  if (b.m > a.m) {
    a.s = a.s * exp(a.m - b.m) + b.s;
    a.m = b.m;
  } else {
    a.s = a.s + b.s * (b.m == a.m ? 1.0 : exp(b.m - a.m));
  }
  const double n = na + nb, d = b.mean - a.mean;
  a.mean = a.mean + d * (nb / n);
  a.m2 = (a.m2 + b.m2) + (d * d) * (na * nb / n);
}

// one workgroup: a tile of entries (blockIdx.y) over one part of the rows (blockIdx.x).  L: where a value comes from
template <bool FOLD, class L>
__device__ inline void pw_body(const PwArgs &a, double *lds) {
  const long long j = (long long)blockIdx.y * PW_TILE + threadIdx.x;
  const bool live = j < a.n_out;
  const long long part = blockIdx.x;
  const long long r0 = part * PW_PART;
  const long long r1 = r0 + PW_PART < a.R ? r0 + PW_PART : a.R;
  PwFold f{pw_neg_inf(), 0.0, 0.0, 0.0};
  double k = 0.0;
  for (long long b0 = r0; b0 < r1; b0 += a.batch) {
    const int nb = (int)(r1 - b0 < a.batch ? r1 - b0 : a.batch);
    L::stage(a, lds, b0, nb);  // (every thread of the workgroup: it synchronises)
    if (live) {
      for (int t = 0; t < nb; ++t) {
        const double l = L::value(a, lds, b0 + t, t, j);
        if (FOLD) {
          k += 1.0;
          pw_fold_draw(f, l, k);
        } else {
          a.out[(b0 + t) * a.n_out + j] = l;
        }
      }
    }
  }
  if (FOLD && live) {
    double *w = a.out + part * 4 * a.n_out + j;
    w[0] = f.m;
    w[a.n_out] = f.s;
    w[2 * a.n_out] = f.mean;
    w[3 * a.n_out] = f.m2;
  }
}

struct PwStored {  // a stored block of values: nothing to stage
  __device__ static inline void stage(const PwArgs &, double *, long long, int) {}
  __device__ static inline double value(const PwArgs &a, const double *, long long r, int, long long j) {
    return a.x[r * a.n_out + j];
  }
};

#ifdef AEHMC_POINTWISE_TARGET
struct PwRow {  // a row of coordinates as the traced functions read it
  const double *p;
  __device__ inline __attribute__((always_inline)) double operator[](long long i) const { return p[i]; }
};
template <bool STAGE>
struct PwTraced {
  __device__ static inline void stage(const PwArgs &a, double *lds, long long b0, int nb) {
    const int tid = threadIdx.x;
    __syncthreads();  // (the previous batch has been read)
    if constexpr (STAGE) {
      const double *src = a.x + b0 * a.D;
      const long long n = (long long)nb * a.D;
      for (long long e = tid; e < n; e += PW_TILE) lds[e] = src[e];
      __syncthreads();
    }
    if (a.n_head > 0 && tid < nb) {
      if constexpr (STAGE)
        aehmc_pointwise_head(PwRow{lds + (long long)tid * a.D}, a.prm, lds + (long long)a.batch * a.D + (long long)tid * a.n_head);
      else
        aehmc_pointwise_head(PwRow{a.x + (b0 + tid) * a.D}, a.prm, lds + (long long)tid * a.n_head);
    }
    __syncthreads();
  }
  __device__ static inline double value(const PwArgs &a, const double *lds, long long r, int t, long long j) {
    if constexpr (STAGE)
      return aehmc_pointwise(PwRow{lds + (long long)t * a.D}, lds + (long long)a.batch * a.D + (long long)t * a.n_head, j, a.prm);
    else
      return aehmc_pointwise(PwRow{a.x + r * a.D}, lds + (long long)t * a.n_head, j, a.prm);
  }
};
template <bool FOLD, bool STAGE>
__global__ __launch_bounds__(PW_TILE) void k_pointwise(PwArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pw_lds[];
  pw_body<FOLD, PwTraced<STAGE>>(a, pw_lds);
}
#endif  // AEHMC_POINTWISE_TARGET

#ifndef __HIPCC_RTC__  // (the host side)
// The batch.  A row of the batch takes D + n_head doubles of LDS when the rows are staged, n_head when they are not.
// Staged if PW_STAGE_MIN_ROWS rows fit in PW_LDS_BYTES (D + n_head <= 2048); the batch is then as many rows as fit, at
// most PW_BATCH_MAX.  Otherwise (positions up to the joint-density limit of 10176 coordinates) the rows stay in global
// memory and the batch is what the head values allow.  batch = 0: the head alone does not fit (n_head > 8192).
struct PwPlan {
  bool stage;
  int batch;
  size_t lds;
};
inline PwPlan pw_plan(long long D, long long n_head) {
  PwPlan p;
  p.stage = (D + n_head) * 8 * PW_STAGE_MIN_ROWS <= PW_LDS_BYTES;
  const long long per_row = ((p.stage ? D : 0) + n_head) * 8;
  long long b = per_row > 0 ? PW_LDS_BYTES / per_row : PW_BATCH_MAX;
  if (b > PW_BATCH_MAX) b = PW_BATCH_MAX;
  p.batch = (int)b;
  p.lds = (size_t)(b * per_row);
  return p;
}
inline long long pw_parts(long long R) { return (R + PW_PART - 1) / PW_PART; }
inline size_t pw_work_doubles(long long R, long long n_obs) { return (size_t)pw_parts(R) * 4 * (size_t)n_obs; }

#endif  // __HIPCC_RTC__

#ifdef AEHMC_POINTWISE_TU  // (the precompiled kernels: instantiated in tu_pointwise.hip alone)
__global__ __launch_bounds__(PW_TILE) void k_waic_fold_stored(PwArgs a) { pw_body<true, PwStored>(a, nullptr); }

// ws [parts][4][n_obs]: part p holds min(part_rows, R - p part_rows) draws; state [4][n_obs] holds n_state draws
__global__ __launch_bounds__(256) void k_waic_merge(const double *ws, long long parts, long long part_rows, long long R,
                                                   double *state, double n_state, long long n_obs) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_obs) return;
  PwFold f{state[j], state[n_obs + j], state[2 * n_obs + j], state[3 * n_obs + j]};
  double na = n_state;
  for (long long p = 0; p < parts; ++p) {
    const long long left = R - p * part_rows;
    const double nb = (double)(left < part_rows ? left : part_rows);
    const double *w = ws + p * 4 * n_obs + j;
    pw_fold_merge(f, na, PwFold{w[0], w[n_obs], w[2 * n_obs], w[3 * n_obs]}, nb);
    na += nb;
  }
  state[j] = f.m;
  state[n_obs + j] = f.s;
  state[2 * n_obs + j] = f.mean;
  state[3 * n_obs + j] = f.m2;
}

__global__ __launch_bounds__(256) void k_waic_final(const double *state, double n_state, long long n_obs, double *lppd,
                                                   double *p) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_obs) return;
  lppd[j] = (state[j] + log(state[n_obs + j])) - log(n_state);
  p[j] = state[3 * n_obs + j] / (n_state - 1.0);
}

inline hipError_t launch_waic_fold_stored(const double *x, long long R, long long n_obs, double *ws, hipStream_t st) {
  PwArgs a{};
  a.x = x; a.out = ws; a.prm = nullptr;
  a.R = R; a.D = 0; a.n_out = n_obs; a.n_head = 0; a.batch = PW_BATCH_MAX;
  hipLaunchKernelGGL(k_waic_fold_stored, dim3((unsigned)pw_parts(R), (unsigned)((n_obs + PW_TILE - 1) / PW_TILE)), dim3(PW_TILE), 0, st, a);
  return hipGetLastError();
}
inline hipError_t launch_waic_merge(const double *ws, long long parts, long long part_rows, long long R, double *state,
                                    double n_state, long long n_obs, hipStream_t st) {
  hipLaunchKernelGGL(k_waic_merge, dim3((unsigned)((n_obs + 255) / 256)), dim3(256), 0, st, ws, parts, part_rows, R, state, n_state, n_obs);
  return hipGetLastError();
}
inline hipError_t launch_waic_final(const double *state, double n_state, long long n_obs, double *lppd, double *p, hipStream_t st) {
  hipLaunchKernelGGL(k_waic_final, dim3((unsigned)((n_obs + 255) / 256)), dim3(256), 0, st, state, n_state, n_obs, lppd, p);
  return hipGetLastError();
}
#endif  // AEHMC_POINTWISE_TU

}  // namespace aehmc
