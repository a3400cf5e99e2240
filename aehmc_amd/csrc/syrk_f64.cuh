// Symmetric rank-C update on fp64 MFMA (gfx950, wave64): the lower triangle of
//     S[i,j] += sum_c (X[c,i] - b[i]) (X[c,j] - b[j]) + w d[i] d[j],      j <= i,
// with X chain-major [C, D] as the engine keeps its draws -- the product X^T X ("TN"), the sum running over the ROWS of
// X.  What pooled window adaptation adds to its Welford matrix per warm-up step (pooled_adapt.cuh).
//
//  - Tiles BM x BM on and below the diagonal only: half the flops of the full product, half of S touched.  Inside a
//    diagonal tile the 16 x 16 blocks strictly above the diagonal are skipped too.
//  - X is read as it lies: a K-tile is 16 chains x BM coordinates, rows contiguous in the coordinate.  Centring
//    (x - b[i], one rounding) happens on the way into LDS; no transposed or centred copy of the draws exists.
//  - The LDS image is [k][i], i contiguous.  v_mfma_f64_16x16x4_f64 wants, from lane l, A[row l & 15][k l >> 4] and
//    B[k l >> 4][col l & 15]: with A[row][k] = tile_i[k][row] and B[k][col] = tile_j[k][col] both are the SAME read,
//    image[4 kk + (l >> 4)][base + (l & 15)] -- no transposing read, and on a diagonal tile one image serves both.
//    Row stride BM + 16 doubles: 2 (BM + 16) = 32 (mod 64) dwords, so the lanes l and l + 16 of a 32-lane half (k and
//    k + 1) fall on opposite halves of the 64 banks -- ds_read_b64 conflict-free.
//  - Chains are summed in ascending K-tiles of 16 with one accumulator chain per output; a tail of C % 16 chains is
//    zero-filled.  Mid-size D has few tiles (D = 200: ten of 64 x 64), so the chain range is cut into a FIXED number of
//    contiguous parts (syrk_plan: a function of C and D alone), each part's tile written to scratch and the parts added
//    in ascending order by a second kernel.  No atomics; the result depends on the shapes alone.
//  - S is read and written once: accumulate and rank-one term in the epilogue (or in the reducing kernel).
// Elements strictly above the diagonal are not written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace aehmc {

typedef double syrk_d4 __attribute__((ext_vector_type(4)));
constexpr int SYRK_BK = 16;

struct SyrkPlan {
  int bm;            // tile edge: 32, 64 or 128
  int nt;            // tiles per edge
  long long tiles;   // nt (nt + 1) / 2
  int parts;         // parts of the chain range (1: epilogue in the product kernel)
  long long kt_per;  // K-tiles per part
};
// the tile by D so that mid-size problems still fill the GPU; a function of the shapes alone
inline SyrkPlan syrk_plan(long long C, long long D) {
  SyrkPlan p;
  p.bm = D <= 32 ? 32 : (D <= 2048 ? 64 : 128);
  p.nt = (int)((D + p.bm - 1) / p.bm);
  p.tiles = (long long)p.nt * (p.nt + 1) / 2;
  const long long nk = (C + SYRK_BK - 1) / SYRK_BK;
  long long want = p.tiles >= 256 ? 1 : (512 + p.tiles - 1) / p.tiles;
  if (want > nk) want = nk;
  if (want < 1) want = 1;
  p.kt_per = (nk + want - 1) / want;
  p.parts = (int)((nk + p.kt_per - 1) / p.kt_per);
  return p;
}
inline size_t syrk_partial_doubles(long long C, long long D) {
  const SyrkPlan p = syrk_plan(C, D);
  return p.parts > 1 ? (size_t)p.parts * p.tiles * p.bm * p.bm : 0;
}

// lower-triangle tile t -> (ti, tj), tj <= ti, t = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void syrk_tile_of(long long t, int &ti, int &tj) {
  long long r = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) r++;
  while (r * (r + 1) / 2 > t) r--;
  ti = (int)r;
  tj = (int)(t - r * (r + 1) / 2);
}

template <int BM>
__global__ __launch_bounds__(256, 2) void syrk_tn_f64_kernel(long long C, long long D, const double *__restrict__ X,
                                                             long long ldx, const double *__restrict__ centre, double w,
                                                             const double *__restrict__ w_dev,
                                                             const double *__restrict__ delta, double *__restrict__ S,
                                                             long long lds_, long long kt_per,
                                                             double *__restrict__ partial) {
  constexpr int LW = BM + 16, HALF = BM / 2, NI = BM / 32, NL = BM / 16;
  __shared__ __attribute__((aligned(16))) double img[2][2][SYRK_BK][LW];  // [stage][row tile | column tile][k][i]
  int ti, tj;
  syrk_tile_of(blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;
  const long long i0 = (long long)ti * BM, j0 = (long long)tj * BM;
  const long long kt0 = (long long)blockIdx.y * kt_per;
  const long long nk_all = (C + SYRK_BK - 1) / SYRK_BK;
  const long long kt1 = kt0 + kt_per < nk_all ? kt0 + kt_per : nk_all;

  // this thread's part of a K-tile: chain kr of the 16, coordinates cl + 16 l of both tiles
  const int kr = tid >> 4, cl = tid & 15;
  double ca[NL], cb[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const long long ci = i0 + cl + 16 * l, cj = j0 + cl + 16 * l;
    ca[l] = (centre && ci < D) ? centre[ci] : 0.0;
    cb[l] = (centre && cj < D) ? centre[cj] : 0.0;
  }
  double ra[NL], rb[NL];
  auto fetch = [&](long long kt) {
    const long long c = kt * SYRK_BK + kr;
    const bool live = c < C;
    const double *row = X + (live ? c : 0) * ldx;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const long long ci = i0 + cl + 16 * l, cj = j0 + cl + 16 * l;
      ra[l] = (live && ci < D) ? row[ci] - ca[l] : 0.0;  // (the zero-filled tail: 0, not -b)
      if (!diag) rb[l] = (live && cj < D) ? row[cj] - cb[l] : 0.0;
    }
  };
  auto stash = [&](int st) {
#pragma unroll
    for (int l = 0; l < NL; l++) {
      img[st][0][kr][cl + 16 * l] = ra[l];
      if (!diag) img[st][1][kr][cl + 16 * l] = rb[l];
    }
  };

  syrk_d4 acc[NI][NI];
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int j = 0; j < NI; j++) acc[i][j] = (syrk_d4){0.0, 0.0, 0.0, 0.0};

  if (kt0 < kt1) {
    fetch(kt0);
    stash(0);
  }
  __syncthreads();
  const int bsel = diag ? 0 : 1;
  for (long long kt = kt0; kt < kt1; kt++) {
    const int st = (int)((kt - kt0) & 1);
    if (kt + 1 < kt1) fetch(kt + 1);
#pragma unroll
    for (int kk = 0; kk < SYRK_BK / 4; kk++) {
      double a[NI], b[NI];
#pragma unroll
      for (int i = 0; i < NI; i++) a[i] = img[st][0][kk * 4 + fk][wm * HALF + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < NI; j++) b[j] = img[st][bsel][kk * 4 + fk][wn * HALF + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < NI; i++)
#pragma unroll
        for (int j = 0; j < NI; j++)
          if (!diag || wn * NI + j <= wm * NI + i)  // (wave-uniform: 16 x 16 blocks above the diagonal are skipped)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < kt1) stash(st ^ 1);
    __syncthreads();
  }

  // C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  if (partial) {
    const long long tiles = (long long)gridDim.x;
    double *out = partial + ((long long)blockIdx.y * tiles + blockIdx.x) * (BM * BM);
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
      for (int j = 0; j < NI; j++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          out[(wm * HALF + i * 16 + fk + 4 * r) * BM + wn * HALF + j * 16 + fr] = acc[i][j][r];
    return;
  }
  const double ww = w_dev ? *w_dev : w;
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const long long col = j0 + wn * HALF + j * 16 + fr;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long long row = i0 + wm * HALF + i * 16 + fk + 4 * r;
        if (row < D && col <= row) {
          double s = S[row * lds_ + col] + acc[i][j][r];
          if (delta) s = s + (ww * delta[row]) * delta[col];
          S[row * lds_ + col] = s;
        }
      }
    }
}

// the parts of a split product, added in ascending order behind S; then the rank-one term
template <int BM>
__global__ __launch_bounds__(256) void syrk_reduce_kernel(long long D, int parts, const double *__restrict__ partial, double w,
                                                          const double *__restrict__ w_dev,
                                                          const double *__restrict__ delta, double *__restrict__ S,
                                                          long long lds_) {
  int ti, tj;
  syrk_tile_of(blockIdx.x, ti, tj);
  const int e = blockIdx.y * 256 + threadIdx.x;
  const long long row = (long long)ti * BM + e / BM, col = (long long)tj * BM + e % BM;
  if (row >= D || col > row) return;
  const long long tiles = (long long)gridDim.x;
  double s = S[row * lds_ + col];
  for (int p = 0; p < parts; p++) s = s + partial[((long long)p * tiles + blockIdx.x) * (BM * BM) + e];
  const double ww = w_dev ? *w_dev : w;
  if (delta) s = s + (ww * delta[row]) * delta[col];
  S[row * lds_ + col] = s;
}

template <int BM>
inline hipError_t syrk_launch_bm(const SyrkPlan &p, long long C, long long D, const double *X, long long ldx,
                                 const double *centre, double w, const double *w_dev, const double *delta, double *S,
                                 long long lds_, double *partial, hipStream_t st) {
  const dim3 grid((unsigned)p.tiles, (unsigned)p.parts);
  hipLaunchKernelGGL((syrk_tn_f64_kernel<BM>), grid, dim3(256), 0, st, C, D, X, ldx, centre, w, w_dev, delta, S, lds_,
                     p.kt_per, p.parts > 1 ? partial : (double *)nullptr);
  if (p.parts > 1)
    hipLaunchKernelGGL((syrk_reduce_kernel<BM>), dim3((unsigned)p.tiles, (unsigned)(BM * BM / 256)), dim3(256), 0, st, D,
                       p.parts, (const double *)partial, w, w_dev, delta, S, lds_);
  return hipGetLastError();
}

// `partial`: syrk_partial_doubles(C, D) doubles of scratch (may be null when that is 0).  `w_dev` (device, optional)
// overrides `w`; `centre` and `delta` may be null
inline hipError_t launch_syrk_tn(long long C, long long D, const double *X, long long ldx, const double *centre, double w,
                                 const double *w_dev, const double *delta, double *S, long long lds_, double *partial,
                                 hipStream_t st) {
  const SyrkPlan p = syrk_plan(C, D);
  if (p.parts > 1 && !partial) return hipErrorInvalidValue;
  if (p.bm == 32) return syrk_launch_bm<32>(p, C, D, X, ldx, centre, w, w_dev, delta, S, lds_, partial, st);
  if (p.bm == 64) return syrk_launch_bm<64>(p, C, D, X, ldx, centre, w, w_dev, delta, S, lds_, partial, st);
  return syrk_launch_bm<128>(p, C, D, X, ldx, centre, w, w_dev, delta, S, lds_, partial, st);
}

}  // namespace aehmc
