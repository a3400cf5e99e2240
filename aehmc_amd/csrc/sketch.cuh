// Streaming quantiles of draws that are not stored (aehmc_summary_sketch_update / _sketch_quantiles):
// a fixed-grid histogram per coordinate, folded chunk by chunk next to the running moments of summary.cuh.
//
// Grid.  Coordinate d has lo[d], width[d] = (hi[d] - lo[d]) / B and inv[d] = 1 / width[d], computed ONCE by the caller
// in fp64 and handed over as [D] device arrays; the kernels never recompute them.  B is a power of two in
// [SKETCH_MIN_BINS, SKETCH_MAX_BINS].  A coordinate has B + 3 counters: slot 0 below the grid, slots 1 ... B interior,
// slot B + 1 above the grid, slot B + 2 NaN.
//
// Binning.  t = (x - lo) * inv, two separately rounded fp64 operations (nothing to contract); NaN t -> B + 2, t < 0 -> 0,
// t >= B -> B + 1, else 1 + (long long)t.  -inf and +inf need no special case, -0.0 at lo = 0 gives t = -0.0 and slot 1.
// The map is monotone in x, so the slot boundaries partition the line and the slot of the k-th order statistic is the
// slot in which the cumulative count passes k.
//
// Counters.  Global counters are 64-bit (a streaming run may pool more than 2^32 draws); a workgroup counts in 32-bit
// LDS words (one call takes fewer than 2^31 rows) and adds every non-empty one to its global counter once.  Integer
// additions only: the result depends neither on chunking, nor on the launch geometry, nor on the order of arrival.
//
// Shape, after k_quantile_hist (quantile.cuh).  A tile is SKETCH_TILE = 16 consecutive coordinates (128 contiguous bytes
// per row), 8 at B = 4096, narrower (a power of two) when D is smaller.  A counter row in LDS is B + 3 words, which is
// odd: the coordinates of a tile at one slot fall into different banks without further padding.  16 * 2051 * 4 B =
// 131 264 B, 8 * 4099 * 4 B = 131 168 B of the CU's 160 KiB: one workgroup per CU at the large grids.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {

constexpr int SKETCH_THREADS = 256;
constexpr int SKETCH_TILE = 16;       // coordinates per workgroup (8 at SKETCH_MAX_BINS; narrower when D is smaller)
constexpr int SKETCH_INFLIGHT = 4;    // rows a lane loads before it counts the first of them
constexpr int SKETCH_MIN_BINS = 64;
constexpr int SKETCH_MAX_BINS = 4096;
constexpr int SKETCH_LDS_WORDS = 16 * (2048 + 3);  // the largest tile: 131 264 B (8 * 4099 words at 4096 bins are fewer)
constexpr int SKETCH_MAX_PROBS = 64;               // probabilities of one quantiles call (QUANTILE_MAX)
constexpr int SKETCH_MAX_RANKS = 2 * SKETCH_MAX_PROBS;

__host__ __device__ inline int sketch_slots(int B) { return B + 3; }

// log2 of the tile width: 16 coordinates (8 at 4096 bins), or the power of two that holds D
inline int sketch_tile_log2(long long D, int B) {
  int twl = B > 2048 ? 3 : 4;
  while (twl > 0 && (1LL << (twl - 1)) >= D) --twl;
  return twl;
}

__device__ inline int sketch_slot(double x, double lo, double inv, int B) {
  const double t = (x - lo) * inv;
  if (t != t) return B + 2;
  if (t < 0.0) return 0;
  if (t >= (double)B) return B + 1;
  return 1 + (int)(long long)t;
}

struct SketchUpdateArgs {
  const double *x;             // [R][D]
  const double *lo, *inv;      // [D]
  unsigned long long *counts;  // [D][B + 3]
  long long R, D, rows_per_chunk;
  int B, tw_log2;
};

// Workgroup (x: tile of coordinates, y: chunk of rows).  Lane (c, rl) walks the rows rl, rl + 256 / tw, ... of its chunk
// at coordinate c: the tw lanes of a row read one contiguous row segment, and a lane keeps lo and inv of its coordinate
// in registers.
__global__ __launch_bounds__(SKETCH_THREADS) void k_sketch_update(SketchUpdateArgs a) {
  extern __shared__ unsigned s_cnt[];  // [tw][B + 3]
  const int tid = threadIdx.x, tw = 1 << a.tw_log2, c = tid & (tw - 1), rl = tid >> a.tw_log2;
  const int rpi = SKETCH_THREADS >> a.tw_log2;  // rows per step of the workgroup
  const int stride = sketch_slots(a.B), words = tw * stride;
  const long long d = (long long)blockIdx.x * tw + c;
  const bool live = d < a.D;
  for (int i = tid; i < words; i += SKETCH_THREADS) s_cnt[i] = 0;
  const double lo = live ? a.lo[d] : 0.0, inv = live ? a.inv[d] : 0.0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.y * a.rows_per_chunk;
  const long long r1 = r0 + a.rows_per_chunk < a.R ? r0 + a.rows_per_chunk : a.R;
  if (live) {
    unsigned *mine = s_cnt + c * stride;
    for (long long row = r0 + rl; row < r1; row += (long long)rpi * SKETCH_INFLIGHT) {
      double v[SKETCH_INFLIGHT];
#pragma unroll
      for (int j = 0; j < SKETCH_INFLIGHT; ++j) {
        const long long rr = row + (long long)j * rpi;
        v[j] = rr < r1 ? a.x[rr * a.D + d] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < SKETCH_INFLIGHT; ++j) {
        if (row + (long long)j * rpi >= r1) break;
        atomicAdd(&mine[sketch_slot(v[j], lo, inv, a.B)], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < words; i += SKETCH_THREADS) {
    const unsigned n = s_cnt[i];
    if (!n) continue;
    const int cc = i / stride, slot = i - cc * stride;
    const long long dd = (long long)blockIdx.x * tw + cc;
    if (dd < a.D) atomicAdd(&a.counts[dd * stride + slot], (unsigned long long)n);
  }
}

struct SketchQuantileArgs {
  const unsigned long long *counts;  // [D][B + 3]
  const double *lo, *width;          // [D]
  double *estimate;                  // [Q][D]
  int *resolved;                     // [Q][D]
  long long D;
  int B, Q, U;                                           // U distinct ranks, ascending
  unsigned long long rank[SKETCH_MAX_RANKS];             // each below the total count
  unsigned char lo_row[SKETCH_MAX_PROBS], hi_row[SKETCH_MAX_PROBS];  // rows of rank[] behind a probability
  double g[SKETCH_MAX_PROBS];
};

// One workgroup per coordinate.  Lane i owns the slots i * per ... (i + 1) * per - 1 of 0 ... B + 1: it sums them, an
// inclusive scan of the 256 sums gives the count below its first slot, and it walks its slots once more to place the
// ranks that fall among them: rank r lies in the slot j with cum[j-1] <= r < cum[j], at
//   pos(r) = lo + width * ((j - 1) + (r - cum[j-1] + 0.5) / count[j]).
// estimate = pos(k) + g (pos(k1) - pos(k)); NaN where the coordinate holds a NaN; resolved where both slots are interior
// and there is no NaN.  A rank that no slot holds (the NaN draws are part of the total) leaves its NaN.
__global__ __launch_bounds__(SKETCH_THREADS) void k_sketch_quantiles(SketchQuantileArgs a) {
  __shared__ unsigned long long s_scan[2][SKETCH_THREADS];
  __shared__ double s_pos[SKETCH_MAX_RANKS];
  __shared__ int s_inner[SKETCH_MAX_RANKS];
  const long long d = blockIdx.x;
  const int tid = threadIdx.x, stride = sketch_slots(a.B), n = a.B + 2;
  const int per = (n + SKETCH_THREADS - 1) / SKETCH_THREADS, j0 = tid * per, j1 = j0 + per < n ? j0 + per : n;
  const unsigned long long *cnt = a.counts + d * stride;
  if (tid < a.U) {
    s_pos[tid] = __longlong_as_double(0x7ff8000000000000LL);
    s_inner[tid] = 0;
  }
  unsigned long long sum = 0;
  for (int j = j0; j < j1; ++j) sum += cnt[j];
  int cur = 0;
  s_scan[0][tid] = sum;
  __syncthreads();
  for (int off = 1; off < SKETCH_THREADS; off <<= 1) {
    const unsigned long long v = s_scan[cur][tid] + (tid >= off ? s_scan[cur][tid - off] : 0ULL);
    s_scan[cur ^ 1][tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  const unsigned long long incl = s_scan[cur][tid];
  unsigned long long below = incl - sum;
  const double lo = a.lo[d], width = a.width[d];
  if (sum) {
    int u = 0;
    while (u < a.U && a.rank[u] < below) ++u;  // (the ranks ascend)
    for (int j = j0; j < j1 && u < a.U && a.rank[u] < incl; ++j) {
      const unsigned long long cj = cnt[j];
      for (; u < a.U && a.rank[u] < below + cj; ++u) {
        const double inside = ((double)(a.rank[u] - below) + 0.5) / (double)cj;
        s_pos[u] = lo + width * ((double)(j - 1) + inside);
        s_inner[u] = j >= 1 && j <= a.B;
      }
      below += cj;
    }
  }
  __syncthreads();
  const bool has_nan = cnt[a.B + 2] != 0;
  for (int q = tid; q < a.Q; q += SKETCH_THREADS) {
    const int k = a.lo_row[q], k1 = a.hi_row[q];
    const double pk = s_pos[k], est = pk + a.g[q] * (s_pos[k1] - pk);
    a.estimate[(long long)q * a.D + d] = has_nan ? __longlong_as_double(0x7ff8000000000000LL) : est;
    a.resolved[(long long)q * a.D + d] = !has_nan && s_inner[k] && s_inner[k1];
  }
}

// x [R][D] into counts [D][B + 3].  Rows are split over several workgroups per tile so that few coordinates still fill
// the GPU: about 1024 workgroups in all, but a workgroup keeps at least as many steps as zeroing and flushing its
// counters take (two LDS sweeps of words / 256 steps each), and never fewer than 16 -- a chunk at the headline shape
// is only 3 draws * 4096 chains.
inline hipError_t launch_sketch_update(const double *x, long long R, long long D, int B, const double *lo,
                                       const double *inv, unsigned long long *counts, hipStream_t st) {
  const int twl = sketch_tile_log2(D, B), tw = 1 << twl, rpi = SKETCH_THREADS / tw;
  const long long tiles = (D + tw - 1) / tw;
  const int words = tw * sketch_slots(B);
  long long steps = 2LL * ((words + SKETCH_THREADS - 1) / SKETCH_THREADS);
  if (steps < 16) steps = 16;
  long long chunks = (1024 + tiles - 1) / tiles;
  const long long most = (R + steps * rpi - 1) / (steps * rpi);
  if (chunks > most) chunks = most;
  if (chunks > 65535) chunks = 65535;
  const long long rows_per_chunk = (R + chunks - 1) / chunks;
  chunks = (R + rows_per_chunk - 1) / rows_per_chunk;
  // up to 131 264 B of dynamic LDS; asked for on every call (no state shared between threads or devices)
  if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sketch_update),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(SKETCH_LDS_WORDS * sizeof(unsigned)));
      e != hipSuccess)
    return e;
  SketchUpdateArgs a;
  a.x = x; a.lo = lo; a.inv = inv; a.counts = counts;
  a.R = R; a.D = D; a.rows_per_chunk = rows_per_chunk;
  a.B = B; a.tw_log2 = twl;
  hipLaunchKernelGGL(k_sketch_update, dim3((unsigned)tiles, (unsigned)chunks), dim3(SKETCH_THREADS),
                     (size_t)words * sizeof(unsigned), st, a);
  return hipGetLastError();
}

inline hipError_t launch_sketch_quantiles(const SketchQuantileArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_sketch_quantiles, dim3((unsigned)a.D), dim3(SKETCH_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
