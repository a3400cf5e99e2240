// Constrained draws from unconstrained positions (aehmc_constrain; aehmc_amd/transforms.py): one pass,
// x [R][D_in] -> y [R][D_out], both fp64, OUT OF PLACE -- the two buffers must not overlap (an Ordered or Simplex entry
// reads up to 64 inputs that other threads' outputs would overwrite); the C-ABI entry refuses buffers that do.
//
// Table.  One ConstrainEntry per OUTPUT coordinate, built once per model on the host and kept on the device:
//   kind           CONSTRAIN_REAL ... CONSTRAIN_SIMPLEX
//   pos, len       the entry's position in its segment and the segment's length in OUTPUT coordinates (a coordinate-wise
//                  kind: 0 and 1; Ordered(n): j and n; Simplex(K): j and K, fed by K - 1 inputs)
//   first          the index of the segment's first INPUT coordinate (a coordinate-wise kind: the entry's own input)
//   lo, hi         the bounds (unused ones are 0)
// An entry whose segment does not lie inside the row (first < 0, first + inputs > D_in, pos >= len, len > 64, an unknown
// kind) writes NaN and reads nothing.
//
// Formulas, in this operation order (every operation rounded on its own: the library is built with -ffp-contract=off):
//   Real        y = x
//   LowerBound  y = lo + exp(x)
//   UpperBound  y = hi - exp(x)
//   Interval    s = 1 / (1 + exp(-x)) where x >= 0, else e / (1 + e) with e = exp(x);  y = lo + (hi - lo) * s;
//               y = hi where s == 1 or y > hi (lo + (hi - lo) need not round to hi)
//   Ordered     t = x_0;  t = t + exp(x_j), j = 1 ... pos, ascending;  y = t
//   Simplex     xt = (x_0 ... x_{K-2}, 0);  m = xt_0, m = xt_j where xt_j > m, j ascending;
//               tot = exp(xt_0 - m), tot = tot + exp(xt_j - m), j = 1 ... K - 1 ascending;  L = m + log(tot);
//               y = exp(xt_pos - L)
// Edges.  NaN in gives NaN out (Ordered: from the NaN's entry on; Simplex: the whole segment).  Interval saturates to
// exactly lo (exp(x) underflows to 0: s = 0) and exactly hi (s = 1) for large |x| and never forms a NaN from a finite x.
// exp overflow gives +inf in LowerBound and Ordered, -inf in UpperBound.  A Simplex with +inf among its inputs gives NaN
// (inf - inf), with -inf a zero weight.
//
// Shape.  A workgroup of 256 threads is a tile of tw output coordinates (a power of two, 256 or the smallest that holds
// D_out, at least 16) times 256 / tw rows; a thread serves one output coordinate of CONSTRAIN_ROWS rows, 256 / tw apart.
// The lanes of a row read and write contiguous memory, the entry is read once per thread, and a segment walk reads at most
// 64 contiguous doubles that its neighbours read too (L1 / L2).  Every output is computed by one thread from its inputs
// alone, in the order above: the result depends neither on the launch geometry nor on how the rows are cut into calls.
// Row indices are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {

constexpr int CONSTRAIN_THREADS = 256;
constexpr int CONSTRAIN_ROWS = 8;      // rows per thread (more when the row blocks would exceed the grid's y limit)
constexpr int CONSTRAIN_MAX_LEN = 64;  // the longest Ordered / Simplex segment (the tracer's limit on written-out sums)

enum ConstrainKind : int32_t {
  CONSTRAIN_REAL = 0, CONSTRAIN_LOWER = 1, CONSTRAIN_UPPER = 2, CONSTRAIN_INTERVAL = 3, CONSTRAIN_ORDERED = 4,
  CONSTRAIN_SIMPLEX = 5
};

struct ConstrainEntry {  // 40 bytes, the layout aehmc_hip.h states (aehmc_constrain_entry)
  int32_t kind, pos, len, reserved;
  int64_t first;
  double lo, hi;
};

struct ConstrainArgs {
  const double *x;            // [R][D_in]
  double *y;                  // [R][D_out]
  const ConstrainEntry *tab;  // [D_out]
  long long R, D_in, D_out, rows_per_block;
  int tw_log2;  // the tile is 1 << tw_log2 coordinates wide
};

__device__ inline double constrain_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ inline double constrain_interval(double x, double lo, double hi) {
  double s;
  if (x >= 0.0) {
    s = 1.0 / (1.0 + exp(-x));
  } else {
    const double e = exp(x);
    s = e / (1.0 + e);
  }
  double y = lo + (hi - lo) * s;
  if (s == 1.0 || y > hi) y = hi;
  return y;
}

__device__ inline double constrain_ordered(const double *seg, int pos) {
  double t = seg[0];
  for (int j = 1; j <= pos; ++j) t = t + exp(seg[j]);
  return t;
}

__device__ inline double constrain_simplex(const double *seg, int pos, int K) {
  double m = K > 1 ? seg[0] : 0.0;
  for (int j = 1; j < K; ++j) {
    const double v = j < K - 1 ? seg[j] : 0.0;
    m = v > m ? v : m;
  }
  double tot = exp((K > 1 ? seg[0] : 0.0) - m);
  for (int j = 1; j < K; ++j) tot = tot + exp((j < K - 1 ? seg[j] : 0.0) - m);
  const double L = m + log(tot);
  return exp((pos < K - 1 ? seg[pos] : 0.0) - L);
}

__global__ __launch_bounds__(CONSTRAIN_THREADS) void k_constrain(ConstrainArgs a) {
  const int tid = threadIdx.x, tw = 1 << a.tw_log2;
  const long long step = CONSTRAIN_THREADS >> a.tw_log2;  // rows the workgroup serves at a time
  const long long d = (long long)blockIdx.x * tw + (tid & (tw - 1));
  if (d >= a.D_out) return;
  const ConstrainEntry e = a.tab[d];
  const long long r0 = (long long)blockIdx.y * a.rows_per_block + (tid >> a.tw_log2);
  const long long rend = (long long)blockIdx.y * a.rows_per_block + a.rows_per_block;
  const long long r1 = rend < a.R ? rend : a.R;
  const long long inputs = e.kind == CONSTRAIN_SIMPLEX ? (long long)e.len - 1 : e.kind == CONSTRAIN_ORDERED ? e.len : 1;
  const bool good = e.kind >= CONSTRAIN_REAL && e.kind <= CONSTRAIN_SIMPLEX && e.len >= 1 && e.len <= CONSTRAIN_MAX_LEN &&
                    e.pos >= 0 && e.pos < e.len && e.first >= 0 && e.first + inputs <= a.D_in &&
                    (e.kind >= CONSTRAIN_ORDERED || (e.len == 1 && e.pos == 0)) && (e.kind != CONSTRAIN_SIMPLEX || e.len >= 2);
  if (!good) {
    for (long long r = r0; r < r1; r += step) a.y[r * a.D_out + d] = constrain_nan();
    return;
  }
  const double *src = a.x + e.first;
  double *dst = a.y + d;
  switch (e.kind) {
    case CONSTRAIN_REAL:
      for (long long r = r0; r < r1; r += step) dst[r * a.D_out] = src[r * a.D_in];
      break;
    case CONSTRAIN_LOWER:
      for (long long r = r0; r < r1; r += step) dst[r * a.D_out] = e.lo + exp(src[r * a.D_in]);
      break;
    case CONSTRAIN_UPPER:
      for (long long r = r0; r < r1; r += step) dst[r * a.D_out] = e.hi - exp(src[r * a.D_in]);
      break;
    case CONSTRAIN_INTERVAL:
      for (long long r = r0; r < r1; r += step) dst[r * a.D_out] = constrain_interval(src[r * a.D_in], e.lo, e.hi);
      break;
    case CONSTRAIN_ORDERED:
      for (long long r = r0; r < r1; r += step) dst[r * a.D_out] = constrain_ordered(src + r * a.D_in, e.pos);
      break;
    default:
      for (long long r = r0; r < r1; r += step) dst[r * a.D_out] = constrain_simplex(src + r * a.D_in, e.pos, e.len);
      break;
  }
}

inline hipError_t launch_constrain(const double *x, long long R, long long D_in, long long D_out, const void *table,
                                   double *y, hipStream_t st) {
  int twl = 8;
  while (twl > 4 && (1LL << (twl - 1)) >= D_out) --twl;
  const long long tw = 1LL << twl;
  long long rows = (long long)CONSTRAIN_ROWS * (CONSTRAIN_THREADS >> twl);
  if ((R + rows - 1) / rows > 65535) rows = (R + 65534) / 65535;
  ConstrainArgs a;
  a.x = x; a.y = y; a.tab = static_cast<const ConstrainEntry *>(table);
  a.R = R; a.D_in = D_in; a.D_out = D_out; a.rows_per_block = rows; a.tw_log2 = twl;
  const long long bx = (D_out + tw - 1) / tw, by = (R + rows - 1) / rows;
  hipLaunchKernelGGL(k_constrain, dim3((unsigned)bx, (unsigned)by), dim3(CONSTRAIN_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace aehmc
