// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "../../include/aehmc_hip.h"
#include "tu.h"
#include "sketch.cuh"

namespace aehmc {
namespace tu {
static_assert(SKETCH_MAX_PROBS == AEHMC_SUMMARY_QUANTILE_MAX, "the header states the limit of sketch.cuh");
static_assert(SKETCH_MIN_BINS == AEHMC_SUMMARY_SKETCH_MIN_BINS && SKETCH_MAX_BINS == AEHMC_SUMMARY_SKETCH_MAX_BINS,
              "the header states the grids of sketch.cuh");
hipError_t sketch_update(const double *x, long long R, long long D, int B, const double *lo, const double *inv,
                         unsigned long long *counts, hipStream_t st) {
  return launch_sketch_update(x, R, D, B, lo, inv, counts, st);
}
hipError_t sketch_quantiles(const unsigned long long *counts, const double *lo, const double *width, long long D, int B,
                            int Q, int U, const long long *ranks, const int *lo_row, const int *hi_row, const double *g,
                            double *estimate, int *resolved, hipStream_t st) {
  SketchQuantileArgs a;
  a.counts = counts; a.lo = lo; a.width = width; a.estimate = estimate; a.resolved = resolved;
  a.D = D; a.B = B; a.Q = Q; a.U = U;
  for (int i = 0; i < SKETCH_MAX_RANKS; ++i) a.rank[i] = i < U ? (unsigned long long)ranks[i] : 0ULL;
  for (int i = 0; i < SKETCH_MAX_PROBS; ++i) {
    a.lo_row[i] = (unsigned char)(i < Q ? lo_row[i] : 0);
    a.hi_row[i] = (unsigned char)(i < Q ? hi_row[i] : 0);
    a.g[i] = i < Q ? g[i] : 0.0;
  }
  return launch_sketch_quantiles(a, st);
}
}  // namespace tu
}  // namespace aehmc
