// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "../../include/aehmc_hip.h"
#include "tu.h"
#include "quantile.cuh"

namespace aehmc {
namespace tu {
static_assert(QUANTILE_MAX == AEHMC_SUMMARY_QUANTILE_MAX, "the header states the limit of quantile.cuh");
size_t quantile_work_bytes(long long D, long long M) { return quantile_work(nullptr, D, M).bytes; }
hipError_t quantile_stats(const double *x, long long R, long long D, int U, const long long *ranks, void *work,
                          long long M, hipStream_t st) {
  return launch_quantile_stats(x, R, D, U, ranks, quantile_work(work, D, M), st);
}
hipError_t quantile_out(void *work, long long D, long long M, int n, const int *lo, const int *hi, const double *g,
                        double *out, hipStream_t st) {
  QuantileOutArgs a;
  a.stats = quantile_work(work, D, M).stats;
  a.out = out; a.D = D; a.n = n; a.interpolate = g != nullptr;
  for (int i = 0; i < n; ++i) {
    a.lo[i] = (unsigned char)lo[i];
    a.hi[i] = (unsigned char)(g ? hi[i] : lo[i]);
    a.g[i] = g ? g[i] : 0.0;
  }
  return launch_quantile_out(a, st);
}
}  // namespace tu
}  // namespace aehmc
