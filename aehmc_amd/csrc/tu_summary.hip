// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "summary.cuh"

namespace aehmc {
namespace tu {
hipError_t summary_update(const double *x, long long T, long long E, long long t0, long long N, int S, double *mean,
                          double *m2, hipStream_t st) {
  return launch_summary_update(x, T, E, t0, N, S, mean, m2, st);
}
hipError_t summary_acov(const double *x, const double *mean, double *partial, double *acov, long long N, long long C,
                        long long D, int S, long long K, int G, hipStream_t st) {
  return launch_summary_acov(x, mean, partial, acov, N, C, D, S, K, G, st);
}
hipError_t summary_final(const double *mean, const double *m2, const double *acov, double *out, int *lag_truncated,
                         long long n, long long m, long long D, long long K, hipStream_t st) {
  return launch_summary_final(mean, m2, acov, out, lag_truncated, n, m, D, K, st);
}
hipError_t summary_lag_update(const double *x, long long T, long long C, long long D, long long t0, long long N, int S,
                              long long K, int CG, double *shift, double *sums, double *ring, double *head,
                              double *prod, double *acov, hipStream_t st) {
  return launch_summary_lag_update(x, T, C, D, t0, N, S, K, CG, shift, sums, ring, head, prod, acov, st);
}
int summary_lag_group(long long K) { return aehmc::summary_lag_group(K); }
}  // namespace tu
}  // namespace aehmc
