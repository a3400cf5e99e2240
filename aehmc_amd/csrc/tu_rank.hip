// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "rank.cuh"
#include "posterior.cuh"
#include "psis.cuh"

namespace aehmc {
namespace tu {
size_t rank_work_bytes(long long R, long long T) { return rank_work(nullptr, R, T).bytes; }
long long rank_tile_width(long long R, long long D, size_t bytes) { return rank_tile(R, D, bytes); }
long long rank_default_tile(long long R, long long D) {
  const long long T = rank_tile(R, D, RANK_DEFAULT_WORK);
  return T < 1 ? 1 : T;
}
hipError_t rank(const double *x, const double *centre, long long R, long long D, int mode, double *out, void *work,
                long long T, hipStream_t st) {
  return launch_rank(x, centre, R, D, mode, out, work, T, st);
}
hipError_t hdi(const double *x, long long R, long long D, long long m, double *lower, double *upper, long long *index,
               void *work, long long T, hipStream_t st) {
  return launch_hdi(x, R, D, m, lower, upper, index, work, T, st);
}
hipError_t quantile_mcse(const double *x, long long R, long long D, int Q, const double *probs, const double *ess,
                         double *out, long long *ranks, void *work, long long T, hipStream_t st) {
  return launch_quantile_mcse(x, R, D, Q, probs, ess, out, ranks, work, T, st);
}
hipError_t beta_quantile(long long n, const double *p, const double *a, const double *b, double *out, hipStream_t st) {
  return launch_beta_quantile(n, p, a, b, out, st);
}
hipError_t psis(const double *x, bool neg, const double *reff, const double *v, double *log_weights, double *pareto_k,
                long long *tail_len, double *log_mean, long long R, long long D, void *work, long long T,
                hipStream_t st) {
  return launch_psis(x, neg, reff, v, log_weights, pareto_k, tail_len, log_mean, R, D, work, T, st);
}
}  // namespace tu
}  // namespace aehmc
