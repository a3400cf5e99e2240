// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#define AEHMC_POINTWISE_TU 1
#include "pointwise.cuh"

namespace aehmc {
namespace tu {
hipError_t waic_fold_stored(const double *x, long long R, long long n_obs, double *ws, hipStream_t st) {
  return launch_waic_fold_stored(x, R, n_obs, ws, st);
}
hipError_t waic_merge(const double *ws, long long parts, long long part_rows, long long R, double *state, double n_state,
                      long long n_obs, hipStream_t st) {
  return launch_waic_merge(ws, parts, part_rows, R, state, n_state, n_obs, st);
}
hipError_t waic_final(const double *state, double n_state, long long n_obs, double *lppd, double *p, hipStream_t st) {
  return launch_waic_final(state, n_state, n_obs, lppd, p, st);
}
}  // namespace tu
}  // namespace aehmc
