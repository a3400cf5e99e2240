// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "pooled_adapt.cuh"
#include "syrk_f64.cuh"

namespace aehmc {
namespace tu {
hipError_t syrk_tn(long long C, long long D, const double *X, long long ldx, const double *centre, double w,
                   const double *w_dev, const double *delta, double *S, long long lds, double *partial, hipStream_t st) {
  return launch_syrk_tn(C, D, X, ldx, centre, w, w_dev, delta, S, lds, partial, st);
}
size_t syrk_partial_doubles(long long C, long long D) { return aehmc::syrk_partial_doubles(C, D); }
hipError_t pool_init(const PoolArgs &a, double initial_step_size, hipStream_t st) {
  return launch_pool_init(a, initial_step_size, st);
}
hipError_t pool_sums(const PoolArgs &a, hipStream_t st) { return launch_pool_sums(a, st); }
hipError_t pool_imm(const PoolArgs &a, hipStream_t st) { return launch_pool_imm(a, st); }
hipError_t pool_scalars(const PoolArgs &a, hipStream_t st) { return launch_pool_scalars(a, st); }
}  // namespace tu
}  // namespace aehmc
