// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "nested.cuh"

namespace aehmc {
namespace tu {
hipError_t nested_update(const double *x, long long T, long long C, long long D, long long t0, long long w, long long M,
                         double *mean, double *m2, double *out, hipStream_t st) {
  return launch_nested_update(x, T, C, D, t0, w, M, mean, m2, out, st);
}
long long nested_blocks(long long D) { return aehmc::nested_blocks(D, nullptr); }
}  // namespace tu
}  // namespace aehmc
