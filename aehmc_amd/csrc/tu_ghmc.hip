// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the function below.
#include "tu.h"
#include "ghmc_fused.cuh"

namespace aehmc {
namespace tu {
hipError_t ghmc_fused(const GhmcArgs &a, hipStream_t st) { return launch_ghmc_fused(a, st); }
}  // namespace tu
}  // namespace aehmc
