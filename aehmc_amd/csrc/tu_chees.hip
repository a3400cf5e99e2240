// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "chees.cuh"

namespace aehmc {
namespace tu {
hipError_t chees_init(const CheesArgs &a, double initial_step_size, double initial_trajectory_length, hipStream_t st) {
  return launch_chees_init(a, initial_step_size, initial_trajectory_length, st);
}
hipError_t chees_update(const CheesArgs &a, hipStream_t st) { return launch_chees_update(a, st); }
}  // namespace tu
}  // namespace aehmc
