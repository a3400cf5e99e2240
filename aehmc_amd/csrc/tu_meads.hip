// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "meads.cuh"

namespace aehmc {
namespace tu {
hipError_t meads_set3(double *cell, double x, double y, double z, hipStream_t st) { return launch_meads_set3(cell, x, y, z, st); }
hipError_t meads_means(const MeadsArgs &a, hipStream_t st) { return launch_meads_means(a, st); }
hipError_t meads_finish(const MeadsArgs &a, hipStream_t st) { return launch_meads_finish(a, st); }
}  // namespace tu
}  // namespace aehmc
