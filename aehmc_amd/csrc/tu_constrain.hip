// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernel behind the function below.
#include "../../include/aehmc_hip.h"
#include "tu.h"
#include "constrain.cuh"
#include <stddef.h>

namespace aehmc {
namespace tu {
static_assert(CONSTRAIN_MAX_LEN == AEHMC_CONSTRAIN_MAX_LEN, "the header states the limit of constrain.cuh");
static_assert(CONSTRAIN_REAL == AEHMC_CONSTRAIN_REAL && CONSTRAIN_LOWER == AEHMC_CONSTRAIN_LOWER &&
                  CONSTRAIN_UPPER == AEHMC_CONSTRAIN_UPPER && CONSTRAIN_INTERVAL == AEHMC_CONSTRAIN_INTERVAL &&
                  CONSTRAIN_ORDERED == AEHMC_CONSTRAIN_ORDERED && CONSTRAIN_SIMPLEX == AEHMC_CONSTRAIN_SIMPLEX,
              "the header states the kinds of constrain.cuh");
static_assert(sizeof(ConstrainEntry) == sizeof(aehmc_constrain_entry) && sizeof(ConstrainEntry) == 40 &&
                  offsetof(ConstrainEntry, first) == offsetof(aehmc_constrain_entry, first) &&
                  offsetof(ConstrainEntry, lo) == offsetof(aehmc_constrain_entry, lo) &&
                  offsetof(ConstrainEntry, hi) == offsetof(aehmc_constrain_entry, hi),
              "the header states the table entry of constrain.cuh");
hipError_t constrain(const double *x, long long R, long long D_in, long long D_out, const void *table, double *y,
                     hipStream_t st) {
  return launch_constrain(x, R, D_in, D_out, table, y, st);
}
}  // namespace tu
}  // namespace aehmc
