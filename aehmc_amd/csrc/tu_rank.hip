// One translation unit of libaehmc_hip.so (see tu.h): instantiates the kernels behind the functions below.
#include "tu.h"
#include "rank.cuh"

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
}  // namespace tu
}  // namespace aehmc
