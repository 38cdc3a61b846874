// One translation unit of the product library (csrc/Makefile): the binarized Dense layer (lce_kernels_bfc.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_bfc.h"

namespace lce {
int launch_binary_fully_connected(const BfcArgs& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per 32 x 32 tile, four to a block, grid-strided past ~8 blocks per CU
  const dim3 grid(bfc_grid(args));
  if (vec) binary_fully_connected<true><<<grid, 256, 0, st>>>(args);
  else binary_fully_connected<false><<<grid, 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
