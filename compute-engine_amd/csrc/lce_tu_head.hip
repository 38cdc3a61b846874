// One translation unit of the product library (csrc/Makefile): the float classifier head (lce_kernels_head.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_head.h"

namespace lce {
int launch_fully_connected(const FcArgs& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per 16 x 16 tile, four to a block, grid-strided past ~8 blocks per CU
  const dim3 grid(fc_grid(args));
  if (vec) fully_connected_f32<true><<<grid, 256, 0, st>>>(args);
  else fully_connected_f32<false><<<grid, 256, 0, st>>>(args);
  return (int)hipGetLastError();
}

int launch_softmax(const SoftmaxArgs& args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per row, four to a block, grid-strided past ~8 blocks per CU
  softmax_f32<4><<<dim3(stream_grid(args.rows)), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
