// One translation unit of the product library (csrc/Makefile): the float classifier head (lce_kernels_head.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_head.h"

namespace lce {
int launch_fully_connected(const FcArgs& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per 16 x 16 tile, four to a block, grid-strided past ~8 blocks per CU
  const uint32_t blocks = (args.tiles + 3u) / 4u, cap = 256u * 8u;
  const dim3 grid(blocks < cap ? blocks : cap);
  if (vec) fully_connected_f32<true><<<grid, 256, 0, st>>>(args);
  else fully_connected_f32<false><<<grid, 256, 0, st>>>(args);
  return (int)hipGetLastError();
}

int launch_softmax(const SoftmaxArgs& args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per row, four to a block, grid-strided past ~8 blocks per CU
  const uint64_t blocks = (args.rows + 3u) / 4u, cap = 256u * 8u;
  softmax_f32<4><<<dim3((uint32_t)(blocks < cap ? blocks : cap)), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
