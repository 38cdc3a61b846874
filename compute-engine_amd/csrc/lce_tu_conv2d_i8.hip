// One translation unit of the product library (csrc/Makefile): the int8 CONV_2D (lce_kernels_conv2d_i8.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_conv2d_i8.h"

namespace lce {
int launch_conv2d_i8(const ConvI8Args& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // 128-pixel tiles, grid-strided past ~8 blocks per CU; grid.y: the 128-channel slices
  unsigned gx = 0, gy = 0;
  conv2d_i8_grid(args, 256u * 8u, &gx, &gy);
  const dim3 grid(gx, gy);
  if (vec) conv2d_i8<true><<<grid, 256, 0, st>>>(args);
  else conv2d_i8<false><<<grid, 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
