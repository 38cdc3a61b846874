// One translation unit of the product library (csrc/Makefile): the float KxK CONV_2D (lce_kernels_conv2d.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_conv2d.h"

namespace lce {
int launch_conv2d(const Conv2dArgs& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (args.Mi > 0) {
    // 128-pixel tiles, grid-strided past ~8 blocks per CU; grid.y: the 128-channel slices
    unsigned gx = 0, gy = 0;
    conv2d_grid(args, 256u * 8u, &gx, &gy);
    const dim3 grid(gx, gy);
    if (vec) conv2d_interior<true><<<grid, 256, 0, st>>>(args);
    else conv2d_interior<false><<<grid, 256, 0, st>>>(args);
    const int e = (int)hipGetLastError();
    if (e != (int)hipSuccess) return e;
  }
  if (args.Mb > 0) {
    // one wave per (border pixel, 64 channels), 4 per block, grid-strided past ~8 blocks per CU
    const unsigned grid = conv2d_border_grid(args);
    if (args.bits) conv2d_border<true><<<grid, 256, 0, st>>>(args);
    else conv2d_border<false><<<grid, 256, 0, st>>>(args);
    return (int)hipGetLastError();
  }
  return (int)hipSuccess;
}
}  // namespace lce
