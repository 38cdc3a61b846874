// One translation unit of the product library (csrc/Makefile): the float 1x1 CONV_2D (lce_kernels_conv1x1.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_conv1x1.h"

namespace lce {
int launch_conv1x1(const Conv1x1Args& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // 128-pixel tiles, grid-strided past ~8 blocks per CU; grid.y: the 128-channel slices
  const uint32_t cap = 256u * 8u;
  const dim3 grid(args.mtiles < cap ? args.mtiles : cap, (args.Cout + kConv1x1BN - 1) / kConv1x1BN);
  if (vec) conv1x1_f32<true><<<grid, 256, 0, st>>>(args);
  else conv1x1_f32<false><<<grid, 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
