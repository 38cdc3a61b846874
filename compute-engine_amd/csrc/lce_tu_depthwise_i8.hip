// One translation unit of the product library (csrc/Makefile): the int8 DEPTHWISE_CONV_2D (lce_kernels_depthwise_i8.h).
// Four kernels: depthwise_i8_vec and depthwise_i8_rows, each with and without the bit output.
#include <hip/hip_runtime.h>
#include "lce_kernels_depthwise_i8.h"

namespace lce {
int launch_depthwise_i8(const DepthwiseI8Args& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // the pools' grid: 4 waves per block, capped, grid-strided past the cap.  pool_vec_grid() counts 64 chunks per wave task;
  // a wave task of the row path is one 64-channel segment
  if (!vec && args.P.bits) depthwise_i8_rows<true><<<pool_vec_grid(args.P.total * 64ull), 256, 0, st>>>(args);
  else if (!vec) depthwise_i8_rows<false><<<pool_vec_grid(args.P.total * 64ull), 256, 0, st>>>(args);
  else if (args.P.bits) depthwise_i8_vec<true><<<pool_vec_grid(args.P.total), 256, 0, st>>>(args);
  else depthwise_i8_vec<false><<<pool_vec_grid(args.P.total), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
