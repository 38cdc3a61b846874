// One translation unit of the product library (csrc/Makefile): the int8 classifier head and QUANTIZE / DEQUANTIZE
// (lce_kernels_head_i8.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_head_i8.h"

namespace lce {
int launch_fully_connected_i8(const FcI8Args& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per 16 x 16 tile, four to a block, grid-strided past ~8 blocks per CU
  const dim3 grid(fc_i8_grid(args));
  if (vec) fully_connected_i8<true><<<grid, 256, 0, st>>>(args);
  else fully_connected_i8<false><<<grid, 256, 0, st>>>(args);
  return (int)hipGetLastError();
}

int launch_mean_i8(const MeanI8Args& args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per image and 16 channels, four to a block, grid-strided past ~8 blocks per CU
  mean_i8<4><<<dim3(stream_grid(args.batch * args.segs)), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}

int launch_softmax_i8(const SoftmaxI8Args& args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // one wave per row, four to a block, grid-strided past ~8 blocks per CU
  softmax_i8<4><<<dim3(stream_grid(args.rows)), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}

// one element per lane and step (n > 0), grid-strided past ~8 blocks per CU
int launch_quantize_f32_i8(const QuantArgs& args, void* stream) {
  quant_i8<true><<<dim3(stream_grid(args.n, 256)), 256, 0, (hipStream_t)stream>>>(args);
  return (int)hipGetLastError();
}

int launch_dequantize_i8_f32(const QuantArgs& args, void* stream) {
  quant_i8<false><<<dim3(stream_grid(args.n, 256)), 256, 0, (hipStream_t)stream>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
