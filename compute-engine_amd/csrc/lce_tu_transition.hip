// One translation unit of the product library (csrc/Makefile): a transition's MAX_POOL_2D and DEPTHWISE_CONV_2D in one launch
// (lce_kernels_transition.h).  Eight kernels: transition_vec / transition_rows and transition_i8_vec / transition_i8_rows, each
// with and without the bit output.
#include <hip/hip_runtime.h>
#include "lce_kernels_transition.h"

namespace lce {
// the pools' grid: 4 waves per block, capped, grid-strided past the cap.  pool_vec_grid() counts 64 chunks per wave task; a wave
// task of the row path is one 64-channel segment
int launch_transition(const TransitionArgs& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const PoolArgs& P = args.D.P;
  if (!vec && P.bits) transition_rows<true><<<pool_vec_grid(P.total * 64ull), 256, 0, st>>>(args);
  else if (!vec) transition_rows<false><<<pool_vec_grid(P.total * 64ull), 256, 0, st>>>(args);
  else if (P.bits) transition_vec<true><<<pool_vec_grid(P.total), 256, 0, st>>>(args);
  else transition_vec<false><<<pool_vec_grid(P.total), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}

int launch_transition_i8(const TransitionI8Args& args, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const PoolArgs& P = args.D.P;
  if (!vec && P.bits) transition_i8_rows<true><<<pool_vec_grid(P.total * 64ull), 256, 0, st>>>(args);
  else if (!vec) transition_i8_rows<false><<<pool_vec_grid(P.total * 64ull), 256, 0, st>>>(args);
  else if (P.bits) transition_i8_vec<true><<<pool_vec_grid(P.total), 256, 0, st>>>(args);
  else transition_i8_vec<false><<<pool_vec_grid(P.total), 256, 0, st>>>(args);
  return (int)hipGetLastError();
}
}  // namespace lce
