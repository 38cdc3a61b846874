// One translation unit of the product library (csrc/Makefile): 2-D pooling (lce_kernels_pool.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_pool.h"

namespace lce {
namespace {
// memory-bound streams: 4 waves per block, at most ~8 blocks per CU, grid-stride the rest (stream_grid, as lce_tu_eltwise.hip)
template <int KIND, int OP>
void launch_kind_op(const PoolArgs& args, bool vec, hipStream_t st) {
  if (!vec) {
    pool_rows<KIND, OP><<<stream_grid(args.total), 256, 0, st>>>(args);
    return;
  }
  const unsigned grid = pool_vec_grid(args.total);
  if (args.bits) pool_vec<KIND, OP, true><<<grid, 256, 0, st>>>(args);
  else pool_vec<KIND, OP, false><<<grid, 256, 0, st>>>(args);
}
}  // namespace

int launch_pool(const PoolArgs& args, int kind, int op, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (kind == kPoolF32 && op == kPoolMax) launch_kind_op<kPoolF32, kPoolMax>(args, vec, st);
  else if (kind == kPoolF32 && op == kPoolAverage) launch_kind_op<kPoolF32, kPoolAverage>(args, vec, st);
  else if (kind == kPoolI8 && op == kPoolMax) launch_kind_op<kPoolI8, kPoolMax>(args, vec, st);
  else if (kind == kPoolI8 && op == kPoolAverage) launch_kind_op<kPoolI8, kPoolAverage>(args, vec, st);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}
}  // namespace lce
