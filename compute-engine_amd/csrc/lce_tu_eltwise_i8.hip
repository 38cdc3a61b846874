// One translation unit of the product library (csrc/Makefile): the int8 residual ADD (lce_kernels_eltwise_i8.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_eltwise_i8.h"

namespace lce {
namespace {
template <int V>
void launch_variant(const AddI8Args& args, bool flat, hipStream_t st) {
  // memory-bound streams: 4 waves per block, at most ~8 blocks per CU, grid-stride the rest (as lce_tu_eltwise.hip)
  auto grid = [](uint64_t wave_tasks) {
    const uint64_t blocks = (wave_tasks + 3) / 4, cap = 256ull * 8ull;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
  };
  if (flat) {
    const uint64_t total_chunks = args.rows * (uint64_t)args.wpr * 2ull;
    add_i8_flat<V><<<grid((total_chunks + 255) / 256), 256, 0, st>>>(args, total_chunks);
  } else {
    const uint32_t segs = (args.channels + 63u) / 64u;
    const uint64_t tasks = args.rows * (uint64_t)segs;
    add_i8_rows<V><<<grid(tasks), 256, 0, st>>>(args, segs, tasks);
  }
}
}  // namespace

int launch_add_i8(const AddI8Args& args, int variant, bool flat, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  switch (variant) {
    case kAddI8Literal: launch_variant<kAddI8Literal>(args, flat, st); break;
    case kAddI8Split: launch_variant<kAddI8Split>(args, flat, st); break;
    case kAddI8Shift: launch_variant<kAddI8Shift>(args, flat, st); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
}  // namespace lce
