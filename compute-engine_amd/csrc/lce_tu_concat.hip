// One translation unit of the product library (csrc/Makefile): the channel join (lce_kernels_concat.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_concat.h"

namespace lce {
namespace {
// memory-bound streams: 4 waves per block, at most ~8 blocks per CU, grid-stride the rest (as lce_tu_eltwise.hip)
unsigned stream_grid(uint64_t wave_tasks) {
  const uint64_t blocks = (wave_tasks + 3) / 4, cap = 256ull * 8ull;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

template <int KIND>
void launch_vec(const ConcatArgs& args, hipStream_t st) {
  const unsigned grid = concat_vec_grid(args.total_chunks);
  if constexpr (KIND != kConcatWords) {
    if (args.bits) { concat_vec<KIND, true><<<grid, 256, 0, st>>>(args); return; }
  }
  concat_vec<KIND, false><<<grid, 256, 0, st>>>(args);
}

template <typename E, int KIND>
void launch_rows(const ConcatArgs& args, hipStream_t st) {
  const uint32_t segs = (args.total + 63u) / 64u;
  const uint64_t tasks = args.rows * (uint64_t)segs;
  concat_rows<E, KIND><<<stream_grid(tasks), 256, 0, st>>>(args, segs, tasks);
}
}  // namespace

unsigned concat_vec_grid(uint64_t total_chunks) { return stream_grid((total_chunks + 255) / 256); }

int launch_concat(const ConcatArgs& args, int kind, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case kConcatF32:
      if (vec) launch_vec<kConcatF32>(args, st); else launch_rows<uint32_t, kConcatF32>(args, st);
      break;
    case kConcatI8:
      if (vec) launch_vec<kConcatI8>(args, st); else launch_rows<int8_t, kConcatI8>(args, st);
      break;
    case kConcatWords:
      if (vec) launch_vec<kConcatWords>(args, st); else launch_rows<uint32_t, kConcatWords>(args, st);
      break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
}  // namespace lce
