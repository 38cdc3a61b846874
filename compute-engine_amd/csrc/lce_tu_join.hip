// One translation unit of the product library (csrc/Makefile): the channel join (lce_kernels_join.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_join.h"

namespace lce {
namespace {
// memory-bound streams: 4 waves per block, at most ~8 blocks per CU, grid-stride the rest (as lce_tu_eltwise.hip)
unsigned join_stream_grid(uint64_t wave_tasks) {
  const uint64_t blocks = (wave_tasks + 3) / 4, cap = 256ull * 8ull;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

template <int KIND, bool ADD>
void join_launch_vec(const JoinArgs& args, hipStream_t st) {
  const unsigned grid = join_vec_grid(args.total_chunks);
  if (args.bits) join_vec<KIND, true, ADD><<<grid, 256, 0, st>>>(args);
  else join_vec<KIND, false, ADD><<<grid, 256, 0, st>>>(args);
}

template <typename E, int KIND, bool ADD>
void join_launch_rows(const JoinArgs& args, hipStream_t st) {
  const uint32_t segs = (args.total + 63u) / 64u;
  const uint64_t tasks = args.rows * (uint64_t)segs;
  join_rows<E, KIND, ADD><<<join_stream_grid(tasks), 256, 0, st>>>(args, segs, tasks);
}
}  // namespace

unsigned join_vec_grid(uint64_t total_chunks) { return join_stream_grid((total_chunks + 255) / 256); }

int launch_join(const JoinArgs& args, int kind, bool vec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool add = join_has_addend(args);
  switch (kind) {
    case kJoinF32:
      if (add) { if (vec) join_launch_vec<kJoinF32, true>(args, st); else join_launch_rows<uint32_t, kJoinF32, true>(args, st); }
      else     { if (vec) join_launch_vec<kJoinF32, false>(args, st); else join_launch_rows<uint32_t, kJoinF32, false>(args, st); }
      break;
    case kJoinI8:
      if (add) return (int)hipErrorInvalidValue;
      if (vec) join_launch_vec<kJoinI8, false>(args, st); else join_launch_rows<int8_t, kJoinI8, false>(args, st);
      break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
}  // namespace lce
