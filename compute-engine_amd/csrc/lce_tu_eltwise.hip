// One translation unit of the product library (csrc/Makefile): the float elementwise tail (lce_kernels_eltwise.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_eltwise.h"

namespace lce {
int launch_eltwise(const EwArgs& args, bool flat, void* stream) {
  // memory-bound streams: 4 waves per block, at most ~8 blocks per CU, grid-stride the rest (as lce_hip_api.hip's bitpack)
  auto grid = [](uint64_t wave_tasks) {
    const uint64_t blocks = (wave_tasks + 3) / 4, cap = 256ull * 8ull;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
  };
  hipStream_t st = (hipStream_t)stream;
  if (flat) {
    const uint64_t total_words = args.rows * (uint64_t)args.wpr;
    eltwise_flat<><<<grid((total_words + 31) / 32), 256, 0, st>>>(args, total_words);
  } else {
    const uint32_t segs = (args.channels + 63u) / 64u;
    const uint64_t tasks = args.rows * (uint64_t)segs;
    eltwise_rows<><<<grid(tasks), 256, 0, st>>>(args, segs, tasks);
  }
  return (int)hipGetLastError();
}
}  // namespace lce
