// One translation unit of the product library (csrc/Makefile): the extended elementwise chain (lce_kernels_eltwise.h, EX = 1),
// the instances lce_hip_elementwise_ex launches -- per-image operands, CLAMP, PRELU, LOGISTIC.
#include <hip/hip_runtime.h>
#include "lce_kernels_eltwise.h"

namespace lce {
int launch_eltwise_ex(const EwArgsEx& args, bool flat, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (flat) {
    const uint64_t total_words = args.rows * (uint64_t)args.wpr;
    eltwise_flat<1><<<eltwise_grid((total_words + 31) / 32), 256, 0, st>>>(args, total_words);
  } else {
    const uint32_t segs = (args.channels + 63u) / 64u;
    const uint64_t tasks = args.rows * (uint64_t)segs;
    eltwise_rows<1><<<eltwise_grid(tasks), 256, 0, st>>>(args, segs, tasks);
  }
  return (int)hipGetLastError();
}
}  // namespace lce
