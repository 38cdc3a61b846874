// One translation unit of the product library (csrc/Makefile): the int8 elementwise chain (lce_kernels_eltwise_i8_chain.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_eltwise_i8_chain.h"

namespace lce {
namespace {
template <int H, int P>
int launch_place(const EwI8Args& args, bool flat, unsigned blocks, unsigned threads, unsigned lds_bytes, hipStream_t st) {
  if (flat) {
    const uint64_t total_chunks = args.A.rows * (uint64_t)args.A.wpr * 2ull;
    auto* kernel = &ew_i8_flat<H, P>;
    static bool raised = false;                                    // more dynamic LDS than the default limit: asked for once per kernel
    if (lds_bytes > 64u * 1024u && !raised) {
      const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEwI8LdsLimit);
      if (e != hipSuccess) return (int)e;
      raised = true;
    }
    kernel<<<blocks, threads, lds_bytes, st>>>(args, total_chunks);
  } else {
    const uint32_t segs = (args.A.channels + 63u) / 64u;
    const uint64_t tasks = args.A.rows * (uint64_t)segs;
    auto* kernel = &ew_i8_rows<H, P>;
    static bool raised = false;
    if (lds_bytes > 64u * 1024u && !raised) {
      const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEwI8LdsLimit);
      if (e != hipSuccess) return (int)e;
      raised = true;
    }
    kernel<<<blocks, threads, lds_bytes, st>>>(args, segs, tasks);
  }
  return (int)hipGetLastError();
}

template <int H>
int launch_head(const EwI8Args& args, int path, bool flat, unsigned blocks, unsigned threads, unsigned lds_bytes, hipStream_t st) {
  switch (path) {
    case kEwI8Lds: return launch_place<H, kEwI8Lds>(args, flat, blocks, threads, lds_bytes, st);
    case kEwI8Global: return launch_place<H, kEwI8Global>(args, flat, blocks, threads, lds_bytes, st);
    case kEwI8OneRow: return launch_place<H, kEwI8OneRow>(args, flat, blocks, threads, lds_bytes, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace

int launch_ew_i8(const EwI8Args& args, int head, int path, bool flat, unsigned blocks, unsigned threads, unsigned lds_bytes,
                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
  switch (head) {
    case kAddI8Literal: return launch_head<kAddI8Literal>(args, path, flat, blocks, threads, lds_bytes, st);
    case kAddI8Split: return launch_head<kAddI8Split>(args, path, flat, blocks, threads, lds_bytes, st);
    case kAddI8Shift: return launch_head<kAddI8Shift>(args, path, flat, blocks, threads, lds_bytes, st);
    case kEwI8NoHead: return launch_head<kEwI8NoHead>(args, path, flat, blocks, threads, lds_bytes, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace lce
