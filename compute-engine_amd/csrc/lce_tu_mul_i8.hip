// One translation unit of the product library (csrc/Makefile): the int8 gate MUL with its residual ADD (lce_kernels_mul_i8.h).
#include <hip/hip_runtime.h>
#include "lce_kernels_mul_i8.h"

namespace lce {
namespace {
template <int MV, int V, bool PI>
void launch_kind(const MulI8Args& args, bool flat, unsigned blocks, hipStream_t st) {
  if (flat) {
    const uint64_t total_chunks = args.A.rows * (uint64_t)args.cpr;
    mul_i8_flat<MV, V, PI><<<blocks, 256, 0, st>>>(args, total_chunks);
  } else {
    const uint32_t segs = (args.A.channels + 63u) / 64u;
    const uint64_t tasks = args.A.rows * (uint64_t)segs;
    mul_i8_rows<MV, V, PI><<<blocks, 256, 0, st>>>(args, segs, tasks);
  }
}

template <int MV, int V>
void launch_add(const MulI8Args& args, bool per_image, bool flat, unsigned blocks, hipStream_t st) {
  if (per_image) launch_kind<MV, V, true>(args, flat, blocks, st);
  else launch_kind<MV, V, false>(args, flat, blocks, st);
}

template <int MV>
int launch_mul(const MulI8Args& args, int add, bool per_image, bool flat, unsigned blocks, hipStream_t st) {
  switch (add) {
    case kAddI8Literal: launch_add<MV, kAddI8Literal>(args, per_image, flat, blocks, st); break;
    case kAddI8Split: launch_add<MV, kAddI8Split>(args, per_image, flat, blocks, st); break;
    case kAddI8Shift: launch_add<MV, kAddI8Shift>(args, per_image, flat, blocks, st); break;
    case kMulI8NoAdd: launch_add<MV, kMulI8NoAdd>(args, per_image, flat, blocks, st); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
}  // namespace

int launch_mul_i8(const MulI8Args& args, int mul, int add, bool per_image, bool flat, unsigned blocks, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  switch (mul) {
    case kMulI8Literal: return launch_mul<kMulI8Literal>(args, add, per_image, flat, blocks, st);
    case kMulI8Fast: return launch_mul<kMulI8Fast>(args, add, per_image, flat, blocks, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace lce
