// Host simulation of lce_hip_elementwise's and lce_hip_elementwise_ex's launches -- TEST ONLY (tests/test_activation_host.py).  The
// real kernel bodies of csrc/lce_kernels_eltwise.h run on the CPU, 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the word and image bookkeeping of the flat path, the grid stride, the partial last
// block, the row path's ballots and every step kind are exercised without a GPU.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "lce_device_intrinsics.h"      // the host replacement: build/ comes first on the include path
inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
#define __HIPCC__ 1
#include "lce_kernels_eltwise.h"

namespace {
template <typename F>
void launch(unsigned gx, F kernel) {
  for (unsigned bx = 0; bx < gx; ++bx) {
    std::vector<uint32_t> xchg(4 * 64);
    lce_dev::FiberBarrier block_bar(256);
    lce_dev::FiberBarrier wave_bar[4] = {lce_dev::FiberBarrier(64), lce_dev::FiberBarrier(64), lce_dev::FiberBarrier(64),
                                         lce_dev::FiberBarrier(64)};
    lce_dev::run_fibers(256,
      [&](int t, lce_dev::ThreadCtx& c) {
        const int w = t >> 6;
        c.tid_x = t; c.bid_x = (int)bx; c.bid_y = 0; c.bdim_x = 256; c.gdim_x = (int)gx;
        c.bar = &wave_bar[w]; c.xchg = xchg.data() + w * 64; c.block_bar = &block_bar;
      },
      [&](int) { kernel(); });
  }
}
}  // namespace

// One launch of the chain.  Step s is (ops[s], operands[s], values[s], scalars[s], acts[s]).  `ex`: 1 runs the instances of
// lce_hip_elementwise_ex, 0 those of lce_hip_elementwise (ADD / MUL with the first three operand kinds only).  `cap`: the most
// blocks of the launch (the product caps its grid at 2048; a small cap makes every wave stride).  The path is chosen by
// the entries' rule; returns 1 when the launch took the flat path.
extern "C" int lce_hostsim_eltwise(int64_t rows, int32_t channels, int64_t rows_per_image, int32_t num_steps, const int32_t* ops,
                                   const int32_t* operands, const float* const* values, const float* scalars, const int32_t* acts,
                                   const float* in, float* out, uint32_t* bits, int32_t cap, int32_t ex) {
  lce::EwArgsEx a;
  memset(&a, 0, sizeof a);
  a.in = in; a.out = out; a.bits = bits;
  a.rows = (uint64_t)rows; a.channels = (uint32_t)channels; a.wpr = (uint32_t)((channels + 31) / 32);
  a.num_steps = num_steps;
  a.rows_per_image = (uint64_t)rows_per_image;
  bool aligned = (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)bits % 16 == 0;
  for (int s = 0; s < num_steps; ++s) {
    lce::EwStep& k = a.steps[s];
    k.op = ops[s]; k.operand = operands[s]; k.values = values[s]; k.scalar = scalars[s];
    switch (acts[s]) {
      case 1: k.lo = 0.0f; k.hi = FLT_MAX; break;
      case 2: k.lo = -1.0f; k.hi = 1.0f; break;
      case 3: k.lo = 0.0f; k.hi = 6.0f; break;
      default: k.lo = -FLT_MAX; k.hi = FLT_MAX;
    }
    if (k.values && (uintptr_t)k.values % 16 != 0) aligned = false;
  }
  const bool flat = channels % 32 == 0 && aligned;
  auto grid = [&](uint64_t wave_tasks) {                    // lce_tu_eltwise.hip's, with the cap a parameter
    const uint64_t blocks = (wave_tasks + 3) / 4;
    return (unsigned)(blocks < 1 ? 1 : (blocks > (uint64_t)cap ? (uint64_t)cap : blocks));
  };
  const lce::EwArgs& a0 = a;
  if (flat) {
    const uint64_t total_words = a.rows * (uint64_t)a.wpr;
    if (ex) launch(grid((total_words + 31) / 32), [&] { lce::eltwise_flat<1>(a, total_words); });
    else launch(grid((total_words + 31) / 32), [&] { lce::eltwise_flat<0>(a0, total_words); });
  } else {
    const uint32_t segs = (a.channels + 63u) / 64u;
    const uint64_t tasks = a.rows * (uint64_t)segs;
    if (ex) launch(grid(tasks), [&] { lce::eltwise_rows<1>(a, segs, tasks); });
    else launch(grid(tasks), [&] { lce::eltwise_rows<0>(a0, segs, tasks); });
  }
  return flat ? 1 : 0;
}

// The stated LOGISTIC alone, element by element.
extern "C" void lce_hostsim_logistic(const float* x, float* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = lce::ew_logistic(x[i]);
}
