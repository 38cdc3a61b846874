// Host simulation of lce_hip_elementwise's and lce_hip_elementwise_ex's launches -- TEST ONLY (tests/test_activation_host.py).  The
// real kernel bodies of csrc/lce_kernels_eltwise.h run on the CPU, 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the word and image bookkeeping of the flat path, the grid stride, the partial last
// block, the row path's ballots and every step kind are exercised without a GPU.
#include <cmath>

#include "sim_harness.h"
inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
#include "lce_kernels_eltwise.h"

namespace {
template <typename F>
void launch(unsigned gx, F kernel) { sim::launch(gx, 256, kernel); }
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
    lce::float_activation_range(acts[s], &k.lo, &k.hi);
    if (k.values && (uintptr_t)k.values % 16 != 0) aligned = false;
  }
  const bool flat = channels % 32 == 0 && aligned;
  auto grid = [&](uint64_t wave_tasks) { return lce::stream_grid(wave_tasks, 4, (uint64_t)cap); };
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
