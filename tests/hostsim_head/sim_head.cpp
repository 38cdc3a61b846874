// Host simulation of lce_hip_fully_connected_f32's and lce_hip_softmax_f32's launches -- TEST ONLY (tests/test_head_host.py).  The
// real kernel bodies of csrc/lce_kernels_head.h run on the CPU, 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the tile enumeration, both load paths, the transpose among the lane groups, the K
// tail, the epilogue, the stated exp and the order of the sum are exercised without a GPU.  What it cannot decide is the premise
// itself: v_mfma_f32_16x16x4_f32 is emulated here as the k-ordered fmaf chain the kernel takes it for (row / column l & 15 at
// k = l >> 4; accumulator register i of lane l is row 4 (l >> 4) + i, column l & 15).  The GPU suite decides that.
#include <cmath>

#include "sim_harness.h"
inline lce_dev::f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float a, float b, lce_dev::f32x4 c, int, int, int) {
  const int lane = g_ctx.tid_x & 63;
  float* x = (float*)g_ctx.mfma_xchg;   // per lane: [a, b, ...]
  x[lane * 8 + 0] = a;
  x[lane * 8 + 1] = b;
  g_ctx.bar->arrive_and_wait();
  const int col = lane & 15;
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * (lane >> 4) + i;
    for (int k = 0; k < 4; ++k) c[i] = fmaf(x[(row + 16 * k) * 8 + 0], x[(col + 16 * k) * 8 + 1], c[i]);
  }
  g_ctx.bar->arrive_and_wait();
  return c;
}
#include "lce_kernels_head.h"

// d: batch, inputs, outputs, activation.  `cap`: the most blocks of the launch (the product caps its grid at 2048; a small cap
// makes the kernel stride).  Returns 1 when the launch took the 16-byte load path.
extern "C" int lce_hostsim_fully_connected(const int32_t* d, const float* in, const float* weights, const float* bias, float* out,
                                           int32_t cap) {
  lce::FcArgs a;
  memset(&a, 0, sizeof a);
  a.in = in; a.filter = weights; a.bias = bias; a.out = out;
  lce::fc_fill(a, d[0], d[1], d[2]);
  lce::float_activation_range(d[3], &a.lo, &a.hi);
  const bool vec = lce::fc_vec_rule(a);
  const unsigned gx = lce::fc_grid(a, (uint64_t)cap);
  if (vec) sim::launch(gx, 256, [&] { lce::fully_connected_f32<true>(a); }, /*mfma_xchg=*/true);
  else sim::launch(gx, 256, [&] { lce::fully_connected_f32<false>(a); }, /*mfma_xchg=*/true);
  return vec ? 1 : 0;
}

extern "C" void lce_hostsim_softmax(int64_t rows, int32_t cols, float beta, const float* in, float* out, int32_t cap) {
  lce::SoftmaxArgs a;
  memset(&a, 0, sizeof a);
  a.in = in; a.out = out; a.rows = (uint64_t)rows; a.cols = (uint32_t)cols; a.beta = beta;
  sim::launch(lce::stream_grid(a.rows, 4, (uint64_t)cap), 256, [&] { lce::softmax_f32<4>(a); });
}

// The stated exp alone, element by element (the accuracy test sweeps it over 10^7 arguments).
extern "C" void lce_hostsim_head_exp(const float* a, float* e, int64_t n) {
  for (int64_t i = 0; i < n; ++i) e[i] = lce::head_exp(a[i]);
}
