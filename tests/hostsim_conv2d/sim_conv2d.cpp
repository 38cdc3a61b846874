// Host simulation of lce_hip_conv2d_f32's two launches -- TEST ONLY (tests/test_conv2d_hostsim.py).  The real kernel bodies of
// csrc/lce_kernels_conv2d.h run on the CPU, 256 lanes of a block as fibers in lock step (tests/hostsim/lce_device_intrinsics.h), so
// the pixel enumerations, the gather, the LDS layout, the K tail, the epilogue and the ballots are exercised without a GPU.  What
// it cannot decide is the premise itself: v_mfma_f32_32x32x2_f32 is emulated here as the k-ordered fmaf chain the kernels take it
// for (rows and columns from lanes 0..31 for k = 0 and 32..63 for k = 1; accumulator register r of lane l is row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31).  The GPU suite decides that.
#include <cmath>

#include "sim_harness.h"
#define __shared__ static               // one block at a time, all of its lanes fibers of one thread
inline void __syncthreads() { g_ctx.block_bar->arrive_and_wait(); }
inline lce_dev::f32x16 __builtin_amdgcn_mfma_f32_32x32x2f32(float a, float b, lce_dev::f32x16 c, int, int, int) {
  const int lane = g_ctx.tid_x & 63;
  float* x = (float*)g_ctx.mfma_xchg;   // per lane: [a, b, ...]
  x[lane * 8 + 0] = a;
  x[lane * 8 + 1] = b;
  g_ctx.bar->arrive_and_wait();
  const int col = lane & 31;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    c[r] = fmaf(x[row * 8 + 0], x[col * 8 + 1], c[r]);                    // k = 0
    c[r] = fmaf(x[(row + 32) * 8 + 0], x[(col + 32) * 8 + 1], c[r]);      // k = 1
  }
  g_ctx.bar->arrive_and_wait();
  return c;
}
#include "lce_kernels_conv2d.h"

namespace {
template <typename F>
void launch(unsigned gx, unsigned gy, F kernel) { sim::launch(gx, gy, 256, kernel, /*mfma_xchg=*/true); }
}  // namespace

// d: batch, in_height, in_width, channels_in, channels_out, filter_height, filter_width, stride_height, stride_width, out_height,
// out_width, activation.  `cap`: the most blocks per launch (the product caps its grids at 2048; a small cap makes the kernels
// stride).  Returns bit 0: the interior took the 16-byte load path; bit 1: the border launch ran.
extern "C" int lce_hostsim_conv2d(const int32_t* d, const float* in, const float* filter, const float* bias, float* out, int32_t* bits,
                                  int32_t cap) {
  lce::Conv2dArgs a;
  memset(&a, 0, sizeof a);
  a.in = in; a.filter = filter; a.bias = bias; a.out = out; a.bits = (uint32_t*)bits;
  lce::conv2d_geometry(a, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10]);
  lce::float_activation_range(d[11], &a.lo, &a.hi);
  const bool vec = lce::conv2d_vec_rule(a);
  // launch_conv2d's two launches (lce_tu_conv2d.hip), their grids capped at `cap`
  if (a.Mi > 0) {
    unsigned gx = 0, gy = 0;
    lce::conv2d_grid(a, (uint32_t)cap, &gx, &gy);
    if (vec) launch(gx, gy, [&] { lce::conv2d_interior<true>(a); });
    else launch(gx, gy, [&] { lce::conv2d_interior<false>(a); });
  }
  if (a.Mb > 0) {
    const unsigned gx = lce::conv2d_border_grid(a, (uint64_t)cap);
    if (a.bits) launch(gx, 1, [&] { lce::conv2d_border<true>(a); });
    else launch(gx, 1, [&] { lce::conv2d_border<false>(a); });
  }
  return (vec ? 1 : 0) | (a.Mb > 0 ? 2 : 0);
}
