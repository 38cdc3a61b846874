// Host simulation of lce_hip_conv2d_f32's two launches -- TEST ONLY (tests/test_conv2d_hostsim.py).  The real kernel bodies of
// csrc/lce_kernels_conv2d.h run on the CPU, 256 lanes of a block as fibers in lock step (tests/hostsim/lce_device_intrinsics.h), so
// the pixel enumerations, the gather, the LDS layout, the K tail, the epilogue and the ballots are exercised without a GPU.  What
// it cannot decide is the premise itself: v_mfma_f32_32x32x2_f32 is emulated here as the k-ordered fmaf chain the kernels take it
// for (rows and columns from lanes 0..31 for k = 0 and 32..63 for k = 1; accumulator register r of lane l is row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31).  The GPU suite decides that.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "lce_device_intrinsics.h"      // the host replacement: build/ comes first on the include path
#define __HIPCC__ 1
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
void launch(unsigned gx, unsigned gy, F kernel) {
  for (unsigned by = 0; by < gy; ++by)
    for (unsigned bx = 0; bx < gx; ++bx) {
      std::vector<uint32_t> xchg(4 * 64), mx(4 * 64 * 8);
      lce_dev::FiberBarrier block_bar(256);
      lce_dev::FiberBarrier wave_bar[4] = {lce_dev::FiberBarrier(64), lce_dev::FiberBarrier(64), lce_dev::FiberBarrier(64),
                                           lce_dev::FiberBarrier(64)};
      lce_dev::run_fibers(256,
        [&](int t, lce_dev::ThreadCtx& c) {
          const int w = t >> 6;
          c.tid_x = t; c.bid_x = (int)bx; c.bid_y = (int)by; c.bdim_x = 256; c.gdim_x = (int)gx;
          c.bar = &wave_bar[w]; c.xchg = xchg.data() + w * 64; c.mfma_xchg = mx.data() + w * 64 * 8; c.block_bar = &block_bar;
        },
        [&](int) { kernel(); });
    }
}
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
  switch (d[11]) {
    case 1: a.lo = 0.0f; a.hi = FLT_MAX; break;
    case 2: a.lo = -1.0f; a.hi = 1.0f; break;
    case 3: a.lo = 0.0f; a.hi = 6.0f; break;
    default: a.lo = -FLT_MAX; a.hi = FLT_MAX;
  }
  const bool vec = a.Cin % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)filter % 16 == 0;       // lce_hip_conv2d_f32's rule
  // launch_conv2d's grids (lce_tu_conv2d.hip), capped at `cap`
  if (a.Mi > 0) {
    const unsigned gx = a.mtiles < (uint32_t)cap ? a.mtiles : (uint32_t)cap, gy = (a.Cout + lce::kConv2dBN - 1) / lce::kConv2dBN;
    if (vec) launch(gx, gy, [&] { lce::conv2d_interior<true>(a); });
    else launch(gx, gy, [&] { lce::conv2d_interior<false>(a); });
  }
  if (a.Mb > 0) {
    const uint64_t tasks = (uint64_t)a.Mb * a.segs, blocks = (tasks + 3) / 4;
    const unsigned gx = (unsigned)(blocks < (uint64_t)cap ? blocks : (uint64_t)cap);
    if (a.bits) launch(gx, 1, [&] { lce::conv2d_border<true>(a); });
    else launch(gx, 1, [&] { lce::conv2d_border<false>(a); });
  }
  return (vec ? 1 : 0) | (a.Mb > 0 ? 2 : 0);
}
