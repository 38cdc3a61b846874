// Host simulation of lce_hip_conv2d_i8's launch -- TEST ONLY (tests/test_conv2d_i8_hostsim.py).  The real kernel body of
// csrc/lce_kernels_conv2d_i8.h runs on the CPU, 256 lanes of a block as fibers in lock step (tests/hostsim/lce_device_intrinsics.h),
// so the pixel enumeration, the gather with its staged zero points, the LDS layout, the K tail, the epilogue and the ballots are
// exercised without a GPU.  What it cannot decide is the premise itself: v_mfma_i32_32x32x32_i8 is emulated here as the exact
// integer dot product under the maps the kernel assumes -- row of A and column of B from lane l & 31, the 16 bytes of lane l
// paired byte for byte with the 16 bytes of the B lane in the same half l >> 5; accumulator register r of lane l is row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.  The GPU suite decides that.
#include "sim_harness.h"
#define __shared__ static               // one block at a time, all of its lanes fibers of one thread
typedef int32_t sim_i32x4 __attribute__((vector_size(16)));      // the kernel header's i32x4 and i32x16
typedef int32_t sim_i32x16 __attribute__((vector_size(64)));
inline void __syncthreads() { g_ctx.block_bar->arrive_and_wait(); }
// (lce_kernels_eltwise_i8.h comes along for its two gemmlowp steps; its kernels are not run here)
inline sim_i32x16 __builtin_amdgcn_mfma_i32_32x32x32_i8(sim_i32x4 a, sim_i32x4 b, sim_i32x16 c, int, int, int) {
  const int lane = g_ctx.tid_x & 63;
  int8_t* x = (int8_t*)g_ctx.mfma_xchg;   // per lane 32 bytes: [a: 16][b: 16]
  memcpy(x + lane * 32, &a, 16);
  memcpy(x + lane * 32 + 16, &b, 16);
  g_ctx.bar->arrive_and_wait();
  const int col = lane & 31;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    int32_t sum = 0;
    for (int h = 0; h < 2; ++h)
      for (int j = 0; j < 16; ++j) sum += (int32_t)x[(row + 32 * h) * 32 + j] * (int32_t)x[(col + 32 * h) * 32 + 16 + j];
    c[r] += sum;
  }
  g_ctx.bar->arrive_and_wait();
  return c;
}
#include "lce_kernels_conv2d_i8.h"

namespace {
template <typename F>
void launch(unsigned gx, unsigned gy, F kernel) { sim::launch(gx, gy, 256, kernel, /*mfma_xchg=*/true); }
}  // namespace

// d: batch, in_height, in_width, channels_in, channels_out, filter_height, filter_width, stride_height, stride_width, out_height,
// out_width, input zero point, output zero point, act_min, act_max.  `table`: [3][Cout] as lce_hip_conv2d_i8_prepare writes it.
// `cap`: the most blocks per grid row (the product caps at 2048; a small cap makes the kernel stride).  Returns 1 when the launch
// took the 16-byte load path.
extern "C" int lce_hostsim_conv2d_i8(const int32_t* d, const int8_t* in, const int8_t* filter, const int32_t* table, int8_t* out,
                                     int32_t* bits, int32_t cap) {
  lce::ConvI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in; a.filter = filter; a.table = table; a.out = out; a.bits = (uint32_t*)bits;
  lce::conv2d_i8_geometry(a, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10]);
  a.zi = d[11]; a.zo = d[12]; a.act_min = d[13]; a.act_max = d[14];
  const bool vec = lce::conv2d_i8_vec_rule(a);
  unsigned gx = 0, gy = 0;
  lce::conv2d_i8_grid(a, (uint32_t)cap, &gx, &gy);                                                  // launch_conv2d_i8's grid, capped at `cap`
  if (vec) launch(gx, gy, [&] { lce::conv2d_i8<true>(a); });
  else launch(gx, gy, [&] { lce::conv2d_i8<false>(a); });
  return vec ? 1 : 0;
}

// The requantization the kernel's epilogue runs (conv2d_i8_requantize), element by element.
extern "C" void lce_hostsim_conv2d_i8_requantize(int64_t n, const int32_t* acc, const int32_t* m, const int32_t* e, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = lce::conv2d_i8_requantize(acc[i], m[i], e[i]);
}
