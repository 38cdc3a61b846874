// Host simulation of lce_hip_depthwise_conv2d_i8's launch -- TEST ONLY (tests/test_depthwise_i8_hostsim.py).  The real kernel
// bodies of csrc/lce_kernels_depthwise_i8.h run on the CPU, 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the chunk and segment enumeration, the clipped window with its unclipped filter index,
// the channel mapping, the epilogue, the two-lane word and the ballots are exercised without a GPU.  Two device-only pieces of
// lce_kernels_pool.h are replaced (tests/hostsim/sim_harness.h): the 16-byte write-through store (inline assembly) is a plain store, and the quad permute
// v_mov_b32 quad_perm:[1,0,3,2] behind lane_neighbour is emulated as the exchange with lane ^ 1 it is.
#define SIM_HARNESS_POOL
#include "sim_harness.h"
#define __shared__ static               // (lce_kernels_conv2d_i8.h comes along for conv2d_i8_requantize; its kernel is not run here)
typedef int32_t sim_i32x4 __attribute__((vector_size(16)));
typedef int32_t sim_i32x16 __attribute__((vector_size(64)));
inline void __syncthreads() { __builtin_trap(); }
inline sim_i32x16 __builtin_amdgcn_mfma_i32_32x32x32_i8(sim_i32x4, sim_i32x4, sim_i32x16, int, int, int) { __builtin_trap(); }
#include "lce_kernels_depthwise_i8.h"

// d: batch, in_height, in_width, channels_in, depth_multiplier, filter_height, filter_width, stride_height, stride_width, out_height,
// out_width, pad_height, pad_width, input zero point, output zero point, act_min, act_max.  `table`: [3][Cout] as
// lce_hip_depthwise_conv2d_i8_prepare writes it.  `path`: -1 the entry's rule, 0 the row path.  `cap`: the most blocks of the launch
// (the product caps its grid at 2048; a small cap makes the kernels stride).  The launch is filled as the entry fills it
// (window_vec_rule, pool_window_fill, pool_vec_grid, pool_set_stride: lce_kernels_pool.h).  Returns 1 when the launch took the
// 16-byte path, 0 for the row path, and -1 when the padding pool_window_fill derived is not the caller's pad_height, pad_width.
extern "C" int lce_hostsim_depthwise_i8(const int32_t* d, const int8_t* in, const int8_t* filter, const int32_t* table, int8_t* out,
                                        int32_t* bits, int32_t path, int32_t cap) {
  lce::DepthwiseI8Args a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.P;
  const uint64_t C = (uint64_t)d[3] * (uint64_t)d[4];
  const bool vec = path != 0 && lce::window_vec_rule(d[4], C, 1, bits != nullptr, in, filter, table, out);
  p.in = in; p.out = out; p.bits = (uint32_t*)bits;
  a.filter = filter; a.table = table; a.zi = d[13];
  a.channels_in = (uint32_t)d[3];
  a.div_multiplier = lce::make_fastdiv((uint32_t)d[4]);
  lce::pool_window_fill(p, d[0], d[1], d[2], d[5], d[6], d[7], d[8], d[9], d[10], C, 16, vec, /*stream_loads_rule=*/true);
  if (p.ph != d[11] || p.pw != d[12]) return -1;
  p.qlo = d[15]; p.qhi = d[16]; p.zero_point = d[14];
  const unsigned gx = lce::pool_vec_grid(vec ? p.total : p.total * 64ull, (uint64_t)cap);      // launch_depthwise_i8's grid
  if (vec) lce::pool_set_stride(p, gx);
  if (!vec && bits) sim::launch(gx, 256, [&] { lce::depthwise_i8_rows<true>(a); });
  else if (!vec) sim::launch(gx, 256, [&] { lce::depthwise_i8_rows<false>(a); });
  else if (bits) sim::launch(gx, 256, [&] { lce::depthwise_i8_vec<true>(a); });
  else sim::launch(gx, 256, [&] { lce::depthwise_i8_vec<false>(a); });
  return vec ? 1 : 0;
}
