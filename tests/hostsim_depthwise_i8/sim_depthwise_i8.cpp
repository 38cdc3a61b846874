// Host simulation of lce_hip_depthwise_conv2d_i8's launch -- TEST ONLY (tests/test_depthwise_i8_hostsim.py).  The real kernel
// bodies of csrc/lce_kernels_depthwise_i8.h run on the CPU, 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the chunk and segment enumeration, the clipped window with its unclipped filter index,
// the channel mapping, the epilogue, the two-lane word and the ballots are exercised without a GPU.  Two device-only pieces of
// lce_kernels_pool.h are replaced here: the 16-byte write-through store (inline assembly) is a plain store, and the quad permute
// v_mov_b32 quad_perm:[1,0,3,2] behind pool_neighbour is emulated as the exchange with lane ^ 1 it is.
#include <cstring>
#include <vector>

#include "lce_device_intrinsics.h"      // the host replacement: build/ comes first on the include path
#define __HIPCC__ 1
#define __host__
#define __device__
#define __forceinline__ inline
#define __shared__ static               // (lce_kernels_conv2d_i8.h comes along for conv2d_i8_requantize; its kernel is not run here)
typedef int32_t sim_i32x4 __attribute__((vector_size(16)));
typedef int32_t sim_i32x16 __attribute__((vector_size(64)));
inline void __syncthreads() { __builtin_trap(); }
inline sim_i32x16 __builtin_amdgcn_mfma_i32_32x32x32_i8(sim_i32x4, sim_i32x4, sim_i32x16, int, int, int) { __builtin_trap(); }
// dpp_ctrl 0xB1 = quad_perm:[1,0,3,2], all rows and banks, bound_ctrl: the value of lane ^ 1 (every lane of the wave calls it)
inline int __builtin_amdgcn_mov_dpp(int v, int ctrl, int row_mask, int bank_mask, bool) {
  if (ctrl != 0xB1 || row_mask != 0xF || bank_mask != 0xF) __builtin_trap();
  return (int)lce_dev::shfl_xor((uint32_t)v, 1);
}
// the header's store keeps its assembly under another name (never called here); the kernels get a plain 16-byte store
#define pool_store_through pool_store_through_device
#include "lce_kernels_pool.h"
#undef pool_store_through
namespace lce {
inline void pool_store_through(u32x4* p, u32x4 v) { memcpy(p, &v, 16); }
}  // namespace lce
#include "lce_kernels_depthwise_i8.h"

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

// d: batch, in_height, in_width, channels_in, depth_multiplier, filter_height, filter_width, stride_height, stride_width, out_height,
// out_width, pad_height, pad_width, input zero point, output zero point, act_min, act_max.  `table`: [3][Cout] as
// lce_hip_depthwise_conv2d_i8_prepare writes it.  `path`: -1 the entry's rule, 0 the row path.  `cap`: the most blocks of the launch
// (the product caps its grid at 2048; a small cap makes the kernels stride).  Returns 1 when the launch took the 16-byte path.
extern "C" int lce_hostsim_depthwise_i8(const int32_t* d, const int8_t* in, const int8_t* filter, const int32_t* table, int8_t* out,
                                        int32_t* bits, int32_t path, int32_t cap) {
  lce::DepthwiseI8Args a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.P;
  const uint64_t C = (uint64_t)d[3] * (uint64_t)d[4], pixels = (uint64_t)d[0] * d[9] * d[10];
  // lce_hip_depthwise_conv2d_i8's rule
  bool vec = d[4] == 1 && C % 16 == 0 && ((uintptr_t)in | (uintptr_t)filter | (uintptr_t)table | (uintptr_t)out) % 16 == 0;
  if (bits && C % 32 != 0) vec = false;
  if (path == 0) vec = false;
  p.in = in; p.out = out; p.bits = (uint32_t*)bits;
  a.filter = filter; a.table = table; a.zi = d[13];
  a.channels_in = (uint32_t)d[3];
  a.div_multiplier = lce::make_fastdiv((uint32_t)d[4]);
  p.H = d[1]; p.W = d[2]; p.OH = d[9]; p.OW = d[10];
  p.fh = d[5]; p.fw = d[6]; p.sh = d[7]; p.sw = d[8]; p.ph = d[11]; p.pw = d[12];
  p.channels = (uint32_t)C;
  p.wpr = (uint32_t)((C + 31) / 32);
  p.per_pixel = (uint32_t)(vec ? C / 16 : (C + 63) / 64);
  p.stream_loads = d[7] >= d[5] && d[8] >= d[6] ? 1u : 0u;
  p.total = pixels * p.per_pixel;
  p.qlo = d[15]; p.qhi = d[16]; p.zero_point = d[14];
  p.div_ow = lce::make_fastdiv((uint32_t)d[10]);
  p.div_oh = lce::make_fastdiv((uint32_t)d[9]);
  // launch_depthwise_i8's grid (pool_vec_grid: 4 waves per block, 64 chunks or one segment per wave task), capped at `cap`
  const uint64_t tasks = vec ? (p.total + 63) / 64 : p.total, blocks = (tasks + 3) / 4;
  const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > (uint64_t)cap ? (uint64_t)cap : blocks);
  if (vec) {                                                       // pool_vec_steps of lce_hip_api.hip for this grid
    const uint64_t stride = (uint64_t)gx * 4ull * 64ull;
    p.step_pixels = (uint32_t)(stride / p.per_pixel);
    p.step_chunks = (uint32_t)(stride % p.per_pixel);
    p.div_per_pixel = lce::make_fastdiv(p.per_pixel);
  }
  if (!vec && bits) launch(gx, [&] { lce::depthwise_i8_rows<true>(a); });
  else if (!vec) launch(gx, [&] { lce::depthwise_i8_rows<false>(a); });
  else if (bits) launch(gx, [&] { lce::depthwise_i8_vec<true>(a); });
  else launch(gx, [&] { lce::depthwise_i8_vec<false>(a); });
  return vec ? 1 : 0;
}
