// Host simulation of lce_hip_pool_depthwise_f32's and lce_hip_pool_depthwise_i8's launches -- TEST ONLY
// (tests/test_transition_hostsim.py).  The real kernel bodies of csrc/lce_kernels_transition.h run on the CPU, 256 lanes of a block as
// fibers in lock step (tests/hostsim/lce_device_intrinsics.h), so the chunk and segment enumeration, the footprint streamed row by
// row, the clipped pool windows, the skipped depthwise taps, the epilogues, the words of bits and the ballots are exercised without
// a GPU.  Two device-only pieces of lce_kernels_pool.h are replaced here, as tests/hostsim_depthwise_i8 replaces them: the 16-byte
// write-through store (inline assembly) is a plain store, and the quad permute behind pool_neighbour is the exchange with lane ^ 1.
#include <cstring>
#include <vector>

#include "lce_device_intrinsics.h"      // the host replacement: build/ comes first on the include path
#define __HIPCC__ 1
#define __host__
#define __device__
#define __forceinline__ inline
#define __shared__                      // (lce_kernels_conv2d_i8.h and depthwise_vec's staged form come along; neither is instantiated here)
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
#include "lce_kernels_transition.h"

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

// d: batch, pool input height, width, channels_in, depth_multiplier; the pool's filter_height, filter_width, stride_height, stride_width,
// pad_height, pad_width; the pooled height and width; the depthwise filter_height, filter_width, stride_height, stride_width, pad_height,
// pad_width; the output height and width.  Fills the geometry of both launches and returns the grid: pool_vec_grid's (4 waves per
// block, 64 chunks or one segment per wave task) capped at `cap`, with pool_vec_steps of lce_hip_api.hip for it.
unsigned fill(lce::PoolArgs& p, lce::TransitionPool& q, const int32_t* d, uint64_t chunk, bool vec, int32_t cap) {
  const uint64_t C = (uint64_t)d[3] * (uint64_t)d[4], pixels = (uint64_t)d[0] * d[19] * d[20];
  q.H = d[1]; q.W = d[2]; q.fh = d[5]; q.fw = d[6]; q.sh = d[7]; q.sw = d[8]; q.ph = d[9]; q.pw = d[10];
  p.H = d[11]; p.W = d[12]; p.OH = d[19]; p.OW = d[20];
  p.fh = d[13]; p.fw = d[14]; p.sh = d[15]; p.sw = d[16]; p.ph = d[17]; p.pw = d[18];
  p.channels = (uint32_t)C;
  p.wpr = (uint32_t)((C + 31) / 32);
  p.per_pixel = (uint32_t)(vec ? C / chunk : (C + 63) / 64);
  p.total = pixels * p.per_pixel;
  p.div_ow = lce::make_fastdiv((uint32_t)d[20]);
  p.div_oh = lce::make_fastdiv((uint32_t)d[19]);
  const uint64_t tasks = vec ? (p.total + 63) / 64 : p.total, blocks = (tasks + 3) / 4;
  const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > (uint64_t)cap ? (uint64_t)cap : blocks);
  if (vec) {
    const uint64_t stride = (uint64_t)gx * 4ull * 64ull;
    p.step_pixels = (uint32_t)(stride / p.per_pixel);
    p.step_chunks = (uint32_t)(stride % p.per_pixel);
    p.div_per_pixel = lce::make_fastdiv(p.per_pixel);
  }
  return gx;
}
bool geometry(const int32_t* d) { return d[7] == 1 && d[8] == 1 && d[5] <= 2 && d[6] <= 2 && d[13] <= 3 && d[14] <= 3; }
}  // namespace

// `range`: the pool's activation range (lo, hi), then the depthwise convolution's.  `path`: -1 the entry's rule, 0 the row path.
// `cap`: the most blocks of the launch (the product caps its grid at 2048; a small cap makes the kernels stride).  Returns 1 when the
// launch took the 16-byte path.
extern "C" int lce_hostsim_transition_f32(const int32_t* d, const float* range, const float* in, const float* filter, const float* bias,
                                          float* out, int32_t* bits, int32_t path, int32_t cap) {
  lce::TransitionArgs a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.D.P;
  const uint64_t C = (uint64_t)d[3] * (uint64_t)d[4];
  // lce_hip_pool_depthwise_f32's rule
  bool vec = d[4] == 1 && C % 4 == 0 && ((uintptr_t)in | (uintptr_t)filter | (uintptr_t)bias | (uintptr_t)out) % 16 == 0 && geometry(d);
  if (bits && C % 32 != 0) vec = false;
  if (path == 0) vec = false;
  p.in = in; p.out = out; p.bits = (uint32_t*)bits;
  a.D.filter = filter; a.D.bias = bias;
  a.D.channels_in = (uint32_t)d[3];
  a.D.div_multiplier = lce::make_fastdiv((uint32_t)d[4]);
  const unsigned gx = fill(p, a.Q, d, 4, vec, cap);
  a.Q.lo = range[0]; a.Q.hi = range[1]; p.lo = range[2]; p.hi = range[3];
  if (!vec && bits) launch(gx, [&] { lce::transition_rows<true>(a); });
  else if (!vec) launch(gx, [&] { lce::transition_rows<false>(a); });
  else if (bits) launch(gx, [&] { lce::transition_vec<true>(a); });
  else launch(gx, [&] { lce::transition_vec<false>(a); });
  return vec ? 1 : 0;
}

// `q`: the shared zero point of the pool's input and output, the output zero point, the depthwise convolution's act_min and act_max,
// the pool's act_min and act_max.  `table`: [3][Cout] as lce_hip_depthwise_conv2d_i8_prepare writes it.
extern "C" int lce_hostsim_transition_i8(const int32_t* d, const int32_t* q, const int8_t* in, const int8_t* filter, const int32_t* table,
                                         int8_t* out, int32_t* bits, int32_t path, int32_t cap) {
  lce::TransitionI8Args a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.D.P;
  const uint64_t C = (uint64_t)d[3] * (uint64_t)d[4];
  // lce_hip_pool_depthwise_i8's rule
  bool vec = d[4] == 1 && C % 16 == 0 && ((uintptr_t)in | (uintptr_t)filter | (uintptr_t)table | (uintptr_t)out) % 16 == 0 && geometry(d);
  if (bits && C % 32 != 0) vec = false;
  if (path == 0) vec = false;
  p.in = in; p.out = out; p.bits = (uint32_t*)bits;
  a.D.filter = filter; a.D.table = table; a.D.zi = q[0];
  a.D.channels_in = (uint32_t)d[3];
  a.D.div_multiplier = lce::make_fastdiv((uint32_t)d[4]);
  const unsigned gx = fill(p, a.Q, d, 16, vec, cap);
  p.zero_point = q[1]; p.qlo = q[2]; p.qhi = q[3]; a.Q.qlo = q[4]; a.Q.qhi = q[5];
  if (!vec && bits) launch(gx, [&] { lce::transition_i8_rows<true>(a); });
  else if (!vec) launch(gx, [&] { lce::transition_i8_rows<false>(a); });
  else if (bits) launch(gx, [&] { lce::transition_i8_vec<true>(a); });
  else launch(gx, [&] { lce::transition_i8_vec<false>(a); });
  return vec ? 1 : 0;
}
