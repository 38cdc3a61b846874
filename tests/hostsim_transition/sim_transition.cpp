// Host simulation of lce_hip_pool_depthwise_f32's and lce_hip_pool_depthwise_i8's launches -- TEST ONLY
// (tests/test_transition_hostsim.py).  The real kernel bodies of csrc/lce_kernels_transition.h run on the CPU, 256 lanes of a block as
// fibers in lock step (tests/hostsim/lce_device_intrinsics.h), so the chunk and segment enumeration, the footprint streamed row by
// row, the clipped pool windows, the skipped depthwise taps, the epilogues, the words of bits and the ballots are exercised without
// a GPU.  Two device-only pieces of lce_kernels_pool.h are replaced (tests/hostsim/sim_harness.h): the 16-byte
// write-through store (inline assembly) is a plain store, and the quad permute behind lane_neighbour is the exchange with lane ^ 1.
#define SIM_HARNESS_POOL
#include "sim_harness.h"
#define __shared__                      // (lce_kernels_conv2d_i8.h and depthwise_vec's staged form come along; neither is instantiated here)
typedef int32_t sim_i32x4 __attribute__((vector_size(16)));
typedef int32_t sim_i32x16 __attribute__((vector_size(64)));
inline void __syncthreads() { __builtin_trap(); }
inline sim_i32x16 __builtin_amdgcn_mfma_i32_32x32x32_i8(sim_i32x4, sim_i32x4, sim_i32x16, int, int, int) { __builtin_trap(); }
#include "lce_kernels_transition.h"

namespace {
// d: batch, pool input height, width, channels_in, depth_multiplier; the pool's filter_height, filter_width, stride_height, stride_width,
// pad_height, pad_width; the pooled height and width; the depthwise filter_height, filter_width, stride_height, stride_width, pad_height,
// pad_width; the output height and width.  Fills the geometry of both windows as the entries fill it (pool_window_fill,
// transition_pool_fill) and sets the stride of the grid: pool_vec_grid's, capped at `cap`.  False when a padding so derived is not
// the caller's.
bool fill(lce::PoolArgs& p, lce::TransitionPool& q, const int32_t* d, uint64_t chunk, bool vec, int32_t cap, unsigned* gx) {
  lce::transition_pool_fill(q, d[1], d[2], d[5], d[6], d[7], d[8], d[11], d[12]);
  lce::pool_window_fill(p, d[0], d[11], d[12], d[13], d[14], d[15], d[16], d[19], d[20], (uint64_t)d[3] * (uint64_t)d[4], chunk, vec,
                        /*stream_loads_rule=*/false);
  *gx = lce::pool_vec_grid(vec ? p.total : p.total * 64ull, (uint64_t)cap);
  if (vec) lce::pool_set_stride(p, *gx);
  return q.ph == d[9] && q.pw == d[10] && p.ph == d[17] && p.pw == d[18];
}
// The 16-byte path's rule of both entries: window_vec_rule on the four operands and the footprint's geometry class.
bool vec_rule(const int32_t* d, uint64_t elem_bytes, bool bits, const void* in, const void* filter, const void* third, const void* out) {
  lce::TransitionPool q;
  memset(&q, 0, sizeof q);
  q.fh = d[5]; q.fw = d[6]; q.sh = d[7]; q.sw = d[8];
  return lce::window_vec_rule(d[4], (uint64_t)d[3] * (uint64_t)d[4], elem_bytes, bits, in, filter, third, out) &&
         lce::transition_vec_geometry(q, d[13], d[14]);
}
}  // namespace

// `range`: the pool's activation range (lo, hi), then the depthwise convolution's.  `path`: -1 the entry's rule, 0 the row path.
// `cap`: the most blocks of the launch (the product caps its grid at 2048; a small cap makes the kernels stride).  Returns 1 when the
// launch took the 16-byte path, 0 for the row path, -1 (nothing ran) when a derived padding is not the caller's.
extern "C" int lce_hostsim_transition_f32(const int32_t* d, const float* range, const float* in, const float* filter, const float* bias,
                                          float* out, int32_t* bits, int32_t path, int32_t cap) {
  lce::TransitionArgs a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.D.P;
  const bool vec = path != 0 && vec_rule(d, 4, bits != nullptr, in, filter, bias, out);
  p.in = in; p.out = out; p.bits = (uint32_t*)bits;
  a.D.filter = filter; a.D.bias = bias;
  a.D.channels_in = (uint32_t)d[3];
  a.D.div_multiplier = lce::make_fastdiv((uint32_t)d[4]);
  unsigned gx = 0;
  if (!fill(p, a.Q, d, 4, vec, cap, &gx)) return -1;
  a.Q.lo = range[0]; a.Q.hi = range[1]; p.lo = range[2]; p.hi = range[3];
  if (!vec && bits) sim::launch(gx, 256, [&] { lce::transition_rows<true>(a); });
  else if (!vec) sim::launch(gx, 256, [&] { lce::transition_rows<false>(a); });
  else if (bits) sim::launch(gx, 256, [&] { lce::transition_vec<true>(a); });
  else sim::launch(gx, 256, [&] { lce::transition_vec<false>(a); });
  return vec ? 1 : 0;
}

// `q`: the shared zero point of the pool's input and output, the output zero point, the depthwise convolution's act_min and act_max,
// the pool's act_min and act_max.  `table`: [3][Cout] as lce_hip_depthwise_conv2d_i8_prepare writes it.
extern "C" int lce_hostsim_transition_i8(const int32_t* d, const int32_t* q, const int8_t* in, const int8_t* filter, const int32_t* table,
                                         int8_t* out, int32_t* bits, int32_t path, int32_t cap) {
  lce::TransitionI8Args a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.D.P;
  const bool vec = path != 0 && vec_rule(d, 1, bits != nullptr, in, filter, table, out);
  p.in = in; p.out = out; p.bits = (uint32_t*)bits;
  a.D.filter = filter; a.D.table = table; a.D.zi = q[0];
  a.D.channels_in = (uint32_t)d[3];
  a.D.div_multiplier = lce::make_fastdiv((uint32_t)d[4]);
  unsigned gx = 0;
  if (!fill(p, a.Q, d, 16, vec, cap, &gx)) return -1;
  p.zero_point = q[1]; p.qlo = q[2]; p.qhi = q[3]; a.Q.qlo = q[4]; a.Q.qhi = q[5];
  if (!vec && bits) sim::launch(gx, 256, [&] { lce::transition_i8_rows<true>(a); });
  else if (!vec) sim::launch(gx, 256, [&] { lce::transition_i8_rows<false>(a); });
  else if (bits) sim::launch(gx, 256, [&] { lce::transition_i8_vec<true>(a); });
  else sim::launch(gx, 256, [&] { lce::transition_i8_vec<false>(a); });
  return vec ? 1 : 0;
}
