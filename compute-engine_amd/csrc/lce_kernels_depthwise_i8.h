// The quantized (int8) depthwise convolution of an int8-converted network (QuickNet's transition blurs its pooled map with a
// fixed 3x3 / 2 [1 2 1] x [1 2 1] / 16 filter; its stem has a depthwise 3x3 / 2): TFLite's builtin DEPTHWISE_CONV_2D on int8
// tensors and the LceQuantize of its result, in one launch (include/lce_hip.h, lce_hip_depthwise_conv2d_i8).  Geometry is the
// float entry's (lce_kernels_depthwise.h): NHWC [B, H, W, Cin] -> [B, OH, OW, Cout], Cout = Cin x m, filter [1, fh, fw, Cout] with
// zero point 0, output channel o reads input channel o / m, the pools' padding rule, dilation 1.
// reference_integer_ops::DepthwiseConvPerChannel in its default (double-rounding) build, per output element:
//
//   acc = sum over IN-BOUNDS taps (fy, fx) of (x[iy][ix][o / m] - zi) * w[fy][fx][o]          exact, int32; the filter index unclipped
//   acc += bias[o]                                                                            table row 0 (0 without a bias)
//   acc = RDivPOT(SRDHM(acc * 2^max(e, 0), m[o]), max(-e[o], 0))                              table rows 1 and 2: conv2d_i8_requantize
//   v   = min(max(acc + zo, act_min), act_max);   bit = v < zo, LSB first, ceil(Cout / 32) words per pixel, padding bits 0
//
// Two paths, siblings of depthwise_vec / depthwise_rows and of the pools' int8 path, whose window, division, grid-stride scheme,
// 16-byte int8 store (lce_kernels_pool.h) and two-lane word (store_half_word) they share (DepthwiseI8Args carries a PoolArgs):
//   depthwise_i8_vec  : m == 1, C % 16 == 0, input, filter, table and output 16-byte aligned (and, with bits, C % 32 == 0) -- a
//                       lane owns one 16-byte chunk (16 channels) of one output pixel: 16 int32 accumulators.  Each tap of the
//                       CLIPPED window is one 16-byte load of the input and one of w[fy][fx][c .. c + 15], up to four taps of a
//                       window row in flight; a byte is sign-extended, zi subtracted, and multiplied-added in 24 bits
//                       (|x - zi| <= 255, |w| <= 128).  The lane's bias, multipliers and exponents are twelve 16-byte loads.
//   depthwise_i8_rows : anything else (ragged C, m > 1, unaligned pointers, bits on C % 32 != 0) -- one wave per 64 output
//                       channels of a pixel, one element per lane, one ballot per two words.
// Offsets are 64-bit beyond the window arithmetic.  No LDS, no scratch, nothing allocated: the launch is capturable.  The
// outputs must not overlap anything the launch reads.
#pragma once
#include <stdint.h>

#include "lce_kernels_conv2d_i8.h"   // conv2d_i8_requantize (with lce_kernels_eltwise_i8.h's two gemmlowp steps)
#include "lce_kernels_pool.h"

namespace lce {

struct DepthwiseI8Args {
  PoolArgs P;                // geometry, outputs and grid stride as the pools' (channels = Cout; in, out, bits; qlo, qhi = the
                             // activation range at (so, zo); zero_point = zo)
  const int8_t* filter;      // [fh][fw][Cout]
  const int32_t* table;      // [3][Cout]: bias[o], m[o], e[o] (lce_hip_depthwise_conv2d_i8_prepare)
  int32_t zi;                // the input zero point
  uint32_t channels_in;      // Cin = Cout / multiplier
  FastDiv div_multiplier;    // o / multiplier
};

// Launches the vector path (vec == true; the caller has checked sizes, the multiplier and alignment and filled P's
// vector-path fields for the grid pool_vec_grid() gives) or the row path on `stream`; returns the launch's hipError_t as an
// int.  Defined in lce_tu_depthwise_i8.hip.
int launch_depthwise_i8(const DepthwiseI8Args& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// One output element from its accumulator and its channel's three constants.
LCE_DEVICE int32_t depthwise_i8_value(int32_t acc, int32_t bias, int32_t mul, int32_t exp, int32_t zo, int32_t lo, int32_t hi) {
  return pool_clamp(conv2d_i8_requantize(acc + bias, mul, exp) + zo, lo, hi);
}

// One lane's walk over its clipped window for the 16-byte chunk c of every pixel: the 16 sums of (x - zi) * w in acc.  NT:
// non-temporal input loads (a separate instantiation behind a wave-uniform branch, as pool_walk_chunk); the weights always take
// plain loads.
template <bool NT>
LCE_DEVICE void depthwise_i8_walk_chunk(const DepthwiseI8Args& A, const PoolWindow& w, uint32_t c, int32_t (&acc)[16]) {
  const PoolArgs& P = A.P;
  const u32x4* in = (const u32x4*)P.in;
  const u32x4* flt = (const u32x4*)A.filter + c;
  const uint32_t cpp = P.per_pixel;
  const int32_t zi = A.zi;
  for (int32_t y = w.y0; y < w.y1; ++y) {
    const u32x4* row = in + ((uint64_t)w.b * (uint64_t)P.H + (uint64_t)y) * (uint64_t)P.W * cpp + c;
    const int64_t tap0 = (int64_t)(y - w.ys) * P.fw - w.xs;        // + x: the filter tap (y - ys, x - xs), unclipped
    for (int32_t x4 = w.x0; x4 < w.x1; x4 += 4) {                  // up to four taps of the row in flight, then accumulated
      u32x4 v[4], k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool tap = x4 + j < w.x1;
        const u32x4* p = row + (uint64_t)(x4 + j) * cpp;
        v[j] = tap ? (NT ? load_streaming(p) : *p) : u32x4{0u, 0u, 0u, 0u};
        k[j] = tap ? flt[(tap0 + x4 + j) * (int64_t)cpp] : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x4 + j < w.x1) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int32_t xe = (int32_t)(int8_t)(v[j][e >> 2] >> (8 * (e & 3)));
            const int32_t we = (int32_t)(int8_t)(k[j][e >> 2] >> (8 * (e & 3)));
            acc[e] += add_i8_mul24(xe - zi, we);
          }
        }
      }
    }
  }
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
depthwise_i8_vec(const DepthwiseI8Args A) {
  const PoolArgs& P = A.P;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (P.total + 63) / 64;
  const uint32_t cpp = P.per_pixel;
  // (pixel, chunk in the pixel) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint32_t pix0 = (uint32_t)((wave0 * 64ull) / cpp);
  uint32_t c0 = (uint32_t)(wave0 * 64ull - (uint64_t)pix0 * cpp);
  const bool nt = P.stream_loads != 0u;
  const i32x4* table = (const i32x4*)A.table;                      // a row is Cout ints = 4 cpp vectors
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 64 chunks = 1 KB of output per wave and iteration
    uint64_t g;                                                    // this lane's chunk
    bool ok;
    uint32_t c;
    const PoolWindow w = pool_chunk_at(P, pix0, c0, blk, lane, g, ok, c);
    int32_t acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    if (nt) depthwise_i8_walk_chunk<true>(A, w, c, acc);
    else depthwise_i8_walk_chunk<false>(A, w, c, acc);
    u32x4 o;
    uint32_t m = 0;                                                // 16 bits
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const i32x4 bias = table[4ull * c + d], mul = table[4ull * cpp + 4ull * c + d], exp = table[8ull * cpp + 4ull * c + d];
      int32_t r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r[e] = depthwise_i8_value(acc[4 * d + e], bias[e], mul[e], exp[e], P.zero_point, P.qlo, P.qhi);
        m |= ((uint32_t)(r[e] - P.zero_point) >> 31) << (4 * d + e);
      }
      o[d] = pack4_u8(r[0], r[1], r[2], r[3]);
    }
    if (P.out && ok) pool_store_through((u32x4*)P.out + g, o);
    if constexpr (BITS) store_half_word<true>(P.bits, g, lane, ok, m);   // per_pixel % 2 == 0: lanes 2p and 2p + 1 agree on ok
    pool_chunk_step(P, pix0, c0);
  }
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
depthwise_i8_rows(const DepthwiseI8Args A) {
  const PoolArgs& P = A.P;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t segs = P.per_pixel, cols = P.channels, cin = A.channels_in;
  const int8_t* in = (const int8_t*)P.in;
  for (uint64_t t = wave0; t < P.total; t += nwaves) {
    const uint64_t pixel = t / segs;                               // < 2^31
    const uint32_t seg = (uint32_t)(t - pixel * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    const PoolWindow w = pool_window(P, (uint32_t)pixel, true);
    bool neg = false;
    if (col < cols) {
      const uint32_t ic = fast_div(col, A.div_multiplier);         // < cin
      int32_t acc = 0;
      for (int32_t y = w.y0; y < w.y1; ++y) {
        const int8_t* row = in + ((uint64_t)w.b * (uint64_t)P.H + (uint64_t)y) * (uint64_t)P.W * cin + ic;
        const int64_t tap0 = (int64_t)(y - w.ys) * P.fw - w.xs;    // + x: the filter tap (y - ys, x - xs), unclipped
        for (int32_t x = w.x0; x < w.x1; ++x)
          acc += add_i8_mul24((int32_t)row[(uint64_t)x * cin] - A.zi, (int32_t)A.filter[(tap0 + x) * (int64_t)cols + col]);
      }
      const int32_t r = depthwise_i8_value(acc, A.table[col], A.table[(uint64_t)cols + col], A.table[2ull * cols + col], P.zero_point,
                                           P.qlo, P.qhi);
      if (P.out) ((int8_t*)P.out)[pixel * (uint64_t)cols + col] = (int8_t)r;
      neg = r < P.zero_point;
    }
    if constexpr (BITS) store_seg_bits(P.bits, P.wpr, pixel, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
