// The float depthwise convolution between binary layers of a converted network (QuickNet's transition blurs its pooled map
// with a fixed 3x3 / 2 [1 2 1] x [1 2 1] / 16 filter in front of the 1x1 convolution): TFLite's builtin DEPTHWISE_CONV_2D and the
// LceQuantize of its result, in one pass (include/lce_hip.h, lce_hip_depthwise_conv2d_f32).  NHWC [B, H, W, Cin] ->
// [B, OH, OW, Cout], Cout = Cin x m (the depth multiplier); filter [1, fh, fw, Cout], bias [Cout] or none; any filter and
// stride, SAME or VALID with the pools' padding rule (pad_before = total / 2); dilation 1.  Output channel o reads input
// channel o / m.  Per output element, over its in-bounds taps in raster order (filter row, then filter column) -- taps in
// the padding are skipped, the filter index is the unclipped one:
//
//   t = +0.0f;  t = fmaf(x[y][x][o / m], w[fy][fx][o], t)      one rounding per tap (__builtin_fmaf: no contraction flag decides)
//   t = t + bias[o]                                             one float32 add; skipped without a bias
//   v = min(max(t, lo), hi)                                     pool_clamp (a NaN passes, -0.0 stays -0.0)
//   bits: bit = v < 0, LSB first, ceil(Cout / 32) words per pixel, padding bits 0, from the registers of the pass
//
// Two paths, siblings of pool_vec / pool_rows (lce_kernels_pool.h), whose window, division, clamp and grid-stride scheme
// they share (DepthwiseArgs carries a PoolArgs):
//   depthwise_vec  : m == 1, C % 4 == 0, input, filter, bias and output 16-byte aligned (and, with bits, C % 32 == 0) -- a
//                    lane owns one 16-byte chunk of one output pixel: four independent fmaf chains.  A window row is walked
//                    with 16-byte loads, up to four taps in flight; the lane's weights w[fy][fx][c .. c + 3] are 16-byte loads
//                    through the cache beside each input tap (the filter is a few KB and every wave reads all of it).
//                    Bits: 8 lanes per word (store_nibble_word).  Streaming stores.
//   depthwise_rows : anything else (ragged C, m > 1, unaligned pointers, bits on C % 32 != 0) -- one wave per 64 output
//                    channels of a pixel, one element per lane, one ballot per two words.
// Offsets are 64-bit beyond the window arithmetic.  No LDS, no scratch, nothing allocated: the launch is capturable.  The
// outputs must not overlap anything the launch reads.
// depthwise_vec<BITS, STAGED = true> is the A/B partner of the shipped form for tools/probes/depthwise_loads.hip: the whole
// filter copied into (dynamic) LDS once per block and read from there.  The library never launches it.
#pragma once
#include <stdint.h>

#include "lce_kernels_pool.h"

namespace lce {

struct DepthwiseArgs {
  PoolArgs P;                // geometry, outputs, clamp and grid stride as the pools' (channels = Cout; in, out, bits; lo, hi)
  const float* filter;       // [fh][fw][Cout]
  const float* bias;         // [Cout]; null: none
  uint32_t channels_in;      // Cin = Cout / multiplier
  FastDiv div_multiplier;    // o / multiplier
};

// Launches the vector path (vec == true; the caller has checked sizes, the multiplier and alignment and filled P's
// vector-path fields for the grid pool_vec_grid() gives) or the row path on `stream`; returns the launch's hipError_t as an
// int.  Defined in lce_tu_depthwise.hip.
int launch_depthwise(const DepthwiseArgs& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// One lane's walk over its window for the 16-byte chunk c of every pixel: four fmaf chains in acc.  NT: non-temporal input
// loads (a separate instantiation behind a wave-uniform branch, as pool_walk_chunk); the weights always take plain loads.
template <bool NT, bool STAGED>
LCE_DEVICE void depthwise_walk_chunk(const DepthwiseArgs& A, const PoolWindow& w, uint32_t c, const f32x4* staged, float (&acc)[4]) {
  const PoolArgs& P = A.P;
  const f32x4* in = (const f32x4*)P.in;
  const f32x4* flt = (STAGED ? staged : (const f32x4*)A.filter) + c;
  const uint32_t cpp = P.per_pixel;
  for (int32_t y = w.y0; y < w.y1; ++y) {
    const f32x4* row = in + ((uint64_t)w.b * (uint64_t)P.H + (uint64_t)y) * (uint64_t)P.W * cpp + c;
    const int64_t tap0 = (int64_t)(y - w.ys) * P.fw - w.xs;        // + x: the filter tap (y - ys, x - xs), unclipped
    for (int32_t x4 = w.x0; x4 < w.x1; x4 += 4) {                  // up to four taps of the row in flight, then chained
      f32x4 v[4], k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool tap = x4 + j < w.x1;
        const f32x4* p = row + (uint64_t)(x4 + j) * cpp;
        v[j] = tap ? (NT ? load_streaming(p) : *p) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        k[j] = tap ? flt[(tap0 + x4 + j) * (int64_t)cpp] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool tap = x4 + j < w.x1;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = tap ? __builtin_fmaf(v[j][e], k[j][e], acc[e]) : acc[e];
      }
    }
  }
}

template <bool BITS, bool STAGED = false>
LCE_KERNEL void __launch_bounds__(256)
depthwise_vec(const DepthwiseArgs A) {
  const PoolArgs& P = A.P;
  extern __shared__ __attribute__((aligned(16))) float depthwise_lds[];
  if constexpr (STAGED) {                                          // the whole filter, once per block
    const uint32_t n = (uint32_t)(P.fh * P.fw) * P.per_pixel;
    for (uint32_t i = thread_idx_x(); i < n; i += block_dim_x()) ((f32x4*)depthwise_lds)[i] = ((const f32x4*)A.filter)[i];
    __syncthreads();
  }
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (P.total + 63) / 64;
  const uint32_t cpp = P.per_pixel;
  // (pixel, chunk in the pixel) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint32_t pix0 = (uint32_t)((wave0 * 64ull) / cpp);
  uint32_t c0 = (uint32_t)(wave0 * 64ull - (uint64_t)pix0 * cpp);
  const bool nt = P.stream_loads != 0u;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 64 chunks = 1 KB of output per wave and iteration
    uint64_t g;                                                    // this lane's chunk
    bool ok;
    uint32_t c;
    const PoolWindow w = pool_chunk_at(P, pix0, c0, blk, lane, g, ok, c);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (nt) depthwise_walk_chunk<true, STAGED>(A, w, c, (const f32x4*)depthwise_lds, acc);
    else depthwise_walk_chunk<false, STAGED>(A, w, c, (const f32x4*)depthwise_lds, acc);
    f32x4 bias = {0.0f, 0.0f, 0.0f, 0.0f};
    if (A.bias) bias = ((const f32x4*)A.bias)[c];
    f32x4 o;
    uint32_t nib = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = acc[e];
      if (A.bias) t = t + bias[e];
      o[e] = pool_clamp(t, P.lo, P.hi);
      nib |= (o[e] < 0.0f ? 1u : 0u) << e;
    }
    if (P.out && ok) store_streaming((f32x4*)P.out + g, o);
    if constexpr (BITS) store_nibble_word(P.bits, g, lane, ok, nib);   // per_pixel % 8 == 0: the 8 lanes of a word agree on ok
    pool_chunk_step(P, pix0, c0);
  }
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
depthwise_rows(const DepthwiseArgs A) {
  const PoolArgs& P = A.P;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t segs = P.per_pixel, cols = P.channels, cin = A.channels_in;
  const float* in = (const float*)P.in;
  for (uint64_t t = wave0; t < P.total; t += nwaves) {
    const uint64_t pixel = t / segs;                               // < 2^31
    const uint32_t seg = (uint32_t)(t - pixel * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    const PoolWindow w = pool_window(P, (uint32_t)pixel, true);
    bool neg = false;
    if (col < cols) {
      const uint32_t ic = fast_div(col, A.div_multiplier);         // < cin
      float acc = 0.0f;
      for (int32_t y = w.y0; y < w.y1; ++y) {
        const float* row = in + ((uint64_t)w.b * (uint64_t)P.H + (uint64_t)y) * (uint64_t)P.W * cin + ic;
        const int64_t tap0 = (int64_t)(y - w.ys) * P.fw - w.xs;    // + x: the filter tap (y - ys, x - xs), unclipped
        for (int32_t x = w.x0; x < w.x1; ++x)
          acc = __builtin_fmaf(row[(uint64_t)x * cin], A.filter[(tap0 + x) * (int64_t)cols + col], acc);
      }
      if (A.bias) acc = acc + A.bias[col];
      const float r = pool_clamp(acc, P.lo, P.hi);
      if (P.out) ((float*)P.out)[pixel * (uint64_t)cols + col] = r;
      neg = r < 0.0f;
    }
    if constexpr (BITS) store_seg_bits(P.bits, P.wpr, pixel, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
