// A QuickNet transition's MAX_POOL_2D and the DEPTHWISE_CONV_2D that alone reads it (pool 2x2 / 1 SAME, then the 3x3 / 2
// [1 2 1] x [1 2 1] / 16 blur), in ONE launch: the pooled map, as large as the pool's input, is never written
// (include/lce_hip.h, lce_hip_pool_depthwise_f32 / lce_hip_pool_depthwise_i8).  The contract is the composition of the two
// entries' (lce_kernels_pool.h, lce_kernels_depthwise.h, lce_kernels_depthwise_i8.h).  Per output element, over the depthwise
// filter's taps in raster order -- the filter index unclipped, a tap whose POOLED pixel lies outside the pooled map skipped -- the
// tap's operand is the value lce_hip_pool2d would have stored there:
//
//   float : m = -FLT_MAX;  m = (m < x) ? x : m over the pool window's in-bounds taps in raster order;  p = pool_clamp(m, pool range)
//           t = +0.0f;  t = fmaf(p, w[fy][fx][o], t);  t + bias[o];  pool_clamp(t, depthwise range);  bit = v < 0
//   int8  : p = clamp(max over the pool window's in-bounds taps, pool range at (s, z))
//           acc = sum (p - z) * w[fy][fx][o];  depthwise_i8_value(acc, table[0..2][o]);  bit = v < zo
//
// so output and bits are byte-equal to the two launches.  Two paths, siblings of depthwise_vec / depthwise_rows, whose window,
// division, clamp, grid-stride scheme, words of bits and stores they share (TransitionArgs carries a DepthwiseArgs whose PoolArgs
// describes the depthwise window ON THE POOLED MAP -- P.H x P.W are the pooled extents -- and whose `in` is the POOL's input):
//   transition_rows : any geometry -- one wave per 64 output channels of a pixel, one element per lane; for every in-bounds
//                     depthwise tap the lane walks that pooled pixel's clipped pool window, then one fmaf / multiply-add.
//                     This path is the definition.
//   transition_vec  : the QuickNet class -- pool stride 1 x 1, pool filter <= 2 x 2, depthwise filter <= 3 x 3 (any depthwise stride,
//                     any padding), multiplier 1, 16-byte chunks -- where the input footprint of an output pixel is at most 4 x 4.
//                     A lane owns one 16-byte chunk of one output pixel and streams the footprint row by row: the (up to) four
//                     16-byte taps of an input row are loaded ONCE, the three horizontal maxima formed, combined with the previous
//                     row's into one pooled row, which is clamped and fed to the accumulators with that row's three weights.  A
//                     footprint tap outside the image (or beyond the footprint) enters as the reduction's identity, -FLT_MAX /
//                     -128: m = (m < x) ? x : m never takes it, because m starts there and never falls.  The raster order of
//                     each pool window's chain (row, then column) and of the fmaf chain is kept: the second row's two taps
//                     continue the chain the first row's two began.  Plain loads: the footprints of neighbouring outputs overlap
//                     (the pools' measured rule, lce_kernels_pool.h).
// Offsets are 64-bit beyond the window arithmetic.  No LDS, no scratch, nothing allocated: the launch is capturable.  The outputs
// must not overlap anything the launch reads.
#pragma once
#include <stdint.h>

#include "lce_kernels_depthwise.h"
#include "lce_kernels_depthwise_i8.h"

namespace lce {

// The pool in front: its input's extents, its window and its activation range (float: lo, hi; int8: qlo, qhi at the shared
// quantization).  The pooled extents are the depthwise PoolArgs' H x W.
struct TransitionPool {
  int32_t H, W;
  int32_t fh, fw, sh, sw, ph, pw;
  float lo, hi;
  int32_t qlo, qhi;
};
struct TransitionArgs {
  DepthwiseArgs D;
  TransitionPool Q;
};
struct TransitionI8Args {
  DepthwiseI8Args D;        // (D.zi: the zero point of the pooled tensor = the pool's)
  TransitionPool Q;
};

// The geometry class of the 16-byte path (the channel and alignment conditions are the caller's).
inline bool transition_vec_geometry(const TransitionPool& q, int32_t dw_fh, int32_t dw_fw) {
  return q.sh == 1 && q.sw == 1 && q.fh <= 2 && q.fw <= 2 && dw_fh <= 3 && dw_fw <= 3;
}

// The window of the pool in front (everything of `q` but the clamp): input H x W, pooled to pooled_h x pooled_w.
inline void transition_pool_fill(TransitionPool& q, int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t sh, int32_t sw, int32_t pooled_h,
                                 int32_t pooled_w) {
  q.H = H; q.W = W; q.fh = fh; q.fw = fw; q.sh = sh; q.sw = sw;
  q.ph = same_pad_before(pooled_h, sh, fh, H);
  q.pw = same_pad_before(pooled_w, sw, fw, W);
}

// Launch the vector path (vec == true; the caller has checked geometry, sizes and alignment and filled the vector-path fields for
// the grid pool_vec_grid() gives) or the row path on `stream`; the launch's hipError_t as an int.  lce_tu_transition.hip.
int launch_transition(const TransitionArgs& args, bool vec, void* stream);
int launch_transition_i8(const TransitionI8Args& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

constexpr float kTransitionLowest = -3.402823466e+38f;            // -FLT_MAX: where lce_hip_pool2d's MAX starts

// The clipped pool window [y0, y1) x [x0, x1) of pooled pixel (y, x).
LCE_DEVICE void transition_pool_window(const TransitionPool& Q, int32_t y, int32_t x, int32_t& y0, int32_t& y1, int32_t& x0, int32_t& x1) {
  const int32_t ys = y * Q.sh - Q.ph, xs = x * Q.sw - Q.pw;
  y0 = ys < 0 ? 0 : ys;
  y1 = ys + Q.fh > Q.H ? Q.H : ys + Q.fh;
  x0 = xs < 0 ? 0 : xs;
  x1 = xs + Q.fw > Q.W ? Q.W : xs + Q.fw;
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
transition_rows(const TransitionArgs A) {
  const PoolArgs& P = A.D.P;
  const TransitionPool& Q = A.Q;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t segs = P.per_pixel, cols = P.channels, cin = A.D.channels_in;
  const float* in = (const float*)P.in;
  for (uint64_t t = wave0; t < P.total; t += nwaves) {
    const uint64_t pixel = t / segs;                               // < 2^31
    const uint32_t seg = (uint32_t)(t - pixel * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    const PoolWindow w = pool_window(P, (uint32_t)pixel, true);    // on the pooled map
    bool neg = false;
    if (col < cols) {
      const uint32_t ic = fast_div(col, A.D.div_multiplier);       // < cin
      float acc = 0.0f;
      for (int32_t y = w.y0; y < w.y1; ++y) {
        const int64_t tap0 = (int64_t)(y - w.ys) * P.fw - w.xs;    // + x: the filter tap (y - ys, x - xs), unclipped
        for (int32_t x = w.x0; x < w.x1; ++x) {
          int32_t y0, y1, x0, x1;
          transition_pool_window(Q, y, x, y0, y1, x0, x1);
          float m = kTransitionLowest;
          for (int32_t iy = y0; iy < y1; ++iy) {
            const float* row = in + ((uint64_t)w.b * (uint64_t)Q.H + (uint64_t)iy) * (uint64_t)Q.W * cin + ic;
            for (int32_t ix = x0; ix < x1; ++ix) {
              const float e = row[(uint64_t)ix * cin];
              m = m < e ? e : m;
            }
          }
          acc = __builtin_fmaf(pool_clamp(m, Q.lo, Q.hi), A.D.filter[(tap0 + x) * (int64_t)cols + col], acc);
        }
      }
      if (A.D.bias) acc = acc + A.D.bias[col];
      const float r = pool_clamp(acc, P.lo, P.hi);
      if (P.out) ((float*)P.out)[pixel * (uint64_t)cols + col] = r;
      neg = r < 0.0f;
    }
    if constexpr (BITS) store_seg_bits(P.bits, P.wpr, pixel, seg, lane, neg);
  }
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
transition_i8_rows(const TransitionI8Args A) {
  const PoolArgs& P = A.D.P;
  const TransitionPool& Q = A.Q;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t segs = P.per_pixel, cols = P.channels, cin = A.D.channels_in;
  const int8_t* in = (const int8_t*)P.in;
  for (uint64_t t = wave0; t < P.total; t += nwaves) {
    const uint64_t pixel = t / segs;                               // < 2^31
    const uint32_t seg = (uint32_t)(t - pixel * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    const PoolWindow w = pool_window(P, (uint32_t)pixel, true);    // on the pooled map
    bool neg = false;
    if (col < cols) {
      const uint32_t ic = fast_div(col, A.D.div_multiplier);       // < cin
      int32_t acc = 0;
      for (int32_t y = w.y0; y < w.y1; ++y) {
        const int64_t tap0 = (int64_t)(y - w.ys) * P.fw - w.xs;    // + x: the filter tap (y - ys, x - xs), unclipped
        for (int32_t x = w.x0; x < w.x1; ++x) {
          int32_t y0, y1, x0, x1;
          transition_pool_window(Q, y, x, y0, y1, x0, x1);
          int32_t m = -128;
          for (int32_t iy = y0; iy < y1; ++iy) {
            const int8_t* row = in + ((uint64_t)w.b * (uint64_t)Q.H + (uint64_t)iy) * (uint64_t)Q.W * cin + ic;
            for (int32_t ix = x0; ix < x1; ++ix) {
              const int32_t e = (int32_t)row[(uint64_t)ix * cin];
              m = m < e ? e : m;
            }
          }
          acc += add_i8_mul24(pool_clamp(m, Q.qlo, Q.qhi) - A.D.zi, (int32_t)A.D.filter[(tap0 + x) * (int64_t)cols + col]);
        }
      }
      const int32_t r = depthwise_i8_value(acc, A.D.table[col], A.D.table[(uint64_t)cols + col], A.D.table[2ull * cols + col], P.zero_point,
                                           P.qlo, P.qhi);
      if (P.out) ((int8_t*)P.out)[pixel * (uint64_t)cols + col] = (int8_t)r;
      neg = r < P.zero_point;
    }
    if constexpr (BITS) store_seg_bits(P.bits, P.wpr, pixel, seg, lane, neg);
  }
}

// What the two 16-byte kernels share of one lane's footprint: which of its (up to) four input rows and columns exist, which of its
// (up to) three pooled rows and columns are pixels of the pooled map, and the first chunk of the footprint.  Pool stride 1:
// pooled pixel (w.ys + r, w.xs + k) reads input rows w.ys - ph + r + {0 .. fh - 1} and the columns alike, so footprint row i is
// input row w.ys - ph + i and feeds pooled rows i (as its first row) and, with a 2-row pool, i - 1 (as its second).
struct TransitionFootprint {
  int32_t iy0, ix0;          // input row and column of footprint (0, 0); may be negative
  int32_t rows, cols;        // footprint extents: depthwise filter + pool filter - 1, each <= 4 (wave-uniform)
};
LCE_DEVICE TransitionFootprint transition_footprint(const PoolArgs& P, const TransitionPool& Q, const PoolWindow& w) {
  return TransitionFootprint{w.ys - Q.ph, w.xs - Q.pw, P.fh + Q.fh - 1, P.fw + Q.fw - 1};
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
transition_vec(const TransitionArgs A) {
  const PoolArgs& P = A.D.P;
  const TransitionPool& Q = A.Q;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (P.total + 63) / 64;
  const uint32_t cpp = P.per_pixel;
  // (pixel, chunk in the pixel) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint32_t pix0 = (uint32_t)((wave0 * 64ull) / cpp);
  uint32_t c0 = (uint32_t)(wave0 * 64ull - (uint64_t)pix0 * cpp);
  const f32x4* in = (const f32x4*)P.in;
  const f32x4 lowest = {kTransitionLowest, kTransitionLowest, kTransitionLowest, kTransitionLowest};
  const bool two_rows = Q.fh == 2, two_cols = Q.fw == 2;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 64 chunks = 1 KB of output per wave and iteration
    uint64_t g;                                                    // this lane's chunk
    bool ok;
    uint32_t c;
    const PoolWindow w = pool_chunk_at(P, pix0, c0, blk, lane, g, ok, c);   // on the pooled map; a lane past the end has no pooled row
    const TransitionFootprint fp = transition_footprint(P, Q, w);
    const f32x4* flt = (const f32x4*)A.D.filter + c;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 prev[3] = {lowest, lowest, lowest};                      // the chains the previous footprint row began
    const uint64_t image = ok ? (uint64_t)w.b * (uint64_t)Q.H : 0ull;   // (a lane past the end reads image 0 and keeps nothing)
#pragma unroll
    for (int32_t i = 0; i < 4; ++i) {
      if (i >= fp.rows) break;                                     // (wave-uniform)
      // every load below is unconditional, from coordinates clamped into the image, and the VALUE is chosen afterwards: a
      // footprint tap outside the image enters as the reduction's identity
      const int32_t iy = fp.iy0 + i;
      const bool row_in = ok && iy >= 0 && iy < Q.H;
      const f32x4* row = in + (image + (uint64_t)(iy < 0 ? 0 : iy >= Q.H ? Q.H - 1 : iy)) * (uint64_t)Q.W * cpp + c;
      const int32_t r = two_rows ? i - 1 : i;                      // the pooled row this footprint row completes
      const bool feeds = r >= 0 && r < P.fh;                       // (wave-uniform)
      const int32_t py = w.ys + r;
      const bool prow = py >= w.y0 && py < w.y1;
      f32x4 v[4], k[3];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                                // each footprint tap is loaded once
        const int32_t ix = fp.ix0 + j;
        v[j] = lowest;
        if (j < fp.cols) {                                         // (wave-uniform)
          const f32x4 t = row[(uint64_t)(ix < 0 ? 0 : ix >= Q.W ? Q.W - 1 : ix) * cpp];
          v[j] = (row_in && ix >= 0 && ix < Q.W) ? t : lowest;
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        k[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (feeds && j < P.fw) k[j] = flt[((int64_t)r * P.fw + j) * (int64_t)cpp];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const f32x4 a = v[j], b = two_cols ? v[j + 1] : lowest;
        f32x4 first, full;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float m = kTransitionLowest;                             // the chain this row begins (the next row may continue it)
          m = m < a[e] ? a[e] : m;
          m = m < b[e] ? b[e] : m;
          first[e] = m;
          // the chain the previous row began, continued by this row's taps: m = (m < x) ? x : m keeps the FIRST of the values no
          // other exceeds (a NaN is never taken), so continuing with a and b is continuing with the first such of a and b
          full[e] = prev[j][e] < m ? m : prev[j][e];
        }
        const f32x4 pooled = two_rows ? full : first;
        prev[j] = first;
        const int32_t px = w.xs + j;
        const bool feed = feeds && prow && px >= w.x0 && px < w.x1;   // the pooled pixel is one of the pooled map's and a tap
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[e] = feed ? __builtin_fmaf(pool_clamp(pooled[e], Q.lo, Q.hi), k[j][e], acc[e]) : acc[e];
      }
    }
    f32x4 bias = {0.0f, 0.0f, 0.0f, 0.0f};
    if (A.D.bias) bias = ((const f32x4*)A.D.bias)[c];
    f32x4 o;
    uint32_t nib = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = acc[e];
      if (A.D.bias) t = t + bias[e];
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
transition_i8_vec(const TransitionI8Args A) {
  const PoolArgs& P = A.D.P;
  const TransitionPool& Q = A.Q;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (P.total + 63) / 64;
  const uint32_t cpp = P.per_pixel;
  // (pixel, chunk in the pixel) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint32_t pix0 = (uint32_t)((wave0 * 64ull) / cpp);
  uint32_t c0 = (uint32_t)(wave0 * 64ull - (uint64_t)pix0 * cpp);
  const u32x4* in = (const u32x4*)P.in;
  const u32x4 lowest = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};   // sixteen times -128
  const i32x4* table = (const i32x4*)A.D.table;                    // a row is Cout ints = 4 cpp vectors
  const bool two_rows = Q.fh == 2, two_cols = Q.fw == 2;
  const int32_t zi = A.D.zi;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 64 chunks = 1 KB of output per wave and iteration
    uint64_t g;                                                    // this lane's chunk
    bool ok;
    uint32_t c;
    const PoolWindow w = pool_chunk_at(P, pix0, c0, blk, lane, g, ok, c);   // on the pooled map; a lane past the end has no pooled row
    const TransitionFootprint fp = transition_footprint(P, Q, w);
    const u32x4* flt = (const u32x4*)A.D.filter + c;
    int32_t acc[16];
    int32_t prev[3][16];                                           // the previous footprint row's horizontal maxima
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0, prev[0][e] = prev[1][e] = prev[2][e] = -128;
    const uint64_t image = ok ? (uint64_t)w.b * (uint64_t)Q.H : 0ull;   // (a lane past the end reads image 0 and keeps nothing)
    for (int32_t i = 0; i < fp.rows; ++i) {
      // every load below is unconditional, from coordinates clamped into the image, and the VALUE is chosen afterwards: a
      // footprint tap outside the image enters as the reduction's identity
      const int32_t iy = fp.iy0 + i;
      const bool row_in = ok && iy >= 0 && iy < Q.H;
      const u32x4* row = in + (image + (uint64_t)(iy < 0 ? 0 : iy >= Q.H ? Q.H - 1 : iy)) * (uint64_t)Q.W * cpp + c;
      const int32_t r = two_rows ? i - 1 : i;                      // the pooled row this footprint row completes
      const bool feeds = r >= 0 && r < P.fh;                       // (wave-uniform)
      const int32_t py = w.ys + r;
      const bool prow = py >= w.y0 && py < w.y1;
      u32x4 v[4], k[3];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                                // each footprint tap is loaded once ...
        const int32_t ix = fp.ix0 + j;
        v[j] = lowest;
        if (j < fp.cols) {                                         // (wave-uniform)
          const u32x4 t = row[(uint64_t)(ix < 0 ? 0 : ix >= Q.W ? Q.W - 1 : ix) * cpp];
          v[j] = (row_in && ix >= 0 && ix < Q.W) ? t : lowest;
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        k[j] = u32x4{0u, 0u, 0u, 0u};
        if (feeds && j < P.fw) k[j] = flt[((int64_t)r * P.fw + j) * (int64_t)cpp];
      }
      int32_t u[4][16];                                            // ... and each of its bytes unpacked once
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) u[j][e] = (int32_t)(int8_t)(v[j][e >> 2] >> (8 * (e & 3)));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int32_t px = w.xs + j;
        const bool feed = feeds && prow && px >= w.x0 && px < w.x1;   // the pooled pixel is one of the pooled map's and a tap
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int32_t b = two_cols ? u[j + 1][e] : -128;
          const int32_t first = u[j][e] < b ? b : u[j][e];
          const int32_t full = prev[j][e] < first ? first : prev[j][e];
          const int32_t pooled = pool_clamp(two_rows ? full : first, Q.qlo, Q.qhi);
          prev[j][e] = first;
          const int32_t we = (int32_t)(int8_t)(k[j][e >> 2] >> (8 * (e & 3)));
          acc[e] += add_i8_mul24(feed ? pooled - zi : 0, we);
        }
      }
    }
    u32x4 o;
    uint32_t m = 0;                                                // 16 bits
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const i32x4 bias = table[4ull * c + d], mul = table[4ull * cpp + 4ull * c + d], exp = table[8ull * cpp + 4ull * c + d];
      int32_t rr[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        rr[e] = depthwise_i8_value(acc[4 * d + e], bias[e], mul[e], exp[e], P.zero_point, P.qlo, P.qhi);
        m |= ((uint32_t)(rr[e] - P.zero_point) >> 31) << (4 * d + e);
      }
      o[d] = pack4_u8(rr[0], rr[1], rr[2], rr[3]);
    }
    if (P.out && ok) pool_store_through((u32x4*)P.out + g, o);
    if constexpr (BITS) store_half_word<true>(P.bits, g, lane, ok, m);   // per_pixel % 2 == 0: lanes 2p and 2p + 1 agree on ok
    pool_chunk_step(P, pix0, c0);
  }
}

}  // namespace lce
#endif  // __HIPCC__
