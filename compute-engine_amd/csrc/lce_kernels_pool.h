// The 2-D pooling between binary layers of a converted network (BinaryAlexNet / XNOR-Net / DoReFa-Net pool 3x3 / 2 behind a
// float LceBconv2d; a dense network's transition and the downsampling shortcuts of Bi-RealNet pool 2x2 / 2): TFLite's builtin
// MAX_POOL_2D / AVERAGE_POOL_2D and the LceQuantize of the pooled tensor, in one pass (include/lce_hip.h, lce_hip_pool2d).
// NHWC [B, H, W, C] -> [B, OH, OW, C], float32 or int8, any filter and stride, SAME or VALID with TFLite's padding rule
// (pad_before = total / 2).  Taps outside the image are EXCLUDED (not zero).  Per output element, over its in-bounds taps in
// raster order (filter row, then filter column), as TFLite's reference kernels (reference/pooling.h, integer_ops/pooling.h):
//
//   float MAX     : m = -FLT_MAX;  m = (m < x) ? x : m      (a NaN never replaces m; a window of NaN / -inf gives -FLT_MAX)
//   float AVERAGE : t = 0.0f;  t += x  (one rounding per add, no reassociation);  t / (float)count  (IEEE division)
//   int8 MAX      : the maximum
//   int8 AVERAGE  : a = sum (int32), n = count;  q = a > 0 ? (a + n / 2) / n : (a - n / 2) / n  (C's truncating division),
//                   computed as (int)((float)(a +- n / 2) / (float)n): exact, because |a| + n / 2 < 2^24 makes both operands
//                   exact floats and a correctly rounded quotient cannot reach the next integer (that would need
//                   n (k + 1) > 2^25) -- the host refuses filters above kPoolMaxTaps taps
//   then v = min(max(v, lo), hi) with std::max(a, b) = a < b ? b : a (a float NaN passes, -0.0 stays -0.0)
//   bits: bit = v < 0 (float) / v < zero_point (int8), LSB first, ceil(C / 32) words per pixel, padding bits 0 (what
//         lce_hip_bitpack writes for the pooled tensor), from the values the pass holds in registers
//
// Two paths, chosen as lce_hip_concat chooses:
//   pool_vec  : C x element size a multiple of 16 bytes, both tensors 16-byte aligned (and, with bits, C a multiple of 32)
//               -- the OUTPUT is one flat array of 16-byte chunks and a lane owns one chunk.  The (pixel, chunk in pixel)
//               of a wave's first chunk is divided out ONCE per wave and then advanced by the grid stride, whose quotient
//               and remainder the host supplies; a lane's own offset (< 64 chunks) and the pixel's (b, oy, ox) take
//               multiply-highs.  A lane walks its window with 16-byte loads, up to four taps of a window row in flight
//               before they are reduced.  Float: a chunk is 4 sign bits, 8 neighbouring lanes make a word
//               (store_nibble_word).  int8: a chunk is 16 bits, 2 neighbouring lanes make a word (store_half_word).
//   pool_rows : anything else (ragged C, unaligned pointers, bits on C % 32 != 0) -- one wave per 64 channels of an output
//               pixel, one element per lane, one ballot per two words (store_seg_bits).
// All offsets are 64-bit (output pixels < 2^31, C < 2^31, their product and the input's unbounded).  No LDS, no scratch,
// nothing allocated: the launch is capturable.  The output must not overlap the input.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"

namespace lce {

enum { kPoolF32 = 0, kPoolI8 = 1 };             // element kinds
enum { kPoolMax = 0, kPoolAverage = 1 };        // lce_hip_pool_op
constexpr int kPoolMaxTaps = 1 << 16;           // filter_height x filter_width: 128.5 x 2^16 < 2^24 (the int8 AVERAGE above)

struct PoolArgs {
  const void* in;
  void* out;                 // null: no pooled tensor
  uint32_t* bits;            // null: no LceQuantize output
  int32_t H, W, OH, OW;
  int32_t fh, fw, sh, sw, ph, pw;
  uint32_t channels;
  uint32_t wpr;              // ceil(channels / 32)
  uint32_t per_pixel;        // vector path: 16-byte chunks per pixel; row path: 64-channel segments per pixel
  uint32_t stream_loads;     // non-temporal window loads: set for windows that do not overlap (every input byte is read once: 2-3 us
                             // faster at 256x28x28x256 2x2 / 2), clear for overlapping ones (plain loads 7-11 us faster at 3x3 / 2;
                             // tools/probes/pool_loads.hip, profiles/r12/pool_sections.txt)
  uint64_t total;            // output pixels * per_pixel
  float lo, hi;              // CalculateActivationRange (float)
  int32_t qlo, qhi;          // CalculateActivationRangeQuantized (int8)
  int32_t zero_point;
  // vector path: the grid stride in chunks = step_pixels * per_pixel + step_chunks
  uint32_t step_pixels, step_chunks;
  FastDiv div_per_pixel, div_ow, div_oh;
};

// The 16-byte-path rule of every pass on PoolArgs: depth multiplier 1 (a pool: 1), a pixel a whole number of 16-byte chunks, the
// operands `p0`..`p3` (0: none) 16-byte aligned and, with bits, C % 32 == 0 (a word of bits would straddle pixels of chunks).
inline bool window_vec_rule(int32_t depth_multiplier, uint64_t channels, uint64_t elem_bytes, bool has_bits, const void* p0, const void* p1,
                            const void* p2, const void* p3) {
  return depth_multiplier == 1 && (channels * elem_bytes) % 16 == 0 &&
         ((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3) % 16 == 0 && !(has_bits && channels % 32 != 0);
}

// The window geometry of `p` (everything but the pointers, the clamp and the grid stride) for the output extents of the entry's
// check; `chunk_elems` elements make a 16-byte chunk.  `stream_loads_rule`: false leaves stream_loads 0 (the transitions).
inline void pool_window_fill(PoolArgs& p, int32_t batch, int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t sh, int32_t sw, int32_t OH,
                             int32_t OW, uint64_t channels, uint64_t chunk_elems, bool vec, bool stream_loads_rule) {
  p.H = H; p.W = W; p.OH = OH; p.OW = OW; p.fh = fh; p.fw = fw; p.sh = sh; p.sw = sw;
  p.ph = same_pad_before(OH, sh, fh, H);
  p.pw = same_pad_before(OW, sw, fw, W);
  p.channels = (uint32_t)channels;
  p.wpr = (uint32_t)((channels + 31) / 32);
  p.per_pixel = (uint32_t)(vec ? channels / chunk_elems : (channels + 63) / 64);
  p.stream_loads = stream_loads_rule && sh >= fh && sw >= fw ? 1u : 0u;
  p.total = (uint64_t)batch * OH * OW * p.per_pixel;
  p.div_ow = make_fastdiv((uint32_t)OW); p.div_oh = make_fastdiv((uint32_t)OH);
}

// Blocks of 4 waves for `total_chunks` chunks, 64 per wave task (a row-path launch passes its segments * 64); at most `cap`.
inline unsigned pool_vec_grid(uint64_t total_chunks, uint64_t cap = 2048) { return stream_grid((total_chunks + 63) / 64, 4, cap); }

// The grid stepping of the 16-byte-chunk kernels on `blocks` blocks: what one grid step advances, in pixels and chunks.
inline void pool_set_stride(PoolArgs& p, unsigned blocks) {
  const uint64_t stride = (uint64_t)blocks * 4ull * 64ull;       // chunks per grid step
  p.step_pixels = (uint32_t)(stride / p.per_pixel);
  p.step_chunks = (uint32_t)(stride % p.per_pixel);
  p.div_per_pixel = make_fastdiv(p.per_pixel);
}

// Launches the vector path (vec == true; the caller has checked sizes and alignment and set the stride for the grid
// pool_vec_grid() gives) or the row path on `stream`; returns the launch's hipError_t as an int.  Defined in lce_tu_pool.hip.
int launch_pool(const PoolArgs& args, int kind, int op, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
#include <type_traits>

#include "lce_device_intrinsics.h"

namespace lce {
using namespace lce_dev;

// 16-byte write-through store (sc1), the project's convention for int8 rows (lce_device_intrinsics.h, buf_store) on a flat
// 64-bit address.  Nothing reads it back in this kernel, so nothing waits for it; the s_nop keeps the data registers
// untouched until the store has read them.
LCE_DEVICE void pool_store_through(u32x4* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}

// The window of one output pixel, clipped to the image: rows [y0, y1), columns [x0, x1) of image b.  (ys, xs): its
// unclipped first row and column (what a filter tap's index counts from: lce_kernels_depthwise.h).
struct PoolWindow {
  uint32_t b;
  int32_t y0, y1, x0, x1;
  int32_t ys, xs;
};
LCE_DEVICE PoolWindow pool_window(const PoolArgs& A, uint32_t pixel, bool ok) {
  const uint32_t row = fast_div(pixel, A.div_ow);                  // b * OH + oy
  const int32_t ox = (int32_t)(pixel - row * (uint32_t)A.OW);
  PoolWindow w;
  w.b = fast_div(row, A.div_oh);
  const int32_t oy = (int32_t)(row - w.b * (uint32_t)A.OH);
  const int32_t ys = oy * A.sh - A.ph, xs = ox * A.sw - A.pw;
  w.y0 = ys < 0 ? 0 : ys;
  w.y1 = ys + A.fh > A.H ? A.H : ys + A.fh;
  w.x0 = xs < 0 ? 0 : xs;
  w.x1 = xs + A.fw > A.W ? A.W : xs + A.fw;
  w.ys = ys;
  w.xs = xs;
  if (!ok) w.y1 = w.y0;                                            // (a lane past the end walks nothing)
  return w;
}

// The 16-byte-chunk kernels on PoolArgs: a wave's first chunk of an iteration is chunk c0 of pixel pix0, and lane l owns chunk
// blk * 64 + l of the launch.  That chunk `g`, whether it exists (`ok`), its place `c` < per_pixel in its pixel (also for a lane
// past the end) and the pixel's window.  Any lanes may be active; pix0, c0 and blk are the wave's.
LCE_DEVICE PoolWindow pool_chunk_at(const PoolArgs& P, uint32_t pix0, uint32_t c0, uint64_t blk, int lane, uint64_t& g, bool& ok, uint32_t& c) {
  g = blk * 64ull + (uint64_t)lane;
  ok = g < P.total;
  const uint32_t x = c0 + (uint32_t)lane;                          // < per_pixel + 64 < 2^31
  const uint32_t q = fast_div(x, P.div_per_pixel);
  c = x - q * P.per_pixel;
  return pool_window(P, pix0 + q, ok);
}
// ... and the wave's first chunk one grid step on (pool_set_stride).  Wave-uniform.
LCE_DEVICE void pool_chunk_step(const PoolArgs& P, uint32_t& pix0, uint32_t& c0) {
  pix0 += P.step_pixels;
  c0 += P.step_chunks;
  if (c0 >= P.per_pixel) { c0 -= P.per_pixel; ++pix0; }
}

LCE_DEVICE float pool_clamp(float v, float lo, float hi) {
  v = v < lo ? lo : v;          // std::max(v, lo)
  return hi < v ? hi : v;       // std::min(v, hi)
}
LCE_DEVICE int32_t pool_clamp(int32_t v, int32_t lo, int32_t hi) {
  v = v < lo ? lo : v;
  return hi < v ? hi : v;
}
// int8 AVERAGE: the rounded quotient of the header comment
LCE_DEVICE int32_t pool_round_div(int32_t a, int32_t n) {
  const int32_t x = a > 0 ? a + (n >> 1) : a - (n >> 1);
  return (int32_t)((float)x / (float)n);
}

// One lane's walk over its window for one 16-byte chunk (chunk c of every pixel): the reduction of the header comment into
// facc (float) or iacc (int8).  NT: non-temporal loads.  The two forms are separate instantiations behind a wave-uniform
// branch -- a select between the two loads of one address would be folded into a plain load.
template <int KIND, int OP, bool NT, int N>
LCE_DEVICE void pool_walk_chunk(const PoolArgs& A, const PoolWindow& w, uint32_t c, float (&facc)[N], int32_t (&iacc)[N]) {
  const u32x4* in = (const u32x4*)A.in;
  const uint32_t cpp = A.per_pixel;
  for (int32_t y = w.y0; y < w.y1; ++y) {
    const u32x4* row = in + ((uint64_t)w.b * (uint64_t)A.H + (uint64_t)y) * (uint64_t)A.W * cpp + c;
    for (int32_t x4 = w.x0; x4 < w.x1; x4 += 4) {                  // up to four taps of the row in flight, then reduced
      u32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x4* p = row + (uint64_t)(x4 + j) * cpp;
        v[j] = x4 + j < w.x1 ? (NT ? load_streaming(p) : *p) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool tap = x4 + j < w.x1;
        if constexpr (KIND == kPoolF32) {
          const f32x4 f = __builtin_bit_cast(f32x4, v[j]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if constexpr (OP == kPoolMax) facc[k] = (tap && facc[k] < f[k]) ? f[k] : facc[k];
            else facc[k] = tap ? facc[k] + f[k] : facc[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const int32_t e = (int32_t)(int8_t)(v[j][k >> 2] >> (8 * (k & 3)));
            if constexpr (OP == kPoolMax) iacc[k] = (tap && iacc[k] < e) ? e : iacc[k];
            else iacc[k] = tap ? iacc[k] + e : iacc[k];
          }
        }
      }
    }
  }
}

template <int KIND, int OP, bool BITS>
LCE_KERNEL void __launch_bounds__(256)
pool_vec(const PoolArgs A) {
  constexpr int kAcc = KIND == kPoolF32 ? 4 : 16;                  // elements of a chunk
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (A.total + 63) / 64;
  const uint32_t cpp = A.per_pixel;
  // (pixel, chunk in the pixel) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint32_t pix0 = (uint32_t)((wave0 * 64ull) / cpp);
  uint32_t c0 = (uint32_t)(wave0 * 64ull - (uint64_t)pix0 * cpp);
  const bool nt = A.stream_loads != 0u;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 64 chunks = 1 KB of output per wave and iteration
    uint64_t g;                                                    // this lane's chunk
    bool ok;
    uint32_t c;
    const PoolWindow w = pool_chunk_at(A, pix0, c0, blk, lane, g, ok, c);
    const int32_t count = (w.y1 - w.y0) * (w.x1 - w.x0);
    float facc[kAcc];
    int32_t iacc[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
      facc[k] = OP == kPoolMax ? -3.402823466e+38f : 0.0f;
      iacc[k] = OP == kPoolMax ? -128 : 0;
    }
    if (nt) pool_walk_chunk<KIND, OP, true>(A, w, c, facc, iacc);
    else pool_walk_chunk<KIND, OP, false>(A, w, c, facc, iacc);
    if constexpr (KIND == kPoolF32) {
      f32x4 o;
      uint32_t nib = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float r = facc[k];
        if constexpr (OP == kPoolAverage) r = r / (float)count;
        o[k] = pool_clamp(r, A.lo, A.hi);
        nib |= (o[k] < 0.0f ? 1u : 0u) << k;
      }
      if (A.out && ok) store_streaming((f32x4*)A.out + g, o);
      if constexpr (BITS) store_nibble_word(A.bits, g, lane, ok, nib);   // per_pixel % 8 == 0: the 8 lanes of a word agree on ok
    } else {
      u32x4 o;
      uint32_t m = 0;                                              // 16 bits
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        int32_t r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          int32_t t = iacc[4 * d + k];
          if constexpr (OP == kPoolAverage) t = pool_round_div(t, count);
          r[k] = pool_clamp(t, A.qlo, A.qhi);
          m |= ((uint32_t)(r[k] - A.zero_point) >> 31) << (4 * d + k);
        }
        o[d] = pack4_u8(r[0], r[1], r[2], r[3]);
      }
      if (A.out && ok) pool_store_through((u32x4*)A.out + g, o);
      if constexpr (BITS) store_half_word<true>(A.bits, g, lane, ok, m);   // per_pixel % 2 == 0: lanes 2p and 2p + 1 agree on ok
    }
    pool_chunk_step(A, pix0, c0);
  }
}

template <int KIND, int OP>
LCE_KERNEL void __launch_bounds__(256)
pool_rows(const PoolArgs A) {
  typedef typename std::conditional<KIND == kPoolF32, float, int8_t>::type E;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t segs = A.per_pixel, cols = A.channels;
  const E* in = (const E*)A.in;
  for (uint64_t t = wave0; t < A.total; t += nwaves) {
    const uint64_t pixel = t / segs;                               // < 2^31
    const uint32_t seg = (uint32_t)(t - pixel * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    const PoolWindow w = pool_window(A, (uint32_t)pixel, true);
    const int32_t count = (w.y1 - w.y0) * (w.x1 - w.x0);
    bool neg = false;
    if (col < cols) {
      float facc = OP == kPoolMax ? -3.402823466e+38f : 0.0f;
      int32_t iacc = OP == kPoolMax ? -128 : 0;
      for (int32_t y = w.y0; y < w.y1; ++y) {
        const E* row = in + ((uint64_t)w.b * (uint64_t)A.H + (uint64_t)y) * (uint64_t)A.W * cols + col;
        for (int32_t x = w.x0; x < w.x1; ++x) {
          const E e = row[(uint64_t)x * cols];
          if constexpr (KIND == kPoolF32) {
            if constexpr (OP == kPoolMax) facc = facc < e ? e : facc;
            else facc = facc + e;
          } else {
            if constexpr (OP == kPoolMax) iacc = iacc < (int32_t)e ? (int32_t)e : iacc;
            else iacc = iacc + (int32_t)e;
          }
        }
      }
      const uint64_t o = pixel * (uint64_t)cols + col;
      if constexpr (KIND == kPoolF32) {
        if constexpr (OP == kPoolAverage) facc = facc / (float)count;
        const float r = pool_clamp(facc, A.lo, A.hi);
        if (A.out) ((float*)A.out)[o] = r;
        neg = r < 0.0f;
      } else {
        if constexpr (OP == kPoolAverage) iacc = pool_round_div(iacc, count);
        const int32_t r = pool_clamp(iacc, A.qlo, A.qhi);
        if (A.out) ((int8_t*)A.out)[o] = (int8_t)r;
        neg = r < A.zero_point;
      }
    }
    if (A.bits) store_seg_bits(A.bits, A.wpr, pixel, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
