// The float CONV_2D with a filter of any extent (the stem of a converted network: QuickNet's 3x3 / 2, the 7x7 / 2 of
// Bi-RealNet / BinaryResNetE / BinaryDenseNet, BinaryAlexNet's 11x11 / 4; also a float KxK convolution between binary layers)
// and the LceQuantize of its result, in one C call (include/lce_hip.h, lce_hip_conv2d_f32).  NHWC float32 in, the filter in the
// file's own layout [Cout][fh][fw][Cin], NHWC float32 out; groups 1, dilation 1; SAME or VALID with the pools' padding rule
// (pad_before = total / 2).  Per output element, over its IN-BOUNDS taps in raster order (filter row, then filter column) and
// within a tap over c = 0 .. Cin-1 in order -- taps in the padding are skipped, the filter index is the unclipped one:
//
//   t = +0.0f;  t = fmaf(x[iy][ix][c], w[o][fy][fx][c], t)   (one rounding per step, never reassociated, never split over K)
//   t = t + bias[o]                                          (one float32 add; no bias: no add)
//   v = min(max(t, lo), hi)                                  (conv1x1_clamp: a NaN passes, -0.0 stays -0.0)
//   bit = v < 0, LSB first, ceil(Cout / 32) words per pixel, padding bits 0, from the values the pass holds
//
// Two enumerations of the output pixels, two launches of one C call:
//   conv2d_interior : the rectangle of output pixels whose window lies wholly inside the image, batch x ih x iw of them, numbered
//                     densely and cut into tiles of 128.  For such a pixel the chain is a plain dot product over K = fh fw Cin
//                     in the filter's own order, and element k = fy (fw Cin) + r of it is the float at
//                     (window corner) + fy (IW Cin) + r of the image: a filter ROW is one contiguous run.  So this is the GEMM
//                     of lce_kernels_conv1x1.h with a gather in front -- v_mfma_f32_32x32x2_f32, pixels on rows and channels on
//                     columns, the whole K loop of an element in one wave's accumulators, K in chunks of 32 through LDS in the
//                     same row layout, the K tail (also a chunk that ends inside a tap) staged as x = -0.0f, w = +0.0f, and the
//                     same epilogue.  A tile's pixels are not consecutive in the output (the rectangle skips the border, a tile
//                     may span images), so the tile's output pixel numbers go through LDS beside the operands.
//   conv2d_border   : every other output pixel.  A clipped tap is the PIXEL's, the instruction's B operand is shared by its 32
//                     pixels, and no stand-in value of x is exact (fmaf(+-0, w, -0.0) is +0.0 for one sign of w, and NaN for an
//                     infinite w), so these pixels run a __builtin_fmaf chain over their in-bounds taps: one wave per 64 output
//                     channels of a pixel, one element per lane, one ballot per two words, as depthwise_rows.  The in-bounds
//                     part of a window row is again one contiguous run of image and of filter.
// Every output element and every bit word is written by exactly one of the two.  All offsets are 64-bit.  Loads: 16 bytes when
// Cin % 4 == 0 and input and filter are 16-byte aligned (interior only), dwords otherwise (Cin = 3, the stems' case); stores
// are dwords.  No scratch, nothing allocated: both launches are capturable.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"
#include "lce_kernels_conv1x1.h"

namespace lce {

constexpr int kConv2dBM = kConv1x1BM;   // pixels per block tile (32 per wave)
constexpr int kConv2dBN = kConv1x1BN;   // channels per block tile
constexpr int kConv2dBK = kConv1x1BK;   // elements of K per LDS chunk
constexpr int kConv2dRow = kConv1x1Row; // floats per LDS row

struct Conv2dArgs {
  const float* in;
  const float* filter;       // [Cout][fh][fw][Cin]
  const float* bias;         // null: none
  float* out;                // null: no float output
  uint32_t* bits;            // null: no LceQuantize output
  uint32_t Cin, Cout;
  uint32_t wpr;              // ceil(Cout / 32)
  uint32_t K;                // fh * fw * Cin < 2^31
  uint32_t rowlen;           // fw * Cin: one filter row, contiguous in the filter and in the image
  uint64_t in_row;           // IW * Cin: floats from one image row to the next
  int32_t IH, IW, OH, OW, fh, fw, sh, sw, ph, pw;
  // the interior rectangle: output rows iy0 .. iy0 + ih - 1, columns ix0 .. ix0 + iw - 1 (empty: all four 0)
  uint32_t iy0, ix0, ih, iw;
  uint32_t Mi;               // interior pixels = batch * ih * iw
  uint32_t mtiles;           // ceil(Mi / 128)
  // the border, per image: `top` pixels in the rows above the rectangle, `mid` beside it (`side` per row), the rest below
  uint32_t Mb;               // border pixels = batch * bpi
  uint32_t bpi, top, mid, side;
  uint32_t segs;             // 64-channel segments per pixel
  float lo, hi;              // CalculateActivationRange (float)
  FastDiv div_rowlen, div_iw, div_ihw, div_bpi, div_ow, div_side;
};

// The geometry of `a` (everything but the pointers and the clamp) for a convolution whose output extents oh x ow the caller has
// from lce_hip_bmaxpool_output_shape and whose sizes it has checked (lce_hip_conv2d_f32_check).  Host side; the host simulation
// of the kernels (tests/hostsim_conv2d) fills its launches with it too.
inline void conv2d_geometry(Conv2dArgs& a, int32_t batch, int32_t in_height, int32_t in_width, int32_t channels_in, int32_t channels_out,
                            int32_t filter_height, int32_t filter_width, int32_t stride_height, int32_t stride_width, int32_t oh, int32_t ow) {
  conv_window_geometry(a, in_height, in_width, channels_in, channels_out, filter_height, filter_width, stride_height, stride_width, oh, ow);
  a.fh = filter_height; a.fw = filter_width;
  // the interior rectangle: output pixels o with 0 <= o * stride - pad and o * stride - pad + filter <= extent
  auto interior = [](int64_t extent, int64_t out, int64_t filter, int64_t stride, int64_t pad, uint32_t* first, uint32_t* count) {
    const int64_t lo = (pad + stride - 1) / stride;
    int64_t hi = extent - filter + pad >= 0 ? (extent - filter + pad) / stride + 1 : 0;       // one past the last
    hi = hi < out ? hi : out;
    *first = hi > lo ? (uint32_t)lo : 0u;
    *count = hi > lo ? (uint32_t)(hi - lo) : 0u;
  };
  interior(in_height, oh, filter_height, stride_height, a.ph, &a.iy0, &a.ih);
  interior(in_width, ow, filter_width, stride_width, a.pw, &a.ix0, &a.iw);
  if (a.ih == 0 || a.iw == 0) a.iy0 = a.ix0 = a.ih = a.iw = 0;
  const uint64_t per_image = (uint64_t)a.ih * a.iw;
  a.Mi = (uint32_t)((uint64_t)batch * per_image);                    // (<= the output's pixels < 2^31)
  a.mtiles = (uint32_t)(((uint64_t)a.Mi + kConv2dBM - 1) / kConv2dBM);
  a.bpi = (uint32_t)((uint64_t)oh * ow - per_image);
  a.Mb = (uint32_t)((uint64_t)batch * a.bpi);
  a.top = a.iy0 * (uint32_t)ow;
  a.side = (uint32_t)ow - a.iw;
  a.mid = a.ih * a.side;
  a.segs = (a.Cout + 63u) / 64u;
  a.div_rowlen = make_fastdiv(a.rowlen);
  a.div_iw = make_fastdiv(a.iw);
  a.div_ihw = make_fastdiv((uint32_t)per_image);
  a.div_bpi = make_fastdiv(a.bpi);
  a.div_ow = make_fastdiv((uint32_t)ow);
  a.div_side = make_fastdiv(a.side);
}

// conv2d_interior's 16-byte load rule (Cin % 4) and grid (as conv2d_i8_grid); conv2d_border's: a wave per (pixel, 64 channels).
inline bool conv2d_vec_rule(const Conv2dArgs& a) { return load_vec_rule(a.Cin, 4, a.in, a.filter); }
inline void conv2d_grid(const Conv2dArgs& a, uint32_t cap, unsigned* gx, unsigned* gy) {
  *gx = a.mtiles < cap ? a.mtiles : cap;
  *gy = (a.Cout + kConv2dBN - 1) / kConv2dBN;
}
inline unsigned conv2d_border_grid(const Conv2dArgs& a, uint64_t cap = 2048) { return stream_grid((uint64_t)a.Mb * a.segs, 4, cap); }

// Launches conv2d_interior (when Mi > 0; vec: the 16-byte load path, the caller has checked Cin % 4 and both alignments) and
// conv2d_border (when Mb > 0) on `stream`; returns the first failing launch's hipError_t as an int.  Defined in
// lce_tu_conv2d.hip.
int launch_conv2d(const Conv2dArgs& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// conv1x1_rows with the tile's output pixel numbers read from LDS (`opix` points at the lane's pixel for G = 0, i = 0;
// 0xffffffff: a row past the end).  `mlim`: 2^31 to store, 0 without a float output or for a channel past the end.
template <int G>
LCE_DEVICE void conv2d_rows(const Conv2dArgs& A, const f32x16& acc, float bias, uint32_t mlim, float thr, uint32_t ch, const uint32_t* opix,
                            uint32_t& words) {
  unsigned long long b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = opix[8 * G + i];
    float v = acc[4 * G + i];
    if (A.bias != nullptr) v = v + bias;
    v = conv1x1_clamp(v, A.lo, A.hi);
    if (m < mlim) A.out[(uint64_t)m * A.Cout + ch] = v;
    b[i] = wave_ballot(v < thr);
  }
  if (A.bits != nullptr) tile_words<G>(b, words);
}

template <bool VEC>
LCE_KERNEL void __launch_bounds__(256)
conv2d_interior(const Conv2dArgs A) {
  __shared__ __attribute__((aligned(16))) float lds_x[kConv2dBM * kConv2dRow];
  __shared__ __attribute__((aligned(16))) float lds_w[kConv2dBN * kConv2dRow];
  __shared__ uint32_t lds_opix[kConv2dBM];
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t col = lane & 31u, half = lane >> 5;
  const uint32_t K = A.K;
  const uint32_t n0 = (uint32_t)block_idx_y() * (uint32_t)kConv2dBN;
  const uint32_t ntiles = uniform(A.Cout - n0 >= (uint32_t)kConv2dBN ? 4u : (A.Cout - n0 + 31u) / 32u);
  // staging: thread t carries elements 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i, i = 0..3, of both tiles
  const uint32_t q = tid & 7u, r0 = tid >> 3;
  const float* wrow[4];
  uint32_t wlim[4];                                                  // K, or 0 for a channel past the end
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t ch = n0 + r0 + 32u * (uint32_t)i;
    wlim[i] = ch < A.Cout ? K : 0u;
    wrow[i] = A.filter + (uint64_t)(ch < A.Cout ? ch : 0u) * K;
  }
  const uint32_t ihw = A.ih * A.iw;
  for (uint32_t tile = (uint32_t)block_idx_x(); tile < A.mtiles; tile += (uint32_t)grid_dim_x()) {
    const uint32_t m0 = tile * (uint32_t)kConv2dBM;                  // < 2^31
    const float* xrow[4];                                            // the window's corner: element 0 of the pixel's chain
    uint32_t xlim[4];                                                // K, or 0 for a pixel past the end
    uint32_t opix[4];                                                // the output pixel; 0xffffffff past the end
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t m1 = m0 + r0 + 32u * (uint32_t)i;
      const bool ok = m1 < A.Mi;
      xlim[i] = ok ? K : 0u;
      const uint32_t m = ok ? m1 : 0u;
      const uint32_t b = fast_div(m, A.div_ihw), rem = m - b * ihw;
      const uint32_t ry = fast_div(rem, A.div_iw), rx = rem - ry * A.iw;
      const uint32_t oy = A.iy0 + ry, ox = A.ix0 + rx;
      const uint64_t y = (uint64_t)oy * (uint32_t)A.sh - (uint32_t)A.ph, x = (uint64_t)ox * (uint32_t)A.sw - (uint32_t)A.pw;   // >= 0: interior
      xrow[i] = A.in + (((uint64_t)b * (uint32_t)A.IH + y) * (uint32_t)A.IW + x) * A.Cin;
      opix[i] = ok ? (b * (uint32_t)A.OH + oy) * (uint32_t)A.OW + ox : 0xffffffffu;
    }
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x16_zero();
    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)kConv2dBK) {
      // element k of the chain is the image float at corner + fy * in_row + r, k = fy * rowlen + r; with VEC, rowlen % 4 == 0
      // and a lane's four elements lie in one filter row
      const uint32_t k = k0 + 4u * q;
      uint64_t off[4];
#pragma unroll
      for (int e = 0; e < (VEC ? 1 : 4); ++e) {
        const uint32_t ke = k + (uint32_t)e < K ? k + (uint32_t)e : 0u;
        const uint32_t fy = fast_div(ke, A.div_rowlen);
        off[e] = (uint64_t)fy * A.in_row + (ke - fy * A.rowlen);
      }
      f32x4 xv[4], wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = {-0.0f, -0.0f, -0.0f, -0.0f};
        if constexpr (VEC) {
          if (k < xlim[i]) v = *(const f32x4*)(xrow[i] + off[0]);    // K % 4 == 0: all four or none
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + (uint32_t)e < xlim[i]) v[e] = xrow[i][off[e]];
        }
        xv[i] = v;
        wv[i] = conv1x1_load4<VEC>(wrow[i], k, wlim[i], 0.0f);
      }
      __syncthreads();                                               // the previous chunk and the previous tile's pixel numbers have been read
      if (k0 == 0u && q == 0u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_opix[r0 + 32u * (uint32_t)i] = opix[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        conv1x1_stage(lds_x + (r0 + 32u * (uint32_t)i) * kConv2dRow, q, xv[i]);
        conv1x1_stage(lds_w + (r0 + 32u * (uint32_t)i) * kConv2dRow, q, wv[i]);
      }
      __syncthreads();
      const uint32_t left = K - k0;
      const uint32_t groups = left >= (uint32_t)kConv2dBK ? 4u : (left + 7u) / 8u;       // of 4 steps = 8 elements
      const float* xa = lds_x + (wave * 32u + col) * kConv2dRow + half * 16u;
      const float* wb = lds_w + col * kConv2dRow + half * 16u;
      for (uint32_t j = 0; j < groups; ++j) {
        const f32x4 a = *(const f32x4*)(xa + 4u * j);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if ((uint32_t)t < ntiles) {
            const f32x4 b = *(const f32x4*)(wb + (uint32_t)t * 32u * kConv2dRow + 4u * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc[t], 0, 0, 0);
          }
        }
      }
    }
    // epilogue: bias, clamp, float store, bits.  Lane p < 32 collects the words of the wave's pixel p.
    uint32_t words[4] = {0u, 0u, 0u, 0u};
    const uint32_t* my_opix = lds_opix + wave * 32u + 4u * half;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if ((uint32_t)t < ntiles) {
        const uint32_t ch = n0 + (uint32_t)t * 32u + col;
        const bool ch_ok = ch < A.Cout;
        const float bias = A.bias != nullptr && ch_ok ? A.bias[ch] : 0.0f;
        const uint32_t mlim = A.out != nullptr && ch_ok ? 0x80000000u : 0u;
        const float thr = ch_ok ? 0.0f : -__builtin_inff();
        conv2d_rows<0>(A, acc[t], bias, mlim, thr, ch, my_opix, words[t]);
        conv2d_rows<1>(A, acc[t], bias, mlim, thr, ch, my_opix, words[t]);
        conv2d_rows<2>(A, acc[t], bias, mlim, thr, ch, my_opix, words[t]);
        conv2d_rows<3>(A, acc[t], bias, mlim, thr, ch, my_opix, words[t]);
      }
    }
    if (A.bits != nullptr && lane < 32u) {
      const uint32_t m = lds_opix[wave * 32u + lane];
      if (m != 0xffffffffu) {
        uint32_t* dst = A.bits + (uint64_t)m * A.wpr + (n0 >> 5);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if ((uint32_t)t < ntiles) dst[t] = words[t];
      }
    }
  }
}

template <bool BITS>
LCE_KERNEL void __launch_bounds__(256)
conv2d_border(const Conv2dArgs A) {
  const uint32_t lane = (uint32_t)thread_idx_x() & 63u;
  const uint64_t wave0 = (uint64_t)block_idx_x() * 4ull + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * 4ull;
  const uint64_t total = (uint64_t)A.Mb * A.segs;
  for (uint64_t t = wave0; t < total; t += nwaves) {
    const uint32_t j = (uint32_t)(t / A.segs);                       // border pixel < 2^31
    const uint32_t seg = (uint32_t)(t - (uint64_t)j * A.segs);
    const uint32_t col = seg * 64u + lane;
    // the pixel: image b, the jj-th border pixel of it
    const uint32_t b = fast_div(j, A.div_bpi), jj = j - b * A.bpi;
    uint32_t oy, ox;
    if (jj < A.top) {
      oy = fast_div(jj, A.div_ow);
      ox = jj - oy * (uint32_t)A.OW;
    } else if (jj - A.top < A.mid) {
      const uint32_t u = jj - A.top, ry = fast_div(u, A.div_side), s = u - ry * A.side;
      oy = A.iy0 + ry;
      ox = s < A.ix0 ? s : s + A.iw;
    } else {
      const uint32_t u = jj - A.top - A.mid, ry = fast_div(u, A.div_ow);
      oy = A.iy0 + A.ih + ry;
      ox = u - ry * (uint32_t)A.OW;
    }
    const uint32_t pixel = (b * (uint32_t)A.OH + oy) * (uint32_t)A.OW + ox;
    const int32_t ys = (int32_t)oy * A.sh - A.ph, xs = (int32_t)ox * A.sw - A.pw;
    const int32_t y0 = ys < 0 ? 0 : ys, y1 = ys + A.fh > A.IH ? A.IH : ys + A.fh;
    const int32_t x0 = xs < 0 ? 0 : xs, x1 = xs + A.fw > A.IW ? A.IW : xs + A.fw;
    bool neg = false;
    if (col < A.Cout) {
      const float* w = A.filter + (uint64_t)col * A.K;
      const uint32_t run = x1 > x0 ? (uint32_t)(x1 - x0) * A.Cin : 0u;             // the in-bounds part of a window row
      float acc = 0.0f;
      for (int32_t y = y0; y < y1; ++y) {
        const float* xr = A.in + (((uint64_t)b * (uint32_t)A.IH + (uint32_t)y) * (uint32_t)A.IW + (uint32_t)x0) * A.Cin;
        const float* wr = w + (uint64_t)(uint32_t)(y - ys) * A.rowlen + (uint64_t)(uint32_t)(x0 - xs) * A.Cin;   // the unclipped tap
        for (uint32_t e = 0; e < run; ++e) acc = __builtin_fmaf(xr[e], wr[e], acc);
      }
      if (A.bias != nullptr) acc = acc + A.bias[col];
      const float r = conv1x1_clamp(acc, A.lo, A.hi);
      if (A.out != nullptr) A.out[(uint64_t)pixel * A.Cout + col] = r;
      neg = r < 0.0f;
    }
    if constexpr (BITS) {
      const unsigned long long bal = wave_ballot(neg);
      const uint32_t wd = seg * 2u + lane;
      if (lane < 2u && wd < A.wpr) A.bits[(uint64_t)pixel * A.wpr + wd] = (uint32_t)(bal >> (32u * lane));
    }
  }
}

}  // namespace lce
#endif  // __HIPCC__
