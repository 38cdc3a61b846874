// The quantized (int8) CONV_2D of an int8-converted network -- its stem (3x3 / 2 or 7x7 / 2 on three channels), the 1x1 behind
// the 2x2 pool of a downsampling shortcut, the 1x1 of a dense network's transition -- and the LceQuantize of its result, in one
// launch (include/lce_hip.h, lce_hip_conv2d_i8).  NHWC int8 in with (si, zi), the filter in the file's own layout
// [Cout][fh][fw][Cin] with zero point 0, NHWC int8 out with (so, zo); groups 1, dilation 1; SAME or VALID with the pools' padding
// rule.  TFLite's reference_integer_ops::ConvPerChannel in its default (double-rounding) build, per output element:
//
//   acc = sum over IN-BOUNDS taps (fy, fx) and c of (x[iy][ix][c] - zi) * w[o][fy][fx][c]      exact, int32
//   acc += bias[o]
//   acc = RDivPOT(SRDHM(acc * 2^max(e, 0), m[o]), max(-e[o], 0))                               (m, e) = QuantizeMultiplier(si sw[o] / so)
//   v   = min(max(acc + zo, act_min), act_max);   bit = v < zo, LSB first, ceil(Cout / 32) words per pixel, padding bits 0
//
// An implicit GEMM on v_mfma_i32_32x32x32_i8: M = output pixels, N = Cout, K = fh fw Cin.  Integer sums are order-free, so ONE
// kernel serves every output pixel and every filter extent, 1x1 included:
//
//   padding   a tap outside the image is staged as x' = zi (itself an int8), every tap inside it as x' = x, and the host folds
//             the zero point into the per-channel constant c[o] = bias[o] - zi * sum_k w[o][k] (lce_hip_conv2d_i8_prepare).
//             Then sum_all-taps x' w + c[o] = sum_in (x - zi) w + sum_out (zi - zi) w + bias[o]: a padded tap contributes
//             zi w - zi w = 0, which is exactly the reference's skip.  No border kernel.
//   K tail    elements of a chunk at or beyond K are staged as w = 0 (x' = zi there, any int8 would do).  A chunk may end
//             inside a tap or inside a filter row.
//   K order   the instruction pairs byte j of a lane's A operand with byte j of the B operand of the lane in the same half
//             (l >> 5), and both operands are staged through the SAME k -> (LDS byte) function and read with the same offsets, so
//             the instruction's internal k order cannot matter.  Relied on: operand row / column = l & 31, and the C/D map of the
//             32x32 shapes (register r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31).  ROWS are pixels, COLUMNS
//             are channels, as lce_kernels_conv1x1.h has them: a lane owns one channel and its three constants.
//
// A block of 4 waves owns 128 pixels x up to 128 channels (grid.y: the 128-channel slices); wave w owns pixels 32 w .. + 31 and
// all of the block's channel tiles.  K advances in chunks of 128 bytes through LDS (32 on the byte path, whose K is small: a
// 3x3 stem is K = 27): a row (a pixel's window, or a channel's filter) is 128 bytes and 16 of padding; a lane's operand of
// instruction j of the chunk is the 16 bytes at 32 j + 16 (l >> 5).
// Gather: element k = fy (fw Cin) + r of a window is the byte at corner + fy (IW Cin) + r of the image -- a filter row is one
// contiguous run, clipped left and right where zi is staged.  Two load paths: 16 bytes per load when Cin % 16 == 0 and input and
// filter are 16-byte aligned (a lane's 16 elements then lie in one tap), bytes otherwise (Cin = 3, the stems' case).
// Epilogue: acc + c[o], the requantization with add_i8_srdhm / add_i8_rdivpot of lce_kernels_eltwise_i8.h, + zo, the clamp, byte
// stores (32 consecutive bytes per half-wave) and the bits as conv1x1_rows collects them.  All offsets are 64-bit.  No scratch,
// nothing allocated: the launch is capturable.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"
#include "lce_kernels_eltwise_i8.h"

namespace lce {

constexpr int kConvI8BM = 128;         // pixels per block tile (32 per wave)
constexpr int kConvI8BN = 128;         // channels per block tile (up to 4 instruction tiles per wave)
constexpr int kConvI8BK = 128;         // bytes of K per LDS chunk on the 16-byte path: 4 instructions
constexpr int kConvI8BKBytes = 32;     // ... on the byte path: 1 instruction
constexpr int kConvI8Row = 144;        // bytes per LDS row: 128 and 16 of padding
constexpr uint32_t kConvI8MaxK = 65793;   // the largest K with 255 * 128 * K <= 2^31 - 1 (lce_hip_conv2d_i8_prepare's bound)

struct ConvI8Args {
  const int8_t* in;
  const int8_t* filter;      // [Cout][fh][fw][Cin]
  const int32_t* table;      // [3][Cout]: c[o], m[o], e[o] (lce_hip_conv2d_i8_prepare)
  int8_t* out;               // null: no int8 output
  uint32_t* bits;            // null: no LceQuantize output
  uint32_t Cin, Cout;
  uint32_t wpr;              // ceil(Cout / 32)
  uint32_t K;                // fh * fw * Cin <= kConvI8MaxK
  uint32_t rowlen;           // fw * Cin: one filter row, contiguous in the filter and in the image
  uint64_t in_row;           // IW * Cin: bytes from one image row to the next
  int32_t IH, IW, OH, OW, sh, sw, ph, pw;
  uint32_t M;                // output pixels = batch * OH * OW < 2^31
  uint32_t mtiles;           // ceil(M / 128)
  int32_t zi, zo;            // input and output zero points
  int32_t act_min, act_max;  // CalculateActivationRangeQuantized at (so, zo)
  FastDiv div_rowlen, div_cin, div_ow, div_ohw;
};

// The geometry of `a` (everything but the pointers, the zero points and the clamp) for a convolution whose output extents
// oh x ow the caller has from lce_hip_conv2d_i8_check.  Host side; the host simulation of the kernel (tests/hostsim_conv2d_i8)
// fills its launches with it too.
inline void conv2d_i8_geometry(ConvI8Args& a, int32_t batch, int32_t in_height, int32_t in_width, int32_t channels_in, int32_t channels_out,
                               int32_t filter_height, int32_t filter_width, int32_t stride_height, int32_t stride_width, int32_t oh, int32_t ow) {
  conv_window_geometry(a, in_height, in_width, channels_in, channels_out, filter_height, filter_width, stride_height, stride_width, oh, ow);
  a.M = (uint32_t)((uint64_t)batch * oh * ow);
  a.mtiles = (uint32_t)(((uint64_t)a.M + kConvI8BM - 1) / kConvI8BM);
  a.div_rowlen = make_fastdiv(a.rowlen);
  a.div_cin = make_fastdiv(a.Cin);
  a.div_ow = make_fastdiv((uint32_t)ow);
  a.div_ohw = make_fastdiv((uint32_t)((uint64_t)oh * ow));
}

// The 16-byte load path's rule: Cin % 16, both operands aligned.
inline bool conv2d_i8_vec_rule(const ConvI8Args& a) { return load_vec_rule(a.Cin, 16, a.in, a.filter); }

// The grid of the launch: 128-pixel tiles, grid-strided past `cap` blocks (the product: ~8 per CU); grid.y: the 128-channel slices.
inline void conv2d_i8_grid(const ConvI8Args& a, uint32_t cap, unsigned* gx, unsigned* gy) {
  *gx = a.mtiles < cap ? a.mtiles : cap;
  *gy = (a.Cout + kConvI8BN - 1) / kConvI8BN;
}

// Launches the kernel on `stream` (vec: the 16-byte load path; the caller has checked Cin % 16 and both alignments); returns the
// launch's hipError_t as an int.  Defined in lce_tu_conv2d_i8.hip.
int launch_conv2d_i8(const ConvI8Args& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// (generic vectors, which the host compiler of the simulation in tests/hostsim_conv2d_i8 knows too)
typedef int32_t i32x4 __attribute__((vector_size(16)));
typedef int32_t i32x16 __attribute__((vector_size(64)));

// MultiplyByQuantizedMultiplier (tensorflow/lite/kernels/internal/common.h, the double-rounding build) for a multiplier m and
// an exponent -31 <= e <= 30.  Compiled for both sides: the host tests run this very function.
LCE_HOST_DEVICE int32_t conv2d_i8_requantize(int32_t acc, int32_t m, int32_t e) {
  const int32_t left = e > 0 ? e : 0, right = e > 0 ? 0 : -e;
  return add_i8_rdivpot(add_i8_srdhm((int32_t)((uint32_t)acc << left), m), right);
}

// Accumulator registers 4 G .. 4 G + 3 of one instruction tile (conv1x1_rows of lce_kernels_conv1x1.h with the integer
// epilogue): pixels 8 G + i of the wave's 32 in lanes 0..31 and 8 G + 4 + i in lanes 32..63 (`mrow`: the lane's pixel for G = 0,
// i = 0), channel `ch` with its constants (cst, mul, exp).  `mlim`: pixels below it are stored (M; 0 without an int8 output or
// for a channel past the end); `thr`: bit = v < thr (zo; INT32_MIN for a channel past the end).
template <int G>
LCE_DEVICE void conv2d_i8_rows(const ConvI8Args& A, const i32x16& acc, int32_t cst, int32_t mul, int32_t exp, uint32_t mlim, int32_t thr,
                               uint32_t ch, uint32_t mrow, uint32_t& words) {
  unsigned long long b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = mrow + 8u * G + (uint32_t)i;
    int32_t v = conv2d_i8_requantize(acc[4 * G + i] + cst, mul, exp) + A.zo;
    v = v < A.act_min ? A.act_min : v;
    v = v > A.act_max ? A.act_max : v;
    if (m < mlim) A.out[(uint64_t)m * A.Cout + ch] = (int8_t)v;
    b[i] = wave_ballot(v < thr);
  }
  if (A.bits != nullptr) tile_words<G>(b, words);
}

template <bool VEC>
LCE_KERNEL void __launch_bounds__(256, 2)
conv2d_i8(const ConvI8Args A) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_x[kConvI8BM * kConvI8Row];
  __shared__ __attribute__((aligned(16))) uint8_t lds_w[kConvI8BN * kConvI8Row];
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t col = lane & 31u, half = lane >> 5;
  const uint32_t K = A.K;
  const uint32_t n0 = (uint32_t)block_idx_y() * (uint32_t)kConvI8BN;
  const uint32_t ntiles = uniform(A.Cout - n0 >= (uint32_t)kConvI8BN ? 4u : (A.Cout - n0 + 31u) / 32u);
  // staging: a thread carries one 16-byte slice of a row of both tiles per pass.  16-byte path: chunks of 128 bytes, slice t & 7 of
  // rows (t >> 3) + 32 i, i = 0..3.  Byte path: chunks of 32 bytes -- one instruction -- so that with the K = 27 of a 3x3 stem every
  // lane gathers, slice t & 1 of row t >> 1, and a thread's sixteen byte loads of x and of w are in flight together ahead of the barrier.
  constexpr uint32_t kSlices = VEC ? (uint32_t)kConvI8BK / 16u : (uint32_t)kConvI8BKBytes / 16u;
  constexpr uint32_t kPass = 256u / kSlices;                         // rows staged per pass
  constexpr int R = (int)((uint32_t)kConvI8BM / kPass);              // passes: 4, or 1
  constexpr uint32_t BK = 16u * kSlices;
  static_assert(kConvI8BM == kConvI8BN && R * (int)kPass == kConvI8BM, "both tiles are staged by the same passes");
  const uint32_t q = tid % kSlices, r0 = tid / kSlices;
  const uint32_t zi1 = (uint32_t)A.zi & 0xffu, zi4 = zi1 * 0x01010101u;
  const int8_t* wrow[R];
  uint32_t wlim[R];                                                  // K, or 0 for a channel past the end
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const uint32_t ch = n0 + r0 + kPass * (uint32_t)i;
    wlim[i] = ch < A.Cout ? K : 0u;
    wrow[i] = A.filter + (uint64_t)(ch < A.Cout ? ch : 0u) * K;
  }
  const uint32_t ohw = (uint32_t)A.OH * (uint32_t)A.OW;
  for (uint32_t tile = (uint32_t)block_idx_x(); tile < A.mtiles; tile += (uint32_t)grid_dim_x()) {
    const uint32_t m0 = tile * (uint32_t)kConvI8BM;                  // < 2^31
    const int8_t* xrow[R];                                           // the window's corner (it may lie outside the image: never read there)
    int32_t ys[R], xs[R];                                            // the corner's row and column; ys = IH for a pixel past the end
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const uint32_t m1 = m0 + r0 + kPass * (uint32_t)i;
      const bool ok = m1 < A.M;
      const uint32_t m = ok ? m1 : 0u;
      const uint32_t b = fast_div(m, A.div_ohw), rem = m - b * ohw;
      const uint32_t oy = fast_div(rem, A.div_ow), ox = rem - oy * (uint32_t)A.OW;
      const int32_t y = (int32_t)oy * A.sh - A.ph, x = (int32_t)ox * A.sw - A.pw;
      ys[i] = ok ? y : A.IH;                                         // (every tap of such a row is out of bounds)
      xs[i] = x;
      xrow[i] = A.in + (((int64_t)b * A.IH + y) * A.IW + x) * (int64_t)A.Cin;
    }
    i32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0;
    for (uint32_t k0 = 0; k0 < K; k0 += BK) {
      // element k of a window is the image byte at corner + fy * in_row + r, k = fy * rowlen + r, of tap fx = r / Cin
      const uint32_t k = k0 + 16u * q;
      const uint32_t kd = k < K ? k : 0u;
      uint32_t fy = fast_div(kd, A.div_rowlen), r = kd - fy * A.rowlen;
      uint32_t fx = fast_div(r, A.div_cin), c = r - fx * A.Cin;
      // staged where nothing is read: x' = zi (a tap in the padding, the K tail, a pixel past the end), w = 0 (the K tail, a
      // channel past the end)
      u32x4 xv[R], wv[R];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        xv[i] = u32x4{zi4, zi4, zi4, zi4};
        wv[i] = u32x4{0u, 0u, 0u, 0u};
      }
      if constexpr (VEC) {
        // Cin % 16 == 0: the lane's 16 elements are channels c .. c + 15 of one tap, and K % 16 == 0: all sixteen or none
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const bool inb = k < K && (uint32_t)(ys[i] + (int32_t)fy) < (uint32_t)A.IH && (uint32_t)(xs[i] + (int32_t)fx) < (uint32_t)A.IW;
          if (inb) xv[i] = *(const u32x4*)(xrow[i] + ((uint64_t)fy * A.in_row + r));
          if (k < wlim[i]) wv[i] = *(const u32x4*)(wrow[i] + k);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const uint32_t ke = k + (uint32_t)e;
          const uint64_t off = (uint64_t)fy * A.in_row + r;
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const bool inb = ke < K && (uint32_t)(ys[i] + (int32_t)fy) < (uint32_t)A.IH && (uint32_t)(xs[i] + (int32_t)fx) < (uint32_t)A.IW;
            if (inb) xv[i][e >> 2] = (xv[i][e >> 2] & ~(0xffu << (8 * (e & 3)))) | ((uint32_t)(uint8_t)xrow[i][off] << (8 * (e & 3)));
            if (ke < wlim[i]) wv[i][e >> 2] |= (uint32_t)(uint8_t)wrow[i][ke] << (8 * (e & 3));
          }
          // the next element: the next channel, the next tap, the next filter row
          ++c; ++r;
          if (r == A.rowlen) { r = 0u; c = 0u; fx = 0u; ++fy; }
          else if (c == A.Cin) { c = 0u; ++fx; }
        }
      }
      __syncthreads();                                               // the previous chunk has been read
#pragma unroll
      for (int i = 0; i < R; ++i) {
        *(u32x4*)(lds_x + (r0 + kPass * (uint32_t)i) * kConvI8Row + 16u * q) = xv[i];
        *(u32x4*)(lds_w + (r0 + kPass * (uint32_t)i) * kConvI8Row + 16u * q) = wv[i];
      }
      __syncthreads();
      const uint32_t left = K - k0;
      const uint32_t steps = left >= BK ? BK / 32u : (left + 31u) / 32u;                  // instructions of 32 elements
      const uint8_t* xa = lds_x + (wave * 32u + col) * kConvI8Row + half * 16u;
      const uint8_t* wb = lds_w + col * kConvI8Row + half * 16u;
      for (uint32_t j = 0; j < steps; ++j) {
        const i32x4 a = *(const i32x4*)(xa + 32u * j);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if ((uint32_t)t < ntiles) {
            const i32x4 b = *(const i32x4*)(wb + (uint32_t)t * 32u * kConvI8Row + 32u * j);
            acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[t], 0, 0, 0);
          }
        }
      }
    }
    // epilogue: the constant, the requantization, the clamp, int8 store, bits.  Lane p < 32 collects the words of the wave's pixel p.
    uint32_t words[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if ((uint32_t)t < ntiles) {
        const uint32_t ch = n0 + (uint32_t)t * 32u + col;
        const bool ch_ok = ch < A.Cout;
        const uint32_t cs = ch_ok ? ch : 0u;
        const int32_t cst = A.table[cs], mul = A.table[(uint64_t)A.Cout + cs], exp = A.table[2ull * A.Cout + cs];
        const uint32_t mlim = A.out != nullptr && ch_ok ? A.M : 0u;
        const int32_t thr = ch_ok ? A.zo : INT32_MIN;
        const uint32_t mrow = m0 + wave * 32u + 4u * half;
        conv2d_i8_rows<0>(A, acc[t], cst, mul, exp, mlim, thr, ch, mrow, words[t]);
        conv2d_i8_rows<1>(A, acc[t], cst, mul, exp, mlim, thr, ch, mrow, words[t]);
        conv2d_i8_rows<2>(A, acc[t], cst, mul, exp, mlim, thr, ch, mrow, words[t]);
        conv2d_i8_rows<3>(A, acc[t], cst, mul, exp, mlim, thr, ch, mrow, words[t]);
      }
    }
    if (A.bits != nullptr && lane < 32u) {
      const uint32_t m = m0 + wave * 32u + lane;
      if (m < A.M) {
        uint32_t* dst = A.bits + (uint64_t)m * A.wpr + (n0 >> 5);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if ((uint32_t)t < ntiles) dst[t] = words[t];
      }
    }
  }
}

}  // namespace lce
#endif  // __HIPCC__
