// The float 1x1 CONV_2D between binary layers of a converted network (the convolution behind the 2x2 pool of a downsampling
// shortcut of Bi-RealNet / BinaryResNetE and of a transition block of BinaryDenseNet / MeliusNet) and the LceQuantize of its
// result, in one pass (include/lce_hip.h, lce_hip_conv1x1_f32).  A GEMM: M = output pixels, N = Cout, K = Cin.  NHWC float32
// in, the filter in the file's own layout [Cout][Cin], NHWC float32 out.  Per output element, over c = 0 .. Cin-1 IN ORDER:
//
//   t = +0.0f;  t = fmaf(x[c], w[o][c], t)     (one rounding per step, never reassociated, never split over K)
//   t = t + bias[o]                            (one float32 add; no bias: no add)
//   v = min(max(t, lo), hi)                    (std::max(a, b) = a < b ? b : a: a NaN passes, -0.0 stays -0.0)
//   bit = v < 0, LSB first, ceil(Cout / 32) words per pixel, padding bits 0, from the values the pass holds
//
// The chain runs on the matrix cores: v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain into its accumulator, one rounding per
// product, and its C/D never flush subnormals.  ROWS of the instruction are pixels, COLUMNS are channels: accumulator register r
// of lane l is pixel (r & 3) + 8 (r >> 2) + 4 (l >> 5) and channel l & 31 of the wave's tile, so the store of one register is
// two runs of 32 consecutive floats and one ballot of it is two pixels' bit words.
//
// A block of 4 waves owns 128 pixels x up to 128 channels; wave w owns pixels 32 w .. 32 w + 31 and ALL of the block's channel
// tiles, so the whole K loop of an output element stays in one wave's accumulators.  K advances in chunks of 32 channels
// through LDS: a row (a pixel of x, or a channel of w) is stored as [its 16 even channels][its 16 odd channels][4 floats of
// padding] -- step s of the instruction takes channel 2 s from lanes 0..31 and channel 2 s + 1 from lanes 32..63, so a lane's
// next FOUR steps are one 16-byte LDS read.  The padding makes the 16 rows of a read phase start in 16 different banks of 4.
//
// The K tail.  An accumulator can be -0.0 (fmaf(1e-30f, -1e-30f, +0.0f)), and fmaf(+0, +0, -0.0) = +0.0 would change it.  So
// the channels beyond Cin are staged as x = -0.0f and w = +0.0f: the product is -0.0 and t + (-0.0) = t for every t (+-0, NaN,
// +-inf included).  Steps beyond the last 8-channel group of the last chunk are not run at all.
//
// Strides only select pixels: output pixel (b, oy, ox) reads input pixel (b, oy * sh, ox * sw).  All offsets are 64-bit.  Two
// load paths, as the pools have: 16-byte loads when Cin % 4 == 0 and both pointers are 16-byte aligned, scalar loads otherwise.
// Stores are scalar per lane (128 contiguous bytes per half-wave) and need 4-byte alignment only.  No scratch, nothing allocated.
#pragma once
#include <stdint.h>

namespace lce {

constexpr int kConv1x1BM = 128;        // pixels per block tile (32 per wave)
constexpr int kConv1x1BN = 128;        // channels per block tile (up to 4 instruction tiles per wave)
constexpr int kConv1x1BK = 32;         // channels of K per LDS chunk
constexpr int kConv1x1Row = 36;        // floats per LDS row: 16 even, 16 odd, 4 padding

struct Conv1x1Args {
  const float* in;
  const float* filter;       // [Cout][Cin]
  const float* bias;         // null: none
  float* out;                // null: no float output
  uint32_t* bits;            // null: no LceQuantize output
  uint32_t M;                // output pixels < 2^31
  uint32_t Cin, Cout;
  uint32_t wpr;              // ceil(Cout / 32)
  uint32_t mtiles;           // ceil(M / 128)
  uint32_t OW, OHW;          // output width, output pixels per image
  uint32_t IW;               // input width
  uint64_t IHW;              // input pixels per image (with strides it may pass 2^32)
  uint32_t sh, sw;
  uint32_t strided;          // sh != 1 || sw != 1
  float lo, hi;              // CalculateActivationRange (float)
};

// Launches the kernel on `stream` (vec: the 16-byte load path; the caller has checked Cin % 4 and both alignments); returns
// the launch's hipError_t as an int.  Defined in lce_tu_conv1x1.hip.
int launch_conv1x1(const Conv1x1Args& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
#include "lce_device_intrinsics.h"

namespace lce {
using namespace lce_dev;

LCE_DEVICE float conv1x1_clamp(float v, float lo, float hi) {
  v = v < lo ? lo : v;          // std::max(v, lo)
  return hi < v ? hi : v;       // std::min(v, hi)
}

// Four consecutive channels k .. k + 3 of one row (`row` points at its channel 0); channels at or beyond K read as `pad`.  A
// row past the end comes with K = 0 (a per-lane limit instead of a null test: the test would be a lane mask kept in scalar
// registers through the whole K loop, one per row).
template <bool VEC>
LCE_DEVICE f32x4 conv1x1_load4(const float* row, uint32_t k, uint32_t K, float pad) {
  f32x4 v = {pad, pad, pad, pad};
  if constexpr (VEC) {
    if (k < K) v = *(const f32x4*)(row + k);        // K % 4 == 0: all four or none
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k + i < K) v[i] = row[k + i];
  }
  return v;
}

// Even channels to the first half of the LDS row, odd channels to the second.
LCE_DEVICE void conv1x1_stage(float* lds_row, uint32_t q, f32x4 v) {
  *(f32x2*)(lds_row + 2 * q) = f32x2{v[0], v[2]};
  *(f32x2*)(lds_row + 16 + 2 * q) = f32x2{v[1], v[3]};
}

// Accumulator registers 4 G .. 4 G + 3 of one instruction tile: pixels 8 G + i of the wave's 32 in lanes 0..31 and pixels
// 8 G + 4 + i in lanes 32..63 (`mrow` is the lane's pixel for G = 0, i = 0), channel `ch`.  Bias, clamp, the float store, and
// -- with a bit output -- one ballot per register, whose two halves go to the lanes of their pixels in `words` (v_writelane:
// no lane masks to keep; the ballots are settled once per group, lce_device_intrinsics.h).  `mlim`: pixels below it are stored
// (M; 0 without a float output or for a channel past the end); `thr`: bit = v < thr (0; -inf for a channel past the end).
// Both are per-lane values of ONE tile: as lane masks they would be loop invariants kept in scalar registers.
template <int G>
LCE_DEVICE void conv1x1_rows(const Conv1x1Args& A, const f32x16& acc, float bias, uint32_t mlim, float thr, uint32_t ch, uint32_t mrow,
                             uint32_t& words) {
  unsigned long long b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = mrow + 8u * G + (uint32_t)i;
    float v = acc[4 * G + i];
    if (A.bias != nullptr) v = v + bias;
    v = conv1x1_clamp(v, A.lo, A.hi);
    if (m < mlim) A.out[(uint64_t)m * A.Cout + ch] = v;
    b[i] = wave_ballot(v < thr);
  }
  if (A.bits != nullptr) {
    settle_ballots(b);
    words = write_lane_settled<8 * G + 0>((uint32_t)b[0], words);
    words = write_lane_settled<8 * G + 1>((uint32_t)b[1], words);
    words = write_lane_settled<8 * G + 2>((uint32_t)b[2], words);
    words = write_lane_settled<8 * G + 3>((uint32_t)b[3], words);
    words = write_lane_settled<8 * G + 4>((uint32_t)(b[0] >> 32), words);
    words = write_lane_settled<8 * G + 5>((uint32_t)(b[1] >> 32), words);
    words = write_lane_settled<8 * G + 6>((uint32_t)(b[2] >> 32), words);
    words = write_lane_settled<8 * G + 7>((uint32_t)(b[3] >> 32), words);
  }
}

template <bool VEC>
LCE_KERNEL void __launch_bounds__(256)
conv1x1_f32(const Conv1x1Args A) {
  __shared__ __attribute__((aligned(16))) float lds_x[kConv1x1BM * kConv1x1Row];
  __shared__ __attribute__((aligned(16))) float lds_w[kConv1x1BN * kConv1x1Row];
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t col = lane & 31u, half = lane >> 5;
  const uint32_t K = A.Cin;
  const uint32_t n0 = (uint32_t)block_idx_y() * (uint32_t)kConv1x1BN;
  const uint32_t ntiles = uniform(A.Cout - n0 >= (uint32_t)kConv1x1BN ? 4u : (A.Cout - n0 + 31u) / 32u);
  // staging: thread t carries channels 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i, i = 0..3, of both tiles
  const uint32_t q = tid & 7u, r0 = tid >> 3;
  const float* wrow[4];
  uint32_t wlim[4];                                                  // K, or 0 for a channel past the end
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t ch = n0 + r0 + 32u * (uint32_t)i;
    wlim[i] = ch < A.Cout ? K : 0u;
    wrow[i] = A.filter + (uint64_t)(ch < A.Cout ? ch : 0u) * K;
  }
  for (uint32_t tile = (uint32_t)block_idx_x(); tile < A.mtiles; tile += (uint32_t)grid_dim_x()) {
    const uint32_t m0 = tile * (uint32_t)kConv1x1BM;                 // < 2^31
    const float* xrow[4];
    uint32_t xlim[4];                                                // K, or 0 for a pixel past the end
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t m1 = m0 + r0 + 32u * (uint32_t)i;
      xlim[i] = m1 < A.M ? K : 0u;
      const uint32_t m = m1 < A.M ? m1 : 0u;
      uint64_t pix = m;
      if (A.strided) {
        const uint32_t b = m / A.OHW, rem = m - b * A.OHW;
        const uint32_t oy = rem / A.OW, ox = rem - oy * A.OW;
        pix = (uint64_t)b * A.IHW + (uint64_t)oy * A.sh * (uint64_t)A.IW + (uint64_t)ox * A.sw;
      }
      xrow[i] = A.in + pix * (uint64_t)K;
    }
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x16_zero();
    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)kConv1x1BK) {
      f32x4 xv[4], wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xv[i] = conv1x1_load4<VEC>(xrow[i], k0 + 4u * q, xlim[i], -0.0f);
        wv[i] = conv1x1_load4<VEC>(wrow[i], k0 + 4u * q, wlim[i], 0.0f);
      }
      __syncthreads();                                               // the previous chunk has been read
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        conv1x1_stage(lds_x + (r0 + 32u * (uint32_t)i) * kConv1x1Row, q, xv[i]);
        conv1x1_stage(lds_w + (r0 + 32u * (uint32_t)i) * kConv1x1Row, q, wv[i]);
      }
      __syncthreads();
      const uint32_t left = K - k0;
      const uint32_t groups = left >= (uint32_t)kConv1x1BK ? 4u : (left + 7u) / 8u;      // of 4 steps = 8 channels
      const float* xa = lds_x + (wave * 32u + col) * kConv1x1Row + half * 16u;
      const float* wb = lds_w + col * kConv1x1Row + half * 16u;
      for (uint32_t j = 0; j < groups; ++j) {
        const f32x4 a = *(const f32x4*)(xa + 4u * j);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if ((uint32_t)t < ntiles) {
            const f32x4 b = *(const f32x4*)(wb + (uint32_t)t * 32u * kConv1x1Row + 4u * j);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc[t], 0, 0, 0);
          }
        }
      }
    }
    // epilogue: bias, clamp, float store, bits.  Lane p < 32 collects the words of the wave's pixel p.
    uint32_t words[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if ((uint32_t)t < ntiles) {
        const uint32_t ch = n0 + (uint32_t)t * 32u + col;
        const bool ch_ok = ch < A.Cout;
        const float bias = A.bias != nullptr && ch_ok ? A.bias[ch] : 0.0f;
        const uint32_t mlim = A.out != nullptr && ch_ok ? A.M : 0u;
        const float thr = ch_ok ? 0.0f : -__builtin_inff();
        const uint32_t mrow = m0 + wave * 32u + 4u * half;
        conv1x1_rows<0>(A, acc[t], bias, mlim, thr, ch, mrow, words[t]);
        conv1x1_rows<1>(A, acc[t], bias, mlim, thr, ch, mrow, words[t]);
        conv1x1_rows<2>(A, acc[t], bias, mlim, thr, ch, mrow, words[t]);
        conv1x1_rows<3>(A, acc[t], bias, mlim, thr, ch, mrow, words[t]);
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
