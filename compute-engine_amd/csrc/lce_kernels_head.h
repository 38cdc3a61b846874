// The float classifier head of a converted network (GlobalAveragePooling -> Dense -> softmax): the FULLY_CONNECTED and the
// SOFTMAX (include/lce_hip.h, lce_hip_fully_connected_f32 and lce_hip_softmax_f32).  The MEAN in front of them is an
// AVERAGE pool over the whole image and runs on lce_kernels_pool.h.
//
// FULLY_CONNECTED.  A GEMM with FEW rows: M = images, N = outputs, K = inputs; x [M][K], w [N][K] (the file's layout), out
// [M][N].  Per output element, over k = 0 .. K-1 IN ORDER -- the chain of lce_kernels_conv1x1.h, so the bytes are those of
// lce_hip_conv1x1_f32 on a [M, 1, 1, K] image:
//
//   t = +0.0f;  t = fmaf(x[m][k], w[o][k], t)   (one rounding per step, never reassociated, never split over K)
//   t = t + bias[o]                             (one float32 add; no bias: no add)
//   v = min(max(t, lo), hi)                     (std::max(a, b) = a < b ? b : a: a NaN passes, -0.0 stays -0.0)
//
// The tile.  lce_kernels_conv1x1.h gives a block 128 rows x 128 columns: a head of 256 images x 1000 classes is 16 blocks on
// 256 compute units, and one image is one block row of which 127 of 128 rows are padding.  Here ONE WAVE owns one 16 x 16 tile
// (rows = images, columns = outputs) and the whole K loop of it: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain of four steps
// into its accumulator (one rounding per product; C/D never flush subnormals), lane l supplies row / column l & 15 at
// k = l >> 4, and accumulator register i of lane l is row 4 (l >> 4) + i, column l & 15.  256 x 1000 is 1008 tiles -- one wave
// for nearly every SIMD of the device -- and a tile's chain is K / 4 instructions of 32 cycles, against K / 2 of 64 cycles for a
// 32 x 32 tile on a quarter of the SIMDs.
//
// Operands come STRAIGHT FROM GLOBAL MEMORY (L2: the weights are read by every row tile, the images by every column tile), with
// no LDS stage: a tile has no second wave to share a staged chunk with, so a stage would only add a write, a read and their
// waits to every 16 channels of K.  K advances in chunks of 64 channels -- four loads of 16 channels per operand -- and the loads
// of the chunk after the one being multiplied are issued before its instructions.  Measured (profiles/head/fc_vs_conv1x1.txt): 3.1
// to 3.6 times faster than the 1x1 kernel on the head's shapes, but one image takes as long as 256, so a wave's own chain is what
// is timed, and a build with chunks of 16 was within 10 % of this one: the chain is NOT bound by the loads alone.  The transpose
// below consumes a chunk's loads as soon as they are issued (only the instructions of the chunk before overlap them) and its
// exchanges wait one by one; moving the transpose behind the instructions, or off the 16-byte path, is the next thing to try.
// Two load paths, as lce_kernels_conv1x1.h has: with K % 4 == 0 and both pointers 16-byte aligned, lane (row, g) loads the four
// consecutive channels 4 g .. 4 g + 3 of its row in one 16-byte load, and the four lane groups of a row transpose them among
// themselves (three exchanges) so that step s holds channel 4 s + g; otherwise every lane loads its channel of each step by
// itself.
//
// The K tail.  An accumulator can be -0.0 (fmaf(1e-30f, -1e-30f, +0.0f)), and fmaf(+0, +0, -0.0) = +0.0 would change it.  So
// the channels beyond K of the last instruction are x = -0.0f and w = +0.0f: the product is -0.0 and t + (-0.0) = t for every t
// (+-0, NaN, +-inf included).  Instructions beyond the last 4-channel group are not run at all.  A row or column past the end
// reads nothing (its limit is 0) and is not stored.
//
// SOFTMAX over the last axis of [rows][cols], ONE WAVE per row.  The bytes are stated, not inherited -- every step is a float32
// add, mul, fmaf, round-to-integer or exponent insertion, so tests/head_ref.py restates them in NumPy:
//
//   m   = max over the row                      (inputs finite; +0 and -0 compare equal and either gives the same bytes below)
//   a_i = (x_i - m) * beta                      (two IEEE operations, no contraction)
//   e_i = head_exp(a_i)                         (lce_kernels_exp.h; restated below)
//   s   : lane l adds e_l, e_{l+64}, e_{l+128}, ... in this order from +0.0f; then s_l = s_l + s_{l ^ d} for d = 32, 16, 8, 4, 2, 1
//   out_i = e_i / s                             (the correctly rounded division)
//
// head_exp(a), Cody-Waite reduction and a Horner polynomial:
//   not (a >= -104)        -> +0.0f             (a < -104, a = -inf, a NaN: exp(-104) is below half the smallest subnormal)
//   a > 0                  -> a = 0             (never with finite inputs: x_i <= m)
//   n = rint(a * 1.44269502f)                   (round to nearest even; -150 <= n <= 0)
//   r = fmaf(n, -0.693145751953125f, a);  r = fmaf(n, -1.42860676e-06f, r)          (|r| <= 0.3466)
//   p = 1/5040;  p = fmaf(p, r, c) for c = 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1       (Taylor to r^7; the constants rounded to float32)
//   n >= -125: the result is p with n added to its exponent field (p is in [0.70, 1.42]: the result is normal)
//   n <  -125: p with n + 64 added to its exponent field, times 2^-64f              (ONE float32 multiply: it rounds into the subnormals)
// Its largest error against exp is measured in tests/test_head_host.py and stated in DESIGN.md.  Rows with a NaN or an infinity
// do not fault; their bytes are unspecified.  In place (in == out) works: a lane writes only elements it alone reads, and
// only after the whole wave has finished the first pass.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"

namespace lce {

constexpr int kFcTile = 16;            // rows and columns of a wave's tile
constexpr int kFcBK = 64;              // channels of K per chunk: four loads of 16 channels, sixteen instructions

struct FcArgs {
  const float* in;           // [M][K]
  const float* filter;       // [N][K]
  const float* bias;         // null: none
  float* out;                // [M][N]
  uint32_t M, K, N;
  uint32_t ntiles;           // ceil(N / 16)
  uint32_t tiles;            // ceil(M / 16) * ntiles < 2^31
  float lo, hi;              // CalculateActivationRange (float)
};

struct SoftmaxArgs {
  const float* in;
  float* out;
  uint64_t rows;
  uint32_t cols;
  float beta;
};

// fully_connected_f32's launch (entry, launcher, host simulation): tile counts, the 16-byte rule (K % 4), one wave per tile.
inline void fc_fill(FcArgs& a, int32_t batch, int32_t inputs, int32_t outputs) { dense_fill(a, batch, inputs, outputs, kFcTile); }
inline bool fc_vec_rule(const FcArgs& a) { return load_vec_rule(a.K, 4, a.in, a.filter); }
inline unsigned fc_grid(const FcArgs& a, uint64_t cap = 2048) { return stream_grid(a.tiles, 4, cap); }

// Launch the kernels on `stream`; return the launch's hipError_t as an int.  Defined in lce_tu_head.hip.
int launch_fully_connected(const FcArgs& args, bool vec, void* stream);
int launch_softmax(const SoftmaxArgs& args, void* stream);

}  // namespace lce

#ifdef __HIPCC__
#include "lce_device_intrinsics.h"
#include "lce_kernels_exp.h"

namespace lce {
using namespace lce_dev;

LCE_DEVICE float head_clamp(float v, float lo, float hi) {
  v = v < lo ? lo : v;          // std::max(v, lo)
  return hi < v ? hi : v;       // std::min(v, hi)
}

// Element `i` (per lane) of `v`, and `v` with element `i` replaced: selects, the vector stays in registers.
LCE_DEVICE float head_pick(const f32x4& v, uint32_t i) {
  const float lo = (i & 1u) ? v[1] : v[0], hi = (i & 1u) ? v[3] : v[2];
  return (i & 2u) ? hi : lo;
}
LCE_DEVICE void head_put(f32x4& v, uint32_t i, float x) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = i == (uint32_t)j ? x : v[j];
}

// The 16 channels k0 .. k0 + 15 of one row as the instructions want them: element s is channel k0 + 4 s + g; channels at or beyond `lim`
// (K, or 0 for a row past the end) read as `pad`.  VEC: one 16-byte load of channels k0 + 4 g .. + 3 (K % 4 == 0: all four or
// none) and the transpose among the lanes l ^ 16, l ^ 32, l ^ 48, which hold the same row.
template <bool VEC>
LCE_DEVICE f32x4 fc_load_chunk(const float* row, uint32_t k0, uint32_t g, uint32_t lim, float pad) {
  f32x4 a = {pad, pad, pad, pad};
  if constexpr (VEC) {
    f32x4 v = {pad, pad, pad, pad};
    if (k0 + 4u * g < lim) v = *(const f32x4*)(row + k0 + 4u * g);
    head_put(a, g, head_pick(v, g));
#pragma unroll
    for (uint32_t m = 1; m < 4; ++m) {
      // lane group g ^ m wants my channel 4 g + (g ^ m); it sends me its channel 4 (g ^ m) + g
      const uint32_t got = shfl_xor(__builtin_bit_cast(uint32_t, head_pick(v, g ^ m)), (int)(16u * m));
      head_put(a, g ^ m, __builtin_bit_cast(float, got));
    }
  } else {
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
      const uint32_t k = k0 + 4u * s + g;
      if (k < lim) a[s] = row[k];
    }
  }
  return a;
}

template <bool VEC>
LCE_KERNEL void __launch_bounds__(256)
fully_connected_f32(const FcArgs A) {
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t r = lane & 15u, g = lane >> 4;
  const uint32_t K = A.K;
  for (uint32_t tile = (uint32_t)block_idx_x() * 4u + wave; tile < A.tiles; tile += (uint32_t)grid_dim_x() * 4u) {
    const uint32_t tm = tile / A.ntiles, tn = tile - tm * A.ntiles;
    const uint32_t m = tm * (uint32_t)kFcTile + r, o = tn * (uint32_t)kFcTile + r;       // this lane's row of x and of w
    const uint32_t xlim = m < A.M ? K : 0u, wlim = o < A.N ? K : 0u;
    const float* xrow = A.in + (uint64_t)(m < A.M ? m : 0u) * K;
    const float* wrow = A.filter + (uint64_t)(o < A.N ? o : 0u) * K;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 xa[4], wb[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      xa[j] = fc_load_chunk<VEC>(xrow, 16u * j, g, xlim, -0.0f);
      wb[j] = fc_load_chunk<VEC>(wrow, 16u * j, g, wlim, 0.0f);
    }
    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)kFcBK) {
      f32x4 xc[4], wc[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) { xc[j] = xa[j]; wc[j] = wb[j]; }
      if (k0 + (uint32_t)kFcBK < K) {                                                    // the next chunk, in flight behind this one
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          xa[j] = fc_load_chunk<VEC>(xrow, k0 + (uint32_t)kFcBK + 16u * j, g, xlim, -0.0f);
          wb[j] = fc_load_chunk<VEC>(wrow, k0 + (uint32_t)kFcBK + 16u * j, g, wlim, 0.0f);
        }
      }
      const uint32_t left = K - k0;
      const uint32_t steps = left >= (uint32_t)kFcBK ? 16u : (left + 3u) / 4u;           // instructions of 4 channels
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j)
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s)
          if (4u * j + s < steps) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[j][s], wc[j][s], acc, 0, 0, 0);
    }
    // epilogue: register i is row 4 g + i of the tile, column r
    const bool col_ok = o < A.N;
    const float bias = A.bias != nullptr && col_ok ? A.bias[o] : 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t row = tm * (uint32_t)kFcTile + 4u * g + i;
      float v = acc[i];
      if (A.bias != nullptr) v = v + bias;
      v = head_clamp(v, A.lo, A.hi);
      if (col_ok && row < A.M) A.out[(uint64_t)row * A.N + o] = v;
    }
  }
}

// head_exp(a): exp(a) for a <= 0 as the header comment states it, in lce_kernels_exp.h (included above) -- the LOGISTIC step of
// lce_kernels_eltwise.h is stated on the same function.  `/` below is the correctly rounded division (hipcc's default for float).

// The second half of the stated sum: s_l = s_l + s_{l ^ d} for d = 32, 16, 8, 4, 2, 1 over the wave's 64 partial sums (every lane ends
// with the same number).  lce_kernels_head_i8.h sums its rows through this function too.
LCE_DEVICE float head_wave_sum(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s = s + __builtin_bit_cast(float, shfl_xor(__builtin_bit_cast(uint32_t, s), d));
  return s;
}

// WAVES: the waves of a block, one row each (a template like every kernel here: one definition however many units include it)
template <int WAVES>
LCE_KERNEL void __launch_bounds__(64 * WAVES)
softmax_f32(const SoftmaxArgs A) {
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  for (uint64_t row = (uint64_t)block_idx_x() * WAVES + wave; row < A.rows; row += (uint64_t)grid_dim_x() * WAVES) {
    const float* x = A.in + row * A.cols;
    float* y = A.out + row * A.cols;
    float m = -__builtin_inff();
    for (uint32_t i = lane; i < A.cols; i += 64u) {
      const float v = x[i];
      m = m < v ? v : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float other = __builtin_bit_cast(float, shfl_xor(__builtin_bit_cast(uint32_t, m), d));
      m = m < other ? other : m;
    }
    float s = 0.0f;
    for (uint32_t i = lane; i < A.cols; i += 64u) s = s + head_exp((x[i] - m) * A.beta);
    s = head_wave_sum(s);
    for (uint32_t i = lane; i < A.cols; i += 64u) y[i] = head_exp((x[i] - m) * A.beta) / s;
  }
}

}  // namespace lce
#endif  // __HIPCC__
