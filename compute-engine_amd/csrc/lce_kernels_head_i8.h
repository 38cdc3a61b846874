// The int8 classifier head of an int8-converted network -- MEAN, FULLY_CONNECTED and SOFTMAX on int8 tensors -- and the two
// operators of the float / int8 boundary, QUANTIZE and DEQUANTIZE (include/lce_hip.h, "The int8 classifier head and the float/int8
// boundary").  The arithmetic of each is stated there completely; tests/head_i8_ref.py restates it in NumPy.
//
// FULLY_CONNECTED.  A GEMM with FEW rows on v_mfma_i32_16x16x64_i8: M = images, N = outputs, K = inputs; x [M][K] int8, w [N][K]
// int8 (the file's layout, zero point 0), out [M][N] int8.  The arithmetic is lce_hip_conv2d_i8's on a [M, 1, 1, K] image: the exact
// int32 sum of x w, the constant c[o] = bias[o] - zi sum_k w[o][k] of the table (so that sum x w + c = sum (x - zi) w + bias), the
// requantization with add_i8_srdhm / add_i8_rdivpot of lce_kernels_eltwise_i8.h, + zo, the clamp.
//
// The tile, as lce_kernels_head.h has it and for its reason: ONE WAVE owns one 16 x 16 tile (rows = images, columns = outputs) and
// the whole K loop of it.  256 x 1000 is 1008 waves for the 1024 SIMDs of the device, where lce_kernels_conv2d_i8.h's blocks of
// 128 x 128 would put the layer on 16 of 256 compute units.
//
//   operands  lane l supplies row (of x) / column (a row of w) l & 15 and the 16-byte k-slice l >> 4 of each 64-byte step: bytes
//             64 s + 16 (l >> 4) .. + 15 of its row, straight from global memory (L2), no LDS stage: a tile has no second wave to
//             share a staged chunk with.  K advances in chunks of four steps (256 bytes of K, four 16-byte loads per operand) and the
//             loads of the chunk after the one being multiplied are issued before its instructions.
//   K order   x and w take their bytes through the SAME k -> (step, lane group, byte) function: the instruction pairs byte j of
//             a lane's A operand with byte j of the B operand of the lane in the same group l >> 4, so its internal k order cannot
//             matter -- an integer sum has one answer.  Relied on: operand row / column = l & 15, and the C/D map of the 16x16
//             shapes (register i of lane l: row 4 (l >> 4) + i, column l & 15).  tests/test_gpu_head_i8.py decides both.
//   K tail    bytes at or beyond K are staged as x = 0 and w = 0; a row or column past the end reads nothing (its limit is 0)
//             and is not stored.  Nothing is read out of bounds.
//   paths     16 bytes per load when K % 16 == 0 and both pointers are 16-byte aligned (a lane's 16 bytes are all inside K or all
//             outside), single bytes otherwise.
//
// MEAN over height and width of NHWC int8: a wave owns 16 channels of one image; lane l adds channel l & 15 of the pixels
// l >> 4, (l >> 4) + 4, ... and the four partial sums meet through two exchanges (integer sums: any order).  Then
// mean_i8_value: the multiply first, the division by the count rounding half away from zero second.
//
// SOFTMAX over the last axis of int8 [rows][cols], ONE WAVE per row as softmax_f32: the row maximum, d = q - max in [-255, 0],
// e = head_exp((float)d * sb) with lce_kernels_head.h's head_exp, that kernel's fixed-order sum (64 partial sums in lane order,
// then head_wave_sum), p = e / s, round(256 p) - 128 clamped at 127.  In place works for the float kernel's reason.
//
// QUANTIZE / DEQUANTIZE: one element per lane and step, 64-bit counts.
#pragma once
#include <stdint.h>

#include "lce_kernels_eltwise_i8.h"
#include "lce_kernels_head.h"

namespace lce {

constexpr int kFcI8Tile = 16;          // rows and columns of a wave's tile
constexpr int kFcI8Step = 64;          // bytes of K per instruction
constexpr int kFcI8Steps = 4;          // instructions per chunk: 256 bytes of K in flight per operand
constexpr uint32_t kFcI8MaxK = 65793;  // the largest K with 255 * 128 * K <= 2^31 - 1 (lce_hip_conv2d_i8's bound)
constexpr int kMeanI8Channels = 16;    // channels of a wave of mean_i8; 64 / 16 = 4 lane groups share the pixels

struct FcI8Args {
  const int8_t* in;          // [M][K]
  const int8_t* filter;      // [N][K]
  const int32_t* table;      // [3][N]: c[o], m[o], e[o] (lce_hip_fully_connected_i8_prepare)
  int8_t* out;               // [M][N]
  uint32_t M, K, N;
  uint32_t ntiles;           // ceil(N / 16)
  uint32_t tiles;            // ceil(M / 16) * ntiles < 2^31
  int32_t zo;                // output zero point
  int32_t act_min, act_max;  // CalculateActivationRangeQuantized at (so, zo)
};

struct MeanI8Args {
  const int8_t* in;          // [batch][n][C]
  int8_t* out;               // [batch][C]
  uint64_t batch;
  uint32_t n, C;             // pixels per image (H * W), channels
  uint32_t segs;             // ceil(C / 16)
  int32_t zi, zo;
  int32_t mul, left, right;  // QuantizeMultiplier(si / so): m, max(e, 0), max(-e, 0)
};

struct SoftmaxI8Args {
  const int8_t* in;
  int8_t* out;
  uint64_t rows;
  uint32_t cols;
  float sb;                  // input scale * beta, one float32 multiply
};

struct QuantArgs {
  const void* in;            // float (quantize) or int8 (dequantize)
  void* out;                 // int8 (quantize) or float (dequantize)
  uint64_t n;
  float scale;
  int32_t zp;
};

// The launch of fully_connected_i8, as fc_fill / fc_vec_rule / fc_grid (lce_kernels_head.h): the load path needs K % 16.
inline void fc_i8_fill(FcI8Args& a, int32_t batch, int32_t inputs, int32_t outputs) { dense_fill(a, batch, inputs, outputs, kFcI8Tile); }
inline bool fc_i8_vec_rule(const FcI8Args& a) { return load_vec_rule(a.K, 16, a.in, a.filter); }
inline unsigned fc_i8_grid(const FcI8Args& a, uint64_t cap = 2048) { return stream_grid(a.tiles, 4, cap); }

// Launch the kernels on `stream`; return the launch's hipError_t as an int.  Defined in lce_tu_head_i8.hip.
int launch_fully_connected_i8(const FcI8Args& args, bool vec, void* stream);
int launch_mean_i8(const MeanI8Args& args, void* stream);
int launch_softmax_i8(const SoftmaxI8Args& args, void* stream);
int launch_quantize_f32_i8(const QuantArgs& args, void* stream);
int launch_dequantize_i8_f32(const QuantArgs& args, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// (a generic vector, which the host compiler of the simulation in tests/hostsim_head_i8 knows too)
typedef int32_t i32x4 __attribute__((vector_size(16)));

// MultiplyByQuantizedMultiplier (the double-rounding build) for a multiplier m and a shift split into left = max(e, 0) and
// right = max(-e, 0).  Compiled for both sides: the host tests run these very functions.
LCE_HOST_DEVICE int32_t head_i8_requantize(int32_t acc, int32_t m, int32_t left, int32_t right) {
  return add_i8_rdivpot(add_i8_srdhm((int32_t)((uint32_t)acc << left), m), right);
}

// One output of FULLY_CONNECTED from its accumulator (the sum of x w) and the channel's three constants.
LCE_HOST_DEVICE int32_t fc_i8_value(int32_t acc, int32_t cst, int32_t m, int32_t e, int32_t zo, int32_t act_min, int32_t act_max) {
  int32_t v = head_i8_requantize(acc + cst, m, e > 0 ? e : 0, e > 0 ? 0 : -e) + zo;
  v = v < act_min ? act_min : v;
  return v > act_max ? act_max : v;
}

// One output of MEAN from acc = sum (x - zi) over the n pixels: reference_integer_ops::Mean -- multiply, then divide rounding half
// away from zero (C++ int32 division truncates).
LCE_HOST_DEVICE int32_t mean_i8_value(int32_t acc, int32_t m, int32_t left, int32_t right, int32_t n, int32_t zo) {
  const int32_t t = head_i8_requantize(acc, m, left, right);
  const int32_t q = t > 0 ? (t + n / 2) / n : (t - n / 2) / n;
  const int32_t v = q + zo;
  return v < -128 ? -128 : (v > 127 ? 127 : v);
}

// QUANTIZE and DEQUANTIZE of one element.  `/` is the correctly rounded division and nothing contracts (-ffp-contract=off).
LCE_HOST_DEVICE int32_t quantize_i8_value(float x, float scale, int32_t zp) {
  const float lo = (float)(-128 - zp), hi = (float)(127 - zp);
  float r = __builtin_roundf(x / scale);         // half away from zero; +-inf stay, a NaN stays
  r = r < lo ? lo : r;
  r = r > hi ? hi : r;
  return (r != r ? 0 : (int32_t)r) + zp;
}
LCE_HOST_DEVICE float dequantize_i8_value(int32_t q, float scale, int32_t zp) { return (float)(q - zp) * scale; }

// The 16 bytes k .. k + 15 of one row as an operand; bytes at or beyond `lim` (K, or 0 for a row past the end) read as 0.
// VEC: k % 16 == 0 and K % 16 == 0, so all sixteen or none.
template <bool VEC>
LCE_DEVICE i32x4 fc_i8_load(const int8_t* row, uint32_t k, uint32_t lim) {
  i32x4 v = {0, 0, 0, 0};
  if constexpr (VEC) {
    if (k < lim) v = *(const i32x4*)(row + k);
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (k + (uint32_t)e < lim) v[e >> 2] |= (int32_t)((uint32_t)(uint8_t)row[k + (uint32_t)e] << (8 * (e & 3)));
  }
  return v;
}

template <bool VEC>
LCE_KERNEL void __launch_bounds__(256)
fully_connected_i8(const FcI8Args A) {
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t r = lane & 15u, g = lane >> 4;
  const uint32_t K = A.K;
  constexpr uint32_t kChunk = (uint32_t)(kFcI8Step * kFcI8Steps);
  for (uint32_t tile = (uint32_t)block_idx_x() * 4u + wave; tile < A.tiles; tile += (uint32_t)grid_dim_x() * 4u) {
    const uint32_t tm = tile / A.ntiles, tn = tile - tm * A.ntiles;
    const uint32_t m = tm * (uint32_t)kFcI8Tile + r, o = tn * (uint32_t)kFcI8Tile + r;   // this lane's row of x and of w
    const uint32_t xlim = m < A.M ? K : 0u, wlim = o < A.N ? K : 0u;
    const int8_t* xrow = A.in + (uint64_t)(m < A.M ? m : 0u) * K;
    const int8_t* wrow = A.filter + (uint64_t)(o < A.N ? o : 0u) * K;
    i32x4 acc = {0, 0, 0, 0};
    i32x4 xa[kFcI8Steps], wb[kFcI8Steps];
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kFcI8Steps; ++j) {
      xa[j] = fc_i8_load<VEC>(xrow, (uint32_t)kFcI8Step * j + 16u * g, xlim);
      wb[j] = fc_i8_load<VEC>(wrow, (uint32_t)kFcI8Step * j + 16u * g, wlim);
    }
    for (uint32_t k0 = 0; k0 < K; k0 += kChunk) {
      i32x4 xc[kFcI8Steps], wc[kFcI8Steps];
#pragma unroll
      for (uint32_t j = 0; j < (uint32_t)kFcI8Steps; ++j) { xc[j] = xa[j]; wc[j] = wb[j]; }
      if (k0 + kChunk < K) {                                                             // the next chunk, in flight behind this one
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)kFcI8Steps; ++j) {
          xa[j] = fc_i8_load<VEC>(xrow, k0 + kChunk + (uint32_t)kFcI8Step * j + 16u * g, xlim);
          wb[j] = fc_i8_load<VEC>(wrow, k0 + kChunk + (uint32_t)kFcI8Step * j + 16u * g, wlim);
        }
      }
      const uint32_t left = K - k0;
      const uint32_t steps = left >= kChunk ? (uint32_t)kFcI8Steps : (left + (uint32_t)kFcI8Step - 1u) / (uint32_t)kFcI8Step;
#pragma unroll
      for (uint32_t j = 0; j < (uint32_t)kFcI8Steps; ++j)
        if (j < steps) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(xc[j], wc[j], acc, 0, 0, 0);
    }
    // epilogue: register i is row 4 g + i of the tile, column r
    const bool col_ok = o < A.N;
    const uint32_t cs = col_ok ? o : 0u;
    const int32_t cst = A.table[cs], mul = A.table[(uint64_t)A.N + cs], exp = A.table[2ull * A.N + cs];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t row = tm * (uint32_t)kFcI8Tile + 4u * g + i;
      const int32_t v = fc_i8_value(acc[i], cst, mul, exp, A.zo, A.act_min, A.act_max);
      if (col_ok && row < A.M) A.out[(uint64_t)row * A.N + o] = (int8_t)v;
    }
  }
}

// WAVES: the waves of a block, one task (an image's 16 channels) each
template <int WAVES>
LCE_KERNEL void __launch_bounds__(64 * WAVES)
mean_i8(const MeanI8Args A) {
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t ch = lane & 15u, g = lane >> 4;
  const uint64_t tasks = A.batch * A.segs;
  for (uint64_t t = (uint64_t)block_idx_x() * WAVES + wave; t < tasks; t += (uint64_t)grid_dim_x() * WAVES) {
    const uint64_t b = t / A.segs;
    const uint32_t c = (uint32_t)(t - b * A.segs) * (uint32_t)kMeanI8Channels + ch;
    const bool ok = c < A.C;
    const int8_t* p = A.in + b * A.n * A.C + (ok ? c : 0u);
    int32_t acc = 0;
    if (ok) {
#pragma unroll 4
      for (uint32_t px = g; px < A.n; px += 4u) acc += (int32_t)p[(uint64_t)px * A.C];
    }
    acc += (int32_t)shfl_xor((uint32_t)acc, 16);
    acc += (int32_t)shfl_xor((uint32_t)acc, 32);
    acc -= (int32_t)A.n * A.zi;                                                          // sum (x - zi): |.| <= 255 n
    if (ok && g == 0u) A.out[b * A.C + c] = (int8_t)mean_i8_value(acc, A.mul, A.left, A.right, (int32_t)A.n, A.zo);
  }
}

LCE_DEVICE float softmax_i8_exp(int32_t d, float sb) { return head_exp((float)d * sb); }
LCE_DEVICE int32_t softmax_i8_value(float e, float s) {
  const float t = (e / s) * 256.0f;
  const int32_t v = (int32_t)__builtin_roundf(t) - 128;                                  // half away from zero; 0 <= t <= 256
  return v > 127 ? 127 : v;
}

template <int WAVES>
LCE_KERNEL void __launch_bounds__(64 * WAVES)
softmax_i8(const SoftmaxI8Args A) {
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  for (uint64_t row = (uint64_t)block_idx_x() * WAVES + wave; row < A.rows; row += (uint64_t)grid_dim_x() * WAVES) {
    const int8_t* x = A.in + row * A.cols;
    int8_t* y = A.out + row * A.cols;
    int32_t m = -128;
    for (uint32_t i = lane; i < A.cols; i += 64u) {
      const int32_t v = x[i];
      m = m < v ? v : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int32_t other = (int32_t)shfl_xor((uint32_t)m, d);
      m = m < other ? other : m;
    }
    float s = 0.0f;
    for (uint32_t i = lane; i < A.cols; i += 64u) s = s + softmax_i8_exp((int32_t)x[i] - m, A.sb);
    s = head_wave_sum(s);
    for (uint32_t i = lane; i < A.cols; i += 64u) y[i] = (int8_t)softmax_i8_value(softmax_i8_exp((int32_t)x[i] - m, A.sb), s);
  }
}

// QUANT: QUANTIZE (float in, int8 out); otherwise DEQUANTIZE (a template like every kernel here: one definition however many units
// include it)
template <bool QUANT>
LCE_KERNEL void __launch_bounds__(256)
quant_i8(const QuantArgs A) {
  const uint64_t step = (uint64_t)grid_dim_x() * 256ull;
  for (uint64_t i = (uint64_t)block_idx_x() * 256ull + (uint64_t)thread_idx_x(); i < A.n; i += step) {
    if constexpr (QUANT) ((int8_t*)A.out)[i] = (int8_t)quantize_i8_value(((const float*)A.in)[i], A.scale, A.zp);
    else ((float*)A.out)[i] = dequantize_i8_value((int32_t)((const int8_t*)A.in)[i], A.scale, A.zp);
  }
}

}  // namespace lce
#endif  // __HIPCC__
