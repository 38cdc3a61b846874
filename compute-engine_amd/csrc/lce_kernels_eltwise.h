// The float elementwise tail between binary layers of a converted residual network: TFLite's builtin ADD / MUL (batch norm
// constants, the residual shortcut) applied op by op, and the LceQuantize of the result, in one pass over the tensor
// (include/lce_hip.h, lce_hip_elementwise).  Per element of an NHWC float32 tensor x (rows = N*H*W, channels = C):
//
//   v = x;  for each step s:  v = fl(v op_s operand_s);  v = min(max(v, lo_s), hi_s)
//   out = v (optional);  bits: bit = v < 0, LSB first, ceil(C/32) words per row, padding bits 0 (optional)
//
// One rounding per op (tensorflow/lite/kernels/internal/reference: Add / Mul, then ActivationFunctionWithMinMax): the
// product and the sum are never contracted into an fma.  The clamp is std::min(std::max(v, lo), hi) with
// std::max(a, b) = a < b ? b : a, written as compares and selects -- v_max_f32 / v_med3_f32 may turn -0.0 into +0.0, which
// RELU(-0.0) = -0.0 forbids.  Subnormals pass through (the library is built without denormal flushing).
//
// Two paths, chosen from the input as lce_hip_bitpack chooses (lce_kernels.h: bitpack_f32_flat / bitpack_rows):
//   eltwise_flat : C % 32 == 0 and every pointer 16-byte aligned -- the tensor is one flat array of whole words; a wave
//                  turns 1024 floats (32 words) per iteration, 8 lanes per 128-byte line, four 16-byte loads of each
//                  tensor in flight per lane, and the 8 nibbles of a word are OR-reduced with 3 xor-shuffles.
//   eltwise_rows : anything else -- one wave per 64 columns of a row, one element per lane, one ballot per two words.
// The steps travel in the kernel arguments; every branch on them is wave-uniform.  `out` may alias `in` or a tensor
// operand: each element is read and written by the same lane, and no pointer is declared __restrict__.
//
// The extended chain (include/lce_hip.h, lce_hip_elementwise_ex) is the EX = 1 instance of the same two kernels; EX = 0, what
// lce_hip_elementwise launches, holds none of it.  It adds
//   a PER_IMAGE_CHANNEL operand : values[batch * channels], element (n, c) reads values[n * channels + c] (the gate of a
//                                 squeeze-and-excite block); the flat path carries the image of each 128-byte word the way it
//                                 carries the channel word: one division per launch, then advanced by the grid stride
//   CLAMP                       : no arithmetic, the step's clamp alone (a standalone RELU / RELU_N1_TO_1 / RELU6)
//   PRELU                       : v = v >= 0 ? v : fl(v * alpha), alpha the step's scalar or per-channel operand; no clamp
//   LOGISTIC                    : x >= 0: e = E(-x), y = 1 / fl(1 + e);  x < 0: e = E(x), y = e / fl(1 + e);  a NaN passes; no
//                                 clamp.  E is lce_kernels_exp.h's head_exp, the softmax's; both divisions correctly rounded.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"

namespace lce {

constexpr int kEwMaxSteps = 8;
enum { kEwAdd = 0, kEwMul = 1, kEwClamp = 2, kEwPrelu = 3, kEwLogistic = 4 };        // lce_hip_ew_op (from 2 on: EX only)
enum { kEwScalar = 0, kEwPerChannel = 1, kEwTensor = 2, kEwPerImageChannel = 3 };   // lce_hip_ew_operand (3: EX only)

struct EwStep {
  const float* values;       // [channels] (per channel), [rows * channels] (tensor) or [batch * channels] (per image); unused for a scalar
  float scalar;
  float lo, hi;              // CalculateActivationRange of the step's fused activation
  int32_t op, operand;
};

struct EwArgs {
  const float* in;
  float* out;                // null: no float output
  uint32_t* bits;            // null: no LceQuantize output
  uint64_t rows;
  uint32_t channels;
  uint32_t wpr;              // ceil(channels / 32)
  int32_t num_steps;         // 1..kEwMaxSteps
  EwStep steps[kEwMaxSteps];
};
// The arguments of the EX = 1 instances (the EX = 0 instances keep EwArgs, so their code is what it was).
struct EwArgsEx : EwArgs {
  uint64_t rows_per_image;   // H * W of the NHWC tensor: >= 1, divides rows
};
template <int EX> struct EwArgsOf { using type = EwArgs; };
template <> struct EwArgsOf<1> { using type = EwArgsEx; };

// Launches the flat path (flat == true; the caller has checked channels % 32 == 0 and 16-byte alignment) or the row path
// on `stream`; returns the launch's hipError_t as an int.  Defined in lce_tu_eltwise.hip.
int launch_eltwise(const EwArgs& args, bool flat, void* stream);
// The same for a chain that may hold the extended step kinds (the EX = 1 instances).  Defined in lce_tu_eltwise_ex.hip.
int launch_eltwise_ex(const EwArgsEx& args, bool flat, void* stream);
// The grid of both launchers.  Memory-bound streams: 4 waves per block, at most ~8 blocks per CU (kEwGridCap blocks), a wave
// strides over what is left (as lce_hip_api.hip's bitpack).
constexpr unsigned kEwGridCap = 256u * 8u;
inline unsigned eltwise_grid(uint64_t wave_tasks) {
  const uint64_t blocks = (wave_tasks + 3) / 4, cap = kEwGridCap;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

}  // namespace lce

#ifdef __HIPCC__
#include "lce_device_intrinsics.h"
#include "lce_kernels_exp.h"

namespace lce {
using namespace lce_dev;

// LOGISTIC as the header comment states it.  `/` is the correctly rounded division (hipcc's default for float).
LCE_DEVICE float ew_logistic(float x) {
  const bool pos = x >= 0.0f;
  const float e = head_exp(pos ? -x : x);
  const float y = (pos ? 1.0f : e) / __fadd_rn(1.0f, e);
  return x != x ? x : y;        // a NaN passes unchanged
}

LCE_DEVICE uint64_t ew_rows_per_image(const EwArgs&) { return 1ull; }
LCE_DEVICE uint64_t ew_rows_per_image(const EwArgsEx& a) { return a.rows_per_image; }

LCE_DEVICE float ew_clamp(float v, const EwStep& s) {
  v = v < s.lo ? s.lo : v;      // std::max(v, lo)
  v = s.hi < v ? s.hi : v;      // std::min(v, hi)
  return v;
}

LCE_DEVICE float ew_apply(float v, const EwStep& s, float operand) {
#pragma clang fp contract(off)
  v = s.op == kEwMul ? __fmul_rn(v, operand) : __fadd_rn(v, operand);
  v = v < s.lo ? s.lo : v;      // std::max(v, lo)
  v = s.hi < v ? s.hi : v;      // std::min(v, hi)
  return v;
}

LCE_DEVICE float ew_prelu(float v, float alpha) {
#pragma clang fp contract(off)
  return v >= 0.0f ? v : __fmul_rn(v, alpha);      // (a NaN takes the multiply)
}

template <int EX = 0>         // (a template so that only the translation unit that launches it emits it)
LCE_KERNEL void __launch_bounds__(256)
eltwise_flat(const typename EwArgsOf<EX>::type A, uint64_t total_words) {
  const int lane = thread_idx_x() & (kWave - 1);
  const int grp = lane >> 3, sub = lane & 7;
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks32 = (total_words + 31) / 32;
  // channel word (mod wpr) of this lane group's first word: one division per launch, then advanced by the grid stride
  const uint32_t wpr = A.wpr;
  uint32_t cw0 = (uint32_t)((wave0 * 32ull + (uint64_t)(grp * 4)) % wpr);
  const uint32_t cw_step = (uint32_t)((nwaves * 32ull) % wpr);
  // EX: the image of this lane group's first word and the word's place in it, kept the same way.  A wave's 32 words may span
  // many images (an image can be one word), so a per-image step steps the image word by word from here.
  const uint64_t wpi = EX ? ew_rows_per_image(A) * (uint64_t)wpr : 1ull;          // words per image, >= 1
  uint64_t img0 = EX ? (wave0 * 32ull + (uint64_t)(grp * 4)) / wpi : 0ull;
  uint64_t iw0 = EX ? (wave0 * 32ull + (uint64_t)(grp * 4)) - img0 * wpi : 0ull;
  const uint64_t img_step = EX ? (nwaves * 32ull) / wpi : 0ull;
  const uint64_t iw_step = EX ? (nwaves * 32ull) - img_step * wpi : 0ull;
  for (uint64_t blk = wave0; blk < nblocks32; blk += nwaves) {   // 32 words = 1024 floats
    const uint64_t word0 = blk * 32ull + (uint64_t)(grp * 4);     // word of v[0]; v[c] is word0 + c
    const uint64_t e0 = word0 * 32ull + (uint64_t)(sub * 4);      // element of v[0][0]
    bool ok[4];
    uint32_t chan[4];                                             // first channel of v[c]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ok[c] = word0 + (uint64_t)c < total_words;
      uint32_t w = cw0 + (uint32_t)c;
      while (w >= wpr) w -= wpr;                                  // (at most 3 times: wpr >= 1)
      chan[c] = w * 32u + (uint32_t)(sub * 4);
    }
    f32x4 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = ok[c] ? load_streaming((const f32x4*)(A.in + e0 + c * 32)) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < A.num_steps; ++s) {
      const EwStep& S = A.steps[s];
      // (the kind of a step is decided once per step, outside the 16 elements: each kind has its own straight-line code)
      if (EX && S.op == kEwLogistic) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = ew_logistic(v[c][k]);
        continue;
      }
      if (EX && S.op == kEwClamp) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = ew_clamp(v[c][k], S);
        continue;
      }
      f32x4 o[4];
      if (S.operand == kEwTensor) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          o[c] = ok[c] ? load_streaming((const f32x4*)(S.values + e0 + c * 32)) : f32x4{0.f, 0.f, 0.f, 0.f};
      } else if (S.operand == kEwPerChannel) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = *(const f32x4*)(S.values + chan[c]);   // small and cached: plain loads
      } else if (EX && S.operand == kEwPerImageChannel) {
        uint64_t img = img0, iw = iw0;                                            // image of v[c], and the word's place in it
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                             // (a word past the end has no image: not read)
          o[c] = ok[c] ? *(const f32x4*)(S.values + img * (uint64_t)A.channels + chan[c]) : f32x4{0.f, 0.f, 0.f, 0.f};
          if (++iw == wpi) { iw = 0; ++img; }
        }
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = f32x4{S.scalar, S.scalar, S.scalar, S.scalar};
      }
      if (EX && S.op == kEwPrelu) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = ew_prelu(v[c][k], o[c][k]);
        continue;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = ew_apply(v[c][k], S, o[c][k]);
    }
    if (A.out) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (ok[c]) *(f32x4*)(A.out + e0 + c * 32) = v[c];
    }
    if (A.bits) {
      u32x4 words;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t nib = (v[c][0] < 0.0f ? 1u : 0u) | (v[c][1] < 0.0f ? 2u : 0u) |
                             (v[c][2] < 0.0f ? 4u : 0u) | (v[c][3] < 0.0f ? 8u : 0u);
        uint32_t w = nib << (4 * sub);
        w |= shfl_xor(w, 1);
        w |= shfl_xor(w, 2);
        w |= shfl_xor(w, 4);
        words[c] = w;
      }
      if (sub == 0) {
        if (ok[3]) {
          *((u32x4*)(A.bits + word0)) = words;
        } else {                                                  // the last, partial block
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if (ok[c]) A.bits[word0 + c] = words[c];
        }
      }
    }
    cw0 += cw_step;
    if (cw0 >= wpr) cw0 -= wpr;
    if (EX) {
      img0 += img_step;
      iw0 += iw_step;
      if (iw0 >= wpi) { iw0 -= wpi; ++img0; }
    }
  }
}

template <int EX = 0>
LCE_KERNEL void __launch_bounds__(256)
eltwise_rows(const typename EwArgsOf<EX>::type A, uint32_t segs, uint64_t total_tasks) {
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t cols = A.channels;
  for (uint64_t t = wave0; t < total_tasks; t += nwaves) {
    const uint64_t row = t / segs;
    const uint32_t seg = (uint32_t)(t - row * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    bool neg = false;
    if (col < cols) {
      const uint64_t e = row * (uint64_t)cols + col;
      float v = A.in[e];
      for (int s = 0; s < A.num_steps; ++s) {
        const EwStep& S = A.steps[s];
        if (EX && S.op == kEwLogistic) { v = ew_logistic(v); continue; }
        if (EX && S.op == kEwClamp) { v = ew_clamp(v, S); continue; }
        float o = S.operand == kEwTensor ? S.values[e] : S.operand == kEwPerChannel ? S.values[col] : S.scalar;
        if (EX && S.operand == kEwPerImageChannel) o = S.values[(row / ew_rows_per_image(A)) * (uint64_t)cols + col];
        if (EX && S.op == kEwPrelu) { v = ew_prelu(v, o); continue; }
        v = ew_apply(v, S, o);
      }
      if (A.out) A.out[e] = v;
      neg = v < 0.0f;
    }
    if (A.bits) store_seg_bits(A.bits, A.wpr, row, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
