// The gate of a squeeze-and-excite block in an int8-converted network (RealToBinaryNet style): TFLite's builtin int8 MUL of the
// block's int8 output by a per-image gate [b, 1, 1, C] (or by a tensor of its own shape), the residual ADD of the shortcut behind it
// and the LceQuantize of the result, in one pass (include/lce_hip.h, lce_hip_mul_int8).  Per element, in int32 / int64:
//
//   p   = clamp(MBQM((x1 - z1) * (x2 - z2), m, e) + zo, lo, hi)                  the MUL's int8 result at ITS (so, zo)
//   out = p                                                                      without the ADD, or
//   out = add_i8_value<V>(p, addend) + zo_add                                    lce_kernels_eltwise_i8.h: the variant the host has
//                                                                                proven for the ADD's parameters over all 65 536 pairs
//   bit = out < zo of the LAST stage; LSB first, ceil(C/32) words per row, padding bits 0
//
// MBQM(x, m, e) = RDivPOT(SRDHM(x << max(e,0), m), max(-e,0)) with the SAME add_i8_srdhm / add_i8_rdivpot the ADD's literal formula
// is written in.  With the ADD a launch moves 3 bytes per element (x, the addend, the result) plus bits, where a MUL launch followed
// by lce_hip_add_int8 moves 5.  Written out, the literal MBQM is a 64-bit product with a sign-dependent nudge, a truncating 64-bit
// division and a mask / threshold rounding: with it the launch is ALU-bound at twice the bare ADD's time (profiles/gate_i8/
// layers.txt).  So the MUL stage has two VARIANTS that give the same bytes (mul_i8_requant), as the ADD has three:
//
//   kMulI8Literal : the formula as written.  The fallback: right for every parameter set.
//   kMulI8Fast    : e <= -1 and m > 0 (every MUL whose products span the int8 range: the real multiplier is far below 1/2):
//                   SRDHM(p, m) = (p m + 2^30) >> 31 in ONE v_mad_i64_i32 (floor: the sign-dependent nudge and the truncating
//                   division are exactly that) and RDivPOT(t, n) = (t + 2^(n-1) + (t >> 31)) >> n -- add_i8_value's output stage.
//
// The fast variant is never chosen on the strength of the algebra: the host runs its mul_i8_requant over ALL 130 051 products
// (x1 - z1)(x2 - z2) in [-65 025, 65 025] against the literal one and picks it only if every byte agrees (lce_hip_api.hip,
// mul_i8_fast_is_proven).  The function is compiled for both sides, so what the host proves is what the device runs.
//
// The two layouts of lce_kernels_eltwise_i8_chain.h:
//   mul_i8_flat : C % 16 == 0 and every pointer 16-byte aligned -- 16 bytes per lane and load, four loads of each tensor in
//                 flight.  A 16-byte chunk lies in ONE row (C % 16 == 0), so in one image: every lane computes its own row and
//                 image (64 lanes span several images when H * W * C is small) and reads its 16 gate bytes in one load; the gate
//                 is b * C bytes and stays in cache.  Bits: for C % 32 == 0 the two halves of a word meet in store_half_word's
//                 quad permute, as in the chain; for C % 32 == 16 a row has an odd number of chunks, so every lane stores its own
//                 16 bits (a row's last chunk the whole word: the upper half is padding, 0).
//   mul_i8_rows : anything else -- one wave per 64 columns of a row, one element per lane, one ballot per two words.  The row,
//                 and with it the image, is the wave's.
// `out` may alias x or the addend: each element is read and written by the same lane and all loads of an iteration come before
// its stores.  No LDS, no scratch; the parameters travel in the kernel arguments.  64-bit element offsets throughout.
#pragma once
#include <stdint.h>

#include "lce_kernels_eltwise_i8.h"

namespace lce {

enum { kMulI8NoAdd = kAddI8Variants };       // the ADD slot after the three ADD variants
enum { kMulI8Literal = 0, kMulI8Fast = 1, kMulI8Variants = 2 };   // lce_hip_mul_int8_launch::mul_variant

struct MulI8Args {
  AddI8Args A;               // out, bits, rows, channels, wpr; with an ADD its parameters in canonical order (in1 / in2 unused)
  const int8_t* x;           // [rows, channels]
  const int8_t* g;           // [rows, channels], or per image [rows / rows_per_image, channels]
  const int8_t* addend;      // [rows, channels]; unused without an ADD
  int32_t z1, z2, zo, m, left, right, lo, hi;   // the MUL stage: e = left - right, one of the two is 0
  int32_t half;              // kMulI8Fast: 2^(right - 1)
  int32_t zo_last;           // the zero point the bits are taken at
  uint32_t product_first;    // with an ADD: 1 when the product is the ADD's canonical input 1, 0 when the addend is
  uint32_t cpr;              // flat layout: channels / 16, the 16-byte chunks of a row
  uint64_t rows_per_image;   // per-image gate: H * W
};

// Launches MUL variant `mul` with ADD slot `add` (an kAddI8* or kMulI8NoAdd) for a tensor or a per-image operand on the flat or the
// row layout with `blocks` blocks of 256 threads; returns the hipError_t as an int.  Defined in lce_tu_mul_i8.hip.
int launch_mul_i8(const MulI8Args& args, int mul, int add, bool per_image, bool flat, unsigned blocks, void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// The MUL's int8 result (absolute, clamped) for the product p = (x1 - z1)(x2 - z2), |p| <= 65 025.
template <int MV>
LCE_HOST_DEVICE int32_t mul_i8_requant(const MulI8Args& M, int32_t p) {
  int32_t raw;
  if constexpr (MV == kMulI8Literal) {
    raw = add_i8_rdivpot(add_i8_srdhm((int32_t)((uint32_t)p << M.left), M.m), M.right) + M.zo;
  } else {
    const int32_t t = (int32_t)(((int64_t)p * (int64_t)M.m + (int64_t)(1 << 30)) >> 31);   // SRDHM(p, m), m > 0
    raw = ((t + M.half + (t >> 31)) >> M.right) + M.zo;                                     // RDivPOT(t, right), right >= 1
  }
  const int32_t q = raw < M.lo ? M.lo : raw;
  return q > M.hi ? M.hi : q;
}

// The launch's int8 result (absolute) for one element: the product, or the ADD of the product and the addend.
template <int MV, int V>
LCE_HOST_DEVICE int32_t mul_i8_element(const MulI8Args& M, int32_t x1, int32_t x2, int32_t ad) {
  const int32_t p = mul_i8_requant<MV>(M, add_i8_mul24(x1 - M.z1, x2 - M.z2));
  if constexpr (V == kMulI8NoAdd) return p;
  else return add_i8_value<V>(M.A, M.product_first ? p : ad, M.product_first ? ad : p) + M.A.zo;
}

// n / d; both are below 2^32 for every tensor short of 64 GiB, where the division is a 32-bit one
LCE_DEVICE uint64_t mul_i8_div(uint64_t n, uint64_t d) {
  return ((n | d) >> 32) == 0 ? (uint64_t)((uint32_t)n / (uint32_t)d) : n / d;
}

template <int MV, int V, bool PI>
LCE_KERNEL void __launch_bounds__(256)
mul_i8_flat(const MulI8Args M, uint64_t total_chunks) {            // chunk = 16 bytes = half a word of bits
  const AddI8Args& A = M.A;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (total_chunks + 255) / 256;
  const u32x4* xs = (const u32x4*)M.x;
  const u32x4* gs = (const u32x4*)M.g;
  const u32x4* as = (const u32x4*)M.addend;
  const uint32_t cpr = M.cpr;
  const bool odd = (cpr & 1u) != 0;                                // a row's last chunk has no partner (uniform)
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 256 chunks = 4096 elements per wave and iteration
    const uint64_t c0 = blk * 256ull + (uint64_t)lane;             // this lane's chunks: c0 + 64 j
    bool ok[4];
    u32x4 a[4], b[4], d[4];
    uint64_t row[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = c0 + 64u * j < total_chunks;   // (cpr even: the count is even, lanes 2p and 2p + 1 agree)
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ok[j] ? load_streaming(xs + c0 + 64u * j) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t ch = c0 + 64u * j;
      row[j] = 0;
      if (PI || odd) row[j] = mul_i8_div(ch, cpr);
      if constexpr (PI) {
        const uint64_t image = mul_i8_div(row[j], M.rows_per_image);
        const uint64_t at = image * cpr + (ch - row[j] * cpr);     // the gate's chunk: this lane's image, this chunk's channels
        b[j] = ok[j] ? gs[at] : u32x4{0u, 0u, 0u, 0u};
      } else {
        b[j] = ok[j] ? load_streaming(gs + ch) : u32x4{0u, 0u, 0u, 0u};
      }
    }
    if constexpr (V != kMulI8NoAdd) {
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = ok[j] ? load_streaming(as + c0 + 64u * j) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t ch = c0 + 64u * j;
      u32x4 o;
      uint32_t m = 0;                                              // 16 sign bits
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int32_t q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int32_t ad = V != kMulI8NoAdd ? (int32_t)(int8_t)(d[j][w] >> (8 * k)) : 0;
          q[k] = mul_i8_element<MV, V>(M, (int32_t)(int8_t)(a[j][w] >> (8 * k)), (int32_t)(int8_t)(b[j][w] >> (8 * k)), ad);
          m |= (uint32_t)(q[k] < M.zo_last) << (4 * w + k);
        }
        o[w] = pack4_u8(q[0], q[1], q[2], q[3]);
      }
      if (A.out && ok[j]) *((u32x4*)A.out + ch) = o;
      if (A.bits) {
        if (!odd) {
          store_half_word<false>(A.bits, ch, lane, ok[j], m);
        } else if (ok[j]) {
          const uint32_t r = (uint32_t)(ch - row[j] * cpr);        // a row is cpr + 1 half words: half word r of row `row` is ch + row
          if (r + 1u == cpr) A.bits[row[j] * (uint64_t)A.wpr + (r >> 1)] = m;   // (r is even) the upper half is padding
          else ((uint16_t*)A.bits)[ch + row[j]] = (uint16_t)m;
        }
      }
    }
  }
}

template <int MV, int V, bool PI>
LCE_KERNEL void __launch_bounds__(256)
mul_i8_rows(const MulI8Args M, uint32_t segs, uint64_t total_tasks) {
  const AddI8Args& A = M.A;
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t cols = A.channels;
  for (uint64_t t = wave0; t < total_tasks; t += nwaves) {
    const uint64_t row = t / segs;
    const uint32_t seg = (uint32_t)(t - row * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    const uint64_t grow = PI ? mul_i8_div(row, M.rows_per_image) : row;   // the operand's row: the image's, or the element's
    bool neg = false;
    if (col < cols) {
      const uint64_t e = row * (uint64_t)cols + col;
      const int32_t ad = V != kMulI8NoAdd ? (int32_t)M.addend[e] : 0;
      const int32_t q = mul_i8_element<MV, V>(M, (int32_t)M.x[e], (int32_t)M.g[grow * (uint64_t)cols + col], ad);
      if (A.out) A.out[e] = (int8_t)q;
      neg = q < M.zo_last;
    }
    if (A.bits) store_seg_bits(A.bits, A.wpr, row, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
