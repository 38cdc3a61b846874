// The int8 residual ADD between binary layers of an int8-converted residual network (Bi-RealNet style: batch norm folded into
// LceBconv2d's multiplier and bias, the shortcut added by TFLite's builtin int8 ADD) and the LceQuantize of the sum, in one
// pass over two NHWC int8 tensors (include/lce_hip.h, lce_hip_add_int8).  Byte for byte the int8 branch of TFLite's ADD in its
// default (double-rounding) build -- Prepare's QuantizeMultiplier parameters, reference_integer_ops::Add per element:
//
//   a = (x1 - z1) << 20;  b = (x2 - z2) << 20
//   sa = RDivPOT(SRDHM(a, m1), n1);  sb = RDivPOT(SRDHM(b, m2), n2)              (n = -shift >= 0)
//   out = min(hi, max(lo, RDivPOT(SRDHM(sa + sb, mo), no) + zo))
//   bits: bit = out < zo, LSB first, ceil(C/32) words per row, padding bits 0 (what lce_hip_bitpack(I8, ..., zo, ...) writes)
//
// which is NOT the correctly rounded (s1 (x1 - z1) + s2 (x2 - z2)) / so.  Written out, that is three 32x32->64 multiplies with
// sign-dependent nudges, a truncating 64-bit division and three mask / threshold roundings per element: ALU-bound on gfx950.
// Three VARIANTS of the per-element arithmetic give the same bytes (add_i8_value):
//
//   kAddI8Literal : the formula as TFLite writes it.  The fallback: right for every parameter set.
//   kAddI8Split   : input 1 is a shift, sa = (x1 - z1) << k (its multiplier is 2^30: always so for the input with the larger
//                   scale).  Input 2 in 24-bit multiply-adds: with d = x2 - z2 and m2 = mh 2^11 + ml,
//                   SRDHM(d << 20, m2) = floor((d m2 + 2^10) / 2^11) = d mh + ((d ml + 2^10) >> 11), no 64-bit product; the
//                   output stage is ONE v_mad_i64_i32, SRDHM(s, mo) = (s mo + 2^30) >> 31 (floor: the sign-dependent nudge
//                   and the truncating division are exactly that), and RDivPOT(t, n) = (t + 2^(n-1) + (t >> 31)) >> n.
//   kAddI8Shift   : both inputs are shifts (equal scales, or a power-of-two ratio): s = x1 ka + x2 kb + c.
//
// The identities hold for the operand ranges that occur, but a variant is never chosen on the strength of the algebra: the
// host runs the variant's own add_i8_value over all 65 536 (x1, x2) pairs against the literal one and picks it only if every
// byte agrees (lce_hip_api.hip, prepared_add_int8 -- the precedent is int8_one_instruction_forms, docs/kernels.md 4.15).
// The function below is compiled for both sides, so what the host proves is what the device runs.
//
// Two paths, chosen as lce_hip_bitpack / lce_hip_elementwise choose:
//   add_i8_flat : C % 32 == 0 and every pointer 16-byte aligned -- the tensors are flat arrays; a lane turns 16 bytes of each
//                 input per load, four loads of each tensor in flight, 64 lanes x 16 contiguous bytes per load instruction;
//                 a lane's 16 sign bits meet its neighbour's and the even lane stores the word (store_half_word).
//   add_i8_rows : anything else -- one wave per 64 columns of a row, one element per lane, one ballot per two words.
// `out` may alias either input: each element is read and written by the same lane, all loads of an iteration come before
// its stores, and no pointer is declared __restrict__.  No LDS, no scratch; the parameters travel in the kernel arguments.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"

namespace lce {

enum { kAddI8Literal = 0, kAddI8Split = 1, kAddI8Shift = 2, kAddI8Variants = 3 };   // lce_hip_add_int8_variant

struct AddI8Args {
  const int8_t* in1;         // canonical order: the launcher has swapped the inputs so that a shift-form input comes first
  const int8_t* in2;
  int8_t* out;               // null: no int8 output
  uint32_t* bits;            // null: no LceQuantize output
  uint64_t rows;
  uint32_t channels;
  uint32_t wpr;              // ceil(channels / 32)
  // the literal formula (lce_hip_add_int8_params; n = -shift)
  int32_t z1, z2, zo, m1, n1, m2, n2, mo, no, lo, hi;
  // kAddI8Shift: sa + sb = x1 ka + x2 kb + c.  kAddI8Split: sa = x1 ka + c, sb from d = x2 - z2, ml, mh, nb, half_b
  int32_t ka, kb, c;
  int32_t ml, mh, nb, half_b;
  int32_t half_o;            // 2^(no - 1)
  int32_t lo_rel, hi_rel;    // lo - zo, hi - zo
};

// Launches variant `variant` on the flat path (flat == true; the caller has checked channels % 32 == 0 and 16-byte
// alignment) or the row path on `stream`; returns the launch's hipError_t as an int.  Defined in lce_tu_eltwise_i8.hip.
int launch_add_i8(const AddI8Args& args, int variant, bool flat, void* stream);

}  // namespace lce

#ifdef __HIPCC__
#include "lce_device_intrinsics.h"

#define LCE_HOST_DEVICE __host__ __device__ __forceinline__

namespace lce {
using namespace lce_dev;

// a * b for |a|, |b| < 2^23 (v_mul_i32_i24 / v_mad_i32_i24: full rate, where v_mul_lo_u32 is not).  The host side of the proof
// multiplies in full, so an operand that did not fit would show as a mismatch there.
LCE_HOST_DEVICE int32_t add_i8_mul24(int32_t a, int32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __mul24(a, b);
#else
  return (int32_t)((int64_t)a * b);
#endif
}

// gemmlowp's SaturatingRoundingDoublingHighMul and RoundingDivideByPOT as TFLite's reference kernels call them
LCE_HOST_DEVICE int32_t add_i8_srdhm(int32_t a, int32_t b) {
  if (a == b && a == INT32_MIN) return INT32_MAX;
  const int64_t p = (int64_t)a * (int64_t)b;
  const int64_t nudge = p >= 0 ? (int64_t)(1 << 30) : (int64_t)(1 - (1 << 30));
  return (int32_t)((p + nudge) / (int64_t)(1ll << 31));
}
LCE_HOST_DEVICE int32_t add_i8_rdivpot(int32_t x, int32_t n) {       // 0 <= n <= 31
  const int32_t mask = (int32_t)((1u << n) - 1u);
  const int32_t rem = x & mask;
  const int32_t thr = (mask >> 1) + (x < 0 ? 1 : 0);
  return (x >> n) + (rem > thr ? 1 : 0);
}

// The sum of one (x1, x2) pair RELATIVE to the output zero point, clamped: out = value + zo, bit = value < 0.
template <int V>
LCE_HOST_DEVICE int32_t add_i8_value(const AddI8Args& A, int32_t x1, int32_t x2) {
  if constexpr (V == kAddI8Literal) {
    const int32_t a = (int32_t)((uint32_t)(x1 - A.z1) << 20), b = (int32_t)((uint32_t)(x2 - A.z2) << 20);
    const int32_t sa = add_i8_rdivpot(add_i8_srdhm(a, A.m1), A.n1);
    const int32_t sb = add_i8_rdivpot(add_i8_srdhm(b, A.m2), A.n2);
    const int32_t raw = add_i8_rdivpot(add_i8_srdhm(sa + sb, A.mo), A.no) + A.zo;
    const int32_t q = raw < A.lo ? A.lo : raw;
    return (q > A.hi ? A.hi : q) - A.zo;
  } else {
    int32_t s;
    if constexpr (V == kAddI8Shift) {
      s = add_i8_mul24(x1, A.ka) + (add_i8_mul24(x2, A.kb) + A.c);
    } else {
      const int32_t d = x2 - A.z2;
      const int32_t u = add_i8_mul24(d, A.ml) + (1 << 10);
      int32_t v = add_i8_mul24(d, A.mh) + (u >> 11);              // SRDHM(d << 20, m2)
      v = (v + A.half_b + (v >> 31)) >> A.nb;                      // RDivPOT(v, nb), nb >= 1
      s = add_i8_mul24(x1, A.ka) + (v + A.c);
    }
    const int32_t t = (int32_t)(((int64_t)s * (int64_t)A.mo + (int64_t)(1 << 30)) >> 31);   // SRDHM(s, mo), mo > 0
    const int32_t r = (t + A.half_o + (t >> 31)) >> A.no;          // RDivPOT(t, no), no >= 1
    const int32_t q = r < A.lo_rel ? A.lo_rel : r;
    return q > A.hi_rel ? A.hi_rel : q;
  }
}

template <int V>
LCE_KERNEL void __launch_bounds__(256)
add_i8_flat(const AddI8Args A, uint64_t total_chunks) {           // chunk = 16 bytes = half a word of bits; the count is even
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (total_chunks + 255) / 256;
  const u32x4* in1 = (const u32x4*)A.in1;
  const u32x4* in2 = (const u32x4*)A.in2;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 256 chunks = 4096 elements per wave and iteration
    const uint64_t c0 = blk * 256ull + (uint64_t)lane;             // this lane's chunks: c0 + 64 j
    bool ok[4];
    u32x4 a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = c0 + 64u * j < total_chunks;   // (lanes 2p and 2p + 1 agree: the count is even)
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ok[j] ? load_streaming(in1 + c0 + 64u * j) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = ok[j] ? load_streaming(in2 + c0 + 64u * j) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u32x4 o;
      uint32_t m = 0;                                              // 16 sign bits
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int32_t q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          q[k] = add_i8_value<V>(A, (int32_t)(int8_t)(a[j][w] >> (8 * k)), (int32_t)(int8_t)(b[j][w] >> (8 * k)));
          m |= ((uint32_t)q[k] >> 31) << (4 * w + k);
        }
        o[w] = pack4_u8(q[0] + A.zo, q[1] + A.zo, q[2] + A.zo, q[3] + A.zo);
      }
      if (A.out && ok[j]) *((u32x4*)A.out + c0 + 64u * j) = o;
      if (A.bits) store_half_word<false>(A.bits, c0 + 64u * j, lane, ok[j], m);
    }
  }
}

template <int V>
LCE_KERNEL void __launch_bounds__(256)
add_i8_rows(const AddI8Args A, uint32_t segs, uint64_t total_tasks) {
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
      const int32_t q = add_i8_value<V>(A, (int32_t)A.in1[e], (int32_t)A.in2[e]);
      if (A.out) A.out[e] = (int8_t)(q + A.zo);
      neg = q < 0;
    }
    if (A.bits) store_seg_bits(A.bits, A.wpr, row, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
