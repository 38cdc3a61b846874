// The channel join between binary layers of a converted DENSE network (BinaryDenseNet, MeliusNet: every binary layer's
// output is joined to its input by TFLite's builtin CONCATENATION on the channel axis) and the LceQuantize of the joined
// tensor, in one pass (include/lce_hip.h, lce_hip_concat).  2..8 NHWC tensors [rows, C_k] of one element type become
// [rows, sum C_k]:
//
//   out[r][start_k + c] = in_k[r][c]                       (a copy: NaN payloads, -0.0 and subnormals come through untouched)
//   bits: bit = out < 0 (float) / out < zero_point (int8), LSB first, ceil(sum C_k / 32) words per row, padding bits 0
//         (what lce_hip_bitpack writes for the joined tensor), from the values the copy holds in registers
//
// Two paths, chosen as lce_hip_bitpack / lce_hip_elementwise choose:
//   concat_vec  : every C_k x element size is a multiple of 16 bytes and every pointer 16-byte aligned (and, with bits, sum C_k
//                 a multiple of 32) -- the OUTPUT is one flat array of 16-byte chunks; lane l of a wave moves chunks
//                 base + l + 64 j, j = 0..3: four loads in flight per lane and 1024 contiguous bytes per store instruction.
//                 The (row, chunk-in-row) of a wave's base is divided out ONCE per wave and then advanced by the grid
//                 stride, whose quotient and remainder the host supplies; a lane's own offset (< 256 chunks) takes one
//                 32-bit multiply-high.  The input a chunk comes from is found by comparing against <= 7 chunk offsets
//                 that travel in the kernel arguments.  Float: a chunk is 4 sign bits, 8 neighbouring lanes make a word
//                 (3 xor-shuffles).  int8: a chunk is 16 bits from four byte-parallel compares, 2 neighbouring lanes make a
//                 word (one DPP quad permute).
//   concat_rows : anything else (ragged channel counts, unaligned pointers) -- one wave per 64 columns of an output row,
//                 one element per lane, one ballot per two words.
// All offsets are 64-bit (rows < 2^32, sum C_k < 2^31, their product unbounded).  No LDS, no scratch, nothing allocated:
// the launch is capturable.  Inputs may repeat; the output must not overlap an input (the row pitches differ).
#pragma once
#include <stdint.h>

#include "lce_kernel_args.h"

namespace lce {

constexpr int kConcatMaxInputs = 8;
enum { kConcatF32 = 0, kConcatI8 = 1, kConcatWords = 2 };         // element kinds: float32, int8, bitpacked int32 words

struct ConcatArgs {
  const void* in[kConcatMaxInputs];
  uint32_t width[kConcatMaxInputs];   // per row and input: 16-byte chunks (vector path) or elements (row path)
  uint32_t start[kConcatMaxInputs];   // where input k begins in an output row (same unit); 0xffffffff for k >= num_inputs
  void* out;                          // null: no joined tensor
  uint32_t* bits;                     // null: no LceQuantize output
  uint64_t rows;
  uint32_t total;                     // sum of width
  uint32_t wpr;                       // ceil(sum C_k / 32)
  int32_t zero_point;
  // vector path
  uint64_t total_chunks;              // rows * total
  uint64_t step_rows;                 // grid stride in chunks = step_rows * total + step_cols
  uint32_t step_cols;
  FastDiv div_total;
};

// Launches the vector path (vec == true; the caller has checked sizes and alignment and filled the vector-path fields for
// the grid concat_vec_grid() gives) or the row path on `stream`; returns the launch's hipError_t as an int.  Defined in
// lce_tu_concat.hip.
int launch_concat(const ConcatArgs& args, int kind, bool vec, void* stream);
// Blocks of 4 waves the vector path is launched with for `total_chunks` chunks (the host derives the grid stride from it).
unsigned concat_vec_grid(uint64_t total_chunks);

}  // namespace lce

#ifdef __HIPCC__
#include "lce_device_intrinsics.h"

namespace lce {
using namespace lce_dev;

LCE_DEVICE uint32_t concat_div(uint32_t n, FastDiv d) { return d.magic == 0u ? n : (mulhi_u32(n, d.magic) >> d.shift); }

// Four int8 values in one dword -> 4 bits, bit k = byte k < zero_point.  `t4` holds zero_point + 128 in every byte: with
// u = x ^ 0x80 per byte the comparison is unsigned, u < t, and per byte u < t <=> (~u & t) | (~(u ^ t) & ~d) at bit 7, where
// d = (u | 0x80) - (t & 0x7f) never borrows from the next byte.  The four bits 7, 15, 23, 31 are gathered by one multiply.
LCE_DEVICE uint32_t concat_lt4(uint32_t x, uint32_t t4) {
  const uint32_t H = 0x80808080u;
  const uint32_t u = x ^ H;
  const uint32_t d = (u | H) - (t4 & ~H);
  const uint32_t lt = ((~u & t4) | (~(u ^ t4) & ~d)) & H;
  return ((lt >> 7) * 0x01020408u) >> 24;                         // bits 0, 8, 16, 24 -> 24, 25, 26, 27
}

// v_mov_b32 quad_perm:[1,0,3,2]: the value of the neighbouring lane (lane ^ 1).  Every lane of the wave must be active.
LCE_DEVICE uint32_t concat_neighbour(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true); }

template <int KIND, bool BITS>
LCE_KERNEL void __launch_bounds__(256)
concat_vec(const ConcatArgs A) {
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (A.total_chunks + 255) / 256;
  // (row, chunk in the row) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint64_t row0 = (wave0 * 256ull) / A.total;
  uint32_t col0 = (uint32_t)(wave0 * 256ull - row0 * A.total);
  const uint32_t t4 = (uint32_t)(A.zero_point + 128) * 0x01010101u;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves) {       // 256 chunks = 4 KB per wave and iteration
    const uint64_t g0 = blk * 256ull + (uint64_t)lane;             // this lane's chunks: g0 + 64 j
    bool ok[4];
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ok[j] = g0 + 64u * j < A.total_chunks;
      const uint32_t x = col0 + (uint32_t)lane + 64u * j;          // < total + 256 < 2^31
      const uint32_t q = concat_div(x, A.div_total);
      const uint32_t c = x - q * A.total;
      const u32x4* src = (const u32x4*)A.in[0];
      uint32_t w = A.width[0], s = 0;
#pragma unroll
      for (int k = 1; k < kConcatMaxInputs; ++k)
        if (c >= A.start[k]) { src = (const u32x4*)A.in[k]; w = A.width[k]; s = A.start[k]; }
      const uint64_t off = (row0 + q) * (uint64_t)w + (uint64_t)(c - s);
      v[j] = ok[j] ? load_streaming(src + off) : u32x4{0u, 0u, 0u, 0u};
    }
    if (A.out) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok[j]) *((u32x4*)A.out + g0 + 64u * j) = v[j];
    }
    if constexpr (BITS && KIND == kConcatF32) {                    // total % 8 == 0: the 8 lanes of a word agree on ok[j]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 f = __builtin_bit_cast(f32x4, v[j]);
        const uint32_t nib = (f[0] < 0.0f ? 1u : 0u) | (f[1] < 0.0f ? 2u : 0u) | (f[2] < 0.0f ? 4u : 0u) | (f[3] < 0.0f ? 8u : 0u);
        uint32_t word = nib << (4 * (lane & 7));
        word |= shfl_xor(word, 1);
        word |= shfl_xor(word, 2);
        word |= shfl_xor(word, 4);
        if (ok[j] && (lane & 7) == 0) A.bits[(g0 + 64u * j) >> 3] = word;
      }
    }
    if constexpr (BITS && KIND == kConcatI8) {                     // total % 2 == 0: lanes 2p and 2p + 1 agree on ok[j]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t m = concat_lt4(v[j][0], t4) | (concat_lt4(v[j][1], t4) << 4) | (concat_lt4(v[j][2], t4) << 8) |
                           (concat_lt4(v[j][3], t4) << 12);
        uint32_t word = ok[j] ? m << (16 * (lane & 1)) : 0u;
        word |= concat_neighbour(word);
        if (ok[j] && (lane & 1) == 0) A.bits[(g0 + 64u * j) >> 1] = word;
      }
    }
    row0 += A.step_rows;
    col0 += A.step_cols;
    if (col0 >= A.total) { col0 -= A.total; ++row0; }
  }
}

template <typename E, int KIND>
LCE_KERNEL void __launch_bounds__(256)
concat_rows(const ConcatArgs A, uint32_t segs, uint64_t total_tasks) {
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t cols = A.total;
  for (uint64_t t = wave0; t < total_tasks; t += nwaves) {
    const uint64_t row = t / segs;
    const uint32_t seg = (uint32_t)(t - row * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    bool neg = false;
    if (col < cols) {
      const E* src = (const E*)A.in[0];
      uint32_t w = A.width[0], s = 0;
#pragma unroll
      for (int k = 1; k < kConcatMaxInputs; ++k)
        if (col >= A.start[k]) { src = (const E*)A.in[k]; w = A.width[k]; s = A.start[k]; }
      const E v = src[row * (uint64_t)w + (uint64_t)(col - s)];
      if (A.out) ((E*)A.out)[row * (uint64_t)cols + col] = v;
      if constexpr (KIND == kConcatF32) neg = __builtin_bit_cast(float, v) < 0.0f;
      if constexpr (KIND == kConcatI8) neg = (int32_t)v < A.zero_point;
    }
    if constexpr (KIND != kConcatWords) {
      if (A.bits) {
        const unsigned long long b = wave_ballot(neg);
        const uint32_t w = seg * 2u + (uint32_t)lane;
        if (lane < 2 && w < A.wpr) A.bits[row * (uint64_t)A.wpr + w] = (uint32_t)(b >> (32 * lane));
      }
    }
  }
}

}  // namespace lce
#endif  // __HIPCC__
