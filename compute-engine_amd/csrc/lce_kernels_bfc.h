// The binarized Dense layer of a converted network (larq's QuantDense behind a sign: BinaryAlexNet's and XNOR-Net's classifier
// layers, every binarized MLP) on the FP4 matrix cores: lce_hip_binary_fully_connected (include/lce_hip.h).
//
// The converter has no binary fully-connected operator: it leaves LceQuantize -> LceDequantize -> a float FULLY_CONNECTED whose
// row o holds only +-s[o] (the +-1 kernel times the batch-norm scale folded in).  lce_hip_bfc_prepare splits such weights into
// their sign bits [N][ceil(K/32)] and s[N]; this kernel reads the BITS of the activations (the LceQuantize's output) and never
// the dequantized floats.  A GEMM: M = images, N = outputs, K = inputs; a [M][Kw] and w [N][Kw] words of 32 channels, LSB first,
// bit 1 = -1.  Per output element:
//
//   t = sum over k < K of a_k * w_k            (a_k, w_k in {+1, -1}: an exact integer, |t| <= K < 2^23; as a float +0.0f when zero)
//   p = t * s[o]                               (one float32 multiply)
//   v = p + bias[o]                            (one float32 add, never contracted with the multiply; no bias: no add)
//   v = min(max(v, lo), hi)                    (head_clamp's comparisons: a NaN passes, -0.0 stays -0.0)
//   bit = v < 0                                (LceQuantize's rule: -0.0 and NaN give 0; padding bits of a ragged last word are 0)
//
// Every partial sum is an integer below 2^24, so the order of the sum does not matter and t is exact.  For s[o] a power of two
// every product x[k] * w[o][k] of the float entry and every partial sum of its chain is exact too, and the two entries give the
// same bytes (tests/test_gpu_binary_dense.py); for other s[o] this entry rounds once where the float chain rounds K times.
//
// The tile.  ONE WAVE owns a 32 x 32 tile of outputs (rows = images, columns = outputs) and its whole K loop on
// v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 operands (lce_device_intrinsics.h: lane l supplies row / column l & 31 and the 32 K
// values of half l >> 5).  It is the SCALED form with explicit unit scales (mfma_fp4_32x32x64), not the unscaled one the
// streaming and pointwise families use: that one relies on the compiler selecting the unscaled encoding and is guarded by a
// known-answer launch that allocates and copies (lce_mfma_selftest.h), which an entry that promises to allocate nothing and to
// be capturable from its first call cannot run; the scaled form needs no guard, and its two extra issue cycles per instruction
// vanish behind the 34 VALU of the expansion.  Four waves to a block, each with its own tile, the launch grid-strided past 8 blocks per compute unit.
// 256 x 4096 outputs are 1024 tiles: one wave for every SIMD of the device.
//
// The operands are expanded IN THE K LOOP, from bit words to FP4 codes in registers (fp4_of_full_word: 17 VALU per 32 channels),
// and prepare stores the weights as bits, not as FP4: expanded they would be 16 times the bytes (9216 -> 4096: 75 MB against
// 4.7 MB), and at batch <= 32 a launch is bound by that stream.  The price is 34 VALU per instruction of the matrix pipe: a
// wave alone on its SIMD (256 x 4096 outputs) spends ~1.2 us per chunk of 8 instructions, nine times the roofline of the layer
// and a small fraction of the float chain's time (profiles/binary_dense/layers.txt).  Sharing one expansion among several column
// tiles of a wave, and splitting K where a launch has few tiles, are the next things to try.
// Operands come STRAIGHT FROM GLOBAL MEMORY, no LDS stage, as in lce_kernels_head.h: a tile has no second wave to share a staged
// chunk with.  Because the sum is order-free, the K axis is PERMUTED to make the loads wide: K advances in chunks of 16 words
// (512 channels); half h of the wave takes the 8 consecutive words 16 c + 8 h .. + 7 of its row -- two 16-byte loads when
// Kw % 4 == 0 and the pointers are 16-byte aligned, eight 4-byte loads otherwise -- and instruction j of the chunk multiplies
// word j of both halves.  Both operands use the same permutation.  The chunk after the one being multiplied is loaded before
// its instructions are issued.  A chunk runs min(8, Kw - 16 c) instructions.
//
// Padding is FP4 ZERO codes, never sign codes: LceQuantize leaves an activation's padding bits 0, which would read as +1.  The
// channels beyond K of a ragged last word (fp4_of_word with its count of valid channels, on BOTH operands), the words beyond Kw
// of a chunk's second half, and the rows and columns past the end all expand to code 0: their products are zeros.  Only the LAST
// chunk can hold the end of K, so only it decides per word (decided in every chunk, the three cases compile to ~90 VALU per
// word instead of 17).  In the
// chunks of 16 whole words a row or column past the end pads through the expansion's own lookup table -- 0 instead of the four
// sign pairs -- at no instruction.
//
// The epilogue works from the accumulator layout: register r of lane l is column l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5).
// A column is a lane, so s[o] and bias[o] are one load per lane, a value row is a 128-byte store, and a row's 32 bits -- one
// whole output word, because a tile is 32 columns wide -- are one half of a ballot, stored by the first lane of that half.
// Columns past N vote 0.
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"

namespace lce {

constexpr int kBfcTile = 32;           // rows and columns of a wave's tile
constexpr int kBfcChunkWords = 16;     // words of K per chunk: 8 per half of the wave, 8 instructions

struct BfcArgs {
  const uint32_t* in;        // [M][Kw] activation bits
  const uint32_t* weights;   // [N][Kw] sign bits (lce_hip_bfc_prepare)
  const float* scale;        // [N]
  const float* bias;         // null: none
  float* out;                // [M][N]; null: none
  uint32_t* bits;            // [M][ceil(N/32)]; null: none
  uint32_t M, K, N, Kw;
  uint32_t ntiles;           // ceil(N / 32)
  uint32_t tiles;            // ceil(M / 32) * ntiles < 2^31
  float lo, hi;              // CalculateActivationRange (float)
};

// As fc_fill / fc_vec_rule / fc_grid (lce_kernels_head.h): Kw = ceil(K / 32) words per row, and the load path needs Kw % 4.
inline void bfc_fill(BfcArgs& a, int32_t batch, int32_t inputs, int32_t outputs) {
  dense_fill(a, batch, inputs, outputs, kBfcTile);
  a.Kw = (a.K + 31) / 32;
}
inline bool bfc_vec_rule(const BfcArgs& a) { return load_vec_rule(a.Kw, 4, a.in, a.weights); }
inline unsigned bfc_grid(const BfcArgs& a, uint64_t cap = 2048) { return stream_grid(a.tiles, 4, cap); }

// Launch the kernel on `stream`; return the launch's hipError_t as an int.  Defined in lce_tu_bfc.hip.
int launch_binary_fully_connected(const BfcArgs& args, bool vec, void* stream);

}  // namespace lce

#ifdef __HIPCC__
#include "lce_kernels_head.h"      // head_clamp
#include "lce_kernels_mfma.h"      // fp4_of_word, fp4_of_full_word

namespace lce {
using namespace lce_dev;

// The 8 words first .. first + 7 of one row; words at or beyond `lim` (Kw, or 0 for a row past the end) read as 0.  VEC: two
// 16-byte loads (Kw % 4 == 0 and first % 4 == 0: all four words of a load or none).
template <bool VEC>
LCE_DEVICE void bfc_load_chunk(const uint32_t* row, uint32_t first, uint32_t lim, uint32_t (&w)[8]) {
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) w[j] = 0u;
  if constexpr (VEC) {
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q)
      if (first + 4u * q < lim) {
        const u32x4 v = *(const u32x4*)(row + first + 4u * q);
        w[4 * q + 0] = v[0]; w[4 * q + 1] = v[1]; w[4 * q + 2] = v[2]; w[4 * q + 3] = v[3];
      }
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j)
      if (first + j < lim) w[j] = row[first + j];
  }
}

// fp4_of_full_word (lce_kernels_mfma.h) with the table of its last lookup as an argument: kBfcSigns gives its codes, 0 gives 32 zero
// codes at the same 17 VALU -- how a row or column past the end pads, with no instruction of its own.
constexpr uint32_t kBfcSigns = 0xAAA22A22u;                      // the pairs {++, -+, +-, --} = {0x22, 0x2A, 0xA2, 0xAA}
LCE_DEVICE u32x4 bfc_fp4_of_full_word(uint32_t word, uint32_t table) {
  const uint32_t w2 = word >> 2;
  u32x4 v;
  auto one = [&](uint32_t sel) LCE_LAMBDA_INLINE {
    const uint32_t u = pk_lshr_b16<0, 4>(perm_b32(w2, word, sel)) & 0x03030303u;
    return perm_b32(0u, table, u);
  };
  v[0] = one(0x04000400u); v[1] = one(0x05010501u); v[2] = one(0x06020602u); v[3] = one(0x07030703u);
  return v;
}

// Word `index` of a row as 32 FP4 codes where the chunk holds the end of K: the channels at or beyond K -- a ragged last word's, a
// whole word's at or beyond Kw, every channel of a row past the end (lim = 0) -- are code 0.
LCE_DEVICE u32x4 bfc_expand_tail(uint32_t word, uint32_t index, uint32_t lim, uint32_t K) {
  if (index >= lim) return u32x4{0u, 0u, 0u, 0u};
  const uint32_t left = K - 32u * index;                        // index < Kw: at least one channel
  return left >= 32u ? fp4_of_full_word(word) : fp4_of_word(word, (int)left);
}

template <bool VEC>
LCE_KERNEL void __launch_bounds__(256)
binary_fully_connected(const BfcArgs A) {
  const uint32_t tid = (uint32_t)thread_idx_x();
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t K = A.K, Kw = A.Kw;
  const uint32_t whole = (K / 32u) / (uint32_t)kBfcChunkWords * (uint32_t)kBfcChunkWords;  // words in chunks of 16 whole words
  for (uint32_t tile = (uint32_t)block_idx_x() * 4u + wave; tile < A.tiles; tile += (uint32_t)grid_dim_x() * 4u) {
    const uint32_t tm = tile / A.ntiles, tn = tile - tm * A.ntiles;
    const uint32_t m = tm * (uint32_t)kBfcTile + r, o = tn * (uint32_t)kBfcTile + r;       // this lane's row of a and of w
    const uint32_t alim = m < A.M ? Kw : 0u, wlim = o < A.N ? Kw : 0u;
    const uint32_t* arow = A.in + (uint64_t)(m < A.M ? m : 0u) * Kw;
    const uint32_t* wrow = A.weights + (uint64_t)(o < A.N ? o : 0u) * Kw;
    const uint32_t atable = m < A.M ? kBfcSigns : 0u, wtable = o < A.N ? kBfcSigns : 0u;
    f32x16 acc = f32x16_zero();
    uint32_t an[8], wn[8];
    bfc_load_chunk<VEC>(arow, 8u * h, alim, an);
    bfc_load_chunk<VEC>(wrow, 8u * h, wlim, wn);
    uint32_t c0 = 0;
    // the chunks of 16 whole words: every word of both halves exists and is full, so nothing is decided per word
    for (; c0 < whole; c0 += (uint32_t)kBfcChunkWords) {
      uint32_t ac[8], wc[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) { ac[j] = an[j]; wc[j] = wn[j]; }
      // the next chunk, in flight behind this one (a load past the end of the row reads nothing)
      bfc_load_chunk<VEC>(arow, c0 + (uint32_t)kBfcChunkWords + 8u * h, alim, an);
      bfc_load_chunk<VEC>(wrow, c0 + (uint32_t)kBfcChunkWords + 8u * h, wlim, wn);
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j)
        acc = mfma_fp4_32x32x64(bfc_fp4_of_full_word(ac[j], atable), bfc_fp4_of_full_word(wc[j], wtable), acc);
    }
    // the last chunk, when it holds the end of K
    for (; c0 < Kw; c0 += (uint32_t)kBfcChunkWords) {
      uint32_t ac[8], wc[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) { ac[j] = an[j]; wc[j] = wn[j]; }
      // the next chunk, in flight behind this one (a load past the end of the row reads nothing)
      bfc_load_chunk<VEC>(arow, c0 + (uint32_t)kBfcChunkWords + 8u * h, alim, an);
      bfc_load_chunk<VEC>(wrow, c0 + (uint32_t)kBfcChunkWords + 8u * h, wlim, wn);
      const uint32_t left = Kw - c0;
      const uint32_t steps = left >= 8u ? 8u : left;                                       // instructions: the first half's words
      const uint32_t first = c0 + 8u * h;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j)
        if (j < steps) {
          const u32x4 a = bfc_expand_tail(ac[j], first + j, alim, K);
          const u32x4 b = bfc_expand_tail(wc[j], first + j, wlim, K);
          acc = mfma_fp4_32x32x64(a, b, acc);
        }
    }
    // epilogue: register i is row (i & 3) + 8 (i >> 2) + 4 h of the tile, column r
    const bool col_ok = o < A.N;
    const float scale = col_ok ? A.scale[o] : 1.0f;
    const float bias = A.bias != nullptr && col_ok ? A.bias[o] : 0.0f;
    const uint32_t wpr = A.ntiles;                                                         // words of a row of the bit output
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
      const uint32_t row = tm * (uint32_t)kBfcTile + (i & 3u) + 8u * (i >> 2) + 4u * h;
      const float t = acc[i] + 0.0f;                                                       // an integer; +0.0f when zero
      float v = A.bias != nullptr ? mul_then_add(t, scale, bias) : t * scale;
      v = head_clamp(v, A.lo, A.hi);
      if (A.out != nullptr && col_ok && row < A.M) A.out[(uint64_t)row * A.N + o] = v;
      if (A.bits != nullptr) {
        const unsigned long long vote = wave_ballot(col_ok && v < 0.0f);                   // (every lane of the wave is here)
        if (r == 0u && row < A.M) A.bits[(uint64_t)row * wpr + tn] = (uint32_t)(vote >> (32u * h));
      }
    }
  }
}

}  // namespace lce
#endif  // __HIPCC__
