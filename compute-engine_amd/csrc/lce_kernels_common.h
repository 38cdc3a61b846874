// What more than one family of section kernels uses (pools, depthwise, joins, the float and the int8 CONV_2D): a host part, and
// a device part for hipcc and for the host simulations of the kernels (tests/hostsim_*).
#pragma once
#include <stdint.h>

#include "lce_kernel_args.h"

namespace lce {

// ComputePaddingHeightWidth: of the SAME padding along one axis, total / 2 goes in front.
inline int32_t same_pad_before(int32_t out, int32_t stride, int32_t filter, int32_t in) {
  const int64_t total = (int64_t)(out - 1) * stride + filter - in;
  return (int32_t)((total > 0 ? total : 0) / 2);
}

// What the launch descriptors of the float and the int8 CONV_2D (Conv2dArgs, ConvI8Args) have in common, for a convolution whose
// sizes the caller has checked and whose output extents oh x ow it knows: the channel counts, K = fh fw Cin < 2^31 and its
// contiguous runs, the extents, the strides and the padding in front.
template <typename Args>
inline void conv_window_geometry(Args& a, int32_t in_height, int32_t in_width, int32_t channels_in, int32_t channels_out, int32_t filter_height,
                                 int32_t filter_width, int32_t stride_height, int32_t stride_width, int32_t oh, int32_t ow) {
  const uint64_t Cin = (uint64_t)channels_in, N = (uint64_t)channels_out;
  a.Cin = (uint32_t)Cin; a.Cout = (uint32_t)N; a.wpr = (uint32_t)((N + 31) / 32);
  a.K = (uint32_t)((uint64_t)filter_height * filter_width * Cin);
  a.rowlen = (uint32_t)((uint64_t)filter_width * Cin);
  a.in_row = (uint64_t)in_width * Cin;
  a.IH = in_height; a.IW = in_width; a.OH = oh; a.OW = ow;
  a.sh = stride_height; a.sw = stride_width;
  a.ph = same_pad_before(oh, stride_height, filter_height, in_height);
  a.pw = same_pad_before(ow, stride_width, filter_width, in_width);
}

// The grid of a grid-strided launch: `per_block` tasks to a block (4 wave tasks; 256 for a kernel of one element per lane), at
// least one block (no entry launches on nothing) and at most `cap` (the product: ~8 per CU; a host simulation passes a small one).
inline unsigned stream_grid(uint64_t tasks, unsigned per_block = 4, uint64_t cap = 2048) {
  const uint64_t blocks = (tasks + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// The 16-byte load path of the matrix kernels: K's contiguous run `k` a multiple of a load's `width` elements, both operands aligned.
inline bool load_vec_rule(uint64_t k, unsigned width, const void* in, const void* filter) {
  return k % width == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)filter % 16 == 0;
}

// M, K, N and the tile counts of a Dense layer's launch (FcArgs, FcI8Args, BfcArgs): one wave per tile x tile outputs.
template <typename Args>
inline void dense_fill(Args& a, int32_t batch, int32_t inputs, int32_t outputs, uint32_t tile) {
  a.M = (uint32_t)batch; a.K = (uint32_t)inputs; a.N = (uint32_t)outputs;
  a.ntiles = (a.N + tile - 1) / tile;
  a.tiles = ((a.M + tile - 1) / tile) * a.ntiles;
}

// CalculateActivationRange (tensorflow/lite/kernels/kernel_util.h) for float and an lce_hip_activation (NONE, RELU, RELU_N1_TO_1,
// RELU6 = 0 .. 3).  False, and the range of NONE, for an activation that is none of the four.
inline bool float_activation_range(int32_t activation, float* lo, float* hi) {
  *lo = -3.402823466e+38f;      // -FLT_MAX
  *hi = 3.402823466e+38f;
  switch (activation) {
    case 0: return true;
    case 1: *lo = 0.0f; return true;
    case 2: *lo = -1.0f; *hi = 1.0f; return true;
    case 3: *lo = 0.0f; *hi = 6.0f; return true;
    default: return false;
  }
}

}  // namespace lce

#ifdef __HIPCC__
#include <lce_device_intrinsics.h>  // resolved through -I: csrc/ for the product, the host replacement for the simulations

namespace lce {
using namespace lce_dev;

// n / d for n < 2^31 and a launch constant d (make_fastdiv, lce_kernel_args.h): one v_mul_hi and a shift.
LCE_DEVICE uint32_t fast_div(uint32_t n, FastDiv d) { return d.magic == 0u ? n : (mulhi_u32(n, d.magic) >> d.shift); }

// The ballots of accumulator registers 4 G .. 4 G + 3 of one 32x32 instruction tile, whose rows are pixels and whose columns
// are channels: register 4 G + i holds pixel 8 G + i of the wave's 32 in lanes 0..31 and pixel 8 G + 4 + i in lanes 32..63, so
// the two halves of b[i] are those two pixels' bit words.  Each goes to the lane of its pixel in `words` (v_writelane: no
// lane masks to keep; the ballots are settled once per group, lce_device_intrinsics.h).
template <int G>
LCE_DEVICE void tile_words(unsigned long long (&b)[4], uint32_t& words) {
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

// How the section kernels write bits from the registers of the pass.  A kernel keeps its own three prologue lines (lane, wave0,
// nwaves from thread_idx_x / block_idx_x / block_dim_x / grid_dim_x): behind a helper the compiler fetches blockDim the long way
// (docs/kernels.md, "Shared device helpers").  The two word helpers form the word's address in front of the shuffles: written
// inside the `if`, the compiler orders the or and the address arithmetic of every caller the other way round.

// The row path: lane l of a wave holds column seg * 64 + l of row `row` and `neg`, its bit (false beyond the row's end); one
// ballot is the row's words seg * 2 and seg * 2 + 1, which lanes 0 and 1 store if the row has them.  Every lane of the wave must
// be active; row and seg are the wave's.
LCE_DEVICE void store_seg_bits(uint32_t* bits, uint32_t wpr, uint64_t row, uint32_t seg, int lane, bool neg) {
  const unsigned long long bal = wave_ballot(neg);
  const uint32_t wd = seg * 2u + (uint32_t)lane;
  if (lane < 2 && wd < wpr) bits[row * (uint64_t)wpr + wd] = (uint32_t)(bal >> (32 * lane));
}

// v_mov_b32 quad_perm:[1,0,3,2]: the value of the neighbouring lane (lane ^ 1).  Every lane of the wave must be active.
LCE_DEVICE uint32_t lane_neighbour(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true); }

// A float 16-byte chunk is 4 sign bits (`nib`), and the 8 neighbouring lanes that hold chunks g & ~7 .. g | 7 make word g >> 3 with
// three xor-shuffles; the first of them stores it.  Every lane of the wave must be active; the 8 lanes of a word must agree on ok
// (the chunk count is a multiple of 8).
LCE_DEVICE void store_nibble_word(uint32_t* bits, uint64_t g, int lane, bool ok, uint32_t nib) {
  uint32_t* at = bits + (g >> 3);
  uint32_t word = nib << (4 * (lane & 7));
  word |= shfl_xor(word, 1);
  word |= shfl_xor(word, 2);
  word |= shfl_xor(word, 4);
  if (ok && (lane & 7) == 0) *at = word;
}

// An int8 16-byte chunk is 16 bits (`m`), and lanes 2p and 2p + 1, which hold chunks g and g + 1, make word g >> 1 with one
// lane_neighbour; the even lane stores it.  Every lane of the wave must be active; the two lanes of a word must agree on ok (the
// chunk count is even).  ZERO_PAST_END: a lane past the end contributes 0 (the kernels on PoolArgs; the flat
// elementwise kernels, whose lanes past the end compute on zeros, leave it out -- such a word is never stored either way).
template <bool ZERO_PAST_END>
LCE_DEVICE void store_half_word(uint32_t* bits, uint64_t g, int lane, bool ok, uint32_t m) {
  uint32_t* at = bits + (g >> 1);
  uint32_t word = ZERO_PAST_END ? (ok ? m << (16 * (lane & 1)) : 0u) : m << (16 * (lane & 1));
  word |= lane_neighbour(word);
  if (ok && (lane & 1) == 0) *at = word;
}

}  // namespace lce
#endif  // __HIPCC__
