// The int8 tail of a ReActNet-style block between binary layers of an int8-converted network -- residual ADD, ADD of a
// per-channel shift, PRELU, ADD of a shift, a standalone RELU, the int8 -> int8 requantize in front of a CONCATENATION -- and the
// LceQuantize of the result, in one pass over an NHWC int8 tensor (include/lce_hip.h, lce_hip_elementwise_i8).
//
// Every step but the tensor + tensor ADD is a function of ONE int8 value and its channel, so a whole chain of them is one
// 256-entry table per channel.  The host evaluates the steps' literal arithmetic for all 256 inputs of every channel once per
// model (lce_hip_api.hip, lce_hip_elementwise_i8_prepare); the device does NO step arithmetic:
//
//   v   = in                        or the head ADD of (in, addend): add_i8_value<V> of lce_kernels_eltwise_i8.h, the variant
//                                   proven for its parameters over all 65 536 pairs as lce_hip_add_int8 proves it
//   out = table[c][v + 128]         (R = channels rows of 256 bytes, or R = 1 when no step is per channel)
//   bit = (int8)out < zo            zo: the LAST step's zero point; LSB first, ceil(C/32) words per row, padding bits 0
//
// The memory layouts are add_i8_flat's and add_i8_rows' (same header): the flat path for C % 32 == 0 and 16-byte aligned
// pointers (16 bytes per lane and load, four loads in flight, the two halves of a word meet in one DPP quad permute), one wave
// per 64 columns of a row otherwise (one ballot per two words).  Three places for the table, each a path of its own:
//
//   kEwI8Lds    : the block copies the R rows into LDS once and every wave of it strides over the tensor.  A lane of the flat
//                 path reads 16 DIFFERENT rows (its 16 channels), and for a given byte position k the 32 lanes of an LDS lane
//                 group read the rows of channels 16 (r + l) + k.  ds_read_u8 banks by (address / 4) mod 32, so rows of 256 bytes
//                 would put every row on the same banks (the bank would be the VALUE's, and activations crowd round the zero
//                 point), and rows padded to 260 bytes in channel order would still leave only two distinct banks (channels 16
//                 apart).  So the rows are stored at a pitch of 260 bytes (65 dwords) in the order
//                     flat: row(c) = (c mod 16) * (C / 16) + c / 16        rows path: row(c) = c
//                 which makes the rows one lane group reads for one k CONSECUTIVE: equal values in different channels fall on
//                 consecutive banks, equal values in the same channel are one address (a broadcast).
//                 LDS: 260 R bytes of the 160 KiB; the largest C is 608 (flat) / 630 (rows).  Above 16 KiB of table the block
//                 has 16 waves instead of 4, so that a CU whose LDS holds one or two tables still has 16 to 32 waves in flight.
//   kEwI8Global : the table stays in global memory ([R][256], as prepare writes it) and is read through the cache with byte
//                 loads; for C beyond the LDS path.
//   kEwI8OneRow : R = 1: the 256 bytes in LDS, one row for every channel (equal values are one address).
//
// `out` may alias either input: each element is read and written by the same lane and all loads of an iteration come before
// its stores.  No scratch.  64-bit element offsets throughout.
#pragma once
#include <stdint.h>

#include "lce_kernels_eltwise_i8.h"

namespace lce {

enum { kEwI8Lds = 0, kEwI8Global = 1, kEwI8OneRow = 2, kEwI8Paths = 3 };   // lce_hip_elementwise_i8_path_id
enum { kEwI8NoHead = kAddI8Variants };                                      // the head slot after the three ADD variants
constexpr uint32_t kEwI8LdsPitch = 260;                                     // bytes per table row in LDS
constexpr uint32_t kEwI8LdsLimit = 160u * 1024u;                            // per workgroup on gfx950
constexpr uint32_t kEwI8WideBlockAbove = 16u * 1024u;                       // LDS table bytes above which a block has 16 waves

struct EwI8Args {
  AddI8Args A;               // tensors and sizes; with a head its parameters in canonical order (in1 may be the addend); without
                             // one in1 is the input and in2 is unused
  const uint8_t* table;      // [R][256] on the device, 4-byte aligned
  int32_t zo_last;
  uint32_t cpr;              // flat path: channels / 16, the 16-byte chunks of a row
};

// Launches head variant `head` (an kAddI8* or kEwI8NoHead) with the table at `path` on the flat or the row layout: `blocks`
// blocks of `threads` threads (256 or 1024) and `lds_bytes` of dynamic LDS.  Returns the hipError_t as an int.  Defined in
// lce_tu_eltwise_i8_chain.hip.
int launch_ew_i8(const EwI8Args& args, int head, int path, bool flat, unsigned blocks, unsigned threads, unsigned lds_bytes,
                 void* stream);

}  // namespace lce

#ifdef __HIPCC__
namespace lce {

// Where channel c's row lies in LDS (in rows of kEwI8LdsPitch bytes).
template <bool FLAT>
LCE_DEVICE uint32_t ew_i8_lds_row(uint32_t c, uint32_t cpr) {
  if constexpr (FLAT) return (c & 15u) * cpr + (c >> 4);
  else return c;
}

// The block's copy of the table into LDS and the barrier behind it (every thread of the block calls it).
template <int P, bool FLAT>
LCE_DEVICE void ew_i8_stage_table(const EwI8Args& E, uint8_t* lds) {
  if constexpr (P != kEwI8Global) {
    const uint32_t dwords = (P == kEwI8OneRow ? 1u : E.A.channels) * 64u;
    const uint32_t* src = (const uint32_t*)E.table;
    for (uint32_t i = (uint32_t)thread_idx_x(); i < dwords; i += (uint32_t)block_dim_x()) {
      const uint32_t c = i >> 6, d = i & 63u;
      const uint32_t row = P == kEwI8OneRow ? 0u : ew_i8_lds_row<FLAT>(c, E.cpr);
      *(uint32_t*)(lds + row * kEwI8LdsPitch + 4u * d) = src[i];
    }
    block_barrier_keep_vm();
  }
}

template <int P>
LCE_DEVICE uint32_t ew_i8_lookup(const EwI8Args& E, const uint8_t* lds, uint32_t row_off, uint32_t u) {
  if constexpr (P == kEwI8Global) return (uint32_t)E.table[row_off + u];
  else return (uint32_t)lds[row_off + u];
}

// a + b mod m for a, b < m < 2^31
LCE_DEVICE uint32_t ew_i8_add_mod(uint32_t a, uint32_t b, uint32_t m) {
  const uint32_t s = a + b;
  return s >= m ? s - m : s;
}

template <int H, int P>
LCE_KERNEL void __launch_bounds__(1024)
ew_i8_flat(const EwI8Args E, uint64_t total_chunks) {              // chunk = 16 bytes = half a word of bits; the count is even
  const AddI8Args& A = E.A;
  uint8_t* lds = P == kEwI8Global ? nullptr : lds_base();
  ew_i8_stage_table<P, true>(E, lds);
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint64_t nblocks = (total_chunks + 255) / 256;
  const u32x4* in1 = (const u32x4*)A.in1;
  const u32x4* in2 = (const u32x4*)A.in2;
  // the chunk's place in its row, kept by modular steps: one 64-bit remainder per thread, none in the loop
  const uint32_t cpr = E.cpr;
  uint32_t r0 = (uint32_t)((wave0 * 256ull + (uint64_t)lane) % cpr);
  const uint32_t step_j = 64u % cpr, step_it = (uint32_t)((nwaves * 256ull) % cpr);
  // byte offset of the row of channel 16 r + k: r * row_step + k * k_step
  const uint32_t row_step = P == kEwI8Lds ? kEwI8LdsPitch : P == kEwI8Global ? 4096u : 0u;
  const uint32_t k_step = P == kEwI8Lds ? cpr * kEwI8LdsPitch : P == kEwI8Global ? 256u : 0u;
  for (uint64_t blk = wave0; blk < nblocks; blk += nwaves, r0 = ew_i8_add_mod(r0, step_it, cpr)) {
    const uint64_t c0 = blk * 256ull + (uint64_t)lane;             // this lane's chunks: c0 + 64 j
    bool ok[4];
    u32x4 a[4], b[4];
    uint32_t rj[4];
    rj[0] = r0;
#pragma unroll
    for (int j = 1; j < 4; ++j) rj[j] = ew_i8_add_mod(rj[j - 1], step_j, cpr);
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = c0 + 64u * j < total_chunks;   // (lanes 2p and 2p + 1 agree: the count is even)
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ok[j] ? load_streaming(in1 + c0 + 64u * j) : u32x4{0u, 0u, 0u, 0u};
    if constexpr (H != kEwI8NoHead) {
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = ok[j] ? load_streaming(in2 + c0 + 64u * j) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u32x4 o;
      uint32_t m = 0;                                              // 16 sign bits
      const uint32_t base = rj[j] * row_step;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          uint32_t u;
          if constexpr (H == kEwI8NoHead) {
            u = ((a[j][w] >> (8 * k)) & 0xffu) ^ 0x80u;
          } else {
            u = (uint32_t)(add_i8_value<H>(A, (int32_t)(int8_t)(a[j][w] >> (8 * k)), (int32_t)(int8_t)(b[j][w] >> (8 * k))) +
                           A.zo + 128);
          }
          t[k] = ew_i8_lookup<P>(E, lds, base + (uint32_t)(4 * w + k) * k_step, u);
          m |= (uint32_t)((int32_t)(int8_t)t[k] < E.zo_last) << (4 * w + k);
        }
        o[w] = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
      }
      if (A.out && ok[j]) *((u32x4*)A.out + c0 + 64u * j) = o;
      if (A.bits) {                                                // (store_half_word's text: through it two instances come out different)
        uint32_t word = m << (16 * (lane & 1));
        word |= lane_neighbour(word);
        if (ok[j] && (lane & 1) == 0) A.bits[(c0 + 64u * j) >> 1] = word;
      }
    }
  }
}

template <int H, int P>
LCE_KERNEL void __launch_bounds__(1024)
ew_i8_rows(const EwI8Args E, uint32_t segs, uint64_t total_tasks) {
  const AddI8Args& A = E.A;
  uint8_t* lds = P == kEwI8Global ? nullptr : lds_base();
  ew_i8_stage_table<P, false>(E, lds);
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  const uint32_t cols = A.channels;
  const uint32_t row_step = P == kEwI8Lds ? kEwI8LdsPitch : P == kEwI8Global ? 256u : 0u;
  for (uint64_t t = wave0; t < total_tasks; t += nwaves) {
    const uint64_t row = t / segs;
    const uint32_t seg = (uint32_t)(t - row * segs);
    const uint32_t col = seg * 64u + (uint32_t)lane;
    bool neg = false;
    if (col < cols) {
      const uint64_t e = row * (uint64_t)cols + col;
      uint32_t u;
      if constexpr (H == kEwI8NoHead) u = (uint32_t)((int32_t)A.in1[e] + 128);
      else u = (uint32_t)(add_i8_value<H>(A, (int32_t)A.in1[e], (int32_t)A.in2[e]) + A.zo + 128);
      const uint32_t q = ew_i8_lookup<P>(E, lds, col * row_step, u);
      if (A.out) A.out[e] = (int8_t)q;
      neg = (int32_t)(int8_t)q < E.zo_last;
    }
    if (A.bits) store_seg_bits(A.bits, A.wpr, row, seg, lane, neg);
  }
}

}  // namespace lce
#endif  // __HIPCC__
