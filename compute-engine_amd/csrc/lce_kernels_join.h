// The channel join (include/lce_hip.h: lce_hip_concat, lce_hip_join_windows).  A source is a channel WINDOW [begin, begin + count)
// of a tensor [rows, pitch]; a float window may have a dense [rows, count] tensor added on the way through.  The join between the
// binary layers of a converted DENSE network (BinaryDenseNet, MeliusNet: TFLite's builtin CONCATENATION on the channel axis) is the
// case begin = 0, count = pitch without addends; MeliusNet's improvement block -- y = CONCATENATION(x[..., :C-64], x[..., C-64:] + w)
// -- is one launch; a standalone channel slice (TFLite's STRIDED_SLICE / SLICE on the last axis) is the one-window case.  Either
// way the LceQuantize of the joined tensor comes out of the same pass.
//
//   out[r][start_k + c] = src_k[r][begin_k + c]                      (a copy: NaN payloads, -0.0 and subnormals come through untouched)
//   out[r][start_k + c] = fl(src_k[r][begin_k + c] + addend_k[r][c]) (one float32 add, round to nearest even, subnormals kept)
//   bits: bit = out < 0 (float) / out < zero_point (int8), LSB first, ceil(sum count / 32) words per row, padding bits 0
//         (what lce_hip_bitpack writes for the joined tensor), from the values the pass holds in registers (after the add)
//
// Two paths, chosen as lce_hip_bitpack / lce_hip_elementwise choose:
//   join_vec  : every begin, count and pitch x element size is a multiple of 16 bytes, every pointer 16-byte aligned (and, with
//               bits, sum count a multiple of 32) -- the OUTPUT is one flat array of 16-byte chunks; lane l of a wave moves
//               chunks base + l + 64 j, j = 0..3: four loads in flight per lane and 1024 contiguous bytes per store instruction.
//               The (row, chunk in row) of a wave's base is divided out ONCE per wave and then advanced by the grid stride,
//               whose quotient and remainder the host supplies; a lane's own offset (< 256 chunks) takes one 32-bit
//               multiply-high.  The window a chunk comes from is found by comparing against <= 7 chunk offsets that travel in
//               the kernel arguments.  All loads of an iteration (sources and addends) are issued before the first add.
//               Float: a chunk is 4 sign bits, 8 neighbouring lanes make a word (3 xor-shuffles).  int8: a chunk is 16 bits
//               from four byte-parallel compares, 2 neighbouring lanes make a word (lane_neighbour).  The words and the row
//               path's ballot are written out here, not through lce_kernels_common.h's helpers: with them the compiler orders
//               the instructions of four of the nine kernels differently (docs/kernels.md, "Shared device helpers").
//   join_rows : anything else (ragged channel counts, unaligned pointers) -- one wave per 64 columns of an output row, one
//               element per lane, one ballot per two words.
// A launch without any addend runs an instance that holds no addend code.  All offsets are 64-bit (rows < 2^32, sum count and
// every pitch < 2^31, their product unbounded).  No LDS, no scratch, nothing allocated, the window table travels in the kernel
// arguments: the launch is capturable.  Sources may repeat and windows of one source may overlap; the outputs must not overlap a
// source or an addend (the row pitches differ, so there is no in-place join).
#pragma once
#include <stdint.h>

#include "lce_kernels_common.h"

namespace lce {

constexpr int kJoinMaxWindows = 8;
// Element kinds.  kJoinF32: 4-byte elements; the sign test only where bits are asked for (so bitpacked int32 words, which
// have no bit output, are joined as kJoinF32).  kJoinI8: int8.
enum { kJoinF32 = 0, kJoinI8 = 1 };

struct JoinArgs {
  const void* src[kJoinMaxWindows];       // the window's first element in row 0 (the source tensor's base + begin)
  const float* addend[kJoinMaxWindows];   // null: the window is a copy
  uint32_t pitch[kJoinMaxWindows];        // per source row: 16-byte chunks (vector path) or elements (row path)
  uint32_t count[kJoinMaxWindows];        // the window's width = the addend's row pitch (same unit)
  uint32_t start[kJoinMaxWindows];        // where window k begins in an output row (same unit); 0xffffffff for k >= num_windows
  void* out;                              // null: no joined tensor
  uint32_t* bits;                         // null: no LceQuantize output
  uint64_t rows;
  uint32_t total;                         // sum of count
  uint32_t wpr;                           // ceil(sum count in elements / 32)
  int32_t zero_point;
  // vector path
  uint64_t total_chunks;                  // rows * total
  uint64_t step_rows;                     // grid stride in chunks = step_rows * total + step_cols
  uint32_t step_cols;
  FastDiv div_total;
};

// A window as the entry point takes it, in elements.
struct JoinWindow {
  const void* src;
  const float* addend;
  uint32_t pitch, begin, count;
};

// The path of a launch (true: join_vec) and everything of `a` but the grid stride.  The caller has checked the windows.
inline bool join_fill(JoinArgs& a, int kind, const JoinWindow* w, int n, uint64_t rows, int32_t zero_point, void* out, uint32_t* bits) {
  const uint64_t esz = kind == kJoinI8 ? 1 : 4;
  uint64_t sum = 0;
  bool vec = (uintptr_t)out % 16 == 0 && (uintptr_t)bits % 4 == 0;
  for (int k = 0; k < n; ++k) {
    sum += w[k].count;
    vec = vec && (uintptr_t)w[k].src % 16 == 0 && (uintptr_t)w[k].addend % 16 == 0 && ((uint64_t)w[k].pitch * esz) % 16 == 0 &&
          ((uint64_t)w[k].begin * esz) % 16 == 0 && ((uint64_t)w[k].count * esz) % 16 == 0;
  }
  if (bits && sum % 32 != 0) vec = false;   // (a word of bits then straddles rows of chunks)
  a = JoinArgs{};
  const uint32_t unit = vec ? (uint32_t)(16 / esz) : 1u;
  uint32_t at = 0;
  for (int k = 0; k < kJoinMaxWindows; ++k) {
    if (k >= n) { a.start[k] = 0xffffffffu; continue; }
    a.src[k] = (const char*)w[k].src + (uint64_t)w[k].begin * esz;
    a.addend[k] = w[k].addend;
    a.pitch[k] = w[k].pitch / unit;
    a.count[k] = w[k].count / unit;
    a.start[k] = at;
    at += a.count[k];
  }
  a.out = out;
  a.bits = bits;
  a.rows = rows;
  a.total = at;
  a.wpr = (uint32_t)((sum + 31) / 32);
  a.zero_point = zero_point;
  if (vec) {
    a.total_chunks = rows * (uint64_t)at;
    a.div_total = make_fastdiv(at);
  }
  return vec;
}
// The vector path's grid stride for a launch of `blocks` blocks of 4 waves.
inline void join_set_stride(JoinArgs& a, unsigned blocks) {
  const uint64_t stride = (uint64_t)blocks * 4ull * 256ull;   // chunks per grid step
  a.step_rows = stride / a.total;
  a.step_cols = (uint32_t)(stride % a.total);
}
inline bool join_has_addend(const JoinArgs& a) {
  for (int k = 0; k < kJoinMaxWindows; ++k)
    if (a.addend[k]) return true;
  return false;
}

// Launches the vector path (vec == true: `args` is join_fill's, with the stride of join_vec_grid()) or the row path on
// `stream`; returns the launch's hipError_t as an int.  Defined in lce_tu_join.hip.
int launch_join(const JoinArgs& args, int kind, bool vec, void* stream);
// Blocks of 4 waves the vector path is launched with for `total_chunks` chunks.
unsigned join_vec_grid(uint64_t total_chunks);

}  // namespace lce

#ifdef __HIPCC__
#include "lce_device_intrinsics.h"

namespace lce {
using namespace lce_dev;

// Four int8 values in one dword -> 4 bits, bit k = byte k < zero_point.  `t4` holds zero_point + 128 in every byte: with
// u = x ^ 0x80 per byte the comparison is unsigned, u < t, and per byte u < t <=> (~u & t) | (~(u ^ t) & ~d) at bit 7, where
// d = (u | 0x80) - (t & 0x7f) never borrows from the next byte.  The four bits 7, 15, 23, 31 are gathered by one multiply.
LCE_DEVICE uint32_t join_lt4(uint32_t x, uint32_t t4) {
  const uint32_t H = 0x80808080u;
  const uint32_t u = x ^ H;
  const uint32_t d = (u | H) - (t4 & ~H);
  const uint32_t lt = ((~u & t4) | (~(u ^ t4) & ~d)) & H;
  return ((lt >> 7) * 0x01020408u) >> 24;                         // bits 0, 8, 16, 24 -> 24, 25, 26, 27
}

template <int KIND, bool BITS, bool ADD>
LCE_KERNEL void __launch_bounds__(256)
join_vec(const JoinArgs A) {
  static_assert(!(ADD && KIND != kJoinF32), "only a float window has an addend");
  const int lane = thread_idx_x() & (kWave - 1);
  const uint64_t wave0 = (uint64_t)block_idx_x() * (uint64_t)(block_dim_x() >> 6) + (uint64_t)(thread_idx_x() >> 6);
  const uint64_t nwaves = (uint64_t)grid_dim_x() * (uint64_t)(block_dim_x() >> 6);
  // (row, chunk in the row) of this wave's first chunk: one division per launch, then advanced by the grid stride
  uint64_t row0 = (wave0 * 256ull) / A.total;
  uint32_t col0 = (uint32_t)(wave0 * 256ull - row0 * A.total);
  const uint32_t t4 = (uint32_t)(A.zero_point + 128) * 0x01010101u;
  for (uint64_t blk = wave0; blk * 256ull < A.total_chunks; blk += nwaves) {   // 256 chunks = 4 KB per wave and iteration
    const uint64_t g0 = blk * 256ull + (uint64_t)lane;             // this lane's chunks: g0 + 64 j
    bool ok[4], has[4];
    u32x4 v[4];
    f32x4 ad[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ok[j] = g0 + 64u * j < A.total_chunks;
      const uint32_t x = col0 + (uint32_t)lane + 64u * j;          // < total + 256 < 2^31
      const uint32_t q = fast_div(x, A.div_total);
      const uint32_t c = x - q * A.total;
      const u32x4* src = (const u32x4*)A.src[0];
      const f32x4* add = (const f32x4*)A.addend[0];
      uint32_t p = A.pitch[0], w = A.count[0], s = 0;
#pragma unroll
      for (int k = 1; k < kJoinMaxWindows; ++k)
        if (c >= A.start[k]) { src = (const u32x4*)A.src[k]; add = (const f32x4*)A.addend[k]; p = A.pitch[k]; w = A.count[k]; s = A.start[k]; }
      const uint64_t row = row0 + q;
      v[j] = ok[j] ? load_streaming(src + (row * (uint64_t)p + (uint64_t)(c - s))) : u32x4{0u, 0u, 0u, 0u};
      if constexpr (ADD) {
        has[j] = ok[j] && add != nullptr;
        ad[j] = has[j] ? load_streaming(add + (row * (uint64_t)w + (uint64_t)(c - s))) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    if constexpr (ADD) {                                           // (x + 0 is no copy of -0.0: only where there is an addend)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (has[j]) {
          const f32x4 f = __builtin_bit_cast(f32x4, v[j]);
          const f32x4 r = {f[0] + ad[j][0], f[1] + ad[j][1], f[2] + ad[j][2], f[3] + ad[j][3]};
          v[j] = __builtin_bit_cast(u32x4, r);
        }
    }
    if (A.out) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok[j]) *((u32x4*)A.out + g0 + 64u * j) = v[j];
    }
    if constexpr (BITS && KIND == kJoinF32) {                      // total % 8 == 0: the 8 lanes of a word agree on ok[j]
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
    if constexpr (BITS && KIND == kJoinI8) {                       // total % 2 == 0: lanes 2p and 2p + 1 agree on ok[j]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t m = join_lt4(v[j][0], t4) | (join_lt4(v[j][1], t4) << 4) | (join_lt4(v[j][2], t4) << 8) |
                           (join_lt4(v[j][3], t4) << 12);
        uint32_t word = ok[j] ? m << (16 * (lane & 1)) : 0u;
        word |= lane_neighbour(word);
        if (ok[j] && (lane & 1) == 0) A.bits[(g0 + 64u * j) >> 1] = word;
      }
    }
    row0 += A.step_rows;
    col0 += A.step_cols;
    if (col0 >= A.total) { col0 -= A.total; ++row0; }
  }
}

template <typename E, int KIND, bool ADD>
LCE_KERNEL void __launch_bounds__(256)
join_rows(const JoinArgs A, uint32_t segs, uint64_t total_tasks) {
  static_assert(!(ADD && KIND != kJoinF32), "only a float window has an addend");
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
      const E* src = (const E*)A.src[0];
      const float* add = A.addend[0];
      uint32_t p = A.pitch[0], w = A.count[0], s = 0;
#pragma unroll
      for (int k = 1; k < kJoinMaxWindows; ++k)
        if (col >= A.start[k]) { src = (const E*)A.src[k]; add = A.addend[k]; p = A.pitch[k]; w = A.count[k]; s = A.start[k]; }
      E v = src[row * (uint64_t)p + (uint64_t)(col - s)];
      if constexpr (ADD) {
        if (add) v = __builtin_bit_cast(E, __builtin_bit_cast(float, v) + add[row * (uint64_t)w + (uint64_t)(col - s)]);
      }
      if (A.out) ((E*)A.out)[row * (uint64_t)cols + col] = v;
      if constexpr (KIND == kJoinF32) neg = __builtin_bit_cast(float, v) < 0.0f;
      if constexpr (KIND == kJoinI8) neg = (int32_t)v < A.zero_point;
    }
    if (A.bits) {
      const unsigned long long m = wave_ballot(neg);
      const uint32_t w = seg * 2u + (uint32_t)lane;
      if (lane < 2 && w < A.wpr) A.bits[row * (uint64_t)A.wpr + w] = (uint32_t)(m >> (32 * lane));
    }
  }
}

}  // namespace lce
#endif  // __HIPCC__
