// Host simulation of lce_hip_binary_fully_connected's launch -- TEST ONLY (tests/test_binary_dense_host.py).  The real kernel body
// of csrc/lce_kernels_bfc.h runs on the CPU, the 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the tile enumeration, both load paths, the permuted K axis, the zero-code padding,
// the epilogue and the ballots are exercised without a GPU.  The FP4 matrix instruction is emulated lane-exactly from the layout
// the kernel takes it for (lane l: row / column l & 31, K half l >> 5; register r: column l & 31, row (r & 3) + 8 (r >> 2) +
// 4 (l >> 5)); whether the hardware agrees is what the GPU suite decides.
#include <cfloat>
#include <cstring>
#include <vector>

#include "lce_device_intrinsics.h"      // the host replacement: build/ comes first on the include path
#define __HIPCC__ 1
// (lce_kernels_head.h, included for head_clamp, names the float head's instruction; nothing here runs it)
inline lce_dev::f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float, float, lce_dev::f32x4, int, int, int) { __builtin_trap(); }
#include "lce_kernels_bfc.h"

namespace {
template <typename F>
void launch(unsigned gx, F kernel) {
  for (unsigned bx = 0; bx < gx; ++bx) {
    std::vector<uint32_t> xchg(4 * 64), mx(4 * 64 * 8);
    lce_dev::FiberBarrier block_bar(256);
    lce_dev::FiberBarrier wave_bar[4] = {lce_dev::FiberBarrier(64), lce_dev::FiberBarrier(64), lce_dev::FiberBarrier(64),
                                         lce_dev::FiberBarrier(64)};
    lce_dev::run_fibers(256,
      [&](int t, lce_dev::ThreadCtx& c) {
        const int w = t >> 6;
        c.tid_x = t; c.bid_x = (int)bx; c.bid_y = 0; c.bdim_x = 256; c.gdim_x = (int)gx;
        c.bar = &wave_bar[w]; c.xchg = xchg.data() + w * 64; c.mfma_xchg = mx.data() + w * 64 * 8; c.block_bar = &block_bar;
      },
      [&](int) { kernel(); });
  }
}
}  // namespace

// d: batch, inputs, outputs, activation.  `out`, `bits`: either may be null.  `cap`: the most blocks of the launch (the product
// caps its grid at 2048; a small cap makes the kernel stride).  Returns 1 when the launch took the 16-byte load path.
extern "C" int lce_hostsim_binary_fully_connected(const int32_t* d, const int32_t* in_bits, const int32_t* weight_bits,
                                                  const float* scale, const float* bias, float* out, int32_t* bits, int32_t cap) {
  lce::BfcArgs a;
  memset(&a, 0, sizeof a);
  a.in = (const uint32_t*)in_bits; a.weights = (const uint32_t*)weight_bits; a.scale = scale; a.bias = bias;
  a.out = out; a.bits = (uint32_t*)bits;
  a.M = (uint32_t)d[0]; a.K = (uint32_t)d[1]; a.N = (uint32_t)d[2]; a.Kw = (a.K + 31) / 32;
  a.ntiles = (a.N + lce::kBfcTile - 1) / lce::kBfcTile;
  a.tiles = ((a.M + lce::kBfcTile - 1) / lce::kBfcTile) * a.ntiles;
  switch (d[3]) {
    case 1: a.lo = 0.0f; a.hi = FLT_MAX; break;
    case 2: a.lo = -1.0f; a.hi = 1.0f; break;
    case 3: a.lo = 0.0f; a.hi = 6.0f; break;
    default: a.lo = -FLT_MAX; a.hi = FLT_MAX;
  }
  const bool vec = a.Kw % 4 == 0 && (uintptr_t)in_bits % 16 == 0 && (uintptr_t)weight_bits % 16 == 0;   // the entry's rule
  const unsigned blocks = (a.tiles + 3) / 4, gx = blocks < (unsigned)cap ? blocks : (unsigned)cap;      // launch_binary_fully_connected's grid
  if (vec) launch(gx, [&] { lce::binary_fully_connected<true>(a); });
  else launch(gx, [&] { lce::binary_fully_connected<false>(a); });
  return vec ? 1 : 0;
}
