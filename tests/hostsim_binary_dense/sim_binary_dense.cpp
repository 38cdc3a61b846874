// Host simulation of lce_hip_binary_fully_connected's launch -- TEST ONLY (tests/test_binary_dense_host.py).  The real kernel body
// of csrc/lce_kernels_bfc.h runs on the CPU, the 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the tile enumeration, both load paths, the permuted K axis, the zero-code padding,
// the epilogue and the ballots are exercised without a GPU.  The FP4 matrix instruction is emulated lane-exactly from the layout
// the kernel takes it for (lane l: row / column l & 31, K half l >> 5; register r: column l & 31, row (r & 3) + 8 (r >> 2) +
// 4 (l >> 5)); whether the hardware agrees is what the GPU suite decides.
#include "sim_harness.h"
// (lce_kernels_head.h, included for head_clamp, names the float head's instruction; nothing here runs it)
inline lce_dev::f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float, float, lce_dev::f32x4, int, int, int) { __builtin_trap(); }
#include "lce_kernels_bfc.h"

// d: batch, inputs, outputs, activation.  `out`, `bits`: either may be null.  `cap`: the most blocks of the launch (the product
// caps its grid at 2048; a small cap makes the kernel stride).  Returns 1 when the launch took the 16-byte load path.
extern "C" int lce_hostsim_binary_fully_connected(const int32_t* d, const int32_t* in_bits, const int32_t* weight_bits,
                                                  const float* scale, const float* bias, float* out, int32_t* bits, int32_t cap) {
  lce::BfcArgs a;
  memset(&a, 0, sizeof a);
  a.in = (const uint32_t*)in_bits; a.weights = (const uint32_t*)weight_bits; a.scale = scale; a.bias = bias;
  a.out = out; a.bits = (uint32_t*)bits;
  lce::bfc_fill(a, d[0], d[1], d[2]);
  lce::float_activation_range(d[3], &a.lo, &a.hi);
  const bool vec = lce::bfc_vec_rule(a);
  const unsigned gx = lce::bfc_grid(a, (uint64_t)cap);
  if (vec) sim::launch(gx, 256, [&] { lce::binary_fully_connected<true>(a); }, /*mfma_xchg=*/true);
  else sim::launch(gx, 256, [&] { lce::binary_fully_connected<false>(a); }, /*mfma_xchg=*/true);
  return vec ? 1 : 0;
}
