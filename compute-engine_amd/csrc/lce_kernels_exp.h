// The library's stated exp, E(a) of include/lce_hip.h (lce_hip_softmax_f32): ONE device function for every kernel whose bytes
// are stated on it -- the float and the int8 softmax (lce_kernels_head.h, lce_kernels_head_i8.h) and the LOGISTIC step of the
// elementwise chain (lce_kernels_eltwise.h).  Included inside the device half of those headers, behind
// "lce_device_intrinsics.h" (it includes nothing itself, so the host simulations' replacement of the intrinsics stays in force).
#pragma once

namespace lce {
using namespace lce_dev;

// exp(a) for a <= 0 as the header comment states it.  (No contraction anywhere in the files that call it: the library and the
// host simulations are built with -ffp-contract=off.)
LCE_DEVICE float head_exp(float a) {
  if (!(a >= -104.0f)) return 0.0f;
  a = a > 0.0f ? 0.0f : a;
  const float n = __builtin_rintf(a * 1.44269502f);
  float r = fma1(n, -0.693145751953125f, a);
  r = fma1(n, -1.42860676e-06f, r);
  float p = 1.98412701e-04f;          // 1/5040
  p = fma1(p, r, 1.38888892e-03f);    // 1/720
  p = fma1(p, r, 8.33333377e-03f);    // 1/120
  p = fma1(p, r, 4.16666679e-02f);    // 1/24
  p = fma1(p, r, 1.66666672e-01f);    // 1/6
  p = fma1(p, r, 0.5f);
  p = fma1(p, r, 1.0f);
  p = fma1(p, r, 1.0f);
  const int32_t ni = (int32_t)n;
  const bool low = ni < -125;
  const uint32_t bits = __builtin_bit_cast(uint32_t, p) + ((uint32_t)(ni + (low ? 64 : 0)) << 23);
  return __builtin_bit_cast(float, bits) * (low ? 5.42101086e-20f : 1.0f);               // 2^-64
}

}  // namespace lce
