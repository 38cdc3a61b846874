// Host simulation of lce_hip_mul_int8's launch -- TEST ONLY (tests/test_gate_i8_hostsim.py).  The real kernel bodies of
// csrc/lce_kernels_mul_i8.h run on the CPU, the lanes of a block as fibers in lock step (tests/hostsim/lce_device_intrinsics.h), so
// every lane's row and image, the gate's 16-byte load, the grid stride, the partial last iteration, the two-lane word, the half-word
// stores of an odd chunk count and the row path's ballots are exercised without a GPU.  One device-only piece is replaced: the quad
// permute v_mov_b32 quad_perm:[1,0,3,2] behind lane_neighbour is emulated as the exchange with lane ^ 1 it is.
#include <cstddef>

#include "sim_harness.h"
#include "lce_kernels_mul_i8.h"

namespace {
// `gx` blocks of `threads` threads, no LDS
template <typename F>
void launch(unsigned gx, unsigned threads, F kernel) { sim::launch(gx, threads, kernel); }

template <int MV, int V, bool PI>
void run_kind(const lce::MulI8Args& M, bool flat, unsigned gx, unsigned threads) {
  if (flat) {
    const uint64_t total_chunks = M.A.rows * (uint64_t)M.cpr;
    launch(gx, threads, [&] { lce::mul_i8_flat<MV, V, PI>(M, total_chunks); });
    return;
  }
  const uint32_t segs = (M.A.channels + 63u) / 64u;
  const uint64_t tasks = M.A.rows * (uint64_t)segs;
  launch(gx, threads, [&] { lce::mul_i8_rows<MV, V, PI>(M, segs, tasks); });
}
template <int MV, int V>
void run_add(const lce::MulI8Args& M, bool per_image, bool flat, unsigned gx, unsigned th) {
  if (per_image) run_kind<MV, V, true>(M, flat, gx, th);
  else run_kind<MV, V, false>(M, flat, gx, th);
}
// `add`: an lce_hip_add_int8_variant_id, or -1 without an ADD
template <int MV>
int run_mul(const lce::MulI8Args& M, int add, bool per_image, bool flat, unsigned gx, unsigned th) {
  switch (add) {
    case -1: run_add<MV, lce::kMulI8NoAdd>(M, per_image, flat, gx, th); return 0;
    case lce::kAddI8Literal: run_add<MV, lce::kAddI8Literal>(M, per_image, flat, gx, th); return 0;
    case lce::kAddI8Split: run_add<MV, lce::kAddI8Split>(M, per_image, flat, gx, th); return 0;
    case lce::kAddI8Shift: run_add<MV, lce::kAddI8Shift>(M, per_image, flat, gx, th); return 0;
  }
  return 1;
}
}  // namespace

// One launch as lce_hip_mul_int8_path describes it: `flat`, `blocks`, `threads` are the entry's own (the test lowers `blocks` to make
// the waves stride), and so are `mul_variant`, the MUL stage's arithmetic, `add_variant` (-1: no ADD), `product_first` and `add`,
// the 21 kernel parameters of that ADD variant in the kernel's input order (lce_hip_mul_int8_launch::add_args: AddI8Args from z1 to
// hi_rel).  `mul`: z1, z2, zo, multiplier, shift, act_min, act_max.  Returns 0, or 1 for a variant that does not exist.
extern "C" int lce_hostsim_gate_i8(const int32_t* mul, const int32_t* add, int32_t add_variant, int32_t product_first, int64_t rows,
                                   int32_t channels, int64_t rows_per_image, int32_t per_image, const int8_t* x, const int8_t* g,
                                   const int8_t* addend, int8_t* out, uint32_t* bits, int32_t flat, int32_t blocks, int32_t threads,
                                   int32_t mul_variant) {
  lce::MulI8Args M;
  memset(&M, 0, sizeof M);
  lce::AddI8Args& a = M.A;
  M.z1 = mul[0]; M.z2 = mul[1]; M.zo = mul[2]; M.m = mul[3];
  M.left = mul[4] > 0 ? mul[4] : 0; M.right = mul[4] > 0 ? 0 : -mul[4];
  M.lo = mul[5]; M.hi = mul[6];
  M.half = M.right >= 1 ? 1 << (M.right - 1) : 0;
  M.zo_last = M.zo;
  if ((add_variant >= 0) != (add != nullptr)) return 1;
  if (add) {
    static_assert(offsetof(lce::AddI8Args, hi_rel) - offsetof(lce::AddI8Args, z1) == 20 * sizeof(int32_t), "z1 .. hi_rel are 21 int32");
    memcpy(&a.z1, add, 21 * sizeof(int32_t));
    M.product_first = product_first ? 1u : 0u;
    M.zo_last = a.zo;
  }
  M.x = x; M.g = g; M.addend = addend; a.out = out; a.bits = bits;
  a.rows = (uint64_t)rows; a.channels = (uint32_t)channels; a.wpr = (uint32_t)((channels + 31) / 32);
  M.cpr = (uint32_t)channels / 16u;
  M.rows_per_image = rows_per_image ? (uint64_t)rows_per_image : (uint64_t)(rows ? rows : 1);
  const unsigned gx = (unsigned)blocks, th = (unsigned)threads;
  if (mul_variant == lce::kMulI8Fast) return run_mul<lce::kMulI8Fast>(M, add_variant, per_image != 0, flat != 0, gx, th);
  return run_mul<lce::kMulI8Literal>(M, add_variant, per_image != 0, flat != 0, gx, th);
}
