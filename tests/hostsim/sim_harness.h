// What every tests/hostsim_<family>/sim_<family>.cpp starts with -- TEST ONLY.  A simulation includes this file first, then defines
// the matrix instruction of its family (if any) and includes the family's kernel header, whose device part it thereby compiles
// for the CPU against the host replacement of the device intrinsics (lce_device_intrinsics.h: build/ comes first on the include
// path).  Here:
//   - the prelude: __HIPCC__, the empty __host__ / __device__ / __forceinline__, and the quad permute v_mov_b32
//     quad_perm:[1,0,3,2] behind lane_neighbour (lce_kernels_common.h), emulated as the exchange with lane ^ 1 it is;
//   - with SIM_HARNESS_POOL defined: lce_kernels_pool.h, its 16-byte write-through store (inline assembly) replaced by a plain
//     store;
//   - sim::launch, which runs a kernel body over a grid, the lanes of a block as fibers in lock step.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include <lce_device_intrinsics.h>      // through -I, as the kernel headers' copies in build/ find it: build/ comes first
#define __HIPCC__ 1
#define __host__
#define __device__
#define __forceinline__ inline

// dpp_ctrl 0xB1 = quad_perm:[1,0,3,2], all rows and banks, bound_ctrl: the value of lane ^ 1 (every lane of the wave calls it)
inline int __builtin_amdgcn_mov_dpp(int v, int ctrl, int row_mask, int bank_mask, bool) {
  if (ctrl != 0xB1 || row_mask != 0xF || bank_mask != 0xF) __builtin_trap();
  return (int)lce_dev::shfl_xor((uint32_t)v, 1);
}

#include "lce_kernels_common.h"          // stream_grid, float_activation_range: what the launchers and entries of every family use

#ifdef SIM_HARNESS_POOL
// the header's store keeps its assembly under another name (never called); the kernels get a plain 16-byte store
#define pool_store_through pool_store_through_device
#include "lce_kernels_pool.h"
#undef pool_store_through
namespace lce {
inline void pool_store_through(u32x4* p, u32x4 v) { memcpy(p, &v, 16); }
}  // namespace lce
#endif

namespace sim {
constexpr unsigned kLdsGuard = 64;
constexpr uint8_t kLdsMark = 0xA7;

// A grid of gx x gy blocks of `threads` threads (whole waves), one block after the other.  `mfma_xchg`: the waves get the
// exchange area the emulated matrix instructions pass their operands through.  `lds_bytes` >= 0: the blocks get that much LDS
// behind lds_base(), 16-byte aligned between guard bytes; false when a block wrote outside it.
template <typename F>
bool launch(unsigned gx, unsigned gy, unsigned threads, F kernel, bool mfma_xchg = false, int lds_bytes = -1) {
  const unsigned waves = threads / 64;
  for (unsigned by = 0; by < gy; ++by)
    for (unsigned bx = 0; bx < gx; ++bx) {
      std::vector<uint32_t> xchg(waves * 64), mx(mfma_xchg ? waves * 64 * 8 : 0);
      std::vector<uint8_t> lds(lds_bytes >= 0 ? lds_bytes + 2 * kLdsGuard + 16 : 0, kLdsMark);
      uint8_t* base = lds_bytes >= 0 ? lds.data() + kLdsGuard : nullptr;
      if (base) base += (16 - (uintptr_t)base % 16) % 16;
      lce_dev::FiberBarrier block_bar((int)threads);
      std::vector<std::unique_ptr<lce_dev::FiberBarrier>> wave_bar;
      for (unsigned w = 0; w < waves; ++w) wave_bar.emplace_back(new lce_dev::FiberBarrier(64));
      lce_dev::run_fibers((int)threads,
        [&](int t, lce_dev::ThreadCtx& c) {
          const int w = t >> 6;
          c.tid_x = t; c.bid_x = (int)bx; c.bid_y = (int)by; c.bdim_x = (int)threads; c.gdim_x = (int)gx;
          c.bar = wave_bar[w].get(); c.xchg = xchg.data() + w * 64; c.block_bar = &block_bar; c.lds = base;
          c.mfma_xchg = mfma_xchg ? mx.data() + w * 64 * 8 : nullptr;
        },
        [&](int) { kernel(); });
      if (base) {
        for (uint8_t* p = lds.data(); p < base; ++p) if (*p != kLdsMark) return false;
        for (uint8_t* p = base + lds_bytes; p < lds.data() + lds.size(); ++p) if (*p != kLdsMark) return false;
      }
    }
  return true;
}
template <typename F>
bool launch(unsigned gx, unsigned threads, F kernel, bool mfma_xchg = false, int lds_bytes = -1) {
  return launch(gx, 1, threads, kernel, mfma_xchg, lds_bytes);
}
}  // namespace sim
