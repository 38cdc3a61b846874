// Host simulation of lce_hip_elementwise_i8's launch -- TEST ONLY (tests/test_elementwise_i8_hostsim.py).  The real kernel bodies of
// csrc/lce_kernels_eltwise_i8_chain.h run on the CPU, the lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the copy of the table into LDS with its row order, the chunk's place in its row kept
// by modular steps, the grid stride, the partial last iteration, the two-lane word and the row path's ballots are exercised without
// a GPU.  One device-only piece is replaced: the quad permute v_mov_b32 quad_perm:[1,0,3,2] behind lane_neighbour is emulated as
// the exchange with lane ^ 1 it is.
#include "sim_harness.h"
#include "lce_kernels_eltwise_i8_chain.h"

namespace {
// `gx` blocks of `threads` threads with `lds_bytes` of LDS between guard bytes; false when a block wrote outside its LDS.
template <typename F>
bool launch(unsigned gx, unsigned threads, unsigned lds_bytes, F kernel) { return sim::launch(gx, threads, kernel, false, (int)lds_bytes); }

template <int H, int P>
bool run_place(const lce::EwI8Args& E, bool flat, unsigned gx, unsigned threads, unsigned lds_bytes) {
  if (flat) {
    const uint64_t total_chunks = E.A.rows * (uint64_t)E.A.wpr * 2ull;
    return launch(gx, threads, lds_bytes, [&] { lce::ew_i8_flat<H, P>(E, total_chunks); });
  }
  const uint32_t segs = (E.A.channels + 63u) / 64u;
  const uint64_t tasks = E.A.rows * (uint64_t)segs;
  return launch(gx, threads, lds_bytes, [&] { lce::ew_i8_rows<H, P>(E, segs, tasks); });
}

template <int H>
bool run_head(const lce::EwI8Args& E, int path, bool flat, unsigned gx, unsigned threads, unsigned lds_bytes) {
  switch (path) {
    case lce::kEwI8Lds: return run_place<H, lce::kEwI8Lds>(E, flat, gx, threads, lds_bytes);
    case lce::kEwI8Global: return run_place<H, lce::kEwI8Global>(E, flat, gx, threads, lds_bytes);
    default: return run_place<H, lce::kEwI8OneRow>(E, flat, gx, threads, lds_bytes);
  }
}
}  // namespace

// One launch as lce_hip_elementwise_i8_path describes it: `path`, `flat`, `blocks`, `threads`, `lds_bytes` are the entry's own
// (the test lowers `blocks` to make the waves stride).  `head`: NULL, or the literal ADD's z1, m1, n1, z2, m2, n2, zo, mo, no, lo, hi
// (n = -shift) -- the head runs the literal variant here; the others are proven against it value by value by the product's host
// code.  Returns 0, or 1 when a block wrote outside its LDS.
extern "C" int lce_hostsim_eltwise_i8(const int32_t* head, int64_t rows, int32_t channels, const int8_t* in, const int8_t* addend,
                                      const uint8_t* table, int32_t zo_last, int8_t* out, uint32_t* bits, int32_t path, int32_t flat,
                                      int32_t blocks, int32_t threads, int32_t lds_bytes) {
  lce::EwI8Args E;
  memset(&E, 0, sizeof E);
  lce::AddI8Args& a = E.A;
  if (head) {
    a.z1 = head[0]; a.m1 = head[1]; a.n1 = head[2]; a.z2 = head[3]; a.m2 = head[4]; a.n2 = head[5];
    a.zo = head[6]; a.mo = head[7]; a.no = head[8]; a.lo = head[9]; a.hi = head[10];
  }
  a.in1 = in; a.in2 = addend; a.out = out; a.bits = bits;
  a.rows = (uint64_t)rows; a.channels = (uint32_t)channels; a.wpr = (uint32_t)((channels + 31) / 32);
  E.table = table; E.zo_last = zo_last; E.cpr = (uint32_t)channels / 16u;
  const bool ok = head ? run_head<lce::kAddI8Literal>(E, path, flat != 0, (unsigned)blocks, (unsigned)threads, (unsigned)lds_bytes)
                       : run_head<lce::kEwI8NoHead>(E, path, flat != 0, (unsigned)blocks, (unsigned)threads, (unsigned)lds_bytes);
  return ok ? 0 : 1;
}
