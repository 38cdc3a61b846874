// Host simulation of lce_hip_join_windows' launch -- TEST ONLY (tests/test_join_hostsim.py).  The real kernel bodies of
// csrc/lce_kernels_join.h run on the CPU, the 256 lanes of a block as fibers in lock step (tests/hostsim/lce_device_intrinsics.h),
// so the window table, the chunk bookkeeping of the vector path, its grid stride, the partial last block, the addend, the
// shuffles and the row path's ballots are exercised without a GPU.  The path and the kernel arguments come from the very
// functions the entry point uses (join_fill, join_set_stride).
#include "sim_harness.h"
#include "lce_kernels_join.h"

namespace {
template <typename F>
void launch(unsigned gx, F kernel) { sim::launch(gx, 256, kernel); }
}  // namespace

// One launch.  `kind`: 0 float32, 1 int8.  Window k is (src[k], pitch[k], begin[k], count[k], addend[k] or null), in elements.
// `cap`: the most blocks of the launch (the product caps its grid at 2048; a small cap makes every wave stride).  Returns 1 when
// the launch took the 16-byte path.
extern "C" int lce_hostsim_join(int32_t kind, int32_t n, const void* const* src, const int32_t* pitch, const int32_t* begin,
                                const int32_t* count, const float* const* addend, int64_t rows, int32_t zero_point, void* out,
                                uint32_t* bits, int32_t cap) {
  lce::JoinWindow w[lce::kJoinMaxWindows];
  for (int k = 0; k < n; ++k) w[k] = lce::JoinWindow{src[k], addend[k], (uint32_t)pitch[k], (uint32_t)begin[k], (uint32_t)count[k]};
  lce::JoinArgs a;
  const bool vec = lce::join_fill(a, kind, w, n, (uint64_t)rows, zero_point, out, bits);
  const bool add = lce::join_has_addend(a);
  auto grid = [&](uint64_t wave_tasks) { return lce::stream_grid(wave_tasks, 4, (uint64_t)cap); };
  if (vec) {
    const unsigned g = grid((a.total_chunks + 255) / 256);
    lce::join_set_stride(a, g);
    const bool b = bits != nullptr;
    if (kind == lce::kJoinI8) {
      if (b) launch(g, [&] { lce::join_vec<lce::kJoinI8, true, false>(a); }); else launch(g, [&] { lce::join_vec<lce::kJoinI8, false, false>(a); });
    } else if (add) {
      if (b) launch(g, [&] { lce::join_vec<lce::kJoinF32, true, true>(a); }); else launch(g, [&] { lce::join_vec<lce::kJoinF32, false, true>(a); });
    } else {
      if (b) launch(g, [&] { lce::join_vec<lce::kJoinF32, true, false>(a); }); else launch(g, [&] { lce::join_vec<lce::kJoinF32, false, false>(a); });
    }
  } else {
    const uint32_t segs = (a.total + 63u) / 64u;
    const uint64_t tasks = a.rows * (uint64_t)segs;
    const unsigned g = grid(tasks);
    if (kind == lce::kJoinI8) launch(g, [&] { lce::join_rows<int8_t, lce::kJoinI8, false>(a, segs, tasks); });
    else if (add) launch(g, [&] { lce::join_rows<uint32_t, lce::kJoinF32, true>(a, segs, tasks); });
    else launch(g, [&] { lce::join_rows<uint32_t, lce::kJoinF32, false>(a, segs, tasks); });
  }
  return vec ? 1 : 0;
}
