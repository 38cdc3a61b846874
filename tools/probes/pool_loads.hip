// Probe: plain against non-temporal window loads in the pooling kernels (lce_kernels_pool.h, PoolArgs::stream_loads), for
// windows that overlap (3x3 / 2) and windows that do not (2x2 / 2).  The product's own kernels, launched with the flag both
// ways on operand sets that rotate through more than twice the 256 MB Infinity Cache, interleaved A-B-A-B, device events.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I compute-engine_amd/csrc -o tools/probes/pool_loads tools/probes/pool_loads.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lce_tu_pool.hip"

#define CHECK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

struct Shape { int kind, h, c, op, f, s; const char* name; };

int main() {
  const int batch = 256, rounds = 5, iters = 20;
  const Shape shapes[] = {{lce::kPoolF32, 56, 64, lce::kPoolMax, 3, 2, "f32 256x56x56x64 MAX 3x3/2 (overlapping)"},
                          {lce::kPoolF32, 28, 192, lce::kPoolMax, 3, 2, "f32 256x28x28x192 MAX 3x3/2 (overlapping)"},
                          {lce::kPoolF32, 28, 256, lce::kPoolMax, 2, 2, "f32 256x28x28x256 MAX 2x2/2 (disjoint)"},
                          {lce::kPoolF32, 28, 256, lce::kPoolAverage, 2, 2, "f32 256x28x28x256 AVERAGE 2x2/2 (disjoint)"},
                          {lce::kPoolI8, 28, 256, lce::kPoolAverage, 2, 2, "i8 256x28x28x256 AVERAGE 2x2/2 (disjoint)"},
                          {lce::kPoolI8, 56, 256, lce::kPoolMax, 3, 2, "i8 256x56x56x256 MAX 3x3/2 (overlapping)"}};
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (const Shape& sh : shapes) {
    const size_t esz = sh.kind == lce::kPoolF32 ? 4 : 1;
    const int oh = (sh.h - sh.f) / sh.s + 1;
    const size_t in_bytes = (size_t)batch * sh.h * sh.h * sh.c * esz, out_bytes = (size_t)batch * oh * oh * sh.c * esz;
    const int sets = (int)std::max<size_t>(2, (2ull * (256u << 20)) / (in_bytes + out_bytes) + 2);
    std::vector<void*> in(sets), out(sets);
    std::vector<uint8_t> host(in_bytes);
    for (size_t i = 0; i < in_bytes; ++i) host[i] = (uint8_t)((i * 2654435761u) >> 24) & (esz == 4 ? 0x3F : 0xFF);   // (small finite floats)
    for (int k = 0; k < sets; ++k) {
      CHECK(hipMalloc(&in[k], in_bytes));
      CHECK(hipMalloc(&out[k], out_bytes));
      CHECK(hipMemcpy(in[k], host.data(), in_bytes, hipMemcpyHostToDevice));
    }
    lce::PoolArgs a;
    memset(&a, 0, sizeof a);
    a.H = a.W = sh.h; a.OH = a.OW = oh; a.fh = a.fw = sh.f; a.sh = a.sw = sh.s;
    a.channels = sh.c; a.wpr = (sh.c + 31) / 32;
    a.per_pixel = (uint32_t)(sh.c * esz / 16);
    a.total = (uint64_t)batch * oh * oh * a.per_pixel;
    a.lo = -FLT_MAX; a.hi = FLT_MAX; a.qlo = -128; a.qhi = 127;
    a.div_ow = lce::make_fastdiv(oh); a.div_oh = lce::make_fastdiv(oh);
    const uint64_t stride = (uint64_t)lce::pool_vec_grid(a.total) * 4ull * 64ull;
    a.step_pixels = (uint32_t)(stride / a.per_pixel); a.step_chunks = (uint32_t)(stride % a.per_pixel);
    a.div_per_pixel = lce::make_fastdiv(a.per_pixel);
    auto timed = [&](uint32_t nt, float* us) -> int {
      a.stream_loads = nt;
      for (int i = -3; i < iters; ++i) {
        if (i == 0) CHECK(hipEventRecord(e0, 0));
        a.in = in[(i + 3) % sets]; a.out = out[(i + 3) % sets];
        if (lce::launch_pool(a, sh.kind, sh.op, true, nullptr) != 0) { printf("launch failed\n"); return 1; }
      }
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      *us = ms * 1e3f / iters;
      return 0;
    };
    std::vector<float> plain, nt;
    for (int r = 0; r < rounds; ++r) {
      float t;
      if (timed(0, &t)) return 1;
      plain.push_back(t);
      if (timed(1, &t)) return 1;
      nt.push_back(t);
    }
    // both policies give the same bytes
    std::vector<uint8_t> o0(out_bytes), o1(out_bytes);
    a.in = in[0]; a.out = out[0]; a.stream_loads = 0;
    lce::launch_pool(a, sh.kind, sh.op, true, nullptr);
    a.out = out[1]; a.stream_loads = 1;
    lce::launch_pool(a, sh.kind, sh.op, true, nullptr);
    CHECK(hipMemcpy(o0.data(), out[0], out_bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(o1.data(), out[1], out_bytes, hipMemcpyDeviceToHost));
    std::sort(plain.begin(), plain.end());
    std::sort(nt.begin(), nt.end());
    printf("loads   %-44s plain median %7.1f us (min %.1f, max %.1f)   non-temporal median %7.1f us (min %.1f, max %.1f)   nt - plain = %+.1f us; "
           "%d operand sets of %.0f MB; bytes equal: %s\n", sh.name, plain[rounds / 2], plain.front(), plain.back(), nt[rounds / 2], nt.front(), nt.back(),
           nt[rounds / 2] - plain[rounds / 2], sets, (in_bytes + out_bytes) / 1048576.0, memcmp(o0.data(), o1.data(), out_bytes) == 0 ? "yes" : "NO");
    for (int k = 0; k < sets; ++k) { hipFree(in[k]); hipFree(out[k]); }
  }
  return 0;
}
