// Probe: the two choices of the depthwise kernel (lce_kernels_depthwise.h) at QuickNet's three transitions, batch 256, 3x3 / 2
// SAME: plain against non-temporal input loads (PoolArgs::stream_loads), and a lane's weights through the cache against the
// filter staged once per block in LDS.  The product's own kernels, launched each way on operand sets that rotate through more
// than twice the 256 MB Infinity Cache, interleaved over five rounds, device events.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I compute-engine_amd/csrc -o tools/probes/depthwise_loads tools/probes/depthwise_loads.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lce_tu_pool.hip"
#include "lce_tu_depthwise.hip"

#define CHECK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

struct Shape { int h, c; const char* name; };

int main() {
  const int batch = 256, rounds = 5, iters = 20, f = 3, s = 2;
  const Shape shapes[] = {{56, 64, "256x56x56x64"}, {28, 128, "256x28x28x128"}, {14, 256, "256x14x14x256"}};
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (const Shape& sh : shapes) {
    const int oh = (sh.h + s - 1) / s;
    const size_t in_bytes = (size_t)batch * sh.h * sh.h * sh.c * 4, out_bytes = (size_t)batch * oh * oh * sh.c * 4;
    const size_t flt_bytes = (size_t)f * f * sh.c * 4;
    const int sets = (int)std::max<size_t>(2, (2ull * (256u << 20)) / (in_bytes + out_bytes) + 2);
    std::vector<void*> in(sets), out(sets);
    std::vector<float> host(in_bytes / 4), flt(flt_bytes / 4);
    for (size_t i = 0; i < host.size(); ++i) host[i] = (float)(int)(((i * 2654435761u) >> 24) & 0xFF) - 127.0f;
    for (size_t i = 0; i < flt.size(); ++i) flt[i] = (float)(1 + (i * 40503u >> 7) % 13) / 16.0f;     // (asymmetric)
    void* flt_dev;
    CHECK(hipMalloc(&flt_dev, flt_bytes));
    CHECK(hipMemcpy(flt_dev, flt.data(), flt_bytes, hipMemcpyHostToDevice));
    for (int k = 0; k < sets; ++k) {
      CHECK(hipMalloc(&in[k], in_bytes));
      CHECK(hipMalloc(&out[k], out_bytes));
      CHECK(hipMemcpy(in[k], host.data(), in_bytes, hipMemcpyHostToDevice));
    }
    lce::DepthwiseArgs a;
    memset(&a, 0, sizeof a);
    lce::PoolArgs& p = a.P;
    a.filter = (const float*)flt_dev;
    a.channels_in = sh.c;
    a.div_multiplier = lce::make_fastdiv(1);
    p.H = p.W = sh.h; p.OH = p.OW = oh; p.fh = p.fw = f; p.sh = p.sw = s;
    p.ph = p.pw = std::max(0, (oh - 1) * s + f - sh.h) / 2;
    p.channels = sh.c; p.wpr = (sh.c + 31) / 32;
    p.per_pixel = (uint32_t)(sh.c / 4);
    p.total = (uint64_t)batch * oh * oh * p.per_pixel;
    p.lo = -FLT_MAX; p.hi = FLT_MAX;
    p.div_ow = lce::make_fastdiv(oh); p.div_oh = lce::make_fastdiv(oh);
    const unsigned grid = lce::pool_vec_grid(p.total);
    const uint64_t stride = (uint64_t)grid * 4ull * 64ull;
    p.step_pixels = (uint32_t)(stride / p.per_pixel); p.step_chunks = (uint32_t)(stride % p.per_pixel);
    p.div_per_pixel = lce::make_fastdiv(p.per_pixel);
    auto launch = [&](int variant) {      // 0: plain loads, weights through the cache; 1: non-temporal loads; 2: plain, weights in LDS
      p.stream_loads = variant == 1 ? 1u : 0u;
      if (variant == 2) lce::depthwise_vec<false, true><<<grid, 256, flt_bytes, 0>>>(a);
      else lce::depthwise_vec<false, false><<<grid, 256, 0, 0>>>(a);
    };
    auto timed = [&](int variant, float* us) -> int {
      for (int i = -3; i < iters; ++i) {
        if (i == 0) CHECK(hipEventRecord(e0, 0));
        p.in = in[(i + 3) % sets]; p.out = out[(i + 3) % sets];
        launch(variant);
      }
      CHECK(hipGetLastError());
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      *us = ms * 1e3f / iters;
      return 0;
    };
    std::vector<float> t[3];
    for (int r = 0; r < rounds; ++r)
      for (int v = 0; v < 3; ++v) {
        float us;
        if (timed(v, &us)) return 1;
        t[v].push_back(us);
      }
    // all three give the same bytes
    std::vector<uint8_t> o[3] = {std::vector<uint8_t>(out_bytes), std::vector<uint8_t>(out_bytes), std::vector<uint8_t>(out_bytes)};
    for (int v = 0; v < 3; ++v) {
      p.in = in[0]; p.out = out[v % sets];
      launch(v);
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(o[v].data(), out[v % sets], out_bytes, hipMemcpyDeviceToHost));
      std::sort(t[v].begin(), t[v].end());
    }
    const bool equal = memcmp(o[0].data(), o[1].data(), out_bytes) == 0 && memcmp(o[0].data(), o[2].data(), out_bytes) == 0;
    printf("loads   %-16s 3x3/2 SAME  plain + cached weights median %7.1f us (min %.1f, max %.1f)   non-temporal median %7.1f us (min %.1f, max %.1f)   "
           "plain + LDS weights median %7.1f us (min %.1f, max %.1f)   nt - plain = %+.1f us, lds - cached = %+.1f us; %d operand sets of %.0f MB; "
           "bytes equal: %s\n", sh.name, t[0][rounds / 2], t[0].front(), t[0].back(), t[1][rounds / 2], t[1].front(), t[1].back(), t[2][rounds / 2],
           t[2].front(), t[2].back(), t[1][rounds / 2] - t[0][rounds / 2], t[2][rounds / 2] - t[0][rounds / 2], sets,
           (in_bytes + out_bytes) / 1048576.0, equal ? "yes" : "NO");
    for (int k = 0; k < sets; ++k) { (void)hipFree(in[k]); (void)hipFree(out[k]); }
    (void)hipFree(flt_dev);
  }
  return 0;
}
