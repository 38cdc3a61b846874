// Host simulation of the int8 head's launches -- TEST ONLY (tests/test_head_i8_hostsim.py, tests/test_head_i8_host.py).  The real
// kernel bodies of csrc/lce_kernels_head_i8.h run on the CPU, 256 lanes of a block as fibers in lock step
// (tests/hostsim/lce_device_intrinsics.h), so the tile enumeration, both load paths, the K tail, the epilogue, the pixel split of
// the MEAN, the softmax's passes and the boundary kernels are exercised without a GPU.  What it cannot decide is the premise
// itself: v_mfma_i32_16x16x64_i8 is emulated here as the exact integer dot product under the maps the kernel assumes -- row of A
// and column of B from lane l & 15, the 16 bytes of lane l paired byte for byte with the 16 bytes of the B lane in the same
// group l >> 4; accumulator register i of lane l is row 4 (l >> 4) + i, column l & 15.  The GPU suite decides that.
#include "sim_harness.h"
typedef int32_t sim_i32x4 __attribute__((vector_size(16)));      // the kernel header's i32x4
// (lce_kernels_eltwise_i8.h and lce_kernels_head.h come along for the gemmlowp steps and the stated exp; their kernels are not run here)
inline lce_dev::f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float, float, lce_dev::f32x4, int, int, int) { __builtin_trap(); }
inline sim_i32x4 __builtin_amdgcn_mfma_i32_16x16x64_i8(sim_i32x4 a, sim_i32x4 b, sim_i32x4 c, int, int, int) {
  const int lane = g_ctx.tid_x & 63;
  int8_t* x = (int8_t*)g_ctx.mfma_xchg;   // per lane 32 bytes: [a: 16][b: 16]
  memcpy(x + lane * 32, &a, 16);
  memcpy(x + lane * 32 + 16, &b, 16);
  g_ctx.bar->arrive_and_wait();
  const int col = lane & 15;
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * (lane >> 4) + i;
    int32_t sum = 0;
    for (int g = 0; g < 4; ++g)
      for (int j = 0; j < 16; ++j) sum += (int32_t)x[(row + 16 * g) * 32 + j] * (int32_t)x[(col + 16 * g) * 32 + 16 + j];
    c[i] += sum;
  }
  g_ctx.bar->arrive_and_wait();
  return c;
}
#include "lce_kernels_head_i8.h"

namespace {
template <typename F>
void launch(unsigned gx, F kernel) { sim::launch(gx, 256, kernel, /*mfma_xchg=*/true); }
}  // namespace

// d: batch, inputs, outputs, output zero point, act_min, act_max.  `table`: [3][outputs] as lce_hip_fully_connected_i8_prepare
// writes it.  `cap`: the most blocks of the launch (the product caps its grid at 2048; a small cap makes the kernel stride).
// Returns 1 when the launch took the 16-byte load path.
extern "C" int lce_hostsim_fully_connected_i8(const int32_t* d, const int8_t* in, const int8_t* weights, const int32_t* table, int8_t* out,
                                              int32_t cap) {
  lce::FcI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in; a.filter = weights; a.table = table; a.out = out;
  lce::fc_i8_fill(a, d[0], d[1], d[2]);
  a.zo = d[3]; a.act_min = d[4]; a.act_max = d[5];
  const bool vec = lce::fc_i8_vec_rule(a);
  const unsigned gx = lce::fc_i8_grid(a, (uint64_t)cap);
  if (vec) launch(gx, [&] { lce::fully_connected_i8<true>(a); });
  else launch(gx, [&] { lce::fully_connected_i8<false>(a); });
  return vec ? 1 : 0;
}

// d: batch, pixels, channels, zi, zo, multiplier, exponent.
extern "C" void lce_hostsim_mean_i8(const int32_t* d, const int8_t* in, int8_t* out, int32_t cap) {
  lce::MeanI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in; a.out = out; a.batch = (uint64_t)d[0]; a.n = (uint32_t)d[1]; a.C = (uint32_t)d[2];
  a.segs = (a.C + lce::kMeanI8Channels - 1) / lce::kMeanI8Channels;
  a.zi = d[3]; a.zo = d[4]; a.mul = d[5]; a.left = d[6] > 0 ? d[6] : 0; a.right = d[6] > 0 ? 0 : -d[6];
  launch(lce::stream_grid(a.batch * a.segs, 4, (uint64_t)cap), [&] { lce::mean_i8<4>(a); });
}

extern "C" void lce_hostsim_softmax_i8(int64_t rows, int32_t cols, float input_scale, float beta, const int8_t* in, int8_t* out, int32_t cap) {
  lce::SoftmaxI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in; a.out = out; a.rows = (uint64_t)rows; a.cols = (uint32_t)cols;
  a.sb = input_scale * beta;
  launch(lce::stream_grid(a.rows, 4, (uint64_t)cap), [&] { lce::softmax_i8<4>(a); });
}

extern "C" void lce_hostsim_quant_i8(int32_t quantize, int64_t n, float scale, int32_t zp, const void* in, void* out, int32_t cap) {
  lce::QuantArgs a;
  memset(&a, 0, sizeof a);
  a.in = in; a.out = out; a.n = (uint64_t)n; a.scale = scale; a.zp = zp;
  const unsigned gx = lce::stream_grid(a.n, 256, (uint64_t)cap);       // one element per lane, as launch_quantize_f32_i8 launches it
  if (quantize) launch(gx, [&] { lce::quant_i8<true>(a); });
  else launch(gx, [&] { lce::quant_i8<false>(a); });
}

// The value functions of the epilogues, element by element (the host tests sweep them over 10^5 random arguments).
extern "C" void lce_hostsim_fc_i8_value(int64_t n, const int32_t* acc, const int32_t* cst, const int32_t* m, const int32_t* e, int32_t zo,
                                        int32_t lo, int32_t hi, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = lce::fc_i8_value(acc[i], cst[i], m[i], e[i], zo, lo, hi);
}
extern "C" void lce_hostsim_mean_i8_value(int64_t k, const int32_t* acc, int32_t m, int32_t e, int32_t n, int32_t zo, int32_t* out) {
  for (int64_t i = 0; i < k; ++i) out[i] = lce::mean_i8_value(acc[i], m, e > 0 ? e : 0, e > 0 ? 0 : -e, n, zo);
}
extern "C" void lce_hostsim_softmax_i8_exp(int64_t n, const int32_t* d, float sb, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = lce::softmax_i8_exp(d[i], sb);
}
extern "C" void lce_hostsim_softmax_i8_value(int64_t n, const float* e, const float* s, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = lce::softmax_i8_value(e[i], s[i]);
}
extern "C" void lce_hostsim_quantize_value(int64_t n, const float* x, float scale, int32_t zp, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = lce::quantize_i8_value(x[i], scale, zp);
}
extern "C" void lce_hostsim_dequantize_value(int64_t n, const int32_t* q, float scale, int32_t zp, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = lce::dequantize_i8_value(q[i], scale, zp);
}
