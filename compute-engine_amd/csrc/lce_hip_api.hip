// C ABI (include/lce_hip.h) over the gfx950 kernels in lce_kernels.h.
// There is no CPU fallback in this file: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lce_hip.h"
#include "lce_kernels.h"          // the LceQuantize / LceDequantize / LceBMaxPool2d kernels are launched from here
#include "lce_kernel_types.h"    // the convolution kernels live in their own translation units (lce_tu_*.hip)
#include "lce_kernels_eltwise.h"  // (lce_tu_eltwise.hip, lce_tu_eltwise_ex.hip)
#include "lce_kernels_eltwise_i8.h"  // (lce_tu_eltwise_i8.hip)
#include "lce_kernels_eltwise_i8_chain.h"   // (lce_tu_eltwise_i8_chain.hip)
#include "lce_kernels_mul_i8.h"      // (lce_tu_mul_i8.hip)
#include "lce_kernels_join.h"        // (lce_tu_join.hip)
#include "lce_kernels_pool.h"        // (lce_tu_pool.hip)
#include "lce_kernels_conv1x1.h"     // (lce_tu_conv1x1.hip)
#include "lce_kernels_depthwise.h"   // (lce_tu_depthwise.hip)
#include "lce_kernels_conv2d.h"      // (lce_tu_conv2d.hip)
#include "lce_kernels_conv2d_i8.h"   // (lce_tu_conv2d_i8.hip)
#include "lce_kernels_head.h"        // (lce_tu_head.hip)
#include "lce_kernels_head_i8.h"     // (lce_tu_head_i8.hip)
#include "lce_kernels_depthwise_i8.h"   // (lce_tu_depthwise_i8.hip)
#include "lce_kernels_transition.h"     // (lce_tu_transition.hip)
#include "lce_kernels_bfc.h"         // (lce_tu_bfc.hip)
#ifdef LCE_UNITY
// single-translation-unit build (tools/build_exp.sh): the time-stamp tools read __device__ arrays that must exist once
#include "lce_tu_valu.hip"
#include "lce_tu_mfma_ws.hip"
#include "lce_tu_mfma_direct.hip"
#include "lce_tu_mfma_2d.hip"
#include "lce_tu_pointwise.hip"
#include "lce_tu_stream_f32.hip"
#include "lce_tu_stream_f32_clamp.hip"
#include "lce_tu_stream_i8.hip"
#include "lce_tu_stream_i8_floor.hip"
#include "lce_tu_stream_bitpacked.hip"
#include "lce_tu_wstream_f32.hip"
#include "lce_tu_wstream_i8.hip"
#include "lce_tu_wstream_i8_floor.hip"
#include "lce_tu_wstream_bitpacked.hip"
#include "lce_tu_eltwise.hip"
#include "lce_tu_eltwise_ex.hip"
#include "lce_tu_eltwise_i8.hip"
#include "lce_tu_eltwise_i8_chain.hip"
#include "lce_tu_mul_i8.hip"
#include "lce_tu_join.hip"
#include "lce_tu_pool.hip"
#include "lce_tu_conv1x1.hip"
#include "lce_tu_depthwise.hip"
#include "lce_tu_conv2d.hip"
#include "lce_tu_conv2d_i8.hip"
#include "lce_tu_head.hip"
#include "lce_tu_head_i8.hip"
#include "lce_tu_depthwise_i8.hip"
#include "lce_tu_transition.hip"
#include "lce_tu_bfc.hip"
#endif
#include "lce_plan.h"
#include "lce_prepare.h"

namespace {

thread_local std::string g_last_error;

lce_hip_status fail(lce_hip_status code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define LCE_HIP_TRY(expr)                                                                  \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? LCE_HIP_ERR_NO_DEVICE \
                                                                         : LCE_HIP_ERR_RUNTIME, \
                  "%s failed: %s", #expr, hipGetErrorString(e_));                          \
  } while (0)

// Asked once per process (the answer cannot change while it runs): the run / bitpack entry points are
// called per layer on 10-30 us kernels and must not pay a runtime query each time.
lce_hip_status require_device() {
  static const int count = [] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
      (void)hipGetLastError();
      n = 0;
    }
    return n;
  }();
  if (count <= 0)
    return fail(LCE_HIP_ERR_NO_DEVICE,
                "no usable HIP device (hipGetDeviceCount found %d); this library has no CPU fallback", count);
  return LCE_HIP_OK;
}

template <typename T>
struct DevBuf {
  T* ptr = nullptr;
  size_t count = 0;
  ~DevBuf() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  hipError_t upload(const std::vector<T>& v) {
    release();
    if (v.empty()) return hipSuccess;
    // +64 B of slack: the kernels' padded tables are read with wide scalar loads
    hipError_t e = hipMalloc((void**)&ptr, v.size() * sizeof(T) + 64);
    if (e != hipSuccess) return e;
    count = v.size();
    return hipMemcpy(ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  }
};

static_assert(LCE_HIP_ACT_NONE == 0 && LCE_HIP_ACT_RELU == 1 && LCE_HIP_ACT_RELU_N1_TO_1 == 2 && LCE_HIP_ACT_RELU6 == 3,
              "lce::float_activation_range (lce_kernels_common.h) states the activations by value");
using lce::float_activation_range;

// ---- The host checks that the windowed passes (pool, float 1x1 / depthwise / KxK convolution) share.  `who` is the entry's
// name: every message is the entry's own. ----
// The window of a pass as its descriptor states it; the 1x1 convolution, which has neither field, is a 1 x 1 VALID window.
struct Window {
  int32_t batch, in_h, in_w, fh, fw, sh, sw, padding, activation;
};

// Filter and stride positive, padding SAME or VALID, an activation float_activation_range knows: in this order.
lce_hip_status check_window_options(const char* who, const Window& w) {
  if (w.fh <= 0 || w.fw <= 0) return fail(LCE_HIP_ERR_INVALID, "%s: the filter must be positive, got %d x %d", who, (int)w.fh, (int)w.fw);
  if (w.sh <= 0 || w.sw <= 0) return fail(LCE_HIP_ERR_INVALID, "%s: the stride must be positive, got %d x %d", who, (int)w.sh, (int)w.sw);
  if (w.padding != LCE_HIP_PADDING_SAME && w.padding != LCE_HIP_PADDING_VALID)
    return fail(LCE_HIP_ERR_INVALID, "%s: padding must be SAME or VALID, got %d", who, (int)w.padding);
  if (w.activation < LCE_HIP_ACT_NONE || w.activation > LCE_HIP_ACT_RELU6)
    return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", who, (int)w.activation);
  return LCE_HIP_OK;
}

// (the kernels' window arithmetic, oy * stride - pad + filter, is 32-bit -- the 1x1 kernel's oy * stride 64-bit from 32-bit
// factors: with these bounds nothing wraps)
lce_hip_status check_extent_limit(const char* who, const Window& w) {
  if (std::max(w.in_h, w.in_w) > (1 << 30) || std::max(w.sh, w.sw) > (1 << 30))
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: image extents and strides above 2^30 are not supported", who);
  return LCE_HIP_OK;
}

// The end of every *_check: an output of oh x ow per image must have fewer than 2^31 pixels; then it is reported.
lce_hip_status report_output(const char* who, const Window& w, int32_t oh, int32_t ow, int32_t* out_height, int32_t* out_width) {
  if ((uint64_t)w.batch * (uint64_t)oh * (uint64_t)ow >= (1ull << 31))
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: the output must have fewer than 2^31 pixels", who);
  if (out_height) *out_height = oh;
  if (out_width) *out_width = ow;
  return LCE_HIP_OK;
}

// The output extent the padding rule gives (lce_hip_bmaxpool_output_shape), which must not be empty; then report_output.
lce_hip_status window_output(const char* who, const Window& w, int32_t* out_height, int32_t* out_width) {
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_bmaxpool_output_shape(w.in_h, w.in_w, w.fh, w.fw, w.sh, w.sw, w.padding, &oh, &ow)) return s;
  if (oh <= 0 || ow <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: empty output (a VALID filter of %d x %d on an image of %d x %d)", who, (int)w.fh, (int)w.fw,
                (int)w.in_h, (int)w.in_w);
  return report_output(who, w, oh, ow, out_height, out_width);
}

// The byte range of an operand; empty for a null pointer.
struct Span {
  uintptr_t lo, hi;
  Span(const void* p, uint64_t bytes) : lo((uintptr_t)p), hi((uintptr_t)p + (p ? bytes : 0)) {}
};
bool meet(uintptr_t a0, uintptr_t a1, uintptr_t c0, uintptr_t c1) { return a0 < c1 && c0 < a1; }

// The pointer checks of a run entry, in its order: descriptor, input, filter (`has_filter`), at least one output.
lce_hip_status check_pointers(const char* who, const void* desc, const void* in, bool has_filter, const void* filter, const void* out,
                              const void* bits) {
  if (!desc) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!in) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (has_filter && !filter) return fail(LCE_HIP_ERR_INVALID, "%s: null filter", who);
  if (!out && !bits) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
  return LCE_HIP_OK;
}

// The outputs must not meet anything the launch reads (another lane still reads what one would overwrite) or each other, and
// the pointers must be aligned: with `float_operands` every one to 4 bytes, otherwise (the pool, whose tensors may be int8)
// `bits` alone.  An operand the pass does not have is an empty Span.
lce_hip_status check_operand_ranges(const char* who, Span in, Span filter, Span bias, Span out, Span bits, bool float_operands) {
  auto reads = [&](Span r) { return meet(out.lo, out.hi, r.lo, r.hi) || meet(bits.lo, bits.hi, r.lo, r.hi); };
  if (reads(in)) return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the input", who);
  if (reads(filter)) return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the filter", who);
  if (reads(bias)) return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the bias", who);
  if (meet(out.lo, out.hi, bits.lo, bits.hi)) return fail(LCE_HIP_ERR_INVALID, "%s: the two outputs overlap", who);
  if (!float_operands && bits.lo % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: out_bits_dev must be 4-byte aligned", who);
  if (float_operands && (in.lo | filter.lo | bias.lo | out.lo | bits.lo) % 4 != 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: every pointer must be 4-byte aligned", who);
  return LCE_HIP_OK;
}

// The path an entry with a forced form takes: `vec`: the operands qualify for the 16-byte path; `path`: -1 (the entry's choice), 0 or 1.
lce_hip_status take_path(const char* who, int32_t path, bool* vec, const char* needs) {
  if (path != -1 && path != 0 && path != 1) return fail(LCE_HIP_ERR_INVALID, "%s: unknown path %d", who, (int)path);
  if (path == 1 && !*vec) return fail(LCE_HIP_ERR_INVALID, "%s: the 16-byte path needs %s", who, needs);
  if (path == 0) *vec = false;
  return LCE_HIP_OK;
}

// The window geometry of a 16-byte-chunk or row launch on PoolArgs (lce_kernels_pool.h), with the grid stride of the product's grid.
void window_fill(lce::PoolArgs& p, int32_t batch, int32_t H, int32_t W, int32_t fh, int32_t fw, int32_t sh, int32_t sw, int32_t oh, int32_t ow,
                 uint64_t C, uint64_t chunk_elems, bool vec, bool stream_loads_rule) {
  lce::pool_window_fill(p, batch, H, W, fh, fw, sh, sw, oh, ow, C, chunk_elems, vec, stream_loads_rule);
  if (vec) lce::pool_set_stride(p, lce::pool_vec_grid(p.total));
}

}  // namespace

struct lce_hip_bconv2d_plan {
  lce::HostPlan host;
  bool device_current = false;
  int64_t selected_for_pixels = -1;
  DevBuf<uint32_t> d_packed, d_filter;
  DevBuf<float> d_mul, d_bias, d_zpc;
  DevBuf<int32_t> d_thr, d_oobc;
  DevBuf<uint8_t> d_wq;
  DevBuf<float> d_thrq;
  DevBuf<uint32_t> d_sched;        // streaming kernel: its production schedule
  int device = -1;                 // the HIP device the plan's buffers live on (bound at the first upload)
  void* workspace = nullptr;       // FP4 expanded activations (matrix-core engine, workspace variant)
  void* lds_opt_in = nullptr;      // kernel already granted > 64 KiB of dynamic LDS
  size_t workspace_bytes = 0;
  // The workspace is ONE buffer per plan: a run on another stream must not start expanding into it while
  // the previous run's GEMM still reads it.  ws_done is recorded behind every workspace GEMM; a run on a
  // different stream waits for it first.
  hipEvent_t ws_done = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
  // run_host: device staging + a three-stream pipeline (H2D | compute | D2H) over batch slices
  void* stage_in = nullptr;
  void* stage_out = nullptr;
  size_t stage_in_bytes = 0, stage_out_bytes = 0;
  hipStream_t s_h2d = nullptr, s_run = nullptr, s_d2h = nullptr;
  std::vector<hipEvent_t> ev_in, ev_run;
  ~lce_hip_bconv2d_plan() {
    for (hipEvent_t e : ev_in) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_run) (void)hipEventDestroy(e);
    if (s_h2d) (void)hipStreamDestroy(s_h2d);
    if (s_run) (void)hipStreamDestroy(s_run);
    if (s_d2h) (void)hipStreamDestroy(s_d2h);
    if (ws_done) (void)hipEventDestroy(ws_done);
    if (stage_in) (void)hipFree(stage_in);
    if (stage_out) (void)hipFree(stage_out);
    if (workspace) (void)hipFree(workspace);
  }
};

namespace {

using lce::ConvArgs;
using lce::tiled_fn;
using lce::general_fn;
using lce::mfma_fn;

size_t out_elem_bytes(int dst) { return dst == LCE_HIP_I8 ? 1 : 4; }

// The unscaled FP4 MFMA's known-answer test (lce_mfma_selftest.h), once per device and kernel family (0: pointwise, 1: stream, 2: wstream)
lce_hip_status mfma_selftest_once(int dev, int family) {
  static std::mutex mu;
  static std::vector<int> state[3];       // -1 unknown, 0 passed, > 0 failed
  std::lock_guard<std::mutex> lock(mu);
  std::vector<int>& st = state[family];
  if (dev < 0) return LCE_HIP_OK;
  if ((size_t)dev >= st.size()) st.resize((size_t)dev + 1, -1);
  if (st[dev] < 0) {
    const int r = family == 2 ? lce::mfma_selftest_wstream() : family ? lce::mfma_selftest_stream() : lce::mfma_selftest_pointwise();
    if (r < 0) return fail(LCE_HIP_ERR_RUNTIME, "the FP4 matrix-core self-test could not run: %s", hipGetErrorString((hipError_t)(-r)));
    st[dev] = r;
  }
  if (st[dev] != 0)
    return fail(LCE_HIP_ERR_RUNTIME, "this build's unscaled FP4 MFMA (v_mfma_f32_32x32x64_f8f6f4 with FP4 operands at scale 1) does not "
                "compute 3 - 64 = -61 for C = 3, A = +1, B = -1 on device %d: the compiler did not select the unscaled encoding "
                "(lce_device_intrinsics.h, mfma_fp4_32x32x64_unscaled); refusing to run the %s kernels", dev, family == 2 ? "weight-streaming" : family ? "streaming" : "pointwise");
  return LCE_HIP_OK;
}

// compute units of HIP device `dev` (0 when unknown), cached per device
int device_compute_units(int dev) {
  static std::mutex mu;
  static std::vector<int> table;
  if (dev < 0) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if ((size_t)dev >= table.size()) table.resize((size_t)dev + 1, -1);
  if (table[dev] < 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      (void)hipGetLastError();
      n = 0;
    }
    table[dev] = n;
  }
  return table[dev];
}

lce_hip_status ensure_selected(lce_hip_bconv2d_plan* plan, int batch_chunk) {
  lce::HostPlan& h = plan->host;
  const int64_t pixels = (int64_t)batch_chunk * h.out_h * h.out_w;
  if (plan->selected_for_pixels == pixels && !h.kernel_name.empty() &&
      (!h.use_tiled || !h.packed.empty() || !h.have_weights) &&
      (!h.use_mfma || !h.wq.empty() || !h.have_weights))
    return LCE_HIP_OK;
  if (!h.cus_forced) {
    // the streaming kernel sizes its grid by the compute units of the device the plan runs on: the one it is bound to, or
    // the current one before its first run (asked once per device and process)
    int dev = plan->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; }
    const int cus = device_compute_units(dev);
    if (cus > 0) h.num_cus = cus;
  }
  const std::string err = lce::select_kernel(h, pixels);
  if (!err.empty()) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s", err.c_str());
  plan->selected_for_pixels = pixels;
  plan->device_current = false;
  return LCE_HIP_OK;
}

// A plan's weights, tables, workspace and staging live on ONE device: the one that is current when it first
// runs.  Running it with another device current would launch on that device with foreign pointers.
lce_hip_status check_device(lce_hip_bconv2d_plan* plan) {
  int cur = -1;
  LCE_HIP_TRY(hipGetDevice(&cur));
  if (plan->device < 0) plan->device = cur;
  if (plan->device != cur)
    return fail(LCE_HIP_ERR_INVALID,
                "bconv2d: this plan is bound to HIP device %d but device %d is current (a plan's buffers live on "
                "the device it first ran on; make that device current or create one plan per device)",
                plan->device, cur);
  return LCE_HIP_OK;
}

lce_hip_status ensure_uploaded(lce_hip_bconv2d_plan* plan) {
  if (plan->device_current) return LCE_HIP_OK;
  lce::HostPlan& h = plan->host;
  if (h.use_mfma) {
    LCE_HIP_TRY(plan->d_wq.upload(h.wq));
    LCE_HIP_TRY(plan->d_mul.upload(h.mul_q));
    LCE_HIP_TRY(plan->d_bias.upload(h.bias_q));
    LCE_HIP_TRY(plan->d_thrq.upload(h.thr_q));
    if (h.use_stream || h.use_wstream) LCE_HIP_TRY(plan->d_sched.upload(h.st_tabs));
    else plan->d_sched.release();
    plan->d_packed.release();
    plan->d_filter.release();
    plan->d_oobc.release();
  } else if (h.use_tiled) {
    LCE_HIP_TRY(plan->d_packed.upload(h.packed));
    LCE_HIP_TRY(plan->d_mul.upload(h.mul_p));
    LCE_HIP_TRY(plan->d_bias.upload(h.bias_p));
    LCE_HIP_TRY(plan->d_thr.upload(h.thr_p));
    LCE_HIP_TRY(plan->d_oobc.upload(h.oob_corr));
    plan->d_filter.release();
  } else {
    LCE_HIP_TRY(plan->d_filter.upload(h.filter));
    LCE_HIP_TRY(plan->d_mul.upload(h.mul));
    LCE_HIP_TRY(plan->d_bias.upload(h.bias));
    LCE_HIP_TRY(plan->d_thr.upload(h.thresholds));
    plan->d_packed.release();
    plan->d_oobc.release();
  }
  LCE_HIP_TRY(plan->d_zpc.upload(h.zero_pad_cache));
  plan->device_current = true;
  return LCE_HIP_OK;
}

}  // namespace

extern "C" {

int lce_hip_abi_version(void) { return LCE_HIP_ABI_VERSION; }
const char* lce_hip_last_error(void) { return g_last_error.c_str(); }
const char* lce_hip_build_flavor(void) { return LCE_BUILD_FLAVOR; }

int lce_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

lce_hip_status lce_hip_set_device(int device) {
  if (lce_hip_status s = require_device()) return s;
  LCE_HIP_TRY(hipSetDevice(device));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_malloc(void** dev_ptr, size_t bytes) {
  if (!dev_ptr) return fail(LCE_HIP_ERR_INVALID, "lce_hip_malloc: null out pointer");
  if (lce_hip_status s = require_device()) return s;
  LCE_HIP_TRY(hipMalloc(dev_ptr, bytes ? bytes : 1));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_free(void* dev_ptr) {
  if (dev_ptr) LCE_HIP_TRY(hipFree(dev_ptr));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  LCE_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  LCE_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  LCE_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_memset(void* dst, int value, size_t bytes, void* stream) {
  LCE_HIP_TRY(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_host_register(void* host_ptr, size_t bytes) {
  if (!host_ptr || !bytes) return fail(LCE_HIP_ERR_INVALID, "lce_hip_host_register: null or empty range");
  if (lce_hip_status s = require_device()) return s;
  LCE_HIP_TRY(hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_host_unregister(void* host_ptr) {
  if (host_ptr) LCE_HIP_TRY(hipHostUnregister(host_ptr));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_stream_create(void** stream) {
  if (!stream) return fail(LCE_HIP_ERR_INVALID, "lce_hip_stream_create: null out pointer");
  if (lce_hip_status s = require_device()) return s;
  hipStream_t st;
  LCE_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  *stream = (void*)st;
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_stream_destroy(void* stream) {
  if (stream) LCE_HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_stream_synchronize(void* stream) {
  LCE_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return LCE_HIP_OK;
}

// ---- HIP graphs behind the C ABI (include/lce_hip.h) ----
lce_hip_status lce_hip_graph_begin_capture(void* stream) {
  if (!stream) return fail(LCE_HIP_ERR_INVALID, "lce_hip_graph_begin_capture: the null stream cannot be captured (lce_hip_stream_create)");
  // thread-local mode: other threads of the host may go on calling the runtime while this one records
  LCE_HIP_TRY(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_graph_end_capture(void* stream, void** graph) {
  if (!stream || !graph) return fail(LCE_HIP_ERR_INVALID, "lce_hip_graph_end_capture: null argument");
  *graph = nullptr;
  hipGraph_t g = nullptr;
  LCE_HIP_TRY(hipStreamEndCapture((hipStream_t)stream, &g));
  if (!g) return fail(LCE_HIP_ERR_RUNTIME, "lce_hip_graph_end_capture: the capture was invalidated");
  hipGraphExec_t exec = nullptr;
  const hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "hipGraphInstantiate: %s", hipGetErrorString(e));
  *graph = (void*)exec;
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_graph_launch(void* graph, void* stream) {
  if (!graph) return fail(LCE_HIP_ERR_INVALID, "lce_hip_graph_launch: null graph");
  LCE_HIP_TRY(hipGraphLaunch((hipGraphExec_t)graph, (hipStream_t)stream));
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_graph_destroy(void* graph) {
  if (graph) LCE_HIP_TRY(hipGraphExecDestroy((hipGraphExec_t)graph));
  return LCE_HIP_OK;
}

int32_t lce_hip_bitpacked_size(int32_t n) { return (n + 31) / 32; }

// ------------------------------------------------------------------------------------
// LceQuantize / LceDequantize
// ------------------------------------------------------------------------------------
static lce_hip_status launch_bitpack_rows(lce_hip_dtype in_type, const void* in_dev, uint64_t rows,
                                          uint64_t cols, int32_t zero_point, uint32_t* out_dev,
                                          hipStream_t st) {
  const uint32_t wpr = (uint32_t)((cols + 31) / 32);
  const uint32_t segs = (uint32_t)((cols + 63) / 64);
  const uint64_t tasks = rows * segs;
  const unsigned grid = lce::stream_grid(tasks);
  const lce::FastDiv dv = lce::make_fastdiv(segs);
  if (in_type == LCE_HIP_F32)
    lce::bitpack_rows<float><<<grid, 256, 0, st>>>((const float*)in_dev, out_dev, (uint32_t)rows, (uint32_t)cols, wpr, 0, dv, segs, tasks);
  else if (in_type == LCE_HIP_I8)
    lce::bitpack_rows<int8_t><<<grid, 256, 0, st>>>((const int8_t*)in_dev, out_dev, (uint32_t)rows, (uint32_t)cols, wpr, zero_point, dv, segs, tasks);
  else
    lce::bitpack_rows<uint8_t><<<grid, 256, 0, st>>>((const uint8_t*)in_dev, out_dev, (uint32_t)rows, (uint32_t)cols, wpr, zero_point, dv, segs, tasks);
  LCE_HIP_TRY(hipGetLastError());
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bitpack(lce_hip_dtype in_type, const void* in_dev, size_t rows, size_t cols,
                               int32_t zero_point, int32_t* out_dev, void* stream) {
  if (in_type != LCE_HIP_F32 && in_type != LCE_HIP_I8 && in_type != LCE_HIP_BOOL)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_bitpack: input type must be float32, int8 or bool");
  if (in_type == LCE_HIP_F32 && zero_point != 0)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_bitpack: float input requires zero_point 0");
  if (rows == 0 || cols == 0) return LCE_HIP_OK;
  if (!in_dev || !out_dev) return fail(LCE_HIP_ERR_INVALID, "lce_hip_bitpack: null tensor");
  if (cols >= (1ull << 31) || rows >= (1ull << 32))
    return fail(LCE_HIP_ERR_UNSUPPORTED, "lce_hip_bitpack: tensor too large");
  if (lce_hip_status s = require_device()) return s;
  hipStream_t st = (hipStream_t)stream;
  if (in_type == LCE_HIP_BOOL) zero_point = 1;  // quantization.cc:86-108
  const size_t esz = in_type == LCE_HIP_F32 ? 4 : 1;
  const uint64_t wpr = (cols + 31) / 32;
  const uint64_t total_words = (uint64_t)rows * wpr;
  const bool flat = cols % 32 == 0 && ((uintptr_t)in_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0);
  if (!flat || total_words < 32)
    return launch_bitpack_rows(in_type, in_dev, rows, cols, zero_point, (uint32_t*)out_dev, st);
  // bitpack.h:294-298: no per-row padding -> the tensor is one flat array; 32 words per wave step
  const uint64_t blocks32 = total_words / 32;
  const unsigned grid = lce::stream_grid(blocks32);
  if (in_type == LCE_HIP_F32)
    lce::bitpack_f32_flat<><<<grid, 256, 0, st>>>((const float*)in_dev, (uint32_t*)out_dev, blocks32);
  else if (in_type == LCE_HIP_I8)
    lce::bitpack_b8_flat<false><<<grid, 256, 0, st>>>((const uint8_t*)in_dev, (uint32_t*)out_dev, blocks32, zero_point);
  else
    lce::bitpack_b8_flat<true><<<grid, 256, 0, st>>>((const uint8_t*)in_dev, (uint32_t*)out_dev, blocks32, zero_point);
  LCE_HIP_TRY(hipGetLastError());
  const uint64_t done_words = blocks32 * 32;
  if (done_words == total_words) return LCE_HIP_OK;
  // fewer than 32 words left: one ragged "row" of the flat array
  return launch_bitpack_rows(in_type, (const char*)in_dev + done_words * 32 * esz, 1,
                             (total_words - done_words) * 32, zero_point,
                             (uint32_t*)out_dev + done_words, st);
}

lce_hip_status lce_hip_unpack(lce_hip_dtype out_type, const int32_t* in_dev, size_t rows, size_t cols,
                              float scale, int32_t zero_point, void* out_dev, void* stream) {
  if (out_type != LCE_HIP_F32 && out_type != LCE_HIP_I8 && out_type != LCE_HIP_BOOL)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_unpack: output type must be float32, int8 or bool");
  if (rows == 0 || cols == 0) return LCE_HIP_OK;
  if (!in_dev || !out_dev) return fail(LCE_HIP_ERR_INVALID, "lce_hip_unpack: null tensor");
  if (cols >= (1ull << 31)) return fail(LCE_HIP_ERR_UNSUPPORTED, "lce_hip_unpack: cols too large");
  if (lce_hip_status s = require_device()) return s;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t wpr = (uint32_t)((cols + 31) / 32);
  const uint64_t total = (uint64_t)rows * cols;
  const unsigned grid = lce::stream_grid((total + 63) / 64);
  // whole words only and a 16-byte aligned destination: the flat, division-free kernel
  const bool flat = cols % 32 == 0 && ((uintptr_t)out_dev & 15) == 0;
  const uint64_t chunks_f32 = total / 4, chunks_b8 = total / 16;
  auto dv = (lce_dev::u32x4*)out_dev;
  if (out_type == LCE_HIP_F32) {
    if (flat) lce::unpack_flat<float><<<lce::stream_grid((chunks_f32 + 63) / 64), 256, 0, st>>>((const uint32_t*)in_dev, dv, chunks_f32, 1.0f, -1.0f);
    else lce::unpack_rows<float><<<grid, 256, 0, st>>>((const uint32_t*)in_dev, (float*)out_dev, total, (uint32_t)cols, wpr, 1.0f, -1.0f);
  } else if (out_type == LCE_HIP_I8) {
    // quantization.cc:131-138
    if (!(scale > 0.0f)) return fail(LCE_HIP_ERR_INVALID, "lce_hip_unpack: int8 output needs a positive scale");
    const int offset = (int)std::round(1.0f / scale);
    const int zero_bit = std::min(127, zero_point + offset);
    const int one_bit = std::max(-128, zero_point - offset);
    if (flat) lce::unpack_flat<int8_t><<<lce::stream_grid((chunks_b8 + 63) / 64), 256, 0, st>>>((const uint32_t*)in_dev, dv, chunks_b8, (int8_t)zero_bit, (int8_t)one_bit);
    else lce::unpack_rows<int8_t><<<grid, 256, 0, st>>>((const uint32_t*)in_dev, (int8_t*)out_dev, total, (uint32_t)cols, wpr, (int8_t)zero_bit, (int8_t)one_bit);
  } else {
    if (flat) lce::unpack_flat<uint8_t><<<lce::stream_grid((chunks_b8 + 63) / 64), 256, 0, st>>>((const uint32_t*)in_dev, dv, chunks_b8, (uint8_t)1, (uint8_t)0);
    else lce::unpack_rows<uint8_t><<<grid, 256, 0, st>>>((const uint32_t*)in_dev, (uint8_t*)out_dev, total, (uint32_t)cols, wpr, (uint8_t)1, (uint8_t)0);
  }
  LCE_HIP_TRY(hipGetLastError());
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// Float ADD / MUL chains (lce_kernels_eltwise.h)
// ------------------------------------------------------------------------------------
lce_hip_status lce_hip_elementwise(const float* in_dev, size_t rows, size_t channels, const lce_hip_ew_step* steps,
                                   int32_t num_steps, float* out_dev, int32_t* out_bits_dev, void* stream) {
  if (num_steps < 1 || num_steps > lce::kEwMaxSteps)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: num_steps must be 1..%d, got %d", lce::kEwMaxSteps, (int)num_steps);
  if (!steps) return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: null steps");
  if (channels >= (1ull << 31)) return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: channels must be below 2^31");
  lce::EwArgs a;
  memset(&a, 0, sizeof a);
  bool aligned = ((uintptr_t)in_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0) && ((uintptr_t)out_bits_dev % 16 == 0);
  for (int32_t s = 0; s < num_steps; ++s) {
    const lce_hip_ew_step& st = steps[s];
    lce::EwStep& k = a.steps[s];
    if (st.op != LCE_HIP_EW_ADD && st.op != LCE_HIP_EW_MUL)
      return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: step %d: unknown op %d", (int)s, (int)st.op);
    if (st.operand != LCE_HIP_EW_SCALAR && st.operand != LCE_HIP_EW_PER_CHANNEL && st.operand != LCE_HIP_EW_TENSOR)
      return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: step %d: unknown operand kind %d", (int)s, (int)st.operand);
    if (!float_activation_range(st.activation, &k.lo, &k.hi))
      return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: step %d: unknown activation %d", (int)s, (int)st.activation);
    k.op = st.op;
    k.operand = st.operand;
    k.values = st.operand == LCE_HIP_EW_SCALAR ? nullptr : st.values;
    k.scalar = st.scalar;
    if (k.values && (uintptr_t)k.values % 16 != 0) aligned = false;
  }
  if (rows == 0 || channels == 0) return LCE_HIP_OK;   // (an empty tensor may come with null pointers)
  for (int32_t s = 0; s < num_steps; ++s)
    if (steps[s].operand != LCE_HIP_EW_SCALAR && !steps[s].values)
      return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: step %d: null operand", (int)s);
  if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: both outputs are null");
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise: null input");
  if (lce_hip_status s = require_device()) return s;
  a.in = in_dev;
  a.out = out_dev;
  a.bits = (uint32_t*)out_bits_dev;
  a.rows = rows;
  a.channels = (uint32_t)channels;
  a.wpr = (uint32_t)((channels + 31) / 32);
  a.num_steps = num_steps;
  const int e = lce::launch_eltwise(a, channels % 32 == 0 && aligned, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "lce_hip_elementwise: launch failed: %s", hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// The extended chain: the steps of lce_hip_elementwise plus a per-image operand, CLAMP, PRELU and LOGISTIC (the EX = 1 instances
// of the same two kernels).  Everything is checked before any device call.
lce_hip_status lce_hip_elementwise_ex(const float* in_dev, size_t rows, size_t channels, size_t rows_per_image,
                                      const lce_hip_ew_step_ex* steps, int32_t num_steps, float* out_dev, int32_t* out_bits_dev,
                                      void* stream) {
  const char* who = "lce_hip_elementwise_ex";
  if (num_steps < 1 || num_steps > lce::kEwMaxSteps)
    return fail(LCE_HIP_ERR_INVALID, "%s: num_steps must be 1..%d, got %d", who, lce::kEwMaxSteps, (int)num_steps);
  if (!steps) return fail(LCE_HIP_ERR_INVALID, "%s: null steps", who);
  if (channels >= (1ull << 31)) return fail(LCE_HIP_ERR_INVALID, "%s: channels must be below 2^31", who);
  lce::EwArgsEx a;
  memset(&a, 0, sizeof a);
  bool aligned = ((uintptr_t)in_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0) && ((uintptr_t)out_bits_dev % 16 == 0);
  bool aligned4 = ((uintptr_t)in_dev % 4 == 0) && ((uintptr_t)out_dev % 4 == 0) && ((uintptr_t)out_bits_dev % 4 == 0);
  bool per_image = false;
  for (int32_t s = 0; s < num_steps; ++s) {
    const lce_hip_ew_step_ex& st = steps[s];
    lce::EwStep& k = a.steps[s];
    if (st.op < LCE_HIP_EW_ADD || st.op > LCE_HIP_EW_LOGISTIC) return fail(LCE_HIP_ERR_INVALID, "%s: step %d: unknown op %d", who, (int)s, (int)st.op);
    if (st.operand < LCE_HIP_EW_SCALAR || st.operand > LCE_HIP_EW_PER_IMAGE_CHANNEL)
      return fail(LCE_HIP_ERR_INVALID, "%s: step %d: unknown operand kind %d", who, (int)s, (int)st.operand);
    if (st.reserved[0] || st.reserved[1]) return fail(LCE_HIP_ERR_INVALID, "%s: step %d: reserved fields must be zero", who, (int)s);
    if (!float_activation_range(st.activation, &k.lo, &k.hi))
      return fail(LCE_HIP_ERR_INVALID, "%s: step %d: unknown activation %d", who, (int)s, (int)st.activation);
    const bool arithmetic = st.op == LCE_HIP_EW_ADD || st.op == LCE_HIP_EW_MUL;
    if (st.op == LCE_HIP_EW_PRELU && st.operand != LCE_HIP_EW_SCALAR && st.operand != LCE_HIP_EW_PER_CHANNEL)
      return fail(LCE_HIP_ERR_INVALID, "%s: step %d: PRELU's alpha is SCALAR or PER_CHANNEL, got operand kind %d", who, (int)s, (int)st.operand);
    if ((st.op == LCE_HIP_EW_PRELU || st.op == LCE_HIP_EW_LOGISTIC) && st.activation != LCE_HIP_ACT_NONE)
      return fail(LCE_HIP_ERR_INVALID, "%s: step %d: PRELU and LOGISTIC take no activation (a CLAMP step follows them)", who, (int)s);
    const bool reads = arithmetic || st.op == LCE_HIP_EW_PRELU;          // CLAMP and LOGISTIC have no operand: theirs is ignored
    k.op = st.op;
    k.operand = reads ? st.operand : (int32_t)LCE_HIP_EW_SCALAR;
    k.values = reads && st.operand != LCE_HIP_EW_SCALAR ? st.values : nullptr;
    k.scalar = st.scalar;
    if (k.operand == LCE_HIP_EW_PER_IMAGE_CHANNEL) per_image = true;
    if (k.values && (uintptr_t)k.values % 16 != 0) aligned = false;
    if (k.values && (uintptr_t)k.values % 4 != 0) aligned4 = false;
  }
  if (rows_per_image == 0 && per_image) return fail(LCE_HIP_ERR_INVALID, "%s: a PER_IMAGE_CHANNEL operand needs rows_per_image", who);
  if (rows_per_image != 0 && rows % rows_per_image != 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: rows_per_image %zu does not divide rows %zu", who, rows_per_image, rows);
  if (rows == 0 || channels == 0) return LCE_HIP_OK;   // (an empty tensor may come with null pointers)
  for (int32_t s = 0; s < num_steps; ++s)
    if (a.steps[s].operand != LCE_HIP_EW_SCALAR && !a.steps[s].values) return fail(LCE_HIP_ERR_INVALID, "%s: step %d: null operand", who, (int)s);
  if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!aligned4) return fail(LCE_HIP_ERR_INVALID, "%s: every pointer must be 4-byte aligned", who);
  if (lce_hip_status s = require_device()) return s;
  a.in = in_dev;
  a.out = out_dev;
  a.bits = (uint32_t*)out_bits_dev;
  a.rows = rows;
  a.channels = (uint32_t)channels;
  a.wpr = (uint32_t)((channels + 31) / 32);
  a.num_steps = num_steps;
  a.rows_per_image = rows_per_image ? rows_per_image : rows;            // (no per-image operand: one image)
  const int e = lce::launch_eltwise_ex(a, channels % 32 == 0 && aligned, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

int32_t lce_hip_elementwise_grid_cap(void) { return (int32_t)lce::kEwGridCap; }

// ------------------------------------------------------------------------------------
// int8 residual ADD (lce_kernels_eltwise_i8.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// QuantizeMultiplier (tensorflow/lite/kernels/internal/quantization_util.cc)
void quantize_multiplier(double d, int32_t* m, int32_t* e) {
  *m = 0;
  *e = 0;
  if (d == 0.0) return;
  int exp = 0;
  const double q = std::frexp(d, &exp);
  int64_t q_fixed = (int64_t)std::round(q * (double)(1ll << 31));
  if (q_fixed == (1ll << 31)) {
    q_fixed /= 2;
    ++exp;
  }
  if (exp < -31) {
    exp = 0;
    q_fixed = 0;
  }
  *m = (int32_t)q_fixed;
  *e = exp;
}

// What the host derives from one lce_hip_add_int8_desc: TFLite's nine parameters, the kernel arguments in canonical input
// order (pointers and sizes unset), and which variants are PROVEN for it.
struct PreparedAddI8 {
  lce_hip_add_int8_params params;
  lce::AddI8Args args;
  bool swapped = false;                         // the kernel's input 1 is the caller's input 2
  int32_t c_for[lce::kAddI8Variants] = {0, 0, 0};
  bool proven[lce::kAddI8Variants] = {true, false, false};
  int variant = lce::kAddI8Literal;             // the chooser's pick
};

// CalculateActivationRangeQuantized (kernel_util.cc) for an int8 tensor of (scale, zero_point):
// Q(f) = zero_point + (int32)round(f / scale), the division in float.  Shared by the int8 ADD and the int8 pools.
void quantized_activation_range(int32_t activation, float scale, int32_t zero_point, int32_t* act_min, int32_t* act_max) {
  auto Q = [&](float f) -> int64_t {
    double r = (double)std::round(f / scale);
    r = std::min(std::max(r, -2147483000.0), 2147483000.0);        // (the cast of a larger value is undefined)
    return (int64_t)zero_point + (int64_t)r;
  };
  int64_t lo = -128, hi = 127;
  if (activation == LCE_HIP_ACT_RELU) {
    lo = std::max<int64_t>(lo, Q(0.0f));
  } else if (activation == LCE_HIP_ACT_RELU6) {
    lo = std::max<int64_t>(lo, Q(0.0f));
    hi = std::min<int64_t>(hi, Q(6.0f));
  } else if (activation == LCE_HIP_ACT_RELU_N1_TO_1) {
    lo = std::max<int64_t>(lo, Q(-1.0f));
    hi = std::min<int64_t>(hi, Q(1.0f));
  }
  *act_min = (int32_t)lo;
  *act_max = (int32_t)hi;
}

lce_hip_status add_int8_params(const lce_hip_add_int8_desc* d, lce_hip_add_int8_params* p, const char* who) {
  if (!d || !p) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  const float scales[3] = {d->in1_scale, d->in2_scale, d->out_scale};
  const int32_t zps[3] = {d->in1_zero_point, d->in2_zero_point, d->out_zero_point};
  static const char* const names[3] = {"in1", "in2", "out"};
  for (int i = 0; i < 3; ++i) {
    if (!std::isfinite(scales[i]) || !(scales[i] > 0.0f))
      return fail(LCE_HIP_ERR_INVALID, "%s: %s_scale must be finite and positive, got %g", who, names[i], (double)scales[i]);
    if (zps[i] < -128 || zps[i] > 127)
      return fail(LCE_HIP_ERR_INVALID, "%s: %s_zero_point must be in [-128, 127], got %d", who, names[i], (int)zps[i]);
  }
  if (d->activation < LCE_HIP_ACT_NONE || d->activation > LCE_HIP_ACT_RELU6)
    return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", who, (int)d->activation);
  // Prepare of the builtin ADD (tensorflow/lite/kernels/add.cc), int8 branch
  const double s1 = (double)d->in1_scale, s2 = (double)d->in2_scale, so = (double)d->out_scale;
  const double twice_max = 2.0 * std::max(s1, s2);
  const double real[3] = {s1 / twice_max, s2 / twice_max, twice_max / ((double)(1 << 20) * so)};
  for (int i = 0; i < 3; ++i)
    if (!(real[i] > 0.0 && real[i] < 1.0))
      return fail(LCE_HIP_ERR_INVALID, "%s: the real multiplier of %s is %g, not in (0, 1)", who, names[i], real[i]);
  p->left_shift = 20;
  quantize_multiplier(real[0], &p->in1_multiplier, &p->in1_shift);
  quantize_multiplier(real[1], &p->in2_multiplier, &p->in2_shift);
  quantize_multiplier(real[2], &p->out_multiplier, &p->out_shift);
  quantized_activation_range(d->activation, d->out_scale, d->out_zero_point, &p->act_min, &p->act_max);
  return LCE_HIP_OK;
}

template <int V>
bool add_i8_variant_is_exact(const lce::AddI8Args& a, const std::vector<int8_t>& literal) {
  for (int x1 = -128; x1 < 128; ++x1)
    for (int x2 = -128; x2 < 128; ++x2)
      if ((int8_t)lce::add_i8_value<V>(a, x1, x2) != literal[(size_t)(x1 + 128) * 256 + (size_t)(x2 + 128)]) return false;
  return true;
}

// The kernel arguments of every variant whose preconditions hold, and the proof: the variant's own arithmetic over all
// 65 536 input pairs against the literal formula (the precedent: int8_one_instruction_forms, lce_plan.cpp).
void prove_add_int8(PreparedAddI8* P, const lce_hip_add_int8_desc& d) {
  const lce_hip_add_int8_params& p = P->params;
  struct In { int32_t z, m, n; } in[2] = {{d.in1_zero_point, p.in1_multiplier, -p.in1_shift},
                                          {d.in2_zero_point, p.in2_multiplier, -p.in2_shift}};
  auto is_shift = [](const In& i) { return i.m == (1 << 30) && i.n >= 0 && i.n <= 19; };   // sa = (x - z) << (19 - n), exact
  // canonical order: a shift-form input first; of two, the one with the smaller shift (so the split form applies to the other)
  P->swapped = is_shift(in[1]) && (!is_shift(in[0]) || in[0].n > in[1].n);
  if (P->swapped) std::swap(in[0], in[1]);
  lce::AddI8Args& a = P->args;
  memset(&a, 0, sizeof a);
  a.z1 = in[0].z; a.m1 = in[0].m; a.n1 = in[0].n;
  a.z2 = in[1].z; a.m2 = in[1].m; a.n2 = in[1].n;
  a.zo = d.out_zero_point; a.mo = p.out_multiplier; a.no = -p.out_shift;
  a.lo = p.act_min; a.hi = p.act_max;
  a.lo_rel = a.lo - a.zo; a.hi_rel = a.hi - a.zo;
  bool candidate[lce::kAddI8Variants] = {true, false, false};
  if (is_shift(in[0]) && a.no >= 1 && a.no <= 30 && a.mo > 0) {
    a.half_o = 1 << (a.no - 1);
    a.ka = 1 << (19 - in[0].n);
    P->c_for[lce::kAddI8Split] = -(in[0].z * a.ka);
    if (in[1].m > 0 && in[1].n >= 1 && in[1].n <= 30) {
      a.mh = in[1].m >> 11;
      a.ml = in[1].m & 2047;
      a.nb = in[1].n;
      a.half_b = 1 << (a.nb - 1);
      candidate[lce::kAddI8Split] = true;
    }
    if (is_shift(in[1])) {
      a.kb = 1 << (19 - in[1].n);
      P->c_for[lce::kAddI8Shift] = -(in[0].z * a.ka) - in[1].z * a.kb;
      candidate[lce::kAddI8Shift] = true;
    }
  }
  if (candidate[lce::kAddI8Split] || candidate[lce::kAddI8Shift]) {
    std::vector<int8_t> literal(65536);
    for (int x1 = -128; x1 < 128; ++x1)
      for (int x2 = -128; x2 < 128; ++x2)
        literal[(size_t)(x1 + 128) * 256 + (size_t)(x2 + 128)] = (int8_t)lce::add_i8_value<lce::kAddI8Literal>(a, x1, x2);
    if (candidate[lce::kAddI8Split]) {
      a.c = P->c_for[lce::kAddI8Split];
      P->proven[lce::kAddI8Split] = add_i8_variant_is_exact<lce::kAddI8Split>(a, literal);
    }
    if (candidate[lce::kAddI8Shift]) {
      a.c = P->c_for[lce::kAddI8Shift];
      P->proven[lce::kAddI8Shift] = add_i8_variant_is_exact<lce::kAddI8Shift>(a, literal);
    }
  }
  P->variant = P->proven[lce::kAddI8Shift] ? lce::kAddI8Shift : P->proven[lce::kAddI8Split] ? lce::kAddI8Split : lce::kAddI8Literal;
}

// One PreparedAddI8 per parameter set, kept by the host: a network has a handful, and the proof takes about a millisecond.
lce_hip_status prepared_add_int8(const lce_hip_add_int8_desc* d, PreparedAddI8* out, const char* who) {
  typedef std::array<int32_t, 7> Key;
  static std::mutex mu;
  static std::map<Key, PreparedAddI8> cache;
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  Key key;
  memcpy(&key[0], &d->in1_scale, 4);
  memcpy(&key[2], &d->in2_scale, 4);
  memcpy(&key[4], &d->out_scale, 4);
  key[1] = d->in1_zero_point; key[3] = d->in2_zero_point; key[5] = d->out_zero_point; key[6] = d->activation;
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) { *out = it->second; return LCE_HIP_OK; }
  }
  PreparedAddI8 P;
  if (lce_hip_status s = add_int8_params(d, &P.params, who)) return s;
  prove_add_int8(&P, *d);
  std::lock_guard<std::mutex> lock(mu);
  if (cache.size() >= 1024) cache.clear();
  cache[key] = P;
  *out = P;
  return LCE_HIP_OK;
}

lce_hip_status add_int8_run(const lce_hip_add_int8_desc* desc, int32_t forced, const int8_t* in1_dev, const int8_t* in2_dev,
                            size_t rows, size_t channels, int8_t* out_dev, int32_t* out_bits_dev, void* stream, const char* who) {
  PreparedAddI8 P;
  if (lce_hip_status s = prepared_add_int8(desc, &P, who)) return s;
  int variant = P.variant;
  if (forced >= 0) {
    if (forced >= lce::kAddI8Variants) return fail(LCE_HIP_ERR_INVALID, "%s: unknown variant %d", who, (int)forced);
    if (!P.proven[forced]) return fail(LCE_HIP_ERR_INVALID, "%s: variant %d is not proven for these parameters", who, (int)forced);
    variant = forced;
  }
  if (channels >= (1ull << 31)) return fail(LCE_HIP_ERR_INVALID, "%s: channels must be below 2^31", who);
  if (rows == 0 || channels == 0) return LCE_HIP_OK;   // (an empty tensor may come with null pointers)
  if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
  if (!in1_dev || !in2_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (lce_hip_status s = require_device()) return s;
  lce::AddI8Args a = P.args;
  a.c = P.c_for[variant];
  a.in1 = P.swapped ? in2_dev : in1_dev;
  a.in2 = P.swapped ? in1_dev : in2_dev;
  a.out = out_dev;
  a.bits = (uint32_t*)out_bits_dev;
  a.rows = rows;
  a.channels = (uint32_t)channels;
  a.wpr = (uint32_t)((channels + 31) / 32);
  const bool aligned = ((uintptr_t)in1_dev % 16 == 0) && ((uintptr_t)in2_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0) &&
                       ((uintptr_t)out_bits_dev % 4 == 0);
  const int e = lce::launch_add_i8(a, variant, channels % 32 == 0 && aligned, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_add_int8_prepare(const lce_hip_add_int8_desc* desc, lce_hip_add_int8_params* params) {
  return add_int8_params(desc, params, "lce_hip_add_int8_prepare");
}

lce_hip_status lce_hip_add_int8_variant(const lce_hip_add_int8_desc* desc, int32_t* variant) {
  if (!variant) return fail(LCE_HIP_ERR_INVALID, "lce_hip_add_int8_variant: null argument");
  PreparedAddI8 P;
  if (lce_hip_status s = prepared_add_int8(desc, &P, "lce_hip_add_int8_variant")) return s;
  *variant = P.variant;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_add_int8(const lce_hip_add_int8_desc* desc, const int8_t* in1_dev, const int8_t* in2_dev, size_t rows,
                                size_t channels, int8_t* out_dev, int32_t* out_bits_dev, void* stream) {
  return add_int8_run(desc, -1, in1_dev, in2_dev, rows, channels, out_dev, out_bits_dev, stream, "lce_hip_add_int8");
}

lce_hip_status lce_hip_add_int8_forced(const lce_hip_add_int8_desc* desc, int32_t variant, const int8_t* in1_dev,
                                       const int8_t* in2_dev, size_t rows, size_t channels, int8_t* out_dev,
                                       int32_t* out_bits_dev, void* stream) {
  if (variant < 0) return fail(LCE_HIP_ERR_INVALID, "lce_hip_add_int8_forced: unknown variant %d", (int)variant);
  return add_int8_run(desc, variant, in1_dev, in2_dev, rows, channels, out_dev, out_bits_dev, stream, "lce_hip_add_int8_forced");
}

// ------------------------------------------------------------------------------------
// int8 elementwise chain (lce_kernels_eltwise_i8_chain.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
const char* const kEwI8OpNames[4] = {"ADD", "PRELU", "CLAMP", "REQUANTIZE"};
// The entry's rule, from profiles/elementwise_i8/chains.txt (batch 256, a ReActNet tail): the LDS path from 128 channels up to what
// fits (it takes 0.90 / 0.60 / 0.77 of the global path's time at 128 / 256 / 512 channels), the global path below (at 64 channels the
// LDS path takes 1.09 of its time: few rows, so the lanes of a group crowd onto few banks) and beyond.
constexpr int32_t kEwI8LdsFromChannels = 128;

// What the host derives from one step: the function of (value, constant) it is.
struct EwI8StepFn {
  int32_t op = 0, zi = 0, zo = 0, za = 0, lo = -128, hi = 127;
  int32_t m1 = 0, e1 = 0, m2 = 0, e2 = 0;                // PRELU: positive / negative side; CLAMP, REQUANTIZE: (m1, e1)
  lce::AddI8Args add;                                    // ADD: the literal formula's parameters
};

int32_t ew_i8_mbqm(int32_t x, int32_t m, int32_t e) {    // MultiplyByQuantizedMultiplier
  const int32_t left = e > 0 ? e : 0, right = e > 0 ? 0 : -e;
  return lce::add_i8_rdivpot(lce::add_i8_srdhm((int32_t)((int64_t)x * ((int64_t)1 << left)), m), right);
}

int32_t ew_i8_eval(const EwI8StepFn& f, int32_t v, int32_t k) {
  int32_t raw;
  switch (f.op) {
    case LCE_HIP_EW_I8_ADD: return lce::add_i8_value<lce::kAddI8Literal>(f.add, v, k) + f.zo;
    case LCE_HIP_EW_I8_PRELU: {
      const int32_t d = v - f.zi;
      raw = (d >= 0 ? ew_i8_mbqm(d, f.m1, f.e1) : ew_i8_mbqm(d * (k - f.za), f.m2, f.e2)) + f.zo;
      break;
    }
    default: raw = ew_i8_mbqm(v - f.zi, f.m1, f.e1) + f.zo;
  }
  return std::min(f.hi, std::max(f.lo, raw));
}

lce_hip_status ew_i8_quant(const char* who, const char* what, float scale, int32_t zp) {
  if (!std::isfinite(scale) || !(scale > 0.0f))
    return fail(LCE_HIP_ERR_INVALID, "%s: %s_scale must be finite and positive, got %g", who, what, (double)scale);
  if (zp < -128 || zp > 127) return fail(LCE_HIP_ERR_INVALID, "%s: %s_zero_point must be in [-128, 127], got %d", who, what, (int)zp);
  return LCE_HIP_OK;
}

// (m, e) of a PRELU / CLAMP / REQUANTIZE real multiplier, and the check that x * 2^e stays in int32 for |x| <= max_abs
lce_hip_status ew_i8_multiplier(const char* who, double real, int64_t max_abs, int32_t* m, int32_t* e) {
  if (!std::isfinite(real) || !(real > 0.0)) return fail(LCE_HIP_ERR_INVALID, "%s: the real multiplier is %g, not finite and positive", who, real);
  quantize_multiplier(real, m, e);
  if (*e > 30 || (*e > 0 && (max_abs << *e) > (int64_t)INT32_MAX))
    return fail(LCE_HIP_ERR_INVALID, "%s: an intermediate could leave int32 (|x| up to %lld times 2^%d)", who, (long long)max_abs, (int)*e);
  return LCE_HIP_OK;
}

void ew_i8_add_args(const lce_hip_add_int8_desc& d, const lce_hip_add_int8_params& p, lce::AddI8Args* a) {
  memset(a, 0, sizeof *a);
  a->z1 = d.in1_zero_point; a->m1 = p.in1_multiplier; a->n1 = -p.in1_shift;
  a->z2 = d.in2_zero_point; a->m2 = p.in2_multiplier; a->n2 = -p.in2_shift;
  a->zo = d.out_zero_point; a->mo = p.out_multiplier; a->no = -p.out_shift;
  a->lo = p.act_min; a->hi = p.act_max;
}

struct EwI8Plan {
  int32_t table_rows = 1;                                // R
  int32_t zo_last = 0;
  EwI8StepFn fn[LCE_HIP_EW_I8_MAX_STEPS];
  lce_hip_add_int8_desc head;
};

// Every check of the descriptor; `who` is the entry's name.  The operand values are not read.
lce_hip_status ew_i8_plan(const lce_hip_elementwise_i8_desc* d, const char* who, EwI8Plan* P) {
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->channels < 0 || d->channels >= (1 << 22)) return fail(LCE_HIP_ERR_INVALID, "%s: channels must be in [0, 2^22), got %d", who, (int)d->channels);
  if (d->reserved[0] || d->reserved[1]) return fail(LCE_HIP_ERR_INVALID, "%s: non-zero reserved field", who);
  if (d->has_head != 0 && d->has_head != 1) return fail(LCE_HIP_ERR_INVALID, "%s: has_head must be 0 or 1, got %d", who, (int)d->has_head);
  if (d->num_steps < 1 || d->num_steps > LCE_HIP_EW_I8_MAX_STEPS)
    return fail(LCE_HIP_ERR_INVALID, "%s: num_steps must be 1..%d, got %d%s", who, LCE_HIP_EW_I8_MAX_STEPS, (int)d->num_steps,
                d->has_head && d->num_steps == 0 ? " (a head with no steps is lce_hip_add_int8's job)" : "");
  if (lce_hip_status s = ew_i8_quant(who, "in", d->in_scale, d->in_zero_point)) return s;
  char name[160];
  float si = d->in_scale;
  int32_t zi = d->in_zero_point;
  if (d->has_head) {
    snprintf(name, sizeof name, "%s: head", who);
    P->head = lce_hip_add_int8_desc{d->in_scale, d->in_zero_point, d->addend_scale, d->addend_zero_point, d->head_scale,
                                    d->head_zero_point, d->head_activation};
    lce_hip_add_int8_params p;
    if (lce_hip_status s = add_int8_params(&P->head, &p, name)) return s;
    si = d->head_scale;
    zi = d->head_zero_point;
  }
  P->table_rows = 1;
  for (int k = 0; k < d->num_steps; ++k) {
    const lce_hip_ew_i8_step& st = d->steps[k];
    EwI8StepFn& f = P->fn[k];
    f = EwI8StepFn();
    if (st.op < 0 || st.op > LCE_HIP_EW_I8_REQUANTIZE) return fail(LCE_HIP_ERR_INVALID, "%s: step %d: unknown op %d", who, k + 1, (int)st.op);
    snprintf(name, sizeof name, "%s: step %d (%s)", who, k + 1, kEwI8OpNames[st.op]);
    const bool has_operand = st.op == LCE_HIP_EW_I8_ADD || st.op == LCE_HIP_EW_I8_PRELU;
    if (st.reserved[0] || st.reserved[1]) return fail(LCE_HIP_ERR_INVALID, "%s: non-zero reserved field", name);
    if (st.operand != LCE_HIP_EW_SCALAR && !(has_operand && st.operand == LCE_HIP_EW_PER_CHANNEL))
      return fail(LCE_HIP_ERR_INVALID, "%s: operand kind %d (%s)", name, (int)st.operand,
                  has_operand ? "SCALAR or PER_CHANNEL" : "this op takes no operand: 0");
    if (st.activation < LCE_HIP_ACT_NONE || st.activation > LCE_HIP_ACT_RELU6) return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", name, (int)st.activation);
    if ((st.op == LCE_HIP_EW_I8_PRELU || st.op == LCE_HIP_EW_I8_REQUANTIZE) && st.activation != LCE_HIP_ACT_NONE)
      return fail(LCE_HIP_ERR_INVALID, "%s: the activation must be NONE, got %d", name, (int)st.activation);
    if (lce_hip_status s = ew_i8_quant(name, "out", st.out_scale, st.out_zero_point)) return s;
    if (has_operand) {
      if (lce_hip_status s = ew_i8_quant(name, "operand", st.operand_scale, st.operand_zero_point)) return s;
      if (st.operand == LCE_HIP_EW_PER_CHANNEL) P->table_rows = d->channels;
    }
    f.op = st.op; f.zi = zi; f.zo = st.out_zero_point; f.za = st.operand_zero_point;
    const float so = st.out_scale;
    if (st.op == LCE_HIP_EW_I8_ADD) {
      const lce_hip_add_int8_desc ad{si, zi, st.operand_scale, st.operand_zero_point, so, st.out_zero_point, st.activation};
      lce_hip_add_int8_params p;
      if (lce_hip_status s = add_int8_params(&ad, &p, name)) return s;
      ew_i8_add_args(ad, p, &f.add);
    } else if (st.op == LCE_HIP_EW_I8_PRELU) {
      const float r1 = si / so;
      volatile float sisa = si * st.operand_scale;         // float32, left to right
      const float r2 = sisa / so;
      if (lce_hip_status s = ew_i8_multiplier(name, (double)r1, 255, &f.m1, &f.e1)) return s;
      if (lce_hip_status s = ew_i8_multiplier(name, (double)r2, 255 * 255, &f.m2, &f.e2)) return s;
    } else if (st.op == LCE_HIP_EW_I8_CLAMP) {
      const float r = si / so;
      if (lce_hip_status s = ew_i8_multiplier(name, (double)r, 255, &f.m1, &f.e1)) return s;
      quantized_activation_range(st.activation, so, st.out_zero_point, &f.lo, &f.hi);
    } else {
      if (lce_hip_status s = ew_i8_multiplier(name, (double)si / (double)so, 255, &f.m1, &f.e1)) return s;
    }
    si = so;
    zi = st.out_zero_point;
  }
  P->zo_last = zi;
  return LCE_HIP_OK;
}

struct EwI8Launch {
  lce::EwI8Args args;
  int head, path;
  bool flat;
  unsigned blocks, threads, lds_bytes;
  int32_t lds_max_channels;
};

// The launch of one call: path, layout, grid.  `forced` < 0: the entry's rule.  Nothing here touches a device.
lce_hip_status ew_i8_launch(const lce_hip_elementwise_i8_desc* desc, int32_t forced, const int8_t* in_dev, const int8_t* addend_dev,
                            const uint8_t* table_dev, size_t rows, const int8_t* out_dev, const int32_t* out_bits_dev, const char* who,
                            bool need_pointers, const EwI8Plan& P, EwI8Launch* L) {
  const uint32_t channels = (uint32_t)desc->channels;
  lce::EwI8Args& E = L->args;
  memset(&E, 0, sizeof E);
  L->head = lce::kEwI8NoHead;
  const int8_t *in1 = in_dev, *in2 = nullptr;
  if (desc->has_head) {
    PreparedAddI8 H;
    if (lce_hip_status s = prepared_add_int8(&P.head, &H, who)) return s;
    E.A = H.args;
    E.A.c = H.c_for[H.variant];
    L->head = H.variant;
    in1 = H.swapped ? addend_dev : in_dev;
    in2 = H.swapped ? in_dev : addend_dev;
  }
  if (need_pointers) {
    if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
    if (!in_dev || !table_dev || (desc->has_head && !addend_dev)) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
    if (!desc->has_head && addend_dev) return fail(LCE_HIP_ERR_INVALID, "%s: an addend without a head", who);
  }
  if ((uintptr_t)table_dev % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: table_dev must be 4-byte aligned", who);
  E.A.in1 = in1; E.A.in2 = in2;
  E.A.out = const_cast<int8_t*>(out_dev);
  E.A.bits = (uint32_t*)const_cast<int32_t*>(out_bits_dev);
  E.A.rows = rows;
  E.A.channels = channels;
  E.A.wpr = (channels + 31u) / 32u;
  E.table = table_dev;
  E.zo_last = P.zo_last;
  E.cpr = channels / 16u;
  const bool aligned = ((uintptr_t)in_dev % 16 == 0) && ((uintptr_t)addend_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0) &&
                       ((uintptr_t)out_bits_dev % 4 == 0);
  L->flat = channels % 32u == 0 && aligned;
  const uint32_t lds_rows = lce::kEwI8LdsLimit / lce::kEwI8LdsPitch;
  L->lds_max_channels = (int32_t)(L->flat ? lds_rows / 32u * 32u : lds_rows);
  const bool one_row = P.table_rows == 1;
  int path = one_row ? lce::kEwI8OneRow : (int32_t)channels >= kEwI8LdsFromChannels && (int32_t)channels <= L->lds_max_channels ? lce::kEwI8Lds : lce::kEwI8Global;
  if (forced >= 0) {
    if (forced >= lce::kEwI8Paths) return fail(LCE_HIP_ERR_INVALID, "%s: unknown path %d", who, (int)forced);
    if (forced == lce::kEwI8OneRow ? !one_row : (uint32_t)P.table_rows != channels)
      return fail(LCE_HIP_ERR_INVALID, "%s: path %d cannot run a table of %d rows on %u channels (ONE_ROW takes one row, LDS and GLOBAL one per channel)",
                  who, (int)forced, (int)P.table_rows, channels);
    if (forced == lce::kEwI8Lds && (int32_t)channels > L->lds_max_channels)
      return fail(LCE_HIP_ERR_INVALID, "%s: the LDS path takes at most %d channels on this layout, got %u", who, (int)L->lds_max_channels, channels);
    path = forced;
  }
  L->path = path;
  L->lds_bytes = path == lce::kEwI8Lds ? channels * lce::kEwI8LdsPitch : path == lce::kEwI8OneRow ? 256u : 0u;
  L->threads = L->lds_bytes > lce::kEwI8WideBlockAbove ? 1024u : 256u;
  // memory-bound streams: at most ~8 blocks of 4 waves per CU (as lce_tu_eltwise_i8.hip), fewer where the tables fill the LDS
  const uint64_t wave_tasks = L->flat ? (rows * (uint64_t)E.A.wpr * 2ull + 255) / 256 : rows * (uint64_t)((channels + 63u) / 64u);
  const uint64_t waves = L->threads / 64u;
  uint64_t per_cu = 32u / waves;
  if (L->lds_bytes) per_cu = std::max<uint64_t>(1, std::min<uint64_t>(per_cu, lce::kEwI8LdsLimit / L->lds_bytes));
  const uint64_t blocks = (wave_tasks + waves - 1) / waves, cap = 256ull * per_cu;
  L->blocks = (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
  return LCE_HIP_OK;
}

lce_hip_status ew_i8_run(const lce_hip_elementwise_i8_desc* desc, int32_t forced, const int8_t* in_dev, const int8_t* addend_dev,
                         const uint8_t* table_dev, size_t rows, int8_t* out_dev, int32_t* out_bits_dev, void* stream, const char* who) {
  EwI8Plan P;
  if (lce_hip_status s = ew_i8_plan(desc, who, &P)) return s;
  if (rows == 0 || desc->channels == 0) return LCE_HIP_OK;   // (an empty tensor may come with null pointers)
  EwI8Launch L;
  if (lce_hip_status s = ew_i8_launch(desc, forced, in_dev, addend_dev, table_dev, rows, out_dev, out_bits_dev, who, true, P, &L)) return s;
  if (lce_hip_status s = require_device()) return s;
  const int e = lce::launch_ew_i8(L.args, L.head, L.path, L.flat, L.blocks, L.threads, L.lds_bytes, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_elementwise_i8_check(const lce_hip_elementwise_i8_desc* desc) {
  EwI8Plan P;
  return ew_i8_plan(desc, "lce_hip_elementwise_i8_check", &P);
}

lce_hip_status lce_hip_elementwise_i8_table_size(const lce_hip_elementwise_i8_desc* desc, size_t* bytes) {
  if (!bytes) return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise_i8_table_size: null argument");
  EwI8Plan P;
  if (lce_hip_status s = ew_i8_plan(desc, "lce_hip_elementwise_i8_table_size", &P)) return s;
  *bytes = (size_t)P.table_rows * 256u;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_elementwise_i8_prepare(const lce_hip_elementwise_i8_desc* desc, uint8_t* table_host) {
  const char* who = "lce_hip_elementwise_i8_prepare";
  EwI8Plan P;
  if (lce_hip_status s = ew_i8_plan(desc, who, &P)) return s;
  if (!table_host) return fail(LCE_HIP_ERR_INVALID, "%s: null table", who);
  for (int k = 0; k < desc->num_steps; ++k)
    if ((desc->steps[k].op == LCE_HIP_EW_I8_ADD || desc->steps[k].op == LCE_HIP_EW_I8_PRELU) && !desc->steps[k].values)
      return fail(LCE_HIP_ERR_INVALID, "%s: step %d (%s): null values", who, k + 1, kEwI8OpNames[desc->steps[k].op]);
  // a step with a SCALAR operand (or none) is the same function in every channel: evaluated once
  uint8_t shared[LCE_HIP_EW_I8_MAX_STEPS][256];
  auto eval_step = [&](int k, int32_t operand, uint8_t* f) {
    for (int v = -128; v < 128; ++v) f[v + 128] = (uint8_t)(int8_t)ew_i8_eval(P.fn[k], v, operand);
  };
  for (int k = 0; k < desc->num_steps; ++k)
    if (desc->steps[k].operand != LCE_HIP_EW_PER_CHANNEL) eval_step(k, desc->steps[k].values ? (int32_t)desc->steps[k].values[0] : 0, shared[k]);
  for (int32_t r = 0; r < P.table_rows; ++r) {
    uint8_t* row = table_host + (size_t)r * 256u;
    for (int i = 0; i < 256; ++i) row[i] = (uint8_t)(int8_t)(i - 128);
    for (int k = 0; k < desc->num_steps; ++k) {
      uint8_t own[256];
      const uint8_t* f = shared[k];
      if (desc->steps[k].operand == LCE_HIP_EW_PER_CHANNEL) {
        eval_step(k, (int32_t)desc->steps[k].values[r], own);
        f = own;
      }
      for (int i = 0; i < 256; ++i) row[i] = f[(uint8_t)(row[i] ^ 0x80u)];
    }
  }
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_elementwise_i8(const lce_hip_elementwise_i8_desc* desc, const int8_t* in_dev, const int8_t* addend_dev,
                                      const uint8_t* table_dev, size_t rows, int8_t* out_dev, int32_t* out_bits_dev, void* stream) {
  return ew_i8_run(desc, -1, in_dev, addend_dev, table_dev, rows, out_dev, out_bits_dev, stream, "lce_hip_elementwise_i8");
}

lce_hip_status lce_hip_elementwise_i8_forced(const lce_hip_elementwise_i8_desc* desc, int32_t path, const int8_t* in_dev,
                                             const int8_t* addend_dev, const uint8_t* table_dev, size_t rows, int8_t* out_dev,
                                             int32_t* out_bits_dev, void* stream) {
  if (path < 0) return fail(LCE_HIP_ERR_INVALID, "lce_hip_elementwise_i8_forced: unknown path %d", (int)path);
  return ew_i8_run(desc, path, in_dev, addend_dev, table_dev, rows, out_dev, out_bits_dev, stream, "lce_hip_elementwise_i8_forced");
}

lce_hip_status lce_hip_elementwise_i8_path(const lce_hip_elementwise_i8_desc* desc, size_t rows, const int8_t* in_dev,
                                           const int8_t* addend_dev, const uint8_t* table_dev, const int8_t* out_dev,
                                           const int32_t* out_bits_dev, int32_t forced_path, lce_hip_elementwise_i8_launch* launch) {
  const char* who = "lce_hip_elementwise_i8_path";
  if (!launch) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  EwI8Plan P;
  if (lce_hip_status s = ew_i8_plan(desc, who, &P)) return s;
  EwI8Launch L;
  if (lce_hip_status s = ew_i8_launch(desc, forced_path, in_dev, addend_dev, table_dev, rows, out_dev, out_bits_dev, who, false, P, &L)) return s;
  launch->path = L.path;
  launch->flat = L.flat ? 1 : 0;
  launch->lds_max_channels = L.lds_max_channels;
  launch->blocks = (int32_t)L.blocks;
  launch->waves_per_block = (int32_t)(L.threads / 64u);
  launch->lds_bytes = (int32_t)L.lds_bytes;
  launch->head_variant = desc->has_head ? L.head : -1;
  launch->table_rows = P.table_rows;
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// int8 squeeze-and-excite gate: MUL with its residual ADD (lce_kernels_mul_i8.h), LOGISTIC as a table of the chain's ONE_ROW path
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
struct MulI8Plan {
  lce_hip_mul_int8_params params;
  lce_hip_add_int8_desc add;
};

// Every check of the descriptor and the parameters it gives; `who` is the entry's name.
lce_hip_status mul_i8_plan(const lce_hip_mul_int8_desc* d, const char* who, MulI8Plan* P) {
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  memset(P, 0, sizeof *P);
  if (lce_hip_status s = ew_i8_quant(who, "in1", d->in1_scale, d->in1_zero_point)) return s;
  if (lce_hip_status s = ew_i8_quant(who, "in2", d->in2_scale, d->in2_zero_point)) return s;
  if (lce_hip_status s = ew_i8_quant(who, "out", d->out_scale, d->out_zero_point)) return s;
  if (d->activation < LCE_HIP_ACT_NONE || d->activation > LCE_HIP_ACT_RELU6)
    return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", who, (int)d->activation);
  if (d->operand != LCE_HIP_EW_TENSOR && d->operand != LCE_HIP_EW_PER_IMAGE_CHANNEL)
    return fail(LCE_HIP_ERR_INVALID, "%s: operand kind %d (TENSOR or PER_IMAGE_CHANNEL)", who, (int)d->operand);
  if (d->has_add != 0 && d->has_add != 1) return fail(LCE_HIP_ERR_INVALID, "%s: has_add must be 0 or 1, got %d", who, (int)d->has_add);
  if (d->reserved[0] || d->reserved[1]) return fail(LCE_HIP_ERR_INVALID, "%s: non-zero reserved field", who);
  volatile float s12 = d->in1_scale * d->in2_scale;        // float32, left to right
  const float real = s12 / d->out_scale;
  if (lce_hip_status s = ew_i8_multiplier(who, (double)real, 255 * 255, &P->params.multiplier, &P->params.shift)) return s;
  quantized_activation_range(d->activation, d->out_scale, d->out_zero_point, &P->params.act_min, &P->params.act_max);
  if (d->has_add) {
    char name[160];
    snprintf(name, sizeof name, "%s: add", who);
    P->add = lce_hip_add_int8_desc{d->out_scale, d->out_zero_point, d->addend_scale, d->addend_zero_point, d->add_scale,
                                   d->add_zero_point, d->add_activation};
    if (lce_hip_status s = add_int8_params(&P->add, &P->params.add, name)) return s;
  }
  return LCE_HIP_OK;
}

// Whether the fast MUL variant gives the literal one's byte for EVERY product (x1 - z1)(x2 - z2), all 130 051 of them, under the
// MUL parameters of `M` (the precedent: prove_add_int8).  Kept per parameter set: a model launches the same few over and over.
bool mul_i8_fast_is_proven(const lce::MulI8Args& M) {
  if (M.left != 0 || M.right < 1 || M.right > 30 || M.m <= 0) return false;
  typedef std::array<int32_t, 5> Key;
  static std::mutex mu;
  static std::map<Key, bool> cache;
  const Key key{M.m, M.right, M.zo, M.lo, M.hi};
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  bool exact = true;
  for (int32_t p = -255 * 255; p <= 255 * 255 && exact; ++p)
    exact = lce::mul_i8_requant<lce::kMulI8Fast>(M, p) == lce::mul_i8_requant<lce::kMulI8Literal>(M, p);
  std::lock_guard<std::mutex> lock(mu);
  if (cache.size() >= 1024) cache.clear();
  cache[key] = exact;
  return exact;
}

struct MulI8Launch {
  lce::MulI8Args args;
  int mul, add;
  bool per_image, flat;
  unsigned blocks;
};

// The launch of one call: layout, ADD variant, grid.  Nothing here touches a device.
lce_hip_status mul_i8_launch(const lce_hip_mul_int8_desc* d, const int8_t* in1_dev, const int8_t* in2_dev, const int8_t* addend_dev,
                             size_t rows, size_t channels, size_t rows_per_image, const int8_t* out_dev, const int32_t* out_bits_dev,
                             const char* who, bool need_pointers, MulI8Launch* L) {
  MulI8Plan P;
  if (lce_hip_status s = mul_i8_plan(d, who, &P)) return s;
  if (channels >= (1ull << 31)) return fail(LCE_HIP_ERR_INVALID, "%s: channels must be below 2^31", who);
  L->per_image = d->operand == LCE_HIP_EW_PER_IMAGE_CHANNEL;
  if (L->per_image && rows_per_image == 0) return fail(LCE_HIP_ERR_INVALID, "%s: rows_per_image is 0 with a per-image operand", who);
  if (rows_per_image != 0 && rows % rows_per_image != 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: rows_per_image %zu does not divide rows %zu", who, rows_per_image, rows);
  lce::MulI8Args& M = L->args;
  memset(&M, 0, sizeof M);
  L->add = lce::kMulI8NoAdd;
  M.zo_last = d->out_zero_point;
  if (d->has_add) {
    PreparedAddI8 H;
    if (lce_hip_status s = prepared_add_int8(&P.add, &H, who)) return s;
    M.A = H.args;
    M.A.c = H.c_for[H.variant];
    L->add = H.variant;
    M.product_first = H.swapped ? 0u : 1u;
    M.zo_last = d->add_zero_point;
  }
  if (need_pointers) {
    if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
    if (!in1_dev || !in2_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
    if (d->has_add && !addend_dev) return fail(LCE_HIP_ERR_INVALID, "%s: addend_dev is null with has_add", who);
    if (!d->has_add && addend_dev) return fail(LCE_HIP_ERR_INVALID, "%s: an addend_dev without has_add", who);
  }
  if ((uintptr_t)out_bits_dev % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: out_bits_dev must be 4-byte aligned", who);
  M.x = in1_dev; M.g = in2_dev; M.addend = addend_dev;
  M.A.out = const_cast<int8_t*>(out_dev);
  M.A.bits = (uint32_t*)const_cast<int32_t*>(out_bits_dev);
  M.A.rows = rows;
  M.A.channels = (uint32_t)channels;
  M.A.wpr = (uint32_t)((channels + 31) / 32);
  M.z1 = d->in1_zero_point; M.z2 = d->in2_zero_point; M.zo = d->out_zero_point;
  M.m = P.params.multiplier;
  M.left = P.params.shift > 0 ? P.params.shift : 0;
  M.right = P.params.shift > 0 ? 0 : -P.params.shift;
  M.lo = P.params.act_min; M.hi = P.params.act_max;
  M.half = M.right >= 1 ? 1 << (M.right - 1) : 0;
  L->mul = mul_i8_fast_is_proven(M) ? lce::kMulI8Fast : lce::kMulI8Literal;
  M.cpr = (uint32_t)(channels / 16);
  M.rows_per_image = rows_per_image ? rows_per_image : (rows ? rows : 1);
  const bool aligned = ((uintptr_t)in1_dev % 16 == 0) && ((uintptr_t)in2_dev % 16 == 0) && ((uintptr_t)addend_dev % 16 == 0) &&
                       ((uintptr_t)out_dev % 16 == 0);
  L->flat = channels % 16 == 0 && aligned;
  // memory-bound streams: 4 waves per block, at most ~8 blocks per CU, the waves stride over the rest (as lce_tu_eltwise_i8.hip)
  const uint64_t wave_tasks = L->flat ? (rows * (uint64_t)M.cpr + 255) / 256 : rows * (uint64_t)((channels + 63) / 64);
  const uint64_t blocks = (wave_tasks + 3) / 4, cap = 256ull * 8ull;
  L->blocks = (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
  return LCE_HIP_OK;
}

// E(a) and LOGISTIC of include/lce_hip.h on the host, operation for operation what lce_kernels_exp.h and lce_kernels_eltwise.h do on
// the device (this file is built with -ffp-contract=off; fmaf is one rounding, rintf rounds to nearest even).
float host_exp_neg(float a) {
  if (!(a >= -104.0f)) return 0.0f;
  a = a > 0.0f ? 0.0f : a;
  const float n = rintf(a * 1.44269502f);
  float r = fmaf(n, -0.693145751953125f, a);
  r = fmaf(n, -1.42860676e-06f, r);
  float p = 1.98412701e-04f;
  p = fmaf(p, r, 1.38888892e-03f);
  p = fmaf(p, r, 8.33333377e-03f);
  p = fmaf(p, r, 4.16666679e-02f);
  p = fmaf(p, r, 1.66666672e-01f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  const int32_t ni = (int32_t)n;
  const bool low = ni < -125;
  uint32_t bits;
  memcpy(&bits, &p, 4);
  bits += (uint32_t)(ni + (low ? 64 : 0)) << 23;
  float y;
  memcpy(&y, &bits, 4);
  return y * (low ? 5.42101086e-20f : 1.0f);
}

float host_logistic(float x) {
  const bool pos = x >= 0.0f;
  const float e = host_exp_neg(pos ? -x : x);
  volatile float den = 1.0f + e;
  return (pos ? 1.0f : e) / den;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_mul_int8_prepare(const lce_hip_mul_int8_desc* desc, lce_hip_mul_int8_params* params) {
  const char* who = "lce_hip_mul_int8_prepare";
  if (!params) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  MulI8Plan P;
  if (lce_hip_status s = mul_i8_plan(desc, who, &P)) return s;
  *params = P.params;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_mul_int8(const lce_hip_mul_int8_desc* desc, const int8_t* in1_dev, const int8_t* in2_dev,
                                const int8_t* addend_dev, size_t rows, size_t channels, size_t rows_per_image, int8_t* out_dev,
                                int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_mul_int8";
  MulI8Launch L;
  const bool empty = rows == 0 || channels == 0;              // (an empty tensor may come with null pointers)
  if (lce_hip_status s = mul_i8_launch(desc, in1_dev, in2_dev, addend_dev, rows, channels, rows_per_image, out_dev, out_bits_dev, who,
                                       !empty, &L)) return s;
  if (empty) return LCE_HIP_OK;
  if (lce_hip_status s = require_device()) return s;
  const int e = lce::launch_mul_i8(L.args, L.mul, L.add, L.per_image, L.flat, L.blocks, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_mul_int8_path(const lce_hip_mul_int8_desc* desc, size_t rows, size_t channels, size_t rows_per_image,
                                     const int8_t* in1_dev, const int8_t* in2_dev, const int8_t* addend_dev, const int8_t* out_dev,
                                     const int32_t* out_bits_dev, lce_hip_mul_int8_launch* launch) {
  const char* who = "lce_hip_mul_int8_path";
  if (!launch) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  MulI8Launch L;
  if (lce_hip_status s = mul_i8_launch(desc, in1_dev, in2_dev, addend_dev, rows, channels, rows_per_image, out_dev, out_bits_dev, who,
                                       false, &L)) return s;
  launch->flat = L.flat ? 1 : 0;
  launch->blocks = (int32_t)L.blocks;
  launch->waves_per_block = 4;
  launch->add_variant = desc->has_add ? L.add : -1;
  launch->mul_variant = L.mul;
  // the ADD kernel's parameters are the 21 consecutive int32 of AddI8Args from z1 to hi_rel
  static_assert(offsetof(lce::AddI8Args, hi_rel) - offsetof(lce::AddI8Args, z1) == 20 * sizeof(int32_t), "z1 .. hi_rel are 21 int32");
  static_assert(sizeof launch->add_args == 21 * sizeof(int32_t), "add_args holds z1 .. hi_rel");
  memset(launch->add_args, 0, sizeof launch->add_args);
  launch->product_first = 0;
  if (desc->has_add) {
    launch->product_first = (int32_t)L.args.product_first;
    memcpy(launch->add_args, &L.args.A.z1, sizeof launch->add_args);
  }
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_logistic_int8_prepare(float in_scale, int32_t in_zero_point, float out_scale, int32_t out_zero_point,
                                             uint8_t* table) {
  const char* who = "lce_hip_logistic_int8_prepare";
  if (lce_hip_status s = ew_i8_quant(who, "in", in_scale, in_zero_point)) return s;
  if (out_scale != 1.0f / 256.0f || out_zero_point != -128)
    return fail(LCE_HIP_ERR_INVALID, "%s: the output quantization must be (1/256, -128), got (%g, %d)", who, (double)out_scale,
                (int)out_zero_point);
  if (!table) return LCE_HIP_OK;
  for (int v = -128; v < 128; ++v) {
    volatile float d = (float)(v - in_zero_point);
    volatile float x = in_scale * d;
    volatile float y256 = host_logistic(x) * 256.0f;
    const int32_t q = (int32_t)std::round((double)y256) - 128;   // round half away from zero (exact in double)
    table[v + 128] = (uint8_t)(int8_t)std::min(127, std::max(-128, q));
  }
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_logistic_int8(const uint8_t* table_dev, const int8_t* in_dev, size_t rows, size_t channels, int8_t* out_dev,
                                     int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_logistic_int8";
  // (the chain entry's own bound, which ew_i8_plan applies and this entry does not pass through)
  if (channels >= (1ull << 22)) return fail(LCE_HIP_ERR_INVALID, "%s: channels must be in [0, 2^22), got %zu", who, channels);
  if (rows == 0 || channels == 0) return LCE_HIP_OK;          // (an empty tensor may come with null pointers)
  if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
  if (!table_dev) return fail(LCE_HIP_ERR_INVALID, "%s: table_dev is null", who);
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: in_dev is null", who);
  // the chain's ONE_ROW launch without a head: one table row for every channel, the bits at the fixed zero point -128
  lce_hip_elementwise_i8_desc d;
  memset(&d, 0, sizeof d);
  d.channels = (int32_t)channels;
  EwI8Plan P;
  P.table_rows = 1;
  P.zo_last = -128;
  EwI8Launch L;
  if (lce_hip_status s = ew_i8_launch(&d, -1, in_dev, nullptr, table_dev, rows, out_dev, out_bits_dev, who, true, P, &L)) return s;
  if (lce_hip_status s = require_device()) return s;
  const int e = lce::launch_ew_i8(L.args, L.head, L.path, L.flat, L.blocks, L.threads, L.lds_bytes, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// Channel join: whole tensors (lce_hip_concat) and channel windows (lce_hip_join_windows), one kernel family (lce_kernels_join.h)
// ------------------------------------------------------------------------------------
static_assert(LCE_HIP_JOIN_MAX_WINDOWS == lce::kJoinMaxWindows, "the header's bound is the kernels'");
static_assert(LCE_HIP_CONCAT_MAX_INPUTS <= lce::kJoinMaxWindows, "a dense join is a join of whole-tensor windows");

// What both entries end with, once `who` has checked its arguments: path, grid stride, launch.
static lce_hip_status join_run(const char* who, int kind, const lce::JoinWindow* jw, int n, uint64_t rows, int32_t zero_point,
                               void* out_dev, int32_t* out_bits_dev, void* stream) {
  if (lce_hip_status s = require_device()) return s;
  lce::JoinArgs a;
  const bool vec = lce::join_fill(a, kind, jw, n, rows, zero_point, out_dev, (uint32_t*)out_bits_dev);
  if (vec) lce::join_set_stride(a, lce::join_vec_grid(a.total_chunks));
  const int e = lce::launch_join(a, kind, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_concat(lce_hip_dtype type, const void* const* inputs_dev, const int32_t* channels, int32_t num_inputs,
                              size_t rows, int32_t zero_point, void* out_dev, int32_t* out_bits_dev, void* stream) {
  if (type != LCE_HIP_F32 && type != LCE_HIP_I8 && type != LCE_HIP_BITPACKED)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: type must be float32, int8 or bitpacked int32, got %d", (int)type);
  if (num_inputs < 2 || num_inputs > LCE_HIP_CONCAT_MAX_INPUTS)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: num_inputs must be 2..%d, got %d", LCE_HIP_CONCAT_MAX_INPUTS, (int)num_inputs);
  if (!inputs_dev || !channels) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: null argument");
  uint64_t sum = 0;
  for (int32_t k = 0; k < num_inputs; ++k) {
    if (channels[k] <= 0) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: input %d: channels must be positive, got %d", (int)k, (int)channels[k]);
    sum += (uint64_t)channels[k];
  }
  if (sum >= (1ull << 31)) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: the joined channel count must be below 2^31");
  if (type == LCE_HIP_BITPACKED && out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: a bitpacked join has no bit output");
  if (type == LCE_HIP_I8 ? (zero_point < -128 || zero_point > 127) : zero_point != 0)
    return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: zero point %d (int8: -128..127; otherwise 0)", (int)zero_point);
  if (rows == 0) return LCE_HIP_OK;   // (an empty tensor may come with null pointers)
  if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: both outputs are null");
  if (rows >= (1ull << 32)) return fail(LCE_HIP_ERR_UNSUPPORTED, "lce_hip_concat: rows must be below 2^32");
  const uint64_t esz = type == LCE_HIP_I8 ? 1 : 4;
  const uint64_t wpr = (sum + 31) / 32;
  // the output ranges must not meet an input range: the row pitches differ, so there is no in-place join
  const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (out_dev ? rows * sum * esz : 0);
  const uintptr_t b0 = (uintptr_t)out_bits_dev, b1 = b0 + (out_bits_dev ? rows * wpr * 4 : 0);
  if (meet(o0, o1, b0, b1)) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: the two outputs overlap");
  lce::JoinWindow jw[lce::kJoinMaxWindows];
  for (int32_t k = 0; k < num_inputs; ++k) {
    if (!inputs_dev[k]) return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: input %d is null", (int)k);
    const uintptr_t i0 = (uintptr_t)inputs_dev[k], i1 = i0 + rows * (uint64_t)channels[k] * esz;
    if (meet(o0, o1, i0, i1) || meet(b0, b1, i0, i1))
      return fail(LCE_HIP_ERR_INVALID, "lce_hip_concat: an output overlaps input %d", (int)k);
    jw[k] = lce::JoinWindow{inputs_dev[k], nullptr, (uint32_t)channels[k], 0u, (uint32_t)channels[k]};   // the whole tensor
  }
  // (bitpacked words are 4-byte elements that nothing interprets: there is no bit output)
  return join_run("lce_hip_concat", type == LCE_HIP_I8 ? lce::kJoinI8 : lce::kJoinF32, jw, (int)num_inputs, rows, zero_point, out_dev,
                  out_bits_dev, stream);
}

// ---- channel windows ----
lce_hip_status lce_hip_join_windows_check(lce_hip_dtype type, const lce_hip_window* windows, int32_t num_windows) {
  const char* who = "lce_hip_join_windows";
  if (type != LCE_HIP_F32 && type != LCE_HIP_I8) return fail(LCE_HIP_ERR_INVALID, "%s: type must be float32 or int8, got %d", who, (int)type);
  if (num_windows < 1 || num_windows > LCE_HIP_JOIN_MAX_WINDOWS)
    return fail(LCE_HIP_ERR_INVALID, "%s: num_windows must be 1..%d, got %d", who, LCE_HIP_JOIN_MAX_WINDOWS, (int)num_windows);
  if (!windows) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  uint64_t sum = 0;
  for (int32_t k = 0; k < num_windows; ++k) {
    const lce_hip_window& w = windows[k];
    if (!w.data_dev) return fail(LCE_HIP_ERR_INVALID, "%s: window %d: data_dev is null", who, (int)k);
    if (w.reserved[0] != 0 || w.reserved[1] != 0) return fail(LCE_HIP_ERR_INVALID, "%s: window %d: reserved fields must be 0", who, (int)k);
    if (w.begin < 0 || w.count < 1 || w.pitch < 1 || (int64_t)w.begin + (int64_t)w.count > (int64_t)w.pitch)
      return fail(LCE_HIP_ERR_INVALID, "%s: window %d: [%d, %d + %d) is no window of %d channels", who, (int)k, (int)w.begin, (int)w.begin,
                  (int)w.count, (int)w.pitch);
    if (w.addend_dev && type != LCE_HIP_F32) return fail(LCE_HIP_ERR_INVALID, "%s: window %d: only a float32 window takes an addend", who, (int)k);
    if ((uintptr_t)w.addend_dev % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: window %d: the addend must be 4-byte aligned", who, (int)k);
    sum += (uint64_t)w.count;
  }
  if (sum >= (1ull << 31)) return fail(LCE_HIP_ERR_INVALID, "%s: the joined channel count must be below 2^31", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_join_windows(lce_hip_dtype type, const lce_hip_window* windows, int32_t num_windows, size_t rows,
                                    int32_t zero_point, void* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_join_windows";
  if (rows == 0) return LCE_HIP_OK;   // (an empty tensor may come with null pointers)
  if (lce_hip_status s = lce_hip_join_windows_check(type, windows, num_windows)) return s;
  if (type == LCE_HIP_I8 ? (zero_point < -128 || zero_point > 127) : zero_point != 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: zero point %d (int8: -128..127; float32: 0)", who, (int)zero_point);
  if (!out_dev && !out_bits_dev) return fail(LCE_HIP_ERR_INVALID, "%s: both outputs are null", who);
  if (rows >= (1ull << 32)) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: rows must be below 2^32", who);
  const uint64_t esz = type == LCE_HIP_I8 ? 1 : 4;
  uint64_t sum = 0;
  for (int32_t k = 0; k < num_windows; ++k) sum += (uint64_t)windows[k].count;
  const uint64_t wpr = (sum + 31) / 32;
  const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (out_dev ? rows * sum * esz : 0);
  const uintptr_t b0 = (uintptr_t)out_bits_dev, b1 = b0 + (out_bits_dev ? rows * wpr * 4 : 0);
  if (meet(o0, o1, b0, b1)) return fail(LCE_HIP_ERR_INVALID, "%s: the two outputs overlap", who);
  lce::JoinWindow jw[lce::kJoinMaxWindows];
  for (int32_t k = 0; k < num_windows; ++k) {
    const lce_hip_window& w = windows[k];
    const uintptr_t i0 = (uintptr_t)w.data_dev, i1 = i0 + rows * (uint64_t)w.pitch * esz;
    if (meet(o0, o1, i0, i1) || meet(b0, b1, i0, i1)) return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the source of window %d", who, (int)k);
    if (w.addend_dev) {
      const uintptr_t a0 = (uintptr_t)w.addend_dev, a1 = a0 + rows * (uint64_t)w.count * 4;
      if (meet(o0, o1, a0, a1) || meet(b0, b1, a0, a1)) return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the addend of window %d", who, (int)k);
    }
    jw[k] = lce::JoinWindow{w.data_dev, w.addend_dev, (uint32_t)w.pitch, (uint32_t)w.begin, (uint32_t)w.count};
  }
  return join_run(who, type == LCE_HIP_F32 ? lce::kJoinF32 : lce::kJoinI8, jw, (int)num_windows, rows, zero_point, out_dev, out_bits_dev, stream);
}

// ------------------------------------------------------------------------------------
// 2-D pooling (lce_kernels_pool.h)
// ------------------------------------------------------------------------------------
static_assert(LCE_HIP_POOL_MAX_TAPS == lce::kPoolMaxTaps, "the header's bound is the kernels'");
lce_hip_status lce_hip_pool2d_check(const lce_hip_pool2d_desc* d, int32_t* out_height, int32_t* out_width) {
  const char* who = "lce_hip_pool2d";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->op != LCE_HIP_POOL_MAX && d->op != LCE_HIP_POOL_AVERAGE) return fail(LCE_HIP_ERR_INVALID, "%s: unknown op %d", who, (int)d->op);
  if (d->type != LCE_HIP_F32 && d->type != LCE_HIP_I8) return fail(LCE_HIP_ERR_INVALID, "%s: type must be float32 or int8, got %d", who, (int)d->type);
  if (d->batch <= 0 || d->in_height <= 0 || d->in_width <= 0 || d->channels <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d, %d, %d]", who, (int)d->batch, (int)d->in_height,
                (int)d->in_width, (int)d->channels);
  const Window w{d->batch, d->in_height, d->in_width, d->filter_height, d->filter_width, d->stride_height, d->stride_width, d->padding,
                 d->activation};
  if (lce_hip_status s = check_window_options(who, w)) return s;
  if (d->type == LCE_HIP_I8) {
    if (d->zero_point < -128 || d->zero_point > 127)
      return fail(LCE_HIP_ERR_INVALID, "%s: zero_point must be in [-128, 127], got %d", who, (int)d->zero_point);
    if (!std::isfinite(d->scale) || !(d->scale > 0.0f))
      return fail(LCE_HIP_ERR_INVALID, "%s: scale must be finite and positive, got %g", who, (double)d->scale);
  }
  if (lce_hip_status s = check_extent_limit(who, w)) return s;
  // (the int8 AVERAGE divides in float: exact while 128.5 taps < 2^24, lce_kernels_pool.h)
  if ((int64_t)d->filter_height * d->filter_width > (int64_t)lce::kPoolMaxTaps)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: a filter of %d x %d has more than %d taps", who, (int)d->filter_height, (int)d->filter_width,
                lce::kPoolMaxTaps);
  return window_output(who, w, out_height, out_width);
}

lce_hip_status lce_hip_pool2d(const lce_hip_pool2d_desc* d, const void* in_dev, void* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_pool2d";
  if (lce_hip_status s = check_pointers(who, d, in_dev, /*has_filter=*/false, nullptr, out_dev, out_bits_dev)) return s;
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_pool2d_check(d, &oh, &ow)) return s;
  const uint64_t esz = d->type == LCE_HIP_I8 ? 1 : 4;
  const uint64_t C = (uint64_t)d->channels, pixels = (uint64_t)d->batch * oh * ow, wpr = (C + 31) / 32;
  const Span in(in_dev, (uint64_t)d->batch * d->in_height * d->in_width * C * esz), none(nullptr, 0);
  const Span out(out_dev, pixels * C * esz), bits(out_bits_dev, pixels * wpr * 4);
  if (lce_hip_status s = check_operand_ranges(who, in, none, none, out, bits, /*float_operands=*/false)) return s;
  if (lce_hip_status s = require_device()) return s;
  const bool vec = lce::window_vec_rule(1, C, esz, out_bits_dev != nullptr, in_dev, out_dev, nullptr, nullptr);
  lce::PoolArgs a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.out = out_dev; a.bits = (uint32_t*)out_bits_dev;
  window_fill(a, d->batch, d->in_height, d->in_width, d->filter_height, d->filter_width, d->stride_height, d->stride_width, oh, ow, C, 16 / esz,
              vec, /*stream_loads_rule=*/true);
  float_activation_range(d->activation, &a.lo, &a.hi);
  if (d->type == LCE_HIP_I8) {
    quantized_activation_range(d->activation, d->scale, d->zero_point, &a.qlo, &a.qhi);
    a.zero_point = d->zero_point;
  }
  const int e = lce::launch_pool(a, d->type == LCE_HIP_I8 ? lce::kPoolI8 : lce::kPoolF32,
                                 d->op == LCE_HIP_POOL_AVERAGE ? lce::kPoolAverage : lce::kPoolMax, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "lce_hip_pool2d: launch failed: %s", hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// float 1x1 CONV_2D (lce_kernels_conv1x1.h)
// ------------------------------------------------------------------------------------
lce_hip_status lce_hip_conv1x1_f32_check(const lce_hip_conv1x1_desc* d, int32_t* out_height, int32_t* out_width) {
  const char* who = "lce_hip_conv1x1_f32";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->in_height <= 0 || d->in_width <= 0 || d->channels_in <= 0 || d->channels_out <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d, %d, %d] -> %d channels", who, (int)d->batch,
                (int)d->in_height, (int)d->in_width, (int)d->channels_in, (int)d->channels_out);
  const Window w{d->batch, d->in_height, d->in_width, 1, 1, d->stride_height, d->stride_width, LCE_HIP_PADDING_VALID, d->activation};
  if (lce_hip_status s = check_window_options(who, w)) return s;
  if (lce_hip_status s = check_extent_limit(who, w)) return s;
  // (one grid row per 128 output channels)
  if ((int64_t)d->channels_out > 65535ll * lce::kConv1x1BN)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: more than %lld output channels are not supported", who, 65535ll * lce::kConv1x1BN);
  // a 1x1 filter has no padding taps: SAME and VALID both give ceil(in / stride)
  const int32_t oh = (int32_t)(((int64_t)d->in_height + d->stride_height - 1) / d->stride_height);
  const int32_t ow = (int32_t)(((int64_t)d->in_width + d->stride_width - 1) / d->stride_width);
  return report_output(who, w, oh, ow, out_height, out_width);
}

lce_hip_status lce_hip_conv1x1_f32(const lce_hip_conv1x1_desc* d, const float* in_dev, const float* filter_dev, const float* bias_dev,
                                   float* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_conv1x1_f32";
  if (lce_hip_status s = check_pointers(who, d, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_conv1x1_f32_check(d, &oh, &ow)) return s;
  const uint64_t K = (uint64_t)d->channels_in, N = (uint64_t)d->channels_out, pixels = (uint64_t)d->batch * oh * ow, wpr = (N + 31) / 32;
  const Span in(in_dev, (uint64_t)d->batch * d->in_height * d->in_width * K * 4), filter(filter_dev, N * K * 4), bias(bias_dev, N * 4);
  const Span out(out_dev, pixels * N * 4), bits(out_bits_dev, pixels * wpr * 4);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, bias, out, bits, /*float_operands=*/true)) return s;
  if (lce_hip_status s = require_device()) return s;
  lce::Conv1x1Args a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.filter = filter_dev; a.bias = bias_dev; a.out = out_dev; a.bits = (uint32_t*)out_bits_dev;
  a.M = (uint32_t)pixels; a.Cin = (uint32_t)K; a.Cout = (uint32_t)N; a.wpr = (uint32_t)wpr;
  a.mtiles = (uint32_t)((pixels + lce::kConv1x1BM - 1) / lce::kConv1x1BM);
  a.OW = (uint32_t)ow; a.OHW = (uint32_t)oh * (uint32_t)ow;          // (both < 2^31: pixels is)
  a.IW = (uint32_t)d->in_width;
  a.IHW = (uint64_t)d->in_height * (uint64_t)d->in_width;
  a.sh = (uint32_t)d->stride_height; a.sw = (uint32_t)d->stride_width;
  a.strided = d->stride_height != 1 || d->stride_width != 1 ? 1u : 0u;
  float_activation_range(d->activation, &a.lo, &a.hi);
  const bool vec = K % 4 == 0 && in.lo % 16 == 0 && filter.lo % 16 == 0;
  const int e = lce::launch_conv1x1(a, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// the float classifier head: FULLY_CONNECTED and SOFTMAX (lce_kernels_head.h)
// ------------------------------------------------------------------------------------
lce_hip_status lce_hip_fully_connected_f32_check(const lce_hip_fc_desc* d) {
  const char* who = "lce_hip_fully_connected_f32";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->inputs <= 0 || d->outputs <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d] -> %d outputs", who, (int)d->batch, (int)d->inputs,
                (int)d->outputs);
  if (d->activation < LCE_HIP_ACT_NONE || d->activation > LCE_HIP_ACT_RELU6)
    return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", who, (int)d->activation);
  // (the kernel numbers its 16 x 16 tiles in 32 bits)
  const uint64_t tiles = (((uint64_t)d->batch + lce::kFcTile - 1) / lce::kFcTile) * (((uint64_t)d->outputs + lce::kFcTile - 1) / lce::kFcTile);
  if (tiles >= (1ull << 31)) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: an output of more than 2^31 tiles of 16 x 16 is not supported", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_fully_connected_f32(const lce_hip_fc_desc* d, const float* in_dev, const float* weights_dev, const float* bias_dev,
                                           float* out_dev, void* stream) {
  const char* who = "lce_hip_fully_connected_f32";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!weights_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null weights", who);
  if (!out_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null output", who);
  if (lce_hip_status s = lce_hip_fully_connected_f32_check(d)) return s;
  const uint64_t M = (uint64_t)d->batch, K = (uint64_t)d->inputs, N = (uint64_t)d->outputs;
  const Span in(in_dev, M * K * 4), weights(weights_dev, N * K * 4), bias(bias_dev, N * 4), out(out_dev, M * N * 4), none(nullptr, 0);
  if (lce_hip_status s = check_operand_ranges(who, in, weights, bias, out, none, /*float_operands=*/true)) return s;
  if (lce_hip_status s = require_device()) return s;
  lce::FcArgs a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.filter = weights_dev; a.bias = bias_dev; a.out = out_dev;
  lce::fc_fill(a, d->batch, d->inputs, d->outputs);
  float_activation_range(d->activation, &a.lo, &a.hi);
  const int e = lce::launch_fully_connected(a, lce::fc_vec_rule(a), stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_softmax_f32_check(size_t rows, size_t cols, float beta) {
  const char* who = "lce_hip_softmax_f32";
  if (rows == 0 || cols == 0) return fail(LCE_HIP_ERR_INVALID, "%s: rows and cols must be positive, got %zu x %zu", who, rows, cols);
  if (!std::isfinite(beta) || !(beta > 0.0f)) return fail(LCE_HIP_ERR_INVALID, "%s: beta must be finite and positive, got %g", who, (double)beta);
  if ((uint64_t)cols >= (1ull << 31) || (uint64_t)rows > (1ull << 60) / (uint64_t)cols)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: rows of 2^31 elements or more, or more than 2^60 elements, are not supported", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_softmax_f32(size_t rows, size_t cols, float beta, const float* in_dev, float* out_dev, void* stream) {
  const char* who = "lce_hip_softmax_f32";
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!out_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null output", who);
  if (lce_hip_status s = lce_hip_softmax_f32_check(rows, cols, beta)) return s;
  const Span in(in_dev, (uint64_t)rows * cols * 4), out(out_dev, (uint64_t)rows * cols * 4);
  if ((in.lo | out.lo) % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: every pointer must be 4-byte aligned", who);
  // in place is the one overlap that is safe: a lane writes only the elements it alone reads
  if (in.lo != out.lo && meet(in.lo, in.hi, out.lo, out.hi)) return fail(LCE_HIP_ERR_INVALID, "%s: the output partly overlaps the input", who);
  if (lce_hip_status s = require_device()) return s;
  lce::SoftmaxArgs a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.out = out_dev; a.rows = rows; a.cols = (uint32_t)cols; a.beta = beta;
  const int e = lce::launch_softmax(a, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// the binarized Dense layer (lce_kernels_bfc.h)
// ------------------------------------------------------------------------------------
lce_hip_status lce_hip_bfc_check(const lce_hip_bfc_desc* d) {
  const char* who = "lce_hip_binary_fully_connected";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->inputs <= 0 || d->outputs <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d] -> %d outputs", who, (int)d->batch, (int)d->inputs,
                (int)d->outputs);
  if (d->activation < LCE_HIP_ACT_NONE || d->activation > LCE_HIP_ACT_RELU6)
    return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", who, (int)d->activation);
  // (every partial sum stays an exact float32 integer -- the planner's bound on a convolution's K)
  if (d->inputs >= (1 << 23)) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: 2^23 or more inputs are not supported", who);
  // (the kernel numbers its 32 x 32 tiles in 32 bits)
  const uint64_t tiles = (((uint64_t)d->batch + lce::kBfcTile - 1) / lce::kBfcTile) * (((uint64_t)d->outputs + lce::kBfcTile - 1) / lce::kBfcTile);
  if (tiles >= (1ull << 31)) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: an output of more than 2^31 tiles of 32 x 32 is not supported", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bfc_prepare(const lce_hip_bfc_desc* d, const float* weights_host, int32_t* bits, float* scale) {
  const char* who = "lce_hip_bfc_prepare";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!weights_host || !bits || !scale) return fail(LCE_HIP_ERR_INVALID, "%s: null weights, bits or scale", who);
  if (lce_hip_status s = lce_hip_bfc_check(d)) return s;
  const size_t K = (size_t)d->inputs, N = (size_t)d->outputs, Kw = (K + 31) / 32;
  const float smin = std::ldexp(1.0f, -100), smax = std::ldexp(1.0f, 100);
  for (size_t o = 0; o < N; ++o) {
    const float* row = weights_host + o * K;
    const float s = std::fabs(row[0]);
    if (!(s >= smin && s <= smax))       // (a NaN fails both comparisons)
      return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: the weights of output %zu are not +-s with 2^-100 <= s <= 2^100 (the first is %g)", who, o,
                  (double)row[0]);
    uint32_t* words = (uint32_t*)bits + o * Kw;
    for (size_t w = 0; w < Kw; ++w) words[w] = 0u;
    for (size_t k = 0; k < K; ++k) {
      if (!(std::fabs(row[k]) == s))
        return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: the weights of output %zu are not all +-%g (input %zu holds %g)", who, o, (double)s, k,
                    (double)row[k]);
      if (std::signbit(row[k])) words[k / 32] |= 1u << (k % 32);
    }
    scale[o] = s;
  }
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_binary_fully_connected(const lce_hip_bfc_desc* d, const int32_t* in_bits_dev, const int32_t* weight_bits_dev,
                                              const float* scale_dev, const float* bias_dev, float* out_dev, int32_t* out_bits_dev,
                                              void* stream) {
  const char* who = "lce_hip_binary_fully_connected";
  if (lce_hip_status s = check_pointers(who, d, in_bits_dev, /*has_filter=*/true, weight_bits_dev, out_dev, out_bits_dev)) return s;
  if (!scale_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null scale", who);
  if (lce_hip_status s = lce_hip_bfc_check(d)) return s;
  const uint64_t M = (uint64_t)d->batch, K = (uint64_t)d->inputs, N = (uint64_t)d->outputs, Kw = (K + 31) / 32, wpr = (N + 31) / 32;
  const Span in(in_bits_dev, M * Kw * 4), weights(weight_bits_dev, N * Kw * 4), scale(scale_dev, N * 4), bias(bias_dev, N * 4);
  const Span out(out_dev, M * N * 4), bits(out_bits_dev, M * wpr * 4);
  if (lce_hip_status s = check_operand_ranges(who, in, weights, bias, out, bits, /*float_operands=*/true)) return s;
  if (meet(out.lo, out.hi, scale.lo, scale.hi) || meet(bits.lo, bits.hi, scale.lo, scale.hi))
    return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the scale", who);
  if (scale.lo % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: every pointer must be 4-byte aligned", who);
  if (lce_hip_status s = require_device()) return s;
  lce::BfcArgs a;
  memset(&a, 0, sizeof a);
  a.in = (const uint32_t*)in_bits_dev; a.weights = (const uint32_t*)weight_bits_dev; a.scale = scale_dev; a.bias = bias_dev;
  a.out = out_dev; a.bits = (uint32_t*)out_bits_dev;
  lce::bfc_fill(a, d->batch, d->inputs, d->outputs);
  float_activation_range(d->activation, &a.lo, &a.hi);
  const int e = lce::launch_binary_fully_connected(a, lce::bfc_vec_rule(a), stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// float DEPTHWISE_CONV_2D (lce_kernels_depthwise.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// The descriptor checks the float and the int8 DEPTHWISE_CONV_2D share: every message is `who`'s own.
lce_hip_status depthwise_desc_check(const char* who, const lce_hip_depthwise_desc* d, int32_t* out_height, int32_t* out_width) {
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->in_height <= 0 || d->in_width <= 0 || d->channels_in <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d, %d, %d]", who, (int)d->batch, (int)d->in_height,
                (int)d->in_width, (int)d->channels_in);
  if (d->depth_multiplier <= 0) return fail(LCE_HIP_ERR_INVALID, "%s: the depth multiplier must be positive, got %d", who, (int)d->depth_multiplier);
  const Window w{d->batch, d->in_height, d->in_width, d->filter_height, d->filter_width, d->stride_height, d->stride_width, d->padding,
                 d->activation};
  if (lce_hip_status s = check_window_options(who, w)) return s;
  if (lce_hip_status s = check_extent_limit(who, w)) return s;
  // (the filter's element count -- and with it Cout and each filter extent -- stays below 2^31; compared by division, so
  // that the product of four 31-bit factors is never formed)
  const uint64_t taps = (uint64_t)d->filter_height * (uint64_t)d->filter_width;
  const uint64_t cout = (uint64_t)d->channels_in * (uint64_t)d->depth_multiplier;
  if (cout > ((1ull << 31) - 1) / taps)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: a filter of 2^31 or more elements (%d x %d x %llu) is not supported", who,
                (int)d->filter_height, (int)d->filter_width, (unsigned long long)cout);
  return window_output(who, w, out_height, out_width);
}
}  // namespace
extern "C" {
lce_hip_status lce_hip_depthwise_conv2d_f32_check(const lce_hip_depthwise_desc* d, int32_t* out_height, int32_t* out_width) {
  return depthwise_desc_check("lce_hip_depthwise_conv2d_f32", d, out_height, out_width);
}

lce_hip_status lce_hip_depthwise_conv2d_f32(const lce_hip_depthwise_desc* d, const float* in_dev, const float* filter_dev,
                                            const float* bias_dev, float* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_depthwise_conv2d_f32";
  if (lce_hip_status s = check_pointers(who, d, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_depthwise_conv2d_f32_check(d, &oh, &ow)) return s;
  const uint64_t Cin = (uint64_t)d->channels_in, C = Cin * (uint64_t)d->depth_multiplier;
  const uint64_t pixels = (uint64_t)d->batch * oh * ow, wpr = (C + 31) / 32;
  const Span in(in_dev, (uint64_t)d->batch * d->in_height * d->in_width * Cin * 4);
  const Span filter(filter_dev, (uint64_t)d->filter_height * d->filter_width * C * 4), bias(bias_dev, C * 4);
  const Span out(out_dev, pixels * C * 4), bits(out_bits_dev, pixels * wpr * 4);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, bias, out, bits, /*float_operands=*/true)) return s;
  if (lce_hip_status s = require_device()) return s;
  const bool vec = lce::window_vec_rule(d->depth_multiplier, C, 4, out_bits_dev != nullptr, in_dev, filter_dev, bias_dev, out_dev);
  lce::DepthwiseArgs a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.P;
  p.in = in_dev; p.out = out_dev; p.bits = (uint32_t*)out_bits_dev;
  a.filter = filter_dev; a.bias = bias_dev;
  a.channels_in = (uint32_t)Cin; a.div_multiplier = lce::make_fastdiv((uint32_t)d->depth_multiplier);
  window_fill(p, d->batch, d->in_height, d->in_width, d->filter_height, d->filter_width, d->stride_height, d->stride_width, oh, ow, C, 4, vec,
              /*stream_loads_rule=*/true);
  float_activation_range(d->activation, &p.lo, &p.hi);
  const int e = lce::launch_depthwise(a, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// float CONV_2D of any filter extent (lce_kernels_conv2d.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// The descriptor checks the float and the int8 CONV_2D share: every message is `who`'s own.
lce_hip_status conv2d_desc_check(const char* who, const lce_hip_conv2d_desc* d, int32_t* out_height, int32_t* out_width) {
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->in_height <= 0 || d->in_width <= 0 || d->channels_in <= 0 || d->channels_out <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d, %d, %d] -> %d channels", who, (int)d->batch,
                (int)d->in_height, (int)d->in_width, (int)d->channels_in, (int)d->channels_out);
  const Window w{d->batch, d->in_height, d->in_width, d->filter_height, d->filter_width, d->stride_height, d->stride_width, d->padding,
                 d->activation};
  if (lce_hip_status s = check_window_options(who, w)) return s;
  if (lce_hip_status s = check_extent_limit(who, w)) return s;
  // (K = fh x fw x Cin -- and with it each filter extent -- stays below 2^31; compared by division, so that the product of
  // three 31-bit factors is never formed)
  const uint64_t taps = (uint64_t)d->filter_height * (uint64_t)d->filter_width;
  if ((uint64_t)d->channels_in > ((1ull << 31) - 1) / taps)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: a filter of 2^31 or more elements per output channel (%d x %d x %d) is not supported", who,
                (int)d->filter_height, (int)d->filter_width, (int)d->channels_in);
  // (one grid row per 128 output channels)
  if ((int64_t)d->channels_out > 65535ll * lce::kConv2dBN)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: more than %lld output channels are not supported", who, 65535ll * lce::kConv2dBN);
  return window_output(who, w, out_height, out_width);
}
}  // namespace
extern "C" {
lce_hip_status lce_hip_conv2d_f32_check(const lce_hip_conv2d_desc* d, int32_t* out_height, int32_t* out_width) {
  return conv2d_desc_check("lce_hip_conv2d_f32", d, out_height, out_width);
}

lce_hip_status lce_hip_conv2d_f32(const lce_hip_conv2d_desc* d, const float* in_dev, const float* filter_dev, const float* bias_dev,
                                  float* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_conv2d_f32";
  if (lce_hip_status s = check_pointers(who, d, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_conv2d_f32_check(d, &oh, &ow)) return s;
  const uint64_t Cin = (uint64_t)d->channels_in, N = (uint64_t)d->channels_out;
  const uint64_t K = (uint64_t)d->filter_height * d->filter_width * Cin;             // < 2^31
  const uint64_t pixels = (uint64_t)d->batch * oh * ow, wpr = (N + 31) / 32;
  const Span in(in_dev, (uint64_t)d->batch * d->in_height * d->in_width * Cin * 4), filter(filter_dev, N * K * 4), bias(bias_dev, N * 4);
  const Span out(out_dev, pixels * N * 4), bits(out_bits_dev, pixels * wpr * 4);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, bias, out, bits, /*float_operands=*/true)) return s;
  if (lce_hip_status s = require_device()) return s;
  lce::Conv2dArgs a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.filter = filter_dev; a.bias = bias_dev; a.out = out_dev; a.bits = (uint32_t*)out_bits_dev;
  lce::conv2d_geometry(a, d->batch, d->in_height, d->in_width, d->channels_in, d->channels_out, d->filter_height, d->filter_width,
                       d->stride_height, d->stride_width, oh, ow);
  float_activation_range(d->activation, &a.lo, &a.hi);
  const int e = lce::launch_conv2d(a, lce::conv2d_vec_rule(a), stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// int8 CONV_2D of any filter extent (lce_kernels_conv2d_i8.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
static_assert(lce::kConvI8BN == lce::kConv2dBN, "conv2d_desc_check bounds the output channels for both");

// The quantization of a lce_hip_conv2d_i8_desc: scales finite and positive, zero points int8 values.
lce_hip_status conv2d_i8_quantization_check(const char* who, const lce_hip_conv2d_i8_desc* d) {
  const float scales[2] = {d->input_scale, d->output_scale};
  const int32_t zps[2] = {d->input_zero_point, d->output_zero_point};
  static const char* const names[2] = {"input", "output"};
  for (int i = 0; i < 2; ++i) {
    if (!std::isfinite(scales[i]) || !(scales[i] > 0.0f))
      return fail(LCE_HIP_ERR_INVALID, "%s: %s_scale must be finite and positive, got %g", who, names[i], (double)scales[i]);
    if (zps[i] < -128 || zps[i] > 127)
      return fail(LCE_HIP_ERR_INVALID, "%s: %s_zero_point must be in [-128, 127], got %d", who, names[i], (int)zps[i]);
  }
  return LCE_HIP_OK;
}

lce_hip_conv2d_desc conv2d_i8_window(const lce_hip_conv2d_i8_desc* d) {
  return lce_hip_conv2d_desc{d->batch, d->in_height, d->in_width, d->channels_in, d->channels_out, d->filter_height, d->filter_width,
                             d->stride_height, d->stride_width, d->padding, d->activation};
}

// Everything lce_hip_conv2d_i8_check refuses but the K limit, which lce_hip_conv2d_i8_prepare states with the bias and a channel.
lce_hip_status conv2d_i8_desc_check(const char* who, const lce_hip_conv2d_i8_desc* d, int32_t* out_height, int32_t* out_width) {
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  const lce_hip_conv2d_desc w = conv2d_i8_window(d);
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = conv2d_desc_check(who, &w, &oh, &ow)) return s;
  if (lce_hip_status s = conv2d_i8_quantization_check(who, d)) return s;
  if (out_height) *out_height = oh;
  if (out_width) *out_width = ow;
  return LCE_HIP_OK;
}

// The table of lce_hip_conv2d_i8_prepare for N output channels of K filter elements each (the FULLY_CONNECTED of the int8 head
// is the 1x1 case: lce_hip_fully_connected_i8_prepare).  The descriptor has been checked.  Without a filter (the depthwise
// entry, whose kernel skips the taps in the padding and subtracts zi itself: K = fh x fw) no zero point is folded: c[o] = bias[o].
lce_hip_status conv2d_i8_table(const char* who, int64_t N, int64_t K, float si, int32_t zi, float so, const int8_t* filter_host,
                               const int32_t* bias_host, const float* filter_scales, int32_t n_scales, int32_t* table) {
  if (n_scales != 1 && (int64_t)n_scales != N)
    return fail(LCE_HIP_ERR_INVALID, "%s: the filter has %d scales, neither 1 nor one per output channel (%d)", who, (int)n_scales, (int)N);
  for (int32_t o = 0; o < n_scales; ++o)
    if (!std::isfinite(filter_scales[o]) || !(filter_scales[o] > 0.0f))
      return fail(LCE_HIP_ERR_INVALID, "%s: the filter scale of channel %d must be finite and positive, got %g", who, (int)o,
                  (double)filter_scales[o]);
  // The reference's accumulator: |x - zi| <= 255, |w| <= 128, K products and the bias.
  const int64_t kMax = 2147483647ll;
  int64_t B = 0, b_channel = 0;
  if (bias_host)
    for (int64_t o = 0; o < N; ++o) {
      const int64_t v = bias_host[o] < 0 ? -(int64_t)bias_host[o] : (int64_t)bias_host[o];
      if (v > B) { B = v; b_channel = o; }
    }
  const int64_t bound = 255ll * 128ll * K + B;                                     // < 2^47
  if (bound > kMax)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: channel %lld: 255 x 128 x K + |bias| = 255 x 128 x %lld + %lld exceeds 2^31 - 1: the reference's "
                "int32 accumulator could overflow", who, (long long)b_channel, (long long)K, (long long)B);
  for (int64_t o = 0; o < N; ++o) {
    const double real = (double)si * (double)filter_scales[n_scales == 1 ? 0 : o] / (double)so;
    int32_t m = 0, e = 0;
    quantize_multiplier(real, &m, &e);
    if (e > 0 && (e >= 31 || (bound << e) > kMax))
      return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: channel %lld: the accumulator bound %lld times 2^%d (the left shift of its multiplier %g) "
                  "exceeds 2^31 - 1", who, (long long)o, (long long)bound, (int)e, real);
    int64_t sum = 0;
    if (filter_host) {
      const int8_t* w = filter_host + (uint64_t)o * (uint64_t)K;
      for (int64_t k = 0; k < K; ++k) sum += w[k];
    }
    // |zi * sum| <= 128 x 128 x K and |bias[o]| <= B, so |c| <= 128 x 128 x K + B <= 255 x 128 x K + B = bound <= 2^31 - 1:
    // the first bound already implies that c fits.  Checked all the same.
    const int64_t c = (bias_host ? (int64_t)bias_host[o] : 0ll) - (int64_t)zi * sum;
    if (c > kMax || c < -kMax - 1)
      return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: channel %lld: the constant bias - zero_point x sum(w) = %lld does not fit int32", who,
                  (long long)o, (long long)c);
    table[o] = (int32_t)c;
    table[N + o] = m;
    table[2 * N + o] = e;
  }
  return LCE_HIP_OK;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_conv2d_i8_check(const lce_hip_conv2d_i8_desc* d, int32_t* out_height, int32_t* out_width) {
  const char* who = "lce_hip_conv2d_i8";
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = conv2d_i8_desc_check(who, d, &oh, &ow)) return s;
  // (lce_hip_conv2d_i8_prepare's first bound without a bias: beyond it no table exists, and the kernel's 32-bit window
  // arithmetic relies on it)
  const uint64_t K = (uint64_t)d->filter_height * d->filter_width * (uint64_t)d->channels_in;       // < 2^31
  if (K > lce::kConvI8MaxK)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: a filter of %llu elements per output channel could overflow the int32 accumulator "
                "(255 x 128 x K must not exceed 2^31 - 1: K <= %u)", who, (unsigned long long)K, (unsigned)lce::kConvI8MaxK);
  if (out_height) *out_height = oh;
  if (out_width) *out_width = ow;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_conv2d_i8_prepare(const lce_hip_conv2d_i8_desc* d, const int8_t* filter_host, const int32_t* bias_host,
                                         const float* filter_scales, int32_t n_scales, int32_t* table, int32_t* act_min, int32_t* act_max) {
  const char* who = "lce_hip_conv2d_i8_prepare";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!filter_host) return fail(LCE_HIP_ERR_INVALID, "%s: null filter", who);
  if (!filter_scales) return fail(LCE_HIP_ERR_INVALID, "%s: null filter scales", who);
  if (!table || !act_min || !act_max) return fail(LCE_HIP_ERR_INVALID, "%s: null result", who);
  if (lce_hip_status s = conv2d_i8_desc_check(who, d, nullptr, nullptr)) return s;
  const int64_t N = d->channels_out, K = (int64_t)d->filter_height * d->filter_width * d->channels_in;       // K < 2^31
  if (lce_hip_status s = conv2d_i8_table(who, N, K, d->input_scale, d->input_zero_point, d->output_scale, filter_host, bias_host,
                                         filter_scales, n_scales, table))
    return s;
  quantized_activation_range(d->activation, d->output_scale, d->output_zero_point, act_min, act_max);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_conv2d_i8(const lce_hip_conv2d_i8_desc* d, const int8_t* in_dev, const int8_t* filter_dev, const int32_t* table_dev,
                                 int8_t* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_conv2d_i8";
  if (lce_hip_status s = check_pointers(who, d, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  if (!table_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null table", who);
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_conv2d_i8_check(d, &oh, &ow)) return s;
  const uint64_t Cin = (uint64_t)d->channels_in, N = (uint64_t)d->channels_out;
  const uint64_t K = (uint64_t)d->filter_height * d->filter_width * Cin;
  const uint64_t pixels = (uint64_t)d->batch * oh * ow, wpr = (N + 31) / 32;
  const Span in(in_dev, (uint64_t)d->batch * d->in_height * d->in_width * Cin), filter(filter_dev, N * K), table(table_dev, 3 * N * 4);
  const Span out(out_dev, pixels * N), bits(out_bits_dev, pixels * wpr * 4);
  // (the table stands where the float entry has its bias)
  if (meet(out.lo, out.hi, table.lo, table.hi) || meet(bits.lo, bits.hi, table.lo, table.hi))
    return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the table", who);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, Span(nullptr, 0), out, bits, /*float_operands=*/false)) return s;
  if (table.lo % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: table_dev must be 4-byte aligned", who);
  if (lce_hip_status s = require_device()) return s;
  lce::ConvI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.filter = filter_dev; a.table = table_dev; a.out = out_dev; a.bits = (uint32_t*)out_bits_dev;
  lce::conv2d_i8_geometry(a, d->batch, d->in_height, d->in_width, d->channels_in, d->channels_out, d->filter_height, d->filter_width,
                          d->stride_height, d->stride_width, oh, ow);
  a.zi = d->input_zero_point; a.zo = d->output_zero_point;
  quantized_activation_range(d->activation, d->output_scale, d->output_zero_point, &a.act_min, &a.act_max);
  const int e = lce::launch_conv2d_i8(a, lce::conv2d_i8_vec_rule(a), stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// the int8 classifier head and the float/int8 boundary (lce_kernels_head_i8.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
static_assert(lce::kFcI8MaxK == lce::kConvI8MaxK, "lce_hip_fully_connected_i8 refuses the K that lce_hip_conv2d_i8 refuses");

// One (scale, zero point) of an int8 tensor: the scale finite and positive, the zero point an int8 value.
lce_hip_status head_i8_quantization_check(const char* who, const char* name, float scale, int32_t zero_point) {
  if (!std::isfinite(scale) || !(scale > 0.0f))
    return fail(LCE_HIP_ERR_INVALID, "%s: %s_scale must be finite and positive, got %g", who, name, (double)scale);
  if (zero_point < -128 || zero_point > 127)
    return fail(LCE_HIP_ERR_INVALID, "%s: %s_zero_point must be in [-128, 127], got %d", who, name, (int)zero_point);
  return LCE_HIP_OK;
}

// lce_hip_mean_i8's multiplier and the bound of its header comment.
lce_hip_status mean_i8_multiplier(const char* who, const lce_hip_mean_i8_desc* d, int32_t* m, int32_t* e) {
  if (lce_hip_status s = lce_hip_mean_i8_check(d)) return s;
  quantize_multiplier((double)d->input_scale / (double)d->output_scale, m, e);
  const int64_t n = (int64_t)d->height * d->width, kMax = 2147483647ll;             // n < 2^62
  const int32_t left = *e > 0 ? *e : 0;
  if (n > kMax / 255 || left >= 31 || ((255ll * n) << left) + n / 2 > kMax)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: 255 x n x 2^max(e,0) + n/2 with n = %lld pixels and e = %d (the multiplier %g) exceeds "
                "2^31 - 1: an intermediate could leave int32", who, (long long)n, (int)*e,
                (double)d->input_scale / (double)d->output_scale);
  return LCE_HIP_OK;
}

// The quantization and pointer checks QUANTIZE and DEQUANTIZE share; `f32` / `i8`: the float and the int8 side.
lce_hip_status quant_check(const char* who, size_t n, float scale, int32_t zero_point, const void* in, const void* out, const void* f32,
                           uint64_t in_size, uint64_t out_size) {
  if (!in) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!out) return fail(LCE_HIP_ERR_INVALID, "%s: null output", who);
  if (lce_hip_status s = head_i8_quantization_check(who, "the", scale, zero_point)) return s;
  if ((uint64_t)n > (1ull << 60)) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: more than 2^60 elements are not supported", who);
  if ((uintptr_t)f32 % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: the float pointer must be 4-byte aligned", who);
  const Span i(in, (uint64_t)n * in_size), o(out, (uint64_t)n * out_size);
  if (meet(i.lo, i.hi, o.lo, o.hi)) return fail(LCE_HIP_ERR_INVALID, "%s: the output overlaps the input", who);
  return LCE_HIP_OK;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_fully_connected_i8_check(const lce_hip_fc_i8_desc* d) {
  const char* who = "lce_hip_fully_connected_i8";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->inputs <= 0 || d->outputs <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d] -> %d outputs", who, (int)d->batch, (int)d->inputs,
                (int)d->outputs);
  if (d->activation < LCE_HIP_ACT_NONE || d->activation > LCE_HIP_ACT_RELU6)
    return fail(LCE_HIP_ERR_INVALID, "%s: unknown activation %d", who, (int)d->activation);
  if (lce_hip_status s = head_i8_quantization_check(who, "input", d->input_scale, d->input_zero_point)) return s;
  if (lce_hip_status s = head_i8_quantization_check(who, "output", d->output_scale, d->output_zero_point)) return s;
  if ((uint32_t)d->inputs > lce::kFcI8MaxK)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: %d inputs per output could overflow the int32 accumulator (255 x 128 x K must not exceed "
                "2^31 - 1: K <= %u)", who, (int)d->inputs, (unsigned)lce::kFcI8MaxK);
  // (the kernel numbers its 16 x 16 tiles in 32 bits)
  const uint64_t tiles = (((uint64_t)d->batch + lce::kFcI8Tile - 1) / lce::kFcI8Tile) * (((uint64_t)d->outputs + lce::kFcI8Tile - 1) / lce::kFcI8Tile);
  if (tiles >= (1ull << 31)) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: an output of more than 2^31 tiles of 16 x 16 is not supported", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_fully_connected_i8_prepare(const lce_hip_fc_i8_desc* d, const int8_t* weights_host, const int32_t* bias_host,
                                                  const float* weight_scales, int32_t n_scales, int32_t* table, int32_t* act_min,
                                                  int32_t* act_max) {
  const char* who = "lce_hip_fully_connected_i8_prepare";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!weights_host) return fail(LCE_HIP_ERR_INVALID, "%s: null weights", who);
  if (!weight_scales) return fail(LCE_HIP_ERR_INVALID, "%s: null weight scales", who);
  if (!table || !act_min || !act_max) return fail(LCE_HIP_ERR_INVALID, "%s: null result", who);
  // (the descriptor checks but the K limit, which the table states with the bias and a channel -- as the conv entry's prepare)
  lce_hip_fc_i8_desc small = *d;
  if (small.inputs > 1) small.inputs = 1;
  if (lce_hip_status s = lce_hip_fully_connected_i8_check(&small)) return s;
  if (lce_hip_status s = conv2d_i8_table(who, d->outputs, d->inputs, d->input_scale, d->input_zero_point, d->output_scale, weights_host,
                                         bias_host, weight_scales, n_scales, table))
    return s;
  quantized_activation_range(d->activation, d->output_scale, d->output_zero_point, act_min, act_max);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_fully_connected_i8(const lce_hip_fc_i8_desc* d, const int8_t* in_dev, const int8_t* weights_dev,
                                          const int32_t* table_dev, int8_t* out_dev, void* stream) {
  const char* who = "lce_hip_fully_connected_i8";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!weights_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null weights", who);
  if (!table_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null table", who);
  if (!out_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null output", who);
  if (lce_hip_status s = lce_hip_fully_connected_i8_check(d)) return s;
  const uint64_t M = (uint64_t)d->batch, K = (uint64_t)d->inputs, N = (uint64_t)d->outputs;
  const Span in(in_dev, M * K), weights(weights_dev, N * K), table(table_dev, 3 * N * 4), out(out_dev, M * N), none(nullptr, 0);
  if (meet(out.lo, out.hi, table.lo, table.hi)) return fail(LCE_HIP_ERR_INVALID, "%s: the output overlaps the table", who);
  if (lce_hip_status s = check_operand_ranges(who, in, weights, none, out, none, /*float_operands=*/false)) return s;
  if (table.lo % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: table_dev must be 4-byte aligned", who);
  if (lce_hip_status s = require_device()) return s;
  lce::FcI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.filter = weights_dev; a.table = table_dev; a.out = out_dev;
  lce::fc_i8_fill(a, d->batch, d->inputs, d->outputs);
  a.zo = d->output_zero_point;
  quantized_activation_range(d->activation, d->output_scale, d->output_zero_point, &a.act_min, &a.act_max);
  const int e = lce::launch_fully_connected_i8(a, lce::fc_i8_vec_rule(a), stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_mean_i8_check(const lce_hip_mean_i8_desc* d) {
  const char* who = "lce_hip_mean_i8";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (d->batch <= 0 || d->height <= 0 || d->width <= 0 || d->channels <= 0)
    return fail(LCE_HIP_ERR_INVALID, "%s: extents must be positive, got [%d, %d, %d, %d]", who, (int)d->batch, (int)d->height, (int)d->width,
                (int)d->channels);
  if (lce_hip_status s = head_i8_quantization_check(who, "input", d->input_scale, d->input_zero_point)) return s;
  if (lce_hip_status s = head_i8_quantization_check(who, "output", d->output_scale, d->output_zero_point)) return s;
  // (four factors below 2^31: compared by division)
  const uint64_t image = (uint64_t)d->height * (uint64_t)d->width;                  // < 2^62
  if (image > (1ull << 60) / (uint64_t)d->channels || image * (uint64_t)d->channels > (1ull << 60) / (uint64_t)d->batch)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: more than 2^60 elements are not supported", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_mean_i8_prepare(const lce_hip_mean_i8_desc* d, int32_t* multiplier, int32_t* exponent) {
  const char* who = "lce_hip_mean_i8_prepare";
  if (!multiplier || !exponent) return fail(LCE_HIP_ERR_INVALID, "%s: null result", who);
  return mean_i8_multiplier(who, d, multiplier, exponent);
}

lce_hip_status lce_hip_mean_i8(const lce_hip_mean_i8_desc* d, const int8_t* in_dev, int8_t* out_dev, void* stream) {
  const char* who = "lce_hip_mean_i8";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!out_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null output", who);
  int32_t m = 0, e = 0;
  if (lce_hip_status s = mean_i8_multiplier(who, d, &m, &e)) return s;
  const uint64_t n = (uint64_t)d->height * (uint64_t)d->width, C = (uint64_t)d->channels, B = (uint64_t)d->batch;
  const Span in(in_dev, B * n * C), out(out_dev, B * C);
  if (meet(in.lo, in.hi, out.lo, out.hi)) return fail(LCE_HIP_ERR_INVALID, "%s: the output overlaps the input", who);
  if (lce_hip_status s = require_device()) return s;
  lce::MeanI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.out = out_dev; a.batch = B; a.n = (uint32_t)n; a.C = (uint32_t)C;
  a.segs = (uint32_t)((C + lce::kMeanI8Channels - 1) / lce::kMeanI8Channels);
  a.zi = d->input_zero_point; a.zo = d->output_zero_point;
  a.mul = m; a.left = e > 0 ? e : 0; a.right = e > 0 ? 0 : -e;
  const int err = lce::launch_mean_i8(a, stream);
  if (err != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)err));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_softmax_i8_check(size_t rows, size_t cols, float input_scale, float beta, float output_scale,
                                        int32_t output_zero_point) {
  const char* who = "lce_hip_softmax_i8";
  if (rows == 0 || cols == 0) return fail(LCE_HIP_ERR_INVALID, "%s: rows and cols must be positive, got %zu x %zu", who, rows, cols);
  if (!std::isfinite(input_scale) || !(input_scale > 0.0f))
    return fail(LCE_HIP_ERR_INVALID, "%s: input_scale must be finite and positive, got %g", who, (double)input_scale);
  if (!std::isfinite(beta) || !(beta > 0.0f)) return fail(LCE_HIP_ERR_INVALID, "%s: beta must be finite and positive, got %g", who, (double)beta);
  if (lce_hip_status s = head_i8_quantization_check(who, "output", output_scale, output_zero_point)) return s;
  if (output_scale != 1.0f / 256.0f || output_zero_point != -128)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: the output quantization must be exactly (1/256, -128), got (%.9g, %d)", who,
                (double)output_scale, (int)output_zero_point);
  if ((uint64_t)cols >= (1ull << 31) || (uint64_t)rows > (1ull << 60) / (uint64_t)cols)
    return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: rows of 2^31 elements or more, or more than 2^60 elements, are not supported", who);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_softmax_i8(size_t rows, size_t cols, float input_scale, float beta, float output_scale, int32_t output_zero_point,
                                  const int8_t* in_dev, int8_t* out_dev, void* stream) {
  const char* who = "lce_hip_softmax_i8";
  if (!in_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null input", who);
  if (!out_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null output", who);
  if (lce_hip_status s = lce_hip_softmax_i8_check(rows, cols, input_scale, beta, output_scale, output_zero_point)) return s;
  const Span in(in_dev, (uint64_t)rows * cols), out(out_dev, (uint64_t)rows * cols);
  // in place is the one overlap that is safe: a lane writes only the elements it alone reads
  if (in.lo != out.lo && meet(in.lo, in.hi, out.lo, out.hi)) return fail(LCE_HIP_ERR_INVALID, "%s: the output partly overlaps the input", who);
  if (lce_hip_status s = require_device()) return s;
  lce::SoftmaxI8Args a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.out = out_dev; a.rows = rows; a.cols = (uint32_t)cols;
  a.sb = input_scale * beta;                     // one float32 multiply (this file is built with -ffp-contract=off)
  const int e = lce::launch_softmax_i8(a, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_quantize_f32_i8(size_t n, float scale, int32_t zero_point, const float* in_dev, int8_t* out_dev, void* stream) {
  const char* who = "lce_hip_quantize_f32_i8";
  if (lce_hip_status s = quant_check(who, n, scale, zero_point, in_dev, out_dev, in_dev, 4, 1)) return s;
  if (n == 0) return LCE_HIP_OK;
  if (lce_hip_status s = require_device()) return s;
  lce::QuantArgs a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.out = out_dev; a.n = n; a.scale = scale; a.zp = zero_point;
  const int e = lce::launch_quantize_f32_i8(a, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_dequantize_i8_f32(size_t n, float scale, int32_t zero_point, const int8_t* in_dev, float* out_dev, void* stream) {
  const char* who = "lce_hip_dequantize_i8_f32";
  if (lce_hip_status s = quant_check(who, n, scale, zero_point, in_dev, out_dev, out_dev, 1, 4)) return s;
  if (n == 0) return LCE_HIP_OK;
  if (lce_hip_status s = require_device()) return s;
  lce::QuantArgs a;
  memset(&a, 0, sizeof a);
  a.in = in_dev; a.out = out_dev; a.n = n; a.scale = scale; a.zp = zero_point;
  const int e = lce::launch_dequantize_i8_f32(a, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// int8 DEPTHWISE_CONV_2D (lce_kernels_depthwise_i8.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
lce_hip_depthwise_desc depthwise_i8_window(const lce_hip_depthwise_i8_desc* d) {
  return lce_hip_depthwise_desc{d->batch, d->in_height, d->in_width, d->channels_in, d->depth_multiplier, d->filter_height, d->filter_width,
                                d->stride_height, d->stride_width, d->padding, d->activation};
}

// What lce_hip_depthwise_conv2d_i8_check refuses, with `who`'s messages.
lce_hip_status depthwise_i8_desc_check(const char* who, const lce_hip_depthwise_i8_desc* d, int32_t* out_height, int32_t* out_width) {
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  const lce_hip_depthwise_desc w = depthwise_i8_window(d);
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = depthwise_desc_check(who, &w, &oh, &ow)) return s;
  if (lce_hip_status s = head_i8_quantization_check(who, "input", d->input_scale, d->input_zero_point)) return s;
  if (lce_hip_status s = head_i8_quantization_check(who, "output", d->output_scale, d->output_zero_point)) return s;
  if (out_height) *out_height = oh;
  if (out_width) *out_width = ow;
  return LCE_HIP_OK;
}

// The launch of lce_hip_depthwise_conv2d_i8 and of its forced form.  `path`: -1 the entry's own choice, 0 the row path, 1 the
// 16-byte path (refused where the operands do not qualify).  `took` (nullable) gets the path; with `launch` false nothing runs.
lce_hip_status depthwise_i8_run(const char* who, const lce_hip_depthwise_i8_desc* d, int32_t path, const int8_t* in_dev, const int8_t* filter_dev,
                                const int32_t* table_dev, int8_t* out_dev, int32_t* out_bits_dev, void* stream, int32_t* took, bool launch) {
  if (lce_hip_status s = check_pointers(who, d, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  if (!table_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null table", who);
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = depthwise_i8_desc_check(who, d, &oh, &ow)) return s;
  const uint64_t Cin = (uint64_t)d->channels_in, C = Cin * (uint64_t)d->depth_multiplier;
  const uint64_t pixels = (uint64_t)d->batch * oh * ow, wpr = (C + 31) / 32;
  const Span in(in_dev, (uint64_t)d->batch * d->in_height * d->in_width * Cin);
  const Span filter(filter_dev, (uint64_t)d->filter_height * d->filter_width * C), table(table_dev, 3 * C * 4);
  const Span out(out_dev, pixels * C), bits(out_bits_dev, pixels * wpr * 4);
  // (the table stands where the float entry has its bias)
  if (meet(out.lo, out.hi, table.lo, table.hi) || meet(bits.lo, bits.hi, table.lo, table.hi))
    return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the table", who);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, Span(nullptr, 0), out, bits, /*float_operands=*/false)) return s;
  if (table.lo % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: table_dev must be 4-byte aligned", who);
  bool vec = lce::window_vec_rule(d->depth_multiplier, C, 1, out_bits_dev != nullptr, in_dev, filter_dev, table_dev, out_dev);
  if (lce_hip_status s = take_path(who, path, &vec, "depth_multiplier 1, channels % 16 == 0 (% 32 with bits) and 16-byte aligned input, filter, "
                                   "table and output"))
    return s;
  if (took) *took = vec ? 1 : 0;
  if (!launch) return LCE_HIP_OK;
  if (lce_hip_status s = require_device()) return s;
  lce::DepthwiseI8Args a;
  memset(&a, 0, sizeof a);
  lce::PoolArgs& p = a.P;
  p.in = in_dev; p.out = out_dev; p.bits = (uint32_t*)out_bits_dev;
  a.filter = filter_dev; a.table = table_dev;
  a.zi = d->input_zero_point;
  a.channels_in = (uint32_t)Cin; a.div_multiplier = lce::make_fastdiv((uint32_t)d->depth_multiplier);
  window_fill(p, d->batch, d->in_height, d->in_width, d->filter_height, d->filter_width, d->stride_height, d->stride_width, oh, ow, C, 16, vec,
              /*stream_loads_rule=*/true);
  quantized_activation_range(d->activation, d->output_scale, d->output_zero_point, &p.qlo, &p.qhi);
  p.zero_point = d->output_zero_point;
  const int e = lce::launch_depthwise_i8(a, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_depthwise_conv2d_i8_check(const lce_hip_depthwise_i8_desc* d, int32_t* out_height, int32_t* out_width) {
  return depthwise_i8_desc_check("lce_hip_depthwise_conv2d_i8", d, out_height, out_width);
}

lce_hip_status lce_hip_depthwise_conv2d_i8_prepare(const lce_hip_depthwise_i8_desc* d, const int8_t* filter_host, const int32_t* bias_host,
                                                   const float* filter_scales, int32_t n_scales, int32_t* table, int32_t* act_min,
                                                   int32_t* act_max) {
  const char* who = "lce_hip_depthwise_conv2d_i8_prepare";
  if (!d) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (!filter_host) return fail(LCE_HIP_ERR_INVALID, "%s: null filter", who);
  if (!filter_scales) return fail(LCE_HIP_ERR_INVALID, "%s: null filter scales", who);
  if (!table || !act_min || !act_max) return fail(LCE_HIP_ERR_INVALID, "%s: null result", who);
  if (lce_hip_status s = depthwise_i8_desc_check(who, d, nullptr, nullptr)) return s;
  // an output element sums K = fh x fw products; the kernel subtracts zi itself and skips the padding, so nothing is folded
  const int64_t N = (int64_t)d->channels_in * d->depth_multiplier, K = (int64_t)d->filter_height * d->filter_width;       // both < 2^31
  if (lce_hip_status s = conv2d_i8_table(who, N, K, d->input_scale, d->input_zero_point, d->output_scale, /*filter_host=*/nullptr, bias_host,
                                         filter_scales, n_scales, table))
    return s;
  quantized_activation_range(d->activation, d->output_scale, d->output_zero_point, act_min, act_max);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_depthwise_conv2d_i8(const lce_hip_depthwise_i8_desc* d, const int8_t* in_dev, const int8_t* filter_dev,
                                           const int32_t* table_dev, int8_t* out_dev, int32_t* out_bits_dev, void* stream) {
  return depthwise_i8_run("lce_hip_depthwise_conv2d_i8", d, -1, in_dev, filter_dev, table_dev, out_dev, out_bits_dev, stream, nullptr, true);
}

lce_hip_status lce_hip_depthwise_conv2d_i8_path(const lce_hip_depthwise_i8_desc* d, const int8_t* in_dev, const int8_t* filter_dev,
                                                const int32_t* table_dev, const int8_t* out_dev, const int32_t* out_bits_dev, int32_t* path) {
  const char* who = "lce_hip_depthwise_conv2d_i8_path";
  if (!path) return fail(LCE_HIP_ERR_INVALID, "%s: null path", who);
  return depthwise_i8_run(who, d, -1, in_dev, filter_dev, table_dev, (int8_t*)out_dev, (int32_t*)out_bits_dev, nullptr, path, false);
}

lce_hip_status lce_hip_depthwise_conv2d_i8_forced(const lce_hip_depthwise_i8_desc* d, int32_t path, const int8_t* in_dev,
                                                  const int8_t* filter_dev, const int32_t* table_dev, int8_t* out_dev, int32_t* out_bits_dev,
                                                  void* stream) {
  const char* who = "lce_hip_depthwise_conv2d_i8_forced";
  if (path != 0 && path != 1) return fail(LCE_HIP_ERR_INVALID, "%s: unknown path %d", who, (int)path);
  return depthwise_i8_run(who, d, path, in_dev, filter_dev, table_dev, out_dev, out_bits_dev, stream, nullptr, true);
}

// ------------------------------------------------------------------------------------
// A transition's MAX_POOL_2D and DEPTHWISE_CONV_2D in one launch (lce_kernels_transition.h)
// ------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// What the two fused checks share once each entry's own check has accepted its descriptor: `pooled_h` x `pooled_w` are the pool's
// output extents, `dw` the depthwise window.  The pool must be of the entry's type, the depthwise convolution must read the
// pool's output, and only then is AVERAGE told apart as unsupported.
lce_hip_status pool_depthwise_join_check(const char* who, const lce_hip_pool2d_desc* pool, int32_t type, int32_t pooled_h, int32_t pooled_w,
                                         const lce_hip_depthwise_desc& dw) {
  if (pool->type != type)
    return fail(LCE_HIP_ERR_INVALID, "%s: the pool's type must be %s, got %d", who, type == LCE_HIP_I8 ? "int8" : "float32", (int)pool->type);
  if (dw.batch != pool->batch || dw.in_height != pooled_h || dw.in_width != pooled_w || dw.channels_in != pool->channels)
    return fail(LCE_HIP_ERR_INVALID, "%s: the depthwise input [%d, %d, %d, %d] is not the pool's output [%d, %d, %d, %d]", who, (int)dw.batch,
                (int)dw.in_height, (int)dw.in_width, (int)dw.channels_in, (int)pool->batch, (int)pooled_h, (int)pooled_w, (int)pool->channels);
  return LCE_HIP_OK;
}
lce_hip_status pool_depthwise_op_check(const char* who, const lce_hip_pool2d_desc* pool) {
  if (pool->op != LCE_HIP_POOL_MAX) return fail(LCE_HIP_ERR_UNSUPPORTED, "%s: only a MAX pool runs in the depthwise convolution's launch", who);
  return LCE_HIP_OK;
}

lce_hip_status pool_depthwise_f32_desc_check(const char* who, const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, int32_t* pooled_h,
                                             int32_t* pooled_w, int32_t* out_height, int32_t* out_width) {
  if (!pool || !dw) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (lce_hip_status s = lce_hip_pool2d_check(pool, pooled_h, pooled_w)) return s;
  if (lce_hip_status s = depthwise_desc_check(who, dw, out_height, out_width)) return s;
  if (lce_hip_status s = pool_depthwise_join_check(who, pool, LCE_HIP_F32, *pooled_h, *pooled_w, *dw)) return s;
  return pool_depthwise_op_check(who, pool);
}
lce_hip_status pool_depthwise_i8_desc_check(const char* who, const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, int32_t* pooled_h,
                                            int32_t* pooled_w, int32_t* out_height, int32_t* out_width) {
  if (!pool || !dw) return fail(LCE_HIP_ERR_INVALID, "%s: null desc", who);
  if (lce_hip_status s = lce_hip_pool2d_check(pool, pooled_h, pooled_w)) return s;
  if (lce_hip_status s = depthwise_i8_desc_check(who, dw, out_height, out_width)) return s;
  if (lce_hip_status s = pool_depthwise_join_check(who, pool, LCE_HIP_I8, *pooled_h, *pooled_w, depthwise_i8_window(dw))) return s;
  // (the pooled tensor is the pool's input requantized by nothing: TFLite's Prepare requires one scale and zero point of both)
  if (dw->input_scale != pool->scale || dw->input_zero_point != pool->zero_point)
    return fail(LCE_HIP_ERR_INVALID, "%s: the depthwise input's quantization (%g, %d) is not the pool's (%g, %d)", who, (double)dw->input_scale,
                (int)dw->input_zero_point, (double)pool->scale, (int)pool->zero_point);
  return pool_depthwise_op_check(who, pool);
}

// The geometry of both fused launches: the depthwise window on the pooled map into `p`, the pool in front into `q`.
void pool_depthwise_fill(lce::PoolArgs& p, lce::TransitionPool& q, const lce_hip_pool2d_desc* pool, int32_t pooled_h, int32_t pooled_w,
                         const lce_hip_depthwise_desc& dw, int32_t oh, int32_t ow, uint64_t C, uint64_t chunk, bool vec) {
  window_fill(p, dw.batch, pooled_h, pooled_w, dw.filter_height, dw.filter_width, dw.stride_height, dw.stride_width, oh, ow, C, chunk, vec,
              /*stream_loads_rule=*/false);
  lce::transition_pool_fill(q, pool->in_height, pool->in_width, pool->filter_height, pool->filter_width, pool->stride_height, pool->stride_width,
                            pooled_h, pooled_w);
  float_activation_range(pool->activation, &q.lo, &q.hi);
  if (pool->type == LCE_HIP_I8) quantized_activation_range(pool->activation, pool->scale, pool->zero_point, &q.qlo, &q.qhi);
}

// The launch of lce_hip_pool_depthwise_f32 and of its forced form (`path`, `took`, `launch`: as depthwise_i8_run's).
lce_hip_status pool_depthwise_f32_run(const char* who, const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, int32_t path,
                                      const float* in_dev, const float* filter_dev, const float* bias_dev, float* out_dev, int32_t* out_bits_dev,
                                      void* stream, int32_t* took, bool launch) {
  if (lce_hip_status s = check_pointers(who, pool, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  int32_t qh = 0, qw = 0, oh = 0, ow = 0;
  if (lce_hip_status s = pool_depthwise_f32_desc_check(who, pool, dw, &qh, &qw, &oh, &ow)) return s;
  const uint64_t Cin = (uint64_t)dw->channels_in, C = Cin * (uint64_t)dw->depth_multiplier;
  const uint64_t pixels = (uint64_t)dw->batch * oh * ow, wpr = (C + 31) / 32;
  const Span in(in_dev, (uint64_t)pool->batch * pool->in_height * pool->in_width * Cin * 4);
  const Span filter(filter_dev, (uint64_t)dw->filter_height * dw->filter_width * C * 4), bias(bias_dev, C * 4);
  const Span out(out_dev, pixels * C * 4), bits(out_bits_dev, pixels * wpr * 4);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, bias, out, bits, /*float_operands=*/true)) return s;
  lce::TransitionArgs a;
  memset(&a, 0, sizeof a);
  a.Q.fh = pool->filter_height; a.Q.fw = pool->filter_width; a.Q.sh = pool->stride_height; a.Q.sw = pool->stride_width;
  bool vec = lce::window_vec_rule(dw->depth_multiplier, C, 4, out_bits_dev != nullptr, in_dev, filter_dev, bias_dev, out_dev) &&
             lce::transition_vec_geometry(a.Q, dw->filter_height, dw->filter_width);
  if (lce_hip_status s = take_path(who, path, &vec, "depth_multiplier 1, channels % 4 == 0 (% 32 with bits), 16-byte aligned input, "
                                             "filter, bias and output, a pool of stride 1 and at most 2 x 2 and a depthwise filter of at most 3 x 3"))
    return s;
  if (took) *took = vec ? 1 : 0;
  if (!launch) return LCE_HIP_OK;
  if (lce_hip_status s = require_device()) return s;
  lce::PoolArgs& p = a.D.P;
  p.in = in_dev; p.out = out_dev; p.bits = (uint32_t*)out_bits_dev;
  a.D.filter = filter_dev; a.D.bias = bias_dev;
  a.D.channels_in = (uint32_t)Cin; a.D.div_multiplier = lce::make_fastdiv((uint32_t)dw->depth_multiplier);
  pool_depthwise_fill(p, a.Q, pool, qh, qw, *dw, oh, ow, C, 4, vec);
  float_activation_range(dw->activation, &p.lo, &p.hi);
  const int e = lce::launch_transition(a, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}

// The launch of lce_hip_pool_depthwise_i8 and of its forced form.
lce_hip_status pool_depthwise_i8_run(const char* who, const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, int32_t path,
                                     const int8_t* in_dev, const int8_t* filter_dev, const int32_t* table_dev, int8_t* out_dev, int32_t* out_bits_dev,
                                     void* stream, int32_t* took, bool launch) {
  if (lce_hip_status s = check_pointers(who, pool, in_dev, /*has_filter=*/true, filter_dev, out_dev, out_bits_dev)) return s;
  if (!table_dev) return fail(LCE_HIP_ERR_INVALID, "%s: null table", who);
  int32_t qh = 0, qw = 0, oh = 0, ow = 0;
  if (lce_hip_status s = pool_depthwise_i8_desc_check(who, pool, dw, &qh, &qw, &oh, &ow)) return s;
  const uint64_t Cin = (uint64_t)dw->channels_in, C = Cin * (uint64_t)dw->depth_multiplier;
  const uint64_t pixels = (uint64_t)dw->batch * oh * ow, wpr = (C + 31) / 32;
  const Span in(in_dev, (uint64_t)pool->batch * pool->in_height * pool->in_width * Cin);
  const Span filter(filter_dev, (uint64_t)dw->filter_height * dw->filter_width * C), table(table_dev, 3 * C * 4);
  const Span out(out_dev, pixels * C), bits(out_bits_dev, pixels * wpr * 4);
  if (meet(out.lo, out.hi, table.lo, table.hi) || meet(bits.lo, bits.hi, table.lo, table.hi))
    return fail(LCE_HIP_ERR_INVALID, "%s: an output overlaps the table", who);
  if (lce_hip_status s = check_operand_ranges(who, in, filter, Span(nullptr, 0), out, bits, /*float_operands=*/false)) return s;
  if (table.lo % 4 != 0) return fail(LCE_HIP_ERR_INVALID, "%s: table_dev must be 4-byte aligned", who);
  lce::TransitionI8Args a;
  memset(&a, 0, sizeof a);
  a.Q.fh = pool->filter_height; a.Q.fw = pool->filter_width; a.Q.sh = pool->stride_height; a.Q.sw = pool->stride_width;
  bool vec = lce::window_vec_rule(dw->depth_multiplier, C, 1, out_bits_dev != nullptr, in_dev, filter_dev, table_dev, out_dev) &&
             lce::transition_vec_geometry(a.Q, dw->filter_height, dw->filter_width);
  if (lce_hip_status s = take_path(who, path, &vec, "depth_multiplier 1, channels % 16 == 0 (% 32 with bits), 16-byte aligned input, "
                                             "filter, table and output, a pool of stride 1 and at most 2 x 2 and a depthwise filter of at most 3 x 3"))
    return s;
  if (took) *took = vec ? 1 : 0;
  if (!launch) return LCE_HIP_OK;
  if (lce_hip_status s = require_device()) return s;
  lce::PoolArgs& p = a.D.P;
  p.in = in_dev; p.out = out_dev; p.bits = (uint32_t*)out_bits_dev;
  a.D.filter = filter_dev; a.D.table = table_dev;
  a.D.zi = dw->input_zero_point;
  a.D.channels_in = (uint32_t)Cin; a.D.div_multiplier = lce::make_fastdiv((uint32_t)dw->depth_multiplier);
  pool_depthwise_fill(p, a.Q, pool, qh, qw, depthwise_i8_window(dw), oh, ow, C, 16, vec);
  quantized_activation_range(dw->activation, dw->output_scale, dw->output_zero_point, &p.qlo, &p.qhi);
  p.zero_point = dw->output_zero_point;
  const int e = lce::launch_transition_i8(a, vec, stream);
  if (e != hipSuccess) return fail(LCE_HIP_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString((hipError_t)e));
  return LCE_HIP_OK;
}
}  // namespace
extern "C" {

lce_hip_status lce_hip_pool_depthwise_f32_check(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, int32_t* out_height,
                                                int32_t* out_width) {
  int32_t qh = 0, qw = 0, oh = 0, ow = 0;
  if (lce_hip_status s = pool_depthwise_f32_desc_check("lce_hip_pool_depthwise_f32", pool, dw, &qh, &qw, &oh, &ow)) return s;
  if (out_height) *out_height = oh;
  if (out_width) *out_width = ow;
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_pool_depthwise_f32(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, const float* in_dev,
                                          const float* filter_dev, const float* bias_dev, float* out_dev, int32_t* out_bits_dev, void* stream) {
  return pool_depthwise_f32_run("lce_hip_pool_depthwise_f32", pool, dw, -1, in_dev, filter_dev, bias_dev, out_dev, out_bits_dev, stream, nullptr, true);
}
lce_hip_status lce_hip_pool_depthwise_f32_path(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, const float* in_dev,
                                               const float* filter_dev, const float* bias_dev, const float* out_dev, const int32_t* out_bits_dev,
                                               int32_t* path) {
  const char* who = "lce_hip_pool_depthwise_f32_path";
  if (!path) return fail(LCE_HIP_ERR_INVALID, "%s: null path", who);
  return pool_depthwise_f32_run(who, pool, dw, -1, in_dev, filter_dev, bias_dev, (float*)out_dev, (int32_t*)out_bits_dev, nullptr, path, false);
}
lce_hip_status lce_hip_pool_depthwise_f32_forced(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, int32_t path, const float* in_dev,
                                                 const float* filter_dev, const float* bias_dev, float* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_pool_depthwise_f32_forced";
  if (path != 0 && path != 1) return fail(LCE_HIP_ERR_INVALID, "%s: unknown path %d", who, (int)path);
  return pool_depthwise_f32_run(who, pool, dw, path, in_dev, filter_dev, bias_dev, out_dev, out_bits_dev, stream, nullptr, true);
}

lce_hip_status lce_hip_pool_depthwise_i8_check(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, int32_t* out_height,
                                               int32_t* out_width) {
  int32_t qh = 0, qw = 0, oh = 0, ow = 0;
  if (lce_hip_status s = pool_depthwise_i8_desc_check("lce_hip_pool_depthwise_i8", pool, dw, &qh, &qw, &oh, &ow)) return s;
  if (out_height) *out_height = oh;
  if (out_width) *out_width = ow;
  return LCE_HIP_OK;
}
lce_hip_status lce_hip_pool_depthwise_i8(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, const int8_t* in_dev,
                                         const int8_t* filter_dev, const int32_t* table_dev, int8_t* out_dev, int32_t* out_bits_dev, void* stream) {
  return pool_depthwise_i8_run("lce_hip_pool_depthwise_i8", pool, dw, -1, in_dev, filter_dev, table_dev, out_dev, out_bits_dev, stream, nullptr, true);
}
lce_hip_status lce_hip_pool_depthwise_i8_path(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, const int8_t* in_dev,
                                              const int8_t* filter_dev, const int32_t* table_dev, const int8_t* out_dev, const int32_t* out_bits_dev,
                                              int32_t* path) {
  const char* who = "lce_hip_pool_depthwise_i8_path";
  if (!path) return fail(LCE_HIP_ERR_INVALID, "%s: null path", who);
  return pool_depthwise_i8_run(who, pool, dw, -1, in_dev, filter_dev, table_dev, (int8_t*)out_dev, (int32_t*)out_bits_dev, nullptr, path, false);
}
lce_hip_status lce_hip_pool_depthwise_i8_forced(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, int32_t path, const int8_t* in_dev,
                                                const int8_t* filter_dev, const int32_t* table_dev, int8_t* out_dev, int32_t* out_bits_dev, void* stream) {
  const char* who = "lce_hip_pool_depthwise_i8_forced";
  if (path != 0 && path != 1) return fail(LCE_HIP_ERR_INVALID, "%s: unknown path %d", who, (int)path);
  return pool_depthwise_i8_run(who, pool, dw, path, in_dev, filter_dev, table_dev, out_dev, out_bits_dev, stream, nullptr, true);
}

// ------------------------------------------------------------------------------------
// LceBconv2d
// ------------------------------------------------------------------------------------
lce_hip_status lce_hip_bconv2d_plan_create(const lce_hip_bconv2d_desc* desc, lce_hip_bconv2d_plan** plan) {
  if (!desc || !plan) return fail(LCE_HIP_ERR_INVALID, "lce_hip_bconv2d_plan_create: null argument");
  lce_hip_bconv2d_plan* p = new lce_hip_bconv2d_plan();
  p->host.d = *desc;
  const std::string err = lce::validate_and_infer(p->host);
  if (!err.empty()) {
    delete p;
    *plan = nullptr;
    return fail(LCE_HIP_ERR_INVALID, "%s", err.c_str());
  }
  *plan = p;
  return LCE_HIP_OK;
}

void lce_hip_bconv2d_plan_destroy(lce_hip_bconv2d_plan* plan) { delete plan; }

lce_hip_status lce_hip_bconv2d_plan_output_shape(const lce_hip_bconv2d_plan* plan, int32_t dims[4]) {
  if (!plan || !dims) return fail(LCE_HIP_ERR_INVALID, "plan_output_shape: null argument");
  const lce::HostPlan& h = plan->host;
  dims[0] = h.d.batch;
  dims[1] = h.out_h;
  dims[2] = h.out_w;
  dims[3] = h.d.dst_type == LCE_HIP_BITPACKED ? h.wout : h.d.channels_out;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bconv2d_plan_padding(const lce_hip_bconv2d_plan* plan, int32_t* pad_h, int32_t* pad_w) {
  if (!plan || !pad_h || !pad_w) return fail(LCE_HIP_ERR_INVALID, "plan_padding: null argument");
  *pad_h = plan->host.pad_h;
  *pad_w = plan->host.pad_w;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bconv2d_plan_set_weights(lce_hip_bconv2d_plan* plan, const int32_t* filter,
                                                const float* post_mul, const float* post_bias,
                                                const int32_t* thresholds) {
  if (!plan || !filter) return fail(LCE_HIP_ERR_INVALID, "plan_set_weights: null plan or filter");
  const bool bp = plan->host.d.dst_type == LCE_HIP_BITPACKED;
  if (bp && !thresholds) return fail(LCE_HIP_ERR_INVALID, "plan_set_weights: bitpacked output needs thresholds");
  if (!bp && (!post_mul || !post_bias))
    return fail(LCE_HIP_ERR_INVALID, "plan_set_weights: float/int8 output needs post_activation_multiplier and _bias");
  lce::fold_parameters(plan->host, filter, post_mul, post_bias, thresholds);
  plan->device_current = false;
  plan->selected_for_pixels = -1;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bconv2d_plan_folded(const lce_hip_bconv2d_plan* plan, float* mul, float* bias,
                                           int32_t* clamp_min, int32_t* clamp_max) {
  if (!plan) return fail(LCE_HIP_ERR_INVALID, "plan_folded: null plan");
  const lce::HostPlan& h = plan->host;
  if (!h.have_weights || h.d.dst_type == LCE_HIP_BITPACKED)
    return fail(LCE_HIP_ERR_INVALID, "plan_folded: no folded float transform on this plan");
  if (mul) memcpy(mul, h.mul.data(), h.mul.size() * sizeof(float));
  if (bias) memcpy(bias, h.bias.data(), h.bias.size() * sizeof(float));
  if (clamp_min) *clamp_min = h.clamp_min;
  if (clamp_max) *clamp_max = h.clamp_max;
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bconv2d_plan_set_option(lce_hip_bconv2d_plan* plan, const char* key, const char* value) {
  if (!plan || !key || !value) return fail(LCE_HIP_ERR_INVALID, "plan_set_option: null argument");
  unsigned stale = 0;
  const std::string err = lce::set_plan_option(plan->host, key, value, &stale);
  if (!err.empty()) return fail(LCE_HIP_ERR_INVALID, "%s", err.c_str());
  if (stale & lce::kStaleSelection) plan->selected_for_pixels = -1;
  if (stale & lce::kStaleUpload) plan->device_current = false;
  if (stale & lce::kStalePacked) plan->host.packed.clear();
  if (stale & lce::kStaleWeightImage) plan->host.wq.clear();
  return LCE_HIP_OK;
}

// (The kernel choice does not depend on whether a call asks for the second output: one plan, one selection, both kinds of call.)
const char* lce_hip_bconv2d_plan_kernel_name(lce_hip_bconv2d_plan* plan);
const char* lce_hip_bconv2d_plan_kernel_name_dual(lce_hip_bconv2d_plan* plan) { return lce_hip_bconv2d_plan_kernel_name(plan); }

const char* lce_hip_bconv2d_plan_kernel_name(lce_hip_bconv2d_plan* plan) {
  if (!plan) return "";
  const int chunk = lce::max_batch_per_launch(plan->host);
  if (ensure_selected(plan, chunk) != LCE_HIP_OK) return "";
  return plan->host.kernel_name.c_str();
}

lce_hip_status lce_hip_bconv2d_plan_int8_epilogue(lce_hip_bconv2d_plan* plan, int32_t* one_instruction_forms, int32_t* adjusted_channels) {
  if (!plan) return fail(LCE_HIP_ERR_INVALID, "plan_int8_epilogue: null plan");
  if (one_instruction_forms) *one_instruction_forms = 0;
  if (adjusted_channels) *adjusted_channels = 0;
  const lce::HostPlan& h = plan->host;
  if (h.d.dst_type != LCE_HIP_I8 || !h.have_weights) return LCE_HIP_OK;
  if (lce_hip_status s = ensure_selected(plan, lce::max_batch_per_launch(h))) return s;
  const bool forms = lce::int8_one_instruction_forms(h);
  if (one_instruction_forms) *one_instruction_forms = forms ? 1 : 0;
  if (adjusted_channels) *adjusted_channels = forms ? h.int8_bias_adjusted : 0;
  return LCE_HIP_OK;
}

// Images [first, first + count) of the plan's batch; input_dev / output_dev / sign_dev point at image 0.
// sign_dev (float output only, may be null): the LceQuantize of the output, written by the same epilogue
// when the kernel variant can do it, otherwise by a bitpack launch behind it.
static lce_hip_status run_images(lce_hip_bconv2d_plan* plan, const int32_t* input_dev, void* output_dev,
                                 int32_t* sign_dev, int first, int count, hipStream_t st) {
  lce::HostPlan& h = plan->host;
  const int chunk = lce::max_batch_per_launch(h);
  if (lce_hip_status s = check_device(plan)) return s;          // binds the plan to the current device on its first run ...
  if (!h.cus_forced && plan->host.num_cus != device_compute_units(plan->device) && device_compute_units(plan->device) > 0)
    plan->selected_for_pixels = -1;                              // ... whose size the streaming kernel's grid follows
  if (lce_hip_status s = ensure_selected(plan, chunk)) return s;
  if (lce_hip_status s = ensure_uploaded(plan)) return s;

  const size_t in_img_words = (size_t)h.d.in_height * h.d.in_width * h.cw;
  const size_t out_row = h.d.dst_type == LCE_HIP_BITPACKED ? (size_t)h.wout : (size_t)h.d.channels_out;
  const size_t out_img_bytes = (size_t)h.out_h * h.out_w * out_row * out_elem_bytes(h.d.dst_type);
  const size_t sign_img_words = (size_t)h.out_h * h.out_w * h.wout;

  for (int b0 = first; b0 < first + count; b0 += chunk) {
    const int nb = std::min(chunk, first + count - b0);
    ConvArgs A = lce::make_conv_args(h, nb);
    const uint32_t* in = (const uint32_t*)input_dev + (size_t)b0 * in_img_words;
    void* out = (char*)output_dev + (size_t)b0 * out_img_bytes;
    uint32_t* sgn = sign_dev ? (uint32_t*)sign_dev + (size_t)b0 * sign_img_words : nullptr;
    bool sign_fused = false;
    if (h.use_mfma && h.use_pointwise && ((uintptr_t)out & 15) == 0) {
      // 1x1 streaming kernel: waves walk 32-pixel tiles of the launch's pixel matrix
      if (lce_hip_status s = mfma_selftest_once(plan->device, 0)) return s;
      lce::pointwise_fn fn = lce::lookup_pointwise(h.d.dst_type, h.pw_nc, h.pw_nj, h.d.stride_height != 1 || h.d.stride_width != 1, h.int8_floor_ok);
      if (!fn) return fail(LCE_HIP_ERR_UNSUPPORTED, "bconv2d_run: no kernel instance for %s", h.kernel_name.c_str());
      const lce::PwArgs P = lce::make_pw_args(h, nb);
      // k tiles per wave: enough blocks (>= 12 per CU when the launch has them) for the dispatcher to even
      // out the CUs, few enough that a wave's register-resident filter bank is loaded once per several tiles
      const int pw_k = h.pw_tiles_pref > 0 ? h.pw_tiles_pref : std::max(1, std::min(8, P.tiles / (4 * 256 * 12)));
      const unsigned gx = (unsigned)(((int64_t)P.tiles + 4 * pw_k - 1) / (4 * pw_k));
      const dim3 grid(gx, (unsigned)(h.d.channels_out / (32 * h.pw_nj)));
      hipLaunchKernelGGL(fn, grid, dim3(256), (size_t)(4 * h.pw_nj * 4096), st, P, in, plan->d_wq.ptr, plan->d_mul.ptr,
                         plan->d_bias.ptr, plan->d_thrq.ptr, out, sgn);
      LCE_HIP_TRY(hipGetLastError());
      sign_fused = true;   // (also when there is none to write)
    } else if (h.use_mfma && h.use_wstream) {
      // weight-streaming kernel: a block per (group of images, part of its pixel blocks), two resident per CU
      if (lce_hip_status s = mfma_selftest_once(plan->device, 2)) return s;
      const lce::WsArgs G = lce::make_ws_args(h, nb);
      const bool with_sign = sgn != nullptr && h.d.dst_type != LCE_HIP_BITPACKED;
      lce::wstream_fn fn = lce::lookup_wstream(h.d.dst_type, lce::stream_chunks(h.d), h.ws_nb, with_sign, h.int8_floor_ok);
      if (!fn) return fail(LCE_HIP_ERR_UNSUPPORTED, "bconv2d_run: no kernel instance for %s", h.kernel_name.c_str());
      const size_t lds = (size_t)lce::wstream_lds_bytes(h);
      if (lds > 64 * 1024 && plan->lds_opt_in != (void*)fn) {
        LCE_HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        plan->lds_opt_in = (void*)fn;
      }
      const dim3 grid((unsigned)(G.GROUPS * G.PARTS), (unsigned)h.ws_ny);
      hipLaunchKernelGGL(fn, grid, dim3(256), lds, st, G, (const uint8_t*)in, plan->d_wq.ptr, plan->d_mul.ptr,
                         plan->d_bias.ptr, plan->d_thrq.ptr, plan->d_sched.ptr, out, with_sign ? sgn : nullptr);
      LCE_HIP_TRY(hipGetLastError());
      sign_fused = true;   // (also when there is none to write)
    } else if (h.use_mfma && h.use_stream) {
      // weight-stationary streaming kernel: one persistent block per CU walks its run of segments
      if (lce_hip_status s = mfma_selftest_once(plan->device, 1)) return s;
      const lce::StreamArgs G = lce::make_stream_args(h, nb);
      const bool with_sign = sgn != nullptr && h.d.dst_type != LCE_HIP_BITPACKED;
      lce::stream_fn fn = lce::lookup_stream(h.d.dst_type, lce::stream_chunks(h.d), lce::stream_fast(G), lce::stream_clamps(G), with_sign, G.NSTRIP > 1, h.int8_floor_ok);
      if (!fn) return fail(LCE_HIP_ERR_UNSUPPORTED, "bconv2d_run: no kernel instance for %s", h.kernel_name.c_str());
      const size_t lds = (size_t)lce::stream_lds_bytes(h);
      if (lds > 64 * 1024 && plan->lds_opt_in != (void*)fn) {
        LCE_HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        plan->lds_opt_in = (void*)fn;
      }
      const dim3 grid((unsigned)G.GX, (unsigned)h.st_ny);
      hipLaunchKernelGGL(fn, grid, dim3(256), lds, st, G, (const uint8_t*)in, plan->d_wq.ptr, plan->d_mul.ptr,
                         plan->d_bias.ptr, plan->d_thrq.ptr, plan->d_sched.ptr, out, with_sign ? sgn : nullptr);
      LCE_HIP_TRY(hipGetLastError());
      sign_fused = true;   // (also when there is none to write)
    } else if (h.use_mfma) {
      mfma_fn fn = lce::lookup_mfma(h.d.dst_type, h.mfma.bm(), h.mfma.bn(), h.zero_pad_mode == lce::kZeroPadCorrection,
                             h.use_direct, h.use_direct && h.tile_tx > 0);
      if (!fn) return fail(LCE_HIP_ERR_UNSUPPORTED, "bconv2d_run: no kernel instance for %s", h.kernel_name.c_str());
      const lce::MfmaArgs G = lce::make_mfma_args(h, nb);
      const int bm = h.mfma.bm(), bn = h.mfma.bn();
      // the joint-transpose float epilogue is the one that can also emit the sign words
      sign_fused = sgn && (h.d.dst_type == LCE_HIP_I8 ? G.i8_wide != 0 : G.f32_wide != 0) &&
                   h.zero_pad_mode != lce::kZeroPadCorrection && ((uintptr_t)out & 15) == 0;
      uint32_t* ksgn = sign_fused ? sgn : nullptr;
      if (h.use_direct) {
        // no workspace: every block expands its own input halo into LDS
        const size_t lds = (size_t)h.mfma.direct_lds_bytes(h.halo_bytes);
        if (lds > 64 * 1024 && plan->lds_opt_in != (void*)fn) {
          LCE_HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
          plan->lds_opt_in = (void*)fn;
        }
        const dim3 grid((unsigned)(h.ipt > 1 ? (nb + h.ipt - 1) / h.ipt : (int64_t)nb * h.tpi), (unsigned)(h.npad / bn));
        hipLaunchKernelGGL(fn, grid, dim3(h.mfma.threads()), lds, st, A, G, (const uint8_t*)in, plan->d_wq.ptr,
                           plan->d_mul.ptr, plan->d_bias.ptr, plan->d_thrq.ptr, plan->d_zpc.ptr, out, ksgn);
        LCE_HIP_TRY(hipGetLastError());
      } else {
        const size_t ws = lce::mfma_workspace_bytes(h, nb);
        // While `st` is being captured into a graph the cross-stream ordering is left to the capture's own stream order:
        // an event recorded inside a capture belongs to the graph and must not be waited on or synchronised from outside.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        const bool capturing = cap != hipStreamCaptureStatusNone;
        if (capturing && plan->workspace_bytes < ws)
          return fail(LCE_HIP_ERR_INVALID, "bconv2d_run: the FP4 workspace must exist before a stream capture (run the plan once first)");
        if (!capturing && plan->ws_used && plan->ws_stream != st) LCE_HIP_TRY(hipStreamWaitEvent(st, plan->ws_done, 0));
        if (plan->workspace_bytes < ws) {
          // a larger workspace: the old one may still be read by a run in flight on another stream
          if (plan->ws_used) LCE_HIP_TRY(hipEventSynchronize(plan->ws_done));
          if (plan->workspace) (void)hipFree(plan->workspace);
          plan->workspace = nullptr;
          plan->workspace_bytes = 0;
          LCE_HIP_TRY(hipMalloc(&plan->workspace, ws + 256));
          plan->workspace_bytes = ws;
        }
        const uint64_t chunks = (uint64_t)G.NPIX * (uint64_t)((G.CPW + 3) / 4);  // threads of expand_fp4
        if (h.phase != 2) {
          LCE_HIP_TRY((hipError_t)lce::launch_expand_fp4(lce::stream_grid((chunks + 63) / 64), (void*)st, in, plan->workspace, G, chunks));
        }
        if (h.phase != 1) {
          const dim3 grid((unsigned)((A.M + bm - 1) / bm), (unsigned)(h.npad / bn));
          hipLaunchKernelGGL(fn, grid, dim3(h.mfma.threads()), (size_t)h.mfma.lds_bytes(), st, A, G,
                             (const uint8_t*)plan->workspace, plan->d_wq.ptr, plan->d_mul.ptr, plan->d_bias.ptr,
                             plan->d_thrq.ptr, plan->d_zpc.ptr, out, ksgn);
          LCE_HIP_TRY(hipGetLastError());
        } else {
          sign_fused = true;   // profiling mode "expand only": nothing to quantize
        }
        if (!capturing) {
          if (!plan->ws_done) LCE_HIP_TRY(hipEventCreateWithFlags(&plan->ws_done, hipEventDisableTiming));
          LCE_HIP_TRY(hipEventRecord(plan->ws_done, st));
          plan->ws_stream = st;
          plan->ws_used = true;
        }
      }
    } else if (h.use_tiled) {
      tiled_fn fn = lce::lookup_tiled(h.d.dst_type, h.tile.tm, h.tile.tn, h.ch);
      if (!fn) return fail(LCE_HIP_ERR_UNSUPPORTED, "bconv2d_run: no kernel instance for %s", h.kernel_name.c_str());
      const int64_t tasks = (int64_t)A.PT * A.NT;
      const int wpb = 4;
      const unsigned grid = (unsigned)((tasks + wpb - 1) / wpb);
      hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * wpb), 0, st, A, in, plan->d_packed.ptr,
                         plan->d_mul.ptr, plan->d_bias.ptr, plan->d_thr.ptr, plan->d_oobc.ptr,
                         plan->d_zpc.ptr, out);
      LCE_HIP_TRY(hipGetLastError());
    } else {
      general_fn fn = lce::lookup_general(h.d.dst_type);
      const unsigned gx = (unsigned)((A.M + 255) / 256);
      const unsigned gy = (unsigned)((h.d.channels_out + 31) / 32);
      hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(256), 0, st, A, in, plan->d_filter.ptr,
                         plan->d_mul.ptr, plan->d_bias.ptr, plan->d_thr.ptr, plan->d_zpc.ptr, out);
      LCE_HIP_TRY(hipGetLastError());
    }
    if (sgn && !sign_fused) {
      // this kernel variant has no second output: LceQuantize as its own launch on the same stream
      const bool i8 = h.d.dst_type == LCE_HIP_I8;
      if (lce_hip_status s = lce_hip_bitpack(i8 ? LCE_HIP_I8 : LCE_HIP_F32, out, (size_t)nb * h.out_h * h.out_w,
                                             (size_t)h.d.channels_out, i8 ? h.d.out_zero_point : 0, (int32_t*)sgn, (void*)st))
        return s;
    }
  }
  return LCE_HIP_OK;
}

static lce_hip_status run_checks(lce_hip_bconv2d_plan* plan, const void* input, const void* output, const char* who) {
  if (!plan) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  if (!plan->host.have_weights) return fail(LCE_HIP_ERR_INVALID, "%s: plan_set_weights was not called", who);
  if (plan->host.d.batch == 0) return LCE_HIP_OK;   // empty batch: tensors may legitimately be null
  if (!input || !output) return fail(LCE_HIP_ERR_INVALID, "%s: null argument", who);
  return require_device();
}

lce_hip_status lce_hip_bconv2d_run(lce_hip_bconv2d_plan* plan, const int32_t* input_dev, void* output_dev, void* stream) {
  if (lce_hip_status s = run_checks(plan, input_dev, output_dev, "bconv2d_run")) return s;
  if (plan->host.d.batch == 0) return LCE_HIP_OK;
  return run_images(plan, input_dev, output_dev, nullptr, 0, plan->host.d.batch, (hipStream_t)stream);
}

lce_hip_status lce_hip_bconv2d_run_dual(lce_hip_bconv2d_plan* plan, const int32_t* input_dev, void* output_dev,
                                        int32_t* output_bits_dev, void* stream) {
  if (lce_hip_status s = run_checks(plan, input_dev, output_dev, "bconv2d_run_dual")) return s;
  if (plan->host.d.dst_type == LCE_HIP_BITPACKED)
    return fail(LCE_HIP_ERR_INVALID, "bconv2d_run_dual: the plan's output type must be float32 or int8 (a bitpacked-output "
                "plan already writes bits)");
  if (plan->host.d.batch == 0) return LCE_HIP_OK;
  if (!output_bits_dev) return fail(LCE_HIP_ERR_INVALID, "bconv2d_run_dual: null argument");
  if (lce_hip_status s = check_device(plan)) return s;
  return run_images(plan, input_dev, output_dev, output_bits_dev, 0, plan->host.d.batch, (hipStream_t)stream);
}

int lce_hip_bconv2d_plan_device(const lce_hip_bconv2d_plan* plan) { return plan ? plan->device : -1; }

// Host tensors (the TFLite interpreter's arena).  The batch is cut into slices that flow through three
// streams -- H2D | kernel | D2H -- so the copies of neighbouring slices overlap the compute of the one in
// between.  The copies are truly asynchronous only from page-locked memory: a host that owns long-lived
// buffers (an arena) registers them once with lce_hip_host_register; with pageable memory the runtime
// stages each copy and the slices still pipeline, just less tightly.
lce_hip_status lce_hip_bconv2d_run_host(lce_hip_bconv2d_plan* plan, const int32_t* input_host, void* output_host) {
  if (lce_hip_status s = run_checks(plan, input_host, output_host, "bconv2d_run_host")) return s;
  const lce::HostPlan& h = plan->host;
  if (h.d.batch == 0) return LCE_HIP_OK;   // empty batch
  if (lce_hip_status s = check_device(plan)) return s;
  const size_t in_img = (size_t)h.d.in_height * h.d.in_width * h.cw * 4;
  const size_t out_row = h.d.dst_type == LCE_HIP_BITPACKED ? (size_t)h.wout : (size_t)h.d.channels_out;
  const size_t out_img = (size_t)h.out_h * h.out_w * out_row * out_elem_bytes(h.d.dst_type);
  const size_t in_bytes = in_img * h.d.batch, out_bytes = out_img * h.d.batch;
  if (plan->stage_in_bytes < in_bytes) {
    if (plan->stage_in) (void)hipFree(plan->stage_in);
    plan->stage_in = nullptr;
    plan->stage_in_bytes = 0;
    LCE_HIP_TRY(hipMalloc(&plan->stage_in, in_bytes));
    plan->stage_in_bytes = in_bytes;
  }
  if (plan->stage_out_bytes < out_bytes) {
    if (plan->stage_out) (void)hipFree(plan->stage_out);
    plan->stage_out = nullptr;
    plan->stage_out_bytes = 0;
    LCE_HIP_TRY(hipMalloc(&plan->stage_out, out_bytes));
    plan->stage_out_bytes = out_bytes;
  }
  // slices of >= ~8 MiB of traffic each, at most 8 of them
  const size_t per_image = in_img + out_img;
  int slices = (int)std::min<size_t>(8, std::max<size_t>(1, (per_image * h.d.batch) / (8u << 20)));
  slices = std::min(slices, h.d.batch);
  if (!plan->s_h2d) {
    LCE_HIP_TRY(hipStreamCreateWithFlags(&plan->s_h2d, hipStreamNonBlocking));
    LCE_HIP_TRY(hipStreamCreateWithFlags(&plan->s_run, hipStreamNonBlocking));
    LCE_HIP_TRY(hipStreamCreateWithFlags(&plan->s_d2h, hipStreamNonBlocking));
  }
  while ((int)plan->ev_in.size() < slices) {
    hipEvent_t a, b;
    LCE_HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming));
    LCE_HIP_TRY(hipEventCreateWithFlags(&b, hipEventDisableTiming));
    plan->ev_in.push_back(a);
    plan->ev_run.push_back(b);
  }
  // on a failure mid-pipeline the copies already queued still read / write the caller's buffers: wait for them before
  // reporting it
  auto drain_and = [&](lce_hip_status s) {
    const std::string keep = g_last_error;
    (void)hipStreamSynchronize(plan->s_h2d);
    (void)hipStreamSynchronize(plan->s_run);
    (void)hipStreamSynchronize(plan->s_d2h);
    (void)hipGetLastError();
    g_last_error = keep;
    return s;
  };
#define LCE_HIP_TRY_DRAIN(expr)                                                                            \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) return drain_and(fail(LCE_HIP_ERR_RUNTIME, "%s failed: %s", #expr, hipGetErrorString(e_))); \
  } while (0)
  const int base = h.d.batch / slices, extra = h.d.batch % slices;
  int first = 0;
  for (int k = 0; k < slices; ++k) {
    const int count = base + (k < extra ? 1 : 0);
    LCE_HIP_TRY_DRAIN(hipMemcpyAsync((char*)plan->stage_in + first * in_img, (const char*)input_host + first * in_img,
                               count * in_img, hipMemcpyHostToDevice, plan->s_h2d));
    LCE_HIP_TRY_DRAIN(hipEventRecord(plan->ev_in[k], plan->s_h2d));
    LCE_HIP_TRY_DRAIN(hipStreamWaitEvent(plan->s_run, plan->ev_in[k], 0));
    if (lce_hip_status s = run_images(plan, (const int32_t*)plan->stage_in, plan->stage_out, nullptr, first, count, plan->s_run))
      return drain_and(s);
    LCE_HIP_TRY_DRAIN(hipEventRecord(plan->ev_run[k], plan->s_run));
    LCE_HIP_TRY_DRAIN(hipStreamWaitEvent(plan->s_d2h, plan->ev_run[k], 0));
    LCE_HIP_TRY_DRAIN(hipMemcpyAsync((char*)output_host + first * out_img, (const char*)plan->stage_out + first * out_img,
                               count * out_img, hipMemcpyDeviceToHost, plan->s_d2h));
    first += count;
  }
#undef LCE_HIP_TRY_DRAIN
  LCE_HIP_TRY(hipStreamSynchronize(plan->s_d2h));   // the last slice's copy is the last thing queued anywhere
  LCE_HIP_TRY(hipStreamSynchronize(plan->s_run));
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// LceBMaxPool2d
// ------------------------------------------------------------------------------------
static int pool_out(int padding, int in, int filter, int stride) {
  if (stride == 0) return 0;
  // (in 64 bits: the operands may come straight from an untrusted file, and in + stride may pass 2^31)
  const int64_t n = padding == LCE_HIP_PADDING_SAME ? ((int64_t)in + stride - 1) / stride : ((int64_t)in + stride - filter) / stride;
  return (int)std::min<int64_t>(std::max<int64_t>(n, INT32_MIN), INT32_MAX);
}

lce_hip_status lce_hip_bmaxpool_output_shape(int32_t in_h, int32_t in_w, int32_t fh, int32_t fw, int32_t sh,
                                             int32_t sw, int32_t padding, int32_t* out_h, int32_t* out_w) {
  if (!out_h || !out_w) return fail(LCE_HIP_ERR_INVALID, "bmaxpool_output_shape: null argument");
  if (sh == 0 || sw == 0 || fh == 0 || fw == 0)
    return fail(LCE_HIP_ERR_INVALID, "bmaxpool: strides and filter sizes must be non-zero");  // bmaxpool.cc:52-55
  if (padding != LCE_HIP_PADDING_SAME && padding != LCE_HIP_PADDING_VALID)
    return fail(LCE_HIP_ERR_INVALID, "bmaxpool: padding must be SAME or VALID");
  *out_h = pool_out(padding, in_h, fh, sh);
  *out_w = pool_out(padding, in_w, fw, sw);
  return LCE_HIP_OK;
}

lce_hip_status lce_hip_bmaxpool(const int32_t* input_dev, int32_t batch, int32_t in_h, int32_t in_w,
                                int32_t words, int32_t fh, int32_t fw, int32_t sh, int32_t sw,
                                int32_t padding, int32_t* output_dev, void* stream) {
  int32_t oh = 0, ow = 0;
  if (lce_hip_status s = lce_hip_bmaxpool_output_shape(in_h, in_w, fh, fw, sh, sw, padding, &oh, &ow)) return s;
  if (batch == 0) return LCE_HIP_OK;   // empty batch: nothing to do (core/bmaxpool.h:43 loops zero times)
  if (!input_dev || !output_dev) return fail(LCE_HIP_ERR_INVALID, "bmaxpool: null tensor");
  if (oh < 1 || ow < 1 || batch < 0 || words < 1) return fail(LCE_HIP_ERR_INVALID, "bmaxpool: empty tensor");
  if (lce_hip_status s = require_device()) return s;
  const int ph = std::max(0, (oh - 1) * sh + fh - in_h) / 2;
  const int pw = std::max(0, (ow - 1) * sw + fw - in_w) / 2;
  // 16 bytes per thread when the words of a pixel come in fours and the tensors are 16-byte aligned
  const bool vec = words % 4 == 0 && ((uintptr_t)input_dev & 15) == 0 && ((uintptr_t)output_dev & 15) == 0;
  const int groups = vec ? words / 4 : words;
  const uint64_t total = (uint64_t)batch * oh * ow * groups;
  const unsigned grid = lce::stream_grid((total + 63) / 64);
  auto kernel = vec ? lce::bmaxpool_words<4> : lce::bmaxpool_words<1>;
  kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const uint32_t*)input_dev, (uint32_t*)output_dev, batch, in_h, in_w,
                                                  groups, oh, ow, fh, fw, sh, sw, ph, pw, total, lce::make_fastdiv((uint32_t)groups),
                                                  lce::make_fastdiv((uint32_t)ow), lce::make_fastdiv((uint32_t)oh));
  LCE_HIP_TRY(hipGetLastError());
  return LCE_HIP_OK;
}

// ------------------------------------------------------------------------------------
// converter-side parameter preparation (host-only, lce_prepare.cpp)
// ------------------------------------------------------------------------------------
static lce_hip_status prep_status(const std::string& err) {
  return err.empty() ? LCE_HIP_OK : fail(LCE_HIP_ERR_INVALID, "%s", err.c_str());
}

lce_hip_status lce_hip_prepare_binary_filter(const float* filter_hwio, int32_t kh, int32_t kw, int32_t cin,
                                             int32_t cout, float* filter_ohwi, float* mul, float* bias) {
  return prep_status(lce::prepare_binary_filter(filter_hwio, kh, kw, cin, cout, filter_ohwi, mul, bias));
}

lce_hip_status lce_hip_prepare_fuse_post_op(lce_hip_post_op op, const float* value, int32_t value_count,
                                            float* mul, float* bias, int32_t channels_out) {
  return prep_status(lce::fuse_post_op((int)op, value, value_count, mul, bias, channels_out));
}

int lce_hip_prepare_can_fuse_activation(const float* mul, const float* bias, int32_t channels_out,
                                        int32_t padding, int32_t pad_values) {
  if (!mul || !bias || channels_out <= 0) return 0;
  return lce::can_fuse_activation(mul, bias, channels_out, padding == LCE_HIP_PADDING_SAME, pad_values) ? 1 : 0;
}

lce_hip_status lce_hip_prepare_bitpacked_output(float* filter_ohwi, int32_t kh, int32_t kw, int32_t cin,
                                                int32_t cout, int32_t activation, int32_t padding,
                                                int32_t pad_values, const float* mul, const float* bias,
                                                int32_t* thresholds) {
  return prep_status(lce::prepare_bitpacked_output(filter_ohwi, kh, kw, cin, cout, activation,
                                                   padding == LCE_HIP_PADDING_SAME, pad_values, mul, bias, thresholds));
}

lce_hip_status lce_hip_prepare_bitpack_filter(const float* filter_ohwi, int32_t kh, int32_t kw, int32_t cin,
                                              int32_t cout, int32_t* filter_words) {
  return prep_status(lce::bitpack_filter(filter_ohwi, kh, kw, cin, cout, filter_words));
}

#ifdef LCE_TIMELINE
#ifndef LCE_UNITY
#error "the time-stamp builds are single-translation-unit builds (-DLCE_UNITY, tools/build_exp.sh)"
#endif
// profiling aid (tools/timeline.py), not part of the ABI: the K-loop time stamps of the last launch
int lce_hip_debug_read_timeline(void* host, size_t bytes) {
  if (bytes > sizeof(lce::lce_timeline)) bytes = sizeof(lce::lce_timeline);
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lce::lce_timeline), bytes);
}
#endif

#ifdef LCE_STREAM_PHASES
#ifndef LCE_UNITY
#error "the time-stamp builds are single-translation-unit builds (-DLCE_UNITY, tools/build_exp.sh)"
#endif
// profiling aid (tools/stream_phases.py), not part of the ABI: the per-block tile-step stamps of the last stream launch
int lce_hip_debug_read_stream_tl(void* host, size_t bytes) {
  if (bytes > sizeof(lce::lce_stream_tl)) bytes = sizeof(lce::lce_stream_tl);
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lce::lce_stream_tl), bytes);
}
#endif

#ifdef LCE_PW_PHASES
#ifndef LCE_UNITY
#error "the time-stamp builds are single-translation-unit builds (-DLCE_UNITY, tools/build_exp.sh)"
#endif
// profiling aid (tools/pw_phases.py), not part of the ABI: the per-block stamps of the last pointwise launch
int lce_hip_debug_read_pw_tl(void* host, size_t bytes) {
  if (bytes > sizeof(lce::lce_pw_tl)) bytes = sizeof(lce::lce_pw_tl);
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lce::lce_pw_tl), bytes);
}
int lce_hip_debug_clear_pw_tl(void) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(lce::lce_pw_tl)) != hipSuccess) return 1;
  return (int)hipMemset(p, 0, sizeof(lce::lce_pw_tl));
}
#endif

#ifdef LCE_PHASES
#ifndef LCE_UNITY
#error "the time-stamp builds are single-translation-unit builds (-DLCE_UNITY, tools/build_exp.sh)"
#endif
// profiling aid (tools/phases.py), not part of the ABI: the per-block phase stamps of the last launch
int lce_hip_debug_read_phases(void* host, size_t bytes) {
  if (bytes > sizeof(lce::lce_phase_tl)) bytes = sizeof(lce::lce_phase_tl);
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lce::lce_phase_tl), bytes);
}
int lce_hip_debug_clear_phases(void) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(lce::lce_phase_tl)) != hipSuccess) return 1;
  return (int)hipMemset(p, 0, sizeof(lce::lce_phase_tl));
}
#endif

}  // extern "C"
