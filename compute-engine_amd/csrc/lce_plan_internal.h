// Shared by the planner's three translation units (lce_plan.cpp: validation, folding, weight images, kernel selection;
// lce_plan_stream.cpp: the two streaming kernels' launch planners; lce_plan_cost.cpp: the cost estimates).  Not part of lce_plan.h: nothing
// outside the planner needs these.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "lce_plan.h"

namespace lce {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// bytes of one output pixel's channels in the layer's output type
inline uint32_t stream_row_bytes(const HostPlan& p) {
  return p.d.dst_type == LCE_HIP_BITPACKED ? (uint32_t)p.wout * 4u : (uint32_t)p.d.channels_out * (p.d.dst_type == LCE_HIP_I8 ? 1u : 4u);
}
inline int64_t out_bytes_of(const HostPlan& p, int batch_chunk) {
  return (int64_t)batch_chunk * p.out_h * p.out_w * stream_row_bytes(p);
}

// "f32" / "i8" / "bitpacked": the output type as the kernel names spell it
inline const char* dst_name(const lce_hip_bconv2d_desc& d) {
  return d.dst_type == LCE_HIP_F32 ? "f32" : d.dst_type == LCE_HIP_I8 ? "i8" : "bitpacked";
}

// Rows / columns of the padded image the matrix-core kernels read: the padding in front plus the input, or as far as the last output's
// taps reach (the streaming kernels run dilation 1 only -- stream_supported -- where the reach is (out - 1) * stride + filter)
inline int64_t padded_extent(int pad, int in, int out, int stride, int filter, int dilation) {
  return std::max<int64_t>(pad + in, (int64_t)(out - 1) * stride + (filter - 1) * dilation + 1);
}
inline int64_t padded_height(const HostPlan& p) {
  return padded_extent(p.pad_h, p.d.in_height, p.out_h, p.d.stride_height, p.d.filter_height, p.d.dilation_height);
}
inline int64_t padded_width(const HostPlan& p) {
  return padded_extent(p.pad_w, p.d.in_width, p.out_w, p.d.stride_width, p.d.filter_width, p.d.dilation_width);
}

// images of a launch of `pixels` output pixels
inline int images_per_launch(const HostPlan& p, int64_t pixels) {
  return (int)std::max<int64_t>(1, pixels / std::max<int64_t>(1, (int64_t)p.out_h * p.out_w));
}

// nothing is forced: the planner's own rule picks engine, kernel and tile
inline bool auto_rule(const PlanOptions& o) { return o.engine_pref == kEngineAuto && o.kernel_pref == kKernelAuto && o.tile_pref.tm == 0; }

// lce_plan.cpp
int group_chunks(const lce_hip_bconv2d_desc& d);
MfmaCfg choose_mfma_cfg(const HostPlan& p, int64_t pixels);

// lce_plan_cost.cpp: microseconds of one launch of `batch_chunk` images (`pixels` output pixels) on the candidate as it has just been
// planned (st_* / ws_* fields of `p`); the constants and where each was measured: the table in that file (dump_cost_table)
double estimate_stream_us(const HostPlan& p, int batch_chunk);
double estimate_wstream_us(const HostPlan& p, int batch_chunk);
double estimate_block_gemm_us(const HostPlan& p, int64_t pixels);
void dump_cost_table(FILE* f);
#ifdef LCE_COST_TUNABLE            // the re-fit build of tests/hostsim (tools/fit_cost.py): the constants by index, live
int cost_constant_count();
const char* cost_constant_name(int i);
double get_cost_constant(int i);
bool set_cost_constant(int i, double v);
#endif          // every constant of the estimates: name, value, unit, where it was measured (LCE_PLAN_DEBUG=3)

}  // namespace lce
