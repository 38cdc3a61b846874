// C ABI of include/lce_tflite_model.h: model reader + "plan from operator" helper.
// Host-side C++ (the reference's host side is C++); no HIP types here.
#include "../../../include/lce_tflite_model.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "flexbuffer_map.h"
#include "tflite_flatbuffer_reader.h"

struct lce_tflite_section {
  std::vector<int32_t> ops, inputs, outputs;
};
// The kinds of builtin operator a section may absorb (lce_tflite_model::absorbed; 0: none), one fused pass each: a row of kPasses.
enum { kAbsorbedElementwise = 1, kAbsorbedInt8Add, kAbsorbedConcat, kAbsorbedPool, kAbsorbedConv1x1, kAbsorbedDepthwise, kAbsorbedConv2d,
       kAbsorbedConvI8, kAbsorbedDepthwiseI8, kAbsorbedMean, kAbsorbedBinaryDense, kAbsorbedFullyConnected, kAbsorbedSoftmax, kAbsorbedMeanI8, kAbsorbedFullyConnectedI8,
       kAbsorbedSoftmaxI8, kAbsorbedQuantize, kAbsorbedDequantize, kAbsorbedActivation, kAbsorbedReshape, kAbsorbedGate, kAbsorbedSlice,
       kAbsorbedElementwiseI8, kAbsorbedLogisticI8, kAbsorbedMulI8, kAbsorbedCount };
// lce_tflite_model::flags_int: what only lce_tflite_model_open_passes can set
enum { kInternalHead = 1u, kInternalConvI8 = 2u, kInternalHeadI8 = 4u, kInternalQuantize = 8u, kInternalDepthwiseI8 = 16u,
       kInternalActivation = 32u, kInternalReshape = 64u, kInternalGate = 128u, kInternalBinaryDense = 256u, kInternalSlice = 512u,
       kInternalElementwiseI8 = 1024u, kInternalGateI8 = 2048u, kInternalTransition = 4096u };
struct lce_tflite_model {
  lce_tfl::Model m;
  uint32_t flags = 0;                         // lce_tflite_model_open_ex
  uint32_t flags_ext = 0;                     // lce_tflite_open_options.sections_ext
  uint32_t flags_int = 0;                     // kInternal*: lce_tflite_model_open_passes (the names of word 2 in kPassNames)
  std::vector<lce_tflite_section> sections;   // built by Partition() right after parsing
  std::vector<char> absorbed;                 // per operator: a builtin operator that runs inside a section (kAbsorbed*)
  std::vector<std::vector<int32_t>> readers;  // per tensor: the operators that read it (once per input slot)
  std::vector<int32_t> producer;              // per tensor: the first operator that lists it as an output; -1: none
  bool rank2_inputs = false;                  // an enabled pass reads rank-2 tensors (FusedPass::rank2): a section input may be one
  void Partition();
  // ---- state of lce_tflite_model_run_section (one run at a time per model) ----
  std::mutex run_mu;
  std::map<std::pair<int32_t, int64_t>, lce_hip_bconv2d_plan*> plans;   // (operator, batch * 2 + semantics) -> ready plan
  struct DevBuf { void* ptr = nullptr; size_t bytes = 0; };
  std::map<int32_t, DevBuf> scratch;                                    // intermediate tensors of a section, grow-only
  std::map<int32_t, DevBuf> consts;                                     // per-channel ADD / MUL constants on the device, uploaded once
  std::map<int32_t, DevBuf> tables;                                     // per int8 CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED and binary Dense operator: its prepare's table, uploaded once
                                                                        // (an int8 elementwise chain's table is kept under the chain's first operator)
  std::map<int32_t, std::vector<int32_t>> host_tables;                  // ... as Partition() prepared it; dropped once it is on the device
  // What one run launched.  A recorded graph keeps the record of its recording, so a replay reports the same numbers.
  struct RunStats {
    int32_t conv_quantize = 0;                                          // LceQuantize launches folded into a convolution (run_dual)
    int32_t ew_ops = 0;                                                 // ADD / MUL operators inside the lce_hip_elementwise launches
    int32_t ex_ops = 0;                                                 // operators of every kind inside the lce_hip_elementwise_ex launches
    int32_t reshape_views = 0, reshape_copies = 0;                      // absorbed RESHAPE operators: aliased / copied device to device
    int32_t dequantize_skipped = 0;                                     // LceDequantize operators only binary Dense layers read: not launched
    int32_t slice_joins = 0;                                            // lce_hip_join_windows launches that took over a CONCATENATION
    int32_t ew_i8_ops = 0;                                              // operators of every kind inside the lce_hip_elementwise_i8 launches (a head ADD included)
    int32_t gate_i8_ops = 0;                                            // MUL and residual ADD operators inside the lce_hip_mul_int8 launches
    int32_t transition_launches = 0, transition_ops = 0, transition_quantize = 0;   // lce_hip_pool_depthwise_f32 launches, the MAX_POOL_2D and
                                                                        // DEPTHWISE_CONV_2D operators inside them, the LceQuantize launches folded into them
    struct Pass { int32_t launches = 0, quantize = 0; };                // launches of a fused pass, and the LceQuantize launches folded into them
    Pass pass[kAbsorbedCount];                                          // by kAbsorbed* kind ([0] unused)
  };
  RunStats last;                                                        // of the last run
  // ---- HIP graphs (lce_tflite_model_use_hip_graphs): a section's launches recorded once per (section, batch, semantics,
  // stream, tensor pointers) and replayed as one launch.  The first call with a key runs eagerly (plans are made, weights
  // uploaded, intermediate buffers sized), the second records, later ones replay.  Recorded launches hold the model's
  // intermediate buffers: when one of those is reallocated every graph is dropped.
  struct GraphKey {
    int32_t section, batch, semantics;
    void* stream;
    std::vector<const void*> ptrs;
    bool operator<(const GraphKey& o) const {
      return std::tie(section, batch, semantics, stream, ptrs) < std::tie(o.section, o.batch, o.semantics, o.stream, o.ptrs);
    }
  };
  struct GraphEntry { int32_t eager_runs = 0; void* graph = nullptr; bool unrecordable = false; RunStats stats; };
  std::map<GraphKey, GraphEntry> graphs;
  bool use_graphs = false;
  int32_t graph_captures = 0, graph_replays = 0;
  void DropGraphs() {
    for (auto& kv : graphs) if (kv.second.graph) lce_hip_graph_destroy(kv.second.graph);
    graphs.clear();
  }
  ~lce_tflite_model() {
    DropGraphs();
    for (auto& kv : plans) lce_hip_bconv2d_plan_destroy(kv.second);
    for (auto& kv : scratch) if (kv.second.ptr) lce_hip_free(kv.second.ptr);
    for (auto& kv : consts) if (kv.second.ptr) lce_hip_free(kv.second.ptr);
    for (auto& kv : tables) if (kv.second.ptr) lce_hip_free(kv.second.ptr);
  }
};

namespace {
bool IsLceOp(const lce_tfl::Operator& o) {
  return o.builtin_code == 32 && (o.custom_code == "LceBconv2d" || o.custom_code == "LceQuantize" ||
                                  o.custom_code == "LceDequantize" || o.custom_code == "LceBMaxPool2d");
}

// Element count of a constant ADD / MUL operand that broadcasts over the last axis: [C] / [1,1,1,C] -> C, [1] / [] -> 1;
// -1 for any other shape.
int64_t BroadcastCount(const lce_tfl::Tensor& t) {
  const std::vector<int32_t>& s = t.shape;
  if (s.empty()) return 1;
  if (s.size() == 1) return s[0];
  if (s.size() == 4 && s[0] == 1 && s[1] == 1 && s[2] == 1) return s[3];
  return -1;
}

// A non-constant 4-D tensor of `out`'s height and width: what a fused pass streams next to its output (batch ignored, the
// channels are the caller's to check).
bool SameImage(const lce_tfl::Tensor& in, const lce_tfl::Tensor& out) {
  return !in.data && in.shape.size() == 4 && in.shape[1] == out.shape[1] && in.shape[2] == out.shape[2];
}

// The static half of "a builtin ADD / MUL that a section may run" (LCE_TFLITE_SECTIONS_ELEMENTWISE): float32 in and out, a
// 4-D output, each input either a non-constant tensor of the output's shape (batch ignored) or a constant of shape [C],
// [1,1,1,C], [1] or [], and an activation lce_hip_elementwise knows.  The other half -- one of its non-constant inputs is
// produced in the same epoch -- is decided by Partition().
bool ElementwiseCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinAdd && o.builtin_code != lce_tfl::kBuiltinMul) return false;
  if (o.inputs.size() != 2 || o.outputs.size() != 1) return false;
  if (o.activation < LCE_HIP_ACT_NONE || o.activation > LCE_HIP_ACT_RELU6) return false;
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (out.type != lce_tfl::kTensorFloat32 || out.shape.size() != 4 || out.shape[3] <= 0) return false;
  int variable = 0;
  for (int32_t t : o.inputs) {
    if (t < 0) return false;
    const lce_tfl::Tensor& in = M.tensors[t];
    if (in.type != lce_tfl::kTensorFloat32) return false;
    if (in.data) {
      const int64_t n = BroadcastCount(in);
      if ((n != 1 && n != out.shape[3]) || in.bytes != (size_t)n * 4) return false;
    } else {
      if (!SameImage(in, out) || in.shape[3] != out.shape[3]) return false;
      ++variable;
    }
  }
  return variable > 0;
}

// lce_hip_add_int8_desc of a builtin int8 ADD from its three tensors; false when a tensor has no quantization parameters or a
// zero point that is no int8.
bool Int8AddDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, lce_hip_add_int8_desc* d) {
  const lce_tfl::Tensor* t[3] = {&M.tensors[o.inputs[0]], &M.tensors[o.inputs[1]], &M.tensors[o.outputs[0]]};
  for (const lce_tfl::Tensor* x : t)
    if (x->type != lce_tfl::kTensorInt8 || !x->quantized || x->zero_point < -128 || x->zero_point > 127) return false;
  d->in1_scale = t[0]->scale; d->in1_zero_point = (int32_t)t[0]->zero_point;
  d->in2_scale = t[1]->scale; d->in2_zero_point = (int32_t)t[1]->zero_point;
  d->out_scale = t[2]->scale; d->out_zero_point = (int32_t)t[2]->zero_point;
  d->activation = o.activation;
  return true;
}

// The static half of "a builtin int8 ADD that a section may run" (LCE_TFLITE_SECTIONS_INT8_ADD): the residual shortcut of an
// int8-converted network.  Two inputs and one output, all int8 with quantization parameters, a 4-D output, both inputs
// non-constant tensors of the output's shape (batch ignored), an activation lce_hip_add_int8 knows, and parameters TFLite's
// Prepare accepts.  The other half -- one input is produced in the same epoch -- is decided by Partition().
bool Int8AddCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinAdd || o.inputs.size() != 2 || o.outputs.size() != 1) return false;
  if (o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (out.shape.size() != 4 || out.shape[3] <= 0) return false;
  for (int32_t t : o.inputs) {
    const lce_tfl::Tensor& in = M.tensors[t];
    if (!SameImage(in, out) || in.shape[3] != out.shape[3]) return false;
  }
  lce_hip_add_int8_desc d;
  lce_hip_add_int8_params p;
  return Int8AddDesc(M, o, &d) && lce_hip_add_int8_prepare(&d, &p) == LCE_HIP_OK;
}

// The static half of "a builtin CONCATENATION that a section may run" (LCE_TFLITE_SECTIONS_CONCAT): the channel join of a dense
// block.  2..8 inputs and one output, all of ONE type among float32, int8 and int32 (bitpacked), a 4-D output joined along its
// last axis (3 or -1) with no fused activation, every input a non-constant 4-D tensor of the output's height and width, the
// inputs' channels summing to the output's; for int8 every tensor carries quantization parameters with the SAME scale and
// zero point (a requantizing join is the host's).  The other half -- it becomes ready in an LCE epoch -- is decided by
// Partition().
bool ConcatCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinConcatenation || o.outputs.size() != 1) return false;
  if (o.inputs.size() < 2 || o.inputs.size() > (size_t)LCE_HIP_CONCAT_MAX_INPUTS) return false;
  if ((o.axis != 3 && o.axis != -1) || o.activation != LCE_HIP_ACT_NONE) return false;
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (out.type != lce_tfl::kTensorFloat32 && out.type != lce_tfl::kTensorInt8 && out.type != lce_tfl::kTensorInt32) return false;
  if (out.shape.size() != 4 || out.shape[3] <= 0) return false;
  const bool i8 = out.type == lce_tfl::kTensorInt8;
  if (i8 && (!out.quantized || out.zero_point < -128 || out.zero_point > 127)) return false;
  int64_t sum = 0;
  for (int32_t t : o.inputs) {
    if (t < 0) return false;
    const lce_tfl::Tensor& in = M.tensors[t];
    if (in.type != out.type || !SameImage(in, out) || in.shape[3] <= 0) return false;
    if (i8 && (!in.quantized || in.scale != out.scale || in.zero_point != out.zero_point)) return false;
    sum += in.shape[3];
  }
  return sum == out.shape[3];
}

// ---- what the candidate predicates of the windowed passes (pool, the float convolutions) share ----
// `in` and `out` are 4-D with positive extents, and `in` is no constant.
bool StreamedImages(const lce_tfl::Tensor& in, const lce_tfl::Tensor& out) {
  if (out.shape.size() != 4 || in.shape.size() != 4 || in.data) return false;
  for (int k = 0; k < 4; ++k)
    if (out.shape[k] <= 0 || in.shape[k] <= 0) return false;
  return true;
}

// Strides positive, padding SAME or VALID, an activation the entries know.
bool WindowOptions(const lce_tfl::Operator& o) {
  if (o.pool_stride_h <= 0 || o.pool_stride_w <= 0) return false;
  if (o.pool_padding != LCE_HIP_PADDING_SAME && o.pool_padding != LCE_HIP_PADDING_VALID) return false;
  return o.activation >= LCE_HIP_ACT_NONE && o.activation <= LCE_HIP_ACT_RELU6;
}

// The option block of a float convolution: WindowOptions and dilations of 1.
bool ConvOptions(const lce_tfl::Operator& o) { return WindowOptions(o) && o.dilation_h == 1 && o.dilation_w == 1; }

// The operands of a float convolution: 2 or 3 inputs (a third input of -1: no bias) and one output; input, filter and output
// float32; StreamedImages of input and output.
bool FloatConvOperands(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if ((o.inputs.size() != 2 && o.inputs.size() != 3) || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorFloat32 || flt.type != lce_tfl::kTensorFloat32 || out.type != lce_tfl::kTensorFloat32) return false;
  return StreamedImages(in, out);
}

// A constant 4-D filter with data in the file, positive extents, and as many bytes as its extents say: 4 x their product,
// compared by division (each extent is below 2^31; the product of the four is never formed).
bool ConstFloatFilter(const lce_tfl::Tensor& flt) {
  if (!flt.data || flt.shape.size() != 4 || (uint64_t)flt.bytes % 4u != 0) return false;
  uint64_t elems = (uint64_t)flt.bytes / 4u;
  for (int32_t extent : flt.shape) {
    if (extent <= 0 || elems % (uint64_t)extent != 0) return false;
    elems /= (uint64_t)extent;
  }
  return elems == 1;
}

// The bias of a float convolution: absent (two inputs, or a third of -1) or a constant float32 [cout] with data in the file.
bool OptionalBias(const lce_tfl::Model& M, const lce_tfl::Operator& o, int64_t cout) {
  if (o.inputs.size() != 3 || o.inputs[2] < 0) return true;
  const lce_tfl::Tensor& bias = M.tensors[o.inputs[2]];
  return bias.type == lce_tfl::kTensorFloat32 && bias.data && bias.shape.size() == 1 && bias.shape[0] == cout &&
         (uint64_t)bias.bytes == (uint64_t)cout * 4u;
}

// lce_hip_pool2d_desc of a builtin pool at `batch` images, from its options and the FILE's input tensor.
lce_hip_pool2d_desc PoolDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  lce_hip_pool2d_desc d;
  memset(&d, 0, sizeof d);
  d.op = o.builtin_code == lce_tfl::kBuiltinMaxPool2d ? LCE_HIP_POOL_MAX : LCE_HIP_POOL_AVERAGE;
  d.type = in.type == lce_tfl::kTensorInt8 ? LCE_HIP_I8 : LCE_HIP_F32;
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels = in.shape[3];
  d.filter_height = o.pool_filter_h; d.filter_width = o.pool_filter_w;
  d.stride_height = o.pool_stride_h; d.stride_width = o.pool_stride_w;
  d.padding = o.pool_padding;
  d.activation = o.activation;
  d.scale = d.type == LCE_HIP_I8 ? in.scale : 1.0f;
  d.zero_point = d.type == LCE_HIP_I8 ? (int32_t)in.zero_point : 0;
  return d;
}

// The static half of "a builtin 2-D pool that a section may run" (LCE_TFLITE_SECTIONS_EXT_POOL): AVERAGE_POOL_2D or
// MAX_POOL_2D with one input and one output; a 4-D output with positive extents; a non-constant 4-D input of the output's
// type and channel count; float32, or int8 with both tensors quantized, zero points that are int8 and the SAME scale and
// zero point (a requantizing pool is the host's); filter and stride positive, padding SAME or VALID, an activation
// lce_hip_pool2d knows; the declared output height and width equal to what the padding rule gives for the declared input;
// and a descriptor lce_hip_pool2d's own check accepts.  The other half -- it becomes ready in an LCE epoch -- is decided by
// Partition().
bool PoolCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinAveragePool2d && o.builtin_code != lce_tfl::kBuiltinMaxPool2d) return false;
  if (o.inputs.size() != 1 || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!StreamedImages(in, out) || in.type != out.type || in.shape[3] != out.shape[3]) return false;
  if (out.type == lce_tfl::kTensorInt8) {
    for (const lce_tfl::Tensor* t : {&in, &out})
      if (!t->quantized || t->zero_point < -128 || t->zero_point > 127) return false;
    if (in.scale != out.scale || in.zero_point != out.zero_point) return false;
  } else if (out.type != lce_tfl::kTensorFloat32) {
    return false;
  }
  if (o.pool_filter_h <= 0 || o.pool_filter_w <= 0 || !WindowOptions(o)) return false;
  const lce_hip_pool2d_desc d = PoolDesc(M, o, in.shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_pool2d_check(&d, &oh, &ow) == LCE_HIP_OK && oh == out.shape[1] && ow == out.shape[2];
}

// lce_hip_conv1x1_desc of a builtin CONV_2D at `batch` images, from its options and the FILE's input and filter tensors.
lce_hip_conv1x1_desc Conv1x1Desc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  lce_hip_conv1x1_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels_in = in.shape[3];
  d.channels_out = M.tensors[o.inputs[1]].shape[0];
  d.stride_height = o.pool_stride_h; d.stride_width = o.pool_stride_w;
  d.activation = o.activation;
  return d;
}

// The static half of "a builtin CONV_2D that a section may run" (LCE_TFLITE_SECTIONS_EXT_CONV1X1): the float 1x1 convolution of
// a transition block or a downsampling shortcut.  2 or 3 inputs (a third input of -1: no bias) and one output; input, filter
// and output float32, the bias float32 when present; a 4-D output with positive extents; a non-constant 4-D data input; the
// filter a constant [Cout, 1, 1, Cin] with data in the file and Cin the input's channels; the bias absent or a constant
// [Cout]; Cout the output's channels; the options table present, strides positive, dilations 1, padding SAME or VALID, an
// activation lce_hip_conv1x1_f32 knows; the declared output height and width equal to ceil(in / stride); and a descriptor
// lce_hip_conv1x1_f32's own check accepts.  The other half -- it becomes ready in an LCE epoch -- is decided by Partition().
bool Conv1x1Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinConv2d || !o.has_conv_options || !FloatConvOperands(M, o)) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!ConstFloatFilter(flt) || flt.shape[1] != 1 || flt.shape[2] != 1 || flt.shape[3] != in.shape[3]) return false;
  if (out.shape[3] != flt.shape[0] || !OptionalBias(M, o, flt.shape[0]) || !ConvOptions(o)) return false;
  const lce_hip_conv1x1_desc d = Conv1x1Desc(M, o, in.shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_conv1x1_f32_check(&d, &oh, &ow) == LCE_HIP_OK && oh == out.shape[1] && ow == out.shape[2];
}

// lce_hip_depthwise_desc of a builtin DEPTHWISE_CONV_2D at `batch` images, from its options and the FILE's input and filter tensors.
lce_hip_depthwise_desc DepthwiseDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  lce_hip_depthwise_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels_in = in.shape[3];
  d.depth_multiplier = o.depth_multiplier;
  d.filter_height = flt.shape[1]; d.filter_width = flt.shape[2];
  d.stride_height = o.pool_stride_h; d.stride_width = o.pool_stride_w;
  d.padding = o.pool_padding;
  d.activation = o.activation;
  return d;
}

// The static half of "a builtin DEPTHWISE_CONV_2D that a section may run" (LCE_TFLITE_SECTIONS_EXT_DEPTHWISE): the float blur of
// QuickNet's transition.  2 or 3 inputs (a third input of -1: no bias) and one output; input, filter and output float32, the
// bias float32 when present; a 4-D output with positive extents; a non-constant 4-D data input; the filter a constant
// [1, fh, fw, Cout] with data in the file; the bias absent or a constant [Cout]; the options table present; a depth multiplier
// >= 1 with Cout == Cin x multiplier == the output's channels; strides positive, dilations 1, padding SAME or VALID, an
// activation lce_hip_depthwise_conv2d_f32 knows; the declared output height and width what the padding rule gives; and a
// descriptor the entry's own check accepts.  The other half -- it becomes ready in an LCE epoch -- is decided by Partition().
bool DepthwiseCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinDepthwiseConv2d || !o.has_depthwise_options || !FloatConvOperands(M, o)) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!ConstFloatFilter(flt) || flt.shape[0] != 1) return false;
  const int64_t cout = flt.shape[3];
  if (o.depth_multiplier < 1 || (int64_t)in.shape[3] * o.depth_multiplier != cout || out.shape[3] != cout) return false;
  if (!OptionalBias(M, o, cout) || !ConvOptions(o)) return false;
  const lce_hip_depthwise_desc d = DepthwiseDesc(M, o, in.shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_depthwise_conv2d_f32_check(&d, &oh, &ow) == LCE_HIP_OK && oh == out.shape[1] && ow == out.shape[2];
}

// lce_hip_conv2d_desc of a builtin CONV_2D at `batch` images, from its options and the FILE's input and filter tensors.
lce_hip_conv2d_desc Conv2dDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  lce_hip_conv2d_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels_in = in.shape[3];
  d.channels_out = flt.shape[0];
  d.filter_height = flt.shape[1]; d.filter_width = flt.shape[2];
  d.stride_height = o.pool_stride_h; d.stride_width = o.pool_stride_w;
  d.padding = o.pool_padding;
  d.activation = o.activation;
  return d;
}

// The static half of "a builtin CONV_2D that a section may run" (LCE_TFLITE_SECTIONS_EXT_CONV2D): the float convolution of a
// network's stem, or one of any filter extent between binary layers.  The conditions of Conv1x1Candidate, except that the
// filter is a constant [Cout, fh, fw, Cin] with fh, fw >= 1 (a grouped filter, shape[3] != Cin, is the host's) whose byte count
// matches (compared by division: the product of the four extents is never formed); the declared output height and width are
// what the padding rule gives; and lce_hip_conv2d_f32's own check accepts the descriptor.  The other half -- when it becomes
// ready -- is decided by Partition().
bool Conv2dCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinConv2d || !o.has_conv_options || !FloatConvOperands(M, o)) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!ConstFloatFilter(flt) || flt.shape[3] != in.shape[3]) return false;
  if (out.shape[3] != flt.shape[0] || !OptionalBias(M, o, flt.shape[0]) || !ConvOptions(o)) return false;
  const lce_hip_conv2d_desc d = Conv2dDesc(M, o, in.shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_conv2d_f32_check(&d, &oh, &ow) == LCE_HIP_OK && oh == out.shape[1] && ow == out.shape[2];
}

// lce_hip_conv2d_i8_desc of a builtin int8 CONV_2D at `batch` images, from its options and the FILE's input, filter and output tensors.
lce_hip_conv2d_i8_desc ConvI8Desc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  lce_hip_conv2d_i8_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels_in = in.shape[3];
  d.channels_out = flt.shape[0];
  d.filter_height = flt.shape[1]; d.filter_width = flt.shape[2];
  d.stride_height = o.pool_stride_h; d.stride_width = o.pool_stride_w;
  d.padding = o.pool_padding;
  d.activation = o.activation;
  d.input_scale = in.scale; d.input_zero_point = (int32_t)in.zero_point;
  d.output_scale = out.scale; d.output_zero_point = (int32_t)out.zero_point;
  return d;
}

// lce_hip_conv2d_i8_prepare on the FILE's constants of int8 CONV_2D `o` (the candidate has checked their types and sizes).
lce_hip_status ConvI8Prepare(const lce_tflite_model& model, const lce_tfl::Operator& o, std::vector<int32_t>* table) {
  const lce_tfl::Model& M = model.m;
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_hip_conv2d_i8_desc d = ConvI8Desc(M, o, M.tensors[o.inputs[0]].shape[0]);
  const bool has_bias = o.inputs.size() == 3 && o.inputs[2] >= 0;
  // (flatbuffer vectors are only guaranteed 4-byte aligned, which is what int32 and float need)
  std::vector<int32_t> bias;
  if (has_bias) {
    bias.resize((size_t)flt.shape[0]);
    memcpy(bias.data(), M.tensors[o.inputs[2]].data, bias.size() * 4);
  }
  table->assign((size_t)flt.shape[0] * 3, 0);
  int32_t lo = 0, hi = 0;
  return lce_hip_conv2d_i8_prepare(&d, (const int8_t*)flt.data, has_bias ? bias.data() : nullptr, flt.scales.data(), (int32_t)flt.scales.size(),
                                   table->data(), &lo, &hi);
}

// The static half of "a builtin CONV_2D that a section may run" ("conv2d_i8" of lce_tflite_model_open_passes): the quantized
// convolution of an int8-converted network -- its stem, the 1x1 of a downsampling shortcut or of a transition.  The options
// table present; 2 or 3 inputs (a third input of -1: no bias) and one output; input and output int8, quantized with exactly ONE
// scale and a zero point in [-128, 127]; a 4-D output with positive extents; a non-constant 4-D data input; the filter a
// constant int8 [Cout, fh, fw, Cin] with data in the file whose byte count matches (compared by division), Cin the input's
// channels (a grouped filter is the host's), no zero point other than 0, and 1 or Cout scales -- with more than one,
// quantized_dimension 0; the bias absent or a constant int32 [Cout]; Cout the output's channels; strides positive, dilations 1,
// padding SAME or VALID, a known activation; and the declared output height and width what the padding rule gives.  The row's
// prepare step then asks lce_hip_conv2d_i8_prepare ONCE whether it accepts the file's constants (a pass over the whole filter) and
// Partition() keeps the table for the run; it also decides the other half -- when the operator becomes ready.
bool ConvI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinConv2d || !o.has_conv_options) return false;
  if ((o.inputs.size() != 2 && o.inputs.size() != 3) || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorInt8 || flt.type != lce_tfl::kTensorInt8 || out.type != lce_tfl::kTensorInt8) return false;
  if (!StreamedImages(in, out)) return false;
  for (const lce_tfl::Tensor* t : {&in, &out})
    if (!t->quantized || t->scales.size() != 1 || t->zero_points.size() > 1 || t->zero_point < -128 || t->zero_point > 127) return false;
  if (!flt.data || flt.shape.size() != 4) return false;
  uint64_t elems = (uint64_t)flt.bytes;
  for (int32_t extent : flt.shape) {
    if (extent <= 0 || elems % (uint64_t)extent != 0) return false;
    elems /= (uint64_t)extent;
  }
  if (elems != 1 || flt.shape[3] != in.shape[3] || out.shape[3] != flt.shape[0]) return false;
  for (int64_t z : flt.zero_points)
    if (z != 0) return false;
  const size_t n_scales = flt.scales.size();
  if (n_scales != 1 && n_scales != (size_t)flt.shape[0]) return false;
  if (n_scales > 1 && flt.quantized_dimension != 0) return false;
  if (o.inputs.size() == 3 && o.inputs[2] >= 0) {
    const lce_tfl::Tensor& bias = M.tensors[o.inputs[2]];
    if (bias.type != lce_tfl::kTensorInt32 || !bias.data || bias.shape.size() != 1 || bias.shape[0] != flt.shape[0] ||
        (uint64_t)bias.bytes != (uint64_t)flt.shape[0] * 4u)
      return false;
  }
  if (!ConvOptions(o)) return false;
  const lce_hip_conv2d_i8_desc d = ConvI8Desc(M, o, in.shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_conv2d_i8_check(&d, &oh, &ow) == LCE_HIP_OK && oh == out.shape[1] && ow == out.shape[2];
}

// lce_hip_depthwise_i8_desc of a builtin int8 DEPTHWISE_CONV_2D at `batch` images, from its options and the FILE's input, filter and
// output tensors.
lce_hip_depthwise_i8_desc DepthwiseI8Desc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  lce_hip_depthwise_i8_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels_in = in.shape[3];
  d.depth_multiplier = o.depth_multiplier;
  d.filter_height = flt.shape[1]; d.filter_width = flt.shape[2];
  d.stride_height = o.pool_stride_h; d.stride_width = o.pool_stride_w;
  d.padding = o.pool_padding;
  d.activation = o.activation;
  d.input_scale = in.scale; d.input_zero_point = (int32_t)in.zero_point;
  d.output_scale = out.scale; d.output_zero_point = (int32_t)out.zero_point;
  return d;
}

// lce_hip_depthwise_conv2d_i8_prepare on the FILE's constants of int8 DEPTHWISE_CONV_2D `o` (the candidate has checked their types
// and sizes).
lce_hip_status DepthwiseI8Prepare(const lce_tflite_model& model, const lce_tfl::Operator& o, std::vector<int32_t>* table) {
  const lce_tfl::Model& M = model.m;
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_hip_depthwise_i8_desc d = DepthwiseI8Desc(M, o, M.tensors[o.inputs[0]].shape[0]);
  const bool has_bias = o.inputs.size() == 3 && o.inputs[2] >= 0;
  // (flatbuffer vectors are only guaranteed 4-byte aligned, which is what int32 and float need)
  std::vector<int32_t> bias;
  if (has_bias) {
    bias.resize((size_t)flt.shape[3]);
    memcpy(bias.data(), M.tensors[o.inputs[2]].data, bias.size() * 4);
  }
  table->assign((size_t)flt.shape[3] * 3, 0);
  int32_t lo = 0, hi = 0;
  return lce_hip_depthwise_conv2d_i8_prepare(&d, (const int8_t*)flt.data, has_bias ? bias.data() : nullptr, flt.scales.data(),
                                             (int32_t)flt.scales.size(), table->data(), &lo, &hi);
}

// The static half of "a builtin DEPTHWISE_CONV_2D that a section may run" ("depthwise_i8" of lce_tflite_model_open_passes): the
// quantized blur of QuickNet's transition and the depthwise convolution of its stem.  The rules of ConvI8Candidate with these
// replacements: the depthwise options table present; the filter a constant int8 [1, fh, fw, Cout] whose byte count matches; a depth
// multiplier >= 1 with Cout == Cin x multiplier == the output's channels; 1 or Cout filter scales -- with more than one,
// quantized_dimension 3; the bias absent or a constant int32 [Cout]; and the declared output height and width what the padding rule
// gives.  A dilation, hybrid (float data, int8 filter) weights, a filter zero point other than 0, scales along another dimension or
// a float bias leave it with the host.  The row's prepare step then asks lce_hip_depthwise_conv2d_i8_prepare ONCE whether it
// accepts the file's constants and Partition() keeps the table for the run; it also decides the other half -- when the operator
// becomes ready.
bool DepthwiseI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinDepthwiseConv2d || !o.has_depthwise_options) return false;
  if ((o.inputs.size() != 2 && o.inputs.size() != 3) || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& flt = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorInt8 || flt.type != lce_tfl::kTensorInt8 || out.type != lce_tfl::kTensorInt8) return false;
  if (!StreamedImages(in, out)) return false;
  for (const lce_tfl::Tensor* t : {&in, &out})
    if (!t->quantized || t->scales.size() != 1 || t->zero_points.size() > 1 || t->zero_point < -128 || t->zero_point > 127) return false;
  if (!flt.data || flt.shape.size() != 4) return false;
  uint64_t elems = (uint64_t)flt.bytes;
  for (int32_t extent : flt.shape) {
    if (extent <= 0 || elems % (uint64_t)extent != 0) return false;
    elems /= (uint64_t)extent;
  }
  if (elems != 1 || flt.shape[0] != 1) return false;
  const int64_t cout = flt.shape[3];
  if (o.depth_multiplier < 1 || (int64_t)in.shape[3] * o.depth_multiplier != cout || out.shape[3] != cout) return false;
  for (int64_t z : flt.zero_points)
    if (z != 0) return false;
  const size_t n_scales = flt.scales.size();
  if (n_scales != 1 && n_scales != (size_t)cout) return false;
  if (n_scales > 1 && flt.quantized_dimension != 3) return false;
  if (o.inputs.size() == 3 && o.inputs[2] >= 0) {
    const lce_tfl::Tensor& bias = M.tensors[o.inputs[2]];
    if (bias.type != lce_tfl::kTensorInt32 || !bias.data || bias.shape.size() != 1 || bias.shape[0] != cout ||
        (uint64_t)bias.bytes != (uint64_t)cout * 4u)
      return false;
  }
  if (!ConvOptions(o)) return false;
  const lce_hip_depthwise_i8_desc d = DepthwiseI8Desc(M, o, in.shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_depthwise_conv2d_i8_check(&d, &oh, &ow) == LCE_HIP_OK && oh == out.shape[1] && ow == out.shape[2];
}


// ---- the classifier head (lce_tflite_model_open_passes, "head") ----
// A head tensor as the section walker carries it: a rank-4 tensor as it is, a rank-2 tensor [b, C] as [b, 1, 1, C]; the extents
// behind the batch must be positive.  False for every other rank.
bool Carried(const lce_tfl::Tensor& t, int32_t dims[4]) {
  if (t.shape.size() == 4) {
    for (int k = 0; k < 4; ++k) dims[k] = t.shape[k];
  } else if (t.shape.size() == 2) {
    dims[0] = t.shape[0]; dims[1] = 1; dims[2] = 1; dims[3] = t.shape[1];
  } else {
    return false;
  }
  return dims[1] > 0 && dims[2] > 0 && dims[3] > 0;
}

// lce_hip_pool2d_desc of a builtin MEAN over height and width at `batch` images: the AVERAGE pool whose filter is the FILE's image.
lce_hip_pool2d_desc MeanDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  lce_hip_pool2d_desc d;
  memset(&d, 0, sizeof d);
  d.op = LCE_HIP_POOL_AVERAGE;
  d.type = LCE_HIP_F32;
  d.batch = batch; d.in_height = in.shape[1]; d.in_width = in.shape[2]; d.channels = in.shape[3];
  d.filter_height = in.shape[1]; d.filter_width = in.shape[2];
  d.stride_height = 1; d.stride_width = 1;
  d.padding = LCE_HIP_PADDING_VALID;
  d.activation = LCE_HIP_ACT_NONE;
  d.scale = 1.0f;
  return d;
}

// The operand rules of "a builtin MEAN that a section may run" for tensors of `type`: two inputs and one output; the data input
// a non-constant 4-D tensor with positive extents; the axis a constant int32 tensor (a scalar or a vector) with data in the file
// whose entries, negative ones + 4, are exactly {1, 2}; the output [b, C] (keep_dims false) or [b, 1, 1, C] (keep_dims true)
// with the input's b and C.
bool MeanOperands(const lce_tfl::Model& M, const lce_tfl::Operator& o, int type) {
  if (o.builtin_code != lce_tfl::kBuiltinMean || o.inputs.size() != 2 || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& axis = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != type || in.data || in.shape.size() != 4 || out.type != type) return false;
  for (int32_t extent : in.shape)
    if (extent <= 0) return false;
  if (axis.type != lce_tfl::kTensorInt32 || !axis.data || axis.shape.size() > 1) return false;
  const int64_t count = axis.shape.empty() ? 1 : axis.shape[0];
  if (count < 1 || count > 4 || (uint64_t)axis.bytes != (uint64_t)count * 4u) return false;
  unsigned seen = 0;
  for (int64_t k = 0; k < count; ++k) {
    int32_t a;
    memcpy(&a, axis.data + 4 * k, 4);
    if (a < 0) a += 4;
    if (a < 0 || a > 3) return false;
    seen |= 1u << a;
  }
  if (seen != ((1u << 1) | (1u << 2))) return false;
  const std::vector<int32_t>& os = out.shape;
  if (o.keep_dims ? !(os.size() == 4 && os[1] == 1 && os[2] == 1) : os.size() != 2) return false;
  return os.front() == in.shape[0] && os.back() == in.shape[3];
}

// "A builtin MEAN that a section may run": GlobalAveragePooling.  MeanOperands on float32 tensors, and lce_hip_pool2d_check
// accepts the AVERAGE / VALID / stride 1 pool whose filter is the image.
bool MeanCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (!MeanOperands(M, o, lce_tfl::kTensorFloat32)) return false;
  const lce_hip_pool2d_desc d = MeanDesc(M, o, M.tensors[o.inputs[0]].shape[0]);
  int32_t oh = 0, ow = 0;
  return lce_hip_pool2d_check(&d, &oh, &ow) == LCE_HIP_OK && oh == 1 && ow == 1;
}

// lce_hip_fc_desc of a builtin FULLY_CONNECTED at `batch` rows, from its options and the FILE's weight tensor.
lce_hip_fc_desc FullyConnectedDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& w = M.tensors[o.inputs[1]];
  lce_hip_fc_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.inputs = w.shape[1]; d.outputs = w.shape[0];
  d.activation = o.activation;
  return d;
}

// "A builtin FULLY_CONNECTED that a section may run": the Dense layer of the head.  2 or 3 inputs (a third input of -1: no bias)
// and one output; input, weights and output float32, the bias float32 when present; the input non-constant, of rank 2 or 4, its
// extents behind the batch multiplying to K; the weights a constant [N, K] with data in the file; the bias absent or a constant
// [N]; the FullyConnectedOptions table present with weights_format 0 (DEFAULT), keep_num_dims false unless the input is rank 2,
// and an activation lce_hip_fully_connected_f32 knows; the output [b, N] with the input's b; and the entry's own check accepts
// the descriptor.  int8 and hybrid weights, a non-constant weight, shuffled weights and TANH stay with the host.
bool FullyConnectedCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinFullyConnected || !o.has_fc_options) return false;
  if ((o.inputs.size() != 2 && o.inputs.size() != 3) || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& w = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorFloat32 || w.type != lce_tfl::kTensorFloat32 || out.type != lce_tfl::kTensorFloat32) return false;
  if (o.fc_weights_format != 0 || (o.fc_keep_num_dims && in.shape.size() != 2)) return false;
  if (o.activation < LCE_HIP_ACT_NONE || o.activation > LCE_HIP_ACT_RELU6) return false;
  int32_t id[4];
  if (in.data || !Carried(in, id) || id[0] <= 0) return false;
  if (!w.data || w.shape.size() != 2 || w.shape[0] <= 0 || w.shape[1] <= 0) return false;
  const uint64_t N = (uint64_t)w.shape[0], K = (uint64_t)w.shape[1];
  if ((uint64_t)w.bytes % 4u != 0 || ((uint64_t)w.bytes / 4u) % N != 0 || (uint64_t)w.bytes / 4u / N != K) return false;
  if ((uint64_t)id[1] * (uint64_t)id[2] > K || (uint64_t)id[1] * (uint64_t)id[2] * (uint64_t)id[3] != K) return false;
  if (!OptionalBias(M, o, w.shape[0])) return false;
  if (out.shape.size() != 2 || out.shape[0] != id[0] || out.shape[1] != w.shape[0]) return false;
  const lce_hip_fc_desc d = FullyConnectedDesc(M, o, id[0]);
  return lce_hip_fully_connected_f32_check(&d) == LCE_HIP_OK;
}

// "A builtin SOFTMAX that a section may run": one float32 non-constant input [b, n] or [b, 1, 1, n]; a float32 output of the
// same shape; the SoftmaxOptions table present with a beta that is finite and > 0; and the entry's own check accepts the extents.
bool SoftmaxCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinSoftmax || !o.has_softmax_options) return false;
  if (o.inputs.size() != 1 || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorFloat32 || out.type != lce_tfl::kTensorFloat32 || in.data || in.shape != out.shape) return false;
  int32_t id[4];
  if (!Carried(in, id) || id[0] <= 0 || id[1] != 1 || id[2] != 1) return false;
  if (!std::isfinite(o.softmax_beta) || !(o.softmax_beta > 0.0f)) return false;
  return lce_hip_softmax_f32_check((size_t)id[0], (size_t)id[3], o.softmax_beta) == LCE_HIP_OK;
}

// ---- the binarized Dense layer (lce_tflite_model_open_passes, "binary_dense") ----
// The converter leaves larq's QuantDense behind a sign as LceQuantize -> LceDequantize -> a float FULLY_CONNECTED whose row o
// holds only +-s[o].  The static half of "a builtin FULLY_CONNECTED that runs as lce_hip_binary_fully_connected on the BITS":
// FullyConnectedCandidate's rules, an input of rank 2 or [b, 1, 1, K], and the entry's own check accepts the descriptor.
// The row's prepare step decides the other half (BinaryDenseSource, BinaryDensePrepare); what it refuses falls to the rows below
// ("head").
lce_hip_bfc_desc BinaryDenseDesc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_hip_fc_desc f = FullyConnectedDesc(M, o, batch);
  lce_hip_bfc_desc d;
  memset(&d, 0, sizeof d);
  d.batch = f.batch; d.inputs = f.inputs; d.outputs = f.outputs; d.activation = f.activation;
  return d;
}
bool BinaryDenseCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (!FullyConnectedCandidate(M, o)) return false;
  int32_t id[4];
  if (!Carried(M.tensors[o.inputs[0]], id) || id[1] != 1 || id[2] != 1) return false;
  const lce_hip_bfc_desc d = BinaryDenseDesc(M, o, id[0]);
  return lce_hip_bfc_check(&d) == LCE_HIP_OK;
}
// The bit tensor a binary Dense candidate `o` reads: its float input is the output of operator `producer`, an LceDequantize
// whose own input is a non-constant bitpacked int32 tensor of rank 2 or [b, 1, 1, ceil(K/32)] with the same batch.  -1: none.
int32_t BinaryDenseSource(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t producer) {
  if (producer < 0) return -1;
  const lce_tfl::Operator& dq = M.operators[producer];
  if (dq.builtin_code != lce_tfl::kBuiltinCustom || dq.custom_code != "LceDequantize" || dq.inputs.size() != 1 || dq.outputs.size() != 1 ||
      dq.outputs[0] != o.inputs[0] || dq.inputs[0] < 0 || dq.inputs[0] >= (int32_t)M.tensors.size())
    return -1;
  const lce_tfl::Tensor& bits = M.tensors[dq.inputs[0]];
  int32_t bd[4], id[4];
  if (bits.type != lce_tfl::kTensorInt32 || bits.data || !Carried(bits, bd) || !Carried(M.tensors[o.inputs[0]], id)) return -1;
  if (bd[0] != id[0] || bd[1] != 1 || bd[2] != 1 || bd[3] != (id[3] + 31) / 32) return -1;
  return dq.inputs[0];
}
// A binary Dense layer needs its bits -- the input of the LceDequantize that feeds it -- and weights lce_hip_bfc_prepare accepts:
// the table is the sign bits [N][ceil(K/32)] followed by the N scales (float32 bit patterns), kept like the int8 passes' tables.
lce_hip_status BinaryDensePrepare(const lce_tflite_model& model, const lce_tfl::Operator& o, std::vector<int32_t>* table) {
  const lce_tfl::Model& M = model.m;
  if (BinaryDenseSource(M, o, model.producer[o.inputs[0]]) < 0) return LCE_HIP_ERR_UNSUPPORTED;
  const lce_hip_bfc_desc d = BinaryDenseDesc(M, o, 1);
  const lce_tfl::Tensor& w = M.tensors[o.inputs[1]];
  const size_t N = (size_t)d.outputs, K = (size_t)d.inputs, Kw = (K + 31) / 32;
  std::vector<float> weights(N * K), scale(N);
  memcpy(weights.data(), w.data, N * K * 4);                 // (the file's bytes need not be aligned)
  table->assign(N * Kw + N, 0);
  if (lce_hip_status s = lce_hip_bfc_prepare(&d, weights.data(), table->data(), scale.data())) return s;
  memcpy(table->data() + N * Kw, scale.data(), N * 4);
  return LCE_HIP_OK;
}

// ---- the int8 classifier head and the float / int8 boundary (lce_tflite_model_open_passes, "head_i8" and "quantize") ----
// An int8 activation tensor as the entries want it: quantized with exactly ONE scale and a zero point that is an int8 value.
bool Int8Activation(const lce_tfl::Tensor& t) {
  return t.type == lce_tfl::kTensorInt8 && t.quantized && t.scales.size() == 1 && t.zero_points.size() <= 1 && t.zero_point >= -128 &&
         t.zero_point <= 127;
}

// lce_hip_mean_i8_desc of a builtin int8 MEAN over height and width at `batch` images, from the FILE's tensors.
lce_hip_mean_i8_desc MeanI8Desc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  lce_hip_mean_i8_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.height = in.shape[1]; d.width = in.shape[2]; d.channels = in.shape[3];
  d.input_scale = in.scale; d.input_zero_point = (int32_t)in.zero_point;
  d.output_scale = out.scale; d.output_zero_point = (int32_t)out.zero_point;
  return d;
}

// "A builtin int8 MEAN that a section may run": MeanOperands on int8 tensors (the axis and keep_dims rules of the float MEAN),
// both tensors Int8Activation, and lce_hip_mean_i8_prepare accepts the descriptor (no intermediate can leave int32).
bool MeanI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (!MeanOperands(M, o, lce_tfl::kTensorInt8)) return false;
  if (!Int8Activation(M.tensors[o.inputs[0]]) || !Int8Activation(M.tensors[o.outputs[0]])) return false;
  const lce_hip_mean_i8_desc d = MeanI8Desc(M, o, M.tensors[o.inputs[0]].shape[0]);
  int32_t m = 0, e = 0;
  return lce_hip_mean_i8_prepare(&d, &m, &e) == LCE_HIP_OK;
}

// lce_hip_fc_i8_desc of a builtin int8 FULLY_CONNECTED at `batch` rows, from its options and the FILE's tensors.
lce_hip_fc_i8_desc FullyConnectedI8Desc(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t batch) {
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& w = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  lce_hip_fc_i8_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch; d.inputs = w.shape[1]; d.outputs = w.shape[0];
  d.activation = o.activation;
  d.input_scale = in.scale; d.input_zero_point = (int32_t)in.zero_point;
  d.output_scale = out.scale; d.output_zero_point = (int32_t)out.zero_point;
  return d;
}

// lce_hip_fully_connected_i8_prepare on the FILE's constants of int8 FULLY_CONNECTED `o` (the candidate has checked their types
// and sizes).
lce_hip_status FullyConnectedI8Prepare(const lce_tflite_model& model, const lce_tfl::Operator& o, std::vector<int32_t>* table) {
  const lce_tfl::Model& M = model.m;
  const lce_tfl::Tensor& w = M.tensors[o.inputs[1]];
  const lce_hip_fc_i8_desc d = FullyConnectedI8Desc(M, o, M.tensors[o.inputs[0]].shape[0]);
  const bool has_bias = o.inputs.size() == 3 && o.inputs[2] >= 0;
  // (flatbuffer vectors are only guaranteed 4-byte aligned, which is what int32 and float need)
  std::vector<int32_t> bias;
  if (has_bias) {
    bias.resize((size_t)w.shape[0]);
    memcpy(bias.data(), M.tensors[o.inputs[2]].data, bias.size() * 4);
  }
  table->assign((size_t)w.shape[0] * 3, 0);
  int32_t lo = 0, hi = 0;
  return lce_hip_fully_connected_i8_prepare(&d, (const int8_t*)w.data, has_bias ? bias.data() : nullptr, w.scales.data(),
                                            (int32_t)w.scales.size(), table->data(), &lo, &hi);
}

// "A builtin int8 FULLY_CONNECTED that a section may run": the Dense layer of an int8 head.  The rules of FullyConnectedCandidate
// with: input and output Int8Activation; the weights a constant int8 [N, K] with data in the file whose byte count matches
// (compared by division), no zero point other than 0, and 1 or N scales -- with more than one, quantized_dimension 0; the bias
// absent or a constant int32 [N]; and the entry's own check accepts the descriptor.  The row's prepare step then asks
// lce_hip_fully_connected_i8_prepare ONCE whether it accepts the file's constants and Partition() keeps the table for the run.  A float
// input (hybrid weights), int16 / uint8 tensors, a weight zero point and shuffled weights stay with the host.
bool FullyConnectedI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinFullyConnected || !o.has_fc_options) return false;
  if ((o.inputs.size() != 2 && o.inputs.size() != 3) || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& w = M.tensors[o.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!Int8Activation(in) || !Int8Activation(out) || w.type != lce_tfl::kTensorInt8) return false;
  if (o.fc_weights_format != 0 || (o.fc_keep_num_dims && in.shape.size() != 2)) return false;
  if (o.activation < LCE_HIP_ACT_NONE || o.activation > LCE_HIP_ACT_RELU6) return false;
  int32_t id[4];
  if (in.data || !Carried(in, id) || id[0] <= 0) return false;
  if (!w.data || w.shape.size() != 2 || w.shape[0] <= 0 || w.shape[1] <= 0) return false;
  const uint64_t N = (uint64_t)w.shape[0], K = (uint64_t)w.shape[1];
  if ((uint64_t)w.bytes % N != 0 || (uint64_t)w.bytes / N != K) return false;
  if ((uint64_t)id[1] * (uint64_t)id[2] > K || (uint64_t)id[1] * (uint64_t)id[2] * (uint64_t)id[3] != K) return false;
  for (int64_t z : w.zero_points)
    if (z != 0) return false;
  const size_t n_scales = w.scales.size();
  if (n_scales != 1 && n_scales != (size_t)N) return false;
  if (n_scales > 1 && w.quantized_dimension != 0) return false;
  if (o.inputs.size() == 3 && o.inputs[2] >= 0) {
    const lce_tfl::Tensor& bias = M.tensors[o.inputs[2]];
    if (bias.type != lce_tfl::kTensorInt32 || !bias.data || bias.shape.size() != 1 || bias.shape[0] != w.shape[0] ||
        (uint64_t)bias.bytes != N * 4u)
      return false;
  }
  if (out.shape.size() != 2 || out.shape[0] != id[0] || out.shape[1] != w.shape[0]) return false;
  const lce_hip_fc_i8_desc d = FullyConnectedI8Desc(M, o, id[0]);
  return lce_hip_fully_connected_i8_check(&d) == LCE_HIP_OK;
}

// "A builtin int8 SOFTMAX that a section may run": one Int8Activation non-constant input [b, n] or [b, 1, 1, n]; an Int8Activation
// output of the same shape; the SoftmaxOptions table present; and lce_hip_softmax_i8_check accepts the scale, beta and the
// output quantization, which must be exactly (1/256, -128).
bool SoftmaxI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinSoftmax || !o.has_softmax_options) return false;
  if (o.inputs.size() != 1 || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!Int8Activation(in) || !Int8Activation(out) || in.data || in.shape != out.shape) return false;
  int32_t id[4];
  if (!Carried(in, id) || id[0] <= 0 || id[1] != 1 || id[2] != 1) return false;
  return lce_hip_softmax_i8_check((size_t)id[0], (size_t)id[3], in.scale, o.softmax_beta, out.scale, (int32_t)out.zero_point) == LCE_HIP_OK;
}

// "A builtin QUANTIZE / DEQUANTIZE that a section may run" ("quantize"): one non-constant input and one output of the same shape, of
// rank 2 or 4 with positive extents; QUANTIZE float32 -> Int8Activation (an int8 input -- a requantization -- is the host's),
// DEQUANTIZE Int8Activation -> float32.
bool BoundaryOperands(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t code, bool to_int8) {
  if (o.builtin_code != code || o.inputs.size() != 1 || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  const lce_tfl::Tensor& f = to_int8 ? in : out;
  const lce_tfl::Tensor& q = to_int8 ? out : in;
  if (f.type != lce_tfl::kTensorFloat32 || !Int8Activation(q) || in.data || in.shape != out.shape) return false;
  if (!std::isfinite(q.scale) || !(q.scale > 0.0f)) return false;
  int32_t id[4];
  return Carried(in, id) && id[0] > 0;
}
bool QuantizeCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) { return BoundaryOperands(M, o, lce_tfl::kBuiltinQuantize, true); }
bool DequantizeCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) { return BoundaryOperands(M, o, lce_tfl::kBuiltinDequantize, false); }

// ---- standalone activations, RESHAPE and the per-image gate (lce_tflite_model_open_passes, "activation", "reshape", "gate") ----
// The step a standalone activation is in the one-pass chain (lce_hip_elementwise_ex): RELU / RELU_N1_TO_1 / RELU6 are a CLAMP with
// that activation, LOGISTIC and PRELU themselves.  False for every other operator.
bool ActivationStep(const lce_tfl::Operator& o, int32_t* op, int32_t* activation) {
  *activation = LCE_HIP_ACT_NONE;
  switch (o.builtin_code) {
    case lce_tfl::kBuiltinRelu: *op = LCE_HIP_EW_CLAMP; *activation = LCE_HIP_ACT_RELU; return true;
    case lce_tfl::kBuiltinReluN1To1: *op = LCE_HIP_EW_CLAMP; *activation = LCE_HIP_ACT_RELU_N1_TO_1; return true;
    case lce_tfl::kBuiltinRelu6: *op = LCE_HIP_EW_CLAMP; *activation = LCE_HIP_ACT_RELU6; return true;
    case lce_tfl::kBuiltinLogistic: *op = LCE_HIP_EW_LOGISTIC; return true;
    case lce_tfl::kBuiltinPrelu: *op = LCE_HIP_EW_PRELU; return true;
    default: return false;
  }
}

// Element count of a constant PRELU alpha that broadcasts over the last axis: BroadcastCount's shapes and [1,1,C] (what the
// converter writes for shared_axes=[1,2]); -1 for any other shape -- a full [H,W,C] alpha is the host's.
int64_t AlphaCount(const lce_tfl::Tensor& t) {
  const std::vector<int32_t>& s = t.shape;
  if (s.size() == 3 && s[0] == 1 && s[1] == 1) return s[2];
  return BroadcastCount(t);
}

// "A standalone activation that a section may run" ("activation"): RELU, RELU_N1_TO_1, RELU6 or LOGISTIC with one input, PRELU
// with two; one output; input and output float32 of the same shape, of rank 2 or 4 with positive extents (Carried), the input
// non-constant; PRELU's alpha a constant float32 with data in the file, of shape [C], [1,1,C], [1,1,1,C], [1] or [] and as many
// bytes.  int8 tensors, a full [H,W,C] alpha and TANH stay with the host.  The operator joins the epoch in which it becomes ready.
bool ActivationCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  int32_t step, act;
  if (!ActivationStep(o, &step, &act)) return false;
  const bool prelu = o.builtin_code == lce_tfl::kBuiltinPrelu;
  if (o.inputs.size() != (prelu ? 2u : 1u) || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorFloat32 || out.type != lce_tfl::kTensorFloat32 || in.data || in.shape != out.shape) return false;
  int32_t id[4];
  if (!Carried(in, id) || id[0] <= 0) return false;
  if (prelu) {
    if (o.inputs[1] < 0) return false;
    const lce_tfl::Tensor& alpha = M.tensors[o.inputs[1]];
    if (alpha.type != lce_tfl::kTensorFloat32 || !alpha.data) return false;
    const int64_t n = AlphaCount(alpha);
    if ((n != 1 && n != id[3]) || (uint64_t)alpha.bytes != (uint64_t)n * 4u) return false;
  }
  return true;
}

// "A builtin RESHAPE that a section may run" ("reshape"): a view of the same bytes.  One or two inputs and one output; the data
// input non-constant, float32, int8 or int32, the output of the same type (int8: the same scale and zero point); the optional
// second input -- the new shape -- absent or a constant (the reshape is judged by the DECLARED shape of its output tensor; a shape
// computed at run time is the host's); input and output of rank 2 or 4 with positive extents (Carried), the same leading extent
// and the same element count behind it.  Anything that moves the batch extent stays with the host.
bool ReshapeCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinReshape || (o.inputs.size() != 1 && o.inputs.size() != 2) || o.outputs.size() != 1) return false;
  if (o.inputs[0] < 0) return false;
  if (o.inputs.size() == 2 && o.inputs[1] >= 0 && !M.tensors[o.inputs[1]].data) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.data || in.type != out.type) return false;
  if (in.type != lce_tfl::kTensorFloat32 && in.type != lce_tfl::kTensorInt8 && in.type != lce_tfl::kTensorInt32) return false;
  if (in.type == lce_tfl::kTensorInt8 && (in.quantized != out.quantized || in.scale != out.scale || in.zero_point != out.zero_point)) return false;
  int32_t id[4], od[4];
  if (!Carried(in, id) || !Carried(out, od) || id[0] <= 0 || id[0] != od[0]) return false;
  return (uint64_t)id[1] * (uint64_t)id[2] * (uint64_t)id[3] == (uint64_t)od[1] * (uint64_t)od[2] * (uint64_t)od[3];
}

// The input slot (0 or 1) of gate `o` that holds the [b,1,1,C] operand; the other slot holds the streamed [b,H,W,C] tensor.  -1
// when the two inputs are not such a pair.  (Both [b,1,1,C]: slot 1 is the operand.)
int GateOperandSlot(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  for (int slot = 1; slot >= 0; --slot) {
    const lce_tfl::Tensor& g = M.tensors[o.inputs[slot]];
    const lce_tfl::Tensor& x = M.tensors[o.inputs[1 - slot]];
    if (g.shape.size() == 4 && g.shape[0] == out.shape[0] && g.shape[1] == 1 && g.shape[2] == 1 && g.shape[3] == out.shape[3] &&
        x.shape == out.shape)
      return slot;
  }
  return -1;
}

// "A float ADD / MUL by a per-image tensor that a section may run" ("gate"): the scale of a squeeze-and-excite block.  Two
// inputs and one output, all float32, both inputs non-constant; a 4-D output [b,H,W,C] with positive extents; one input of the
// output's shape, the other [b,1,1,C]; an activation lce_hip_elementwise knows.  A [b,C] operand does not qualify (TFLite's
// broadcast aligns it to the trailing axes: it is not per image), and rank-2 ADD / MUL stay with the host.
bool GateCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinAdd && o.builtin_code != lce_tfl::kBuiltinMul) return false;
  if (o.inputs.size() != 2 || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  if (o.activation < LCE_HIP_ACT_NONE || o.activation > LCE_HIP_ACT_RELU6) return false;
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (out.type != lce_tfl::kTensorFloat32 || out.shape.size() != 4) return false;
  for (int32_t extent : out.shape)
    if (extent <= 0) return false;
  for (int32_t t : o.inputs)
    if (M.tensors[t].type != lce_tfl::kTensorFloat32 || M.tensors[t].data) return false;
  return GateOperandSlot(M, o) >= 0;
}

// The channel window [begin, begin + count) that STRIDED_SLICE / SLICE `o` cuts out of its 4-D data input, resolved as TFLite
// resolves a stride of 1: a masked begin is 0 and a masked end the extent, a negative index gets the extent added, begin and end
// are then clamped to [0, extent]; for SLICE a size of -1 means "to the end".  False unless the index operands are constant int32
// [4] tensors with data in the file, every stride is 1, axes 0..2 come out as their whole extent and axis 3 as a window of at
// least one channel.
bool SliceWindow(const lce_tfl::Model& M, const lce_tfl::Operator& o, int32_t* begin, int32_t* count) {
  const bool strided = o.builtin_code == lce_tfl::kBuiltinStridedSlice;
  const size_t operands = strided ? 4 : 3;
  if (o.inputs.size() != operands) return false;
  int32_t v[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {1, 1, 1, 1}};        // begin, end / size, strides
  for (size_t k = 1; k < operands; ++k) {
    if (o.inputs[k] < 0) return false;
    const lce_tfl::Tensor& T = M.tensors[o.inputs[k]];
    if (T.type != lce_tfl::kTensorInt32 || !T.data || T.shape.size() != 1 || T.shape[0] != 4 || T.bytes != 16) return false;
    memcpy(v[k - 1], T.data, 16);
  }
  const std::vector<int32_t>& shape = M.tensors[o.inputs[0]].shape;
  for (int axis = 0; axis < 4; ++axis) {
    const int64_t extent = shape[axis];
    int64_t b = v[0][axis], e = v[1][axis];
    if (strided) {
      if (v[2][axis] != 1) return false;
      if (b < 0) b += extent;
      if (e < 0) e += extent;
      if (o.begin_mask & (1 << axis)) b = 0;
      if (o.end_mask & (1 << axis)) e = extent;
      b = std::min(std::max<int64_t>(b, 0), extent);
      e = std::min(std::max<int64_t>(e, 0), extent);
    } else {
      if (b < 0 || b > extent || e < -1) return false;
      e = e == -1 ? extent : b + e;
      if (e > extent) return false;
    }
    if (axis < 3 ? (b != 0 || e != extent) : e - b < 1) return false;
    if (axis == 3) { *begin = (int32_t)b; *count = (int32_t)(e - b); }
  }
  return true;
}

// "A builtin STRIDED_SLICE / SLICE that a section may run" ("slice"): the channel window of MeliusNet's improvement block.  One
// output; the data input a non-constant float32 or int8 4-D tensor with positive extents; the output of the same type and, for
// int8, both tensors with ONE scale and zero point each, the same (a requantizing slice is the host's); for STRIDED_SLICE the
// options table present, no ellipsis, new-axis or shrink mask and `offset` false; a window SliceWindow resolves; and the declared
// output [b, H, W, count].  Everything else stays with the host: another axis, a stride, a run-time index tensor, another type.
bool SliceCandidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinStridedSlice && o.builtin_code != lce_tfl::kBuiltinSlice) return false;
  if (o.inputs.empty() || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (in.type != lce_tfl::kTensorFloat32 && in.type != lce_tfl::kTensorInt8) return false;
  if (!StreamedImages(in, out) || in.type != out.type) return false;
  if (in.type == lce_tfl::kTensorInt8) {
    for (const lce_tfl::Tensor* t : {&in, &out})
      if (!t->quantized || t->scales.size() != 1 || t->zero_points.size() > 1 || t->zero_point < -128 || t->zero_point > 127) return false;
    if (in.scale != out.scale || in.zero_point != out.zero_point) return false;
  }
  if (o.builtin_code == lce_tfl::kBuiltinStridedSlice &&
      (!o.has_slice_options || o.ellipsis_mask != 0 || o.new_axis_mask != 0 || o.shrink_axis_mask != 0 || o.slice_offset))
    return false;
  int32_t begin = 0, count = 0;
  if (!SliceWindow(M, o, &begin, &count)) return false;
  return out.shape[0] == in.shape[0] && out.shape[1] == in.shape[1] && out.shape[2] == in.shape[2] && out.shape[3] == count;
}

// ---- the int8 elementwise chain ("elementwise_i8" of lce_tflite_model_open_passes) ----
// The step of lce_hip_elementwise_i8 that builtin operator `o` is, with its constant in the file (`values` points into the
// model), and the tensor it streams.  It is a step when the output is int8 and 4-D with positive extents, the streamed input a
// non-constant int8 tensor of the output's shape (batch ignored), every tensor quantized with ONE scale and a zero point in
// [-128, 127] (Int8Activation), and the operator one of
//   ADD with exactly one constant operand of shape [C], [1,1,1,C], [1] or [] whose data is in the file, as many bytes;
//   PRELU with a constant alpha of shape [C], [1,1,C], [1,1,1,C], [1] or [], likewise;
//   RELU, RELU_N1_TO_1, RELU6;
//   QUANTIZE int8 -> int8 (the requantize in front of a CONCATENATION whose inputs differ in scale).
// These stay with the host (int8 MUL and int8 LOGISTIC are the "gate_i8" rows'): a full [H,W,C] alpha, a non-constant alpha, a per-channel-quantized
// constant, uint8 / int16 tensors, rank-2 tensors.
bool ElementwiseI8Step(const lce_tfl::Model& M, const lce_tfl::Operator& o, lce_hip_ew_i8_step* st, int32_t* x_t) {
  memset(st, 0, sizeof *st);
  if (o.outputs.size() != 1 || o.inputs.empty() || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!Int8Activation(out) || out.shape.size() != 4) return false;
  for (int32_t extent : out.shape)
    if (extent <= 0) return false;
  int32_t x = o.inputs[0];
  const lce_tfl::Tensor* k = nullptr;
  int64_t n = 0;
  switch (o.builtin_code) {
    case lce_tfl::kBuiltinAdd: {
      if (o.inputs.size() != 2 || o.inputs[1] < 0) return false;
      const bool c0 = M.tensors[o.inputs[0]].data != nullptr, c1 = M.tensors[o.inputs[1]].data != nullptr;
      if (c0 == c1) return false;                                  // (two tensors: the residual ADD's; two constants: nobody's)
      x = o.inputs[c0 ? 1 : 0];
      k = &M.tensors[o.inputs[c0 ? 0 : 1]];
      n = BroadcastCount(*k);
      st->op = LCE_HIP_EW_I8_ADD;
      st->activation = o.activation;
      break;
    }
    case lce_tfl::kBuiltinPrelu:
      if (o.inputs.size() != 2 || o.inputs[1] < 0) return false;
      k = &M.tensors[o.inputs[1]];
      n = AlphaCount(*k);
      st->op = LCE_HIP_EW_I8_PRELU;
      break;
    case lce_tfl::kBuiltinRelu: case lce_tfl::kBuiltinReluN1To1: case lce_tfl::kBuiltinRelu6:
      if (o.inputs.size() != 1) return false;
      st->op = LCE_HIP_EW_I8_CLAMP;
      st->activation = o.builtin_code == lce_tfl::kBuiltinRelu ? LCE_HIP_ACT_RELU
                       : o.builtin_code == lce_tfl::kBuiltinRelu6 ? LCE_HIP_ACT_RELU6 : LCE_HIP_ACT_RELU_N1_TO_1;
      break;
    case lce_tfl::kBuiltinQuantize:
      if (o.inputs.size() != 1) return false;
      st->op = LCE_HIP_EW_I8_REQUANTIZE;
      break;
    default: return false;
  }
  const lce_tfl::Tensor& in = M.tensors[x];
  if (!Int8Activation(in) || !SameImage(in, out) || in.shape[3] != out.shape[3]) return false;
  if (k) {
    if (!k->data || !Int8Activation(*k)) return false;
    if ((n != 1 && n != out.shape[3]) || (uint64_t)k->bytes != (uint64_t)n) return false;
    st->operand = n == 1 ? LCE_HIP_EW_SCALAR : LCE_HIP_EW_PER_CHANNEL;
    st->values = (const int8_t*)k->data;
    st->operand_scale = k->scale;
    st->operand_zero_point = (int32_t)k->zero_point;
  }
  st->out_scale = out.scale;
  st->out_zero_point = (int32_t)out.zero_point;
  *x_t = x;
  return true;
}
bool ElementwiseI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  lce_hip_ew_i8_step st;
  int32_t x = -1;
  return ElementwiseI8Step(M, o, &st, &x);
}
// The row's prepare step: lce_hip_elementwise_i8_prepare on the operator as a chain of ONE step, from the file's constants.  What
// it refuses (an ADD multiplier outside (0, 1), an intermediate that could leave int32) stays with the host.  The table it writes
// is dropped: a run prepares ONE table for the whole chain the operator ends up in.
lce_hip_status ElementwiseI8Prepare(const lce_tflite_model& model, const lce_tfl::Operator& o, std::vector<int32_t>* table) {
  const lce_tfl::Model& M = model.m;
  lce_hip_elementwise_i8_desc d;
  memset(&d, 0, sizeof d);
  int32_t x = -1;
  if (!ElementwiseI8Step(M, o, &d.steps[0], &x)) return LCE_HIP_ERR_INVALID;
  d.channels = M.tensors[o.outputs[0]].shape[3];
  d.in_scale = M.tensors[x].scale;
  d.in_zero_point = (int32_t)M.tensors[x].zero_point;
  d.num_steps = 1;
  size_t bytes = 0;
  if (lce_hip_status s = lce_hip_elementwise_i8_table_size(&d, &bytes)) return s;
  std::vector<uint8_t> scratch(bytes);
  table->clear();
  return lce_hip_elementwise_i8_prepare(&d, scratch.data());
}

// ---- the int8 squeeze-and-excite gate ("gate_i8" of lce_tflite_model_open_passes) ----
// "A builtin int8 LOGISTIC that a section may run": one input and one output, both Int8Activation and of the same shape, of rank 2
// or 4 with positive extents (Carried), the input non-constant.  The prepare step (lce_hip_logistic_int8_prepare) wants the output
// at exactly (1/256, -128) and keeps the 256-byte table for the first run.
bool LogisticI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  if (o.builtin_code != lce_tfl::kBuiltinLogistic || o.inputs.size() != 1 || o.outputs.size() != 1 || o.inputs[0] < 0) return false;
  const lce_tfl::Tensor& in = M.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!Int8Activation(in) || !Int8Activation(out) || in.data || in.shape != out.shape) return false;
  int32_t id[4];
  return Carried(in, id) && id[0] > 0;
}
lce_hip_status LogisticI8Prepare(const lce_tflite_model& model, const lce_tfl::Operator& o, std::vector<int32_t>* table) {
  const lce_tfl::Tensor& in = model.m.tensors[o.inputs[0]];
  const lce_tfl::Tensor& out = model.m.tensors[o.outputs[0]];
  table->assign(64, 0);
  return lce_hip_logistic_int8_prepare(in.scale, (int32_t)in.zero_point, out.scale, (int32_t)out.zero_point, (uint8_t*)table->data());
}

// lce_hip_mul_int8_desc (without an ADD) of builtin int8 MUL `o`, the tensor it streams and its operand.  It is one when it has two
// non-constant Int8Activation inputs and one Int8Activation 4-D output with positive extents, one input of the output's shape and
// the other of that shape too (a TENSOR operand: input 1) or [b,1,1,C] (GateOperandSlot's rule: the per-image gate, in either slot;
// a [b,C] operand does not qualify), and an activation in NONE..RELU6.  A constant operand stays with the host.
bool MulI8Desc(const lce_tfl::Model& M, const lce_tfl::Operator& o, lce_hip_mul_int8_desc* d, int32_t* x_t, int32_t* g_t) {
  memset(d, 0, sizeof *d);
  if (o.builtin_code != lce_tfl::kBuiltinMul || o.inputs.size() != 2 || o.outputs.size() != 1 || o.inputs[0] < 0 || o.inputs[1] < 0) return false;
  if (o.activation < LCE_HIP_ACT_NONE || o.activation > LCE_HIP_ACT_RELU6) return false;
  const lce_tfl::Tensor& out = M.tensors[o.outputs[0]];
  if (!Int8Activation(out) || out.shape.size() != 4) return false;
  for (int32_t extent : out.shape)
    if (extent <= 0) return false;
  for (int32_t t : o.inputs)
    if (!Int8Activation(M.tensors[t]) || M.tensors[t].data) return false;
  const int slot = GateOperandSlot(M, o);
  if (slot >= 0) {
    d->operand = LCE_HIP_EW_PER_IMAGE_CHANNEL;
    *x_t = o.inputs[1 - slot];
    *g_t = o.inputs[slot];
  } else {
    if (M.tensors[o.inputs[0]].shape != out.shape || M.tensors[o.inputs[1]].shape != out.shape) return false;
    d->operand = LCE_HIP_EW_TENSOR;
    *x_t = o.inputs[0];
    *g_t = o.inputs[1];
  }
  const lce_tfl::Tensor &x = M.tensors[*x_t], &g = M.tensors[*g_t];
  d->in1_scale = x.scale; d->in1_zero_point = (int32_t)x.zero_point;
  d->in2_scale = g.scale; d->in2_zero_point = (int32_t)g.zero_point;
  d->out_scale = out.scale; d->out_zero_point = (int32_t)out.zero_point;
  d->activation = o.activation;
  return true;
}
// "A builtin int8 MUL that a section may run": MulI8Desc, and lce_hip_mul_int8_prepare accepts it.
bool MulI8Candidate(const lce_tfl::Model& M, const lce_tfl::Operator& o) {
  lce_hip_mul_int8_desc d;
  lce_hip_mul_int8_params p;
  int32_t x = -1, g = -1;
  return MulI8Desc(M, o, &d, &x, &g) && lce_hip_mul_int8_prepare(&d, &p) == LCE_HIP_OK;
}

// THE names of lce_tflite_model_open_passes, each with the flag word (0 `flags`, 1 `flags_ext`, 2 `flags_int`) and the bit of it
// that the name sets: the only place the three are written.  "stem" is a name that is no pass (Partition() reads its bit), and so is
// "transition" (Walk::Pool2d reads its bit: the partition does not move); "head", "head_i8" and "quantize" enable several rows of
// kPasses each.
struct PassName { const char* name; int word; uint32_t bit; };
constexpr PassName kPassNames[] = {
    {"elementwise", 0, LCE_TFLITE_SECTIONS_ELEMENTWISE}, {"int8_add", 0, LCE_TFLITE_SECTIONS_INT8_ADD},
    {"concat", 0, LCE_TFLITE_SECTIONS_CONCAT},           {"pool", 1, LCE_TFLITE_SECTIONS_EXT_POOL},
    {"conv1x1", 1, LCE_TFLITE_SECTIONS_EXT_CONV1X1},     {"depthwise", 1, LCE_TFLITE_SECTIONS_EXT_DEPTHWISE},
    {"conv2d", 1, LCE_TFLITE_SECTIONS_EXT_CONV2D},       {"stem", 1, LCE_TFLITE_SECTIONS_EXT_STEM},
    {"head", 2, kInternalHead},                          {"conv2d_i8", 2, kInternalConvI8},
    {"head_i8", 2, kInternalHeadI8},                     {"quantize", 2, kInternalQuantize},
    {"depthwise_i8", 2, kInternalDepthwiseI8},           {"activation", 2, kInternalActivation},
    {"reshape", 2, kInternalReshape},                    {"gate", 2, kInternalGate},
    {"binary_dense", 2, kInternalBinaryDense},           {"slice", 2, kInternalSlice},
    {"elementwise_i8", 2, kInternalElementwiseI8},       {"gate_i8", 2, kInternalGateI8},
    {"transition", 2, kInternalTransition}};
// The entry of kPassNames called `name`; null when there is none.
constexpr const PassName* Named(const char* name) {
  for (const PassName& n : kPassNames) {
    const char *a = n.name, *b = name;
    while (*a && *a == *b) ++a, ++b;
    if (*a == *b) return &n;
  }
  return nullptr;
}

// One fused pass, a row of kPasses (in priority order, below Walk): its kind; the name that enables it; the static half of "a
// section may run this operator"; the walker that runs it; and everything else Partition() and the walk ask about a pass --
//   prepare   (optional) the step that follows the predicate: it sees the model (the binary Dense row looks at `producer`) and
//             fills the table Partition() keeps for the first run (host_tables); when it refuses, the search goes on with the rows below
//   as_lce    the operator is queued as the LCE operators are, whatever made it ready (see Partition())
//   rank2     the pass reads rank-2 tensors, carried as [b, 1, 1, C]: while its flag is set a section input may be one
struct Walk;
struct FusedPass {
  int kind;
  const PassName* name;
  bool (*candidate)(const lce_tfl::Model&, const lce_tfl::Operator&);
  lce_hip_status (Walk::*walker)(int32_t);
  lce_hip_status (*prepare)(const lce_tflite_model&, const lce_tfl::Operator&, std::vector<int32_t>* table);
  bool as_lce, rank2;
};
extern const FusedPass kPasses[kAbsorbedCount - 1];
}  // namespace

// The partition a delegate would get (tensorflow/lite/graph_info.cc, PartitionGraphIntoIndependentNodeSubsets, restated from
// its published description): alternate between epochs of LCE operators and epochs of the others, starting with the kind of
// the first ready operator; in an epoch every operator of the epoch's kind whose inputs are all ready joins, repeatedly, until nothing more
// can; the LCE operators of one epoch, sorted by index, are one section.  (On a chain this is "walk the file, cut at
// every builtin operator"; on a branched graph an LCE op further down the file joins an EARLIER section when nothing it
// reads depends on a builtin operator in between.)  Linear in operators + tensor uses: per-tensor reader lists and a count
// of unready inputs per operator; the model is untrusted input.
void lce_tflite_model::Partition() {
  const int n_ops = (int)m.operators.size(), n_t = (int)m.tensors.size();
  auto valid = [&](int32_t t) { return t >= 0 && t < n_t; };
  std::vector<char> produced(n_t, 0), is_output(n_t, 0), is_lce(n_ops, 0), candidate(n_ops, 0);
  const uint32_t words[3] = {flags, flags_ext, flags_int};
  for (const FusedPass& p : kPasses) rank2_inputs = rank2_inputs || (p.rank2 && (words[p.name->word] & p.name->bit));
  readers.assign(n_t, {});
  producer.assign(n_t, -1);
  absorbed.assign(n_ops, 0);
  std::vector<int32_t> unready(n_ops, 0);
  for (int i = 0; i < n_ops; ++i)
    for (int32_t t : m.operators[i].outputs)
      if (valid(t) && producer[t] < 0) producer[t] = i;
  for (int i = 0; i < n_ops; ++i) {
    is_lce[i] = IsLceOp(m.operators[i]) ? 1 : 0;
    // the first pass, in the table's order, that is enabled, whose predicate holds and whose prepare step, if it has one,
    // accepts the file's constants (its table is kept for the first run).  An absorbed operator joins the epoch in
    // which it becomes ready, so it lands in a section exactly when the last of its inputs was produced by an LCE epoch (one
    // that is ready from the start -- a stem op -- is a builtin one without LCE_TFLITE_SECTIONS_EXT_STEM, below)
    for (const FusedPass& p : kPasses) {
      if (!(words[p.name->word] & p.name->bit) || !p.candidate(m, m.operators[i])) continue;
      if (p.prepare) {
        std::vector<int32_t> table;
        if (p.prepare(*this, m.operators[i], &table) != LCE_HIP_OK) continue;
        host_tables[i] = std::move(table);
      }
      candidate[i] = (char)p.kind;
      // a head operator (MEAN, FULLY_CONNECTED -- float, int8 or binary --, SOFTMAX) is queued as the LCE operators are, whatever
      // made it ready: behind a host operator the head is a section of its own, behind the body it joins the body's epoch
      if (p.as_lce) is_lce[i] = 1;
      break;
    }
    for (int32_t t : m.operators[i].outputs)
      if (valid(t)) produced[t] = 1;                         // produced by an operator: not ready until it has run
  }
  for (int i = 0; i < n_ops; ++i)
    for (int32_t t : m.operators[i].inputs)
      if (valid(t)) {
        readers[t].push_back(i);
        if (produced[t]) ++unready[i];
      }
  for (int32_t t : m.outputs)
    if (valid(t)) is_output[t] = 1;
  // ready operators of either kind, waiting for their epoch
  std::vector<int32_t> queue[2];
  // (a candidate ready from the start is a builtin op -- the stem is the host's -- unless LCE_TFLITE_SECTIONS_EXT_STEM queues it
  // with the LCE operators: a stem of candidates then joins the first LCE epoch, and a section need not hold an LCE operator)
  const bool stem = (flags_ext & LCE_TFLITE_SECTIONS_EXT_STEM) != 0;
  for (int i = 0; i < n_ops; ++i)
    if (unready[i] == 0) queue[is_lce[i] || (stem && candidate[i]) ? 1 : 0].push_back(i);
  std::vector<int32_t> section_of(n_ops, -1);
  std::vector<char> made(n_t, 0), listed(n_t, 0);
  int remaining = n_ops;
  // the first epoch has the kind of the first ready operator in execution order (graph_info.cc takes it from there: usually a
  // builtin stem operator), so an LCE operator that is ready at the start beside a builtin one lands in the same section a
  // delegate would be handed
  int kind = 1;                                              // 1: LCE epoch
  if (!queue[0].empty() && (queue[1].empty() || queue[0].front() < queue[1].front())) kind = 0;
  int idle_epochs = 0;
  while (remaining > 0 && idle_epochs < 2) {                 // (a graph with a cycle or a dangling input never finishes)
    std::vector<int32_t>& q = queue[kind];
    lce_tflite_section sec;
    bool any = false;
    for (size_t head = 0; head < q.size(); ++head) {         // grows while it is walked
      const int32_t i = q[head];
      any = true;
      --remaining;
      if (kind) sec.ops.push_back(i);
      if (kind && candidate[i]) absorbed[i] = candidate[i];
      for (int32_t t : m.operators[i].outputs) {
        if (!valid(t) || made[t]) continue;
        made[t] = 1;
        for (int32_t r : readers[t])
          if (--unready[r] == 0) queue[candidate[r] && !is_lce[r] ? kind : (int)is_lce[r]].push_back(r);
      }
    }
    q.clear();
    if (kind && !sec.ops.empty()) {
      std::sort(sec.ops.begin(), sec.ops.end());
      const int32_t id = (int32_t)sections.size();
      for (int32_t i : sec.ops) section_of[i] = id;
      std::vector<int32_t> ins, outs;
      for (int32_t i : sec.ops) {
        for (int32_t t : m.operators[i].inputs)
          if (valid(t) && !m.tensors[t].data) ins.push_back(t);
        for (int32_t t : m.operators[i].outputs)
          if (valid(t)) outs.push_back(t);
      }
      std::sort(outs.begin(), outs.end());
      outs.erase(std::unique(outs.begin(), outs.end()), outs.end());
      for (int32_t t : ins)                                  // first-use order
        if (!listed[t] && !std::binary_search(outs.begin(), outs.end(), t)) {
          listed[t] = 1;
          sec.inputs.push_back(t);
        }
      for (int32_t t : sec.inputs) listed[t] = 0;
      for (int32_t t : outs) {
        bool outside_reader = is_output[t] != 0;
        for (size_t k = 0; k < readers[t].size() && !outside_reader; ++k) outside_reader = section_of[readers[t][k]] != id;
        if (outside_reader) sec.outputs.push_back(t);
      }
      sections.push_back(sec);
    }
    idle_epochs = any ? 0 : idle_epochs + 1;
    kind ^= 1;
  }
}

namespace {
thread_local std::string g_model_error;
lce_hip_status Fail(lce_hip_status code, const std::string& msg) {
  g_model_error = msg;
  return code;
}
}  // namespace

extern "C" {

lce_tflite_model* lce_tflite_model_open(const void* data, size_t size, char* err, size_t err_len) {
  return lce_tflite_model_open_ex(data, size, 0u, err, err_len);
}

// Both entries funnel into ONE pair of flag words; `allowed` is the entry's own mask of the first.
static lce_tflite_model* OpenWithFlags(const void* data, size_t size, uint32_t flags, uint32_t allowed, uint32_t flags_ext,
                                       uint32_t allowed_ext, const char* refusal, char* err, size_t err_len, uint32_t flags_int = 0u) {
  auto* model = new (std::nothrow) lce_tflite_model{};
  std::string e = "out of memory";
  if (refusal) {
    e = refusal;
  } else if ((flags & ~allowed) || (flags_ext & ~allowed_ext)) {
    e = "unknown flags";
  } else if (model && data && model->m.Parse(data, size, &e)) {
    model->flags = flags;
    model->flags_ext = flags_ext;
    model->flags_int = flags_int;
    model->Partition();
    return model;
  }
  if (!data && !refusal) e = "null buffer";
  if (err && err_len) snprintf(err, err_len, "%s", e.c_str());
  delete model;
  return nullptr;
}

lce_tflite_model* lce_tflite_model_open_ex(const void* data, size_t size, uint32_t flags, char* err, size_t err_len) {
  return OpenWithFlags(data, size, flags, LCE_TFLITE_SECTIONS_ELEMENTWISE | LCE_TFLITE_SECTIONS_INT8_ADD, 0u, 0u, nullptr, err, err_len);
}

lce_tflite_model* lce_tflite_model_open_opts(const void* data, size_t size, const lce_tflite_open_options* options, char* err,
                                             size_t err_len) {
  // versioned by size: the first form is 8 bytes (struct_size, sections), the second 24 (+ sections_ext, reserved[3]), the
  // third 40 (+ reserved2[4]), the fourth 56 (+ reserved3[4]); nothing behind the size the caller states is read
  constexpr uint32_t kFirstForm = 8, kSecondForm = 24, kThirdForm = 40;
  static_assert(sizeof(lce_tflite_open_options) == 56, "the fourth form of the options struct");
  const char* refusal = nullptr;
  uint32_t sections = 0, ext = 0, allowed_ext = 0;
  uint32_t words[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (copied: the caller's object may be only 8, 24 or 40 bytes long)
  if (options) memcpy(words, options, kFirstForm);
  if (!options) {
    refusal = "null options";
  } else if (words[0] != kFirstForm && words[0] != kSecondForm && words[0] != kThirdForm &&
             words[0] != (uint32_t)sizeof(lce_tflite_open_options)) {
    refusal = "options: unknown struct_size";
  } else {
    memcpy(words, options, words[0]);
    sections = words[1];
    if (words[0] != kFirstForm) {
      ext = words[2];
      allowed_ext = LCE_TFLITE_SECTIONS_EXT_POOL;
      if (words[0] != kSecondForm) allowed_ext |= LCE_TFLITE_SECTIONS_EXT_CONV1X1;
      // (the fourth form also carries the bits assigned after it: none of them widens the struct)
      if (words[0] != kSecondForm && words[0] != kThirdForm)
        allowed_ext |= LCE_TFLITE_SECTIONS_EXT_DEPTHWISE | LCE_TFLITE_SECTIONS_EXT_CONV2D | LCE_TFLITE_SECTIONS_EXT_STEM;
      uint32_t rest = 0;
      for (uint32_t k = 3; k < words[0] / 4; ++k) rest |= words[k];
      if (rest) refusal = "options: reserved fields must be zero";
    }
  }
  return OpenWithFlags(data, size, sections, LCE_TFLITE_SECTIONS_ELEMENTWISE | LCE_TFLITE_SECTIONS_INT8_ADD | LCE_TFLITE_SECTIONS_CONCAT,
                       ext, allowed_ext, refusal, err, err_len);
}

lce_tflite_model* lce_tflite_model_open_passes(const void* data, size_t size, const char* passes, char* err, size_t err_len) {
  uint32_t words[3] = {0u, 0u, 0u};
  std::string refusal;
  if (!passes) refusal = "null passes";
  for (const char* at = passes; at && *at && refusal.empty();) {
    const char* end = strchr(at, ',');
    const std::string name = end ? std::string(at, end) : std::string(at);
    const PassName* found = Named(name.c_str());
    if (!found) refusal = "passes: unknown name '" + name + "'";
    else if (words[found->word] & found->bit) refusal = "passes: '" + name + "' is named twice";
    else words[found->word] |= found->bit;
    if (end && !end[1] && refusal.empty()) refusal = "passes: unknown name ''";      // a trailing comma
    at = end ? end + 1 : nullptr;
  }
  return OpenWithFlags(data, size, words[0], ~0u, words[1], ~0u, refusal.empty() ? nullptr : refusal.c_str(), err, err_len, words[2]);
}

void lce_tflite_model_close(lce_tflite_model* model) { delete model; }

int32_t lce_tflite_model_num_tensors(const lce_tflite_model* model) { return model ? (int32_t)model->m.tensors.size() : 0; }
int32_t lce_tflite_model_num_operators(const lce_tflite_model* model) { return model ? (int32_t)model->m.operators.size() : 0; }

static int32_t copy_indices(const std::vector<int32_t>& v, int32_t* out, int32_t cap) {
  for (int32_t i = 0; out && i < cap && i < (int32_t)v.size(); ++i) out[i] = v[i];
  return (int32_t)v.size();
}
int32_t lce_tflite_model_inputs(const lce_tflite_model* model, int32_t* indices, int32_t cap) {
  return model ? copy_indices(model->m.inputs, indices, cap) : 0;
}
int32_t lce_tflite_model_outputs(const lce_tflite_model* model, int32_t* indices, int32_t cap) {
  return model ? copy_indices(model->m.outputs, indices, cap) : 0;
}

lce_hip_status lce_tflite_model_tensor(const lce_tflite_model* model, int32_t index, lce_tflite_tensor_info* info) {
  if (!model || !info || index < 0 || index >= (int32_t)model->m.tensors.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_tensor: bad argument");
  const lce_tfl::Tensor& t = model->m.tensors[index];
  if (t.shape.size() > 8) return Fail(LCE_HIP_ERR_UNSUPPORTED, "lce_tflite_model_tensor: rank > 8");
  memset(info, 0, sizeof *info);
  info->type = t.type;
  info->rank = (int32_t)t.shape.size();
  for (size_t i = 0; i < t.shape.size(); ++i) info->dims[i] = t.shape[i];
  info->quantized = t.quantized ? 1 : 0;
  info->scale = t.scale;
  info->zero_point = (int32_t)t.zero_point;
  info->data = t.data;
  info->bytes = t.bytes;
  info->name = t.name.c_str();
  return LCE_HIP_OK;
}

int32_t lce_tflite_model_tensor_scales(const lce_tflite_model* model, int32_t index, float* scales, int32_t cap, int32_t* quantized_dimension) {
  if (!model || index < 0 || index >= (int32_t)model->m.tensors.size()) return -1;
  const lce_tfl::Tensor& t = model->m.tensors[index];
  for (int32_t k = 0; scales && k < cap && k < (int32_t)t.scales.size(); ++k) scales[k] = t.scales[k];
  if (quantized_dimension) *quantized_dimension = t.quantized_dimension;
  return (int32_t)t.scales.size();
}

lce_hip_status lce_tflite_model_operator(const lce_tflite_model* model, int32_t index, lce_tflite_operator_info* info) {
  if (!model || !info || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator: bad argument");
  const lce_tfl::Operator& o = model->m.operators[index];
  info->builtin_code = o.builtin_code;
  info->custom_code = o.custom_code.c_str();
  info->inputs = o.inputs.data();
  info->num_inputs = (int32_t)o.inputs.size();
  info->outputs = o.outputs.data();
  info->num_outputs = (int32_t)o.outputs.size();
  info->custom_options = o.custom_options;
  info->custom_options_size = o.custom_options_size;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_activation(const lce_tflite_model* model, int32_t index, int32_t* activation) {
  if (!model || !activation || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_activation: bad argument");
  *activation = model->m.operators[index].activation;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_axis(const lce_tflite_model* model, int32_t index, int32_t* axis) {
  if (!model || !axis || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_axis: bad argument");
  *axis = model->m.operators[index].axis;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_pool2d(const lce_tflite_model* model, int32_t index, int32_t options[5]) {
  if (!model || !options || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_pool2d: bad argument");
  const lce_tfl::Operator& o = model->m.operators[index];
  options[0] = o.pool_padding; options[1] = o.pool_stride_w; options[2] = o.pool_stride_h;
  options[3] = o.pool_filter_w; options[4] = o.pool_filter_h;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_conv2d(const lce_tflite_model* model, int32_t index, int32_t options[5]) {
  if (!model || !options || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_conv2d: bad argument");
  const lce_tfl::Operator& o = model->m.operators[index];
  const bool conv = o.has_conv_options;
  options[0] = conv ? o.pool_padding : 0; options[1] = conv ? o.pool_stride_w : 0; options[2] = conv ? o.pool_stride_h : 0;
  options[3] = o.dilation_w; options[4] = o.dilation_h;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_depthwise(const lce_tflite_model* model, int32_t index, int32_t options[6]) {
  if (!model || !options || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_depthwise: bad argument");
  const lce_tfl::Operator& o = model->m.operators[index];
  const bool dw = o.has_depthwise_options;
  options[0] = dw ? o.pool_padding : 0; options[1] = dw ? o.pool_stride_w : 0; options[2] = dw ? o.pool_stride_h : 0;
  options[3] = dw ? o.depth_multiplier : 0;
  options[4] = dw ? o.dilation_w : 1; options[5] = dw ? o.dilation_h : 1;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_reducer(const lce_tflite_model* model, int32_t index, int32_t* keep_dims) {
  if (!model || !keep_dims || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_reducer: bad argument");
  *keep_dims = model->m.operators[index].keep_dims ? 1 : 0;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_fully_connected(const lce_tflite_model* model, int32_t index, int32_t options[3], int32_t* present) {
  if (!model || !options || !present || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_fully_connected: bad argument");
  const lce_tfl::Operator& o = model->m.operators[index];
  *present = o.has_fc_options ? 1 : 0;
  options[0] = o.has_fc_options ? o.activation : 0;
  options[1] = o.fc_weights_format;
  options[2] = o.fc_keep_num_dims ? 1 : 0;
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_operator_softmax(const lce_tflite_model* model, int32_t index, float* beta, int32_t* present) {
  if (!model || !beta || !present || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_operator_softmax: bad argument");
  const lce_tfl::Operator& o = model->m.operators[index];
  *present = o.has_softmax_options ? 1 : 0;
  *beta = o.softmax_beta;
  return LCE_HIP_OK;
}

int32_t lce_tflite_model_num_sections(const lce_tflite_model* model) { return model ? (int32_t)model->sections.size() : 0; }
lce_hip_status lce_tflite_model_section(const lce_tflite_model* model, int32_t index, lce_tflite_section_info* info) {
  if (!model || !info || index < 0 || index >= (int32_t)model->sections.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_section: bad argument");
  const lce_tflite_section& s = model->sections[index];
  info->ops = s.ops.data();
  info->num_ops = (int32_t)s.ops.size();
  info->inputs = s.inputs.data();
  info->num_inputs = (int32_t)s.inputs.size();
  info->outputs = s.outputs.data();
  info->num_outputs = (int32_t)s.outputs.size();
  return LCE_HIP_OK;
}

int lce_tflite_option_int(const uint8_t* custom_options, size_t size, const char* key, int32_t* value) {
  const lce_flex::Map m(custom_options, size);
  if (!m.valid() || !key || m.IsNull(key)) return 1;
  if (value) *value = m.AsInt32(key);
  return 0;
}

lce_hip_status lce_tflite_model_bconv2d_plan(const lce_tflite_model* model, int32_t index, int32_t batch,
                                             int32_t semantics, lce_hip_bconv2d_plan** plan) {
  g_model_error.clear();   // failures inside the GPU library report through lce_hip_last_error()
  if (!model || !plan || index < 0 || index >= (int32_t)model->m.operators.size())
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_bconv2d_plan: bad argument");
  const lce_tfl::Model& M = model->m;
  const lce_tfl::Operator& op = M.operators[index];
  if (op.builtin_code != lce_tfl::kBuiltinCustom || op.custom_code != "LceBconv2d")
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_bconv2d_plan: operator is not an LceBconv2d");
  // bconv2d.cc:145-152: 5 inputs (input, filter, post_activation_multiplier, post_activation_bias,
  // output_threshold), 1 output
  if (op.inputs.size() != 5 || op.outputs.size() != 1)
    return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: expected 5 inputs and 1 output");
  for (int i = 0; i < 2; ++i)
    if (op.inputs[i] < 0) return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: input and filter are required");
  const lce_tfl::Tensor& in = M.tensors[op.inputs[0]];
  const lce_tfl::Tensor& filter = M.tensors[op.inputs[1]];
  const lce_tfl::Tensor& out = M.tensors[op.outputs[0]];
  if (in.shape.size() != 4 || filter.shape.size() != 4 || in.type != lce_tfl::kTensorInt32 ||
      filter.type != lce_tfl::kTensorInt32)
    return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: input and filter must be 4-D int32 (bitpacked)");

  // Init: the option map (bconv2d.cc:85-131)
  const lce_flex::Map m(op.custom_options, op.custom_options_size);
  static const char* const kRequired[] = {"stride_height", "stride_width", "dilation_height_factor",
                                          "dilation_width_factor", "padding", "pad_values",
                                          "channels_in", "fused_activation_function"};
  for (const char* key : kRequired)
    if (!m.valid() || m.IsNull(key)) return Fail(LCE_HIP_ERR_INVALID, std::string("LceBconv2d: option missing: ") + key);

  lce_hip_bconv2d_desc d;
  memset(&d, 0, sizeof d);
  d.batch = batch > 0 ? batch : in.shape[0];
  d.in_height = in.shape[1];
  d.in_width = in.shape[2];
  d.channels_in = m.AsInt32("channels_in");
  d.channels_out = filter.shape[0];
  d.filter_height = filter.shape[1];
  d.filter_width = filter.shape[2];
  if (d.channels_in <= 0) return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: channels_in must be positive");
  // groups from the filter's packed depth (bconv2d.cc:169-186)
  const int32_t cw = (d.channels_in + 31) / 32;
  if (in.shape[3] != cw) return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: input depth does not match channels_in");
  if (filter.shape[3] == cw) {
    d.groups = 1;
  } else {
    if (filter.shape[3] <= 0 || cw % filter.shape[3] != 0)
      return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: filter depth does not divide the input depth");
    d.groups = cw / filter.shape[3];
  }
  d.stride_height = m.AsInt32("stride_height");
  d.stride_width = m.AsInt32("stride_width");
  d.dilation_height = m.AsInt32("dilation_height_factor");
  d.dilation_width = m.AsInt32("dilation_width_factor");
  d.padding = m.AsInt32("padding");
  d.pad_values = m.AsInt32("pad_values");
  const int act = m.AsInt32("fused_activation_function");   // ConvertActivation, tflite/kernels/utils.h:10-25
  d.activation = (act >= LCE_HIP_ACT_NONE && act <= LCE_HIP_ACT_RELU6) ? act : LCE_HIP_ACT_NONE;
  d.semantics = semantics;
  d.out_scale = 1.0f;
  switch (out.type) {   // bconv2d.cc:158-162
    case lce_tfl::kTensorFloat32: d.dst_type = LCE_HIP_F32; break;
    case lce_tfl::kTensorInt8:
      d.dst_type = LCE_HIP_I8;
      if (!out.quantized) return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: int8 output without quantization parameters");
      d.out_scale = out.scale;
      d.out_zero_point = (int32_t)out.zero_point;
      break;
    case lce_tfl::kTensorInt32: d.dst_type = LCE_HIP_BITPACKED; break;
    default: return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: output type must be float32, int8 or int32");
  }

  // OneTimeSetup's sources: constant tensors
  auto constant = [&](int slot, int type, size_t count, const void** p) -> bool {
    *p = nullptr;
    const int32_t ti = op.inputs[slot];
    if (ti < 0) return true;
    const lce_tfl::Tensor& t = M.tensors[ti];
    if (!t.data) return true;                                  // "none" placeholder tensor
    const size_t esz = 4;
    if (t.type != type || t.bytes != count * esz) return false;
    *p = t.data;
    return true;
  };
  const size_t fcount = (size_t)filter.shape[0] * filter.shape[1] * filter.shape[2] * filter.shape[3];
  const void *fw, *mul, *bias, *thr;
  if (!constant(1, lce_tfl::kTensorInt32, fcount, &fw) || !fw)
    return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: the filter must be a constant int32 tensor of the declared shape");
  if (!constant(2, lce_tfl::kTensorFloat32, (size_t)d.channels_out, &mul) ||
      !constant(3, lce_tfl::kTensorFloat32, (size_t)d.channels_out, &bias) ||
      !constant(4, lce_tfl::kTensorInt32, (size_t)d.channels_out, &thr))
    return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: per-channel constants have the wrong type or size");
  if (d.dst_type == LCE_HIP_BITPACKED ? !thr : (!mul || !bias))
    return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: missing thresholds (int32 output) or multiplier/bias (float/int8 output)");

  lce_hip_bconv2d_plan* p = nullptr;
  if (lce_hip_status s = lce_hip_bconv2d_plan_create(&d, &p)) return s;   // message in lce_hip_last_error()
  // flatbuffer vectors are only guaranteed 4-byte aligned; the library copies them
  if (lce_hip_status s = lce_hip_bconv2d_plan_set_weights(p, (const int32_t*)fw, (const float*)mul,
                                                          (const float*)bias, (const int32_t*)thr)) {
    lce_hip_bconv2d_plan_destroy(p);
    return s;
  }
  *plan = p;
  return LCE_HIP_OK;
}

const char* lce_tflite_model_last_error(void) { return g_model_error.c_str(); }

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// Running a binary section on device tensors (the C counterpart of examples/lce_minimal.cc:28-62 for a host without a
// TensorFlow Lite interpreter, and what compute-engine_amd/model_runner.py calls).
// ------------------------------------------------------------------------------------------------------------------
namespace {
struct Shape {
  int32_t dims[4] = {0, 0, 0, 0};
  int type = 0;
  size_t bytes() const {
    const size_t esz = (type == lce_tfl::kTensorInt8 || type == lce_tfl::kTensorBool) ? 1 : 4;
    return (size_t)dims[0] * dims[1] * dims[2] * dims[3] * esz;
  }
};

lce_hip_status PlanFor(lce_tflite_model* model, int32_t op, int32_t batch, int32_t semantics, lce_hip_bconv2d_plan** plan) {
  const auto key = std::make_pair(op, (int64_t)batch * 2 + (semantics ? 1 : 0));
  auto it = model->plans.find(key);
  if (it == model->plans.end()) {
    lce_hip_bconv2d_plan* p = nullptr;
    if (lce_hip_status s = lce_tflite_model_bconv2d_plan(model, op, batch, semantics, &p)) return s;
    it = model->plans.emplace(key, p).first;
  }
  *plan = it->second;
  return LCE_HIP_OK;
}

// The LceQuantize operators of section `sec` that read the float / int8 output of LceBconv2d `conv` (their result is
// the second output of the convolution's epilogue: lce_hip_bconv2d_run_dual).
std::vector<int32_t> QuantizeConsumers(const lce_tflite_model* model, const lce_tflite_section& sec, int32_t conv) {
  std::vector<int32_t> js;
  const lce_tfl::Operator& op = model->m.operators[conv];
  const int out_type = model->m.tensors[op.outputs[0]].type;
  if (out_type != lce_tfl::kTensorFloat32 && out_type != lce_tfl::kTensorInt8) return js;
  for (int32_t j : sec.ops) {
    const lce_tfl::Operator& q = model->m.operators[j];
    if (j > conv && q.custom_code == "LceQuantize" && q.inputs.size() == 1 && q.inputs[0] == op.outputs[0]) js.push_back(j);
  }
  return js;
}

// Device copy of a constant ADD / MUL operand, uploaded on `stream` by the first run that needs it (never while a graph is
// being recorded: the eager run before a recording has made every one).
lce_hip_status ConstOnDevice(lce_tflite_model* model, int32_t t, void* stream, bool capturing, const float** out) {
  lce_tflite_model::DevBuf& b = model->consts[t];
  if (!b.ptr) {
    if (capturing) return Fail(LCE_HIP_ERR_INVALID, "run_section: a constant would have to be uploaded during graph capture");
    const lce_tfl::Tensor& T = model->m.tensors[t];
    if (lce_hip_status s = lce_hip_malloc(&b.ptr, T.bytes)) return s;
    b.bytes = T.bytes;
    if (lce_hip_status s = lce_hip_memcpy_h2d(b.ptr, T.data, T.bytes, stream)) return s;
  }
  *out = (const float*)b.ptr;
  return LCE_HIP_OK;
}

// One walk of a section at `batch` images: shapes of every tensor it touches (shape inference exactly as the ops' Prepare
// does it) and, with `run`, the launches.  `ptr` maps tensor -> device pointer (section inputs and outputs on entry;
// intermediates are added from the model's scratch buffers).  A fused pass between binary layers plugs in as a row of kPasses
// (below): a candidate predicate (above) and a walker here -- a call of OnePass for a pass that streams one input into one
// output -- that ends in FoldQuantize / FoldBuffers / Launched.
struct Walk {
  lce_tflite_model* model;
  const lce_tflite_section& sec;
  int32_t batch, semantics;
  bool run;
  void* stream;
  bool capturing;                        // `stream` records a HIP graph: nothing may be allocated, freed or uploaded
  std::map<int32_t, void*> ptr;
  std::map<int32_t, Shape> shapes;
  std::vector<char> done;                // per operator: a launch further up has already produced its output
  // A WINDOW TENSOR: the output of an absorbed slice (or of the ADD behind it) that is no buffer but channels [begin, begin + count)
  // of tensor `src`, with tensor `addend` (-1: none) added, for the CONCATENATION that reads it (Slice, Concat)
  struct Window { int32_t src, begin, count, addend; };
  std::map<int32_t, Window> windows;

  bool IsSectionOutput(int32_t t) const { return std::find(sec.outputs.begin(), sec.outputs.end(), t) != sec.outputs.end(); }

  // The walk's inferred shape `s` is a `type` tensor of `batch` x h x w x c.  The file's shapes were checked by the partition;
  // what the walk infers must agree with them (untrusted input).
  bool Agrees(const Shape& s, int type, int32_t h, int32_t w, int32_t c) const {
    return s.type == type && s.dims[0] == batch && s.dims[1] == h && s.dims[2] == w && s.dims[3] == c;
  }

  // Device pointer of tensor `t`, which `what` reads ("an input tensor", "a CONCATENATION input", ...).
  lce_hip_status DevicePtr(int32_t t, const char* what, const void** out) const {
    auto p = ptr.find(t);
    if (p == ptr.end() || !p->second) return Fail(LCE_HIP_ERR_INVALID, "run_section: missing device pointer of " + std::string(what));
    *out = p->second;
    return LCE_HIP_OK;
  }

  // Device buffer of tensor `t`: the caller's for a section input or output, otherwise the model's grow-only scratch buffer.
  lce_hip_status BufferFor(int32_t t, size_t bytes, void** out) {
    auto it = ptr.find(t);
    if (it != ptr.end()) { *out = it->second; return LCE_HIP_OK; }
    lce_tflite_model::DevBuf& b = model->scratch[t];
    if (b.bytes < bytes) {
      // while `stream` records a graph nothing may be freed or allocated (a hipFree / hipMalloc inside a capture invalidates it and
      // the pointer would leak): the eager run before the recording sized every buffer, so this only fires if a size changed
      if (capturing) return Fail(LCE_HIP_ERR_INVALID, "run_section: a scratch buffer would have to grow during graph capture");
      // (a buffer a previous run's kernels may still use: the free below is ordered behind them by the runtime)
      if (b.ptr) lce_hip_free(b.ptr);
      model->DropGraphs();          // (recorded launches may hold the old pointer; the free above has drained the device)
      b.ptr = nullptr;
      b.bytes = 0;
      if (lce_hip_status s = lce_hip_malloc(&b.ptr, bytes ? bytes : 1)) return s;
      b.bytes = bytes;
    }
    ptr[t] = b.ptr;
    *out = b.ptr;
    return LCE_HIP_OK;
  }

  // Where the result of a fused pass (an ADD / MUL chain, an int8 ADD, a CONCATENATION, a pool, a 1x1, depthwise or KxK convolution) goes.
  struct Fold {
    int32_t value_t;                     // the tensor the pass produces
    int32_t bits_t = -1;                 // the output of the folded LceQuantize; -1: none
    bool need_value = true;              // false: only the folded LceQuantize reads value_t, so it is not written
  };
  // THE fold rule.  Tensor `t` of shape `s` is produced by a pass whose last operator is `last`.  The first LceQuantize of the
  // section after `last` that reads `t` and has not run becomes the pass's bit output (`allowed`: a bitpacked join has none):
  // it is marked done -- its own launch disappears -- and its output's shape registered.  `t` itself is still written when
  // nothing folds, when the section delivers it, or when anything but the folded LceQuantize reads it.
  Fold FoldQuantize(int32_t last, int32_t t, const Shape& s, bool allowed = true) {
    const lce_tfl::Model& M = model->m;
    Fold f{t};
    int32_t quant = -1;
    if (allowed)
      for (int32_t j : sec.ops) {
        const lce_tfl::Operator& q = M.operators[j];
        if (j > last && !done[j] && q.builtin_code == lce_tfl::kBuiltinCustom && q.custom_code == "LceQuantize" &&
            q.inputs.size() == 1 && q.inputs[0] == t && q.outputs.size() == 1) { quant = j; break; }
      }
    f.need_value = quant < 0 || IsSectionOutput(t);
    for (int32_t r : model->readers[t]) f.need_value = f.need_value || r != quant;
    if (quant >= 0) {
      done[quant] = 1;
      f.bits_t = M.operators[quant].outputs[0];
      Shape q = s;
      q.dims[3] = (s.dims[3] + 31) / 32;
      q.type = lce_tfl::kTensorInt32;
      shapes[f.bits_t] = q;
    }
    return f;
  }
  // The (value, bits) buffers of a fused pass; null for an output that is not written.
  lce_hip_status FoldBuffers(const Fold& f, void** value, void** bits) {
    *value = *bits = nullptr;
    if (f.need_value)
      if (lce_hip_status s = BufferFor(f.value_t, shapes[f.value_t].bytes(), value)) return s;
    if (f.bits_t >= 0)
      if (lce_hip_status s = BufferFor(f.bits_t, shapes[f.bits_t].bytes(), bits)) return s;
    return LCE_HIP_OK;
  }
  // The tail of every fused pass: count one launch of `kind` and, when an LceQuantize folded into it, that.
  lce_hip_status Launched(int kind, const Fold& f) {
    lce_tflite_model::RunStats::Pass& p = model->last.pass[kind];
    ++p.launches;
    if (f.bits_t >= 0) ++p.quantize;
    return LCE_HIP_OK;
  }

  // A maximal chain of absorbed ADD / MUL operators that starts at operator `first`, as ONE lce_hip_elementwise launch.  The
  // chain streams a float tensor x (an input of `first`: an LceBconv2d output or a section input) and extends through an
  // operator whose input tensor has exactly one reader and is not a section output (up to 8 steps); the other input of each
  // operator is the step's operand (a constant: scalar or per channel; otherwise a tensor of x's shape).  The chain's last
  // tensor is written in float when anything but a folded LceQuantize reads it or the section delivers it; the first
  // LceQuantize of the section that reads it becomes the launch's bit output and its own launch disappears.
  // The chain extends, by the same rules, through the absorbed operators of the other two elementwise kinds: a standalone
  // activation ("activation": a CLAMP, PRELU or LOGISTIC step) and an ADD / MUL by a [b,1,1,C] tensor ("gate": a
  // PER_IMAGE_CHANNEL operand; the gate must be the operand, never the streamed tensor).  A chain that holds one of those is
  // ONE lce_hip_elementwise_ex launch; a chain of the old step kinds alone goes through lce_hip_elementwise as before.
  static bool ChainKind(int kind) { return kind == kAbsorbedElementwise || kind == kAbsorbedActivation || kind == kAbsorbedGate; }
  lce_hip_status ElementwiseChain(int32_t first) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op0 = M.operators[first];
    const int kind0 = model->absorbed[first];
    int32_t x_t = M.tensors[op0.inputs[0]].data ? op0.inputs[1] : op0.inputs[0];
    if (kind0 == kAbsorbedActivation) x_t = op0.inputs[0];
    if (kind0 == kAbsorbedGate) x_t = op0.inputs[1 - GateOperandSlot(M, op0)];
    auto x_it = shapes.find(x_t);
    if (x_it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an ADD / MUL reads a tensor nothing produced");
    const Shape xs = x_it->second;
    if (kind0 == kAbsorbedElementwise) {
      const std::vector<int32_t>& fs = M.tensors[op0.outputs[0]].shape;
      if (!Agrees(xs, lce_tfl::kTensorFloat32, fs[1], fs[2], fs[3]))
        return Fail(LCE_HIP_ERR_INVALID, "run_section: an ADD / MUL input's shape does not match the one its producer infers");
    }
    const size_t rows = (size_t)xs.dims[0] * xs.dims[1] * xs.dims[2], channels = (size_t)xs.dims[3];

    std::vector<lce_hip_ew_step_ex> steps;
    std::vector<int32_t> chain;
    bool extended = false, gated = false;
    int32_t cur = first, v_t = x_t;
    // (an activation's or a gate's declared output must be the streamed tensor's shape: the file is untrusted input)
    auto same_image = [&](const lce_tfl::Operator& o) {
      int32_t want[4];
      return Carried(M.tensors[o.outputs[0]], want) && Agrees(xs, lce_tfl::kTensorFloat32, want[1], want[2], want[3]);
    };
    // the operand of operator `o` whose streamed input is `v`; false when it is not available yet (produced further down)
    auto operand_of = [&](const lce_tfl::Operator& o, int kind, int32_t v, lce_hip_ew_step_ex* st) -> lce_hip_status {
      memset(st, 0, sizeof *st);
      if (kind == kAbsorbedActivation) {
        if (!ActivationStep(o, &st->op, &st->activation) || o.inputs[0] != v || !same_image(o))
          return Fail(LCE_HIP_ERR_INVALID, "run_section: an activation's shape does not match the one its producer infers");
        st->operand = LCE_HIP_EW_SCALAR;
        if (st->op != LCE_HIP_EW_PRELU) return LCE_HIP_OK;
        const lce_tfl::Tensor& A = M.tensors[o.inputs[1]];
        if (A.bytes == 4) {
          memcpy(&st->scalar, A.data, 4);
          return LCE_HIP_OK;
        }
        st->operand = LCE_HIP_EW_PER_CHANNEL;
        if (A.bytes != channels * 4) return Fail(LCE_HIP_ERR_INVALID, "run_section: a PRELU alpha does not match the channels");
        if (run)
          if (lce_hip_status s = ConstOnDevice(model, o.inputs[1], stream, capturing, &st->values)) return s;
        return LCE_HIP_OK;
      }
      if (kind == kAbsorbedGate) {
        const int slot = GateOperandSlot(M, o);
        if (slot < 0 || o.inputs[1 - slot] != v) return LCE_HIP_ERR_UNSUPPORTED;     // (the chain's tensor is the gate itself: it stops before `o`)
        if (!same_image(o)) return Fail(LCE_HIP_ERR_INVALID, "run_section: a gated ADD / MUL's shape does not match the one its producer infers");
        auto it = shapes.find(o.inputs[slot]);
        if (it == shapes.end()) return LCE_HIP_ERR_UNSUPPORTED;        // (not an error: the chain stops before `o`)
        const Shape& gs = it->second;
        if (gs.type != lce_tfl::kTensorFloat32 || gs.dims[0] != xs.dims[0] || gs.dims[1] != 1 || gs.dims[2] != 1 || gs.dims[3] != xs.dims[3])
          return Fail(LCE_HIP_ERR_INVALID, "run_section: a gate is not [batch, 1, 1, channels] of the tensor it scales");
        st->op = o.builtin_code == lce_tfl::kBuiltinMul ? LCE_HIP_EW_MUL : LCE_HIP_EW_ADD;
        st->activation = o.activation;
        st->operand = LCE_HIP_EW_PER_IMAGE_CHANNEL;
        if (run) {
          const void* p = nullptr;
          if (lce_hip_status s = DevicePtr(o.inputs[slot], "a gate", &p)) return s;
          st->values = (const float*)p;
        }
        return LCE_HIP_OK;
      }
      const int32_t other = (o.inputs[0] == v) ? o.inputs[1] : o.inputs[0];
      const lce_tfl::Tensor& T = M.tensors[other];
      st->op = o.builtin_code == lce_tfl::kBuiltinMul ? LCE_HIP_EW_MUL : LCE_HIP_EW_ADD;
      st->activation = o.activation;
      if (T.data) {
        if (T.bytes == 4) {
          st->operand = LCE_HIP_EW_SCALAR;
          memcpy(&st->scalar, T.data, 4);
        } else {
          st->operand = LCE_HIP_EW_PER_CHANNEL;
          if (T.bytes != channels * 4) return Fail(LCE_HIP_ERR_INVALID, "run_section: a per-channel constant does not match the channels");
          if (run) {
            const float* d = nullptr;
            if (lce_hip_status s = ConstOnDevice(model, other, stream, capturing, &d)) return s;
            st->values = d;
          }
        }
        return LCE_HIP_OK;
      }
      auto it = shapes.find(other);
      if (it == shapes.end()) return LCE_HIP_ERR_UNSUPPORTED;        // (not an error: the chain stops before `o`)
      const Shape& os = it->second;
      if (os.type != lce_tfl::kTensorFloat32 || memcmp(os.dims, xs.dims, sizeof xs.dims) != 0)
        return Fail(LCE_HIP_ERR_INVALID, "run_section: the two tensors of an ADD / MUL differ in shape");
      st->operand = LCE_HIP_EW_TENSOR;
      if (run) {
        const void* p = nullptr;
        if (lce_hip_status s = DevicePtr(other, "an ADD / MUL input", &p)) return s;
        st->values = (const float*)p;
      }
      return LCE_HIP_OK;
    };
    for (;;) {
      const lce_tfl::Operator& o = M.operators[cur];
      const int kind = model->absorbed[cur];
      lce_hip_ew_step_ex st;
      const lce_hip_status s = operand_of(o, kind, v_t, &st);
      if (s == LCE_HIP_ERR_UNSUPPORTED && chain.empty())
        return Fail(LCE_HIP_ERR_INVALID, "run_section: an ADD / MUL reads a tensor nothing produced");
      if (s == LCE_HIP_ERR_UNSUPPORTED) break;
      if (s != LCE_HIP_OK) return s;
      steps.push_back(st);
      chain.push_back(cur);
      extended = extended || kind != kAbsorbedElementwise;
      gated = gated || kind == kAbsorbedGate;
      done[cur] = 1;
      v_t = o.outputs[0];
      shapes[v_t] = xs;
      const std::vector<int32_t>& rd = model->readers[v_t];
      if (steps.size() == 8 || rd.size() != 1 || IsSectionOutput(v_t)) break;
      const int32_t next = rd[0];
      if (!ChainKind(model->absorbed[next]) || done[next] || !std::binary_search(sec.ops.begin(), sec.ops.end(), next)) break;
      cur = next;
    }
    const Fold fold = FoldQuantize(chain.back(), v_t, xs);
    if (!run) return LCE_HIP_OK;
    const void* in = nullptr;
    if (lce_hip_status s = DevicePtr(x_t, "an ADD / MUL input", &in)) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    if (!extended) {
      std::vector<lce_hip_ew_step> old(steps.size());
      for (size_t k = 0; k < steps.size(); ++k) {
        memset(&old[k], 0, sizeof old[k]);
        old[k].op = steps[k].op; old[k].operand = steps[k].operand; old[k].values = steps[k].values;
        old[k].scalar = steps[k].scalar; old[k].activation = steps[k].activation;
      }
      if (lce_hip_status s = lce_hip_elementwise((const float*)in, rows, channels, old.data(), (int32_t)old.size(), (float*)out,
                                                 (int32_t*)bits, stream)) return s;
      model->last.ew_ops += (int32_t)chain.size();
      return Launched(kAbsorbedElementwise, fold);
    }
    if (lce_hip_status s = lce_hip_elementwise_ex((const float*)in, rows, channels, (size_t)xs.dims[1] * xs.dims[2], steps.data(),
                                                  (int32_t)steps.size(), (float*)out, (int32_t*)bits, stream)) return s;
    model->last.ex_ops += (int32_t)chain.size();
    if (gated) Launched(kAbsorbedGate, fold);
    return Launched(kAbsorbedActivation, fold);
  }

  // An absorbed RESHAPE ("reshape" of lce_tflite_model_open_passes): a view of the same bytes.  Its output takes the input's
  // device buffer -- no launch -- unless the output already has a buffer of its own (the section delivers it into the caller's):
  // then ONE device-to-device copy on `stream`.
  lce_hip_status Reshape(int32_t i) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t in_t = op.inputs[0], out_t = op.outputs[0];
    auto it = shapes.find(in_t);
    if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: a RESHAPE reads a tensor nothing produced");
    int32_t id[4], od[4];
    if (!Carried(M.tensors[in_t], id) || !Carried(M.tensors[out_t], od) || !Agrees(it->second, M.tensors[in_t].type, id[1], id[2], id[3]))
      return Fail(LCE_HIP_ERR_INVALID, "run_section: a RESHAPE input's shape or type does not match the one its producer infers");
    Shape os;
    os.dims[0] = batch; os.dims[1] = od[1]; os.dims[2] = od[2]; os.dims[3] = od[3];
    os.type = it->second.type;
    if (os.bytes() != it->second.bytes()) return Fail(LCE_HIP_ERR_INVALID, "run_section: a RESHAPE changes the element count");
    shapes[out_t] = os;
    done[i] = 1;
    if (!run) return LCE_HIP_OK;
    const void* in = nullptr;
    if (lce_hip_status s = DevicePtr(in_t, "a RESHAPE input", &in)) return s;
    auto own = ptr.find(out_t);
    if (own == ptr.end()) {
      ptr[out_t] = const_cast<void*>(in);
      ++model->last.reshape_views;
      return LCE_HIP_OK;
    }
    ++model->last.reshape_copies;
    return own->second == in ? LCE_HIP_OK : lce_hip_memcpy_d2d(own->second, in, os.bytes(), stream);
  }

  // A maximal chain of absorbed int8 elementwise operators ("elementwise_i8") that starts at operator `first`, as ONE
  // lce_hip_elementwise_i8 launch.  The chain extends by ElementwiseChain's rules: through an operator of the same kind whose
  // streamed input has exactly one reader and is not a section output, up to 8 steps.  ONE table is prepared for the whole chain and
  // uploaded once per model (kept under `first`); the first LceQuantize of the section that reads the chain's last tensor becomes the
  // launch's bit output.  `head` (-1: none): an absorbed residual int8 ADD whose sum only `first` reads -- it becomes the launch's
  // head instead of a launch of its own (Int8Add hands it over), and counts among the launch's operators.
  lce_hip_status ElementwiseI8(int32_t first) { return ElementwiseI8Chain(first, -1); }
  lce_hip_status ElementwiseI8Chain(int32_t first, int32_t head) {
    const lce_tfl::Model& M = model->m;
    lce_hip_elementwise_i8_desc d;
    memset(&d, 0, sizeof d);
    lce_hip_ew_i8_step st;
    int32_t x_t = -1;
    if (!ElementwiseI8Step(M, M.operators[first], &st, &x_t)) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 elementwise operator is no step");
    const std::vector<int32_t>& fs = M.tensors[M.operators[first].outputs[0]].shape;
    int32_t in_t = x_t, addend_t = -1;
    Shape xs;
    if (head >= 0) {
      const lce_tfl::Operator& h = M.operators[head];
      lce_hip_add_int8_desc hd;
      if (!Int8AddDesc(M, h, &hd)) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 ADD without quantization parameters");
      for (int k = 0; k < 2; ++k) {
        auto it = shapes.find(h.inputs[k]);
        if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 ADD reads a tensor nothing produced");
        xs = it->second;
        if (!Agrees(xs, lce_tfl::kTensorInt8, fs[1], fs[2], fs[3]))
          return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 ADD input's shape or type does not match the one its producer infers");
      }
      in_t = h.inputs[0];
      addend_t = h.inputs[1];
      d.has_head = 1;
      d.in_scale = hd.in1_scale; d.in_zero_point = hd.in1_zero_point;
      d.addend_scale = hd.in2_scale; d.addend_zero_point = hd.in2_zero_point;
      d.head_scale = hd.out_scale; d.head_zero_point = hd.out_zero_point;
      d.head_activation = hd.activation;
      shapes[x_t] = xs;
      done[head] = 1;
    } else {
      auto it = shapes.find(x_t);
      if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 elementwise operator reads a tensor nothing produced");
      xs = it->second;
      if (!Agrees(xs, lce_tfl::kTensorInt8, fs[1], fs[2], fs[3]))
        return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 elementwise input's shape or type does not match the one its producer infers");
      d.in_scale = M.tensors[x_t].scale;
      d.in_zero_point = (int32_t)M.tensors[x_t].zero_point;
    }
    d.channels = xs.dims[3];
    std::vector<int32_t> chain;
    int32_t cur = first, v_t = x_t;
    for (;;) {
      const lce_tfl::Operator& o = M.operators[cur];
      int32_t sx = -1;
      const std::vector<int32_t>& os = M.tensors[o.outputs[0]].shape;
      if (!ElementwiseI8Step(M, o, &st, &sx) || sx != v_t || !Agrees(xs, lce_tfl::kTensorInt8, os[1], os[2], os[3])) {
        if (chain.empty()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 elementwise operator's shape does not match the one its producer infers");
        break;
      }
      d.steps[d.num_steps++] = st;
      chain.push_back(cur);
      done[cur] = 1;
      v_t = o.outputs[0];
      shapes[v_t] = xs;
      const std::vector<int32_t>& rd = model->readers[v_t];
      if (d.num_steps == LCE_HIP_EW_I8_MAX_STEPS || rd.size() != 1 || IsSectionOutput(v_t)) break;
      const int32_t next = rd[0];
      if (model->absorbed[next] != kAbsorbedElementwiseI8 || done[next] || !std::binary_search(sec.ops.begin(), sec.ops.end(), next)) break;
      cur = next;
    }
    const Fold fold = FoldQuantize(chain.back(), v_t, xs);
    if (!run) return LCE_HIP_OK;
    const void *in = nullptr, *addend = nullptr;
    if (lce_hip_status s = DevicePtr(in_t, "an int8 elementwise input", &in)) return s;
    if (addend_t >= 0)
      if (lce_hip_status s = DevicePtr(addend_t, "an int8 ADD input", &addend)) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    lce_tflite_model::DevBuf& b = model->tables[first];
    if (!b.ptr) {
      if (capturing) return Fail(LCE_HIP_ERR_INVALID, "run_section: a constant would have to be uploaded during graph capture");
      size_t bytes = 0;
      if (lce_hip_status s = lce_hip_elementwise_i8_table_size(&d, &bytes)) return s;
      std::vector<uint8_t> table(bytes);
      if (lce_hip_status s = lce_hip_elementwise_i8_prepare(&d, table.data())) return s;
      // (the buffer becomes the model's only once the copy has completed, as TableOnDevice's)
      void* dev = nullptr;
      if (lce_hip_status s = lce_hip_malloc(&dev, bytes ? bytes : 1)) return s;
      lce_hip_status s = lce_hip_memcpy_h2d(dev, table.data(), bytes, stream);
      if (s == LCE_HIP_OK) s = lce_hip_stream_synchronize(stream);
      if (s != LCE_HIP_OK) {
        lce_hip_free(dev);
        return s;
      }
      b.ptr = dev;
      b.bytes = bytes;
    }
    if (lce_hip_status s = lce_hip_elementwise_i8(&d, (const int8_t*)in, (const int8_t*)addend, (const uint8_t*)b.ptr,
                                                  (size_t)xs.dims[0] * xs.dims[1] * xs.dims[2], (int8_t*)out, (int32_t*)bits, stream)) return s;
    model->last.ew_i8_ops += (int32_t)chain.size() + (head >= 0 ? 1 : 0);
    return Launched(kAbsorbedElementwiseI8, fold);
  }

  // An absorbed int8 LOGISTIC ("gate_i8") as ONE lce_hip_logistic_int8 launch on the table the row's prepare step made, uploaded once
  // per model.  A rank-2 tensor [b, C] -- the gate of a squeeze-and-excite block -- is carried as [b, 1, 1, C].
  lce_hip_status LogisticI8(int32_t i) {
    const lce_tfl::Model& M = model->m;
    int32_t od[4];
    if (!Carried(M.tensors[M.operators[i].outputs[0]], od)) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 LOGISTIC output of no carried rank");
    return OnePass(i, "an int8 LOGISTIC", lce_tfl::kTensorInt8, OutShape(od[1], od[2], od[3], lce_tfl::kTensorInt8), /*fold_quantize=*/true,
                   /*constants=*/0, [&](const void* x, const void*, const void*, void* out, int32_t* bits) {
                     const int32_t* table = nullptr;
                     if (lce_hip_status s = TableOnDevice(i, "an int8 LOGISTIC", &table)) return s;
                     return lce_hip_logistic_int8((const uint8_t*)table, (const int8_t*)x, (size_t)batch * od[1] * od[2], (size_t)od[3],
                                                  (int8_t*)out, bits, stream);
                   });
  }

  // An absorbed int8 MUL ("gate_i8") as ONE lce_hip_mul_int8 launch.  When the product's ONLY reader is an absorbed int8 residual
  // ADD of this section ("int8_add") whose other input has the same shape and has been produced, and the section does not deliver
  // the product, the ADD rides in the same launch (has_add: the product is never written) and is marked done; it is then counted
  // here, not by the int8 ADD's pass.  The first LceQuantize of the section that reads the result becomes the launch's bit output.
  lce_hip_status MulI8(int32_t i) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t out_t = op.outputs[0];
    const std::vector<int32_t>& fs = M.tensors[out_t].shape;
    lce_hip_mul_int8_desc d;
    int32_t x_t = -1, g_t = -1;
    if (!MulI8Desc(M, op, &d, &x_t, &g_t)) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 MUL is no gate");
    const bool per_image = d.operand == LCE_HIP_EW_PER_IMAGE_CHANNEL;
    // the inferred shape and type of BOTH inputs must agree with the file's (a producer whose output is smaller than the file
    // declares must not be read past its buffer)
    auto xi = shapes.find(x_t), gi = shapes.find(g_t);
    if (xi == shapes.end() || gi == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 MUL reads a tensor nothing produced");
    const Shape xs = xi->second;
    if (!Agrees(xs, lce_tfl::kTensorInt8, fs[1], fs[2], fs[3]) ||
        !Agrees(gi->second, lce_tfl::kTensorInt8, per_image ? 1 : fs[1], per_image ? 1 : fs[2], fs[3]))
      return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 MUL input's shape or type does not match the one its producer infers");
    shapes[out_t] = xs;
    done[i] = 1;
    int32_t add = -1, addend_t = -1, v_t = out_t;
    const std::vector<int32_t>& rd = model->readers[out_t];
    if (rd.size() == 1 && !IsSectionOutput(out_t) && model->absorbed[rd[0]] == kAbsorbedInt8Add && !done[rd[0]] &&
        std::binary_search(sec.ops.begin(), sec.ops.end(), rd[0])) {
      const lce_tfl::Operator& a = M.operators[rd[0]];
      const int32_t other = a.inputs[0] == out_t ? a.inputs[1] : a.inputs[0];
      auto oi = shapes.find(other);
      lce_hip_add_int8_desc ad;
      // (a window tensor -- a slice's output -- has a shape and no buffer of its own: such an ADD stays the int8 ADD pass's)
      if (oi != shapes.end() && !windows.count(other) && Agrees(oi->second, lce_tfl::kTensorInt8, fs[1], fs[2], fs[3]) &&
          M.tensors[a.outputs[0]].shape == M.tensors[out_t].shape && Int8AddDesc(M, a, &ad)) {
        // (TFLite's ADD scales each input by itself and sums: which slot the product stands in does not change a byte)
        const bool first = a.inputs[0] == out_t;
        d.has_add = 1;
        d.addend_scale = first ? ad.in2_scale : ad.in1_scale;
        d.addend_zero_point = first ? ad.in2_zero_point : ad.in1_zero_point;
        d.add_scale = ad.out_scale; d.add_zero_point = ad.out_zero_point;
        d.add_activation = ad.activation;
        add = rd[0];
        addend_t = other;
        v_t = a.outputs[0];
        shapes[v_t] = xs;
        done[add] = 1;
        // the product exists in registers only: the walk holds no tensor of that name (lce_tflite_model_section_tensor_shape
        // refuses it), which is how a walk without launches shows that the two operators share one
        shapes.erase(out_t);
      }
    }
    const Fold fold = FoldQuantize(add >= 0 ? add : i, v_t, xs);
    if (!run) return LCE_HIP_OK;
    const void *x = nullptr, *g = nullptr, *addend = nullptr;
    if (lce_hip_status s = DevicePtr(x_t, "an int8 MUL input", &x)) return s;
    if (lce_hip_status s = DevicePtr(g_t, "an int8 MUL input", &g)) return s;
    if (addend_t >= 0)
      if (lce_hip_status s = DevicePtr(addend_t, "an int8 ADD input", &addend)) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    if (lce_hip_status s = lce_hip_mul_int8(&d, (const int8_t*)x, (const int8_t*)g, (const int8_t*)addend, (size_t)xs.dims[0] * xs.dims[1] * xs.dims[2],
                                            (size_t)xs.dims[3], per_image ? (size_t)xs.dims[1] * xs.dims[2] : 0, (int8_t*)out, (int32_t*)bits, stream)) return s;
    model->last.gate_i8_ops += add >= 0 ? 2 : 1;
    return Launched(kAbsorbedMulI8, fold);
  }

  // An absorbed int8 ADD (LCE_TFLITE_SECTIONS_INT8_ADD) as ONE lce_hip_add_int8 launch.  The first LceQuantize of the section
  // that reads the sum becomes the launch's bit output and its own launch disappears; the int8 sum is written when anything
  // else reads it (in a residual chain the next ADD does) or the section delivers it.
  lce_hip_status Int8Add(int32_t i) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t out_t = op.outputs[0];
    const std::vector<int32_t>& fs = M.tensors[out_t].shape;
    // a sum that only an absorbed int8 elementwise chain of this section reads is that chain's head: no launch here
    const std::vector<int32_t>& rd = model->readers[out_t];
    if (rd.size() == 1 && !IsSectionOutput(out_t) && model->absorbed[rd[0]] == kAbsorbedElementwiseI8 && !done[rd[0]] &&
        std::binary_search(sec.ops.begin(), sec.ops.end(), rd[0]))
      return ElementwiseI8Chain(rd[0], i);
    // the inferred shape and type of BOTH inputs must agree with the file's (a convolution whose output is smaller than the
    // file declares must not be read past its buffer)
    Shape xs;
    for (int k = 0; k < 2; ++k) {
      auto it = shapes.find(op.inputs[k]);
      if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 ADD reads a tensor nothing produced");
      xs = it->second;
      if (!Agrees(xs, lce_tfl::kTensorInt8, fs[1], fs[2], fs[3]))
        return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 ADD input's shape or type does not match the one its producer infers");
    }
    shapes[out_t] = xs;
    done[i] = 1;
    const Fold fold = FoldQuantize(i, out_t, xs);
    if (!run) return LCE_HIP_OK;
    lce_hip_add_int8_desc d;
    if (!Int8AddDesc(M, op, &d)) return Fail(LCE_HIP_ERR_INVALID, "run_section: an int8 ADD without quantization parameters");
    const void* in[2];
    for (int k = 0; k < 2; ++k)
      if (lce_hip_status s = DevicePtr(op.inputs[k], "an int8 ADD input", &in[k])) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    if (lce_hip_status s = lce_hip_add_int8(&d, (const int8_t*)in[0], (const int8_t*)in[1], (size_t)xs.dims[0] * xs.dims[1] * xs.dims[2],
                                            (size_t)xs.dims[3], (int8_t*)out, (int32_t*)bits, stream)) return s;
    return Launched(kAbsorbedInt8Add, fold);
  }

  // An absorbed CONCATENATION (LCE_TFLITE_SECTIONS_CONCAT) as ONE launch.  Every input is a window: a window tensor gives its own
  // (with its addend), a plain input the whole tensor.  With no window tensor among them the launch is lce_hip_concat (which also
  // joins bitpacked words), otherwise lce_hip_join_windows.  The first LceQuantize of the section that reads the joined tensor
  // becomes the launch's bit output and its own launch disappears; the joined tensor itself is written when anything else reads
  // it (in a dense block the next join does) or the section delivers it.
  lce_hip_status Concat(int32_t i) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t out_t = op.outputs[0];
    const lce_tfl::Tensor& OT = M.tensors[out_t];
    const std::vector<int32_t>& fs = OT.shape;
    bool windowed = false;
    for (int32_t t : op.inputs) windowed = windowed || windows.count(t);
    if (windowed && OT.type != lce_tfl::kTensorFloat32 && OT.type != lce_tfl::kTensorInt8)
      return Fail(LCE_HIP_ERR_INVALID, "run_section: a CONCATENATION of windows is neither float32 nor int8");
    // the inferred shape and type of EVERY source and addend must agree with the file's before anything is read (a producer
    // whose output is smaller than the file declares must not be read past its buffer)
    static_assert(LCE_HIP_CONCAT_MAX_INPUTS <= LCE_HIP_JOIN_MAX_WINDOWS, "ConcatCandidate's bound on the inputs");
    Window win[LCE_HIP_JOIN_MAX_WINDOWS];
    int32_t pitch[LCE_HIP_JOIN_MAX_WINDOWS];
    const size_t n = op.inputs.size();
    int64_t sum = 0;
    for (size_t k = 0; k < n; ++k) {
      const int32_t t = op.inputs[k];
      auto w = windows.find(t);
      win[k] = w != windows.end() ? w->second : Window{t, 0, M.tensors[t].shape[3], -1};
      auto it = shapes.find(win[k].src);
      if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: a CONCATENATION reads a tensor nothing produced");
      const Shape& xs = it->second;
      pitch[k] = M.tensors[win[k].src].shape[3];
      if (!Agrees(xs, OT.type, fs[1], fs[2], pitch[k]) || win[k].begin < 0 || win[k].count < 1 || win[k].begin + (int64_t)win[k].count > pitch[k] ||
          win[k].count != M.tensors[t].shape[3])
        return Fail(LCE_HIP_ERR_INVALID, "run_section: a CONCATENATION input's shape or type does not match the one its producer infers");
      if (win[k].addend >= 0) {
        auto ad = shapes.find(win[k].addend);
        if (ad == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an ADD behind a slice reads a tensor nothing produced");
        if (!Agrees(ad->second, lce_tfl::kTensorFloat32, fs[1], fs[2], win[k].count) || OT.type != lce_tfl::kTensorFloat32)
          return Fail(LCE_HIP_ERR_INVALID, "run_section: the addend of a window does not match the window's shape");
      }
      sum += win[k].count;
    }
    if (sum != fs[3]) return Fail(LCE_HIP_ERR_INVALID, "run_section: a CONCATENATION's inputs do not add up to its output");
    const Shape os = OutShape(fs[1], fs[2], fs[3], OT.type);
    shapes[out_t] = os;
    done[i] = 1;
    const Fold fold = FoldQuantize(i, out_t, os, /*allowed=*/OT.type != lce_tfl::kTensorInt32);
    if (!run) return LCE_HIP_OK;
    lce_hip_window w[LCE_HIP_JOIN_MAX_WINDOWS];
    memset(w, 0, sizeof w);
    for (size_t k = 0; k < n; ++k) {
      if (lce_hip_status s = DevicePtr(win[k].src, "a CONCATENATION input", &w[k].data_dev)) return s;
      w[k].pitch = pitch[k]; w[k].begin = win[k].begin; w[k].count = win[k].count;
      if (win[k].addend >= 0) {
        const void* a = nullptr;
        if (lce_hip_status s = DevicePtr(win[k].addend, "the addend of a window", &a)) return s;
        w[k].addend_dev = (const float*)a;
      }
    }
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    const lce_hip_dtype type = OT.type == lce_tfl::kTensorFloat32 ? LCE_HIP_F32 : OT.type == lce_tfl::kTensorInt8 ? LCE_HIP_I8 : LCE_HIP_BITPACKED;
    const size_t rows = (size_t)batch * fs[1] * fs[2];
    const int32_t zero_point = type == LCE_HIP_I8 ? (int32_t)OT.zero_point : 0;
    if (windowed) {
      if (lce_hip_status s = lce_hip_join_windows(type, w, (int32_t)n, rows, zero_point, out, (int32_t*)bits, stream)) return s;
      ++model->last.slice_joins;
      return Launched(kAbsorbedSlice, fold);
    }
    const void* in[LCE_HIP_CONCAT_MAX_INPUTS];
    int32_t channels[LCE_HIP_CONCAT_MAX_INPUTS];
    for (size_t k = 0; k < n; ++k) { in[k] = w[k].data_dev; channels[k] = w[k].count; }
    if (lce_hip_status s = lce_hip_concat(type, in, channels, (int32_t)n, rows, zero_point, out, (int32_t*)bits, stream)) return s;
    return Launched(kAbsorbedConcat, fold);
  }

  // The reader of window-tensor candidate `t` (an absorbed slice's output, or the output of the ADD behind one) when `t` is not
  // delivered and has exactly one reader, an operator of this section after `after`; -1 otherwise.
  int32_t OnlyReader(int32_t t, int32_t after) const {
    const std::vector<int32_t>& rd = model->readers[t];
    if (IsSectionOutput(t) || rd.size() != 1 || rd[0] <= after || !std::binary_search(sec.ops.begin(), sec.ops.end(), rd[0])) return -1;
    return rd[0];
  }
  // Operator `j` is an absorbed CONCATENATION of float32 or int8 tensors that has not run.
  bool JoinsWindows(int32_t j) const {
    const int type = model->m.tensors[model->m.operators[j].outputs[0]].type;
    return model->absorbed[j] == kAbsorbedConcat && !done[j] && (type == lce_tfl::kTensorFloat32 || type == lce_tfl::kTensorInt8);
  }

  // An absorbed STRIDED_SLICE / SLICE on the channel axis ("slice" of lce_tflite_model_open_passes).  Decided from the graph
  // alone: when its output is a WINDOW TENSOR -- not delivered, exactly one reader, later in the section, which is (a) an absorbed
  // CONCATENATION of float32 / int8 tensors or (b) an "elementwise" float ADD with no fused activation, whose other input is a
  // non-constant tensor of the window's shape that is neither produced by an operator of the elementwise chain's kinds in this
  // section nor itself a window tensor, and whose output is not delivered and has exactly one reader, a CONCATENATION as in (a) --
  // the slice launches nothing and gets no buffer (in case (b) neither does the ADD, whose output is the window with an addend):
  // the CONCATENATION runs them as one lce_hip_join_windows launch.  Any other slice is ONE such launch with one window, into which
  // the first LceQuantize that reads it folds.
  lce_hip_status Slice(int32_t i) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t in_t = op.inputs[0], out_t = op.outputs[0];
    const lce_tfl::Tensor& IT = M.tensors[in_t];
    auto it = shapes.find(in_t);
    if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: a slice reads a tensor nothing produced");
    int32_t begin = 0, count = 0;
    if (!Agrees(it->second, IT.type, IT.shape[1], IT.shape[2], IT.shape[3]) || !SliceWindow(M, op, &begin, &count))
      return Fail(LCE_HIP_ERR_INVALID, "run_section: a slice input's shape or type does not match the one its producer infers");
    const Shape os = OutShape(IT.shape[1], IT.shape[2], count, IT.type);
    shapes[out_t] = os;
    done[i] = 1;
    const int32_t reader = OnlyReader(out_t, i);
    if (reader >= 0 && JoinsWindows(reader)) {
      windows[out_t] = Window{in_t, begin, count, -1};
      return LCE_HIP_OK;
    }
    if (reader >= 0 && model->absorbed[reader] == kAbsorbedElementwise && !done[reader]) {
      const lce_tfl::Operator& add = M.operators[reader];
      const int32_t other = add.inputs[0] == out_t ? add.inputs[1] : add.inputs[0];
      const int32_t sum_t = add.outputs[0];
      const lce_tfl::Tensor& OT = M.tensors[other];
      const int32_t made_by = model->producer[other];
      const bool chained = made_by >= 0 && ChainKind(model->absorbed[made_by]) && std::binary_search(sec.ops.begin(), sec.ops.end(), made_by);
      const int32_t join = OnlyReader(sum_t, reader);
      if (add.builtin_code == lce_tfl::kBuiltinAdd && add.activation == LCE_HIP_ACT_NONE && IT.type == lce_tfl::kTensorFloat32 &&
          other != out_t && !OT.data && OT.type == lce_tfl::kTensorFloat32 && OT.shape == M.tensors[out_t].shape && !chained &&
          !windows.count(other) && join >= 0 && JoinsWindows(join)) {
        done[reader] = 1;
        shapes[sum_t] = os;
        windows[sum_t] = Window{in_t, begin, count, other};
        return LCE_HIP_OK;
      }
    }
    const Fold fold = FoldQuantize(i, out_t, os);
    if (!run) return LCE_HIP_OK;
    lce_hip_window w;
    memset(&w, 0, sizeof w);
    if (lce_hip_status s = DevicePtr(in_t, "a slice input", &w.data_dev)) return s;
    w.pitch = IT.shape[3]; w.begin = begin; w.count = count;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    const bool i8 = IT.type == lce_tfl::kTensorInt8;
    if (lce_hip_status s = lce_hip_join_windows(i8 ? LCE_HIP_I8 : LCE_HIP_F32, &w, 1, (size_t)batch * IT.shape[1] * IT.shape[2],
                                                i8 ? (int32_t)IT.zero_point : 0, out, (int32_t*)bits, stream)) return s;
    return Launched(kAbsorbedSlice, fold);
  }

  // An absorbed operator `i` that streams ONE input of `in_type` and makes ONE output of shape and type `os`, as ONE launch of its
  // pass; `noun` names it in the messages ("a pool").  A rank-2 input is carried as [batch, 1, 1, C].  `launch(in, c1, c2, out, bits)`
  // is the entry, on untyped pointers: c1 and c2 are inputs 1 and 2 of the operator -- its filter or weights and its optional
  // bias --, of which the first `constants` are uploaded as they are, once per model.  With `fold_quantize` the first LceQuantize
  // of the section that reads the result becomes the launch's bit output and its own launch disappears, and the tensor itself is
  // written when anything else reads it or the section delivers it; without, `bits` is null and the output is always written.
  template <class Launch>
  lce_hip_status OnePass(int32_t i, const std::string& noun, int in_type, const Shape& os, bool fold_quantize, int constants, Launch launch) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t out_t = op.outputs[0];
    // the inferred shape and type of the input must agree with the file's (a producer whose output is smaller than the file
    // declares must not be read past its buffer)
    int32_t want[4];
    auto it = shapes.find(op.inputs[0]);
    if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: " + noun + " reads a tensor nothing produced");
    if (!Carried(M.tensors[op.inputs[0]], want) || !Agrees(it->second, in_type, want[1], want[2], want[3]))
      return Fail(LCE_HIP_ERR_INVALID, "run_section: " + noun + " input's shape or type does not match the one its producer infers");
    shapes[out_t] = os;
    done[i] = 1;
    const Fold fold = FoldQuantize(i, out_t, os, fold_quantize);
    if (!run) return LCE_HIP_OK;
    const void* in = nullptr;
    if (lce_hip_status s = DevicePtr(op.inputs[0], (noun + " input").c_str(), &in)) return s;
    const float *c1 = nullptr, *c2 = nullptr;
    if (constants >= 1)
      if (lce_hip_status s = ConstOnDevice(model, op.inputs[1], stream, capturing, &c1)) return s;
    if (constants >= 2 && op.inputs.size() == 3 && op.inputs[2] >= 0)
      if (lce_hip_status s = ConstOnDevice(model, op.inputs[2], stream, capturing, &c2)) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    if (lce_hip_status s = launch(in, (const void*)c1, (const void*)c2, out, (int32_t*)bits)) return s;
    return Launched(model->absorbed[i], fold);
  }
  // The output of a pass at this walk's batch.
  Shape OutShape(int32_t h, int32_t w, int32_t c, int type = lce_tfl::kTensorFloat32) const {
    Shape os;
    os.dims[0] = batch; os.dims[1] = h; os.dims[2] = w; os.dims[3] = c;
    os.type = type;
    return os;
  }

  // ---- the windowed passes: the entry's own *_check of the descriptor at this walk's batch gives the output's height and width ----
  // An absorbed AVERAGE_POOL_2D / MAX_POOL_2D (LCE_TFLITE_SECTIONS_EXT_POOL) as ONE lce_hip_pool2d launch -- unless "transition" is
  // named and the pool is the front of a transition (Transition, below).
  lce_hip_status Pool2d(int32_t i) {
    const lce_tfl::Operator& op = model->m.operators[i];
    const lce_tfl::Tensor& in = model->m.tensors[op.inputs[0]];
    const lce_hip_pool2d_desc d = PoolDesc(model->m, op, batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_pool2d_check(&d, &h, &w)) return s;
    const int32_t reader = TransitionReader(i, d);
    if (reader >= 0) return Transition(i, reader, d);
    return OnePass(i, "a pool", in.type, OutShape(h, w, in.shape[3], in.type), /*fold_quantize=*/true, /*constants=*/0,
                   [&](const void* x, const void*, const void*, void* out, int32_t* bits) { return lce_hip_pool2d(&d, x, out, bits, stream); });
  }

  // ---- a transition's pool and blur as one launch ("transition" of lce_tflite_model_open_passes) ----
  // The DEPTHWISE_CONV_2D that takes pool `i` (descriptor `d`) into its launch, or -1: the name is given and the pool is a float
  // MAX pool; the pooled tensor is not delivered and has exactly one reader; that reader is an absorbed float depthwise convolution
  // in this section that has not run and reads the pooled tensor as its input; and the fused entry's own check accepts the two
  // descriptors (which compares the shapes).  Decided from the graph and the descriptors alone, so a walk without launches decides
  // as a run does.
  // An int8 pair is left as two launches: lce_hip_pool_depthwise_i8 measured 1.09 - 1.24 of the two launches' time at QuickNet's
  // three transitions (profiles/transition/layers.txt; the float entry 0.82 - 0.94).  The rule is: a type is fused here only if
  // its fused launch is faster at all three shapes by more than the larger leg's spread.
  int32_t TransitionReader(int32_t i, const lce_hip_pool2d_desc& d) const {
    if (!(model->flags_int & kInternalTransition) || d.op != LCE_HIP_POOL_MAX || d.type != LCE_HIP_F32) return -1;
    const lce_tfl::Model& M = model->m;
    const int32_t pooled_t = M.operators[i].outputs[0];
    const int32_t r = OnlyReader(pooled_t, i);
    if (r < 0 || done[r] || model->absorbed[r] != kAbsorbedDepthwise) return -1;
    const lce_tfl::Operator& dw = M.operators[r];
    if (dw.inputs.empty() || dw.inputs[0] != pooled_t) return -1;
    const lce_hip_depthwise_desc dd = DepthwiseDesc(M, dw, batch);
    return lce_hip_pool_depthwise_f32_check(&d, &dd, nullptr, nullptr) == LCE_HIP_OK ? r : -1;
  }
  // Pool `i` and the depthwise convolution `r` that alone reads it as ONE lce_hip_pool_depthwise_f32 launch.  Both operators are
  // marked done; the pooled tensor exists in registers only, so the walk holds no tensor of that name
  // (lce_tflite_model_section_tensor_shape refuses it).  The first LceQuantize of the section that reads the blurred map folds in as
  // it folds into the depthwise walker's launch.  The launch is counted by lce_tflite_model_transition_stats and by neither
  // operator's own pass.
  lce_hip_status Transition(int32_t i, int32_t r, const lce_hip_pool2d_desc& d) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator &op = M.operators[i], &dw = M.operators[r];
    int32_t want[4];
    auto it = shapes.find(op.inputs[0]);
    if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: a pool reads a tensor nothing produced");
    if (!Carried(M.tensors[op.inputs[0]], want) || !Agrees(it->second, lce_tfl::kTensorFloat32, want[1], want[2], want[3]))
      return Fail(LCE_HIP_ERR_INVALID, "run_section: a pool input's shape or type does not match the one its producer infers");
    const lce_hip_depthwise_desc dd = DepthwiseDesc(M, dw, batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_pool_depthwise_f32_check(&d, &dd, &h, &w)) return s;
    const int32_t out_t = dw.outputs[0];
    const Shape os = OutShape(h, w, M.tensors[dw.inputs[1]].shape[3]);
    shapes.erase(op.outputs[0]);
    shapes[out_t] = os;
    done[i] = done[r] = 1;
    const Fold fold = FoldQuantize(r, out_t, os);
    if (!run) return LCE_HIP_OK;
    const void* in = nullptr;
    if (lce_hip_status s = DevicePtr(op.inputs[0], "a pool input", &in)) return s;
    const float *filter = nullptr, *bias = nullptr;
    if (lce_hip_status s = ConstOnDevice(model, dw.inputs[1], stream, capturing, &filter)) return s;
    if (dw.inputs.size() == 3 && dw.inputs[2] >= 0)
      if (lce_hip_status s = ConstOnDevice(model, dw.inputs[2], stream, capturing, &bias)) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    if (lce_hip_status s = lce_hip_pool_depthwise_f32(&d, &dd, (const float*)in, filter, bias, (float*)out, (int32_t*)bits, stream)) return s;
    ++model->last.transition_launches;
    model->last.transition_ops += 2;
    if (fold.bits_t >= 0) ++model->last.transition_quantize;
    return LCE_HIP_OK;
  }

  // An absorbed float 1x1 CONV_2D (LCE_TFLITE_SECTIONS_EXT_CONV1X1) as ONE lce_hip_conv1x1_f32 launch.
  lce_hip_status Conv1x1(int32_t i) {
    const lce_hip_conv1x1_desc d = Conv1x1Desc(model->m, model->m.operators[i], batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_conv1x1_f32_check(&d, &h, &w)) return s;
    return OnePass(i, "a CONV_2D", lce_tfl::kTensorFloat32, OutShape(h, w, d.channels_out), /*fold_quantize=*/true, /*constants=*/2,
                   [&](const void* x, const void* filter, const void* bias, void* out, int32_t* bits) {
                     return lce_hip_conv1x1_f32(&d, (const float*)x, (const float*)filter, (const float*)bias, (float*)out, bits, stream);
                   });
  }

  // An absorbed float DEPTHWISE_CONV_2D (LCE_TFLITE_SECTIONS_EXT_DEPTHWISE) as ONE lce_hip_depthwise_conv2d_f32 launch.
  lce_hip_status Depthwise(int32_t i) {
    const lce_tfl::Operator& op = model->m.operators[i];
    const lce_hip_depthwise_desc d = DepthwiseDesc(model->m, op, batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_depthwise_conv2d_f32_check(&d, &h, &w)) return s;
    return OnePass(i, "a DEPTHWISE_CONV_2D", lce_tfl::kTensorFloat32, OutShape(h, w, model->m.tensors[op.inputs[1]].shape[3]),
                   /*fold_quantize=*/true, /*constants=*/2,
                   [&](const void* x, const void* filter, const void* bias, void* out, int32_t* bits) {
                     return lce_hip_depthwise_conv2d_f32(&d, (const float*)x, (const float*)filter, (const float*)bias, (float*)out, bits, stream);
                   });
  }

  // An absorbed float CONV_2D of any filter extent (LCE_TFLITE_SECTIONS_EXT_CONV2D) as ONE lce_hip_conv2d_f32 call.
  lce_hip_status Conv2d(int32_t i) {
    const lce_hip_conv2d_desc d = Conv2dDesc(model->m, model->m.operators[i], batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_conv2d_f32_check(&d, &h, &w)) return s;
    return OnePass(i, "a CONV_2D", lce_tfl::kTensorFloat32, OutShape(h, w, d.channels_out), /*fold_quantize=*/true, /*constants=*/2,
                   [&](const void* x, const void* filter, const void* bias, void* out, int32_t* bits) {
                     return lce_hip_conv2d_f32(&d, (const float*)x, (const float*)filter, (const float*)bias, (float*)out, bits, stream);
                   });
  }

  // The table Partition() had an entry's prepare make of the constants of operator `i` (`noun`), on the device: uploaded once per
  // model, where the filters are.
  lce_hip_status TableOnDevice(int32_t i, const char* noun, const int32_t** out) {
    lce_tflite_model::DevBuf& b = model->tables[i];
    if (!b.ptr) {
      if (capturing) return Fail(LCE_HIP_ERR_INVALID, "run_section: a constant would have to be uploaded during graph capture");
      auto prepared = model->host_tables.find(i);
      if (prepared == model->host_tables.end()) return Fail(LCE_HIP_ERR_INVALID, std::string("run_section: ") + noun + " without a prepared table");
      const std::vector<int32_t>& table = prepared->second;
      // (the buffer becomes the model's only once the copy has completed: a failed upload leaves nothing a later run would launch on)
      void* dev = nullptr;
      if (lce_hip_status s = lce_hip_malloc(&dev, table.size() * 4)) return s;
      lce_hip_status s = lce_hip_memcpy_h2d(dev, table.data(), table.size() * 4, stream);
      if (s == LCE_HIP_OK) s = lce_hip_stream_synchronize(stream);
      if (s != LCE_HIP_OK) {
        lce_hip_free(dev);
        return s;
      }
      b.ptr = dev;
      b.bytes = table.size() * 4;
      model->host_tables.erase(prepared);
    }
    *out = (const int32_t*)b.ptr;
    return LCE_HIP_OK;
  }

  // An absorbed int8 CONV_2D of any filter extent ("conv2d_i8" of lce_tflite_model_open_passes) as ONE lce_hip_conv2d_i8 launch.
  // The table the row's prepare step made of the file's constants is uploaded once per model, where the filters are (the int32
  // bias is uploaded beside the filter, though the entry reads the table's copy).
  lce_hip_status ConvI8(int32_t i) {
    const lce_hip_conv2d_i8_desc d = ConvI8Desc(model->m, model->m.operators[i], batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_conv2d_i8_check(&d, &h, &w)) return s;
    return OnePass(i, "an int8 CONV_2D", lce_tfl::kTensorInt8, OutShape(h, w, d.channels_out, lce_tfl::kTensorInt8), /*fold_quantize=*/true,
                   /*constants=*/2, [&](const void* x, const void* filter, const void*, void* out, int32_t* bits) -> lce_hip_status {
                     const int32_t* table = nullptr;
                     if (lce_hip_status s = TableOnDevice(i, "an int8 CONV_2D", &table)) return s;
                     return lce_hip_conv2d_i8(&d, (const int8_t*)x, (const int8_t*)filter, table, (int8_t*)out, bits, stream);
                   });
  }

  // An absorbed int8 DEPTHWISE_CONV_2D ("depthwise_i8" of lce_tflite_model_open_passes) as ONE lce_hip_depthwise_conv2d_i8 launch; its
  // table is uploaded once per model, as the int8 CONV_2D's.
  lce_hip_status DepthwiseI8(int32_t i) {
    const lce_tfl::Operator& op = model->m.operators[i];
    const lce_hip_depthwise_i8_desc d = DepthwiseI8Desc(model->m, op, batch);
    int32_t h = 0, w = 0;
    if (lce_hip_status s = lce_hip_depthwise_conv2d_i8_check(&d, &h, &w)) return s;
    return OnePass(i, "an int8 DEPTHWISE_CONV_2D", lce_tfl::kTensorInt8,
                   OutShape(h, w, model->m.tensors[op.inputs[1]].shape[3], lce_tfl::kTensorInt8), /*fold_quantize=*/true, /*constants=*/2,
                   [&](const void* x, const void* filter, const void*, void* out, int32_t* bits) -> lce_hip_status {
                     const int32_t* table = nullptr;
                     if (lce_hip_status s = TableOnDevice(i, "an int8 DEPTHWISE_CONV_2D", &table)) return s;
                     return lce_hip_depthwise_conv2d_i8(&d, (const int8_t*)x, (const int8_t*)filter, table, (int8_t*)out, bits, stream);
                   });
  }

  // ---- the classifier head ("head" of lce_tflite_model_open_passes).  Rank-2 tensors are carried as [batch, 1, 1, C]; no
  // LceQuantize folds into a head operator. ----
  // An absorbed MEAN over height and width as ONE lce_hip_pool2d launch: the AVERAGE pool whose filter is the image.
  lce_hip_status Mean(int32_t i) {
    const lce_hip_pool2d_desc d = MeanDesc(model->m, model->m.operators[i], batch);
    int32_t oh = 0, ow = 0;
    if (lce_hip_status s = lce_hip_pool2d_check(&d, &oh, &ow)) return s;
    return OnePass(i, "a MEAN", lce_tfl::kTensorFloat32, OutShape(oh, ow, d.channels), /*fold_quantize=*/false, /*constants=*/0,
                   [&](const void* x, const void*, const void*, void* out, int32_t*) { return lce_hip_pool2d(&d, x, out, nullptr, stream); });
  }

  // An absorbed float FULLY_CONNECTED as ONE lce_hip_fully_connected_f32 launch.
  lce_hip_status FullyConnected(int32_t i) {
    const lce_hip_fc_desc d = FullyConnectedDesc(model->m, model->m.operators[i], batch);
    if (lce_hip_status s = lce_hip_fully_connected_f32_check(&d)) return s;
    return OnePass(i, "a FULLY_CONNECTED", lce_tfl::kTensorFloat32, OutShape(1, 1, d.outputs), /*fold_quantize=*/false, /*constants=*/2,
                   [&](const void* x, const void* weights, const void* bias, void* out, int32_t*) {
                     return lce_hip_fully_connected_f32(&d, (const float*)x, (const float*)weights, (const float*)bias, (float*)out, stream);
                   });
  }

  // An absorbed binarized Dense layer ("binary_dense" of lce_tflite_model_open_passes) as ONE lce_hip_binary_fully_connected launch
  // on the BIT tensor its LceDequantize reads; the dequantized floats are never read.  The first LceQuantize of the section that
  // reads the result folds into the launch (a hidden binary Dense layer then writes only bits).  The table Partition() had
  // lce_hip_bfc_prepare make of the file's weights -- sign bits, then scales -- is uploaded once per model.
  lce_hip_status BinaryDense(int32_t i) {
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t out_t = op.outputs[0];
    const lce_hip_bfc_desc d = BinaryDenseDesc(M, op, batch);
    if (lce_hip_status s = lce_hip_bfc_check(&d)) return s;
    const int32_t bits_t = BinaryDenseSource(M, op, model->producer[op.inputs[0]]);
    if (bits_t < 0) return Fail(LCE_HIP_ERR_INVALID, "run_section: a binary FULLY_CONNECTED without an LceDequantize in front of it");
    // the inferred shape and type of the bits must agree with the file's (a producer whose output is smaller than the file
    // declares must not be read past its buffer)
    auto it = shapes.find(bits_t);
    if (it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: a binary FULLY_CONNECTED reads bits nothing produced");
    if (!Agrees(it->second, lce_tfl::kTensorInt32, 1, 1, (d.inputs + 31) / 32))
      return Fail(LCE_HIP_ERR_INVALID, "run_section: a binary FULLY_CONNECTED's bits do not have the shape or type their producer infers");
    const Shape os = OutShape(1, 1, d.outputs);
    shapes[out_t] = os;
    done[i] = 1;
    const Fold fold = FoldQuantize(i, out_t, os);
    if (!run) return LCE_HIP_OK;
    const void* in = nullptr;
    if (lce_hip_status s = DevicePtr(bits_t, "a binary FULLY_CONNECTED's bits", &in)) return s;
    const int32_t* table = nullptr;
    if (lce_hip_status s = TableOnDevice(i, "a binary FULLY_CONNECTED", &table)) return s;
    const float* bias = nullptr;
    if (op.inputs.size() == 3 && op.inputs[2] >= 0)
      if (lce_hip_status s = ConstOnDevice(model, op.inputs[2], stream, capturing, &bias)) return s;
    void *out, *bits;
    if (lce_hip_status s = FoldBuffers(fold, &out, &bits)) return s;
    const size_t words = (size_t)d.outputs * (size_t)((d.inputs + 31) / 32);
    if (lce_hip_status s = lce_hip_binary_fully_connected(&d, (const int32_t*)in, table, (const float*)(table + words), bias, (float*)out,
                                                          (int32_t*)bits, stream))
      return s;
    return Launched(kAbsorbedBinaryDense, fold);
  }

  // An absorbed float SOFTMAX as ONE lce_hip_softmax_f32 launch.
  lce_hip_status Softmax(int32_t i) {
    const lce_tfl::Operator& op = model->m.operators[i];
    int32_t id[4];
    if (!Carried(model->m.tensors[op.inputs[0]], id)) return Fail(LCE_HIP_ERR_INVALID, "run_section: a SOFTMAX of a rank that is neither 2 nor 4");
    if (lce_hip_status s = lce_hip_softmax_f32_check((size_t)batch, (size_t)id[3], op.softmax_beta)) return s;
    return OnePass(i, "a SOFTMAX", lce_tfl::kTensorFloat32, OutShape(1, 1, id[3]), /*fold_quantize=*/false, /*constants=*/0,
                   [&](const void* x, const void*, const void*, void* out, int32_t*) {
                     return lce_hip_softmax_f32((size_t)batch, (size_t)id[3], op.softmax_beta, (const float*)x, (float*)out, stream);
                   });
  }

  // ---- the int8 head and the float / int8 boundary ("head_i8" and "quantize" of lce_tflite_model_open_passes) ----
  // An absorbed int8 MEAN over height and width as ONE lce_hip_mean_i8 launch.
  lce_hip_status MeanI8(int32_t i) {
    const lce_hip_mean_i8_desc d = MeanI8Desc(model->m, model->m.operators[i], batch);
    if (lce_hip_status s = lce_hip_mean_i8_check(&d)) return s;
    return OnePass(i, "an int8 MEAN", lce_tfl::kTensorInt8, OutShape(1, 1, d.channels, lce_tfl::kTensorInt8), /*fold_quantize=*/false,
                   /*constants=*/0, [&](const void* x, const void*, const void*, void* out, int32_t*) {
                     return lce_hip_mean_i8(&d, (const int8_t*)x, (int8_t*)out, stream);
                   });
  }

  // An absorbed int8 FULLY_CONNECTED as ONE lce_hip_fully_connected_i8 launch; its bias lives in the prepared table.
  lce_hip_status FullyConnectedI8(int32_t i) {
    const lce_hip_fc_i8_desc d = FullyConnectedI8Desc(model->m, model->m.operators[i], batch);
    if (lce_hip_status s = lce_hip_fully_connected_i8_check(&d)) return s;
    return OnePass(i, "an int8 FULLY_CONNECTED", lce_tfl::kTensorInt8, OutShape(1, 1, d.outputs, lce_tfl::kTensorInt8), /*fold_quantize=*/false,
                   /*constants=*/1, [&](const void* x, const void* weights, const void*, void* out, int32_t*) -> lce_hip_status {
                     const int32_t* table = nullptr;
                     if (lce_hip_status s = TableOnDevice(i, "an int8 FULLY_CONNECTED", &table)) return s;
                     return lce_hip_fully_connected_i8(&d, (const int8_t*)x, (const int8_t*)weights, table, (int8_t*)out, stream);
                   });
  }

  // An absorbed int8 SOFTMAX as ONE lce_hip_softmax_i8 launch.
  lce_hip_status SoftmaxI8(int32_t i) {
    const lce_tfl::Operator& op = model->m.operators[i];
    const lce_tfl::Tensor& in = model->m.tensors[op.inputs[0]];
    const lce_tfl::Tensor& out = model->m.tensors[op.outputs[0]];
    int32_t id[4];
    if (!Carried(in, id)) return Fail(LCE_HIP_ERR_INVALID, "run_section: a SOFTMAX of a rank that is neither 2 nor 4");
    if (lce_hip_status s = lce_hip_softmax_i8_check((size_t)batch, (size_t)id[3], in.scale, op.softmax_beta, out.scale, (int32_t)out.zero_point)) return s;
    return OnePass(i, "an int8 SOFTMAX", lce_tfl::kTensorInt8, OutShape(1, 1, id[3], lce_tfl::kTensorInt8), /*fold_quantize=*/false,
                   /*constants=*/0, [&](const void* x, const void*, const void*, void* o, int32_t*) {
                     return lce_hip_softmax_i8((size_t)batch, (size_t)id[3], in.scale, op.softmax_beta, out.scale, (int32_t)out.zero_point,
                                               (const int8_t*)x, (int8_t*)o, stream);
                   });
  }

  // An absorbed QUANTIZE (float32 -> int8) or DEQUANTIZE (int8 -> float32) as ONE launch over the tensor's elements.
  lce_hip_status Boundary(int32_t i, bool to_int8) {
    const lce_tfl::Operator& op = model->m.operators[i];
    const lce_tfl::Tensor& q = model->m.tensors[to_int8 ? op.outputs[0] : op.inputs[0]];
    int32_t id[4];
    if (!Carried(model->m.tensors[op.inputs[0]], id)) return Fail(LCE_HIP_ERR_INVALID, "run_section: a QUANTIZE / DEQUANTIZE of a rank that is neither 2 nor 4");
    const size_t n = (size_t)batch * (size_t)id[1] * (size_t)id[2] * (size_t)id[3];
    const float scale = q.scale;
    const int32_t zp = (int32_t)q.zero_point;
    if (to_int8)
      return OnePass(i, "a QUANTIZE", lce_tfl::kTensorFloat32, OutShape(id[1], id[2], id[3], lce_tfl::kTensorInt8), /*fold_quantize=*/false,
                     /*constants=*/0, [&](const void* x, const void*, const void*, void* out, int32_t*) {
                       return lce_hip_quantize_f32_i8(n, scale, zp, (const float*)x, (int8_t*)out, stream);
                     });
    return OnePass(i, "a DEQUANTIZE", lce_tfl::kTensorInt8, OutShape(id[1], id[2], id[3]), /*fold_quantize=*/false, /*constants=*/0,
                   [&](const void* x, const void*, const void*, void* out, int32_t*) {
                     return lce_hip_dequantize_i8_f32(n, scale, zp, (const int8_t*)x, (float*)out, stream);
                   });
  }
  lce_hip_status QuantizeF32I8(int32_t i) { return Boundary(i, true); }
  lce_hip_status DequantizeI8F32(int32_t i) { return Boundary(i, false); }

  // The four LCE operators.  `in` is the inferred shape of operator `i`'s first input, `in_dev` its device pointer (with `run`).
  lce_hip_status Quantize(int32_t i, const Shape& in, const void* in_dev) {                      // quantization.cc:19-41,76-114
    const lce_tfl::Operator& op = model->m.operators[i];
    if (in.type != lce_tfl::kTensorFloat32 && in.type != lce_tfl::kTensorInt8 && in.type != lce_tfl::kTensorBool)
      return Fail(LCE_HIP_ERR_INVALID, "LceQuantize: input must be float32, int8 or bool");
    Shape out = in;
    out.dims[3] = (in.dims[3] + 31) / 32;
    out.type = lce_tfl::kTensorInt32;
    shapes[op.outputs[0]] = out;
    if (!run) return LCE_HIP_OK;
    void* o = nullptr;
    if (lce_hip_status s = BufferFor(op.outputs[0], out.bytes(), &o)) return s;
    const lce_hip_dtype t = in.type == lce_tfl::kTensorFloat32 ? LCE_HIP_F32 : in.type == lce_tfl::kTensorInt8 ? LCE_HIP_I8 : LCE_HIP_BOOL;
    const int32_t zp = in.type == lce_tfl::kTensorInt8 ? (int32_t)model->m.tensors[op.inputs[0]].zero_point : in.type == lce_tfl::kTensorBool ? 1 : 0;
    return lce_hip_bitpack(t, in_dev, (size_t)in.dims[0] * in.dims[1] * in.dims[2], (size_t)in.dims[3], zp, (int32_t*)o, stream);
  }

  lce_hip_status Dequantize(int32_t i, const Shape& in, const void* in_dev) {                    // quantization.cc:43-74,116-147
    const lce_tfl::Operator& op = model->m.operators[i];
    const lce_tfl::Tensor& OT = model->m.tensors[op.outputs[0]];
    // (any rank in the reference, quantization.cc:55-66; here rank 4, or rank 2 carried as [b, 1, 1, C] like every rank-2 tensor of the walk)
    int32_t od[4];
    if (!Carried(OT, od)) return Fail(LCE_HIP_ERR_UNSUPPORTED, "LceDequantize: the output's channel count comes from the file (2-D or 4-D)");
    Shape out = in;
    out.type = OT.type;
    out.dims[3] = od[3];
    if ((out.dims[3] + 31) / 32 != in.dims[3]) return Fail(LCE_HIP_ERR_INVALID, "LceDequantize: output channels do not match the packed input");
    shapes[op.outputs[0]] = out;
    // Binary Dense layers read the BITS.  When they, in this section, are the only readers and the section does not deliver the
    // floats, nothing reads them: no launch and no buffer (the shape stays registered)
    bool skip = !IsSectionOutput(op.outputs[0]) && !model->readers[op.outputs[0]].empty();
    for (int32_t r : model->readers[op.outputs[0]])
      skip = skip && model->absorbed[r] == kAbsorbedBinaryDense && std::binary_search(sec.ops.begin(), sec.ops.end(), r);
    if (skip) {
      if (run) ++model->last.dequantize_skipped;
      return LCE_HIP_OK;
    }
    if (!run) return LCE_HIP_OK;
    void* o = nullptr;
    if (lce_hip_status s = BufferFor(op.outputs[0], out.bytes(), &o)) return s;
    const lce_hip_dtype t = out.type == lce_tfl::kTensorFloat32 ? LCE_HIP_F32 : out.type == lce_tfl::kTensorInt8 ? LCE_HIP_I8 : LCE_HIP_BOOL;
    return lce_hip_unpack(t, (const int32_t*)in_dev, (size_t)out.dims[0] * out.dims[1] * out.dims[2], (size_t)out.dims[3],
                          OT.quantized ? OT.scale : 1.0f, OT.quantized ? (int32_t)OT.zero_point : 0, o, stream);
  }

  lce_hip_status BMaxPool2d(int32_t i, const Shape& in, const void* in_dev) {                    // bmaxpool.cc:20-91
    const lce_tfl::Operator& op = model->m.operators[i];
    if (in.type != lce_tfl::kTensorInt32) return Fail(LCE_HIP_ERR_INVALID, "LceBMaxPool2d: input must be bitpacked int32");
    const lce_flex::Map fm(op.custom_options, op.custom_options_size);
    if (!fm.valid()) return Fail(LCE_HIP_ERR_INVALID, "LceBMaxPool2d: unreadable options");
    const int32_t fh = fm.AsInt32("filter_height"), fw = fm.AsInt32("filter_width"), sh = fm.AsInt32("stride_height"),
                  sw = fm.AsInt32("stride_width"), pad = fm.AsInt32("padding");
    Shape out = in;
    out.type = model->m.tensors[op.outputs[0]].type;
    if (lce_hip_status s = lce_hip_bmaxpool_output_shape(in.dims[1], in.dims[2], fh, fw, sh, sw, pad, &out.dims[1], &out.dims[2])) return s;
    shapes[op.outputs[0]] = out;
    if (!run) return LCE_HIP_OK;
    void* o = nullptr;
    if (lce_hip_status s = BufferFor(op.outputs[0], out.bytes(), &o)) return s;
    return lce_hip_bmaxpool((const int32_t*)in_dev, in.dims[0], in.dims[1], in.dims[2], in.dims[3], fh, fw, sh, sw, pad, (int32_t*)o, stream);
  }

  lce_hip_status Bconv2d(int32_t i, const Shape& in, const void* in_dev) {                       // bconv2d.cc:137-300,550-564
    const lce_tfl::Model& M = model->m;
    const lce_tfl::Operator& op = M.operators[i];
    const int32_t out_t = op.outputs[0];
    // The plan is built from the FILE's static shape of the input tensor (lce_tflite_model_bconv2d_plan); the buffer it will
    // read was sized from THIS walk's shape inference.  A model whose declared shapes disagree with what its operators
    // produce (dynamic / -1 dimensions, a hand-edited file, an int8 tensor wired into a convolution) must fail here, not read
    // past a scratch buffer on the device: the file is untrusted input.
    const std::vector<int32_t>& is = M.tensors[op.inputs[0]].shape;
    if (in.type != lce_tfl::kTensorInt32)
      return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: the tensor feeding the convolution is not bitpacked int32");
    if (is.size() != 4 || !Agrees(in, lce_tfl::kTensorInt32, is[1], is[2], is[3]))
      return Fail(LCE_HIP_ERR_INVALID, "LceBconv2d: the input tensor's declared shape does not match the shape its producer infers");
    lce_hip_bconv2d_plan* plan = nullptr;
    if (lce_hip_status s = PlanFor(model, i, batch, semantics, &plan)) return s;
    Shape out = in;
    out.type = M.tensors[out_t].type;
    if (lce_hip_status s = lce_hip_bconv2d_plan_output_shape(plan, out.dims)) return s;
    shapes[out_t] = out;
    // (not the fold rule of the passes above: EVERY LceQuantize reading the output gets its shape here, the first one's launch
    // disappears, and the convolution's own output is always written)
    const std::vector<int32_t> fused = QuantizeConsumers(model, sec, i);
    for (int32_t j : fused) {
      Shape q = out;
      q.dims[3] = (out.dims[3] + 31) / 32;
      q.type = lce_tfl::kTensorInt32;
      shapes[M.operators[j].outputs[0]] = q;
    }
    if (!fused.empty()) done[fused[0]] = 1;
    if (!run) return LCE_HIP_OK;
    void* o = nullptr;
    if (lce_hip_status s = BufferFor(out_t, out.bytes(), &o)) return s;
    if (fused.empty()) return lce_hip_bconv2d_run(plan, (const int32_t*)in_dev, o, stream);
    void* bits = nullptr;
    const int32_t bits_t = M.operators[fused[0]].outputs[0];
    if (lce_hip_status s = BufferFor(bits_t, shapes[bits_t].bytes(), &bits)) return s;
    if (lce_hip_status s = lce_hip_bconv2d_run_dual(plan, (const int32_t*)in_dev, o, (int32_t*)bits, stream)) return s;
    ++model->last.conv_quantize;
    return LCE_HIP_OK;
  }

  lce_hip_status LceOp(int32_t i) {
    const lce_tfl::Operator& op = model->m.operators[i];
    if (op.inputs.empty() || op.outputs.size() != 1 || op.inputs[0] < 0)
      return Fail(LCE_HIP_ERR_INVALID, "run_section: malformed LCE operator");
    auto in_it = shapes.find(op.inputs[0]);
    if (in_it == shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "run_section: an operator reads a tensor nothing produced");
    const Shape in = in_it->second;
    const void* in_dev = nullptr;
    if (run)
      if (lce_hip_status s = DevicePtr(op.inputs[0], "an input tensor", &in_dev)) return s;
    if (op.custom_code == "LceQuantize") return Quantize(i, in, in_dev);
    if (op.custom_code == "LceDequantize") return Dequantize(i, in, in_dev);
    if (op.custom_code == "LceBMaxPool2d") return BMaxPool2d(i, in, in_dev);
    if (op.custom_code == "LceBconv2d") return Bconv2d(i, in, in_dev);
    return Fail(LCE_HIP_ERR_UNSUPPORTED, "run_section: operator " + op.custom_code + " is not an LCE op");
  }

  lce_hip_status Section() {
    const lce_tfl::Model& M = model->m;
    for (int32_t t : sec.inputs) {
      const lce_tfl::Tensor& T = M.tensors[t];
      Shape sh;
      // (a rank-2 input -- of a head that starts behind a host operator -- is carried as [batch, 1, 1, C])
      if (T.shape.size() == 2 && model->rank2_inputs) {
        if (!Carried(T, sh.dims)) return Fail(LCE_HIP_ERR_INVALID, "run_section: a section input with an extent that is not positive");
      } else {
        if (T.shape.size() != 4) return Fail(LCE_HIP_ERR_UNSUPPORTED, "run_section: section inputs must be 4-D tensors (NHWC)");
        for (int k = 0; k < 4; ++k) sh.dims[k] = T.shape[k];
      }
      sh.dims[0] = batch;
      sh.type = T.type;
      shapes[t] = sh;
    }
    done = std::vector<char>(M.operators.size(), 0);
    for (int32_t i : sec.ops) {
      if (done[i]) continue;
      const int kind = model->absorbed[i];
      if (lce_hip_status s = kind ? (this->*kPasses[kind - 1].walker)(i) : LceOp(i)) return s;
    }
    return LCE_HIP_OK;
  }
};

// THE table of fused passes, in priority order (the first enabled row whose predicate holds and whose prepare step accepts takes
// the operator) and in the order of the kinds (row k is kind k + 1).  A new pass is a row here, a predicate built from the helpers
// above, a walker that ends in FoldQuantize / FoldBuffers / Launched, and an exported *_stats.  Columns: kind, name, predicate,
// walker, prepare step, queued as an LCE operator, reads rank-2 tensors (FusedPass).
// A row whose prepare step refuses hands the operator to the rows below it.  For the binary Dense row that is the point: the head's
// FULLY_CONNECTED row takes what it refuses.  For the three int8 rows it is the same as leaving the operator with the host, because
// every predicate begins with its builtin code and no row below accepts theirs: below the int8 CONV_2D row stand DEPTHWISE_CONV_2D,
// MEAN, FULLY_CONNECTED, SOFTMAX, QUANTIZE, DEQUANTIZE, the activations, RESHAPE and ADD / MUL (the gate); below the int8
// DEPTHWISE_CONV_2D row the same without the first; below the int8 FULLY_CONNECTED row SOFTMAX and what follows it.
constexpr bool kAsLce = true, kRank2 = true;
constexpr FusedPass kPasses[kAbsorbedCount - 1] = {
    {kAbsorbedElementwise, Named("elementwise"), ElementwiseCandidate, &Walk::ElementwiseChain, nullptr, false, false},
    {kAbsorbedInt8Add, Named("int8_add"), Int8AddCandidate, &Walk::Int8Add, nullptr, false, false},
    {kAbsorbedConcat, Named("concat"), ConcatCandidate, &Walk::Concat, nullptr, false, false},
    {kAbsorbedPool, Named("pool"), PoolCandidate, &Walk::Pool2d, nullptr, false, false},
    {kAbsorbedConv1x1, Named("conv1x1"), Conv1x1Candidate, &Walk::Conv1x1, nullptr, false, false},
    {kAbsorbedDepthwise, Named("depthwise"), DepthwiseCandidate, &Walk::Depthwise, nullptr, false, false},
    // (Conv1x1Candidate is tried first: with both bits a 1x1 filter runs as before)
    {kAbsorbedConv2d, Named("conv2d"), Conv2dCandidate, &Walk::Conv2d, nullptr, false, false},
    // the quantized convolution: no float predicate takes an int8 tensor
    {kAbsorbedConvI8, Named("conv2d_i8"), ConvI8Candidate, &Walk::ConvI8, ConvI8Prepare, false, false},
    // the quantized depthwise convolution: DepthwiseCandidate above takes float tensors only
    {kAbsorbedDepthwiseI8, Named("depthwise_i8"), DepthwiseI8Candidate, &Walk::DepthwiseI8, DepthwiseI8Prepare, false, false},
    // the classifier head: one name enables the three rows.  MEAN reads an image; the Dense layer and the softmax may read [b, C]
    {kAbsorbedMean, Named("head"), MeanCandidate, &Walk::Mean, nullptr, kAsLce, false},
    // the binarized Dense layer: in front of the head's FULLY_CONNECTED row, which takes what this one refuses
    {kAbsorbedBinaryDense, Named("binary_dense"), BinaryDenseCandidate, &Walk::BinaryDense, BinaryDensePrepare, kAsLce, kRank2},
    {kAbsorbedFullyConnected, Named("head"), FullyConnectedCandidate, &Walk::FullyConnected, nullptr, kAsLce, kRank2},
    {kAbsorbedSoftmax, Named("head"), SoftmaxCandidate, &Walk::Softmax, nullptr, kAsLce, kRank2},
    // the int8 head and the float / int8 boundary: no float predicate above takes an int8 MEAN / FULLY_CONNECTED / SOFTMAX and
    // none of these takes a float one, so the two heads never compete
    {kAbsorbedMeanI8, Named("head_i8"), MeanI8Candidate, &Walk::MeanI8, nullptr, kAsLce, false},
    {kAbsorbedFullyConnectedI8, Named("head_i8"), FullyConnectedI8Candidate, &Walk::FullyConnectedI8, FullyConnectedI8Prepare, kAsLce, kRank2},
    {kAbsorbedSoftmaxI8, Named("head_i8"), SoftmaxI8Candidate, &Walk::SoftmaxI8, nullptr, kAsLce, kRank2},
    {kAbsorbedQuantize, Named("quantize"), QuantizeCandidate, &Walk::QuantizeF32I8, nullptr, false, kRank2},
    {kAbsorbedDequantize, Named("quantize"), DequantizeCandidate, &Walk::DequantizeI8F32, nullptr, false, kRank2},
    // the standalone activations and the per-image gate are steps of the elementwise chain, so their walker is the chain's;
    // ElementwiseCandidate above takes no ADD / MUL with a non-constant [b,1,1,C] input on a larger image, and where the image is
    // 1 x 1 the gate is a tensor operand like any other.  RESHAPE launches nothing.
    {kAbsorbedActivation, Named("activation"), ActivationCandidate, &Walk::ElementwiseChain, nullptr, false, kRank2},
    {kAbsorbedReshape, Named("reshape"), ReshapeCandidate, &Walk::Reshape, nullptr, false, kRank2},
    {kAbsorbedGate, Named("gate"), GateCandidate, &Walk::ElementwiseChain, nullptr, false, false},
    // the channel window of MeliusNet's improvement block: no row above takes a STRIDED_SLICE / SLICE
    {kAbsorbedSlice, Named("slice"), SliceCandidate, &Walk::Slice, nullptr, false, false},
    // the int8 tail of a ReActNet block: no row above takes an int8 ADD with a constant operand (the residual ADD's row wants two
    // tensors), an int8 PRELU or RELU (the activation row is float) or an int8 -> int8 QUANTIZE (the quantize row wants a float input)
    {kAbsorbedElementwiseI8, Named("elementwise_i8"), ElementwiseI8Candidate, &Walk::ElementwiseI8, ElementwiseI8Prepare, false, false},
    // the int8 squeeze-and-excite gate: no row above takes an int8 LOGISTIC (the activation row is float) or an int8 MUL (the
    // elementwise and gate rows are float, the int8 chain's has no MUL step)
    {kAbsorbedLogisticI8, Named("gate_i8"), LogisticI8Candidate, &Walk::LogisticI8, LogisticI8Prepare, false, kRank2},
    {kAbsorbedMulI8, Named("gate_i8"), MulI8Candidate, &Walk::MulI8, nullptr, false, false},
};
// (row k is kind k + 1, and every row names an entry of kPassNames)
constexpr bool RowsInOrder() {
  for (int k = 0; k < kAbsorbedCount - 1; ++k)
    if (kPasses[k].kind != k + 1 || !kPasses[k].name) return false;
  return true;
}
static_assert(RowsInOrder(), "kPasses");

// The *_stats exports: `read` copies counters of the last run, under the model's lock, into the pointers that are not null.
template <class Read>
void Stats(lce_tflite_model* model, Read read) {
  if (!model) return;
  std::lock_guard<std::mutex> lock(model->run_mu);
  read(model->last);
}
void Put(int32_t* out, int32_t value) {
  if (out) *out = value;
}
using RunStats = lce_tflite_model::RunStats;
// (launches of pass `kind`, LceQuantize launches folded into them): what most passes report
void LaunchStats(lce_tflite_model* model, int kind, int32_t* launches, int32_t* quantize_folded) {
  Stats(model, [&](const RunStats& r) { Put(launches, r.pass[kind].launches); Put(quantize_folded, r.pass[kind].quantize); });
}
}  // namespace

extern "C" {

lce_hip_status lce_tflite_model_section_tensor_shape(lce_tflite_model* model, int32_t section, int32_t tensor, int32_t batch,
                                                     int32_t semantics, int32_t dims[4], size_t* bytes) {
  g_model_error.clear();
  if (!model || section < 0 || section >= (int32_t)model->sections.size() || batch <= 0)
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_section_tensor_shape: bad argument");
  std::lock_guard<std::mutex> lock(model->run_mu);
  Walk w{model, model->sections[section], batch, semantics, /*run=*/false, /*stream=*/nullptr, /*capturing=*/false, {}, {}, {}};
  if (lce_hip_status s = w.Section()) return s;
  auto it = w.shapes.find(tensor);
  if (it == w.shapes.end()) return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_section_tensor_shape: the section does not touch this tensor");
  for (int k = 0; dims && k < 4; ++k) dims[k] = it->second.dims[k];
  if (bytes) *bytes = it->second.bytes();
  return LCE_HIP_OK;
}

lce_hip_status lce_tflite_model_run_section(lce_tflite_model* model, int32_t section, int32_t batch, int32_t semantics,
                                            const void* const* inputs_dev, void* const* outputs_dev, void* stream) {
  g_model_error.clear();
  if (!model || section < 0 || section >= (int32_t)model->sections.size() || batch <= 0 || !inputs_dev || !outputs_dev)
    return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_run_section: bad argument");
  const lce_tflite_section& sec = model->sections[section];
  std::lock_guard<std::mutex> lock(model->run_mu);
  std::map<int32_t, void*> ptr;
  for (size_t k = 0; k < sec.inputs.size(); ++k) {
    if (!inputs_dev[k]) return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_run_section: null input pointer");
    ptr[sec.inputs[k]] = const_cast<void*>(inputs_dev[k]);
  }
  for (size_t k = 0; k < sec.outputs.size(); ++k) {
    if (!outputs_dev[k]) return Fail(LCE_HIP_ERR_INVALID, "lce_tflite_model_run_section: null output pointer");
    ptr[sec.outputs[k]] = outputs_dev[k];
  }
  // every walk starts from the caller's pointers alone (a walk adds the scratch buffers it uses to its own copy)
  auto walk = [&](bool capturing) { return Walk{model, sec, batch, semantics, /*run=*/true, stream, capturing, ptr, {}, {}}.Section(); };
  model->last = lce_tflite_model::RunStats();
  if (!model->use_graphs || !stream) return walk(false);

  lce_tflite_model::GraphKey key{section, batch, semantics, stream, {}};
  for (size_t k = 0; k < sec.inputs.size(); ++k) key.ptrs.push_back(inputs_dev[k]);
  for (size_t k = 0; k < sec.outputs.size(); ++k) key.ptrs.push_back(outputs_dev[k]);
  {
    lce_tflite_model::GraphEntry& e = model->graphs[key];
    if (e.graph) {
      model->last = e.stats;
      ++model->graph_replays;
      return lce_hip_graph_launch(e.graph, stream);
    }
    if (e.eager_runs >= 1 && !e.unrecordable) {
      // record: the same walk, on a capturing stream (nothing executes); whatever goes wrong, the section then runs eagerly
      bool recorded = false;
      void* g = nullptr;
      if (lce_hip_graph_begin_capture(stream) == LCE_HIP_OK) {
        const lce_hip_status walked = walk(true);
        const lce_hip_status ended = lce_hip_graph_end_capture(stream, &g);
        recorded = walked == LCE_HIP_OK && ended == LCE_HIP_OK && g != nullptr;
        if (!recorded && g) { lce_hip_graph_destroy(g); g = nullptr; }
      }
      g_model_error.clear();
      lce_tflite_model::GraphEntry& e2 = model->graphs[key];     // (the walk may have dropped the table)
      if (recorded) {
        e2.graph = g;
        e2.stats = model->last;
        e2.eager_runs = 1;
        ++model->graph_captures;
        ++model->graph_replays;
        return lce_hip_graph_launch(g, stream);
      }
      e2.unrecordable = true;
      model->last = lce_tflite_model::RunStats();
    }
  }
  const lce_hip_status s = walk(false);
  if (s == LCE_HIP_OK) ++model->graphs[key].eager_runs;
  return s;
}

void lce_tflite_model_use_hip_graphs(lce_tflite_model* model, int32_t on) {
  if (!model) return;
  std::lock_guard<std::mutex> lock(model->run_mu);
  model->use_graphs = on != 0;
  if (!on) model->DropGraphs();
}

void lce_tflite_model_graph_stats(lce_tflite_model* model, int32_t* recorded, int32_t* replays) {
  if (!model) return;
  std::lock_guard<std::mutex> lock(model->run_mu);
  if (recorded) *recorded = model->graph_captures;
  if (replays) *replays = model->graph_replays;
}

void lce_tflite_model_elementwise_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded) {
  Stats(model, [&](const RunStats& r) {
    Put(launches, r.pass[kAbsorbedElementwise].launches); Put(ops_folded, r.ew_ops); Put(quantize_folded, r.pass[kAbsorbedElementwise].quantize);
  });
}
void lce_tflite_model_int8_add_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedInt8Add, launches, quantize_folded);
}
void lce_tflite_model_concat_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedConcat, launches, quantize_folded);
}
void lce_tflite_model_pool_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedPool, launches, quantize_folded);
}
void lce_tflite_model_conv1x1_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedConv1x1, launches, quantize_folded);
}
void lce_tflite_model_depthwise_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedDepthwise, launches, quantize_folded);
}
void lce_tflite_model_conv2d_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedConv2d, launches, quantize_folded);
}
void lce_tflite_model_conv_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedConvI8, launches, quantize_folded);
}
void lce_tflite_model_depthwise_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedDepthwiseI8, launches, quantize_folded);
}
void lce_tflite_model_gate_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded) {
  LaunchStats(model, kAbsorbedGate, launches, quantize_folded);
}
void lce_tflite_model_head_stats(lce_tflite_model* model, int32_t* mean, int32_t* fully_connected, int32_t* softmax) {
  Stats(model, [&](const RunStats& r) {
    Put(mean, r.pass[kAbsorbedMean].launches); Put(fully_connected, r.pass[kAbsorbedFullyConnected].launches); Put(softmax, r.pass[kAbsorbedSoftmax].launches);
  });
}
void lce_tflite_model_head_i8_stats(lce_tflite_model* model, int32_t* mean, int32_t* fully_connected, int32_t* softmax) {
  Stats(model, [&](const RunStats& r) {
    Put(mean, r.pass[kAbsorbedMeanI8].launches); Put(fully_connected, r.pass[kAbsorbedFullyConnectedI8].launches); Put(softmax, r.pass[kAbsorbedSoftmaxI8].launches);
  });
}
void lce_tflite_model_binary_dense_stats(lce_tflite_model* model, int32_t* launches, int32_t* dequantize_skipped, int32_t* quantize_absorbed) {
  Stats(model, [&](const RunStats& r) {
    Put(launches, r.pass[kAbsorbedBinaryDense].launches); Put(dequantize_skipped, r.dequantize_skipped); Put(quantize_absorbed, r.pass[kAbsorbedBinaryDense].quantize);
  });
}
void lce_tflite_model_quantize_stats(lce_tflite_model* model, int32_t* quantize, int32_t* dequantize) {
  Stats(model, [&](const RunStats& r) { Put(quantize, r.pass[kAbsorbedQuantize].launches); Put(dequantize, r.pass[kAbsorbedDequantize].launches); });
}
void lce_tflite_model_activation_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded) {
  Stats(model, [&](const RunStats& r) {
    Put(launches, r.pass[kAbsorbedActivation].launches); Put(ops_folded, r.ex_ops); Put(quantize_folded, r.pass[kAbsorbedActivation].quantize);
  });
}
void lce_tflite_model_slice_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded, int32_t* joins) {
  Stats(model, [&](const RunStats& r) {
    Put(launches, r.pass[kAbsorbedSlice].launches); Put(quantize_folded, r.pass[kAbsorbedSlice].quantize); Put(joins, r.slice_joins);
  });
}
void lce_tflite_model_elementwise_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded) {
  Stats(model, [&](const RunStats& r) {
    Put(launches, r.pass[kAbsorbedElementwiseI8].launches); Put(ops_folded, r.ew_i8_ops); Put(quantize_folded, r.pass[kAbsorbedElementwiseI8].quantize);
  });
}
void lce_tflite_model_gate_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded) {
  Stats(model, [&](const RunStats& r) {
    Put(launches, r.pass[kAbsorbedMulI8].launches); Put(ops_folded, r.gate_i8_ops); Put(quantize_folded, r.pass[kAbsorbedMulI8].quantize);
  });
}
void lce_tflite_model_transition_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded) {
  Stats(model, [&](const RunStats& r) { Put(launches, r.transition_launches); Put(ops_folded, r.transition_ops); Put(quantize_folded, r.transition_quantize); });
}
void lce_tflite_model_reshape_stats(lce_tflite_model* model, int32_t* views, int32_t* copies) {
  Stats(model, [&](const RunStats& r) { Put(views, r.reshape_views); Put(copies, r.reshape_copies); });
}

void lce_tflite_model_run_stats(lce_tflite_model* model, int32_t* cached_plans, int32_t* fused_quantize_ops, size_t* scratch_bytes) {
  if (!model) return;
  std::lock_guard<std::mutex> lock(model->run_mu);
  if (cached_plans) *cached_plans = (int32_t)model->plans.size();
  if (fused_quantize_ops) *fused_quantize_ops = model->last.conv_quantize;
  size_t b = 0;
  for (auto& kv : model->scratch) b += kv.second.bytes;
  if (scratch_bytes) *scratch_bytes = b;
}

}  // extern "C"
