// Bounds-checked reader for the subset of the TFLite flatbuffer (.tflite) that a converted
// Larq model needs to hand its LCE custom ops to this library: operator codes, the first
// subgraph's tensors / operators / inputs / outputs, quantization scale + zero point, and
// constant buffers.  SURVEY.md section 8(f) row n3.
//
// The reference reads models through TensorFlow Lite itself (tflite::FlatBufferModel +
// InterpreterBuilder, examples/lce_minimal.cc:28-40; tflite/python/interpreter_wrapper_lite.cc:
// 40-58) -- an un-vendored third-party dependency (tensorflow v2.16.1, WORKSPACE:12-24), as is
// the flatbuffers library.  This file restates the published FlatBuffers wire format and the
// field numbering of tensorflow/lite/schema/schema.fbs (file identifier "TFL3"):
//   Model            0 version  1 operator_codes  2 subgraphs  3 description  4 buffers
//   OperatorCode     0 deprecated_builtin_code(int8)  1 custom_code  2 version  3 builtin_code(int32)
//   SubGraph         0 tensors  1 inputs  2 outputs  3 operators  4 name
//   Tensor           0 shape  1 type(int8)  2 buffer(uint32)  3 name  4 quantization
//   QuantizationParameters  0 min  1 max  2 scale[float]  3 zero_point[int64]  4/5 details (union)  6 quantized_dimension(int32)
//   Operator         0 opcode_index  1 inputs  2 outputs  3/4 builtin_options (union)
//                    5 custom_options[ubyte]  6 custom_options_format
//   Buffer           0 data[ubyte]
//   BuiltinOptions union types: 11 AddOptions, 21 MulOptions; both tables: 0 fused_activation_function(int8,
//   ActivationFunctionType: 0 NONE, 1 RELU, 2 RELU_N1_TO_1, 3 RELU6, 4 TANH, 5 SIGN_BIT); BuiltinOperator 0 ADD, 18 MUL.
//   BuiltinOptions union type 10 ConcatenationOptions: 0 axis(int32, default 0), 1 fused_activation_function(int8);
//   BuiltinOperator 2 CONCATENATION.
//   BuiltinOptions union type 5 Pool2DOptions: 0 padding(int8, Padding: 0 SAME, 1 VALID)  1 stride_w(int32)  2 stride_h(int32)
//   3 filter_width(int32)  4 filter_height(int32)  5 fused_activation_function(int8); BuiltinOperator 1 AVERAGE_POOL_2D,
//   17 MAX_POOL_2D.
//   BuiltinOptions union type 1 Conv2DOptions: 0 padding(int8)  1 stride_w(int32)  2 stride_h(int32)
//   3 fused_activation_function(int8)  4 dilation_w_factor(int32, default 1)  5 dilation_h_factor(int32, default 1);
//   BuiltinOperator 3 CONV_2D.
//   BuiltinOptions union type 2 DepthwiseConv2DOptions: 0 padding(int8)  1 stride_w(int32)  2 stride_h(int32)
//   3 depth_multiplier(int32)  4 fused_activation_function(int8)  5 dilation_w_factor(int32, default 1)
//   6 dilation_h_factor(int32, default 1); BuiltinOperator 4 DEPTHWISE_CONV_2D.
//   BuiltinOptions union type 27 ReducerOptions: 0 keep_dims(bool); BuiltinOperator 40 MEAN.
//   BuiltinOptions union type 8 FullyConnectedOptions: 0 fused_activation_function(int8)  1 weights_format(int8, 0 DEFAULT)
//   2 keep_num_dims(bool)  3 asymmetric_quantize_inputs(bool); BuiltinOperator 9 FULLY_CONNECTED.
//   BuiltinOptions union type 9 SoftmaxOptions: 0 beta(float); BuiltinOperator 25 SOFTMAX.
//   BuiltinOperator 6 DEQUANTIZE, 114 QUANTIZE: no option this reader needs.
//   BuiltinOperator 14 LOGISTIC, 19 RELU, 20 RELU_N1_TO_1, 21 RELU6, 54 PRELU (inputs: data, alpha): no options table.
//   BuiltinOperator 22 RESHAPE (inputs: data and, optionally, the new shape as an int32 tensor): its ReshapeOptions.new_shape
//   repeats the declared shape of the output tensor, which is what this library goes by; the table is not read.
//   BuiltinOptions union type 32 StridedSliceOptions: 0 begin_mask  1 end_mask  2 ellipsis_mask  3 new_axis_mask
//   4 shrink_axis_mask (all int32, default 0)  5 offset(bool, default false); BuiltinOperator 45 STRIDED_SLICE (inputs: data,
//   begin, end, strides), 65 SLICE (inputs: data, begin, size; no option this reader needs).
//   (Restated from the published schema.fbs: no schema file exists in the build image either.)
// No .tflite file and no flatbuffers library exist in the build image: the only byte-level
// known answers are the reference's flexbuffer option blobs (mlir/tests/legalize-lce.mlir:9,21),
// which custom_options carry unchanged.  Everything else is tested against a writer that
// follows the same specification (tests/tflite_writer.py) -- parity with real converter output
// is UNPINNED until a real model file is available.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace lce_tfl {

constexpr int32_t kBuiltinCustom = 32;   // BuiltinOperator_CUSTOM
constexpr int32_t kBuiltinAdd = 0, kBuiltinAveragePool2d = 1, kBuiltinConcatenation = 2, kBuiltinConv2d = 3, kBuiltinDepthwiseConv2d = 4, kBuiltinMaxPool2d = 17, kBuiltinMul = 18;
constexpr int32_t kBuiltinFullyConnected = 9, kBuiltinSoftmax = 25, kBuiltinMean = 40;
constexpr int32_t kBuiltinDequantize = 6, kBuiltinQuantize = 114;   // (their options tables, QuantizeOptions and DequantizeOptions, are empty)
constexpr int32_t kBuiltinLogistic = 14, kBuiltinRelu = 19, kBuiltinReluN1To1 = 20, kBuiltinRelu6 = 21, kBuiltinReshape = 22, kBuiltinPrelu = 54;
constexpr int kOptionsConv2d = 1, kOptionsDepthwiseConv2d = 2, kOptionsPool2d = 5, kOptionsConcatenation = 10, kOptionsAdd = 11, kOptionsMul = 21;   // BuiltinOptions union types
constexpr int kOptionsFullyConnected = 8, kOptionsSoftmax = 9, kOptionsReducer = 27;
constexpr int32_t kBuiltinStridedSlice = 45, kBuiltinSlice = 65;
constexpr int kOptionsStridedSlice = 32;
// TensorType values used by LCE graphs
constexpr int kTensorFloat32 = 0, kTensorInt32 = 2, kTensorBool = 6, kTensorInt8 = 9;

struct Tensor {
  std::vector<int32_t> shape;
  int type = 0;
  uint32_t buffer = 0;
  std::string name;
  bool quantized = false;
  float scale = 0.0f;                // the first element of `scales`
  int64_t zero_point = 0;            // the first element of `zero_points`
  std::vector<float> scales;         // the whole scale vector: one element per tensor, or one per slice of quantized_dimension
  std::vector<int64_t> zero_points;
  int32_t quantized_dimension = 0;
  const uint8_t* data = nullptr;   // constant data (inside the model buffer), or null
  size_t bytes = 0;
};

struct Operator {
  int32_t builtin_code = 0;
  std::string custom_code;         // "LceBconv2d", ... when builtin_code == kBuiltinCustom
  std::vector<int32_t> inputs, outputs;   // tensor indices, -1 = optional input not present
  const uint8_t* custom_options = nullptr;
  size_t custom_options_size = 0;
  int32_t activation = 0;          // fused_activation_function of AddOptions / MulOptions / ConcatenationOptions / Pool2DOptions; 0 (NONE) when absent
  int32_t axis = 0;                // ConcatenationOptions.axis; 0 when absent
  // Pool2DOptions; all 0 when absent (schema defaults: padding SAME, the strides and the filter 0)
  int32_t pool_padding = 0, pool_stride_w = 0, pool_stride_h = 0, pool_filter_w = 0, pool_filter_h = 0;
  // Conv2DOptions: padding and strides in the pool fields above (filter 0); the dilations (schema default 1; 1 when absent)
  int32_t dilation_w = 1, dilation_h = 1;
  bool has_conv_options = false;   // a Conv2DOptions table is present
  // DepthwiseConv2DOptions: padding, strides and dilations in the fields above; the multiplier (0 when absent)
  int32_t depth_multiplier = 0;
  bool has_depthwise_options = false;   // a DepthwiseConv2DOptions table is present
  // ReducerOptions (false when absent); FullyConnectedOptions (its activation in `activation`); SoftmaxOptions
  bool keep_dims = false;
  bool has_fc_options = false, fc_keep_num_dims = false;
  int32_t fc_weights_format = 0;
  bool has_softmax_options = false;
  float softmax_beta = 0.0f;
  // StridedSliceOptions (all 0 / false when absent)
  bool has_slice_options = false, slice_offset = false;
  int32_t begin_mask = 0, end_mask = 0, ellipsis_mask = 0, new_axis_mask = 0, shrink_axis_mask = 0;
};

class Model {
 public:
  std::vector<Tensor> tensors;
  std::vector<Operator> operators;
  std::vector<int32_t> inputs, outputs;
  uint32_t version = 0;
  std::string description;

  // `data` must stay alive while the Model is used (constant tensors point into it).
  bool Parse(const void* data, size_t size, std::string* err) {
    b_ = (const uint8_t*)data;
    n_ = size;
    err_.clear();
    tensors.clear(); operators.clear(); inputs.clear(); outputs.clear();
    const bool ok = ParseImpl();
    if (!ok && err) *err = err_.empty() ? "malformed flatbuffer" : err_;
    return ok;
  }

 private:
  const uint8_t* b_ = nullptr;
  size_t n_ = 0;
  std::string err_;

  bool Fail(const char* what) { if (err_.empty()) err_ = what; return false; }
  bool In(size_t pos, size_t len) const { return pos <= n_ && len <= n_ - pos; }
  template <typename T> bool Rd(size_t pos, T* out) const {
    if (!In(pos, sizeof(T))) return false;
    memcpy(out, b_ + pos, sizeof(T));   // little-endian hosts only, like the reference
    return true;
  }
  // Position of field `id` inside table `t`, 0 when absent; false on a malformed table.
  bool Field(size_t t, int id, size_t* pos) const {
    *pos = 0;
    int32_t so;
    if (!Rd(t, &so)) return false;
    const int64_t vt = (int64_t)t - so;
    if (vt < 0 || !In((size_t)vt, 4)) return false;
    uint16_t vsize, fo;
    if (!Rd((size_t)vt, &vsize) || vsize < 4 || !In((size_t)vt, vsize)) return false;
    const size_t slot = 4 + 2 * (size_t)id;
    if (slot + 2 > vsize) return true;               // field not in this (older) vtable
    if (!Rd((size_t)vt + slot, &fo)) return false;
    if (fo == 0) return true;
    if (!In(t + fo, 1)) return false;
    *pos = t + fo;
    return true;
  }
  // Follows the uoffset stored at `pos`.
  bool Indirect(size_t pos, size_t* target) const {
    uint32_t off;
    if (!Rd(pos, &off)) return false;
    *target = pos + off;
    return In(*target, 4);
  }
  // Vector header at `v`: element count and position of element 0.
  bool Vec(size_t v, size_t elem, uint32_t* count, size_t* first) const {
    if (!Rd(v, count)) return false;
    *first = v + 4;
    return In(*first, (size_t)*count * elem);
  }
  template <typename T> bool Scalar(size_t t, int id, T dflt, T* out) const {
    size_t p;
    if (!Field(t, id, &p)) return false;
    *out = dflt;
    return p == 0 || Rd(p, out);
  }
  bool String(size_t t, int id, std::string* out) const {
    size_t p, s, first;
    uint32_t len;
    out->clear();
    if (!Field(t, id, &p)) return false;
    if (p == 0) return true;
    if (!Indirect(p, &s) || !Vec(s, 1, &len, &first)) return false;
    out->assign((const char*)b_ + first, len);
    return true;
  }
  // Vector field of scalars -> (count, first); count 0 when absent.
  bool VecField(size_t t, int id, size_t elem, uint32_t* count, size_t* first) const {
    size_t p, v;
    *count = 0; *first = 0;
    if (!Field(t, id, &p)) return false;
    if (p == 0) return true;
    return Indirect(p, &v) && Vec(v, elem, count, first);
  }
  bool IntVec(size_t t, int id, std::vector<int32_t>* out) const {
    uint32_t c; size_t f;
    if (!VecField(t, id, 4, &c, &f)) return false;
    out->resize(c);
    if (c) memcpy(out->data(), b_ + f, (size_t)c * 4);
    return true;
  }
  // Element i of a vector of tables.
  bool TableAt(size_t first, uint32_t i, size_t* t) const { return Indirect(first + 4 * (size_t)i, t); }

  bool ParseImpl() {
    if (n_ < 8) return Fail("buffer too small for a flatbuffer");
    if (memcmp(b_ + 4, "TFL3", 4) != 0) return Fail("file identifier is not TFL3");
    size_t root;
    if (!Indirect(0, &root)) return Fail("bad root offset");
    if (!Scalar<uint32_t>(root, 0, 0u, &version)) return Fail("bad Model table");
    if (!String(root, 3, &description)) return Fail("bad Model.description");

    // buffers
    uint32_t nbuf; size_t bfirst;
    if (!VecField(root, 4, 4, &nbuf, &bfirst)) return Fail("bad Model.buffers");
    std::vector<std::pair<const uint8_t*, size_t>> buffers(nbuf);
    for (uint32_t i = 0; i < nbuf; ++i) {
      size_t t; uint32_t c; size_t f;
      if (!TableAt(bfirst, i, &t) || !VecField(t, 0, 1, &c, &f)) return Fail("bad Buffer");
      buffers[i] = {c ? b_ + f : nullptr, c};
    }
    // operator codes
    uint32_t ncode; size_t cfirst;
    if (!VecField(root, 1, 4, &ncode, &cfirst)) return Fail("bad Model.operator_codes");
    struct Code { int32_t builtin; std::string custom; };
    std::vector<Code> codes(ncode);
    for (uint32_t i = 0; i < ncode; ++i) {
      size_t t; int8_t dep; int32_t bc;
      if (!TableAt(cfirst, i, &t) || !Scalar<int8_t>(t, 0, 0, &dep) || !Scalar<int32_t>(t, 3, 0, &bc) ||
          !String(t, 1, &codes[i].custom))
        return Fail("bad OperatorCode");
      // schema.fbs: builtin_code supersedes deprecated_builtin_code once it exceeds 127
      codes[i].builtin = bc != 0 ? bc : (int32_t)dep;
    }
    // first subgraph
    uint32_t nsub; size_t sfirst, sg;
    if (!VecField(root, 2, 4, &nsub, &sfirst) || nsub == 0) return Fail("model has no subgraph");
    if (!TableAt(sfirst, 0, &sg)) return Fail("bad SubGraph");
    if (!IntVec(sg, 1, &inputs) || !IntVec(sg, 2, &outputs)) return Fail("bad SubGraph.inputs/outputs");
    uint32_t nt; size_t tfirst;
    if (!VecField(sg, 0, 4, &nt, &tfirst)) return Fail("bad SubGraph.tensors");
    tensors.resize(nt);
    for (uint32_t i = 0; i < nt; ++i) {
      size_t t, qp, q;
      Tensor& T = tensors[i];
      int8_t ty;
      if (!TableAt(tfirst, i, &t) || !IntVec(t, 0, &T.shape) || !Scalar<int8_t>(t, 1, 0, &ty) ||
          !Scalar<uint32_t>(t, 2, 0u, &T.buffer) || !String(t, 3, &T.name) || !Field(t, 4, &qp))
        return Fail("bad Tensor");
      T.type = ty;
      if (T.buffer >= nbuf && nbuf != 0) return Fail("Tensor.buffer out of range");
      if (T.buffer != 0 && T.buffer < nbuf) { T.data = buffers[T.buffer].first; T.bytes = buffers[T.buffer].second; }
      if (qp != 0) {
        uint32_t c; size_t f;
        if (!Indirect(qp, &q)) return Fail("bad Tensor.quantization");
        if (!VecField(q, 2, 4, &c, &f)) return Fail("bad QuantizationParameters.scale");
        if (c >= 1) { memcpy(&T.scale, b_ + f, 4); T.quantized = true; }
        T.scales.resize(c);                                        // (VecField has checked that c elements lie in the buffer)
        if (c) memcpy(T.scales.data(), b_ + f, (size_t)c * 4);
        if (!VecField(q, 3, 8, &c, &f)) return Fail("bad QuantizationParameters.zero_point");
        if (c >= 1) memcpy(&T.zero_point, b_ + f, 8);
        T.zero_points.resize(c);
        if (c) memcpy(T.zero_points.data(), b_ + f, (size_t)c * 8);
        if (!Scalar<int32_t>(q, 6, 0, &T.quantized_dimension)) return Fail("bad QuantizationParameters.quantized_dimension");
      }
    }
    uint32_t no; size_t ofirst;
    if (!VecField(sg, 3, 4, &no, &ofirst)) return Fail("bad SubGraph.operators");
    operators.resize(no);
    for (uint32_t i = 0; i < no; ++i) {
      size_t t; uint32_t idx, c; size_t f;
      Operator& O = operators[i];
      if (!TableAt(ofirst, i, &t) || !Scalar<uint32_t>(t, 0, 0u, &idx) || !IntVec(t, 1, &O.inputs) ||
          !IntVec(t, 2, &O.outputs) || !VecField(t, 5, 1, &c, &f))
        return Fail("bad Operator");
      if (idx >= ncode) return Fail("Operator.opcode_index out of range");
      O.builtin_code = codes[idx].builtin;
      O.custom_code = codes[idx].custom;
      O.custom_options = c ? b_ + f : nullptr;
      O.custom_options_size = c;
      uint8_t opt_type;
      size_t opt_pos, opt;
      if (!Scalar<uint8_t>(t, 3, 0, &opt_type) || !Field(t, 4, &opt_pos)) return Fail("bad Operator.builtin_options");
      if ((opt_type == kOptionsAdd || opt_type == kOptionsMul) && opt_pos != 0) {
        int8_t act;
        if (!Indirect(opt_pos, &opt) || !Scalar<int8_t>(opt, 0, 0, &act)) return Fail("bad AddOptions / MulOptions");
        O.activation = act;
      }
      if (opt_type == kOptionsConcatenation && opt_pos != 0) {
        int32_t axis;
        int8_t act;
        if (!Indirect(opt_pos, &opt) || !Scalar<int32_t>(opt, 0, 0, &axis) || !Scalar<int8_t>(opt, 1, 0, &act))
          return Fail("bad ConcatenationOptions");
        O.axis = axis;
        O.activation = act;
      }
      if (opt_type == kOptionsPool2d && opt_pos != 0) {
        int8_t pad, act;
        if (!Indirect(opt_pos, &opt) || !Scalar<int8_t>(opt, 0, 0, &pad) || !Scalar<int32_t>(opt, 1, 0, &O.pool_stride_w) ||
            !Scalar<int32_t>(opt, 2, 0, &O.pool_stride_h) || !Scalar<int32_t>(opt, 3, 0, &O.pool_filter_w) ||
            !Scalar<int32_t>(opt, 4, 0, &O.pool_filter_h) || !Scalar<int8_t>(opt, 5, 0, &act))
          return Fail("bad Pool2DOptions");
        O.pool_padding = pad;
        O.activation = act;
      }
      if (opt_type == kOptionsConv2d && opt_pos != 0) {
        int8_t pad, act;
        if (!Indirect(opt_pos, &opt) || !Scalar<int8_t>(opt, 0, 0, &pad) || !Scalar<int32_t>(opt, 1, 0, &O.pool_stride_w) ||
            !Scalar<int32_t>(opt, 2, 0, &O.pool_stride_h) || !Scalar<int8_t>(opt, 3, 0, &act) ||
            !Scalar<int32_t>(opt, 4, 1, &O.dilation_w) || !Scalar<int32_t>(opt, 5, 1, &O.dilation_h))
          return Fail("bad Conv2DOptions");
        O.pool_padding = pad;
        O.activation = act;
        O.has_conv_options = true;
      }
      if (opt_type == kOptionsDepthwiseConv2d && opt_pos != 0) {
        int8_t pad, act;
        if (!Indirect(opt_pos, &opt) || !Scalar<int8_t>(opt, 0, 0, &pad) || !Scalar<int32_t>(opt, 1, 0, &O.pool_stride_w) ||
            !Scalar<int32_t>(opt, 2, 0, &O.pool_stride_h) || !Scalar<int32_t>(opt, 3, 0, &O.depth_multiplier) ||
            !Scalar<int8_t>(opt, 4, 0, &act) || !Scalar<int32_t>(opt, 5, 1, &O.dilation_w) ||
            !Scalar<int32_t>(opt, 6, 1, &O.dilation_h))
          return Fail("bad DepthwiseConv2DOptions");
        O.pool_padding = pad;
        O.activation = act;
        O.has_depthwise_options = true;
      }
      if (opt_type == kOptionsReducer && opt_pos != 0) {
        uint8_t keep;
        if (!Indirect(opt_pos, &opt) || !Scalar<uint8_t>(opt, 0, 0, &keep)) return Fail("bad ReducerOptions");
        O.keep_dims = keep != 0;
      }
      if (opt_type == kOptionsFullyConnected && opt_pos != 0) {
        int8_t act, format;
        uint8_t keep;
        if (!Indirect(opt_pos, &opt) || !Scalar<int8_t>(opt, 0, 0, &act) || !Scalar<int8_t>(opt, 1, 0, &format) ||
            !Scalar<uint8_t>(opt, 2, 0, &keep))
          return Fail("bad FullyConnectedOptions");
        O.activation = act;
        O.fc_weights_format = format;
        O.fc_keep_num_dims = keep != 0;
        O.has_fc_options = true;
      }
      if (opt_type == kOptionsSoftmax && opt_pos != 0) {
        if (!Indirect(opt_pos, &opt) || !Scalar<float>(opt, 0, 0.0f, &O.softmax_beta)) return Fail("bad SoftmaxOptions");
        O.has_softmax_options = true;
      }
      if (opt_type == kOptionsStridedSlice && opt_pos != 0) {
        uint8_t offset;
        if (!Indirect(opt_pos, &opt) || !Scalar<int32_t>(opt, 0, 0, &O.begin_mask) || !Scalar<int32_t>(opt, 1, 0, &O.end_mask) ||
            !Scalar<int32_t>(opt, 2, 0, &O.ellipsis_mask) || !Scalar<int32_t>(opt, 3, 0, &O.new_axis_mask) ||
            !Scalar<int32_t>(opt, 4, 0, &O.shrink_axis_mask) || !Scalar<uint8_t>(opt, 5, 0, &offset))
          return Fail("bad StridedSliceOptions");
        O.slice_offset = offset != 0;
        O.has_slice_options = true;
      }
      for (int32_t x : O.inputs) if (x < -1 || x >= (int32_t)nt) return Fail("Operator input index out of range");
      for (int32_t x : O.outputs) if (x < 0 || x >= (int32_t)nt) return Fail("Operator output index out of range");
    }
    for (int32_t x : inputs) if (x < 0 || x >= (int32_t)nt) return Fail("SubGraph input index out of range");
    for (int32_t x : outputs) if (x < 0 || x >= (int32_t)nt) return Fail("SubGraph output index out of range");
    return true;
  }
};

}  // namespace lce_tfl
