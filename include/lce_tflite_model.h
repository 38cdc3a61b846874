/* lce_tflite_model.h -- read a converted Larq model (.tflite) and hand its LCE custom ops to
 * the GPU library.  C ABI of liblce_tflite_ops.so.
 *
 * Replaces, for the LCE part of a graph, what the reference's callers obtain from TensorFlow
 * Lite: tflite::FlatBufferModel::BuildFromBuffer + InterpreterBuilder + the interpreter's
 * tensor table (examples/lce_minimal.cc:28-40; tflite/python/interpreter_wrapper_lite.cc:40-58;
 * tflite/python/interpreter_wrapper_utils.h).  Host-only except where a plan is created.
 * The flatbuffer reader restates the published format (see
 * compute-engine_amd/csrc/tflite/tflite_flatbuffer_reader.h); no real converter output exists
 * in the build image, so parity with real files is unpinned.
 */
#ifndef LCE_TFLITE_MODEL_H_
#define LCE_TFLITE_MODEL_H_
#include <stddef.h>
#include <stdint.h>

#include "lce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lce_tflite_model lce_tflite_model;

/* TensorType values of schema.fbs that LCE graphs use */
enum { LCE_TFLITE_FLOAT32 = 0, LCE_TFLITE_INT32 = 2, LCE_TFLITE_BOOL = 6, LCE_TFLITE_INT8 = 9 };

/* Parses `data` (kept by reference: it must outlive the model).  Returns NULL and writes a
 * message into err (if given) when the buffer is not a well-formed TFL3 flatbuffer. */
lce_tflite_model* lce_tflite_model_open(const void* data, size_t size, char* err, size_t err_len);

/* lce_tflite_model_open with flags (0: exactly lce_tflite_model_open).
 *   LCE_TFLITE_SECTIONS_ELEMENTWISE: the host hands the float ADD / MUL BETWEEN binary layers (batch norm constants,
 *   residual shortcuts) to this library, so they join the binary sections.  A builtin operator joins an LCE epoch of the
 *   partition below when it is ADD (0) or MUL (18) on float32 tensors with a 4-D output, each input either a tensor of
 *   the output's shape (batch ignored) or a constant of shape [C], [1,1,1,C], [1] or [], its fused activation is NONE /
 *   RELU / RELU_N1_TO_1 / RELU6, and one of its non-constant inputs is produced by an operator of the same epoch (so stem
 *   and head ops, and ops on unrelated branches, stay with the host).  lce_tflite_model_run_section then runs each chain
 *   of such operators as one lce_hip_elementwise launch, with the LceQuantize that reads its result as the launch's bit
 *   output.  Every other builtin operator still cuts a section.  The flag changes the partition -- the host's contract --
 *   and is therefore opt-in.
 *   LCE_TFLITE_SECTIONS_INT8_ADD: the same for the int8 residual ADD of an int8-converted network (batch norm folded into
 *   LceBconv2d, the shortcut added by the builtin int8 ADD).  A builtin ADD (0) joins the LCE epoch in which it becomes ready
 *   when it has two inputs and one output, all three int8 WITH quantization parameters, the output is 4-D, both inputs are
 *   non-constant tensors of the output's shape (batch ignored), its fused activation is NONE / RELU / RELU_N1_TO_1 / RELU6,
 *   lce_hip_add_int8_prepare accepts its parameters, and one input is produced by an operator of the same epoch.  A constant
 *   or broadcast int8 operand, int8 MUL or SUB, and uint8 / int16 tensors do not join.  lce_tflite_model_run_section runs
 *   such an ADD as one lce_hip_add_int8 launch (TFLite's arithmetic byte for byte), with the first LceQuantize of the section
 *   that reads the sum as the launch's bit output; the int8 sum is written only when something else reads it.
 *   The flags combine; every other bit is refused. */
enum { LCE_TFLITE_SECTIONS_ELEMENTWISE = 1u, LCE_TFLITE_SECTIONS_INT8_ADD = 2u };
lce_tflite_model* lce_tflite_model_open_ex(const void* data, size_t size, uint32_t flags, char* err, size_t err_len);

/* lce_tflite_model_open with an options struct: the entry that new opt-ins extend (lce_tflite_model_open_ex keeps its two
 * flags and refuses every other bit).  `struct_size` must be sizeof(lce_tflite_open_options); `sections` takes the two
 * flags above with the meaning given there, and
 *   LCE_TFLITE_SECTIONS_CONCAT: the same for the channel join of a DENSE network (BinaryDenseNet, MeliusNet: each binary
 *   layer's output is joined to its input by the builtin CONCATENATION).  A CONCATENATION (2) joins the LCE epoch in which
 *   it becomes ready when it has 2..8 inputs and one output, all tensors of one type among float32, int8 and int32, the
 *   output is 4-D and the axis is 3 or -1, its fused activation is NONE, every input is a non-constant 4-D tensor of the
 *   output's height and width, the inputs' channels add up to the output's, and -- for int8 -- all inputs and the output
 *   carry quantization parameters with the SAME scale and zero point (a requantizing join stays with the host).  A join
 *   that is ready from the start is the host's (without LCE_TFLITE_SECTIONS_EXT_STEM).  lce_tflite_model_run_section runs such a join as one lce_hip_concat
 *   launch, with the first LceQuantize of the section that reads the joined tensor as the launch's bit output; the joined
 *   tensor itself is written only when something else reads it or the section delivers it.  Together with
 *   LCE_TFLITE_SECTIONS_ELEMENTWISE a float dense block is one section; the float MAX_POOL_2D / CONV_2D of a transition
 *   block still cut (the pool joins with LCE_TFLITE_SECTIONS_EXT_POOL, below).
 * sections == 0..3 gives exactly lce_tflite_model_open_ex with that value; every other bit is refused.
 *
 * The struct is versioned by its size.  struct_size == 8 is the first form (struct_size and sections alone): it behaves
 * exactly as it always did and nothing beyond its 8 bytes is read.  struct_size == sizeof(lce_tflite_open_options) == 24
 * also reads `sections_ext`, the opt-ins that do not fit the refusals the first form promises (a host may rely on
 * sections == 8 being refused), and `reserved`, which must be zero.  Every other size is refused.
 *   LCE_TFLITE_SECTIONS_EXT_POOL: the same for the builtin 2-D pooling between binary layers (BinaryAlexNet, XNOR-Net and
 *   DoReFa-Net pool 3x3 / 2 behind a float LceBconv2d; a dense network's transition block and the downsampling shortcuts
 *   of Bi-RealNet / BinaryResNetE pool 2x2 / 2).  An AVERAGE_POOL_2D (1) or MAX_POOL_2D (17) joins the LCE epoch in which it
 *   becomes ready when it has one input and one output, the output is 4-D with positive extents, the input is a
 *   non-constant 4-D tensor of the output's type and channel count, the type is float32 -- or int8 with both tensors
 *   carrying quantization parameters, zero points in [-128, 127] and the SAME scale and zero point (a requantizing pool
 *   stays with the host) --, filter and stride are positive, the padding is SAME or VALID, the fused activation is NONE /
 *   RELU / RELU_N1_TO_1 / RELU6, the file's declared output height and width are what the padding rule gives for the
 *   declared input, and lce_hip_pool2d_check accepts the descriptor.  A pool that is ready from the start (a stem pool)
 *   is the host's without LCE_TFLITE_SECTIONS_EXT_STEM.  lce_tflite_model_run_section runs such a pool as one lce_hip_pool2d launch, with the first LceQuantize
 *   of the section that reads the pooled tensor as the launch's bit output; the pooled tensor itself is written only when
 *   something else reads it or the section delivers it.  Together with LCE_TFLITE_SECTIONS_ELEMENTWISE the body of a
 *   BinaryAlexNet is one section.  L2 pooling, a CONV_2D and bitpacked pooling (LceBMaxPool2d, an LCE operator already)
 *   are not concerned (the float 1x1 CONV_2D joins with LCE_TFLITE_SECTIONS_EXT_CONV1X1, below).
 *
 * struct_size == 40 is the third form: four more words after `reserved`, which must be zero too, and one more bit in
 * `sections_ext` (the 24-byte form promises that sections_ext == 2 is refused, and still refuses it; nothing past its 24 bytes
 * is read).
 *   LCE_TFLITE_SECTIONS_EXT_CONV1X1: the same for the float 1x1 CONV_2D behind the pool of a downsampling shortcut (Bi-RealNet,
 *   BinaryResNetE) or of a transition block (BinaryDenseNet, MeliusNet).  A CONV_2D (3) joins the LCE epoch in which it
 *   becomes ready when it has 2 or 3 inputs (a third input of -1: no bias) and one output; input, filter and output are
 *   float32, and the bias when present; the output is 4-D with positive extents; the data input is a non-constant 4-D tensor;
 *   the filter is a constant [Cout, 1, 1, Cin] with data in the file and Cin the input's channels; the bias is absent or a
 *   constant [Cout]; Cout is the output's channels; the Conv2DOptions table is present, the strides are positive, the
 *   dilations 1, the padding SAME or VALID, the fused activation NONE / RELU / RELU_N1_TO_1 / RELU6; the declared output
 *   height and width are ceil(in / stride); and lce_hip_conv1x1_f32_check accepts the descriptor.  A convolution that is
 *   ready from the start (a stem) is the host's without LCE_TFLITE_SECTIONS_EXT_STEM, and so is everything else: a 3x3 filter (it
 *   joins with LCE_TFLITE_SECTIONS_EXT_CONV2D), int8 or hybrid weights, a
 *   non-constant filter, DEPTHWISE_CONV_2D, TANH / SIGN_BIT, a missing options table.  lce_tflite_model_run_section runs such
 *   a convolution as one lce_hip_conv1x1_f32 launch (its arithmetic: include/lce_hip.h), with the first LceQuantize of the
 *   section that reads the result as the launch's bit output; the float tensor itself is written only when something else
 *   reads it or the section delivers it; filter and bias are uploaded once per model.  Together with the element-wise and
 *   pool flags the body of a Bi-RealNet-style or dense network is one section.
 *
 * struct_size == 56 is the fourth form: four more words after `reserved2`, which must be zero too, and one more bit in
 * `sections_ext` (the 40-byte form promises that sections_ext & 4 is refused, and still refuses it; nothing past its 40 bytes
 * is read).  This form ends the growth of the struct: bits of `sections_ext` that this version does not know are refused, but
 * they are NOT promised to stay refused -- a later version may assign them at this size.  Only bit 31 is reserved forever.
 *   LCE_TFLITE_SECTIONS_EXT_DEPTHWISE: the same for the float DEPTHWISE_CONV_2D of QuickNet's transition block (ReLU ->
 *   MAX_POOL_2D -> the fixed 3x3 / 2 blur -> CONV_2D 1x1).  A DEPTHWISE_CONV_2D (4) joins the LCE epoch in which it becomes
 *   ready when it has 2 or 3 inputs (a third input of -1: no bias) and one output; input, filter and output are float32, and
 *   the bias when present; the output is 4-D with positive extents; the data input is a non-constant 4-D tensor; the filter
 *   is a constant [1, fh, fw, Cout] with data in the file; the bias is absent or a constant [Cout]; the
 *   DepthwiseConv2DOptions table is present; depth_multiplier >= 1 and Cout == Cin x depth_multiplier == the output's
 *   channels; the strides are positive, the dilations 1, the padding SAME or VALID, the fused activation NONE / RELU /
 *   RELU_N1_TO_1 / RELU6; the declared output height and width are what the padding rule gives; and
 *   lce_hip_depthwise_conv2d_f32_check accepts the descriptor.  A depthwise convolution that is ready from the start
 *   (QuickNet's stem) is the host's without LCE_TFLITE_SECTIONS_EXT_STEM, and so is everything else: int8 or hybrid weights, a non-constant filter, a dilation,
 *   TANH / SIGN_BIT, a missing options table.  lce_tflite_model_run_section runs such a convolution as one
 *   lce_hip_depthwise_conv2d_f32 launch (its arithmetic: include/lce_hip.h), with the first LceQuantize of the section that
 *   reads the result as the launch's bit output; the float tensor itself is written only when something else reads it or the
 *   section delivers it; filter and bias are uploaded once per model.  Together with the element-wise, pool and 1x1 flags a
 *   QuickNet body is one section.
 * Two bits assigned later at the 56-byte size (the 24- and 40-byte forms refuse them):
 *   LCE_TFLITE_SECTIONS_EXT_CONV2D: the same for a float CONV_2D of ANY filter extent -- the first operator of every converted
 *   network (QuickNet 3x3 / 2, Bi-RealNet / BinaryResNetE / BinaryDenseNet 7x7 / 2, BinaryAlexNet 11x11 / 4).  A CONV_2D (3)
 *   joins the LCE epoch in which it becomes ready under the conditions of LCE_TFLITE_SECTIONS_EXT_CONV1X1, except that the
 *   filter is a constant [Cout, fh, fw, Cin] with fh, fw >= 1 whose byte count matches, the declared output height and width
 *   are what the padding rule gives, and lce_hip_conv2d_f32_check accepts the descriptor.  A grouped filter (shape[3] != Cin),
 *   int8 or hybrid weights, a non-constant filter or bias, a dilation, TANH / SIGN_BIT and a missing options table stay with
 *   the host.  LCE_TFLITE_SECTIONS_EXT_CONV1X1 is tried first: with both bits a 1x1 filter runs exactly as before, with this
 *   bit alone it runs on lce_hip_conv2d_f32 (the same bytes).  lce_tflite_model_run_section runs such a convolution as one
 *   lce_hip_conv2d_f32 call, folded and fed as the 1x1 convolution is.
 *   LCE_TFLITE_SECTIONS_EXT_STEM: an operator that qualifies under any ENABLED opt-in and whose inputs are all ready at the
 *   start (model inputs and constants) is queued with the LCE operators instead of the builtin ones.  Nothing else in the
 *   partition changes.  A stem of such operators therefore joins the first LCE epoch: stem and body are one section whose
 *   input is the model's input tensor, and a section need not contain an LCE operator.  A stem operator that does not qualify
 *   (QUANTIZE, PAD, a uint8 input) still opens a builtin epoch, and what it feeds joins later by the rules above.  After both
 *   bits only the classifier head (MEAN, FULLY_CONNECTED, SOFTMAX) of a converted network is the host's -- through this entry.
 *   The head joins through lce_tflite_model_open_passes (below), which names passes instead of adding a bit or a size here.
 * The flags of both words combine. */
enum { LCE_TFLITE_SECTIONS_CONCAT = 4u };
enum {
  LCE_TFLITE_SECTIONS_EXT_POOL = 1u,
  LCE_TFLITE_SECTIONS_EXT_CONV1X1 = 2u,  /* the 40- and 56-byte forms only */
  LCE_TFLITE_SECTIONS_EXT_DEPTHWISE = 4u, /* the 56-byte form only */
  LCE_TFLITE_SECTIONS_EXT_CONV2D = 8u,    /* the 56-byte form only */
  LCE_TFLITE_SECTIONS_EXT_STEM = 16u      /* the 56-byte form only */
};
typedef struct lce_tflite_open_options {
  uint32_t struct_size;    /* 8 (the first two fields only), 24 (up to `reserved`), 40 (up to `reserved2`) or
                              sizeof(lce_tflite_open_options) == 56 */
  uint32_t sections;       /* LCE_TFLITE_SECTIONS_*: 0..7, every other bit refused */
  uint32_t sections_ext;   /* LCE_TFLITE_SECTIONS_EXT_*; every other bit refused (at 56 bytes: refused by THIS version, see above) */
  uint32_t reserved[3];    /* must be zero */
  uint32_t reserved2[4];   /* the 40-byte form: must be zero */
  uint32_t reserved3[4];   /* the 56-byte form: must be zero */
} lce_tflite_open_options;
lce_tflite_model* lce_tflite_model_open_opts(const void* data, size_t size, const lce_tflite_open_options* options, char* err,
                                             size_t err_len);

/* lce_tflite_model_open with the opt-ins NAMED: `passes` is a comma-separated list (no spaces) drawn from
 *   elementwise, int8_add, concat, pool, conv1x1, depthwise, conv2d, stem, head, conv2d_i8, head_i8, quantize, depthwise_i8, activation, reshape, gate,
 *   binary_dense, slice, elementwise_i8, gate_i8
 * "" is exactly lce_tflite_model_open.  The first eight names set exactly the bits LCE_TFLITE_SECTIONS_ELEMENTWISE ..
 * LCE_TFLITE_SECTIONS_EXT_STEM set through lce_tflite_model_open_opts, so the partition is the same.  NULL, an unknown name (an
 * empty one included) and a name given twice are refused; the message names the offender.  lce_tflite_model_open_opts and
 * lce_tflite_model_open_ex are unchanged: no bit and no size of lce_tflite_open_options enables what follows.
 *   head: the float classifier head of a converted network (GlobalAveragePooling -> Dense -> softmax) joins the sections; no
 *   other entry can ask for it.  A head operator is queued with the LCE operators whatever made it ready: behind the body (with
 *   the flags that make the body one section) it joins the body's section, behind an operator of the host it opens a section
 *   of its own.  Three builtin operators qualify.
 *   MEAN (40): two inputs and one output; the data input is a non-constant float32 4-D tensor with positive extents; the axis
 *   is a constant int32 scalar or vector with data in the file whose entries (negative ones + 4) are exactly {1, 2}; the output
 *   is float32 [b, C] (ReducerOptions.keep_dims false, or no options table) or [b, 1, 1, C] (keep_dims true); and
 *   lce_hip_pool2d_check accepts the AVERAGE, VALID, stride-1 pool whose filter is the image (H x W <= LCE_HIP_POOL_MAX_TAPS).
 *   It runs as ONE lce_hip_pool2d launch, whose arithmetic (the sequential float sum in raster order, then the IEEE division
 *   by the count) is reference_ops::Mean's.
 *   FULLY_CONNECTED (9): 2 or 3 inputs (a third input of -1: no bias) and one output; input, weights and output float32, the
 *   bias when present; the input is non-constant, of rank 2 or 4, and its extents behind the batch multiply to K; the weights
 *   are a constant [N, K] with data in the file; the bias is absent or a constant [N]; the FullyConnectedOptions table is
 *   present, weights_format is 0 (DEFAULT), keep_num_dims is false or the input is rank 2, the fused activation is NONE / RELU /
 *   RELU_N1_TO_1 / RELU6; the output is [b, N]; and lce_hip_fully_connected_f32_check accepts the descriptor.  It runs as ONE
 *   lce_hip_fully_connected_f32 launch (its arithmetic: include/lce_hip.h); weights and bias are uploaded once per model.
 *   SOFTMAX (25): one float32 non-constant input [b, n] or [b, 1, 1, n] and an output of the same shape; the SoftmaxOptions
 *   table is present and beta is finite and > 0.  It runs as ONE lce_hip_softmax_f32 launch (its bytes: include/lce_hip.h).
 *   Everything else stays with the host, as before: int8 or hybrid FULLY_CONNECTED, a non-constant weight, shuffled weights, a
 *   MEAN over other axes, TANH, a missing options table.  (RESHAPE / Flatten and LOGISTIC: `reshape` and `activation`, below.)
 *   No LceQuantize folds into a head operator.  With every name a converted network is ONE section from the image to the
 *   probabilities and no builtin operator is left for the host.
 *   conv2d_i8: the quantized builtin CONV_2D (3) of an int8-converted network -- its stem, the 1x1 behind the pool of a
 *   downsampling shortcut, the 1x1 of a transition -- joins the sections; no other entry can ask for it, and no float predicate
 *   takes an int8 tensor, so it moves nothing in a float-converted file.  It qualifies when: the Conv2DOptions table is present;
 *   it has 2 or 3 inputs (a third input of -1: no bias) and one output; input and output are int8, each quantized with exactly
 *   one scale and a zero point in [-128, 127]; the output is 4-D with positive extents and the data input non-constant and 4-D;
 *   the filter is a constant int8 [Cout, fh, fw, Cin] with data in the file whose byte count matches (compared by division),
 *   Cin the input's channels, no zero point other than 0, and 1 or Cout scales (with more than one, quantized_dimension 0); the
 *   bias is absent or a constant int32 [Cout]; the dilations are 1, the strides positive, the padding SAME or VALID, the fused
 *   activation NONE / RELU / RELU_N1_TO_1 / RELU6; the declared output height and width are what the padding rule gives; and
 *   lce_hip_conv2d_i8_prepare accepts the file's constants (include/lce_hip.h: where the reference's own int32 accumulator
 *   could overflow it does not).  A grouped or dilated convolution, hybrid weights, a filter zero point, scales along another
 *   dimension and a float bias stay with the host.  It joins the epoch in which it becomes ready, and `stem` applies to it as to
 *   any enabled opt-in.  lce_tflite_model_run_section runs it as ONE lce_hip_conv2d_i8 launch -- TFLite's integer arithmetic
 *   byte for byte -- whose table is prepared and uploaded once per model beside the filter; a following LceQuantize folds into
 *   the launch's bits.  With int8_add, pool and stem an int8 Bi-RealNet-style block with its downsampling shortcut, and an int8
 *   stem with the binary layer behind it, are one section each.  Not this name's: int8 DEPTHWISE_CONV_2D (depthwise_i8, below), the
 *   int8 head and QUANTIZE / DEQUANTIZE (head_i8 and quantize, below).  Kernel time at batch 256 against the float entry at the same shape: 0.80 of it on the
 *   3x3 / 2 stem, 0.41 on the 7x7 / 2 stem, 0.57 on the 1x1 shortcut (profiles/conv2d_i8).
 *   head_i8: the int8 classifier head of an int8-converted network joins the sections, queued as `head` queues the float one; no
 *   other entry can ask for it, no float predicate takes an int8 MEAN / FULLY_CONNECTED / SOFTMAX and none of these takes a float
 *   one, so a float file's partition is unchanged.  Every activation tensor is int8, quantized with exactly ONE scale and a zero
 *   point in [-128, 127].
 *   MEAN (40): the axis / keep_dims / shape rules of `head`'s MEAN on int8 tensors, and lce_hip_mean_i8_prepare accepts the
 *   descriptor.  ONE lce_hip_mean_i8 launch (a requantizing MEAN included: one arithmetic for every pair of quantizations).
 *   FULLY_CONNECTED (9): the rules of `head`'s with: the weights a constant int8 [N, K] with data in the file whose byte count
 *   matches (compared by division), no zero point other than 0, and 1 or N scales (with more than one, quantized_dimension 0);
 *   the bias absent or a constant int32 [N]; lce_hip_fully_connected_i8_check accepts the descriptor and
 *   lce_hip_fully_connected_i8_prepare the file's constants.  ONE lce_hip_fully_connected_i8 launch; the weights and the
 *   prepared table are uploaded once per model.
 *   SOFTMAX (25): `head`'s rules on int8 tensors, and lce_hip_softmax_i8_check accepts the input scale, beta and the output
 *   quantization, which must be exactly (1/256, -128).  ONE lce_hip_softmax_i8 launch.
 *   A hybrid FULLY_CONNECTED (float input, int8 weights), int16 and uint8 tensors, a weight zero point, another softmax output
 *   quantization stay with the host.
 *   quantize: the builtin QUANTIZE (114) float32 -> int8 and DEQUANTIZE (6) int8 -> float32 join the sections: one non-constant
 *   input and one output of the same shape, rank 2 or 4 with positive extents, the int8 side quantized as above.  They join the
 *   epoch in which they become ready, and `stem` applies to a QUANTIZE at the graph's input as to any enabled opt-in.  ONE
 *   lce_hip_quantize_f32_i8 / lce_hip_dequantize_i8_f32 launch each.  A QUANTIZE with an int8 input (a requantization) stays with
 *   the host.  With every name an int8-converted network with a float interface is ONE section from the float image to the
 *   float probabilities, provided it holds no depthwise convolution (depthwise_i8, next).
 *   depthwise_i8: the quantized builtin DEPTHWISE_CONV_2D (4) of an int8-converted network -- the fixed 3x3 / 2 blur of each of
 *   QuickNet's transitions, the depthwise 3x3 / 2 of its stem -- joins the sections; no other entry can ask for it, no bit and no
 *   struct size enables it, and `depthwise` takes float tensors only, so a float file's partition is unchanged.  It qualifies
 *   under the rules of conv2d_i8 with these replacements: the DepthwiseConv2DOptions table is present; the filter is a constant
 *   int8 [1, fh, fw, Cout] with data in the file whose byte count matches; depth_multiplier >= 1 and Cout == Cin x
 *   depth_multiplier == the output's channels; 1 or Cout filter scales (with more than one, quantized_dimension 3); the declared
 *   output height and width are what the padding rule gives; and lce_hip_depthwise_conv2d_i8_check accepts the descriptor and
 *   lce_hip_depthwise_conv2d_i8_prepare the file's constants.  A dilation, hybrid weights, a filter zero point, scales along
 *   another dimension, a float bias and a missing options table leave it with the host, as before.  It joins the epoch in which
 *   it becomes ready, and `stem` applies to it.  lce_tflite_model_run_section runs it as ONE lce_hip_depthwise_conv2d_i8 launch
 *   -- TFLite's integer arithmetic byte for byte -- whose filter and prepared table are uploaded once per model; a following
 *   LceQuantize folds into the launch's bits, and the int8 tensor is written only when something else reads it or the section
 *   delivers it.  With every name an int8 QuickNet with a float interface is ONE section from the float image to the float
 *   probabilities.  Still the host's: dilated, hybrid, uint8 or int16 depthwise convolutions.
 *   activation: a standalone float RELU (19), RELU_N1_TO_1 (20), RELU6 (21), LOGISTIC (14) or PRELU (54) joins the sections -- the
 *   RPReLU of a ReActNet (ADD, PRELU, ADD), the sigmoid of a squeeze-and-excite gate.  One input (PRELU: two) and one output;
 *   input and output float32 of the same shape, of rank 2 or 4 with positive extents, the input non-constant; PRELU's alpha a
 *   constant float32 with data in the file, of shape [C], [1,1,C], [1,1,1,C], [1] or [].  It joins the epoch in which it becomes
 *   ready, and `stem` applies to it as to any opt-in.  It is a step of the elementwise chain: lce_tflite_model_run_section extends
 *   a chain of absorbed ADD / MUL (`elementwise`) through it by the chain's own rules (one reader, not a section output, up to 8
 *   steps), and a chain that holds one runs as ONE lce_hip_elementwise_ex launch (its arithmetic, LOGISTIC's stated bytes
 *   included: include/lce_hip.h) whose bit output replaces a following LceQuantize: with `elementwise,activation` the whole tail
 *   of a ReActNet block behind its binary convolution -- batch norm, shortcut, shift, PRELU, shift, sign bits -- is one pass over
 *   the tensor.  A chain of ADD / MUL alone still runs through lce_hip_elementwise.
 *   reshape: a builtin RESHAPE (22) of a non-constant float32, int8 or int32 tensor joins the sections when it keeps the batch:
 *   input and output of the same type (int8: the same quantization), of rank 2 or 4 with positive extents, the same leading
 *   extent and the same element count behind it -- Flatten in front of a Dense layer, Reshape((1,1,C)) of a gate.  It is judged
 *   by the DECLARED shape of its output tensor; its optional second input must be a constant.  It is a view of the same bytes: no
 *   launch, and at most one device-to-device copy where the output has a buffer of its own (the section delivers it).
 *   gate: a float ADD (0) / MUL (18) whose two inputs are both non-constant, one of the output's [b,H,W,C] shape and the other
 *   [b,1,1,C] -- the per-image scale of a RealToBinaryNet block -- joins the sections, with a fused activation lce_hip_elementwise
 *   knows.  It is a step of the same chain (a PER_IMAGE_CHANNEL operand of lce_hip_elementwise_ex); the gate is always the
 *   operand, the [b,H,W,C] tensor the one streamed.  A [b,C] operand does not qualify: TFLite's broadcast aligns it to the
 *   trailing axes, so it is not per image.
 *   None of the three moves anything unless it is named.  Still the host's: TANH, HARD_SWISH, LEAKY_RELU, int8 activations, a full
 *   [H,W,C] PRELU alpha, rank-2 ADD / MUL (the dense batch norm of BinaryAlexNet), a RESHAPE that moves the batch extent or whose
 *   shape is computed at run time, PAD.
 *   binary_dense: a binarized Dense layer (larq's QuantDense behind a sign: BinaryAlexNet's and XNOR-Net's classifier layers, a
 *   binarized MLP) joins the sections and runs on the FP4 matrix cores.  The converter has no binary fully-connected operator: it
 *   leaves LceQuantize -> LceDequantize -> a float FULLY_CONNECTED (9) whose row o holds only +-s[o].  Such an operator qualifies
 *   under the rules of `head`'s FULLY_CONNECTED with: the input of rank 2 or [b, 1, 1, K]; the input the float32 output of an
 *   LceDequantize whose own input is a non-constant bitpacked int32 tensor of ceil(K/32) words; lce_hip_bfc_check accepts the
 *   descriptor and lce_hip_bfc_prepare the file's weights (every entry of row o of the same magnitude s[o], finite, 2^-100 <=
 *   s[o] <= 2^100, K < 2^23).  Its row of the pass table stands in front of `head`'s, which takes what this one refuses (with
 *   `head` named too).  It is queued with the LCE operators, as the head's.  lce_tflite_model_run_section runs it as ONE
 *   lce_hip_binary_fully_connected launch on the BIT tensor (the prepared sign bits and scales are uploaded once per model); the
 *   first LceQuantize of the section that reads its result folds into the launch by the fold rule, so a hidden binary Dense layer
 *   writes only bits.  An LceDequantize that only binary Dense operators of its own section read, and that the section does not
 *   deliver, is not launched and gets no buffer (its shape is still registered).  LceQuantize and LceDequantize take rank-2
 *   tensors for this, carried as [b, 1, 1, C] like every rank-2 tensor of the walk (a rank-2 SECTION INPUT needs this name or
 *   another that carries rank-2 tensors).  No partition and no launch changes unless it is named.
 *   slice: a builtin STRIDED_SLICE (45) or SLICE (65) that cuts a CHANNEL window out of an image joins the sections -- MeliusNet's
 *   improvement block is w = LceBconv2d(..x..); f = x[..., :C-64]; b = x[..., C-64:] + w; y = CONCATENATION(f, b).  No other entry
 *   can ask for it, and no bit and no struct size enables it.  It qualifies when: it has one output; the data input (0) is a
 *   non-constant float32 or int8 4-D tensor with positive extents; the output has the same type and, for int8, both tensors carry
 *   ONE scale and zero point each, the same; for STRIDED_SLICE the StridedSliceOptions table is present, ellipsis_mask,
 *   new_axis_mask and shrink_axis_mask are 0 and offset is false, begin, end and strides are constant int32 [4] tensors with data
 *   in the file and every stride is 1; for SLICE begin and size are such tensors.  The ranges are resolved as TFLite resolves a
 *   stride of 1: a masked begin is 0 and a masked end the extent, a negative index gets the extent added, begin and end are then
 *   clamped to [0, extent]; a SLICE size of -1 means "to the end" (a negative SLICE begin or a range past the extent is refused).
 *   Axes 0..2 must come out as their whole extent, axis 3 as a window of count >= 1 channels, and the declared output must be
 *   [b, H, W, count].  Everything else stays with the host: another axis, a stride, a shrink mask, a run-time index tensor, another
 *   type.  It joins the epoch in which it becomes ready, and `stem` applies to it as to any opt-in.
 *   lce_tflite_model_run_section decides from the graph alone, when the walk reaches the slice, whether its output is a WINDOW
 *   TENSOR: one the section does not deliver and that has exactly one reader, later in the section, which is (a) an absorbed
 *   CONCATENATION (`concat`) of float32 or int8 tensors, or (b) an `elementwise`-absorbed float ADD with fused activation NONE, whose
 *   other input is a non-constant tensor of the window's shape that is neither produced by an operator of the elementwise chain's
 *   kinds (`elementwise`, `activation`, `gate`) in this section nor itself a window tensor, and whose output is not delivered and
 *   has exactly one reader, a CONCATENATION as in (a).  Such a slice launches nothing and gets no buffer (its shape is still
 *   registered); in case (b) neither does the ADD, whose output is the window with an addend.  An absorbed CONCATENATION with at
 *   least one window tensor among its inputs runs as ONE lce_hip_join_windows launch (its plain inputs are whole-tensor windows;
 *   the first LceQuantize that reads it folds, as for every join): with `elementwise,concat,slice` the improvement block is one
 *   pass that reads x and w once and writes y once, and a MeliusNet body is ONE section.  Any other absorbed slice is ONE
 *   lce_hip_join_windows launch with one window, into which a following LceQuantize folds by the fold rule.  A CONCATENATION
 *   without a window tensor still runs on lce_hip_concat, byte for byte as before.  Nothing moves unless it is named.  Still the
 *   host's: SPLIT / SPLIT_V, slices of other axes or with strides, slices of bit tensors.
 *   elementwise_i8: the int8 tail of a ReActNet-style block -- LceBconv2d (int8 out), ADD shortcut, ADD per-channel shift, PRELU,
 *   ADD per-channel shift, LceQuantize -- a standalone int8 RELU, and the int8 -> int8 QUANTIZE the converter puts in front of a
 *   CONCATENATION whose inputs differ in scale join the sections.  An operator qualifies when its output is int8 and 4-D with
 *   positive extents, the tensor it streams is a non-constant int8 tensor of the output's shape (batch ignored), every tensor
 *   carries ONE scale and a zero point in [-128, 127], and it is one of: ADD with exactly one constant operand of shape [C],
 *   [1,1,1,C], [1] or [] whose data is in the file (as many bytes); PRELU with a constant alpha of shape [C], [1,1,C], [1,1,1,C],
 *   [1] or []; RELU, RELU_N1_TO_1, RELU6; QUANTIZE int8 -> int8 -- and lce_hip_elementwise_i8_prepare accepts it, as a chain of
 *   one step, with the file's constants (an ADD whose real multiplier is outside (0, 1) stays with the host, as for int8_add).  It
 *   joins the epoch in which it becomes ready.  lce_tflite_model_run_section extends a chain through consecutive absorbed
 *   operators of this kind by the elementwise chain's rules (each step reads only the previous result, which nothing else reads and
 *   the section does not deliver; up to 8 steps), prepares ONE table for the chain, uploads it once per model, folds the first
 *   LceQuantize that reads the result and launches lce_hip_elementwise_i8 ONCE.  With int8_add also named, an absorbed residual
 *   ADD whose sum only such a chain reads becomes the chain's head instead of a launch of its own: that launch is counted by
 *   lce_tflite_model_elementwise_i8_stats (the ADD among its operators), not by lce_tflite_model_int8_add_stats.  With
 *   `int8_add,elementwise_i8` the body of an int8 ReActNet is ONE section and each block's tail ONE launch.  Without the name
 *   every partition, launch and counter is what it was; with it a float file's partition is unchanged.  Still the host's: a full
 *   [H,W,C] alpha, a non-constant alpha, per-channel-quantized constants, uint8 / int16 tensors, rank-2 tensors (int8 MUL and int8
 *   LOGISTIC are gate_i8's).
 *   gate_i8: the squeeze-and-excite gate of an int8-converted RealToBinaryNet block -- y = LceBconv2d (int8 out); MEAN(y),
 *   FULLY_CONNECTED, FULLY_CONNECTED, LOGISTIC, RESHAPE [b,1,1,C]; ADD(MUL(y, gate), x) -- joins the sections (MEAN and
 *   FULLY_CONNECTED through head_i8, RESHAPE through reshape, the ADD through int8_add).  An int8 LOGISTIC qualifies with one
 *   non-constant input and an output of the same shape, of rank 2 or 4 with positive extents, both with ONE scale and a zero point
 *   in [-128, 127], when lce_hip_logistic_int8_prepare accepts the quantization (the output at exactly (1/256, -128)); its 256-byte
 *   table is uploaded once per model and the launch is lce_hip_logistic_int8.  An int8 MUL qualifies with two non-constant inputs
 *   and a 4-D output with positive extents, all with ONE scale and a zero point in [-128, 127], one input of the output's shape and
 *   the other of that shape too or [b,1,1,C] (in either slot; a [b,C] operand does not qualify), an activation in NONE..RELU6, when
 *   lce_hip_mul_int8_prepare accepts; a constant operand stays with the host.  Both join the epoch in which they become ready.
 *   lce_tflite_model_run_section launches lce_hip_mul_int8 ONCE per MUL.  With int8_add also named, when the product's ONLY reader
 *   is an absorbed residual int8 ADD of the same shape and the section does not deliver the product, the MUL and the ADD are ONE
 *   launch (has_add; the product is never written, and lce_tflite_model_section_tensor_shape refuses it): the ADD is then
 *   counted by lce_tflite_model_gate_i8_stats, not by lce_tflite_model_int8_add_stats.  An ADD whose other input has no buffer of
 *   its own (the channel window of an absorbed slice) is not fused.  Otherwise the ADD stays int8_add's.  Either way the first LceQuantize that reads the result
 *   folds into the launch, and the int8 tensor is written only if something else reads it.  With
 *   `head_i8,reshape,int8_add,gate_i8` the body of an int8 RealToBinaryNet is ONE section.  Without the name every partition,
 *   launch and counter is what it was; with it a float file's partition is unchanged.  Still the host's: int8 MUL by a constant,
 *   a [b,C] operand, uint8 / int16 tensors.
 *   transition: a name that enables no operator -- the partition is what it is without it -- and changes how one pair runs.  An
 *   absorbed float MAX_POOL_2D ("pool") whose pooled tensor the section does not deliver and whose ONLY reader is an absorbed float
 *   DEPTHWISE_CONV_2D of this section ("depthwise") that reads it as its input runs WITH that convolution as ONE
 *   lce_hip_pool_depthwise_f32 launch, when the entry's own check accepts the two descriptors: QuickNet's transition (pool 2x2 / 1
 *   SAME, then the 3x3 / 2 blur), whose pooled map, as large as the pool's input, is then never written -- the walk holds no tensor
 *   of that name and lce_tflite_model_section_tensor_shape refuses it.  The first LceQuantize that reads the blurred map folds into
 *   the launch as it folds into the depthwise launch.  The bytes are those of the two launches.  Such a launch is counted by
 *   lce_tflite_model_transition_stats and by neither lce_tflite_model_pool_stats nor lce_tflite_model_depthwise_stats.  A pooled tensor
 *   with a second reader or one the section delivers, and an AVERAGE pool, run as two launches as before -- and so does an int8
 *   pair: lce_hip_pool_depthwise_i8 exists and gives the two launches' bytes, but measured slower than they are
 *   (profiles/transition/layers.txt), so the reader does not call it. */
lce_tflite_model* lce_tflite_model_open_passes(const void* data, size_t size, const char* passes, char* err, size_t err_len);
void lce_tflite_model_close(lce_tflite_model* model);

int32_t lce_tflite_model_num_tensors(const lce_tflite_model* model);
int32_t lce_tflite_model_num_operators(const lce_tflite_model* model);
/* Subgraph inputs / outputs (tensor indices); returns the count, fills up to `cap`. */
int32_t lce_tflite_model_inputs(const lce_tflite_model* model, int32_t* indices, int32_t cap);
int32_t lce_tflite_model_outputs(const lce_tflite_model* model, int32_t* indices, int32_t cap);

typedef struct lce_tflite_tensor_info {
  int32_t type;            /* schema TensorType */
  int32_t rank;
  int32_t dims[8];
  int32_t quantized;       /* 1 when scale / zero_point are present */
  float scale;
  int32_t zero_point;
  const void* data;        /* constant data inside the model buffer, or NULL */
  size_t bytes;
  const char* name;        /* owned by the model */
} lce_tflite_tensor_info;
lce_hip_status lce_tflite_model_tensor(const lce_tflite_model* model, int32_t index, lce_tflite_tensor_info* info);

typedef struct lce_tflite_operator_info {
  int32_t builtin_code;    /* 32 = CUSTOM */
  const char* custom_code; /* "LceBconv2d", "LceQuantize", "LceDequantize", "LceBMaxPool2d", or "" */
  const int32_t* inputs;   /* tensor indices (-1: optional input absent); owned by the model */
  int32_t num_inputs;
  const int32_t* outputs;
  int32_t num_outputs;
  const uint8_t* custom_options;   /* flexbuffer map, as written by mlir/ir/lce_ops.cc:36-51 */
  size_t custom_options_size;
} lce_tflite_operator_info;
/* The whole scale vector of tensor `index` (lce_tflite_tensor_info::scale is its first element): up to `cap` scales are copied
 * to `scales` (nullable) and QuantizationParameters.quantized_dimension is reported (nullable).  Returns the number of scales
 * in the file (0: not quantized), -1 for a bad argument. */
int32_t lce_tflite_model_tensor_scales(const lce_tflite_model* model, int32_t index, float* scales, int32_t cap, int32_t* quantized_dimension);
lce_hip_status lce_tflite_model_operator(const lce_tflite_model* model, int32_t index, lce_tflite_operator_info* info);
/* fused_activation_function of a builtin ADD / MUL (AddOptions / MulOptions: lce_hip_activation values, and 4 TANH /
 * 5 SIGN_BIT as the file says); 0 (NONE) when the options table is absent and for every other operator. */
lce_hip_status lce_tflite_model_operator_activation(const lce_tflite_model* model, int32_t index, int32_t* activation);
/* axis of a builtin CONCATENATION (ConcatenationOptions, as the file says: may be negative); 0 when the options table is
 * absent and for every other operator.  Its fused activation is reported by the call above. */
lce_hip_status lce_tflite_model_operator_axis(const lce_tflite_model* model, int32_t index, int32_t* axis);

/* Pool2DOptions of a builtin AVERAGE_POOL_2D / MAX_POOL_2D, as the file says: options[0..4] = padding (0 SAME, 1 VALID),
 * stride_w, stride_h, filter_width, filter_height; all 0 when the options table is absent and for every other operator.
 * Its fused activation is reported by lce_tflite_model_operator_activation. */
lce_hip_status lce_tflite_model_operator_pool2d(const lce_tflite_model* model, int32_t index, int32_t options[5]);

/* Conv2DOptions of a builtin CONV_2D, as the file says: options[0..4] = padding (0 SAME, 1 VALID), stride_w, stride_h,
 * dilation_w_factor, dilation_h_factor (schema default 1).  {0, 0, 0, 1, 1} when the options table is absent and for every
 * other operator.  Its fused activation is reported by lce_tflite_model_operator_activation. */
lce_hip_status lce_tflite_model_operator_conv2d(const lce_tflite_model* model, int32_t index, int32_t options[5]);

/* DepthwiseConv2DOptions of a builtin DEPTHWISE_CONV_2D, as the file says: options[0..5] = padding (0 SAME, 1 VALID), stride_w,
 * stride_h, depth_multiplier, dilation_w_factor, dilation_h_factor (schema default 1).  {0, 0, 0, 0, 1, 1} when the options
 * table is absent and for every other operator.  Its fused activation is reported by lce_tflite_model_operator_activation. */
lce_hip_status lce_tflite_model_operator_depthwise(const lce_tflite_model* model, int32_t index, int32_t options[6]);

/* ReducerOptions of a builtin MEAN (or another reducer), as the file says: *keep_dims is 0 or 1; 0 when the options table is absent
 * and for every other operator. */
lce_hip_status lce_tflite_model_operator_reducer(const lce_tflite_model* model, int32_t index, int32_t* keep_dims);

/* FullyConnectedOptions of a builtin FULLY_CONNECTED, as the file says: options[0..2] = fused_activation_function,
 * weights_format (0 DEFAULT, 1 SHUFFLED4x16INT8), keep_num_dims (0 or 1).  *present is 0, and options {0, 0, 0}, when the
 * options table is absent and for every other operator. */
lce_hip_status lce_tflite_model_operator_fully_connected(const lce_tflite_model* model, int32_t index, int32_t options[3], int32_t* present);

/* SoftmaxOptions of a builtin SOFTMAX, as the file says: *beta.  *present is 0, and *beta 0, when the options table is absent
 * and for every other operator. */
lce_hip_status lce_tflite_model_operator_softmax(const lce_tflite_model* model, int32_t index, float* beta, int32_t* present);

/* Binary SECTIONS of a mixed graph.  A converted model interleaves builtin float operators (the stem, batch norms, adds,
 * the head) with LCE custom ops; what this library runs are the maximal groups of LCE ops that can execute without a
 * builtin operator in between -- the partition a TFLite delegate would be handed (TensorFlow Lite's
 * PartitionGraphIntoIndependentNodeSubsets, restated): epochs alternate between LCE operators and all others, starting
 * with LCE; in an epoch EVERY operator of the epoch's kind whose inputs are all ready joins -- wherever it stands in the
 * file -- repeatedly, until none is left; the LCE operators of one epoch, sorted by index, are one section.  On a chain
 * that is "cut at every builtin operator"; on a branched graph an LCE op further down the file belongs to an earlier
 * section when nothing it reads depends on a builtin operator in between.  The reference runs whole
 * graphs through one interpreter (tflite/python/interpreter_base.py:74-95, examples/lce_minimal.cc:28-62); a host that
 * keeps TensorFlow Lite for the float operators calls a section between them: feed `inputs`, collect `outputs`.
 *   ops     : operator indices of the section, in execution order
 *   inputs  : non-constant tensors the section reads but does not produce
 *   outputs : tensors it produces that an operator outside the section, or the graph's output list, reads
 * The arrays are owned by the model. */
typedef struct lce_tflite_section_info {
  const int32_t* ops;
  int32_t num_ops;
  const int32_t* inputs;
  int32_t num_inputs;
  const int32_t* outputs;
  int32_t num_outputs;
} lce_tflite_section_info;
int32_t lce_tflite_model_num_sections(const lce_tflite_model* model);
lce_hip_status lce_tflite_model_section(const lce_tflite_model* model, int32_t index, lce_tflite_section_info* info);

/* Runs section `section` on DEVICE tensors at `batch` images per tensor (the file's own leading dimension, which the
 * converter pins to 1, is replaced): the C entry for a host without a TensorFlow Lite interpreter -- what
 * examples/lce_minimal.cc:28-62 / tflite/benchmark/lce_benchmark_main.cc:24-48 do with Interpreter::Invoke, for the
 * binary part of the graph -- and what compute-engine_amd/model_runner.py calls.
 *   inputs_dev[k]  : device pointer of tensor section.inputs[k]  ([batch, H, W, C] in the file's type)
 *   outputs_dev[k] : device buffer for tensor section.outputs[k] (lce_tflite_model_section_tensor_shape says how large)
 * Everything in between stays in device buffers the MODEL owns (grow-only, reused by the next call); plans are made
 * once per (operator, batch, semantics) and cached in the model; an LceBconv2d whose float / int8 output feeds an
 * LceQuantize of the same section writes both tensors from one epilogue (lce_hip_bconv2d_run_dual), the quantize launch
 * disappears.  Asynchronous on `stream` (a hipStream_t, or NULL); calls on one model are serialised by a mutex and must
 * use one stream at a time.  `semantics`: lce_hip_semantics (which registration's SAME-zero behaviour).  Shape inference
 * is the ops' own Prepare (quantization.cc:19-41, bmaxpool.cc:41-77, bconv2d.cc:137-300; an absorbed pool: the padding rule; an absorbed CONV_2D: ceil(in / stride); an absorbed DEPTHWISE_CONV_2D: the padding rule). */
lce_hip_status lce_tflite_model_run_section(lce_tflite_model* model, int32_t section, int32_t batch, int32_t semantics,
                                            const void* const* inputs_dev, void* const* outputs_dev, void* stream);
/* Shape ([N,H,W,C], C in words for bitpacked tensors) and size in bytes of a tensor section `section` reads or produces,
 * at `batch` images.  The walk is 4-D throughout: a rank-2 tensor of the classifier head ([b, C] in the file: the output of a
 * MEAN, a FULLY_CONNECTED or a SOFTMAX) reports {batch, 1, 1, C}; the bytes are the same, and the caller restores the file's
 * rank.  A product that an int8 MUL hands to its residual ADD inside one lce_hip_mul_int8 launch ("gate_i8" with "int8_add") is
 * never written and is no tensor of the walk: asking for it is refused like a tensor the section does not touch.  Host-only
 * (no device needed). */
lce_hip_status lce_tflite_model_section_tensor_shape(lce_tflite_model* model, int32_t section, int32_t tensor, int32_t batch,
                                                     int32_t semantics, int32_t dims[4], size_t* bytes);

/* What the model holds for lce_tflite_model_run_section: plans cached so far (one per operator x batch size x semantics),
 * LceQuantize launches the LAST run folded into a convolution's epilogue, bytes of intermediate buffers.  Any pointer may
 * be NULL. */
void lce_tflite_model_run_stats(lce_tflite_model* model, int32_t* cached_plans, int32_t* fused_quantize_ops, size_t* scratch_bytes);
/* The LAST run's lce_hip_elementwise launches (LCE_TFLITE_SECTIONS_ELEMENTWISE): launches, ADD / MUL operators they ran,
 * LceQuantize operators whose launch they absorbed.  Any pointer may be NULL. */
void lce_tflite_model_elementwise_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded);
/* The LAST run's lce_hip_add_int8 launches (LCE_TFLITE_SECTIONS_INT8_ADD): launches (one per absorbed ADD) and LceQuantize
 * operators whose launch they absorbed.  Any pointer may be NULL. */
void lce_tflite_model_int8_add_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_concat launches (LCE_TFLITE_SECTIONS_CONCAT): launches (one per absorbed CONCATENATION) and
 * LceQuantize operators whose launch they absorbed.  Any pointer may be NULL. */
void lce_tflite_model_concat_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_pool2d launches (LCE_TFLITE_SECTIONS_EXT_POOL): launches (one per absorbed pool) and LceQuantize
 * operators whose launch they absorbed.  Any pointer may be NULL. */
void lce_tflite_model_pool_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_conv1x1_f32 launches (LCE_TFLITE_SECTIONS_EXT_CONV1X1): launches (one per absorbed CONV_2D) and
 * LceQuantize operators whose launch they absorbed.  Any pointer may be NULL. */
void lce_tflite_model_conv1x1_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_depthwise_conv2d_f32 launches (LCE_TFLITE_SECTIONS_EXT_DEPTHWISE): launches (one per absorbed
 * DEPTHWISE_CONV_2D) and LceQuantize operators whose launch they absorbed.  Any pointer may be NULL. */
void lce_tflite_model_depthwise_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_conv2d_f32 calls (LCE_TFLITE_SECTIONS_EXT_CONV2D): launches (one per absorbed CONV_2D) and the
 * LceQuantize launches folded into them.  Nullable outputs. */
void lce_tflite_model_conv2d_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_conv2d_i8 launches ("conv2d_i8" of lce_tflite_model_open_passes): launches (one per absorbed int8
 * CONV_2D) and the LceQuantize launches folded into them.  Nullable outputs. */
void lce_tflite_model_conv_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's lce_hip_depthwise_conv2d_i8 launches ("depthwise_i8" of lce_tflite_model_open_passes): launches (one per
 * absorbed int8 DEPTHWISE_CONV_2D) and the LceQuantize launches folded into them.  Nullable outputs. */
void lce_tflite_model_depthwise_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's launches for the classifier head ("head" of lce_tflite_model_open_passes): lce_hip_pool2d launches that ran a
 * MEAN, lce_hip_fully_connected_f32 launches, lce_hip_softmax_f32 launches.  Nullable outputs. */
void lce_tflite_model_head_stats(lce_tflite_model* model, int32_t* mean, int32_t* fully_connected, int32_t* softmax);
/* The LAST run's binary Dense layers ("binary_dense" of lce_tflite_model_open_passes): lce_hip_binary_fully_connected launches, the
 * LceDequantize operators that were not launched because only such layers read them, and the LceQuantize launches the layers
 * absorbed.  Nullable outputs. */
void lce_tflite_model_binary_dense_stats(lce_tflite_model* model, int32_t* launches, int32_t* dequantize_skipped, int32_t* quantize_absorbed);
/* The LAST run's launches for the int8 head ("head_i8"): lce_hip_mean_i8, lce_hip_fully_connected_i8 and lce_hip_softmax_i8
 * launches; and for the float / int8 boundary ("quantize"): lce_hip_quantize_f32_i8 and lce_hip_dequantize_i8_f32 launches. */
void lce_tflite_model_head_i8_stats(lce_tflite_model* model, int32_t* mean, int32_t* fully_connected, int32_t* softmax);
void lce_tflite_model_quantize_stats(lce_tflite_model* model, int32_t* quantize, int32_t* dequantize);
/* The LAST run's lce_hip_elementwise_ex launches ("activation" and "gate" of lce_tflite_model_open_passes): launches (one per
 * chain that holds a standalone activation or a gate), the operators of every kind -- ADD / MUL included -- inside them, and the
 * LceQuantize launches they absorbed.  Chains of ADD / MUL alone are lce_tflite_model_elementwise_stats', as before. */
void lce_tflite_model_activation_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded);
/* ... those of them that hold a gate, and the LceQuantize launches these absorbed. */
void lce_tflite_model_gate_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded);
/* The LAST run's absorbed RESHAPE operators ("reshape"): those that were a view of their input's buffer, and those that cost one
 * device-to-device copy. */
void lce_tflite_model_reshape_stats(lce_tflite_model* model, int32_t* views, int32_t* copies);
/* The LAST run's lce_hip_join_windows launches ("slice" of lce_tflite_model_open_passes): launches (standalone slices and
 * CONCATENATIONs with a window tensor among their inputs), the LceQuantize launches folded into them, and those of the launches
 * that took over a CONCATENATION (lce_tflite_model_concat_stats counts lce_hip_concat launches only).  Nullable outputs. */
void lce_tflite_model_slice_stats(lce_tflite_model* model, int32_t* launches, int32_t* quantize_folded, int32_t* joins);
/* The LAST run's lce_hip_elementwise_i8 launches ("elementwise_i8" of lce_tflite_model_open_passes): launches (one per chain),
 * operators of every kind inside them (a residual ADD taken as a chain's head included) and LceQuantize launches folded into
 * them.  Any pointer may be NULL. */
void lce_tflite_model_elementwise_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded);
/* The LAST run's lce_hip_mul_int8 launches ("gate_i8" of lce_tflite_model_open_passes): launches (one per absorbed int8 MUL), the
 * MUL and residual ADD operators inside them (2 for a launch with has_add, 1 otherwise) and LceQuantize launches folded into
 * them.  The int8 LOGISTIC launches are not among them.  Any pointer may be NULL. */
void lce_tflite_model_gate_i8_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded);
/* The LAST run's lce_hip_pool_depthwise_f32 launches ("transition" of lce_tflite_model_open_passes): launches, the MAX_POOL_2D
 * and DEPTHWISE_CONV_2D operators inside them (2 per launch) and LceQuantize launches folded into them.  Any pointer may be NULL. */
void lce_tflite_model_transition_stats(lce_tflite_model* model, int32_t* launches, int32_t* ops_folded, int32_t* quantize_folded);

/* HIP graphs for lce_tflite_model_run_section (off by default).  A binary section is a chain of short kernels -- QuickNet's
 * last layers take 10-17 us each -- and a host call per kernel leaves gaps between them.  With graphs on, the launches of a
 * section are recorded once per (section, batch, semantics, stream, tensor pointers) and replayed as ONE launch: the first call
 * with such a key runs eagerly (plans, uploads, buffers), the second records and launches, later ones replay.  Needs a stream
 * of its own (not NULL: the null stream cannot be recorded; lce_hip_stream_create).  The recording holds the device pointers it
 * was given: call with the same tensors to replay, with others to get another recording; turning graphs off drops them all.
 * If a section cannot be recorded it simply keeps running eagerly.  graph_stats: recordings made / launches served by one. */
void lce_tflite_model_use_hip_graphs(lce_tflite_model* model, int32_t on);
void lce_tflite_model_graph_stats(lce_tflite_model* model, int32_t* recorded, int32_t* replays);

/* Builds a ready-to-run plan for operator `index`, which must be an LceBconv2d: descriptor
 * from the op's option map + tensor shapes / types / output quantization exactly as
 * bconv2d::Init + Prepare collect them (tflite/kernels/bconv2d.cc:85-131,137-300), weights
 * from the constant tensors (OneTimeSetup, :324-392).  `batch` > 0 overrides the batch
 * dimension recorded in the file (the converter pins it to 1, mlir/tf_tfl_passes.cc:141-144).
 * `semantics` selects which registration's behaviour to follow (lce_hip_semantics). */
lce_hip_status lce_tflite_model_bconv2d_plan(const lce_tflite_model* model, int32_t index, int32_t batch,
                                             int32_t semantics, lce_hip_bconv2d_plan** plan);

/* Option lookup on any LCE op's custom_options (bmaxpool: filter_height, filter_width,
 * stride_height, stride_width, padding).  Returns 0 and writes *value when the key exists. */
int lce_tflite_option_int(const uint8_t* custom_options, size_t size, const char* key, int32_t* value);

/* Message of the last failing lce_tflite_model_* call on this thread (plan creation failures
 * report through lce_hip_last_error()). */
const char* lce_tflite_model_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LCE_TFLITE_MODEL_H_ */
