/*
 * lce_hip.h -- C ABI of the MI355X-native LceBconv2d / LceQuantize hot path.
 *
 * This is the drop-in boundary under Larq Compute Engine's TFLite custom-op glue: the
 * C++ op glue (compute-engine_amd/csrc/tflite/, same Register_* entry points as the
 * reference) and any other host language bind THESE functions -- plain pointers,
 * sizes and int status codes, no C++/torch/HIP types in any signature.  Each entry
 * point names the reference interface it replaces (paths relative to
 * /root/reference/larq_compute_engine/).
 *
 * Conventions
 *   - every function returns LCE_HIP_OK (0) or an error code; lce_hip_last_error()
 *     returns a thread-local human-readable message for the last failure;
 *   - `*_dev` pointers are device (HBM) pointers of the current HIP device, `*_host`
 *     pointers are ordinary host memory; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - tensors use the reference's layouts: activations NHWC with channels bitpacked
 *     into int32 words LSB-first (core/types.h:41, core/bitpacking/bitpack.h:72-110),
 *     filters OHWI bitpacked (tflite/kernels/bconv2d.cc:145-152), outputs NHWC;
 *   - there is NO CPU fallback: without a usable GPU the compute entry points fail
 *     with LCE_HIP_ERR_NO_DEVICE.
 */
#ifndef LCE_HIP_H_
#define LCE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCE_HIP_ABI_VERSION 3   /* 3 (round 6): + lce_hip_bconv2d_plan_int8_epilogue; additive */

typedef enum lce_hip_status {
  LCE_HIP_OK = 0,
  LCE_HIP_ERR_INVALID = 1,     /* bad argument / rejected by the same checks as Prepare */
  LCE_HIP_ERR_UNSUPPORTED = 2, /* valid for the reference but outside what this build runs */
  LCE_HIP_ERR_RUNTIME = 3,     /* a HIP call failed */
  LCE_HIP_ERR_NO_DEVICE = 4    /* no gfx950 device / HIP runtime unusable */
} lce_hip_status;

/* element types of the tensors that cross the boundary */
typedef enum lce_hip_dtype {
  LCE_HIP_F32 = 0,       /* kTfLiteFloat32 */
  LCE_HIP_I8 = 1,        /* kTfLiteInt8    */
  LCE_HIP_BITPACKED = 2, /* kTfLiteInt32 holding 32 sign bits (TBitpacked, core/types.h:41) */
  LCE_HIP_BOOL = 3       /* kTfLiteBool (1 byte) */
} lce_hip_dtype;

/* tflite schema enums as they arrive in the op's flexbuffer options
 * (tflite/kernels/bconv2d.cc:94-124, tflite/kernels/utils.h:10-35) */
typedef enum lce_hip_padding { LCE_HIP_PADDING_SAME = 0, LCE_HIP_PADDING_VALID = 1 } lce_hip_padding;
typedef enum lce_hip_activation {
  LCE_HIP_ACT_NONE = 0, LCE_HIP_ACT_RELU = 1, LCE_HIP_ACT_RELU_N1_TO_1 = 2, LCE_HIP_ACT_RELU6 = 3
} lce_hip_activation;

/* Which reference registration's semantics to follow.  They only differ for SAME
 * padding with pad_values == 0 (tflite/kernels/bconv2d.cc:188-200):
 *   REFERENCE : Register_BCONV_2D_REF -- exact integer zero padding
 *               (core/bconv2d/reference.h:76-103); needs an even channels_in.
 *   OPTIMIZED : Register_BCONV_2D_OPT_BGEMM / _OPT_INDIRECT_BGEMM -- one-padded
 *               convolution plus float correction (core/bconv2d/zero_padding_correction.h);
 *               float output and no fused activation only. */
typedef enum lce_hip_semantics { LCE_HIP_SEM_REFERENCE = 0, LCE_HIP_SEM_OPTIMIZED = 1 } lce_hip_semantics;

/* ------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------- */
int lce_hip_abi_version(void);
const char* lce_hip_last_error(void);
/* "product", or "experiment" for a library built with measuring aids compiled in (timing ablations whose results are
 * wrong by construction, time-stamp builds: csrc/lce_experiments.h).  The library csrc/Makefile builds is "product" and
 * cannot be anything else (the switches are compile errors there); a host may refuse to load anything else. */
const char* lce_hip_build_flavor(void);
/* number of usable HIP devices (0 when there is none; never fails) */
int lce_hip_device_count(void);
lce_hip_status lce_hip_set_device(int device);

/* Device-memory plumbing for hosts that have no HIP binding of their own (the TFLite
 * glue stages interpreter tensors through these). */
lce_hip_status lce_hip_malloc(void** dev_ptr, size_t bytes);
lce_hip_status lce_hip_free(void* dev_ptr);
lce_hip_status lce_hip_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
lce_hip_status lce_hip_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
lce_hip_status lce_hip_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);   /* asynchronous on `stream`, capturable */
lce_hip_status lce_hip_memset(void* dst_dev, int value, size_t bytes, void* stream);
/* Page-locks [host_ptr, host_ptr + bytes) (hipHostRegister) so that copies from / to it are truly
 * asynchronous and lce_hip_bconv2d_run_host can overlap them with compute.  For buffers the caller keeps
 * alive and reuses (the interpreter's tensor arena); the range must be unregistered before it is freed. */
lce_hip_status lce_hip_host_register(void* host_ptr, size_t bytes);
lce_hip_status lce_hip_host_unregister(void* host_ptr);
lce_hip_status lce_hip_stream_create(void** stream);
lce_hip_status lce_hip_stream_destroy(void* stream);
lce_hip_status lce_hip_stream_synchronize(void* stream);
/* HIP graphs for hosts without a HIP binding: everything launched on `stream` (a stream from lce_hip_stream_create, not the
 * null stream) between begin and end is recorded instead of executed -- lce_hip_bconv2d_run / _run_dual of plans that have
 * run once before, lce_hip_bitpack / _unpack / _bmaxpool -- and comes back as ONE launchable object: a chain of short layers
 * replays without a host call per kernel.  The recorded launches keep the device pointers they were given.  A plan's first run
 * (uploads, a known-answer check) cannot be recorded: run the sequence once eagerly first.  end_capture returns the error of
 * a failed recording and leaves the stream usable. */
lce_hip_status lce_hip_graph_begin_capture(void* stream);
lce_hip_status lce_hip_graph_end_capture(void* stream, void** graph);
lce_hip_status lce_hip_graph_launch(void* graph, void* stream);
lce_hip_status lce_hip_graph_destroy(void* graph);

/* ------------------------------------------------------------------------------------
 * LceQuantize / LceDequantize
 * ---------------------------------------------------------------------------------- */

/* ceil(n / 32): core/bitpacking/bitpack.h:24-26 (GetBitpackedSize) */
int32_t lce_hip_bitpacked_size(int32_t unpacked_elements);

/* Replaces core::bitpacking::bitpack_matrix<T> (core/bitpacking/bitpack.h:248-308) as
 * called by QuantizeEval (tflite/kernels/quantization.cc:76-114): packs each of the
 * `rows` rows of `cols` elements into ceil(cols/32) words; bit = (x < zero_point)
 * (float: zero_point must be 0, test is x < 0; bool: pass zero_point 1), padding bits 0.
 * in_type is F32, I8 or BOOL. */
lce_hip_status lce_hip_bitpack(lce_hip_dtype in_type, const void* in_dev, size_t rows,
                               size_t cols, int32_t zero_point, int32_t* out_dev, void* stream);

/* Replaces core::bitpacking::unpack_matrix<T> (bitpack.h:327-346) as called by
 * DequantizeEval (quantization.cc:116-147).  out_type F32: bit0 -> +1, bit1 -> -1;
 * I8: zero_point +- round(1/scale) clamped to int8; BOOL: bit0 -> true. */
lce_hip_status lce_hip_unpack(lce_hip_dtype out_type, const int32_t* in_dev, size_t rows,
                              size_t cols, float scale, int32_t zero_point, void* out_dev,
                              void* stream);

/* ------------------------------------------------------------------------------------
 * Float ADD / MUL between binary layers (TFLite builtins) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* A converted residual binary network runs, between two LceBconv2d, the builtin float ADD / MUL of its batch norm
 * and its residual shortcut, then the next layer's LceQuantize.  lce_hip_elementwise runs such a chain in ONE pass
 * over an NHWC float32 tensor `in_dev` ([rows, channels], rows = N*H*W): per element
 *     v = in;  for each step: v = fl(v op operand) (one rounding, never an fma); v = min(max(v, lo), hi)
 * where [lo, hi] is CalculateActivationRange of the step's activation (NONE = [-FLT_MAX, FLT_MAX]: an infinity
 * becomes +-FLT_MAX; RELU = [0, FLT_MAX]; RELU_N1_TO_1 = [-1, 1]; RELU6 = [0, 6]) and std::max(a, b) = a < b ? b : a
 * (RELU(-0.0) = -0.0); subnormals are kept.  `out_dev` (nullable) gets v; `out_bits_dev` (nullable) gets the
 * LceQuantize of v as lce_hip_bitpack(F32, ...) writes it: bit = v < 0, ceil(channels/32) words per row.  out_dev
 * may be in_dev or a TENSOR operand (in place).  Steps (1..8) are read at the call; their device arrays at run time.
 * Zero rows or channels is a no-op (checked before the pointers: an empty tensor may have none).  Asynchronous on
 * `stream`. */
typedef enum lce_hip_ew_op { LCE_HIP_EW_ADD = 0, LCE_HIP_EW_MUL = 1 } lce_hip_ew_op;
typedef enum lce_hip_ew_operand {
  LCE_HIP_EW_SCALAR = 0,        /* `scalar` */
  LCE_HIP_EW_PER_CHANNEL = 1,   /* values[channels] (a batch norm's constants) */
  LCE_HIP_EW_TENSOR = 2         /* values[rows * channels] (the residual) */
} lce_hip_ew_operand;
typedef struct lce_hip_ew_step {
  int32_t op, operand;      /* lce_hip_ew_op, lce_hip_ew_operand */
  const float* values;      /* device: [channels] or [rows * channels]; NULL for SCALAR */
  float scalar;
  int32_t activation;       /* an lce_hip_activation: NONE, RELU, RELU_N1_TO_1 or RELU6 */
} lce_hip_ew_step;
lce_hip_status lce_hip_elementwise(const float* in_dev, size_t rows, size_t channels,
                                   const lce_hip_ew_step* steps, int32_t num_steps,
                                   float* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);

/* lce_hip_elementwise_ex: the same one pass with more kinds of step -- what a ReActNet tail (ADD shift, PRELU, ADD shift), the
 * gate of a squeeze-and-excite block (MUL by a [batch, 1, 1, C] tensor) and a standalone activation need.  The contract for
 * `out_dev`, `out_bits_dev` and in place is lce_hip_elementwise's.  A step (1..8 of them) is one of
 *   ADD / MUL with a SCALAR, PER_CHANNEL or TENSOR operand: exactly lce_hip_elementwise's bytes.
 *   ADD / MUL with a PER_IMAGE_CHANNEL operand: values[batch * channels], batch = rows / rows_per_image; the element of image n,
 *     channel c reads values[n * channels + c].  One rounding per op, never an fma; the step's clamp follows.
 *   CLAMP: no arithmetic, only the clamp of `activation` -- a standalone RELU, RELU_N1_TO_1 or RELU6:
 *     v = v < lo ? lo : v;  v = hi < v ? hi : v.  RELU(-0.0) = -0.0; a NaN passes.  The operand is ignored.
 *   PRELU: v = v >= 0 ? v : fl(v * alpha), alpha the SCALAR or PER_CHANNEL operand.  -0.0 stays -0.0; a NaN takes the multiply and
 *     stays NaN; an infinity is not clamped.  `activation` must be NONE.
 *   LOGISTIC: the library's own bytes (no two libraries agree on them), in float32 operations that NumPy restates
 *     (tests/activation_ref.py), on the SAME E(a) that lce_hip_softmax_f32 states below:
 *       x >= 0:  e = E(-x);  y = 1 / fl(1 + e)
 *       x <  0:  e = E(x);   y = e / fl(1 + e)
 *     both divisions correctly rounded.  A NaN passes unchanged; +inf -> 1; -inf and x < -104 -> +0; -0.0 -> 0.5.  Measured on
 *     1.8e8 arguments: at most 2.40 ulp of the float32 result from 1 / (1 + exp(-x)) in float64 (tests hold
 *     3.40).  `activation` must be NONE; the operand is ignored.
 * `rows_per_image` (H * W of the NHWC tensor) is needed by a PER_IMAGE_CHANNEL operand and may be 0 without one; when it is not
 * 0 it must divide `rows`.  Refused before any device call, LCE_HIP_ERR_INVALID: NULL steps, input, operand or both outputs, an
 * unknown op, operand kind or activation, a PRELU operand that is TENSOR or PER_IMAGE_CHANNEL, an activation on PRELU or LOGISTIC,
 * non-zero reserved fields, a rows_per_image that does not divide rows (or 0 with a per-image operand), a pointer that is not
 * 4-byte aligned.  Zero rows or channels is a no-op.  Asynchronous on `stream`, capturable in a HIP graph, allocates nothing. */
typedef enum lce_hip_ew_op_ex { LCE_HIP_EW_CLAMP = 2, LCE_HIP_EW_PRELU = 3, LCE_HIP_EW_LOGISTIC = 4 } lce_hip_ew_op_ex;   /* after ADD 0, MUL 1 */
typedef enum lce_hip_ew_operand_ex { LCE_HIP_EW_PER_IMAGE_CHANNEL = 3 } lce_hip_ew_operand_ex;   /* after SCALAR 0, PER_CHANNEL 1, TENSOR 2 */
typedef struct lce_hip_ew_step_ex {
  int32_t op, operand;      /* lce_hip_ew_op / _ex, lce_hip_ew_operand / _ex */
  const float* values;      /* device: [channels], [rows * channels] or [batch * channels]; NULL for SCALAR */
  float scalar;
  int32_t activation;       /* an lce_hip_activation: NONE, RELU, RELU_N1_TO_1 or RELU6 */
  int32_t reserved[2];      /* 0 */
} lce_hip_ew_step_ex;
lce_hip_status lce_hip_elementwise_ex(const float* in_dev, size_t rows, size_t channels, size_t rows_per_image,
                                      const lce_hip_ew_step_ex* steps, int32_t num_steps,
                                      float* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);
/* The most blocks lce_hip_elementwise and lce_hip_elementwise_ex launch (4 waves each; a wave strides over the rest).  Host only. */
int32_t lce_hip_elementwise_grid_cap(void);

/* ------------------------------------------------------------------------------------
 * int8 residual ADD between binary layers (TFLite builtin) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* In an int8-converted residual network the batch norm is folded into LceBconv2d and the one operator left between two
 * binary layers is TFLite's builtin int8 ADD of the shortcut.  lce_hip_add_int8 computes it byte for byte as TFLite's
 * default (double-rounding) build does -- which is NOT the correctly rounded (s1 (x1 - z1) + s2 (x2 - z2)) / so:
 *   prepare, once per operator, in double:
 *     left_shift = 20; twice_max = 2 max(s1, s2); (m1, e1) = QuantizeMultiplier(s1 / twice_max); (m2, e2) likewise;
 *     (mo, eo) = QuantizeMultiplier(twice_max / (2^20 so)); [act_min, act_max] = CalculateActivationRangeQuantized
 *   per element, in int32 / int64:
 *     sa = RDivPOT(SRDHM((x1 - z1) << 20, m1), -e1);  sb likewise;  out = clamp(RDivPOT(SRDHM(sa + sb, mo), -eo) + zo)
 * over two NHWC int8 tensors ([rows, channels], rows = N*H*W) in ONE pass.  `out_dev` (nullable) gets the int8 sum and may
 * be in1_dev or in2_dev (in place); `out_bits_dev` (nullable) gets the LceQuantize of the sum at ITS zero point, as
 * lce_hip_bitpack(I8, ..., out_zero_point, ...) writes it: bit = out < zo, ceil(channels/32) words per row.
 * Refused (LCE_HIP_ERR_INVALID, before any pointer is touched): a scale that is not finite and positive, a zero point
 * outside [-128, 127], an activation other than NONE / RELU / RELU_N1_TO_1 / RELU6, a real multiplier outside (0, 1),
 * both outputs NULL.  Zero rows or channels is a no-op.  Asynchronous on `stream`, capturable in a HIP graph, allocates
 * nothing on the device (the parameters travel as kernel arguments; the host keeps what it derived per parameter set). */
typedef struct lce_hip_add_int8_desc {
  float in1_scale; int32_t in1_zero_point;
  float in2_scale; int32_t in2_zero_point;
  float out_scale; int32_t out_zero_point;
  int32_t activation;       /* an lce_hip_activation */
} lce_hip_add_int8_desc;
typedef struct lce_hip_add_int8_params {
  int32_t left_shift, in1_multiplier, in1_shift, in2_multiplier, in2_shift, out_multiplier, out_shift, act_min, act_max;
} lce_hip_add_int8_params;
/* TFLite's Prepare for this operator.  Host only: needs no device. */
lce_hip_status lce_hip_add_int8_prepare(const lce_hip_add_int8_desc* desc, lce_hip_add_int8_params* params);
lce_hip_status lce_hip_add_int8(const lce_hip_add_int8_desc* desc, const int8_t* in1_dev, const int8_t* in2_dev,
                                size_t rows, size_t channels, int8_t* out_dev /* nullable */,
                                int32_t* out_bits_dev /* nullable */, void* stream);
/* The kernel has three variants of the per-element arithmetic that give the same bytes.  For each parameter set the host
 * runs a cheap variant over all 65 536 input pairs against the literal formula and uses it only if every byte agrees:
 *   LITERAL: the formula as written above (three 64-bit products); right for every parameter set.
 *   SPLIT  : one input is a shift ((x - z) << k: its multiplier is 2^30), the other in 24-bit multiply-adds; one 64-bit
 *            multiply-add in the output stage.
 *   SHIFT  : both inputs are shifts (equal scales, power-of-two ratios).
 * lce_hip_add_int8_variant reports the variant lce_hip_add_int8 uses for `desc` (host only).  lce_hip_add_int8_forced runs
 * a given variant -- for tests and measurements -- and refuses one that is not proven for `desc`. */
typedef enum lce_hip_add_int8_variant_id {
  LCE_HIP_ADD_INT8_LITERAL = 0, LCE_HIP_ADD_INT8_SPLIT = 1, LCE_HIP_ADD_INT8_SHIFT = 2
} lce_hip_add_int8_variant_id;
lce_hip_status lce_hip_add_int8_variant(const lce_hip_add_int8_desc* desc, int32_t* variant);
lce_hip_status lce_hip_add_int8_forced(const lce_hip_add_int8_desc* desc, int32_t variant, const int8_t* in1_dev,
                                       const int8_t* in2_dev, size_t rows, size_t channels, int8_t* out_dev,
                                       int32_t* out_bits_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * int8 elementwise chain between binary layers (constant ADD, PRELU, RELU, requantize) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* The tail of an int8-converted ReActNet block -- LceBconv2d (int8 out), ADD shortcut, ADD per-channel shift, PRELU, ADD
 * per-channel shift, LceQuantize -- a standalone int8 RELU, and the int8 -> int8 QUANTIZE the converter puts in front of a
 * CONCATENATION whose inputs differ in scale.  lce_hip_elementwise_i8 is ONE pass over an NHWC int8 tensor [rows, channels]:
 *
 *   v = in                                             (quantization si, zi)
 *   optional head:  v = ADD(v, addend[rows, channels])  exactly lce_hip_add_int8's arithmetic and prepare, own (s, z) and activation
 *   steps 1..8, each with its own output (so, zo), which is the next step's (si, zi):
 *     ADD    constant operand k (SCALAR, or PER_CHANNEL values[channels]; int8 with its own scale and zero point):
 *            lce_hip_add_int8's arithmetic with x2 = k or k[c]; prepare and refusals as lce_hip_add_int8_prepare
 *     PRELU  alpha int8 SCALAR or PER_CHANNEL with (sa, za);  d = v - zi
 *            d >= 0: MBQM(d, m1, e1) + zo      (m1, e1) = QuantizeMultiplier((double)(float)(si / so))
 *            d <  0: MBQM(d * (alpha - za), m2, e2) + zo      (m2, e2) = QuantizeMultiplier((double)(float)(si * sa / so))
 *            clamped to [-128, 127]; activation must be NONE
 *            (both real multipliers are evaluated in float32, left to right, then widened: TFLite's Prepare divides two floats)
 *     CLAMP  standalone RELU / RELU_N1_TO_1 / RELU6: MBQM(v - zi, m, e) + zo with (m, e) = QuantizeMultiplier((double)(float)(si / so)),
 *            clamped to CalculateActivationRangeQuantized at (so, zo), which lce_hip_add_int8_prepare reports as act_min / act_max
 *     REQUANTIZE  QUANTIZE int8 -> int8: MBQM(v - zi, m, e) + zo with (m, e) = QuantizeMultiplier((double)si / (double)so),
 *            clamped to [-128, 127]
 *
 * MBQM(x, m, e) = RDivPOT(SRDHM(x * 2^max(e,0), m), max(-e,0)); SRDHM, RDivPOT and QuantizeMultiplier as lce_hip_add_int8 states
 * them.  Real multipliers of 1 and above are allowed for PRELU, CLAMP and REQUANTIZE.  This statement is the authority (no
 * TFLite source is consulted); tests/elementwise_i8_ref.py restates it in NumPy int64.  It restates reference_integer_ops::Add
 * (broadcast), reference_ops::BroadcastPrelu4DSlow (int8), optimized_ops::ReluX / QuantizedReluX and reference_ops::Requantize.
 * Against the real-valued result in float64 (clamped the same way) one step alone deviates by at most, measured over 300 seeded
 * parameter draws per kind and all 256 inputs on the CPU: ADD 0.5000 LSB, PRELU 0.7498, CLAMP 0.7495, REQUANTIZE 0.7497 (MBQM
 * rounds twice: a half and a quarter can stack).  tests/test_elementwise_i8_host.py holds 0.51 / 0.75 / 0.75 / 0.75.  (The same
 * measurement for lce_hip_mul_int8 and lce_hip_logistic_int8 below: MUL 0.5039, LOGISTIC 0.5000; tests/test_gate_i8_host.py.)
 *
 * Every step is a function of one int8 value and its channel, so the chain is one 256-entry table per channel:
 *   lce_hip_elementwise_i8_check: the descriptor checks alone (the operand values are not read).  Host only.
 *   lce_hip_elementwise_i8_table_size: the table's bytes, 256 R with R = channels, or R = 1 when no step is PER_CHANNEL.
 *   lce_hip_elementwise_i8_prepare: host only.  Evaluates the steps' literal arithmetic for all 256 inputs of every channel and
 *     writes uint8 table[R][256]: table[c][v + 128] is the chain's int8 result (as a byte) for the value v in channel c.
 *   Refused (LCE_HIP_ERR_INVALID, the message names the step): a scale that is not finite and positive or a zero point outside
 *   [-128, 127]; an ADD real multiplier outside (0, 1) as lce_hip_add_int8_prepare refuses it; a PRELU / CLAMP / REQUANTIZE real
 *   multiplier that is not finite and positive; an activation on PRELU or REQUANTIZE; an unknown op, operand kind or activation;
 *   an operand on CLAMP / REQUANTIZE; non-zero reserved fields; num_steps outside 1..8 (a head with no steps is
 *   lce_hip_add_int8's job); channels negative or 2^22 and above; an intermediate that could leave int32 (x * 2^e); in prepare a
 *   NULL values pointer of an ADD or PRELU.
 *   lce_hip_elementwise_i8: ONE launch.  `table_dev`: prepare's table on the device, 4-byte aligned.  `addend_dev`: the head's
 *     second tensor (NULL without a head).  `out_dev` (nullable) gets the last step's int8 value and may be in_dev or addend_dev
 *     (in place); `out_bits_dev` (nullable) gets its LceQuantize at the LAST step's zero point: bit = out < zo, ceil(channels/32)
 *     words per row, padding bits 0.  The int8 pointers need no alignment.  Zero rows or channels is a no-op.  Asynchronous on
 *     `stream`, capturable in a HIP graph, allocates and copies nothing, 64-bit offsets.  The device computes the head ADD (with
 *     the variant lce_hip_add_int8 has proven for its parameters) and looks the rest up.
 * The table lives in one of three places, each a path:
 *   LDS     : every block copies the table into LDS (260 R bytes of the 160 KiB: channels <= 608 on the 16-byte layout, <= 630
 *             on the row layout).  A kernel's first launch with more than 64 KiB of LDS raises that kernel's limit, a host call:
 *             make it before a capture, as lce_tflite_model_run_section's eager first run does.
 *   GLOBAL  : the table is read from global memory through the cache; any channel count.
 *   ONE_ROW : R = 1, the 256 bytes in LDS; what a chain with R = 1 runs on.  LDS and GLOBAL need R = channels.
 * lce_hip_elementwise_i8_path reports what the launch would be for these operands (host only, nothing runs; the pointers are
 * looked at for their alignment alone and may be NULL where the call allows it); lce_hip_elementwise_i8_forced runs a given
 * path -- for tests and measurements -- and refuses one that cannot hold the table. */
typedef enum lce_hip_ew_i8_op {
  LCE_HIP_EW_I8_ADD = 0, LCE_HIP_EW_I8_PRELU = 1, LCE_HIP_EW_I8_CLAMP = 2, LCE_HIP_EW_I8_REQUANTIZE = 3
} lce_hip_ew_i8_op;
typedef enum lce_hip_elementwise_i8_path_id {
  LCE_HIP_EW_I8_PATH_LDS = 0, LCE_HIP_EW_I8_PATH_GLOBAL = 1, LCE_HIP_EW_I8_PATH_ONE_ROW = 2
} lce_hip_elementwise_i8_path_id;
#define LCE_HIP_EW_I8_MAX_STEPS 8
typedef struct lce_hip_ew_i8_step {
  int32_t op, operand;             /* lce_hip_ew_i8_op; LCE_HIP_EW_SCALAR or LCE_HIP_EW_PER_CHANNEL (0 for CLAMP / REQUANTIZE) */
  const int8_t* values;            /* HOST, read by prepare only: [1] for SCALAR, [channels] for PER_CHANNEL; NULL for CLAMP / REQUANTIZE */
  float operand_scale; int32_t operand_zero_point;   /* of the constant (ADD) or of alpha (PRELU); 0 otherwise */
  float out_scale; int32_t out_zero_point;
  int32_t activation;              /* ADD, CLAMP: an lce_hip_activation; NONE for PRELU and REQUANTIZE */
  int32_t reserved[2];             /* 0 */
} lce_hip_ew_i8_step;
typedef struct lce_hip_elementwise_i8_desc {
  int32_t channels;
  float in_scale; int32_t in_zero_point;
  int32_t has_head;                /* 0 or 1 */
  float addend_scale; int32_t addend_zero_point;     /* the head's second input, its output and its activation (0 without a head) */
  float head_scale; int32_t head_zero_point;
  int32_t head_activation;
  int32_t num_steps;               /* 1..8 */
  lce_hip_ew_i8_step steps[LCE_HIP_EW_I8_MAX_STEPS];
  int32_t reserved[2];             /* 0 */
} lce_hip_elementwise_i8_desc;
typedef struct lce_hip_elementwise_i8_launch {
  int32_t path;                    /* an lce_hip_elementwise_i8_path_id */
  int32_t flat;                    /* 1: the 16-byte layout (4096 elements per wave and iteration), 0: one wave per 64 columns of a row */
  int32_t lds_max_channels;        /* the largest channel count the LDS path takes on this layout */
  int32_t blocks, waves_per_block; /* the launch */
  int32_t lds_bytes;
  int32_t head_variant;            /* the lce_hip_add_int8_variant_id of the head, -1 without one */
  int32_t table_rows;              /* R */
} lce_hip_elementwise_i8_launch;
lce_hip_status lce_hip_elementwise_i8_check(const lce_hip_elementwise_i8_desc* desc);
lce_hip_status lce_hip_elementwise_i8_table_size(const lce_hip_elementwise_i8_desc* desc, size_t* bytes);
lce_hip_status lce_hip_elementwise_i8_prepare(const lce_hip_elementwise_i8_desc* desc, uint8_t* table_host /* [R][256] */);
lce_hip_status lce_hip_elementwise_i8(const lce_hip_elementwise_i8_desc* desc, const int8_t* in_dev, const int8_t* addend_dev /* nullable */,
                                      const uint8_t* table_dev, size_t rows, int8_t* out_dev /* nullable */,
                                      int32_t* out_bits_dev /* nullable */, void* stream);
lce_hip_status lce_hip_elementwise_i8_path(const lce_hip_elementwise_i8_desc* desc, size_t rows, const int8_t* in_dev,
                                           const int8_t* addend_dev, const uint8_t* table_dev, const int8_t* out_dev,
                                           const int32_t* out_bits_dev, int32_t forced_path /* -1: the entry's rule */,
                                           lce_hip_elementwise_i8_launch* launch);
lce_hip_status lce_hip_elementwise_i8_forced(const lce_hip_elementwise_i8_desc* desc, int32_t path, const int8_t* in_dev,
                                             const int8_t* addend_dev, const uint8_t* table_dev, size_t rows, int8_t* out_dev,
                                             int32_t* out_bits_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * int8 squeeze-and-excite gate between binary layers (TFLite builtin LOGISTIC and MUL) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* In an int8-converted RealToBinaryNet a block is  y = LceBconv2d(bits(x));  gate = MEAN(y) -> FULLY_CONNECTED -> FULLY_CONNECTED
 * -> LOGISTIC -> RESHAPE [b,1,1,C];  out = ADD(MUL(y, gate), x).  lce_hip_mul_int8 is TFLite's builtin int8 MUL, per element
 *
 *   (m, e) = QuantizeMultiplier((double)(float)(s1 * s2 / so))      float32, left to right, then widened (as PRELU's above)
 *   out    = clamp(MBQM((x1 - z1) * (x2 - z2), m, e) + zo, act_min, act_max)
 *
 * with MBQM, QuantizeMultiplier and the activation range exactly as lce_hip_elementwise_i8 and lce_hip_add_int8 state them.  This
 * statement is the authority (no TFLite source is consulted); tests/gate_i8_ref.py restates it in NumPy int64 / float32.
 * `in1_dev` is NHWC int8 [rows, channels].  `in2_dev` is, by desc->operand,
 *   LCE_HIP_EW_TENSOR            : [rows, channels]
 *   LCE_HIP_EW_PER_IMAGE_CHANNEL : [rows / rows_per_image, channels], the gate: element (n, c) is read at n * channels + c
 *                                  (lce_hip_elementwise_ex's rule; rows_per_image = H * W, 0 allowed for a TENSOR operand).
 * Optional residual ADD behind the MUL (desc->has_add): the MUL's int8 result, at the MUL's own (so, zo) and clamped, is the first
 * input of lce_hip_add_int8's arithmetic, `addend_dev` [rows, channels] at (addend_scale, addend_zero_point) the second; the ADD has
 * its own output quantization (add_scale, add_zero_point) and add_activation.  The bytes are exactly those of lce_hip_mul_int8
 * without the ADD followed by lce_hip_add_int8; the ADD runs the variant lce_hip_add_int8_variant has proven for its parameters.
 * The MUL stage has two variants of the per-element arithmetic that give the same bytes: LITERAL, the formula as written (right for
 * every parameter set), and FAST (e <= -1: one 64-bit multiply-add and one shift for SRDHM, one add and one shift for RDivPOT).  With
 * the literal one the launch is ALU-bound at twice the bare ADD's time (profiles/gate_i8/layers.txt), so for each parameter set the
 * host runs FAST over ALL 130 051 products (x1 - z1)(x2 - z2) against LITERAL and uses it only if every byte agrees.
 * Outputs as lce_hip_add_int8's: `out_dev` (nullable) may be in1_dev or addend_dev (in place); `out_bits_dev` (nullable) gets
 * bit = value < the LAST stage's zero point (the ADD's with has_add, the MUL's without), ceil(channels/32) words per row, padding
 * bits 0.  int8 pointers may have any alignment; out_bits_dev is 4-byte aligned.  64-bit offsets.  Zero rows or channels is a
 * no-op.  Asynchronous on `stream`, capturable in a HIP graph, allocates and copies nothing.
 * Against the real-valued s1 s2 (x1 - z1)(x2 - z2) / so + zo in float64, clamped the same way, the MUL deviates by at most
 * 0.5039 LSB, measured over 300 seeded parameter draws and all 65 536 input pairs on the CPU (tests/test_gate_i8_host.py holds
 * 0.51; the figure is that of the NumPy restatement tests/gate_i8_ref.py, to which the parameters, the kernel bodies on the CPU
 * and the GPU's bytes are each held equal).  MBQM rounds twice here as well, but where the products of two int8 differences span the int8 range (the draws keep
 * fewer than 10 % of the results at a clamp bound) the real multiplier is a hundredth or less, so the first rounding weighs 2^-7
 * of the second: not the 0.75 of PRELU, CLAMP and REQUANTIZE above.  The LOGISTIC table below, as lce_hip_logistic_int8_prepare
 * writes it: at most 0.5000 LSB from float64's 256 / (1 + exp(-x)) - 128 over 300 draws and all 256 inputs (held at 0.51).
 * Refused, LCE_HIP_ERR_INVALID, before any pointer is touched, the message naming the field: a scale that is not finite and
 * positive or a zero point outside [-128, 127] (in1, in2, out; with has_add also addend, add); an unknown activation or operand
 * kind; has_add other than 0 or 1; a real multiplier that is not finite and positive, or an (x1 - z1)(x2 - z2) * 2^e that could
 * leave int32; the ADD's refusals exactly as lce_hip_add_int8_prepare gives them; a rows_per_image of 0 with a per-image operand,
 * or one that does not divide rows; both outputs NULL; a NULL input; has_add with a NULL addend; non-zero reserved fields.
 *   lce_hip_mul_int8_prepare: host only; the MUL's multiplier, shift and activation range and, with has_add, the ADD's parameters
 *     (zeros without).
 *   lce_hip_mul_int8_path: host only, nothing runs; the launch lce_hip_mul_int8 would make for these operands (the pointers are
 *     looked at for their alignment alone).  flat: the 16-byte layout (channels % 16 == 0 and every pointer 16-byte aligned, 4096
 *     elements per wave and iteration); otherwise one wave per 64 columns of a row. */
typedef struct lce_hip_mul_int8_desc {
  float in1_scale; int32_t in1_zero_point;
  float in2_scale; int32_t in2_zero_point;
  float out_scale; int32_t out_zero_point;           /* of the MUL */
  int32_t activation;                                /* of the MUL: an lce_hip_activation */
  int32_t operand;                                   /* LCE_HIP_EW_TENSOR or LCE_HIP_EW_PER_IMAGE_CHANNEL */
  int32_t has_add;                                   /* 0 or 1 */
  float addend_scale; int32_t addend_zero_point;     /* the ADD's second input, its output and its activation (ignored without) */
  float add_scale; int32_t add_zero_point;
  int32_t add_activation;
  int32_t reserved[2];                               /* 0 */
} lce_hip_mul_int8_desc;
typedef struct lce_hip_mul_int8_params {
  int32_t multiplier, shift, act_min, act_max;
  lce_hip_add_int8_params add;                       /* in1 = the product, in2 = the addend */
} lce_hip_mul_int8_params;
typedef struct lce_hip_mul_int8_launch {
  int32_t flat;                    /* 1: the 16-byte layout, 0: one wave per 64 columns of a row */
  int32_t blocks, waves_per_block; /* the launch */
  int32_t add_variant;             /* the lce_hip_add_int8_variant_id of the ADD, -1 without one */
  int32_t mul_variant;             /* 0: LITERAL, 1: FAST (proven for these parameters) */
  /* With an ADD, what its variant's kernel is given, so that a simulation on the host runs that kernel and no other (zeros
   * without): whether the product is the kernel's first input (the host puts a shift-form input first), and the parameters in
   * that order -- z1, z2, zo, m1, n1, m2, n2, mo, no, lo, hi (n = -shift), then ka, kb, c, ml, mh, nb, half_b, half_o,
   * lo - zo, hi - zo of the SPLIT and SHIFT variants. */
  int32_t product_first;
  int32_t add_args[21];
} lce_hip_mul_int8_launch;
lce_hip_status lce_hip_mul_int8_prepare(const lce_hip_mul_int8_desc* desc, lce_hip_mul_int8_params* params);
lce_hip_status lce_hip_mul_int8(const lce_hip_mul_int8_desc* desc, const int8_t* in1_dev, const int8_t* in2_dev,
                                const int8_t* addend_dev /* NULL without has_add */, size_t rows, size_t channels,
                                size_t rows_per_image, int8_t* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */,
                                void* stream);
lce_hip_status lce_hip_mul_int8_path(const lce_hip_mul_int8_desc* desc, size_t rows, size_t channels, size_t rows_per_image,
                                     const int8_t* in1_dev, const int8_t* in2_dev, const int8_t* addend_dev, const int8_t* out_dev,
                                     const int32_t* out_bits_dev, lce_hip_mul_int8_launch* launch);

/* TFLite's builtin int8 LOGISTIC as a 256-byte table; the launch is the ONE_ROW path of lce_hip_elementwise_i8's kernels.
 *   lce_hip_logistic_int8_prepare: host only.  For v in -128..127, in float32:
 *       x = fl(si * fl(v - zi));  y = LOGISTIC(x) as lce_hip_elementwise_ex states it (E(a) of lce_hip_softmax_f32), evaluated on
 *       the host;  table[v + 128] = clamp(round_half_away(fl(y * 256)) - 128, -128, 127)
 *     The output quantization must be exactly (1/256, -128), as TFLite fixes it; anything else is refused, as are an input scale
 *     that is not finite and positive and an input zero point outside [-128, 127].  `table` NULL: the checks alone.
 *   lce_hip_logistic_int8: [rows, channels] int8 of any rows (the gate's tensor is [b, C]); `table_dev`: the table on the device,
 *     4-byte aligned; `out_dev` (nullable, may be in_dev) and `out_bits_dev` (nullable: bit = out < -128, so every bit is 0) as
 *     above.  channels < 2^22, lce_hip_elementwise_i8's own bound.  Zero rows or channels is a no-op; both outputs NULL, a NULL
 *     `table_dev` and a NULL `in_dev` are refused, each by name.  Asynchronous on `stream`, capturable in a HIP graph, allocates
 *     and copies nothing. */
lce_hip_status lce_hip_logistic_int8_prepare(float in_scale, int32_t in_zero_point, float out_scale, int32_t out_zero_point,
                                             uint8_t* table /* [256], nullable */);
lce_hip_status lce_hip_logistic_int8(const uint8_t* table_dev, const int8_t* in_dev, size_t rows, size_t channels,
                                     int8_t* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------
 * Channel join between binary layers (TFLite builtin CONCATENATION) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* A converted dense binary network (BinaryDenseNet, MeliusNet) joins every binary layer's output to its input with the
 * builtin CONCATENATION on the channel axis.  lce_hip_concat joins `num_inputs` (2..8) NHWC tensors [rows, channels[k]]
 * (rows = N*H*W) of ONE element type -- F32, I8 or BITPACKED (int32 words, channels[k] counted in words) -- along the last
 * axis into [rows, sum channels[k]] in ONE pass.  `out_dev` (nullable) gets exactly the bytes of the inputs side by side:
 * a copy, so float NaN payloads, -0.0 and subnormals come through untouched.  `out_bits_dev` (nullable; F32 and I8 only)
 * gets the LceQuantize of the joined tensor as lce_hip_bitpack(type, out, rows, sum, zero_point, ...) writes it: bit =
 * out < 0 (F32) or out < zero_point (I8), ceil(sum/32) words per row, padding bits 0 -- from the values the copy holds,
 * the inputs are read once.  The same input may appear twice.  `inputs_dev` and `channels` are host arrays read at the call.
 * Refused (LCE_HIP_ERR_INVALID, before any device pointer is dereferenced or a device touched): num_inputs outside 2..8,
 * a channels[k] <= 0 (or a sum of 2^31 or more), a type other than the three, bits for BITPACKED, a zero point outside
 * [-128, 127] for I8 or non-zero otherwise, both outputs NULL, a NULL input, an output range that overlaps an input range or
 * the other output (the row pitches differ: there is no in-place join).  Zero rows is a no-op (checked before the
 * pointers).  rows must be below 2^32; the byte counts are unbounded (64-bit offsets throughout).  Asynchronous on
 * `stream`, capturable in a HIP graph, allocates nothing and copies nothing between host and device (offsets and counts
 * travel as kernel arguments). */
#define LCE_HIP_CONCAT_MAX_INPUTS 8
lce_hip_status lce_hip_concat(lce_hip_dtype type, const void* const* inputs_dev, const int32_t* channels,
                              int32_t num_inputs, size_t rows, int32_t zero_point, void* out_dev /* nullable */,
                              int32_t* out_bits_dev /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------
 * Join of channel windows (TFLite builtin STRIDED_SLICE / SLICE on the channel axis, MeliusNet's improvement block)
 * ---------------------------------------------------------------------------------- */

/* MeliusNet's improvement block adds a binary layer's 64 channels to the LAST 64 channels of its input:
 *   f = x[..., :C-64];  b = x[..., C-64:] + w;  y = CONCATENATION(f, b)
 * lce_hip_join_windows is lce_hip_concat with a source generalised to a channel WINDOW [begin, begin + count) of a wider
 * NHWC tensor [rows, pitch], and an optional dense float tensor [rows, count] added to a window on the way through, so the
 * block is ONE launch that reads x and w once and writes y once; a channel slice alone is the one-window call.  `type` is
 * F32 or I8.  For window k, which begins at start_k = sum of the counts before it:
 *   without an addend  out[r][start_k + c] = src_k[r][begin_k + c] -- a copy: NaN payloads, -0.0 and subnormals come
 *                      through untouched;
 *   with an addend     out[r][start_k + c] = fl(src_k[r][begin_k + c] + addend_k[r][c]) -- ONE float32 add, round to nearest
 *                      even, subnormals not flushed; a NaN result is a NaN whose payload is unspecified.
 * `out_dev` (nullable) is [rows, sum count]; `out_bits_dev` (nullable) gets the LceQuantize of that tensor exactly as
 * lce_hip_concat writes it (bit = v < 0 for F32, v < zero_point for I8, ceil(sum count / 32) words per row, padding bits
 * 0), from the values the pass holds.  The same source may appear in several windows and windows of one source may
 * overlap.  `windows` is a host array read at the call.
 * Refused (LCE_HIP_ERR_INVALID, before any device pointer is dereferenced or a device touched): a type other than F32 / I8
 * (no converted network slices a bit tensor), num_windows outside 1..8, NULL windows or a NULL data_dev, a window outside
 * its pitch (begin < 0, count < 1, begin + count > pitch), a sum of counts of 2^31 or more, an addend with I8, an addend
 * that is not 4-byte aligned, a zero point outside [-128, 127] for I8 or non-zero for F32, non-zero reserved fields, both
 * outputs NULL, an output range that overlaps a source's whole [rows, pitch] range, an addend or the other output.  Zero rows
 * is a no-op, checked first (an empty tensor may come with null pointers).  rows must be below 2^32; byte counts are
 * unbounded (64-bit offsets).  lce_hip_join_windows_check is the host-only part: the checks that need neither rows nor the
 * outputs.  Asynchronous on `stream`, capturable in a HIP graph, allocates nothing and copies nothing between host and
 * device (the window table travels in the kernel arguments). */
typedef struct lce_hip_window {
  const void* data_dev;     /* the source tensor [rows, pitch] */
  int32_t pitch;            /* channels per source row */
  int32_t begin, count;     /* the window [begin, begin + count) of every row: begin >= 0, count >= 1, begin + count <= pitch */
  const float* addend_dev;  /* nullable, F32 only: a dense [rows, count] tensor added to the window */
  int32_t reserved[2];      /* 0 */
} lce_hip_window;
#define LCE_HIP_JOIN_MAX_WINDOWS 8
lce_hip_status lce_hip_join_windows(lce_hip_dtype type, const lce_hip_window* windows, int32_t num_windows /* 1..8 */,
                                    size_t rows, int32_t zero_point, void* out_dev /* nullable */,
                                    int32_t* out_bits_dev /* nullable */, void* stream);
lce_hip_status lce_hip_join_windows_check(lce_hip_dtype type, const lce_hip_window* windows, int32_t num_windows);  /* host only */

/* ------------------------------------------------------------------------------------
 * 2-D pooling between binary layers (TFLite builtin MAX_POOL_2D / AVERAGE_POOL_2D) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* BinaryAlexNet, XNOR-Net and DoReFa-Net pool (3x3, stride 2) behind a float LceBconv2d; a dense network's transition block
 * and the downsampling shortcuts of Bi-RealNet / BinaryResNetE pool 2x2, stride 2.  lce_hip_pool2d is TFLite's builtin
 * MAX_POOL_2D / AVERAGE_POOL_2D (tensorflow/lite/kernels/pooling.cc: reference_ops::MaxPool / AveragePool for float32,
 * reference_integer_ops::MaxPool / AveragePool for int8) over an NHWC tensor [batch, in_height, in_width, channels] in ONE
 * pass.  The output is [batch, out_height, out_width, channels] with the extents of lce_hip_bmaxpool_output_shape and
 * TFLite's padding (ComputePaddingHeightWidth: total = max(0, (out - 1) stride + filter - in), total / 2 of it in front).
 * Taps that fall into the padding are EXCLUDED, not read as zero.  Per output element, over its in-bounds taps in raster
 * order (filter row, then filter column):
 *   float MAX    : m = -FLT_MAX; m = (m < x) ? x : m.  A NaN never replaces m; a window of only NaN / -inf gives -FLT_MAX;
 *                  which of +0.0 / -0.0 a window of both gives is unspecified.
 *   float AVERAGE: t = 0.0f; t += x, one float32 rounding per add, never reassociated; then t / (float)count, the IEEE
 *                  (correctly rounded) division by the number of in-bounds taps.  Subnormals are not flushed.
 *   int8 MAX     : the maximum.
 *   int8 AVERAGE : a = the int32 sum, n = the number of in-bounds taps; q = a > 0 ? (a + n / 2) / n : (a - n / 2) / n with
 *                  C's truncating division.
 *   then v = min(max(v, act_min), act_max): CalculateActivationRange of `activation` for float (NONE: [-FLT_MAX, FLT_MAX],
 *   so an infinity becomes +-FLT_MAX; a NaN passes), CalculateActivationRangeQuantized at (scale, zero_point) for int8 --
 *   the computation lce_hip_add_int8_prepare reports as act_min / act_max.  int8 input and output share ONE scale and zero
 *   point (TFLite's Prepare requires it of both pools).
 * `out_dev` (nullable) gets the pooled tensor; `out_bits_dev` (nullable) gets its LceQuantize as lce_hip_bitpack(type, out,
 * batch * out_height * out_width, channels, zero_point, ...) writes it: bit = v < 0 (F32) or v < zero_point (I8), LSB first,
 * ceil(channels/32) words per pixel, padding bits 0 -- from the values the pass holds, the pooled tensor is not read again.
 * Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc or input, both outputs NULL, an extent, filter or
 * stride <= 0, an unknown op, type, padding or activation, for I8 a zero point outside [-128, 127] or a scale that is not
 * finite and positive, an empty output (VALID with a filter larger than the image), an output that overlaps the input or the
 * other output; LCE_HIP_ERR_UNSUPPORTED: filter_height x filter_width above LCE_HIP_POOL_MAX_TAPS (the bound under which
 * the int8 AVERAGE's division, done in float, is proven exact: |a| + n / 2 <= 128.5 n < 2^24), 2^31 or more output pixels,
 * an image extent or a stride above 2^30 (the window arithmetic is 32-bit).
 * The byte counts are unbounded (64-bit offsets throughout).  Asynchronous on `stream`, capturable in a HIP graph, allocates
 * nothing and copies nothing between host and device.  Bitpacked pooling is lce_hip_bmaxpool. */
#define LCE_HIP_POOL_MAX_TAPS 65536
typedef enum lce_hip_pool_op { LCE_HIP_POOL_MAX = 0, LCE_HIP_POOL_AVERAGE = 1 } lce_hip_pool_op;
typedef struct lce_hip_pool2d_desc {
  int32_t op, type;                 /* lce_hip_pool_op; LCE_HIP_F32 | LCE_HIP_I8 */
  int32_t batch, in_height, in_width, channels;
  int32_t filter_height, filter_width, stride_height, stride_width;
  int32_t padding, activation;      /* lce_hip_padding; NONE | RELU | RELU_N1_TO_1 | RELU6 */
  float scale; int32_t zero_point;  /* int8: shared by input and output */
} lce_hip_pool2d_desc;
lce_hip_status lce_hip_pool2d(const lce_hip_pool2d_desc* desc, const void* in_dev, void* out_dev /* nullable */,
                              int32_t* out_bits_dev /* nullable */, void* stream);
/* The descriptor checks of lce_hip_pool2d alone, and the output extents (nullable).  Host only: needs no device. */
lce_hip_status lce_hip_pool2d_check(const lce_hip_pool2d_desc* desc, int32_t* out_height, int32_t* out_width);

/* ------------------------------------------------------------------------------------
 * The float 1x1 CONV_2D between binary layers (TFLite builtin CONV_2D) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* The downsampling shortcuts of Bi-RealNet / BinaryResNetE and the transition blocks of BinaryDenseNet / MeliusNet run a float
 * 1x1 convolution behind their 2x2 pool.  lce_hip_conv1x1_f32 is that convolution over an NHWC float32 tensor [batch,
 * in_height, in_width, channels_in] with the filter in the file's own layout [channels_out][channels_in] ([Cout, 1, 1, Cin])
 * and an optional bias [channels_out], in ONE pass.  The output is [batch, out_height, out_width, channels_out] with
 * out = (in + stride - 1) / stride: a 1x1 filter has no padding taps, so SAME and VALID agree, and a stride only selects the
 * input pixel (b, oy * stride_height, ox * stride_width).
 * Float CONV_2D has no single "TFLite bytes" (reference_ops::Conv's `total += in * w` is a multiply and an add on baseline
 * x86-64 and an FMA on AArch64; XNNPACK and Eigen block and reorder), so the library states its own: reference_ops::Conv
 * (float) as a CONTRACTING build computes it.  Per output element, over input channels c = 0 .. channels_in - 1 in order:
 *   t = +0.0f;  t = fmaf(x[c], w[o][c], t)     one rounding per step, never reassociated, never split over K
 *   t = t + bias[o]                            one float32 add; skipped when bias_dev is NULL
 *   v = min(max(t, act_min), act_max)          the clamp of lce_hip_pool2d (NONE: [-FLT_MAX, FLT_MAX]; a NaN passes)
 * Subnormals are not flushed, going in or coming out; NaN and infinity flow through the chain.  The kernel runs the chain on
 * the f32-input matrix instruction, whose result is such a chain bit for bit.
 * `out_dev` (nullable) gets the result; `out_bits_dev` (nullable) gets its LceQuantize as lce_hip_bitpack(F32, out, ...)
 * writes it: bit = v < 0, LSB first, ceil(channels_out/32) words per pixel, padding bits 0 -- from the values the pass holds.
 * Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc, input or filter, both outputs NULL, an extent, channel
 * count or stride <= 0, an unknown activation, an output that overlaps the input, the filter, the bias or the other output, a
 * pointer that is not 4-byte aligned; LCE_HIP_ERR_UNSUPPORTED: 2^31 or more output pixels, an image extent or a stride above
 * 2^30, more than 65535 x 128 output channels.
 * Pointers need 4-byte alignment only (16-byte aligned input and filter with channels_in % 4 == 0 take a faster load path);
 * the byte counts are unbounded (64-bit offsets throughout).  Asynchronous on `stream`, capturable in a HIP graph, allocates
 * nothing and copies nothing between host and device. */
typedef struct lce_hip_conv1x1_desc {
  int32_t batch, in_height, in_width, channels_in, channels_out;
  int32_t stride_height, stride_width, activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
} lce_hip_conv1x1_desc;
lce_hip_status lce_hip_conv1x1_f32(const lce_hip_conv1x1_desc* desc, const float* in_dev, const float* filter_dev /* [Cout][Cin] */,
                                   const float* bias_dev /* nullable */, float* out_dev /* nullable */,
                                   int32_t* out_bits_dev /* nullable */, void* stream);
/* The descriptor checks of lce_hip_conv1x1_f32 alone, and the output extents (nullable).  Host only: needs no device. */
lce_hip_status lce_hip_conv1x1_f32_check(const lce_hip_conv1x1_desc* desc, int32_t* out_height, int32_t* out_width);

/* ------------------------------------------------------------------------------------
 * The float DEPTHWISE_CONV_2D between binary layers (TFLite builtin DEPTHWISE_CONV_2D) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* QuickNet's transition block blurs its pooled map with a fixed 3x3 / 2 depthwise filter ([1 2 1] x [1 2 1] / 16) in front of
 * its 1x1 convolution.  lce_hip_depthwise_conv2d_f32 is TFLite's float reference_ops::DepthwiseConv over an NHWC float32
 * tensor [batch, in_height, in_width, channels_in] with the filter in the file's own layout [1, filter_height, filter_width,
 * Cout], Cout = channels_in x depth_multiplier, and an optional bias [Cout], in ONE pass.  Output channel o reads input
 * channel o / depth_multiplier.  The output is [batch, out_height, out_width, Cout]; its extents and the padding are exactly
 * lce_hip_pool2d's (lce_hip_bmaxpool_output_shape; pad_before = total / 2).  The dilation is 1.
 * As for lce_hip_conv1x1_f32 the library states its own bytes: the reference as a CONTRACTING build computes it.  Per output
 * element, over its in-bounds taps in raster order (filter row, then filter column) -- taps in the padding are SKIPPED, not
 * read as zero, and the filter tap index is the unclipped one:
 *   t = +0.0f;  t = fmaf(x[y][x][o / m], w[fy][fx][o], t)   one rounding per tap, never reassociated
 *   t = t + bias[o]                                         one float32 add; skipped when bias_dev is NULL
 *   v = min(max(t, act_min), act_max)                       the clamp of lce_hip_pool2d (NONE: [-FLT_MAX, FLT_MAX]; a NaN passes)
 * Subnormals are not flushed, going in or coming out; NaN and infinity flow through the chain.
 * `out_dev` (nullable) gets the result; `out_bits_dev` (nullable) gets its LceQuantize as lce_hip_bitpack(F32, out, ...)
 * writes it: bit = v < 0, LSB first, ceil(Cout/32) words per pixel, padding bits 0 -- from the values the pass holds.
 * Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc, input or filter, both outputs NULL, an extent, channel
 * count, multiplier, filter or stride <= 0, an unknown padding or activation, an empty output, an output that overlaps the
 * input, the filter, the bias or the other output, a pointer that is not 4-byte aligned; LCE_HIP_ERR_UNSUPPORTED: 2^31 or more
 * output pixels, an image extent or a stride above 2^30, filter_height x filter_width x Cout >= 2^31.
 * Pointers need 4-byte alignment only (depth_multiplier 1 with channels % 4 == 0 and 16-byte aligned input, filter, bias and
 * output takes a 16-byte path; with bits it also needs channels % 32 == 0); the byte counts are unbounded (64-bit offsets).
 * Asynchronous on `stream`, capturable in a HIP graph, allocates nothing and copies nothing between host and device. */
typedef struct lce_hip_depthwise_desc {
  int32_t batch, in_height, in_width, channels_in, depth_multiplier;
  int32_t filter_height, filter_width, stride_height, stride_width;
  int32_t padding;      /* lce_hip_padding: SAME or VALID */
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
} lce_hip_depthwise_desc;
lce_hip_status lce_hip_depthwise_conv2d_f32(const lce_hip_depthwise_desc* desc, const float* in_dev,
                                            const float* filter_dev /* [1][fh][fw][Cout] */, const float* bias_dev /* nullable */,
                                            float* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);
/* The descriptor checks of lce_hip_depthwise_conv2d_f32 alone, and the output extents (nullable).  Host only: needs no device. */
lce_hip_status lce_hip_depthwise_conv2d_f32_check(const lce_hip_depthwise_desc* desc, int32_t* out_height, int32_t* out_width);

/* ------------------------------------------------------------------------------------
 * The float CONV_2D of any filter extent (TFLite builtin CONV_2D: a network's stem) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* Every converted network opens with a float convolution: QuickNet 3x3 / 2, Bi-RealNet / BinaryResNetE / BinaryDenseNet
 * 7x7 / 2, BinaryAlexNet 11x11 / 4.  lce_hip_conv2d_f32 is TFLite's float reference_ops::Conv over an NHWC float32 tensor
 * [batch, in_height, in_width, channels_in] with the filter in the file's own layout [channels_out][filter_height]
 * [filter_width][channels_in] and an optional bias [channels_out], in ONE call.  groups is 1 and the dilation is 1.  The
 * output is [batch, out_height, out_width, channels_out]; its extents and the padding are exactly lce_hip_pool2d's and
 * lce_hip_depthwise_conv2d_f32's (lce_hip_bmaxpool_output_shape; pad_before = total / 2).
 * As for lce_hip_conv1x1_f32 the library states its own bytes: the reference as a CONTRACTING build computes it.  Per output
 * element, over its in-bounds taps in raster order (filter row, then filter column) and within a tap over
 * c = 0 .. channels_in - 1 in order -- taps in the padding are SKIPPED, not read as zero, and the filter index is the
 * unclipped one:
 *   t = +0.0f;  t = fmaf(x[iy][ix][c], w[o][fy][fx][c], t)   one rounding per step, never reassociated, never split over K
 *   t = t + bias[o]                                          one float32 add; skipped when bias_dev is NULL
 *   v = min(max(t, act_min), act_max)                        the clamp of lce_hip_pool2d (NONE: [-FLT_MAX, FLT_MAX]; a NaN passes)
 * Subnormals are not flushed, going in or coming out; NaN and infinity flow through the chain.  For a 1x1 filter the bytes are
 * those of lce_hip_conv1x1_f32.  Output pixels whose window lies inside the image run the chain on the f32-input matrix
 * instruction, whose result is such a chain bit for bit; pixels with a clipped window run it as fmaf, tap by tap.
 * `out_dev` (nullable) gets the result; `out_bits_dev` (nullable) gets its LceQuantize as lce_hip_bitpack(F32, out, ...)
 * writes it: bit = v < 0, LSB first, ceil(channels_out/32) words per pixel, padding bits 0 -- from the values the pass holds.
 * Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc, input or filter, both outputs NULL, an extent, channel
 * count, filter or stride <= 0, an unknown padding or activation, an empty output, an output that overlaps the input, the
 * filter, the bias or the other output, a pointer that is not 4-byte aligned; LCE_HIP_ERR_UNSUPPORTED: 2^31 or more output
 * pixels, an image extent or a stride above 2^30, filter_height x filter_width x channels_in >= 2^31, more than 65535 x 128
 * output channels.
 * Pointers need 4-byte alignment only (16-byte aligned input and filter with channels_in % 4 == 0 take a faster load path);
 * the byte counts are unbounded (64-bit offsets throughout).  Asynchronous on `stream` (up to two launches), capturable in a
 * HIP graph, allocates nothing and copies nothing between host and device. */
typedef struct lce_hip_conv2d_desc {
  int32_t batch, in_height, in_width, channels_in, channels_out;
  int32_t filter_height, filter_width, stride_height, stride_width;
  int32_t padding;      /* lce_hip_padding: SAME or VALID */
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
} lce_hip_conv2d_desc;
lce_hip_status lce_hip_conv2d_f32(const lce_hip_conv2d_desc* desc, const float* in_dev, const float* filter_dev /* [Cout][fh][fw][Cin] */,
                                  const float* bias_dev /* nullable */, float* out_dev /* nullable */,
                                  int32_t* out_bits_dev /* nullable */, void* stream);
/* The descriptor checks of lce_hip_conv2d_f32 alone, and the output extents (nullable).  Host only: needs no device. */
lce_hip_status lce_hip_conv2d_f32_check(const lce_hip_conv2d_desc* desc, int32_t* out_height, int32_t* out_width);

/* ------------------------------------------------------------------------------------
 * The int8 CONV_2D of any filter extent (TFLite builtin CONV_2D, quantized) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* An int8-converted network (inference_input_type int8) keeps three kinds of builtin CONV_2D, all quantized: the stem
 * (3x3 / 2 or 7x7 / 2 on three channels), the 1x1 behind the 2x2 pool of a downsampling shortcut and the 1x1 of a dense
 * network's transition.  lce_hip_conv2d_i8 is TFLite's reference_integer_ops::ConvPerChannel in its default (double-rounding)
 * build, byte for byte.  Input: NHWC int8 [batch, in_height, in_width, channels_in] with quantization (input_scale,
 * input_zero_point) = (si, zi).  Filter: int8 in the file's own layout [channels_out][filter_height][filter_width][channels_in]
 * with zero point 0 and scales sw[o], one per output channel or a single one that stands for all.  Bias: optional int32
 * [channels_out].  Output: NHWC int8 with (output_scale, output_zero_point) = (so, zo).  groups is 1 and the dilation is 1;
 * extents and padding are lce_hip_conv2d_f32's.  Per output element:
 *   acc = sum over in-bounds taps (fy, fx) and c of (x[iy][ix][c] - zi) * w[o][fy][fx][c]   exact, int32; taps in the padding are skipped
 *   acc += bias[o]                                                                          when there is a bias
 *   (m[o], e[o]) = QuantizeMultiplier((double)si * (double)sw[o] / (double)so)
 *   acc = RoundingDivideByPOT(SaturatingRoundingDoublingHighMul(acc * 2^max(e,0), m), max(-e,0))   as lce_hip_add_int8 states the two
 *   v   = min(max(acc + zo, act_min), act_max)      CalculateActivationRangeQuantized at (so, zo): what lce_hip_add_int8_prepare reports
 *   bit = v < zo                                    as lce_hip_pool2d's int8 bits: LSB first, ceil(channels_out/32) words per pixel, padding bits 0
 * Integer arithmetic has one answer: the sum runs on the int8 matrix instruction in whatever order, a tap in the padding is
 * read as x = zi and the constant c[o] = bias[o] - zi * sum_k w[o][k] of the table makes that the reference's skip.
 *
 * lce_hip_conv2d_i8_check: the descriptor checks alone and the output extents (nullable).  Host only.
 * lce_hip_conv2d_i8_prepare: host only.  From the constants of the file -- the filter, the bias (nullable), `n_scales` (1 or
 *   channels_out) filter scales -- the table int32 [3][channels_out] = c[o], m[o], e[o], which the caller uploads once, and the
 *   activation range.  LCE_HIP_ERR_UNSUPPORTED, with a message that names the channel: with K = filter_height x filter_width x
 *   channels_in and B = max |bias|, 255 x 128 x K + B > 2^31 - 1 (the reference's own accumulator could overflow); for a channel
 *   with e > 0, that bound times 2^e > 2^31 - 1; a c[o] that does not fit int32 (the first bound implies it fits).
 *   LCE_HIP_ERR_INVALID: a NULL pointer (the bias excepted), a scale that is not finite and positive, a zero point outside
 *   [-128, 127], n_scales neither 1 nor channels_out, and what lce_hip_conv2d_f32 refuses of a descriptor.
 * lce_hip_conv2d_i8: ONE launch.  `table_dev`: prepare's table on the device.  `out_dev` (nullable) gets the int8 result,
 *   `out_bits_dev` (nullable) its LceQuantize at zo.  Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc, input,
 *   filter or table, both outputs NULL, what the check refuses, an output that overlaps the input, the filter, the table or the
 *   other output, an out_bits_dev or table_dev that is not 4-byte aligned; LCE_HIP_ERR_UNSUPPORTED: lce_hip_conv2d_f32's limits,
 *   and K > 65793 (255 x 128 x K > 2^31 - 1: no table exists for it).
 *   The int8 pointers need no alignment (16-byte aligned input and filter with channels_in % 16 == 0 take a faster load path);
 *   the byte counts are unbounded (64-bit offsets throughout).  Asynchronous on `stream`, capturable in a HIP graph, allocates
 *   nothing and copies nothing between host and device. */
typedef struct lce_hip_conv2d_i8_desc {
  int32_t batch, in_height, in_width, channels_in, channels_out;
  int32_t filter_height, filter_width, stride_height, stride_width;
  int32_t padding;      /* lce_hip_padding: SAME or VALID */
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
  float input_scale;
  int32_t input_zero_point;
  float output_scale;
  int32_t output_zero_point;
} lce_hip_conv2d_i8_desc;
lce_hip_status lce_hip_conv2d_i8_check(const lce_hip_conv2d_i8_desc* desc, int32_t* out_height, int32_t* out_width);
lce_hip_status lce_hip_conv2d_i8_prepare(const lce_hip_conv2d_i8_desc* desc, const int8_t* filter_host /* [Cout][fh][fw][Cin] */,
                                         const int32_t* bias_host /* nullable */, const float* filter_scales, int32_t n_scales /* 1 or Cout */,
                                         int32_t* table /* [3][Cout] */, int32_t* act_min, int32_t* act_max);
lce_hip_status lce_hip_conv2d_i8(const lce_hip_conv2d_i8_desc* desc, const int8_t* in_dev, const int8_t* filter_dev /* [Cout][fh][fw][Cin] */,
                                 const int32_t* table_dev /* [3][Cout] */, int8_t* out_dev /* nullable */,
                                 int32_t* out_bits_dev /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------
 * The int8 DEPTHWISE_CONV_2D (TFLite builtin DEPTHWISE_CONV_2D, quantized) and the LceQuantize that follows
 * ---------------------------------------------------------------------------------- */

/* An int8-converted QuickNet keeps two quantized depthwise convolutions: the fixed 3x3 / 2 blur ([1 2 1] x [1 2 1] / 16) of every
 * transition block and a depthwise 3x3 / 2 in the stem.  lce_hip_depthwise_conv2d_i8 is TFLite's
 * reference_integer_ops::DepthwiseConvPerChannel in its default (double-rounding) build, byte for byte.  The geometry is exactly
 * lce_hip_depthwise_conv2d_f32's.  Input: NHWC int8 [batch, in_height, in_width, channels_in] with quantization (input_scale,
 * input_zero_point) = (si, zi).  Filter: int8 in the file's own layout [1, filter_height, filter_width, Cout], Cout =
 * channels_in x depth_multiplier (= m), with zero point 0 and scales sw[o], one per output channel or a single one that stands
 * for all.  Output channel o reads input channel o / m.  Bias: optional int32 [Cout].  Output: NHWC int8 [batch, out_height,
 * out_width, Cout] with (output_scale, output_zero_point) = (so, zo); extents and padding are lce_hip_pool2d's (SAME or VALID,
 * pad_before = total / 2).  The dilation is 1.  Per output element:
 *   acc = sum over IN-BOUNDS taps (fy, fx) of (x[iy][ix][o / m] - zi) * w[fy][fx][o]       exact, int32; taps in the padding are SKIPPED
 *                                                                                          (not read as 0), the filter index is the unclipped one
 *   acc += bias[o]                                                                         when there is a bias
 *   (m[o], e[o]) = QuantizeMultiplier((double)si * (double)sw[o] / (double)so)
 *   acc = RoundingDivideByPOT(SaturatingRoundingDoublingHighMul(acc * 2^max(e,0), m), max(-e,0))   as lce_hip_add_int8 states the two
 *   v   = min(max(acc + zo, act_min), act_max)      CalculateActivationRangeQuantized at (so, zo): what lce_hip_add_int8_prepare reports
 *   bit = v < zo                                    as lce_hip_pool2d's int8 bits: LSB first, ceil(Cout/32) words per pixel, padding bits 0
 * QuantizeMultiplier, the bounds below and the activation range are the routines lce_hip_conv2d_i8_prepare uses.
 *
 * lce_hip_depthwise_conv2d_i8_check: the descriptor checks alone and the output extents (nullable).  Host only.  It refuses
 *   what lce_hip_depthwise_conv2d_f32_check refuses of the geometry (with this entry's name in the message), a scale that is not
 *   finite and positive and a zero point outside [-128, 127] (LCE_HIP_ERR_INVALID).
 * lce_hip_depthwise_conv2d_i8_prepare: host only.  From the constants of the file -- the filter (read for nothing but its
 *   presence: the kernel subtracts zi itself), the bias (nullable), `n_scales` (1 or Cout) filter scales -- the table int32
 *   [3][Cout] = bias[o] (0 without a bias), m[o], e[o], which the caller uploads once, and the activation range.
 *   LCE_HIP_ERR_UNSUPPORTED, with a message that names the channel: with K = filter_height x filter_width and B = max |bias|,
 *   255 x 128 x K + B > 2^31 - 1 (the reference's own accumulator could overflow); for a channel with e > 0, that bound times
 *   2^e > 2^31 - 1.  LCE_HIP_ERR_INVALID: a NULL pointer (the bias excepted), a filter scale that is not finite and positive,
 *   n_scales neither 1 nor Cout, and what the check refuses.
 * lce_hip_depthwise_conv2d_i8: ONE launch.  `table_dev`: prepare's table on the device.  `out_dev` (nullable) gets the int8
 *   result, `out_bits_dev` (nullable) its LceQuantize at zo.  Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc,
 *   input, filter or table, both outputs NULL, what the check refuses, an output that overlaps the input, the filter, the table
 *   or the other output, an out_bits_dev or table_dev that is not 4-byte aligned.  The int8 pointers need no alignment
 *   (depth_multiplier 1 with Cout % 16 == 0 and 16-byte aligned input, filter, table and output takes a 16-byte path; with bits
 *   it also needs Cout % 32 == 0); the byte counts are unbounded (64-bit offsets beyond the window arithmetic).  Asynchronous on
 *   `stream`, capturable in a HIP graph, allocates nothing and copies nothing between host and device.
 * lce_hip_depthwise_conv2d_i8_path reports the path that launch takes for these operands (1: the 16-byte path, 0: the row path;
 *   host only, nothing runs).  lce_hip_depthwise_conv2d_i8_forced runs a given path -- for tests and measurements; the row path
 *   serves every operand, the 16-byte path is refused where the operands do not qualify.  Both give the same bytes. */
typedef struct lce_hip_depthwise_i8_desc {
  int32_t batch, in_height, in_width, channels_in, depth_multiplier;
  int32_t filter_height, filter_width, stride_height, stride_width;
  int32_t padding;      /* lce_hip_padding: SAME or VALID */
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
  float input_scale;
  int32_t input_zero_point;
  float output_scale;
  int32_t output_zero_point;
} lce_hip_depthwise_i8_desc;
lce_hip_status lce_hip_depthwise_conv2d_i8_check(const lce_hip_depthwise_i8_desc* desc, int32_t* out_height, int32_t* out_width);
lce_hip_status lce_hip_depthwise_conv2d_i8_prepare(const lce_hip_depthwise_i8_desc* desc, const int8_t* filter_host /* [1][fh][fw][Cout] */,
                                                   const int32_t* bias_host /* nullable */, const float* filter_scales,
                                                   int32_t n_scales /* 1 or Cout */, int32_t* table /* [3][Cout] */, int32_t* act_min,
                                                   int32_t* act_max);
lce_hip_status lce_hip_depthwise_conv2d_i8(const lce_hip_depthwise_i8_desc* desc, const int8_t* in_dev,
                                           const int8_t* filter_dev /* [1][fh][fw][Cout] */, const int32_t* table_dev /* [3][Cout] */,
                                           int8_t* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);
lce_hip_status lce_hip_depthwise_conv2d_i8_path(const lce_hip_depthwise_i8_desc* desc, const int8_t* in_dev, const int8_t* filter_dev,
                                                const int32_t* table_dev, const int8_t* out_dev /* nullable */,
                                                const int32_t* out_bits_dev /* nullable */, int32_t* path);
lce_hip_status lce_hip_depthwise_conv2d_i8_forced(const lce_hip_depthwise_i8_desc* desc, int32_t path /* 0: rows, 1: 16-byte */,
                                                  const int8_t* in_dev, const int8_t* filter_dev, const int32_t* table_dev,
                                                  int8_t* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------
 * A transition's MAX_POOL_2D and the DEPTHWISE_CONV_2D that reads it, in one launch (float32 and int8)
 * ---------------------------------------------------------------------------------- */

/* QuickNet's transition pools 2x2 / 1 SAME and blurs the pooled map, which is as large as the pool's input, with the fixed
 * 3x3 / 2 depthwise filter.  lce_hip_pool_depthwise_f32 / _i8 run lce_hip_pool2d (`pool`, op MAX) and lce_hip_depthwise_conv2d_f32
 * / _i8 (`dw`, whose input is the pool's output) as ONE launch that never writes the pooled tensor.  The contract is the
 * composition of the two entries' contracts.  Per output element, over the depthwise filter's in-bounds taps in raster order:
 *   - the filter index is the unclipped one;
 *   - a tap whose POOLED pixel lies outside the pooled map is skipped, as lce_hip_depthwise_conv2d_* skips it;
 *   - the tap's operand is the pooled value lce_hip_pool2d would have stored there:
 *       float : m = -FLT_MAX; m = (m < x) ? x : m over the pool window's in-bounds taps in raster order (a NaN never replaces
 *               m; of +0.0 and -0.0 the first in raster order stays), then the clamp to the pool's activation range;
 *       int8  : the maximum, clamped to the pool's CalculateActivationRangeQuantized at its (scale, zero_point);
 *   - everything behind the pooled value is the depthwise entry's arithmetic, unchanged: float t = fmaf(p, w, t) from +0.0, one
 *     float32 add of the bias, the clamp, bit = v < 0; int8 the exact int32 sum of (p - zi) w, lce_hip_depthwise_conv2d_i8_prepare's
 *     table [3][Cout] used as it is, the requantization, + zo, the clamp, bit = v < zo.
 * So `out_dev` and `out_bits_dev` (each nullable, not both) get, byte for byte, what lce_hip_pool2d followed by
 * lce_hip_depthwise_conv2d_f32 / _i8 writes.
 * lce_hip_pool_depthwise_*_check: host only, and the output extents (nullable).  LCE_HIP_ERR_INVALID: a NULL desc, what
 *   lce_hip_pool2d_check or the depthwise entry's check refuses, a pool `type` that is not the entry's, a `dw` input (batch, extents,
 *   channels) that is not the pool's output, for int8 a `dw` input (scale, zero point) that differs from the pool's.
 *   LCE_HIP_ERR_UNSUPPORTED: what those checks report as unsupported (the 2^31 / 2^30 bounds), and pool `op` AVERAGE.
 * The run entries refuse, before any device call and with LCE_HIP_ERR_INVALID, also a NULL input, filter or table, both outputs
 *   NULL, an output that overlaps the input, the filter, the bias / table or the other output, and the misalignments the
 *   depthwise entry refuses.  ONE launch, asynchronous on `stream`, capturable in a HIP graph; allocates nothing and copies
 *   nothing; offsets are 64-bit beyond the window arithmetic.
 * Two paths with the same bytes (lce_hip_pool_depthwise_*_path reports the one a launch takes, host only; *_forced runs a given
 *   one, for tests and measurements): 0, the row path, takes every geometry; 1, the 16-byte path, needs depth_multiplier 1,
 *   channels % 4 == 0 (float) or % 16 == 0 (int8), 16-byte aligned input, filter, bias / table and output, channels % 32 == 0 with
 *   bits, a pool of stride 1 x 1 and a filter of at most 2 x 2, and a depthwise filter of at most 3 x 3; it loads every input tap
 *   of an output's (at most 4 x 4) footprint once. */
lce_hip_status lce_hip_pool_depthwise_f32_check(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, int32_t* out_height,
                                                int32_t* out_width);
lce_hip_status lce_hip_pool_depthwise_f32(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, const float* in_dev,
                                          const float* filter_dev /* [1][fh][fw][Cout] */, const float* bias_dev /* nullable */,
                                          float* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);
lce_hip_status lce_hip_pool_depthwise_f32_path(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw, const float* in_dev,
                                               const float* filter_dev, const float* bias_dev /* nullable */,
                                               const float* out_dev /* nullable */, const int32_t* out_bits_dev /* nullable */, int32_t* path);
lce_hip_status lce_hip_pool_depthwise_f32_forced(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_desc* dw,
                                                 int32_t path /* 0: rows, 1: 16-byte */, const float* in_dev, const float* filter_dev,
                                                 const float* bias_dev /* nullable */, float* out_dev /* nullable */,
                                                 int32_t* out_bits_dev /* nullable */, void* stream);
lce_hip_status lce_hip_pool_depthwise_i8_check(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, int32_t* out_height,
                                               int32_t* out_width);
lce_hip_status lce_hip_pool_depthwise_i8(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, const int8_t* in_dev,
                                         const int8_t* filter_dev /* [1][fh][fw][Cout] */, const int32_t* table_dev /* [3][Cout] */,
                                         int8_t* out_dev /* nullable */, int32_t* out_bits_dev /* nullable */, void* stream);
lce_hip_status lce_hip_pool_depthwise_i8_path(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw, const int8_t* in_dev,
                                              const int8_t* filter_dev, const int32_t* table_dev, const int8_t* out_dev /* nullable */,
                                              const int32_t* out_bits_dev /* nullable */, int32_t* path);
lce_hip_status lce_hip_pool_depthwise_i8_forced(const lce_hip_pool2d_desc* pool, const lce_hip_depthwise_i8_desc* dw,
                                                int32_t path /* 0: rows, 1: 16-byte */, const int8_t* in_dev, const int8_t* filter_dev,
                                                const int32_t* table_dev, int8_t* out_dev /* nullable */,
                                                int32_t* out_bits_dev /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------
 * The float classifier head (TFLite builtin MEAN, FULLY_CONNECTED, SOFTMAX)
 * ---------------------------------------------------------------------------------- */

/* Every converted network ends in GlobalAveragePooling -> Dense -> softmax.  The MEAN over height and width is an AVERAGE pool
 * whose filter is the image (lce_hip_pool2d: the sequential float sum in raster order, then the IEEE division by the count,
 * which is reference_ops::Mean's arithmetic).  The other two:
 *
 * lce_hip_fully_connected_f32: out[batch][outputs] from in[batch][inputs], the weights in the file's layout
 * [outputs][inputs] and an optional bias [outputs], in ONE launch.  The arithmetic is exactly lce_hip_conv1x1_f32's chain
 * -- t = +0.0f; t = fmaf(x[k], w[o][k], t) over k = 0 .. inputs - 1 in order, never split over k; one float32 add of the bias
 * (skipped when bias_dev is NULL); the std::max / std::min clamp (a NaN passes) -- so the bytes are those of
 * lce_hip_conv1x1_f32 on a [batch, 1, 1, inputs] image.  The kernel is tiled for few rows and many columns (one wave per
 * 16 x 16 tile: lce_kernels_head.h).
 * Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc, input, weights or output, an extent <= 0, an unknown
 * activation, an output that overlaps the input, the weights or the bias, a pointer that is not 4-byte aligned;
 * LCE_HIP_ERR_UNSUPPORTED: 2^31 or more tiles of 16 x 16 outputs.  Pointers need 4-byte alignment only (16-byte aligned input
 * and weights with inputs % 4 == 0 take a faster load path); offsets are 64-bit.  Asynchronous on `stream`, capturable in a HIP
 * graph, allocates nothing and copies nothing between host and device. */
typedef struct lce_hip_fc_desc {
  int32_t batch, inputs, outputs;
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
} lce_hip_fc_desc;
lce_hip_status lce_hip_fully_connected_f32(const lce_hip_fc_desc* desc, const float* in_dev, const float* weights_dev /* [outputs][inputs] */,
                                           const float* bias_dev /* nullable */, float* out_dev, void* stream);
/* The descriptor checks of lce_hip_fully_connected_f32 alone.  Host only: needs no device. */
lce_hip_status lce_hip_fully_connected_f32_check(const lce_hip_fc_desc* desc);

/* lce_hip_softmax_f32: the softmax over the last axis of in[rows][cols], one launch.  No two libraries agree on the bytes of a
 * float softmax (their exp differ), so the library states its own, every step a float32 add, multiply, fmaf, round-to-integer or
 * exponent insertion that NumPy can restate (tests/head_ref.py does):
 *   m     = max over the row (inputs finite; +0 and -0 compare equal and either gives the same bytes)
 *   a_i   = (x_i - m) * beta                   two IEEE operations, no contraction
 *   e_i   = E(a_i), where E(a) is
 *             +0.0f unless a >= -104 (a < -104, -inf, NaN; exp(-104) is below half the smallest subnormal);  a > 0 counts as 0;
 *             n = rint(a * 1.44269502f), to nearest even;
 *             r = fmaf(n, -0.693145751953125f, a);  r = fmaf(n, -1.42860676e-06f, r);
 *             p = 1.98412701e-04f;  p = fmaf(p, r, c) for c = 1.38888892e-03f, 8.33333377e-03f, 4.16666679e-02f, 1.66666672e-01f,
 *             0.5f, 1.0f, 1.0f in this order (the Taylor polynomial of exp to r^7);
 *             n >= -125: p with n added to its exponent field (a normal number);
 *             n <  -125: p with n + 64 added to its exponent field, times 2^-64 in ONE float32 multiply (it rounds into the
 *             subnormals: nothing is flushed).
 *           E is within 1 ulp of exp on [-104, 0] (measured: DESIGN.md).
 *   s     = the sum of the row in a FIXED order: 64 partial sums, partial sum l adding e_l, e_{l+64}, e_{l+128}, ... in this
 *           order from +0.0f; then s_l = s_l + s_{l ^ d} for d = 32, 16, 8, 4, 2, 1 (every s_l ends as the same number)
 *   out_i = e_i / s                            the correctly rounded float32 division
 * A row that holds a NaN or an infinity does not fault; its bytes are unspecified.  in_dev == out_dev (in place) is allowed.
 * Refused before any device call, LCE_HIP_ERR_INVALID: a NULL pointer, rows or cols of 0, a beta that is not finite and > 0, a
 * pointer that is not 4-byte aligned, an output that overlaps the input without being it; LCE_HIP_ERR_UNSUPPORTED: cols >= 2^31
 * or more than 2^60 elements.  Asynchronous on `stream`, capturable in a HIP graph, allocates nothing. */
lce_hip_status lce_hip_softmax_f32(size_t rows, size_t cols, float beta, const float* in_dev, float* out_dev, void* stream);
/* The argument checks of lce_hip_softmax_f32 that need no pointer.  Host only: needs no device. */
lce_hip_status lce_hip_softmax_f32_check(size_t rows, size_t cols, float beta);

/* ------------------------------------------------------------------------------------
 * The binarized Dense layer (larq's QuantDense behind a sign) on the FP4 matrix cores
 * ---------------------------------------------------------------------------------- */

/* The converter has no binary fully-connected operator: a binarized Dense layer arrives as LceQuantize -> LceDequantize -> a float
 * FULLY_CONNECTED whose weights in row o are all +s[o] or -s[o] (the +-1 kernel times the folded batch-norm scale).
 *
 * lce_hip_bfc_prepare (host only, needs no device): from the descriptor and the file's float weights [outputs][inputs] it writes
 *   bits[outputs][ceil(inputs/32)], LSB first, bit 1 for a NEGATIVE weight, the padding bits of a ragged last word 0, and
 *   scale[outputs] = s[o].  LCE_HIP_ERR_UNSUPPORTED unless every entry of row o has the same magnitude s[o], finite, with
 *   2^-100 <= s[o] <= 2^100: a zero (+0.0 or -0.0), a NaN, an infinity or a row of mixed magnitudes is refused, and so is
 *   inputs >= 2^23 (every partial sum must stay an exact float32 integer).  LCE_HIP_ERR_INVALID: a NULL pointer, what the
 *   check refuses.
 * lce_hip_bfc_check (host only): the descriptor rules alone -- LCE_HIP_ERR_INVALID for a NULL desc, an extent <= 0, an unknown
 *   activation; LCE_HIP_ERR_UNSUPPORTED for inputs >= 2^23 or 2^31 or more tiles of 32 x 32 outputs.
 * lce_hip_binary_fully_connected: ONE launch on the activation BITS in_bits_dev [batch][ceil(inputs/32)] (an LceQuantize's
 *   output: bit 1 = negative; the padding bits are never read as channels).  Per output element, the bytes stated:
 *     t = sum over k < inputs of a_k * w_k      a_k, w_k in {+1, -1} (bit 0 is +1): an exact integer; as a float +0.0f when zero
 *     p = t * s[o]                              one float32 multiply
 *     v = p + bias[o]                           one float32 add, never contracted with the multiply; bias_dev NULL: no add
 *     v = min(max(v, lo), hi)                   std::max(a, b) = a < b ? b : a: a NaN passes, -0.0 stays -0.0
 *     bit = v < 0                               LceQuantize's rule: -0.0 and NaN give 0; padding bits of a ragged last word are 0
 *   out_dev (nullable) gets v as float32 [batch][outputs], out_bits_dev (nullable) the bits as int32 [batch][ceil(outputs/32)].
 *   For s[o] a power of two the bytes are those of lce_hip_unpack + lce_hip_fully_connected_f32 on the same bits and the float
 *   weights (every step of that chain is then exact); for other s[o] this entry rounds once where the chain rounds per step.
 *   Refused before any device call, LCE_HIP_ERR_INVALID: a NULL desc, input, weights or scale, both outputs NULL, what the check
 *   refuses, an output that overlaps the input, the weights, the scale, the bias or the other output, a pointer that is not
 *   4-byte aligned.  16-byte aligned input and weights with ceil(inputs/32) % 4 == 0 take a wider load path (the same bytes).
 *   Asynchronous on `stream`, capturable in a HIP graph, allocates nothing and copies nothing between host and device. */
typedef struct lce_hip_bfc_desc {
  int32_t batch, inputs, outputs;
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
} lce_hip_bfc_desc;
lce_hip_status lce_hip_bfc_check(const lce_hip_bfc_desc* desc);
lce_hip_status lce_hip_bfc_prepare(const lce_hip_bfc_desc* desc, const float* weights_host /* [outputs][inputs] */,
                                   int32_t* bits /* [outputs][ceil(inputs/32)] */, float* scale /* [outputs] */);
lce_hip_status lce_hip_binary_fully_connected(const lce_hip_bfc_desc* desc, const int32_t* in_bits_dev, const int32_t* weight_bits_dev,
                                              const float* scale_dev, const float* bias_dev /* nullable */, float* out_dev /* nullable */,
                                              int32_t* out_bits_dev /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------
 * The int8 classifier head and the float/int8 boundary (TFLite builtin MEAN, FULLY_CONNECTED, SOFTMAX on int8; QUANTIZE, DEQUANTIZE)
 * ---------------------------------------------------------------------------------- */

/* An int8-converted network ends in the same GlobalAveragePooling -> Dense -> softmax, on int8 tensors, between a QUANTIZE behind
 * its float input and a DEQUANTIZE in front of its float output.  The contracts below are the authority: each states its
 * arithmetic completely and tests/head_i8_ref.py restates it in NumPy.  INTEGRATION.md says which TFLite function each one
 * restates.  Common to the five launch entries: ONE launch, asynchronous on `stream`, capturable in a HIP graph, nothing
 * allocated and nothing copied between host and device, 64-bit offsets throughout; refused before any device call with
 * LCE_HIP_ERR_INVALID: a NULL pointer, an output that overlaps an input (the softmax in place excepted), a scale that is not finite
 * and positive, a zero point outside [-128, 127].  int8 pointers need no alignment; the table and float pointers need 4 bytes.
 * SRDHM (SaturatingRoundingDoublingHighMul), RoundingDivideByPOT and QuantizeMultiplier are as lce_hip_add_int8 states them.
 *
 * lce_hip_fully_connected_i8: out[batch][outputs] int8 at (so, zo) from in[batch][inputs] int8 at (si, zi), the weights int8 in the
 * file's layout [outputs][inputs] with zero point 0 and scales sw[o] (one for all, or one per output), and an optional int32 bias.
 * The arithmetic is exactly lce_hip_conv2d_i8's on a [batch, 1, 1, inputs] image with a 1x1 filter, per output element:
 *   acc = sum_k (x[k] - zi) * w[o][k]                    exact, int32
 *   acc += bias[o]                                       when there is a bias
 *   (m[o], e[o]) = QuantizeMultiplier((double)si * (double)sw[o] / (double)so)
 *   acc = RoundingDivideByPOT(SRDHM(acc * 2^max(e,0), m), max(-e,0))
 *   v   = min(max(acc + zo, act_min), act_max)           CalculateActivationRangeQuantized at (so, zo)
 * so the bytes are lce_hip_conv2d_i8's there.  The kernel is tiled for few rows and many columns: one wave per 16 x 16 tile on
 * v_mfma_i32_16x16x64_i8 (lce_kernels_head_i8.h).
 *   _check: the descriptor alone.  LCE_HIP_ERR_INVALID: a NULL desc, an extent <= 0, an unknown activation, a bad scale or zero
 *     point.  LCE_HIP_ERR_UNSUPPORTED: inputs > 65793 (255 x 128 x K > 2^31 - 1: no table exists), 2^31 or more tiles of 16 x 16.
 *   _prepare: host only; lce_hip_conv2d_i8_prepare's table int32 [3][outputs] = c[o] = bias[o] - zi * sum_k w[o][k], m[o], e[o], and
 *     the activation range, with that entry's refusals, which name the channel (LCE_HIP_ERR_UNSUPPORTED: 255 x 128 x K + max|bias|
 *     > 2^31 - 1; for a channel with e > 0 that bound times 2^e > 2^31 - 1) and its LCE_HIP_ERR_INVALID cases.
 *   launch: `table_dev` is prepare's table on the device.  16-byte aligned input and weights with inputs % 16 == 0 take a faster
 *     load path. */
typedef struct lce_hip_fc_i8_desc {
  int32_t batch, inputs, outputs;
  int32_t activation;   /* NONE | RELU | RELU_N1_TO_1 | RELU6 */
  float input_scale;
  int32_t input_zero_point;
  float output_scale;
  int32_t output_zero_point;
} lce_hip_fc_i8_desc;
lce_hip_status lce_hip_fully_connected_i8_check(const lce_hip_fc_i8_desc* desc);
lce_hip_status lce_hip_fully_connected_i8_prepare(const lce_hip_fc_i8_desc* desc, const int8_t* weights_host /* [outputs][inputs] */,
                                                  const int32_t* bias_host /* nullable */, const float* weight_scales,
                                                  int32_t n_scales /* 1 or outputs */, int32_t* table /* [3][outputs] */,
                                                  int32_t* act_min, int32_t* act_max);
lce_hip_status lce_hip_fully_connected_i8(const lce_hip_fc_i8_desc* desc, const int8_t* in_dev, const int8_t* weights_dev,
                                          const int32_t* table_dev /* [3][outputs] */, int8_t* out_dev, void* stream);

/* lce_hip_mean_i8: out[batch][channels] int8 at (so, zo) from NHWC int8 [batch, height, width, channels] at (si, zi): the MEAN over
 * height and width (keep_dims or not: the bytes are the same).  With n = height * width, per output element:
 *   acc    = sum over the n pixels of (x - zi)                                     exact, int32
 *   (m, e) = QuantizeMultiplier((double)si / (double)so)
 *   t      = RoundingDivideByPOT(SRDHM(acc * 2^max(e,0), m), max(-e,0))
 *   q      = t > 0 ? (t + n/2) / n : (t - n/2) / n                                 C++ int32 division (truncating); n/2 truncating
 *   v      = min(max(q + zo, -128), 127)
 * -- multiply first, then divide rounding half away from zero (reference_integer_ops::Mean).  Equal input and output
 * quantization goes through the same arithmetic: there is no special case.
 *   _check: LCE_HIP_ERR_INVALID: a NULL desc, an extent <= 0, a bad scale or zero point.  LCE_HIP_ERR_UNSUPPORTED: more than 2^60
 *     elements.
 *   _prepare: the check, then (m, e).  LCE_HIP_ERR_UNSUPPORTED where an intermediate could leave int32: |acc| <= 255 n, the left
 *     shift makes it 255 n 2^max(e,0), SRDHM and the rounding division do not enlarge it (m < 2^31), and n/2 is added to it, so
 *     the entry requires  255 * n * 2^max(e,0) + n/2 <= 2^31 - 1  (a multiplier below 1 has e <= 0: n <= 8405024; equal scales
 *     give the multiplier 1 = 2^30 x 2^(1 - 31), e = 1: n <= 4206628).
 *   launch: what the prepare refuses, it refuses. */
typedef struct lce_hip_mean_i8_desc {
  int32_t batch, height, width, channels;
  float input_scale;
  int32_t input_zero_point;
  float output_scale;
  int32_t output_zero_point;
} lce_hip_mean_i8_desc;
lce_hip_status lce_hip_mean_i8_check(const lce_hip_mean_i8_desc* desc);
lce_hip_status lce_hip_mean_i8_prepare(const lce_hip_mean_i8_desc* desc, int32_t* multiplier, int32_t* exponent);
lce_hip_status lce_hip_mean_i8(const lce_hip_mean_i8_desc* desc, const int8_t* in_dev, int8_t* out_dev, void* stream);

/* lce_hip_softmax_i8: the softmax over the last axis of in[rows][cols] int8 at scale si (the zero point cancels), int8 out at
 * EXACTLY (1/256, -128).  It states its own bytes, built on lce_hip_softmax_f32's pieces (every operation float32, no contraction):
 *   d_i = q_i - max_j q_j                         an integer in [-255, 0]
 *   sb  = si * beta                               one float32 multiply
 *   a_i = (float)d_i * sb
 *   e_i = E(a_i)                                  E exactly as lce_hip_softmax_f32 states it
 *   s   = that entry's fixed-order sum            64 partial sums in order from +0.0f, then s_l = s_l + s_{l ^ d}, d = 32 .. 1
 *   p_i = e_i / s                                 the correctly rounded division
 *   t   = p_i * 256.0f
 *   r   = roundf(t)                               half away from zero (NOT floor(t + 0.5f), whose add can round up across 1.0)
 *   v   = min((int)r - 128, 127)
 * in_dev == out_dev (in place) is allowed.
 *   _check: LCE_HIP_ERR_INVALID: rows or cols of 0, an input scale or beta that is not finite and positive, an output scale that
 *     is not finite and positive, an output zero point outside [-128, 127].  LCE_HIP_ERR_UNSUPPORTED: an output quantization other
 *     than (1/256, -128); cols >= 2^31 or more than 2^60 elements.
 *   launch: the check and the pointers (an output that overlaps the input without being it is refused). */
lce_hip_status lce_hip_softmax_i8_check(size_t rows, size_t cols, float input_scale, float beta, float output_scale,
                                        int32_t output_zero_point);
lce_hip_status lce_hip_softmax_i8(size_t rows, size_t cols, float input_scale, float beta, float output_scale,
                                  int32_t output_zero_point, const int8_t* in_dev, int8_t* out_dev, void* stream);

/* lce_hip_quantize_f32_i8 / lce_hip_dequantize_i8_f32: `n` elements across the float / int8 boundary at (scale, zero_point) = (s, zp).
 *   dequantize: out = (float)(q - zp) * s         one float32 multiply; it equals the double product rounded once (AffineDequantize)
 *   quantize:   t = x / s                         the IEEE float32 division
 *               r = roundf(t)                     half away from zero
 *               r = min(max(r, -128 - zp), 127 - zp)   in float, before the conversion: nothing is undefined
 *               v = (int)r + zp                   a NaN gives zp; +inf and -inf saturate to 127 and -128 (AffineQuantize)
 * n == 0 is a no-op.  LCE_HIP_ERR_INVALID: a NULL pointer, a bad scale or zero point, a float pointer that is not 4-byte aligned,
 * an output that overlaps the input.  LCE_HIP_ERR_UNSUPPORTED: more than 2^60 elements. */
lce_hip_status lce_hip_quantize_f32_i8(size_t n, float scale, int32_t zero_point, const float* in_dev, int8_t* out_dev, void* stream);
lce_hip_status lce_hip_dequantize_i8_f32(size_t n, float scale, int32_t zero_point, const int8_t* in_dev, float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * LceBconv2d
 * ---------------------------------------------------------------------------------- */

/* The op attributes + tensor metadata that bconv2d::Init/Prepare collect
 * (tflite/kernels/bconv2d.cc:85-131,137-300; core/bconv2d/params.h:12-32). */
typedef struct lce_hip_bconv2d_desc {
  int32_t batch, in_height, in_width;
  int32_t channels_in;    /* unpacked input channels (attribute "channels_in") */
  int32_t filter_height, filter_width;
  int32_t channels_out;
  int32_t groups;         /* the glue infers it from the filter shape, bconv2d.cc:169-186 */
  int32_t stride_height, stride_width;
  int32_t dilation_height, dilation_width;
  int32_t padding;        /* lce_hip_padding    */
  int32_t pad_values;     /* 0 or 1             */
  int32_t activation;     /* lce_hip_activation */
  int32_t dst_type;       /* LCE_HIP_F32 / LCE_HIP_I8 / LCE_HIP_BITPACKED */
  int32_t semantics;      /* lce_hip_semantics  */
  float out_scale;        /* int8 output: output->params.scale      */
  int32_t out_zero_point; /* int8 output: output->params.zero_point */
} lce_hip_bconv2d_desc;

typedef struct lce_hip_bconv2d_plan lce_hip_bconv2d_plan;

/* Validates the descriptor with the same rules as bconv2d::Prepare (bconv2d.cc:137-300)
 * and infers padding and output shape (TFLite ComputePaddingHeightWidth, :203-210).
 * Host-only: does not touch the GPU, so shape inference works anywhere. */
lce_hip_status lce_hip_bconv2d_plan_create(const lce_hip_bconv2d_desc* desc,
                                           lce_hip_bconv2d_plan** plan);
void lce_hip_bconv2d_plan_destroy(lce_hip_bconv2d_plan* plan);

/* [batch, out_height, out_width, channels_out or ceil(channels_out/32)] (bconv2d.cc:241-248) */
lce_hip_status lce_hip_bconv2d_plan_output_shape(const lce_hip_bconv2d_plan* plan, int32_t dims[4]);
/* padding_values.{height,width} as Prepare stores them (core/bconv2d/params.h:29-31) */
lce_hip_status lce_hip_bconv2d_plan_padding(const lce_hip_bconv2d_plan* plan, int32_t* pad_h,
                                            int32_t* pad_w);

/* Replaces OneTimeSetup (bconv2d.cc:324-392) + indirect_bgemm::Kernel::PackWeights
 * (core/indirect_bgemm/kernel.h:54-94): folds post_activation_{multiplier,bias}, the int8
 * scale/zero-point and the fused activation into the output transform, precomputes the
 * zero-padding correction, repacks the OHWI filter for the kernel.  All pointers are
 * HOST memory and are copied; `thresholds` is required (and the float arrays ignored)
 * iff dst_type is BITPACKED.  Host-only; the upload happens on first run. */
lce_hip_status lce_hip_bconv2d_plan_set_weights(lce_hip_bconv2d_plan* plan,
                                                const int32_t* filter_ohwi_host,
                                                const float* post_activation_multiplier_host,
                                                const float* post_activation_bias_host,
                                                const int32_t* thresholds_host);

/* The folded transform, for inspection: mul/bias have channels_out entries. */
lce_hip_status lce_hip_bconv2d_plan_folded(const lce_hip_bconv2d_plan* plan, float* mul,
                                           float* bias, int32_t* clamp_min, int32_t* clamp_max);

/* Tuning/testing knobs (defaults are all "auto"):
 *   "engine" = "auto" | "valu" (v_xor + v_bcnt popcount kernels) | "mfma" (FP4 matrix cores, FP4
 *              workspace + GEMM whose tiles span images) | "direct" (FP4 matrix cores, each block
 *              expands its own input halo into LDS; what "auto" picks whenever it fits) | "pointwise" (1x1
 *              ungrouped layers of any stride, 64 / 128 / 256 / 512 input channels after padding to 64, a multiple
 *              of 32 output channels: filter bank
 *              in registers, waves stream 32-pixel tiles; what "auto" picks for such layers)
 *              | "stream" (ungrouped 3x3 layers without dilation, up to 512 input channels -- on the 64- / 128- / 256- / 512-channel instance: persistent
 *              blocks, the filter bank resident in registers, input rows expanded once into an LDS ring; its cheapest variant by the
 *              planner's estimate) | "wstream" (the same layers from 65 input channels on: activations stationary in LDS, weights
 *              streamed into registers during the K loop; for launches of a few block steps).  "auto" prices every kernel that can
 *              run the layer -- the streaming kernel's variants, the weight-streaming kernel, the block GEMM -- and takes the
 *              cheapest (csrc/lce_plan.cpp, estimate_*_us; LCE_PLAN_DEBUG=1 in the environment prints the prices);
 *   "stream_rows" = "0" (auto) | rows per segment (a divisor of the output height), "stream_interleave" = "auto" | "0" | "1"
 *              (a block owns segments b, b + grid, ... instead of consecutive ones), "stream_strip" = "-1" (auto) | "0" | a strip width,
 *              "stream_blocks_per_cu" = "auto" | "1" | "2" (two resident blocks per CU: the bitpacked-output instance of the 64-input-channel
 *              bank, where both blocks' LDS fit),
 *              "stream_pixel_phases", "stream_flat", "compute_units", "wstream_blocks" = "0".."4", "wstream_images": tuning / testing
 *              aids of the two streaming kernels;
 *   "int8_rounding" = "auto" | "exact": int8 outputs of the streaming / weight-streaming / pointwise kernels round with floor(y + 0.5)
 *              and (the first two) transform with one fma -- one instruction each -- on plans where the planner proves the bytes equal
 *              to the reference's two roundings + round-half-away for every value the accumulator can take (csrc/lce_plan.cpp,
 *              prepare_int8_epilogue), and run the reference's own sequence otherwise; "exact": always the latter;
 *   "kernel" = "auto" | "tiled" | "general"                        (valu engine);
 *   "tile"   = "auto" | valu lane tile "4x16"|"2x32"|"2x16"|"1x32"|"1x16"
 *                     | matrix-core block tile "256x256"|"256x128"|"512x64"|"128x256"|"128x128"|"256x64"|"128x64"
 *                       (pixels x channels; with engine = mfma or direct);
 *   "phase"  = "all" | "expand" | "gemm"   (engine = mfma, profiling aid: run one of its two kernels);
 *   "epilogue" = "auto" | "tile" | "wide"   (matrix-core float / int8 epilogue: per-tile or joint transpose);
 *   "pointwise_tiles" = "0" (auto) | "1".."8"   (pointwise kernel: 32-pixel tiles per wave);
 *   "pointwise_channels" = "0" (auto) | "32" | "64" | "128"   (pointwise kernel: output channels per block);
 *   "tile2d" = "auto" | "on" | "off"   (direct variant: 2-D tiles of BM/32 rows x 32 columns instead of row-major strips;
 *              auto takes them on wide images, where they stage <= 0.7 of the strip's halo at <= 3 % more padding). */
lce_hip_status lce_hip_bconv2d_plan_set_option(lce_hip_bconv2d_plan* plan, const char* key,
                                               const char* value);
/* Name of the kernel variant the next run will launch (static string owned by the plan). */
const char* lce_hip_bconv2d_plan_kernel_name(lce_hip_bconv2d_plan* plan);
/* The same for lce_hip_bconv2d_run_dual.  Since round 5 the choice does not depend on the kind of call (one selection per plan):
 * kept for callers of round 4's ABI, returns what lce_hip_bconv2d_plan_kernel_name returns. */
const char* lce_hip_bconv2d_plan_kernel_name_dual(lce_hip_bconv2d_plan* plan);

/* What the int8 epilogue of the kernel the next run will launch does (int8 plans with weights set; otherwise both outputs are 0):
 * *one_instruction_forms = 1 when it transforms with one fma and / or rounds with floor(y + 0.5) -- forms the planner has proven
 * byte-identical to the reference's two roundings + round-half-away (core/bconv2d/output_transform.h:31-44,125-144) for every value the
 * accumulator can take on this plan -- and 0 when it runs the reference's own sequence; *adjusted_channels = the number of output
 * channels whose folded multiplier / bias that proof replaced by NEIGHBOURING floats (<= 2 ulps / 4 grid steps; the bytes written are
 * still the reference's on the original parameters).  "int8_rounding" = "exact" forces 0 / 0.  Either pointer may be NULL. */
lce_hip_status lce_hip_bconv2d_plan_int8_epilogue(lce_hip_bconv2d_plan* plan, int32_t* one_instruction_forms,
                                                  int32_t* adjusted_channels);

/* Replaces bconv2d::Eval (bconv2d.cc:550-564) -> BConv2DReference /
 * BConv2DOptimizedBGEMM / BConv2DOptimizedIndirectBGEMM (core/bconv2d/ headers) with
 * device-resident tensors: input int32 [B,H,W,ceil(Cin/32)], output per dst_type.
 * Asynchronous on `stream`.
 *
 * Devices and streams.  A plan's weights, tables, workspace and staging buffers live on ONE HIP device:
 * the one that is current at the plan's first run (lce_hip_bconv2d_plan_device).  Running it while another
 * device is current fails with LCE_HIP_ERR_INVALID -- create one plan per device (the batch-shard mode of
 * SURVEY.md 8(e) runs one process per GPU).  A plan may be run on any stream of that device, one call at a
 * time per plan: calls from several host threads into the SAME plan must be serialised by the caller (the
 * reference's OpData is per node and TFLite invokes a node from one thread, tflite/kernels/bconv2d.cc:44-74);
 * calls on different streams are ordered by the library where they share the plan's workspace.  Different
 * plans are independent. */
lce_hip_status lce_hip_bconv2d_run(lce_hip_bconv2d_plan* plan, const int32_t* input_dev,
                                   void* output_dev, void* stream);
/* The HIP device the plan is bound to, -1 before its first run. */
int lce_hip_bconv2d_plan_device(const lce_hip_bconv2d_plan* plan);

/* LceBconv2d (float or int8 output) and the LceQuantize that follows it in a converted graph
 * (tflite/kernels/quantization.cc:76-114 on the convolution's output), in one pass: `output_dev` gets the
 * tensor [B,OH,OW,Cout] exactly as lce_hip_bconv2d_run writes it, `output_bits_dev` its quantization
 * [B,OH,OW,ceil(Cout/32)] exactly as lce_hip_bitpack(F32, output_dev, ..., 0, ...) -- sign bits -- or, for an int8
 * plan, lce_hip_bitpack(I8, output_dev, ..., out_zero_point, ...) -- bit = (q < zero_point) -- would: from the same
 * epilogue (the value a lane just produced is compared and balloted) where the kernel variant allows, by a second
 * launch on the same stream otherwise.  Saves re-reading the tensor between the binary convolutions of a
 * device-resident chain.  The plan's dst_type must be LCE_HIP_F32 or LCE_HIP_I8. */
lce_hip_status lce_hip_bconv2d_run_dual(lce_hip_bconv2d_plan* plan, const int32_t* input_dev,
                                        void* output_dev, int32_t* output_bits_dev, void* stream);

/* Same as lce_hip_bconv2d_run with host tensors (the interpreter arena), synchronous.  The batch is cut
 * into slices that flow through three streams (H2D | kernel | D2H) so that the copies of neighbouring
 * slices overlap the compute.  The overlap is complete when the two buffers are page-locked
 * (lce_hip_host_register -- an arena is reused for every Invoke, so the glue registers it once); pageable
 * buffers work too, with the runtime staging every copy. */
lce_hip_status lce_hip_bconv2d_run_host(lce_hip_bconv2d_plan* plan, const int32_t* input_host,
                                        void* output_host);

/* ------------------------------------------------------------------------------------
 * LceBMaxPool2d (core/bmaxpool.h:24-88; tflite/kernels/bmaxpool.cc:20-98)
 * ---------------------------------------------------------------------------------- */
lce_hip_status lce_hip_bmaxpool_output_shape(int32_t in_height, int32_t in_width,
                                             int32_t filter_height, int32_t filter_width,
                                             int32_t stride_height, int32_t stride_width,
                                             int32_t padding, int32_t* out_height,
                                             int32_t* out_width);
lce_hip_status lce_hip_bmaxpool(const int32_t* input_dev, int32_t batch, int32_t in_height,
                                int32_t in_width, int32_t words, int32_t filter_height,
                                int32_t filter_width, int32_t stride_height, int32_t stride_width,
                                int32_t padding, int32_t* output_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Converter-side parameter preparation (host-only).
 * What the reference's MLIR converter does offline to the constants of one binary
 * convolution, so that an unconverted Larq layer (float +-scale HWIO filter, fused
 * mul/add constants) arrives at exactly the tensors LceBconv2d expects.  WEIGHTS only --
 * nothing here processes activations.  Paths relative to larq_compute_engine/mlir/.
 * ---------------------------------------------------------------------------------- */

/* transforms/prepare_patterns_common.td:97-168 + prepare_tf.cc:40-92: checks the filter is
 * binary (+-scale[o] within 0.5 %), writes filter/|scale| transposed HWIO -> OHWI,
 * post_activation_multiplier = |scale|, post_activation_bias = 0 (either may be NULL). */
lce_hip_status lce_hip_prepare_binary_filter(const float* filter_hwio, int32_t filter_height,
                                             int32_t filter_width, int32_t channels_in_per_group,
                                             int32_t channels_out, float* filter_ohwi,
                                             float* post_activation_multiplier,
                                             float* post_activation_bias);

typedef enum lce_hip_post_op {
  LCE_HIP_POST_ADD = 0, LCE_HIP_POST_SUB = 1, LCE_HIP_POST_MUL = 2, LCE_HIP_POST_DIV = 3
} lce_hip_post_op;
/* transforms/optimize_patterns_common.td:39-118: fuse `conv <op> constant` (constant scalar
 * or per-channel) into post_activation_{multiplier,bias}, float arithmetic. */
lce_hip_status lce_hip_prepare_fuse_post_op(lce_hip_post_op op, const float* value,
                                            int32_t value_count, float* post_activation_multiplier,
                                            float* post_activation_bias, int32_t channels_out);
/* transforms/optimize_patterns_common.td:122-182: 1 iff a following Relu/Relu1/Relu6 may
 * become the fused activation (multiplier all 1, bias all 0, VALID or SAME/pad_values 1). */
int lce_hip_prepare_can_fuse_activation(const float* post_activation_multiplier,
                                        const float* post_activation_bias, int32_t channels_out,
                                        int32_t padding, int32_t pad_values);

/* transforms/bitpack_activations_patterns.td:19-60 + optimize.cc:128-244: the rewrite of
 * LceQuantize(LceBconv2d(x)) into a bit-writing convolution: multiplies filter_ohwi IN PLACE
 * by sign(multiplier) and computes the int32 thresholds (bit = accumulator > threshold). */
lce_hip_status lce_hip_prepare_bitpacked_output(float* filter_ohwi, int32_t filter_height,
                                                int32_t filter_width, int32_t channels_in_per_group,
                                                int32_t channels_out, int32_t activation,
                                                int32_t padding, int32_t pad_values,
                                                const float* post_activation_multiplier,
                                                const float* post_activation_bias,
                                                int32_t* thresholds);

/* transforms/bitpack.cc:19-57: float OHWI filter -> int32 [O][H][W][ceil(I/32)]
 * (bit = x < 0, LSB first, rows padded with 0 bits) = input 1 of LceBconv2d. */
lce_hip_status lce_hip_prepare_bitpack_filter(const float* filter_ohwi, int32_t filter_height,
                                              int32_t filter_width, int32_t channels_in_per_group,
                                              int32_t channels_out, int32_t* filter_words);

#ifdef __cplusplus
}
#endif
#endif /* LCE_HIP_H_ */
