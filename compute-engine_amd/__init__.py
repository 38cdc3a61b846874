"""MI355X-native LceBconv2d / LceQuantize hot path -- thin Python binding of the C ABI.

The product is the C-ABI shared library ``csrc/liblce_hip.so`` (hand-written gfx950
kernels, declared in ``include/lce_hip.h``) plus the C++ TFLite op glue in
``csrc/tflite/``.  This module only loads the library with ``ctypes`` and passes raw
device pointers to it (PyTorch is used by callers purely to own HBM buffers and
streams).  There is no fallback of any kind: if the library is missing or there is no
GPU, calls raise.

The directory name contains a hyphen, so import it with
``importlib.import_module("compute-engine_amd")``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LCE_HIP_LIBRARY: an alternative build of the same library (kernel A/B experiments, tools/)
LIB_PATH = os.environ.get("LCE_HIP_LIBRARY") or os.path.join(_HERE, "csrc", "liblce_hip.so")

# enums of include/lce_hip.h
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_RUNTIME, ERR_NO_DEVICE = range(5)
F32, I8, BITPACKED, BOOL = range(4)
PADDING_SAME, PADDING_VALID = 0, 1
ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6 = range(4)
SEM_REFERENCE, SEM_OPTIMIZED = 0, 1

# every symbol include/lce_hip.h declares (tests check the library exports them all)
ABI_SYMBOLS = (
    "lce_hip_abi_version", "lce_hip_last_error", "lce_hip_build_flavor", "lce_hip_device_count", "lce_hip_set_device",
    "lce_hip_malloc", "lce_hip_free", "lce_hip_memcpy_h2d", "lce_hip_memcpy_d2h", "lce_hip_memcpy_d2d", "lce_hip_memset",
    "lce_hip_host_register", "lce_hip_host_unregister",
    "lce_hip_stream_create", "lce_hip_stream_destroy", "lce_hip_stream_synchronize",
    "lce_hip_graph_begin_capture", "lce_hip_graph_end_capture", "lce_hip_graph_launch", "lce_hip_graph_destroy",
    "lce_hip_bitpacked_size", "lce_hip_bitpack", "lce_hip_unpack", "lce_hip_elementwise",
    "lce_hip_elementwise_ex", "lce_hip_elementwise_grid_cap",
    "lce_hip_add_int8_prepare", "lce_hip_add_int8", "lce_hip_add_int8_variant", "lce_hip_add_int8_forced",
    "lce_hip_elementwise_i8_check", "lce_hip_elementwise_i8_table_size", "lce_hip_elementwise_i8_prepare", "lce_hip_elementwise_i8",
    "lce_hip_elementwise_i8_path", "lce_hip_elementwise_i8_forced",
    "lce_hip_mul_int8_prepare", "lce_hip_mul_int8", "lce_hip_mul_int8_path", "lce_hip_logistic_int8_prepare", "lce_hip_logistic_int8",
    "lce_hip_concat", "lce_hip_join_windows", "lce_hip_join_windows_check", "lce_hip_pool2d", "lce_hip_pool2d_check", "lce_hip_conv1x1_f32", "lce_hip_conv1x1_f32_check",
    "lce_hip_depthwise_conv2d_f32", "lce_hip_depthwise_conv2d_f32_check", "lce_hip_conv2d_f32", "lce_hip_conv2d_f32_check",
    "lce_hip_conv2d_i8", "lce_hip_conv2d_i8_check", "lce_hip_conv2d_i8_prepare",
    "lce_hip_depthwise_conv2d_i8", "lce_hip_depthwise_conv2d_i8_check", "lce_hip_depthwise_conv2d_i8_prepare",
    "lce_hip_depthwise_conv2d_i8_path", "lce_hip_depthwise_conv2d_i8_forced",
    "lce_hip_pool_depthwise_f32", "lce_hip_pool_depthwise_f32_check", "lce_hip_pool_depthwise_f32_path", "lce_hip_pool_depthwise_f32_forced",
    "lce_hip_pool_depthwise_i8", "lce_hip_pool_depthwise_i8_check", "lce_hip_pool_depthwise_i8_path", "lce_hip_pool_depthwise_i8_forced",
    "lce_hip_fully_connected_f32", "lce_hip_fully_connected_f32_check", "lce_hip_softmax_f32", "lce_hip_softmax_f32_check",
    "lce_hip_bfc_check", "lce_hip_bfc_prepare", "lce_hip_binary_fully_connected",
    "lce_hip_fully_connected_i8", "lce_hip_fully_connected_i8_check", "lce_hip_fully_connected_i8_prepare",
    "lce_hip_mean_i8", "lce_hip_mean_i8_check", "lce_hip_mean_i8_prepare", "lce_hip_softmax_i8", "lce_hip_softmax_i8_check",
    "lce_hip_quantize_f32_i8", "lce_hip_dequantize_i8_f32",
    "lce_hip_bconv2d_plan_create", "lce_hip_bconv2d_plan_destroy", "lce_hip_bconv2d_plan_output_shape",
    "lce_hip_bconv2d_plan_padding", "lce_hip_bconv2d_plan_set_weights", "lce_hip_bconv2d_plan_folded",
    "lce_hip_bconv2d_plan_set_option", "lce_hip_bconv2d_plan_kernel_name", "lce_hip_bconv2d_plan_kernel_name_dual", "lce_hip_bconv2d_plan_int8_epilogue", "lce_hip_bconv2d_run",
    "lce_hip_bconv2d_run_dual", "lce_hip_bconv2d_plan_device", "lce_hip_bconv2d_run_host", "lce_hip_bmaxpool_output_shape", "lce_hip_bmaxpool",
    "lce_hip_prepare_binary_filter", "lce_hip_prepare_fuse_post_op", "lce_hip_prepare_can_fuse_activation",
    "lce_hip_prepare_bitpacked_output", "lce_hip_prepare_bitpack_filter",
)
POST_ADD, POST_SUB, POST_MUL, POST_DIV = 0, 1, 2, 3
EW_ADD, EW_MUL = 0, 1                                   # lce_hip_ew_op
EW_SCALAR, EW_PER_CHANNEL, EW_TENSOR = 0, 1, 2          # lce_hip_ew_operand
EW_CLAMP, EW_PRELU, EW_LOGISTIC = 2, 3, 4                # lce_hip_ew_op_ex
EW_PER_IMAGE_CHANNEL = 3                                # lce_hip_ew_operand_ex
EW_MAX_STEPS = 8
CONCAT_MAX_INPUTS = 8                                   # LCE_HIP_CONCAT_MAX_INPUTS
JOIN_MAX_WINDOWS = 8                                    # LCE_HIP_JOIN_MAX_WINDOWS
POOL_MAX, POOL_AVERAGE = 0, 1                           # lce_hip_pool_op
POOL_MAX_TAPS = 65536                                   # LCE_HIP_POOL_MAX_TAPS
ADD_INT8_LITERAL, ADD_INT8_SPLIT, ADD_INT8_SHIFT = 0, 1, 2   # lce_hip_add_int8_variant_id
EW_I8_ADD, EW_I8_PRELU, EW_I8_CLAMP, EW_I8_REQUANTIZE = 0, 1, 2, 3   # lce_hip_ew_i8_op
EW_I8_PATH_LDS, EW_I8_PATH_GLOBAL, EW_I8_PATH_ONE_ROW = 0, 1, 2      # lce_hip_elementwise_i8_path_id


class LceHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"lce_hip error {code}: {message}")
        self.code = code
        self.message = message


class Bconv2dDesc(C.Structure):
    """``lce_hip_bconv2d_desc``."""
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "in_height", "in_width", "channels_in", "filter_height", "filter_width",
        "channels_out", "groups", "stride_height", "stride_width", "dilation_height",
        "dilation_width", "padding", "pad_values", "activation", "dst_type", "semantics")] + [
        ("out_scale", C.c_float), ("out_zero_point", C.c_int32)]


class EwStep(C.Structure):
    """``lce_hip_ew_step``."""
    _fields_ = [("op", C.c_int32), ("operand", C.c_int32), ("values", C.c_void_p), ("scalar", C.c_float),
                ("activation", C.c_int32)]


class EwStepEx(C.Structure):
    """``lce_hip_ew_step_ex``."""
    _fields_ = [("op", C.c_int32), ("operand", C.c_int32), ("values", C.c_void_p), ("scalar", C.c_float),
                ("activation", C.c_int32), ("reserved", C.c_int32 * 2)]


class AddInt8Desc(C.Structure):
    """``lce_hip_add_int8_desc``."""
    _fields_ = [("in1_scale", C.c_float), ("in1_zero_point", C.c_int32), ("in2_scale", C.c_float), ("in2_zero_point", C.c_int32),
                ("out_scale", C.c_float), ("out_zero_point", C.c_int32), ("activation", C.c_int32)]


class AddInt8Params(C.Structure):
    """``lce_hip_add_int8_params``."""
    _fields_ = [(n, C.c_int32) for n in ("left_shift", "in1_multiplier", "in1_shift", "in2_multiplier", "in2_shift",
                                         "out_multiplier", "out_shift", "act_min", "act_max")]


class EwI8Step(C.Structure):
    """``lce_hip_ew_i8_step``."""
    _fields_ = [("op", C.c_int32), ("operand", C.c_int32), ("values", C.c_void_p), ("operand_scale", C.c_float),
                ("operand_zero_point", C.c_int32), ("out_scale", C.c_float), ("out_zero_point", C.c_int32), ("activation", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class EwI8Desc(C.Structure):
    """``lce_hip_elementwise_i8_desc``."""
    _fields_ = [("channels", C.c_int32), ("in_scale", C.c_float), ("in_zero_point", C.c_int32), ("has_head", C.c_int32),
                ("addend_scale", C.c_float), ("addend_zero_point", C.c_int32), ("head_scale", C.c_float),
                ("head_zero_point", C.c_int32), ("head_activation", C.c_int32), ("num_steps", C.c_int32),
                ("steps", EwI8Step * EW_MAX_STEPS), ("reserved", C.c_int32 * 2)]


class EwI8Launch(C.Structure):
    """``lce_hip_elementwise_i8_launch``."""
    _fields_ = [(n, C.c_int32) for n in ("path", "flat", "lds_max_channels", "blocks", "waves_per_block", "lds_bytes", "head_variant",
                                         "table_rows")]


class MulInt8Desc(C.Structure):
    """``lce_hip_mul_int8_desc``."""
    _fields_ = [("in1_scale", C.c_float), ("in1_zero_point", C.c_int32), ("in2_scale", C.c_float), ("in2_zero_point", C.c_int32),
                ("out_scale", C.c_float), ("out_zero_point", C.c_int32), ("activation", C.c_int32), ("operand", C.c_int32),
                ("has_add", C.c_int32), ("addend_scale", C.c_float), ("addend_zero_point", C.c_int32), ("add_scale", C.c_float),
                ("add_zero_point", C.c_int32), ("add_activation", C.c_int32), ("reserved", C.c_int32 * 2)]


class MulInt8Params(C.Structure):
    """``lce_hip_mul_int8_params``."""
    _fields_ = [("multiplier", C.c_int32), ("shift", C.c_int32), ("act_min", C.c_int32), ("act_max", C.c_int32), ("add", AddInt8Params)]


class MulInt8Launch(C.Structure):
    """``lce_hip_mul_int8_launch``."""
    _fields_ = [(n, C.c_int32) for n in ("flat", "blocks", "waves_per_block", "add_variant", "mul_variant", "product_first")] + \
               [("add_args", C.c_int32 * 21)]


class Pool2dDesc(C.Structure):
    """``lce_hip_pool2d_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("op", "type", "batch", "in_height", "in_width", "channels", "filter_height",
                                         "filter_width", "stride_height", "stride_width", "padding", "activation")] + [
        ("scale", C.c_float), ("zero_point", C.c_int32)]


class Conv1x1Desc(C.Structure):
    """``lce_hip_conv1x1_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "in_height", "in_width", "channels_in", "channels_out", "stride_height",
                                         "stride_width", "activation")]


class DepthwiseDesc(C.Structure):
    """``lce_hip_depthwise_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "in_height", "in_width", "channels_in", "depth_multiplier", "filter_height",
                                         "filter_width", "stride_height", "stride_width", "padding", "activation")]


class Conv2dDesc(C.Structure):
    """``lce_hip_conv2d_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "in_height", "in_width", "channels_in", "channels_out", "filter_height",
                                         "filter_width", "stride_height", "stride_width", "padding", "activation")]


class Conv2dI8Desc(C.Structure):
    """``lce_hip_conv2d_i8_desc``."""
    _fields_ = Conv2dDesc._fields_ + [("input_scale", C.c_float), ("input_zero_point", C.c_int32), ("output_scale", C.c_float),
                                      ("output_zero_point", C.c_int32)]


class DepthwiseI8Desc(C.Structure):
    """``lce_hip_depthwise_i8_desc``."""
    _fields_ = DepthwiseDesc._fields_ + [("input_scale", C.c_float), ("input_zero_point", C.c_int32), ("output_scale", C.c_float),
                                         ("output_zero_point", C.c_int32)]


class FcDesc(C.Structure):
    """``lce_hip_fc_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "inputs", "outputs", "activation")]


class BfcDesc(C.Structure):
    """``lce_hip_bfc_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "inputs", "outputs", "activation")]


class FcI8Desc(C.Structure):
    """``lce_hip_fc_i8_desc``."""
    _fields_ = FcDesc._fields_ + [("input_scale", C.c_float), ("input_zero_point", C.c_int32), ("output_scale", C.c_float),
                                  ("output_zero_point", C.c_int32)]


class MeanI8Desc(C.Structure):
    """``lce_hip_mean_i8_desc``."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "height", "width", "channels")] + [
        ("input_scale", C.c_float), ("input_zero_point", C.c_int32), ("output_scale", C.c_float), ("output_zero_point", C.c_int32)]


_lib = None


def lib() -> C.CDLL:
    """Load ``liblce_hip.so``; raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with `make -C compute-engine_amd/csrc` "
                "(there is no Python or CPU fallback for the HIP kernels)")
        l = C.CDLL(LIB_PATH)
        l.lce_hip_last_error.restype = C.c_char_p
        l.lce_hip_build_flavor.restype = C.c_char_p
        l.lce_hip_bconv2d_plan_kernel_name.restype = C.c_char_p
        l.lce_hip_bconv2d_plan_kernel_name.argtypes = [C.c_void_p]
        l.lce_hip_bconv2d_plan_kernel_name_dual.restype = C.c_char_p
        l.lce_hip_bconv2d_plan_kernel_name_dual.argtypes = [C.c_void_p]
        l.lce_hip_bconv2d_plan_int8_epilogue.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_bconv2d_plan_destroy.restype = None
        l.lce_hip_bconv2d_plan_destroy.argtypes = [C.c_void_p]
        l.lce_hip_bconv2d_plan_create.argtypes = [C.POINTER(Bconv2dDesc), C.POINTER(C.c_void_p)]
        l.lce_hip_bconv2d_plan_output_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        l.lce_hip_bconv2d_plan_padding.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_bconv2d_plan_set_weights.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        l.lce_hip_bconv2d_plan_folded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_bconv2d_plan_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        l.lce_hip_bconv2d_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_bconv2d_run_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_bconv2d_run_dual.argtypes = [C.c_void_p] * 5
        l.lce_hip_host_register.argtypes = [C.c_void_p, C.c_size_t]
        l.lce_hip_host_unregister.argtypes = [C.c_void_p]
        l.lce_hip_bconv2d_plan_device.argtypes = [C.c_void_p]
        l.lce_hip_bitpack.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32,
                                      C.c_void_p, C.c_void_p]
        l.lce_hip_unpack.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float,
                                     C.c_int32, C.c_void_p, C.c_void_p]
        l.lce_hip_elementwise.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(EwStep), C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_elementwise_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(EwStepEx), C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_elementwise_grid_cap.argtypes, l.lce_hip_elementwise_grid_cap.restype = [], C.c_int32
        l.lce_hip_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        l.lce_hip_add_int8_prepare.argtypes = [C.POINTER(AddInt8Desc), C.POINTER(AddInt8Params)]
        l.lce_hip_add_int8_variant.argtypes = [C.POINTER(AddInt8Desc), C.POINTER(C.c_int32)]
        l.lce_hip_add_int8.argtypes = [C.POINTER(AddInt8Desc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_add_int8_forced.argtypes = [C.POINTER(AddInt8Desc), C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_elementwise_i8_check.argtypes = [C.POINTER(EwI8Desc)]
        l.lce_hip_elementwise_i8_table_size.argtypes = [C.POINTER(EwI8Desc), C.POINTER(C.c_size_t)]
        l.lce_hip_elementwise_i8_prepare.argtypes = [C.POINTER(EwI8Desc), C.c_void_p]
        l.lce_hip_elementwise_i8.argtypes = [C.POINTER(EwI8Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        l.lce_hip_elementwise_i8_path.argtypes = [C.POINTER(EwI8Desc), C.c_size_t] + [C.c_void_p] * 5 + [C.c_int32, C.POINTER(EwI8Launch)]
        l.lce_hip_elementwise_i8_forced.argtypes = [C.POINTER(EwI8Desc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_mul_int8_prepare.argtypes = [C.POINTER(MulInt8Desc), C.POINTER(MulInt8Params)]
        l.lce_hip_mul_int8.argtypes = [C.POINTER(MulInt8Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_mul_int8_path.argtypes = [C.POINTER(MulInt8Desc), C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_void_p] * 5 + \
                                           [C.POINTER(MulInt8Launch)]
        l.lce_hip_logistic_int8_prepare.argtypes = [C.c_float, C.c_int32, C.c_float, C.c_int32, C.c_void_p]
        l.lce_hip_logistic_int8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_concat.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_size_t, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_join_windows.argtypes = [C.c_int, C.POINTER(Window), C.c_int32, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_join_windows_check.argtypes = [C.c_int, C.POINTER(Window), C.c_int32]
        l.lce_hip_pool2d.argtypes = [C.POINTER(Pool2dDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_pool2d_check.argtypes = [C.POINTER(Pool2dDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_conv1x1_f32.argtypes = [C.POINTER(Conv1x1Desc)] + [C.c_void_p] * 6
        l.lce_hip_conv1x1_f32_check.argtypes = [C.POINTER(Conv1x1Desc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_depthwise_conv2d_f32.argtypes = [C.POINTER(DepthwiseDesc)] + [C.c_void_p] * 6
        l.lce_hip_depthwise_conv2d_f32_check.argtypes = [C.POINTER(DepthwiseDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_conv2d_f32.argtypes = [C.POINTER(Conv2dDesc)] + [C.c_void_p] * 6
        l.lce_hip_conv2d_f32_check.argtypes = [C.POINTER(Conv2dDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_conv2d_i8.argtypes = [C.POINTER(Conv2dI8Desc)] + [C.c_void_p] * 6
        l.lce_hip_conv2d_i8_check.argtypes = [C.POINTER(Conv2dI8Desc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_conv2d_i8_prepare.argtypes = [C.POINTER(Conv2dI8Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_depthwise_conv2d_i8.argtypes = [C.POINTER(DepthwiseI8Desc)] + [C.c_void_p] * 6
        l.lce_hip_depthwise_conv2d_i8_check.argtypes = [C.POINTER(DepthwiseI8Desc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_depthwise_conv2d_i8_prepare.argtypes = [C.POINTER(DepthwiseI8Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                          C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_depthwise_conv2d_i8_path.argtypes = [C.POINTER(DepthwiseI8Desc)] + [C.c_void_p] * 5 + [C.POINTER(C.c_int32)]
        l.lce_hip_depthwise_conv2d_i8_forced.argtypes = [C.POINTER(DepthwiseI8Desc), C.c_int32] + [C.c_void_p] * 6
        for kind, dw in (("f32", DepthwiseDesc), ("i8", DepthwiseI8Desc)):
            descs = [C.POINTER(Pool2dDesc), C.POINTER(dw)]
            getattr(l, "lce_hip_pool_depthwise_%s_check" % kind).argtypes = descs + [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            getattr(l, "lce_hip_pool_depthwise_%s" % kind).argtypes = descs + [C.c_void_p] * 6
            getattr(l, "lce_hip_pool_depthwise_%s_path" % kind).argtypes = descs + [C.c_void_p] * 5 + [C.POINTER(C.c_int32)]
            getattr(l, "lce_hip_pool_depthwise_%s_forced" % kind).argtypes = descs + [C.c_int32] + [C.c_void_p] * 6
        l.lce_hip_fully_connected_f32.argtypes = [C.POINTER(FcDesc)] + [C.c_void_p] * 5
        l.lce_hip_fully_connected_f32_check.argtypes = [C.POINTER(FcDesc)]
        l.lce_hip_softmax_f32.argtypes = [C.c_size_t, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hip_softmax_f32_check.argtypes = [C.c_size_t, C.c_size_t, C.c_float]
        l.lce_hip_bfc_check.argtypes = [C.POINTER(BfcDesc)]
        l.lce_hip_bfc_prepare.argtypes = [C.POINTER(BfcDesc)] + [C.c_void_p] * 3
        l.lce_hip_binary_fully_connected.argtypes = [C.POINTER(BfcDesc)] + [C.c_void_p] * 7
        l.lce_hip_fully_connected_i8.argtypes = [C.POINTER(FcI8Desc)] + [C.c_void_p] * 5
        l.lce_hip_fully_connected_i8_check.argtypes = [C.POINTER(FcI8Desc)]
        l.lce_hip_fully_connected_i8_prepare.argtypes = [C.POINTER(FcI8Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_mean_i8.argtypes = [C.POINTER(MeanI8Desc)] + [C.c_void_p] * 3
        l.lce_hip_mean_i8_check.argtypes = [C.POINTER(MeanI8Desc)]
        l.lce_hip_mean_i8_prepare.argtypes = [C.POINTER(MeanI8Desc), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_hip_softmax_i8_check.argtypes = [C.c_size_t, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_int32]
        l.lce_hip_softmax_i8.argtypes = [C.c_size_t, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_int32] + [C.c_void_p] * 3
        l.lce_hip_quantize_f32_i8.argtypes = [C.c_size_t, C.c_float, C.c_int32] + [C.c_void_p] * 3
        l.lce_hip_dequantize_i8_f32.argtypes = [C.c_size_t, C.c_float, C.c_int32] + [C.c_void_p] * 3
        l.lce_hip_bmaxpool.argtypes = [C.c_void_p] + [C.c_int32] * 9 + [C.c_void_p, C.c_void_p]
        l.lce_hip_bmaxpool_output_shape.argtypes = [C.c_int32] * 7 + [C.POINTER(C.c_int32)] * 2
        _lib = l
    return _lib


def check(code: int) -> None:
    if code != OK:
        raise LceHipError(code, lib().lce_hip_last_error().decode(errors="replace"))


def device_count() -> int:
    return lib().lce_hip_device_count()


def bitpacked_size(n: int) -> int:
    return (n + 31) // 32


def _host_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class ConvParams:
    """The LceBconv2d attributes (tflite/kernels/bconv2d.cc:94-124) plus tensor metadata."""
    batch: int
    in_height: int
    in_width: int
    channels_in: int
    filter_height: int
    filter_width: int
    channels_out: int
    groups: int = 1
    stride_height: int = 1
    stride_width: int = 1
    dilation_height: int = 1
    dilation_width: int = 1
    padding: int = PADDING_VALID
    pad_values: int = 0
    activation: int = ACT_NONE
    dst_type: int = F32
    semantics: int = SEM_OPTIMIZED
    out_scale: float = 1.0
    out_zero_point: int = 0

    def desc(self) -> Bconv2dDesc:
        return Bconv2dDesc(self.batch, self.in_height, self.in_width, self.channels_in,
                           self.filter_height, self.filter_width, self.channels_out, self.groups,
                           self.stride_height, self.stride_width, self.dilation_height,
                           self.dilation_width, self.padding, self.pad_values, self.activation,
                           self.dst_type, self.semantics, float(self.out_scale),
                           int(self.out_zero_point))


class Bconv2dPlan:
    """Owns one ``lce_hip_bconv2d_plan`` (Prepare + OneTimeSetup of one LceBconv2d node)."""

    def __init__(self, params: ConvParams):
        self.params = params
        self._h = C.c_void_p()
        d = params.desc()
        check(lib().lce_hip_bconv2d_plan_create(C.byref(d), C.byref(self._h)))
        dims = (C.c_int32 * 4)()
        check(lib().lce_hip_bconv2d_plan_output_shape(self._h, dims))
        self.output_shape = tuple(dims)

    @classmethod
    def from_handle(cls, handle: int, dst_type: int, channels_out: int = 0) -> "Bconv2dPlan":
        """Adopts a plan created through the C ABI elsewhere (lce_tflite_model_bconv2d_plan)."""
        import types
        self = cls.__new__(cls)
        self.params = types.SimpleNamespace(dst_type=dst_type, channels_out=channels_out)
        self._h = C.c_void_p(handle)
        dims = (C.c_int32 * 4)()
        check(lib().lce_hip_bconv2d_plan_output_shape(self._h, dims))
        self.output_shape = tuple(dims)
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None:
            _lib.lce_hip_bconv2d_plan_destroy(self._h)   # (_lib is None again during interpreter teardown)
            self._h = C.c_void_p()

    __del__ = close

    def padding(self):
        ph, pw = C.c_int32(), C.c_int32()
        check(lib().lce_hip_bconv2d_plan_padding(self._h, C.byref(ph), C.byref(pw)))
        return ph.value, pw.value

    def set_weights(self, filter_ohwi, post_mul=None, post_bias=None, thresholds=None):
        """Host numpy arrays: int32 OHWI filter words, float32 [Cout] x2, int32 [Cout]."""
        import numpy as np
        f = np.ascontiguousarray(filter_ohwi, np.int32)
        m = None if post_mul is None else np.ascontiguousarray(post_mul, np.float32)
        b = None if post_bias is None else np.ascontiguousarray(post_bias, np.float32)
        t = None if thresholds is None else np.ascontiguousarray(thresholds, np.int32)
        p = self.params
        if hasattr(p, "filter_height"):   # (a plan adopted from a handle carries no descriptor: the C side owns it)
            # the C ABI reads exactly this many elements from the raw pointers
            want = p.channels_out * p.filter_height * p.filter_width * bitpacked_size(p.channels_in // max(1, p.groups))
            if f.size != want:
                raise ValueError(f"filter has {f.size} words, the plan needs Cout*KH*KW*ceil(Cin/G/32) = {want}")
            for name, a in (("post_activation_multiplier", m), ("post_activation_bias", b), ("thresholds", t)):
                if a is not None and a.size != p.channels_out:
                    raise ValueError(f"{name} has {a.size} entries, the plan needs channels_out = {p.channels_out}")
        check(lib().lce_hip_bconv2d_plan_set_weights(self._h, _host_ptr(f), _host_ptr(m),
                                                     _host_ptr(b), _host_ptr(t)))

    def folded(self):
        import numpy as np
        n = self.params.channels_out
        mul, bias = np.empty(n, np.float32), np.empty(n, np.float32)
        lo, hi = C.c_int32(), C.c_int32()
        check(lib().lce_hip_bconv2d_plan_folded(self._h, _host_ptr(mul), _host_ptr(bias),
                                                C.byref(lo), C.byref(hi)))
        return mul, bias, lo.value, hi.value

    def set_option(self, key: str, value: str):
        check(lib().lce_hip_bconv2d_plan_set_option(self._h, key.encode(), value.encode()))

    def kernel_name(self, dual: bool = False) -> str:
        if dual:
            return lib().lce_hip_bconv2d_plan_kernel_name_dual(self._h).decode()
        return lib().lce_hip_bconv2d_plan_kernel_name(self._h).decode()

    def int8_epilogue(self):
        """(one_instruction_forms, adjusted_channels) of the kernel the next run launches: ``lce_hip_bconv2d_plan_int8_epilogue``."""
        forms, adjusted = C.c_int32(), C.c_int32()
        check(lib().lce_hip_bconv2d_plan_int8_epilogue(self._h, C.byref(forms), C.byref(adjusted)))
        return bool(forms.value), int(adjusted.value)

    def run_ptr(self, input_dev: int, output_dev: int, stream: int = 0):
        check(lib().lce_hip_bconv2d_run(self._h, C.c_void_p(input_dev), C.c_void_p(output_dev),
                                        C.c_void_p(stream)))

    def device(self) -> int:
        """The HIP device the plan's buffers live on (-1 before the first run)."""
        return lib().lce_hip_bconv2d_plan_device(self._h)

    def _check_input(self, x):
        import torch
        assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous()
        p = self.params
        if hasattr(p, "in_height"):
            want = (p.batch, p.in_height, p.in_width, bitpacked_size(p.channels_in))
            if tuple(x.shape) != want:
                raise ValueError(f"input shape {tuple(x.shape)} does not match the plan's {want}")

    def _out(self, x, out, dtype):
        import torch
        if out is None:
            return torch.empty(self.output_shape, dtype=dtype, device=x.device)
        assert out.is_cuda and out.device == x.device and out.dtype == dtype and out.is_contiguous()
        if tuple(out.shape) != tuple(self.output_shape):
            raise ValueError(f"output shape {tuple(out.shape)} does not match the plan's {tuple(self.output_shape)}")
        return out

    def run(self, x, out=None, stream: int | None = None):
        """x: CUDA int32 tensor [B,H,W,ceil(Cin/32)]; returns / fills the output tensor."""
        import torch
        self._check_input(x)
        out = self._out(x, out, {F32: torch.float32, I8: torch.int8, BITPACKED: torch.int32}[self.params.dst_type])
        with torch.cuda.device(x.device):   # the plan's buffers land on (and must stay on) the tensor's device
            if stream is None:
                stream = torch.cuda.current_stream(x.device).cuda_stream
            self.run_ptr(x.data_ptr(), out.data_ptr(), stream)
        return out

    def run_dual(self, x, out=None, out_bits=None, stream: int | None = None):
        """Float or int8 output AND its LceQuantize ([B,OH,OW,ceil(Cout/32)] int32: sign bits, or for an int8 plan
        bit = q < out_zero_point) in one pass."""
        import torch
        self._check_input(x)
        if self.params.dst_type == BITPACKED:
            raise ValueError("run_dual: the plan already writes bits")
        out = self._out(x, out, torch.float32 if self.params.dst_type == F32 else torch.int8)
        b, oh, ow, n = self.output_shape
        if out_bits is None:
            out_bits = torch.empty((b, oh, ow, bitpacked_size(n)), dtype=torch.int32, device=x.device)
        assert out_bits.is_cuda and out_bits.dtype == torch.int32 and out_bits.is_contiguous()
        if tuple(out_bits.shape) != (b, oh, ow, bitpacked_size(n)):
            raise ValueError(f"bit output shape {tuple(out_bits.shape)} does not match {(b, oh, ow, bitpacked_size(n))}")
        with torch.cuda.device(x.device):
            if stream is None:
                stream = torch.cuda.current_stream(x.device).cuda_stream
            check(lib().lce_hip_bconv2d_run_dual(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(out_bits.data_ptr()), C.c_void_p(stream)))
        return out, out_bits

    def run_host(self, x_np, out=None):
        """Host (NumPy) tensors through H2D | kernel | D2H; pass page-locked arrays (``host_register``) and an
        ``out`` to reuse for fully overlapped copies."""
        import numpy as np
        x = np.ascontiguousarray(x_np, np.int32)
        dt = {F32: np.float32, I8: np.int8, BITPACKED: np.int32}[self.params.dst_type]
        if out is None:
            out = np.empty(self.output_shape, dt)
        assert out.dtype == dt and out.flags.c_contiguous and tuple(out.shape) == tuple(self.output_shape)
        check(lib().lce_hip_bconv2d_run_host(self._h, _host_ptr(x), _host_ptr(out)))
        return out


class host_register:
    """``with host_register(a, b): ...`` page-locks the NumPy arrays for the duration of the block."""

    def __init__(self, *arrays):
        self.arrays = arrays

    def __enter__(self):
        self.done = []
        for a in self.arrays:
            check(lib().lce_hip_host_register(_host_ptr(a), C.c_size_t(a.nbytes)))
            self.done.append(a)
        return self

    def __exit__(self, *exc):
        for a in self.done:
            lib().lce_hip_host_unregister(_host_ptr(a))
        return False


def bitpack(x, zero_point: int = 0, out=None, stream: int | None = None):
    """LceQuantize on a CUDA tensor (float32 / int8 / bool), packing the last axis."""
    import torch
    assert x.is_cuda and x.is_contiguous()
    t = {torch.float32: F32, torch.int8: I8, torch.bool: BOOL}[x.dtype]
    cols = x.shape[-1]
    rows = x.numel() // cols if cols else 0
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (bitpacked_size(cols),), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        check(lib().lce_hip_bitpack(t, C.c_void_p(x.data_ptr()), rows, cols, int(zero_point),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out


def unpack(words, channels: int, dtype, scale: float = 1.0, zero_point: int = 0, stream: int | None = None, out=None):
    """LceDequantize on a CUDA int32 tensor."""
    import torch
    assert words.is_cuda and words.dtype == torch.int32 and words.is_contiguous()
    t = {torch.float32: F32, torch.int8: I8, torch.bool: BOOL}[dtype]
    rows = words.numel() // words.shape[-1]
    if out is None:
        out = torch.empty(tuple(words.shape[:-1]) + (channels,), dtype=dtype, device=words.device)
    assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == tuple(words.shape[:-1]) + (channels,)
    with torch.cuda.device(words.device):
        if stream is None:
            stream = torch.cuda.current_stream(words.device).cuda_stream
        check(lib().lce_hip_unpack(t, C.c_void_p(words.data_ptr()), rows, channels, float(scale),
                                   int(zero_point), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out


# ---- what the fused passes between binary layers share (elementwise, add_int8, concat, pool2d, conv1x1, depthwise_conv2d) ----
def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _check_outputs(who, out, out_bits, dtype, shape):
    """The ``out`` (a tensor to fill, None, or False) and ``out_bits`` (a tensor to fill, True, or None) of a pass that produces
    a ``dtype`` tensor of ``shape``, on shapes and dtypes only (NumPy or torch): nothing here touches a device."""
    if out is False and out_bits is None:
        raise ValueError("%s: no output requested" % who)
    want_bits = shape[:-1] + (bitpacked_size(shape[-1]),)
    for name, a, dt, want in (("out", out, dtype, shape), ("out_bits", out_bits, "int32", want_bits)):
        if a is not None and a is not False and a is not True and (tuple(a.shape) != want or _dtype_name(a) != dt):
            raise ValueError("%s: %s must be %s of shape %r, got %s %r" % (who, name, dt, want, a.dtype, tuple(a.shape)))


def _on_dev(a, dev, who, whose):
    """``a`` as a contiguous tensor on ``dev`` (a NumPy array is copied there); ``whose`` device that is, for the message."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a
    if not (t.is_cuda and t.device == dev and t.is_contiguous()):
        raise ValueError("%s: tensors must be contiguous and on %s device %s" % (who, whose, dev))
    return t


def _new_bits(lead, channels, dev):
    import torch
    return torch.empty(tuple(lead) + (bitpacked_size(channels),), dtype=torch.int32, device=dev)


def _stream_or_current(stream, dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream if stream is None else stream


def _dev_ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _results(host, out_d, bits_d, out=None, out_bits=None):
    """What a pass returns: the device tensors, or for NumPy input NumPy arrays (the caller's own where they passed some)."""
    if not host:
        return out_d, bits_d
    ret = []
    for t, mine in ((out_d, out), (bits_d, out_bits)):
        a = None if t is None else t.cpu().numpy()
        if isinstance(mine, np.ndarray) and a is not None:
            mine[...] = a
            a = mine
        ret.append(a)
    return tuple(ret)


def _ew_check(x, steps, out, out_bits):
    """Argument checks of ``elementwise`` on shapes and dtypes only (NumPy or torch): nothing here touches a device."""
    shape = tuple(x.shape)
    if _dtype_name(x) != "float32" or len(shape) < 1:
        raise ValueError("elementwise: x must be a float32 tensor with a channel axis, got %s %r" % (x.dtype, shape))
    channels = shape[-1]
    if not isinstance(steps, (list, tuple)) or not 1 <= len(steps) <= EW_MAX_STEPS:
        raise ValueError("elementwise: 1..%d steps, got %r" % (EW_MAX_STEPS, steps))
    kinds = []
    for k, step in enumerate(steps):
        if not isinstance(step, (list, tuple)) or len(step) != 3:
            raise ValueError("elementwise: step %d must be (op, operand, activation), got %r" % (k, step))
        op, operand, act = step
        if op not in (EW_ADD, EW_MUL, "add", "mul"):
            raise ValueError("elementwise: step %d: unknown op %r" % (k, op))
        if act not in (ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6):
            raise ValueError("elementwise: step %d: unknown activation %r" % (k, act))
        if operand is None:
            raise ValueError("elementwise: step %d: no operand" % k)
        if isinstance(operand, (int, float, np.floating, np.integer)):
            kinds.append(EW_SCALAR)
            continue
        oshape = tuple(operand.shape)
        if _dtype_name(operand) != "float32":
            raise ValueError("elementwise: step %d: operand must be float32, got %s" % (k, operand.dtype))
        if oshape == shape:
            kinds.append(EW_TENSOR)
        elif oshape == (channels,):
            kinds.append(EW_PER_CHANNEL)
        else:
            raise ValueError("elementwise: step %d: operand shape %r is neither x's %r nor [channels] (%d,)" % (k, oshape, shape, channels))
    _check_outputs("elementwise", out, out_bits, "float32", shape)
    return kinds


def elementwise(x, steps, out=None, out_bits=None, stream: int | None = None):
    """TFLite's float ADD / MUL chain between binary layers and the LceQuantize of its result, in one pass
    (``lce_hip_elementwise``).  ``x``: float32 [..., C] on the device (or NumPy: copied to cuda:0 and back).  ``steps``: up to 8
    ``(op, operand, activation)`` -- op ``EW_ADD`` / ``EW_MUL`` (or "add" / "mul"), operand a Python float (scalar), a [C]
    tensor (per channel) or a tensor of x's shape, activation ``ACT_*``.  ``out``: a float32 tensor to fill (may be ``x`` or a
    tensor operand), None for a new one, False for none.  ``out_bits``: an int32 [..., ceil(C/32)] tensor to fill, True for a
    new one, None for none.  Returns ``(out, out_bits)`` with None for an output not asked for."""
    kinds = _ew_check(x, steps, out, out_bits)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "elementwise", "x's")
    xd = on_dev(x)
    operands = [None if k == EW_SCALAR else on_dev(step[1]) for k, step in zip(kinds, steps)]
    channels = x.shape[-1]
    rows = xd.numel() // channels if channels else 0
    out_d = None if out is False else torch.empty_like(xd) if out is None else on_dev(out)
    bits_d = None if out_bits is None else _new_bits(xd.shape[:-1], channels, dev) if out_bits is True else on_dev(out_bits)
    arr = (EwStep * len(steps))()
    for k, ((op, operand, act), kind, t) in enumerate(zip(steps, kinds, operands)):
        arr[k].op = {EW_ADD: EW_ADD, EW_MUL: EW_MUL, "add": EW_ADD, "mul": EW_MUL}[op]
        arr[k].operand = kind
        arr[k].values = None if t is None else t.data_ptr()
        arr[k].scalar = float(operand) if kind == EW_SCALAR else 0.0
        arr[k].activation = int(act)
    with torch.cuda.device(dev):
        check(lib().lce_hip_elementwise(_dev_ptr(xd), rows, channels, arr, len(steps), _dev_ptr(out_d), _dev_ptr(bits_d),
                                        C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, out, out_bits)


_EW_EX_OPS = {EW_ADD: EW_ADD, EW_MUL: EW_MUL, EW_CLAMP: EW_CLAMP, EW_PRELU: EW_PRELU, EW_LOGISTIC: EW_LOGISTIC,
              "add": EW_ADD, "mul": EW_MUL, "clamp": EW_CLAMP, "prelu": EW_PRELU, "logistic": EW_LOGISTIC}


def _ew_ex_check(x, steps, out, out_bits):
    """Argument checks of ``elementwise_ex`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    the operand kind of every step."""
    shape = tuple(x.shape)
    if _dtype_name(x) != "float32" or len(shape) < 2:
        raise ValueError("elementwise_ex: x must be a float32 tensor [batch, ..., channels], got %s %r" % (x.dtype, shape))
    channels = shape[-1]
    per_image = (shape[0],) + (1,) * (len(shape) - 2) + (channels,)
    if not isinstance(steps, (list, tuple)) or not 1 <= len(steps) <= EW_MAX_STEPS:
        raise ValueError("elementwise_ex: 1..%d steps, got %r" % (EW_MAX_STEPS, steps))
    kinds = []
    for k, step in enumerate(steps):
        if not isinstance(step, (list, tuple)) or len(step) != 3:
            raise ValueError("elementwise_ex: step %d must be (op, operand, activation), got %r" % (k, step))
        op, operand, act = step
        if isinstance(op, (list, dict)) or op not in _EW_EX_OPS:
            raise ValueError("elementwise_ex: step %d: unknown op %r" % (k, op))
        op = _EW_EX_OPS[op]
        if act not in (ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6):
            raise ValueError("elementwise_ex: step %d: unknown activation %r" % (k, act))
        if op in (EW_PRELU, EW_LOGISTIC) and act != ACT_NONE:
            raise ValueError("elementwise_ex: step %d: PRELU and LOGISTIC take no activation" % k)
        if op in (EW_CLAMP, EW_LOGISTIC):
            if operand is not None:
                raise ValueError("elementwise_ex: step %d: CLAMP and LOGISTIC take no operand" % k)
            kinds.append(EW_SCALAR)
            continue
        if operand is None:
            raise ValueError("elementwise_ex: step %d: no operand" % k)
        if isinstance(operand, (int, float, np.floating, np.integer)):
            kinds.append(EW_SCALAR)
            continue
        oshape = tuple(operand.shape)
        if _dtype_name(operand) != "float32":
            raise ValueError("elementwise_ex: step %d: operand must be float32, got %s" % (k, operand.dtype))
        if oshape == (channels,):
            kinds.append(EW_PER_CHANNEL)
        elif op == EW_PRELU:
            raise ValueError("elementwise_ex: step %d: PRELU's alpha is a float or [channels], got shape %r" % (k, oshape))
        elif oshape == shape:
            kinds.append(EW_TENSOR)
        elif oshape == per_image:
            kinds.append(EW_PER_IMAGE_CHANNEL)
        else:
            raise ValueError("elementwise_ex: step %d: operand shape %r is neither x's %r, per image %r nor [channels] (%d,)"
                             % (k, oshape, shape, per_image, channels))
    _check_outputs("elementwise_ex", out, out_bits, "float32", shape)
    return kinds


def elementwise_ex(x, steps, out=None, out_bits=None, stream: int | None = None):
    """``elementwise`` with more kinds of step (``lce_hip_elementwise_ex``; its arithmetic: include/lce_hip.h).  ``x``: float32
    [batch, ..., C].  ``steps``: up to 8 ``(op, operand, activation)``:
    ``("add" | "mul", operand, ACT_*)`` -- the operand a float, a [C] tensor, a tensor of x's shape, or a [batch, 1, ..., 1, C]
    tensor (one value per image and channel: the gate of a squeeze-and-excite block);
    ``("clamp", None, ACT_*)`` -- a standalone RELU / RELU_N1_TO_1 / RELU6;
    ``("prelu", alpha, ACT_NONE)`` -- alpha a float or a [C] tensor;
    ``("logistic", None, ACT_NONE)``.
    ``out``, ``out_bits``, ``stream`` and the result: as ``elementwise``."""
    kinds = _ew_ex_check(x, steps, out, out_bits)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "elementwise_ex", "x's")
    xd = on_dev(x)
    operands = [None if k == EW_SCALAR else on_dev(step[1]) for k, step in zip(kinds, steps)]
    channels = x.shape[-1]
    rows = xd.numel() // channels if channels else 0
    rows_per_image = rows // x.shape[0] if x.shape[0] else 0
    out_d = None if out is False else torch.empty_like(xd) if out is None else on_dev(out)
    bits_d = None if out_bits is None else _new_bits(xd.shape[:-1], channels, dev) if out_bits is True else on_dev(out_bits)
    arr = (EwStepEx * len(steps))()
    for k, ((op, operand, act), kind, t) in enumerate(zip(steps, kinds, operands)):
        arr[k].op = _EW_EX_OPS[op]
        arr[k].operand = kind
        arr[k].values = None if t is None else t.data_ptr()
        arr[k].scalar = float(operand) if kind == EW_SCALAR and operand is not None else 0.0
        arr[k].activation = int(act)
    with torch.cuda.device(dev):
        check(lib().lce_hip_elementwise_ex(_dev_ptr(xd), rows, channels, rows_per_image, arr, len(steps), _dev_ptr(out_d), _dev_ptr(bits_d),
                                           C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, out, out_bits)


def _add_int8_desc(q1, q2, q_out, activation) -> AddInt8Desc:
    """Checks of the quantization arguments that need no library: each q is (scale, zero_point)."""
    vals = []
    for name, q in (("q1", q1), ("q2", q2), ("q_out", q_out)):
        if not isinstance(q, (list, tuple)) or len(q) != 2:
            raise ValueError("add_int8: %s must be (scale, zero_point), got %r" % (name, q))
        scale, zp = float(q[0]), q[1]
        if not (np.isfinite(scale) and scale > 0):
            raise ValueError("add_int8: %s scale must be finite and positive, got %r" % (name, q[0]))
        if int(zp) != zp or not -128 <= int(zp) <= 127:
            raise ValueError("add_int8: %s zero point must be an integer in [-128, 127], got %r" % (name, zp))
        vals += [scale, int(zp)]
    if activation not in (ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6):
        raise ValueError("add_int8: unknown activation %r" % (activation,))
    return AddInt8Desc(*vals, int(activation))


def add_int8_params(q1, q2, q_out, activation=ACT_NONE) -> dict:
    """TFLite's Prepare of the builtin int8 ADD (``lce_hip_add_int8_prepare``, host only): the nine numbers of
    ``lce_hip_add_int8_params`` as a dict, plus ``variant`` -- the kernel variant ``add_int8`` uses for these parameters
    (``ADD_INT8_*``).  Raises ``LceHipError`` for parameters TFLite's Prepare refuses (a real multiplier outside (0, 1))."""
    d = _add_int8_desc(q1, q2, q_out, activation)
    p, v = AddInt8Params(), C.c_int32()
    check(lib().lce_hip_add_int8_prepare(C.byref(d), C.byref(p)))
    check(lib().lce_hip_add_int8_variant(C.byref(d), C.byref(v)))
    out = {n: int(getattr(p, n)) for n, _ in AddInt8Params._fields_}
    out["variant"] = int(v.value)
    return out


def _add_int8_check(x1, x2, out, out_bits):
    """Argument checks of ``add_int8`` on shapes and dtypes only (NumPy or torch): nothing here touches a device."""
    shape = tuple(x1.shape)
    if _dtype_name(x1) != "int8" or len(shape) < 1:
        raise ValueError("add_int8: x1 must be an int8 tensor with a channel axis, got %s %r" % (x1.dtype, shape))
    if _dtype_name(x2) != "int8" or tuple(x2.shape) != shape:
        raise ValueError("add_int8: x2 must be int8 of x1's shape %r, got %s %r" % (shape, x2.dtype, tuple(x2.shape)))
    _check_outputs("add_int8", out, out_bits, "int8", shape)


def add_int8(x1, x2, q1, q2, q_out, activation=ACT_NONE, out=None, out_bits=None, stream: int | None = None,
             variant: int | None = None):
    """TFLite's builtin int8 ADD of two tensors -- the residual shortcut of an int8-converted network -- byte for byte, and
    the LceQuantize of the sum at the sum's zero point, in one pass (``lce_hip_add_int8``).  ``x1``, ``x2``: int8 [..., C] of
    one shape on the device (or NumPy: copied to cuda:0 and back).  ``q1``, ``q2``, ``q_out``: (scale, zero_point) of the two
    inputs and the sum.  ``out``: an int8 tensor to fill (may be ``x1`` or ``x2``), None for a new one, False for none.
    ``out_bits``: an int32 [..., ceil(C/32)] tensor to fill, True for a new one, None for none.  ``variant``: run this kernel
    variant (``ADD_INT8_*``; refused when it is not proven for the parameters) instead of the chosen one -- for tests and
    measurements.  Returns ``(out, out_bits)`` with None for an output not asked for."""
    desc = _add_int8_desc(q1, q2, q_out, activation)
    _add_int8_check(x1, x2, out, out_bits)
    if variant is not None and variant not in (ADD_INT8_LITERAL, ADD_INT8_SPLIT, ADD_INT8_SHIFT):
        raise ValueError("add_int8: unknown variant %r" % (variant,))
    import torch
    host = isinstance(x1, np.ndarray)
    dev = torch.device("cuda:0") if host else x1.device
    on_dev = lambda a: _on_dev(a, dev, "add_int8", "x1's")
    a, b = on_dev(x1), on_dev(x2)
    channels = x1.shape[-1]
    rows = a.numel() // channels if channels else 0
    out_d = None if out is False else torch.empty_like(a) if out is None else on_dev(out)
    bits_d = None if out_bits is None else _new_bits(a.shape[:-1], channels, dev) if out_bits is True else on_dev(out_bits)
    args = (_dev_ptr(a), _dev_ptr(b), rows, channels, _dev_ptr(out_d), _dev_ptr(bits_d), C.c_void_p(_stream_or_current(stream, dev)))
    with torch.cuda.device(dev):
        if variant is None:
            check(lib().lce_hip_add_int8(C.byref(desc), *args))
        else:
            check(lib().lce_hip_add_int8_forced(C.byref(desc), int(variant), *args))
    return _results(host, out_d, bits_d, out, out_bits)


def _ew_i8_q(who, name, q):
    if not isinstance(q, (list, tuple)) or len(q) != 2:
        raise ValueError("%s: %s must be (scale, zero_point), got %r" % (who, name, q))
    if int(q[1]) != q[1]:
        raise ValueError("%s: %s zero point must be an integer, got %r" % (who, name, q[1]))
    return float(q[0]), int(q[1])


def _ew_i8_desc(who, channels, q_in, steps, head):
    """``lce_hip_elementwise_i8_desc`` of a chain and the host arrays its ``values`` point into (keep them alive as long as the
    descriptor).  Shapes and kinds are checked here; the numbers are the library's to refuse."""
    channels = int(channels)
    d = EwI8Desc()
    d.channels = channels
    d.in_scale, d.in_zero_point = _ew_i8_q(who, "q_in", q_in)
    if head is not None:
        if not isinstance(head, (list, tuple)) or len(head) not in (2, 3):
            raise ValueError("%s: head must be (q_addend, q_out[, activation]), got %r" % (who, head))
        d.has_head = 1
        d.addend_scale, d.addend_zero_point = _ew_i8_q(who, "head q_addend", head[0])
        d.head_scale, d.head_zero_point = _ew_i8_q(who, "head q_out", head[1])
        d.head_activation = int(head[2]) if len(head) == 3 else ACT_NONE
    steps = list(steps)
    if len(steps) > EW_MAX_STEPS:
        raise ValueError("%s: at most %d steps, got %d" % (who, EW_MAX_STEPS, len(steps)))
    d.num_steps = len(steps)
    keep = []
    for k, st in enumerate(steps):
        name = "step %d" % (k + 1)
        if not isinstance(st, (list, tuple)) or not st or st[0] not in ("add", "prelu", "clamp", "requantize"):
            raise ValueError("%s: %s must begin with 'add', 'prelu', 'clamp' or 'requantize', got %r" % (who, name, st))
        kind = st[0]
        want = {"add": 5, "prelu": 4, "clamp": 3, "requantize": 2}[kind]
        if len(st) != want:
            raise ValueError("%s: %s (%s) takes %d fields, got %d" % (who, name, kind, want, len(st)))
        e = d.steps[k]
        e.op = {"add": EW_I8_ADD, "prelu": EW_I8_PRELU, "clamp": EW_I8_CLAMP, "requantize": EW_I8_REQUANTIZE}[kind]
        if kind in ("add", "prelu"):
            v = np.asarray(st[1])
            if v.dtype != np.int8 and not (v.dtype.kind in "iu" and v.size and -128 <= int(v.min()) and int(v.max()) <= 127):
                raise ValueError("%s: %s operand must hold int8 values, got %s" % (who, name, v.dtype))
            v = np.ascontiguousarray(v.astype(np.int8).reshape(-1))
            if v.size == 1 and np.ndim(st[1]) == 0:
                e.operand = EW_SCALAR
            elif v.size == channels:
                e.operand = EW_PER_CHANNEL
            else:
                raise ValueError("%s: %s operand must be a scalar or %d values, got shape %r" % (who, name, channels, np.shape(st[1])))
            keep.append(v)
            e.values = v.ctypes.data
            e.operand_scale, e.operand_zero_point = _ew_i8_q(who, name + " operand quantization", st[2])
            e.out_scale, e.out_zero_point = _ew_i8_q(who, name + " q_out", st[3])
            e.activation = int(st[4]) if kind == "add" else ACT_NONE
        else:
            e.out_scale, e.out_zero_point = _ew_i8_q(who, name + " q_out", st[1])
            e.activation = int(st[2]) if kind == "clamp" else ACT_NONE
    return d, keep


def elementwise_i8_prepare(channels, q_in, steps, head=None):
    """The table of one int8 elementwise chain (``lce_hip_elementwise_i8_prepare``, host only): uint8 NumPy [R, 256] with
    R = ``channels``, or R = 1 when no step has a per-channel operand; ``table[c, v + 128]`` is the chain's int8 result, as a byte,
    for the value v in channel c.  ``q_in``: (scale, zero_point) of the input.  ``steps``: 1..8 of
    ``("add", values, q_operand, q_out, act)``, ``("prelu", alpha, q_alpha, q_out)``, ``("clamp", q_out, act)`` and
    ``("requantize", q_out)`` -- ``values`` / ``alpha`` a Python or NumPy scalar (SCALAR) or ``channels`` int8 values (PER_CHANNEL),
    every q a (scale, zero_point), ``act`` an ``ACT_*``; each step's ``q_out`` is the next step's input quantization.  ``head``:
    None, or ``(q_addend, q_out[, act])`` of a tensor + tensor ADD in front of the steps (``add_int8``'s arithmetic), whose sum the
    steps then take.  TFLite's integer arithmetic, byte for byte (include/lce_hip.h).  Raises ``LceHipError`` naming the step the
    library refuses."""
    d, keep = _ew_i8_desc("elementwise_i8_prepare", channels, q_in, steps, head)
    n = C.c_size_t()
    check(lib().lce_hip_elementwise_i8_table_size(C.byref(d), C.byref(n)))
    table = np.zeros((n.value // 256, 256), np.uint8)
    check(lib().lce_hip_elementwise_i8_prepare(C.byref(d), _host_ptr(table)))
    del keep
    return table


def _ew_i8_check(x, table, addend, head, out, out_bits):
    """Argument checks of ``elementwise_i8`` on shapes and dtypes only (NumPy or torch): nothing here touches a device."""
    who = "elementwise_i8"
    shape = tuple(x.shape)
    if _dtype_name(x) != "int8" or len(shape) < 1:
        raise ValueError("%s: x must be an int8 tensor with a channel axis, got %s %r" % (who, x.dtype, shape))
    if (addend is None) != (head is None):
        raise ValueError("%s: addend and head come together" % who)
    if addend is not None and (_dtype_name(addend) != "int8" or tuple(addend.shape) != shape):
        raise ValueError("%s: addend must be int8 of x's shape %r, got %s %r" % (who, shape, addend.dtype, tuple(addend.shape)))
    if _dtype_name(table) != "uint8" or len(table.shape) != 2 or table.shape[1] != 256 or table.shape[0] not in (1, shape[-1]):
        raise ValueError("%s: table must be uint8 [1 or %d, 256] (elementwise_i8_prepare), got %s %r" % (who, shape[-1], table.dtype,
                                                                                                       tuple(table.shape)))
    _check_outputs(who, out, out_bits, "int8", shape)


def elementwise_i8(x, table, q_in, steps, addend=None, head=None, out=None, out_bits=None, stream: int | None = None,
                   path: int | None = None, report_launch: bool = False):
    """One int8 elementwise chain between binary layers -- the tail of an int8 ReActNet block (residual ADD, per-channel shift,
    PRELU, shift), a standalone RELU, an int8 requantize -- and the LceQuantize of its result at the last step's zero point, in one
    launch (``lce_hip_elementwise_i8``).  ``x``: int8 [..., C] on the device (or NumPy: copied to cuda:0 and back).  ``table``:
    ``elementwise_i8_prepare``'s for the same ``channels``, ``q_in``, ``steps`` and ``head`` (NumPy or on the device).
    ``addend`` with ``head``: the second tensor of a head ADD.  ``out``: an int8 tensor to fill (may be ``x`` or ``addend``), None
    for a new one, False for none.  ``out_bits``: an int32 [..., ceil(C/32)] tensor to fill, True for a new one, None for none.
    ``path``: None for the entry's choice, or an ``EW_I8_PATH_*`` to force (for tests and measurements; the bytes are the same).
    Returns ``(out, out_bits)``, and with ``report_launch`` a third value: the ``lce_hip_elementwise_i8_launch`` of the call as a
    dict."""
    import torch
    who = "elementwise_i8"
    _ew_i8_check(x, table, addend, head, out, out_bits)
    d, keep = _ew_i8_desc(who, x.shape[-1], q_in, steps, head)
    if path not in (None, EW_I8_PATH_LDS, EW_I8_PATH_GLOBAL, EW_I8_PATH_ONE_ROW):
        raise ValueError("%s: unknown path %r" % (who, path))
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    a = on_dev(x)
    b = None if addend is None else on_dev(addend)
    t = on_dev(table)
    channels = x.shape[-1]
    rows = a.numel() // channels if channels else 0
    out_d = None if out is False else torch.empty_like(a) if out is None else on_dev(out)
    bits_d = None if out_bits is None else _new_bits(a.shape[:-1], channels, dev) if out_bits is True else on_dev(out_bits)
    launch = EwI8Launch()
    with torch.cuda.device(dev):
        st = C.c_void_p(_stream_or_current(stream, dev))
        if report_launch and rows and channels:
            check(lib().lce_hip_elementwise_i8_path(C.byref(d), rows, _dev_ptr(a), _dev_ptr(b), _dev_ptr(t), _dev_ptr(out_d), _dev_ptr(bits_d),
                                                    -1 if path is None else int(path), C.byref(launch)))
        if path is None:
            check(lib().lce_hip_elementwise_i8(C.byref(d), _dev_ptr(a), _dev_ptr(b), _dev_ptr(t), rows, _dev_ptr(out_d), _dev_ptr(bits_d), st))
        else:
            check(lib().lce_hip_elementwise_i8_forced(C.byref(d), int(path), _dev_ptr(a), _dev_ptr(b), _dev_ptr(t), rows, _dev_ptr(out_d),
                                                      _dev_ptr(bits_d), st))
    del keep
    res = _results(host, out_d, bits_d, out, out_bits)
    return (*res, {n: int(getattr(launch, n)) for n, _ in EwI8Launch._fields_}) if report_launch else res


LOGISTIC_I8_OUT = (1.0 / 256.0, -128)                   # the output quantization TFLite fixes for an int8 LOGISTIC


def _mul_int8_desc(who, q_x, q_operand, q_out, act, per_image, add) -> MulInt8Desc:
    """``lce_hip_mul_int8_desc``; shapes and kinds are checked here, the numbers are the library's to refuse."""
    d = MulInt8Desc()
    d.in1_scale, d.in1_zero_point = _ew_i8_q(who, "q_x", q_x)
    d.in2_scale, d.in2_zero_point = _ew_i8_q(who, "q_operand", q_operand)
    d.out_scale, d.out_zero_point = _ew_i8_q(who, "q_out", q_out)
    d.activation = int(act)
    d.operand = EW_PER_IMAGE_CHANNEL if per_image else EW_TENSOR
    if add is not None:
        if not isinstance(add, (list, tuple)) or len(add) not in (2, 3):
            raise ValueError("%s: add must be (q_addend, q_out[, activation]), got %r" % (who, add))
        d.has_add = 1
        d.addend_scale, d.addend_zero_point = _ew_i8_q(who, "add q_addend", add[0])
        d.add_scale, d.add_zero_point = _ew_i8_q(who, "add q_out", add[1])
        d.add_activation = int(add[2]) if len(add) == 3 else ACT_NONE
    return d


def mul_int8_params(q_x, q_operand, q_out, act=ACT_NONE, add=None) -> dict:
    """Prepare of the builtin int8 MUL (``lce_hip_mul_int8_prepare``, host only): ``multiplier``, ``shift``, ``act_min``,
    ``act_max`` and, with ``add = (q_addend, q_out[, act])`` -- a residual ADD behind the MUL -- under ``"add"`` the dict
    ``add_int8_params`` gives for (the product, the addend).  Raises ``LceHipError`` for what the library refuses."""
    d = _mul_int8_desc("mul_int8_params", q_x, q_operand, q_out, act, False, add)
    p = MulInt8Params()
    check(lib().lce_hip_mul_int8_prepare(C.byref(d), C.byref(p)))
    out = {n: int(getattr(p, n)) for n in ("multiplier", "shift", "act_min", "act_max")}
    if add is not None:
        out["add"] = add_int8_params(q_out, add[0], add[1], add[2] if len(add) == 3 else ACT_NONE)
    return out


def _mul_int8_check(x, operand, per_image, rows_per_image, addend, add, out, out_bits):
    """Argument checks of ``mul_int8`` on shapes and dtypes only (NumPy or torch): nothing here touches a device."""
    who = "mul_int8"
    shape = tuple(x.shape)
    if _dtype_name(x) != "int8" or len(shape) < 1:
        raise ValueError("%s: x must be an int8 tensor with a channel axis, got %s %r" % (who, x.dtype, shape))
    if _dtype_name(operand) != "int8":
        raise ValueError("%s: operand must be int8, got %s" % (who, operand.dtype))
    if per_image:
        if len(operand.shape) < 1 or operand.shape[-1] != shape[-1]:
            raise ValueError("%s: a per-image operand must be int8 [..., %d], got %r" % (who, shape[-1], tuple(operand.shape)))
    elif tuple(operand.shape) != shape:
        raise ValueError("%s: operand must be int8 of x's shape %r, got %r" % (who, shape, tuple(operand.shape)))
    if (addend is None) != (add is None):
        raise ValueError("%s: addend and add come together" % who)
    if addend is not None and (_dtype_name(addend) != "int8" or tuple(addend.shape) != shape):
        raise ValueError("%s: addend must be int8 of x's shape %r, got %s %r" % (who, shape, addend.dtype, tuple(addend.shape)))
    if int(rows_per_image) != rows_per_image or rows_per_image < 0:
        raise ValueError("%s: rows_per_image must be a non-negative integer, got %r" % (who, rows_per_image))
    _check_outputs(who, out, out_bits, "int8", shape)


def mul_int8(x, operand, q_x, q_operand, q_out, act=ACT_NONE, per_image=False, rows_per_image=0, addend=None, add=None, out=None,
             out_bits=None, stream: int | None = None, report_launch: bool = False):
    """TFLite's builtin int8 MUL -- the gate of a squeeze-and-excite block in an int8-converted network -- byte for byte, the
    residual ADD behind it and the LceQuantize of the result, in one launch (``lce_hip_mul_int8``).  ``x``: int8 [..., C] on the
    device (or NumPy: copied to cuda:0 and back).  ``operand``: int8 of ``x``'s shape, or with ``per_image`` the gate
    [rows / rows_per_image, C] (any leading shape with that many elements), ``rows_per_image`` = H * W.  ``q_x``, ``q_operand``,
    ``q_out``: (scale, zero_point) of the inputs and the product; ``act``: the MUL's ``ACT_*``.  ``addend`` with
    ``add = (q_addend, q_out[, act])``: the tensor ``add_int8`` then adds to the product.  ``out``: an int8 tensor to fill (may be
    ``x`` or ``addend``), None for a new one, False for none.  ``out_bits``: an int32 [..., ceil(C/32)] tensor to fill, True for a
    new one, None for none; the bits are taken at the last stage's zero point.  Returns ``(out, out_bits)``, and with
    ``report_launch`` a third value: the ``lce_hip_mul_int8_launch`` of the call as a dict."""
    import torch
    who = "mul_int8"
    _mul_int8_check(x, operand, per_image, rows_per_image, addend, add, out, out_bits)
    d = _mul_int8_desc(who, q_x, q_operand, q_out, act, per_image, add)
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    a, g = on_dev(x), on_dev(operand)
    b = None if addend is None else on_dev(addend)
    channels = x.shape[-1]
    rows = a.numel() // channels if channels else 0
    out_d = None if out is False else torch.empty_like(a) if out is None else on_dev(out)
    bits_d = None if out_bits is None else _new_bits(a.shape[:-1], channels, dev) if out_bits is True else on_dev(out_bits)
    if per_image and rows_per_image and rows % int(rows_per_image) == 0 and g.numel() != rows // int(rows_per_image) * channels:
        raise ValueError("%s: a per-image operand holds %d values, got %d" % (who, rows // int(rows_per_image) * channels, g.numel()))
    launch = MulInt8Launch()
    with torch.cuda.device(dev):
        if report_launch and rows and channels:
            check(lib().lce_hip_mul_int8_path(C.byref(d), rows, channels, int(rows_per_image), _dev_ptr(a), _dev_ptr(g), _dev_ptr(b),
                                              _dev_ptr(out_d), _dev_ptr(bits_d), C.byref(launch)))
        check(lib().lce_hip_mul_int8(C.byref(d), _dev_ptr(a), _dev_ptr(g), _dev_ptr(b), rows, channels, int(rows_per_image),
                                     _dev_ptr(out_d), _dev_ptr(bits_d), C.c_void_p(_stream_or_current(stream, dev))))
    res = _results(host, out_d, bits_d, out, out_bits)
    return (*res, {n: int(getattr(launch, n)) for n, t in MulInt8Launch._fields_ if t is C.c_int32}) if report_launch else res


def logistic_int8_table(q_in, q_out=LOGISTIC_I8_OUT):
    """The table of TFLite's builtin int8 LOGISTIC (``lce_hip_logistic_int8_prepare``, host only): uint8 NumPy [256];
    ``table[v + 128]`` is the int8 result, as a byte, for the input value v at ``q_in`` = (scale, zero_point).  The output
    quantization is fixed at (1/256, -128); any other ``q_out`` is refused."""
    si, zi = _ew_i8_q("logistic_int8_table", "q_in", q_in)
    so, zo = _ew_i8_q("logistic_int8_table", "q_out", q_out)
    table = np.zeros(256, np.uint8)
    check(lib().lce_hip_logistic_int8_prepare(si, zi, so, zo, _host_ptr(table)))
    return table


def logistic_int8(x, q_in, out=None, out_bits=None, stream: int | None = None, table=None):
    """TFLite's builtin int8 LOGISTIC of ``x`` (int8 [..., C] on the device, or NumPy: copied to cuda:0 and back) at ``q_in`` =
    (scale, zero_point), as one table look-up per element (``lce_hip_logistic_int8``); the result is at (1/256, -128).  ``table``:
    ``logistic_int8_table(q_in)`` (NumPy or on the device) when the caller keeps it; computed and uploaded here otherwise.
    ``out`` / ``out_bits`` as ``mul_int8``'s (bit = value < -128: every bit is 0).  Returns ``(out, out_bits)``."""
    import torch
    who = "logistic_int8"
    shape = tuple(x.shape)
    if _dtype_name(x) != "int8" or len(shape) < 1:
        raise ValueError("%s: x must be an int8 tensor with a channel axis, got %s %r" % (who, x.dtype, shape))
    _check_outputs(who, out, out_bits, "int8", shape)
    if table is None:
        table = logistic_int8_table(q_in)
    if _dtype_name(table) != "uint8" or tuple(table.shape) != (256,):
        raise ValueError("%s: table must be uint8 [256] (logistic_int8_table), got %s %r" % (who, table.dtype, tuple(table.shape)))
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    a, t = on_dev(x), on_dev(table)
    channels = x.shape[-1]
    rows = a.numel() // channels if channels else 0
    out_d = None if out is False else torch.empty_like(a) if out is None else on_dev(out)
    bits_d = None if out_bits is None else _new_bits(a.shape[:-1], channels, dev) if out_bits is True else on_dev(out_bits)
    with torch.cuda.device(dev):
        check(lib().lce_hip_logistic_int8(_dev_ptr(t), _dev_ptr(a), rows, channels, _dev_ptr(out_d), _dev_ptr(bits_d),
                                          C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, out, out_bits)


def _concat_check(tensors, out, out_bits, zero_point):
    """Argument checks of ``concat`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (lce_hip_dtype, leading shape, channels per input)."""
    tensors = list(tensors)
    if not 2 <= len(tensors) <= CONCAT_MAX_INPUTS:
        raise ValueError("concat: 2..%d tensors, got %d" % (CONCAT_MAX_INPUTS, len(tensors)))
    name = _dtype_name(tensors[0])
    kinds = {"float32": F32, "int8": I8, "int32": BITPACKED}
    if name not in kinds:
        raise ValueError("concat: tensors must be float32, int8 or int32 (bitpacked), got %s" % name)
    lead = tuple(tensors[0].shape[:-1])
    for k, t in enumerate(tensors):
        if _dtype_name(t) != name or len(t.shape) < 1 or tuple(t.shape[:-1]) != lead or t.shape[-1] < 1:
            raise ValueError("concat: tensor %d must be %s of shape %r + (C,), got %s %r" % (k, name, lead, _dtype_name(t), tuple(t.shape)))
    channels = [int(t.shape[-1]) for t in tensors]
    kind = kinds[name]
    if out_bits and kind == BITPACKED:
        raise ValueError("concat: a bitpacked join has no bit output")
    zp = int(zero_point)
    if (kind == I8 and not -128 <= zp <= 127) or (kind != I8 and zp != 0):
        raise ValueError("concat: zero point %r (int8: -128..127; otherwise 0)" % (zero_point,))
    _check_outputs("concat", out, True if out_bits else None, name, lead + (sum(channels),))
    return kind, lead, channels


def concat(tensors, out=None, out_bits=False, zero_point: int = 0, stream: int | None = None):
    """The channel join of a dense block -- TFLite's builtin CONCATENATION on the last axis -- and the LceQuantize of the
    joined tensor, in one pass (``lce_hip_concat``).  ``tensors``: 2..8 tensors [..., C_k] of one dtype (float32, int8, or
    int32 holding bitpacked words) and one leading shape, contiguous on one device (or NumPy: copied to cuda:0 and back);
    one may appear twice.  ``out``: a tensor [..., sum C_k] to fill (it must not overlap an input), None for a new one, False
    for none.  ``out_bits``: True for the int32 [..., ceil(sum C_k / 32)] bits of the joined tensor (float32: value < 0; int8:
    value < ``zero_point``).  Returns ``(joined or None, bits or None)``."""
    tensors = list(tensors)
    kind, lead, channels = _concat_check(tensors, out, out_bits, zero_point)
    import torch
    host = isinstance(tensors[0], np.ndarray)
    dev = torch.device("cuda:0") if host else tensors[0].device
    on_dev = lambda a: _on_dev(a, dev, "concat", "the first tensor's")
    ins = [on_dev(t) for t in tensors]
    total = sum(channels)
    rows = ins[0].numel() // channels[0]
    out_d = None if out is False else torch.empty(lead + (total,), dtype=ins[0].dtype, device=dev) if out is None else on_dev(out)
    bits_d = _new_bits(lead, total, dev) if out_bits else None
    ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    ch = (C.c_int32 * len(ins))(*channels)
    with torch.cuda.device(dev):
        check(lib().lce_hip_concat(kind, ptrs, ch, len(ins), rows, int(zero_point), _dev_ptr(out_d), _dev_ptr(bits_d),
                                   C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, out)


class Window(C.Structure):
    """``lce_hip_window``."""
    _fields_ = [("data_dev", C.c_void_p), ("pitch", C.c_int32), ("begin", C.c_int32), ("count", C.c_int32),
                ("addend_dev", C.c_void_p), ("reserved", C.c_int32 * 2)]


def _join_check(windows, out, out_bits, zero_point):
    """Argument checks of ``join_windows`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (lce_hip_dtype, leading shape, [(tensor, begin, count, addend or None)])."""
    windows = [tuple(w) for w in windows]
    if not 1 <= len(windows) <= JOIN_MAX_WINDOWS:
        raise ValueError("join_windows: 1..%d windows, got %d" % (JOIN_MAX_WINDOWS, len(windows)))
    if any(len(w) not in (3, 4) for w in windows):
        raise ValueError("join_windows: a window is (tensor, begin, count) or (tensor, begin, count, addend)")
    windows = [w if len(w) == 4 else w + (None,) for w in windows]
    name = _dtype_name(windows[0][0])
    kinds = {"float32": F32, "int8": I8}
    if name not in kinds:
        raise ValueError("join_windows: tensors must be float32 or int8, got %s" % name)
    lead = tuple(windows[0][0].shape[:-1])
    for k, (t, begin, count, addend) in enumerate(windows):
        if _dtype_name(t) != name or len(t.shape) < 1 or tuple(t.shape[:-1]) != lead:
            raise ValueError("join_windows: tensor %d must be %s of shape %r + (C,), got %s %r" % (k, name, lead, _dtype_name(t), tuple(t.shape)))
        if not (isinstance(begin, (int, np.integer)) and isinstance(count, (int, np.integer)) and 0 <= begin and 1 <= count and
                begin + count <= t.shape[-1]):
            raise ValueError("join_windows: window %d: [%r, %r + %r) is no window of %d channels" % (k, begin, begin, count, t.shape[-1]))
        if addend is not None:
            if name != "float32":
                raise ValueError("join_windows: window %d: only a float32 window takes an addend" % k)
            if _dtype_name(addend) != "float32" or tuple(addend.shape) != lead + (int(count),):
                raise ValueError("join_windows: window %d: the addend must be float32 of shape %r, got %s %r" %
                                 (k, lead + (int(count),), _dtype_name(addend), tuple(addend.shape)))
    zp = int(zero_point)
    if (name == "int8" and not -128 <= zp <= 127) or (name != "int8" and zp != 0):
        raise ValueError("join_windows: zero point %r (int8: -128..127; float32: 0)" % (zero_point,))
    total = sum(int(w[2]) for w in windows)
    _check_outputs("join_windows", out, True if out_bits else None, name, lead + (total,))
    return kinds[name], lead, windows


def join_windows(windows, out=None, out_bits=False, zero_point: int = 0, stream: int | None = None):
    """The join of channel windows (``lce_hip_join_windows``): ``concat`` with every source a channel range of a wider tensor.
    ``windows``: 1..8 of ``(tensor, begin, count)`` or ``(tensor, begin, count, addend)`` -- the channels [begin, begin + count)
    of a tensor [..., C_k]; all tensors of one dtype (float32 or int8) and one leading shape, contiguous on one device (or NumPy:
    copied to cuda:0 and back); a tensor may appear in several windows, and these may overlap.  ``addend`` (float32 only): a
    dense [..., count] tensor added to the window (one float32 add); a window without one is a copy, bit for bit.  MeliusNet's
    improvement block is ``join_windows([(x, 0, C - 64), (x, C - 64, 64, w)])``.  ``out``: a tensor [..., sum count] to fill (it
    must not overlap a source or an addend), None for a new one, False for none.  ``out_bits``: True for the int32
    [..., ceil(sum count / 32)] bits of the joined tensor (float32: value < 0; int8: value < ``zero_point``).  Returns
    ``(joined or None, bits or None)``."""
    kind, lead, windows = _join_check(windows, out, out_bits, zero_point)
    import torch
    host = isinstance(windows[0][0], np.ndarray)
    dev = torch.device("cuda:0") if host else windows[0][0].device
    on_dev = lambda a: _on_dev(a, dev, "join_windows", "the first tensor's")
    placed = {}                                           # (a NumPy source that appears twice is copied once)
    def once(a):
        if id(a) not in placed:
            placed[id(a)] = on_dev(a)
        return placed[id(a)]
    arr = (Window * len(windows))()
    keep = []
    for k, (t, begin, count, addend) in enumerate(windows):
        td, ad = once(t), None if addend is None else once(addend)
        keep += [td, ad]
        arr[k].data_dev, arr[k].pitch, arr[k].begin, arr[k].count = td.data_ptr(), int(t.shape[-1]), int(begin), int(count)
        arr[k].addend_dev = None if ad is None else ad.data_ptr()
    first = keep[0]
    total = sum(int(w[2]) for w in windows)
    rows = first.numel() // first.shape[-1]
    out_d = None if out is False else torch.empty(lead + (total,), dtype=first.dtype, device=dev) if out is None else on_dev(out)
    bits_d = _new_bits(lead, total, dev) if out_bits else None
    with torch.cuda.device(dev):
        check(lib().lce_hip_join_windows(kind, arr, len(windows), rows, int(zero_point), _dev_ptr(out_d), _dev_ptr(bits_d),
                                         C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, out)


def channel_slice(x, begin: int, count: int, out=None, out_bits=False, zero_point: int = 0, stream: int | None = None):
    """The channels [begin, begin + count) of ``x`` [..., C] (TFLite's STRIDED_SLICE / SLICE on the last axis) and their
    LceQuantize, in one pass: the one-window ``join_windows``."""
    return join_windows([(x, begin, count)], out=out, out_bits=out_bits, zero_point=zero_point, stream=stream)


def _pair(who, name, v):
    """An (height, width) argument: one int for both, or two."""
    hw = (v, v) if isinstance(v, (int, np.integer)) else tuple(v) if isinstance(v, (list, tuple)) else None
    if hw is None or len(hw) != 2 or any(not isinstance(a, (int, np.integer)) or a <= 0 for a in hw):
        raise ValueError("%s: %s must be a positive int or a pair of them, got %r" % (who, name, v))
    return int(hw[0]), int(hw[1])


def pool2d_output_hw(in_hw, filter, stride, padding):
    """Output (height, width) of a pool: SAME ceil(in / stride), VALID ceil((in - filter + 1) / stride) (host only)."""
    return tuple((i + s - 1) // s if padding == PADDING_SAME else (i + s - f) // s for i, f, s in zip(in_hw, filter, stride))


def _nhwc_check(who, x, dtypes):
    """``x`` is a non-empty NHWC tensor of one of ``dtypes``: its dtype's name and its four extents."""
    name = _dtype_name(x)
    if name not in dtypes or len(x.shape) != 4 or min(x.shape) < 1:
        raise ValueError("%s: x must be a non-empty %s NHWC tensor, got %s %r" % (who, " or ".join(dtypes), x.dtype, tuple(x.shape)))
    return (name,) + tuple(int(v) for v in x.shape)


def _padding_activation_check(who, padding, activation):
    """``padding`` (None: the pass has none) and ``activation`` are known values."""
    if padding is not None and padding not in (PADDING_SAME, PADDING_VALID):
        raise ValueError("%s: padding must be PADDING_SAME or PADDING_VALID, got %r" % (who, padding))
    if activation not in (ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6):
        raise ValueError("%s: unknown activation %r" % (who, activation))


def _window_output_hw(who, in_hw, filter, stride, padding):
    """``pool2d_output_hw``, which must not be empty."""
    oh, ow = pool2d_output_hw(in_hw, filter, stride, padding)
    if oh < 1 or ow < 1:
        raise ValueError("%s: empty output (a VALID filter of %d x %d on an image of %d x %d)" % ((who,) + tuple(filter) + tuple(in_hw)))
    return oh, ow


def _float_conv_check(who, x, filter_of, bias, stride, padding, activation, out, out_bits):
    """The argument checks the float convolutions share, in their order: ``x`` float32 NHWC and non-empty; the pass's own
    ``filter_of(cin)``, which checks the filter and returns (Cout, fh, fw); ``bias`` float32 [Cout] or None; ``stride``;
    ``padding`` (None: a 1x1 filter has none, the extent is ceil(in / stride)) and ``activation``; an output that is not empty;
    ``out`` and ``out_bits``.  Returns (b, h, w, cin, cout, fh, fw, sh, sw) and the output shape."""
    _, b, h, w, cin = _nhwc_check(who, x, ("float32",))
    cout, fh, fw = filter_of(cin)
    if bias is not None and (_dtype_name(bias) != "float32" or tuple(bias.shape) != (cout,)):
        raise ValueError("%s: bias must be float32 [%d], got %s %r" % (who, cout, bias.dtype, tuple(bias.shape)))
    sh, sw = _pair(who, "stride", stride)
    _padding_activation_check(who, padding, activation)
    oh, ow = _window_output_hw(who, (h, w), (fh, fw), (sh, sw), PADDING_SAME if padding is None else padding)
    shape = (b, oh, ow, cout)
    _check_outputs(who, None if out is True else out, None if out_bits is False else out_bits, "float32", shape)
    return (b, h, w, cin, cout, fh, fw, sh, sw), shape


def _run_windowed(who, entry, desc, shape, x, constants, out, out_bits, stream, fresh=(True, None)):
    """The run the windowed passes share: ``x`` and the ``constants`` behind it (filter and bias; None for an absent one) on
    x's device (NumPy: cuda:0); ``out`` -- one of ``fresh`` for a new tensor of ``shape``, False for none, else the caller's --
    and ``out_bits`` -- True for new bits, False or None for none, else the caller's; the library's ``entry`` on ``stream``."""
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    xd = on_dev(x)
    operands = [None if c is None else on_dev(c) for c in constants]
    out_d = None if out is False else torch.empty(shape, dtype=xd.dtype, device=dev) if any(out is f for f in fresh) else on_dev(out)
    bits_d = None if (out_bits is False or out_bits is None) else _new_bits(shape[:-1], shape[-1], dev) if out_bits is True else on_dev(out_bits)
    with torch.cuda.device(dev):
        check(getattr(lib(), entry)(C.byref(desc), _dev_ptr(xd), *[_dev_ptr(t) for t in operands], _dev_ptr(out_d), _dev_ptr(bits_d),
                                    C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, None if out is True else out, None if out_bits is True else out_bits)


def _pool2d_check(x, op, filter, stride, padding, activation, out, out_bits, scale, zero_point):
    """Argument checks of ``pool2d`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (Pool2dDesc, output shape)."""
    ops = {POOL_MAX: POOL_MAX, POOL_AVERAGE: POOL_AVERAGE, "max": POOL_MAX, "average": POOL_AVERAGE}
    if op not in ops:
        raise ValueError("pool2d: unknown op %r" % (op,))
    name, b, h, w, c = _nhwc_check("pool2d", x, ("float32", "int8"))
    fh, fw = _pair("pool2d", "filter", filter)
    sh, sw = _pair("pool2d", "stride", stride)
    if fh * fw > POOL_MAX_TAPS:
        raise ValueError("pool2d: a filter of %d x %d has more than %d taps" % (fh, fw, POOL_MAX_TAPS))
    _padding_activation_check("pool2d", padding, activation)
    if name == "int8":
        if scale is None or not (np.isfinite(float(scale)) and float(scale) > 0):
            raise ValueError("pool2d: an int8 tensor needs a finite positive scale, got %r" % (scale,))
        if int(zero_point) != zero_point or not -128 <= int(zero_point) <= 127:
            raise ValueError("pool2d: zero point must be an integer in [-128, 127], got %r" % (zero_point,))
    elif zero_point != 0:
        raise ValueError("pool2d: a float32 tensor has no zero point, got %r" % (zero_point,))
    oh, ow = _window_output_hw("pool2d", (h, w), (fh, fw), (sh, sw), padding)
    shape = (b, oh, ow, c)
    _check_outputs("pool2d", None if out is True else out, None if out_bits is False else out_bits, name, shape)
    desc = Pool2dDesc(ops[op], F32 if name == "float32" else I8, b, h, w, c, fh, fw, sh, sw, int(padding), int(activation),
                      float(scale) if name == "int8" else 1.0, int(zero_point))
    return desc, shape


def pool2d(x, op, filter, stride, padding, activation=ACT_NONE, out=True, out_bits=False, scale=None, zero_point: int = 0,
           stream: int | None = None):
    """TFLite's builtin MAX_POOL_2D / AVERAGE_POOL_2D between binary layers and the LceQuantize of the pooled tensor, in one
    pass (``lce_hip_pool2d``).  ``x``: float32 or int8 NHWC on the device (or NumPy: copied to cuda:0 and back).  ``op``:
    ``POOL_MAX`` / ``POOL_AVERAGE`` (or "max" / "average").  ``filter``, ``stride``: an int or (height, width).  ``padding``:
    ``PADDING_SAME`` / ``PADDING_VALID`` (taps in the padding are excluded).  ``activation``: ``ACT_*``.  int8: ``scale`` and
    ``zero_point`` of the tensor (the output keeps them).  ``out``: True for a new pooled tensor, a tensor to fill (it must not
    overlap ``x``), False for none.  ``out_bits``: True for new int32 [B, OH, OW, ceil(C/32)] bits (float32: value < 0; int8:
    value < ``zero_point``), a tensor to fill, False for none.  Returns ``(pooled or None, bits or None)``."""
    desc, shape = _pool2d_check(x, op, filter, stride, padding, activation, out, out_bits, scale, zero_point)
    return _run_windowed("pool2d", "lce_hip_pool2d", desc, shape, x, (), out, out_bits, stream)


def _conv1x1_check(x, w, bias, stride, activation, out, out_bits):
    """Argument checks of ``conv1x1`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (Conv1x1Desc, output shape)."""
    def filter_of(cin):
        ws = tuple(int(v) for v in w.shape)
        if _dtype_name(w) != "float32" or len(ws) not in (2, 4) or ws not in ((ws[0], cin), (ws[0], 1, 1, cin)) or ws[0] < 1:
            raise ValueError("conv1x1: w must be float32 [Cout, %d] or [Cout, 1, 1, %d], got %s %r" % (cin, cin, w.dtype, ws))
        return ws[0], 1, 1
    (b, h, wd, cin, cout, _, _, sh, sw), shape = _float_conv_check("conv1x1", x, filter_of, bias, stride, None, activation, out, out_bits)
    return Conv1x1Desc(b, h, wd, cin, cout, sh, sw, int(activation)), shape


def conv1x1(x, w, bias=None, stride=1, activation=ACT_NONE, out=None, out_bits=False, stream: int | None = None):
    """TFLite's builtin float CONV_2D with a 1x1 filter between binary layers (the convolution of a transition block or a
    downsampling shortcut) and the LceQuantize of its result, in one pass (``lce_hip_conv1x1_f32``).  ``x``: float32 NHWC on
    the device (or NumPy: copied to cuda:0 and back).  ``w``: float32 [Cout, Cin] or [Cout, 1, 1, Cin].  ``bias``: float32
    [Cout] or None.  ``stride``: an int or (height, width); the output extent is ceil(in / stride).  ``activation``: ``ACT_*``.
    Per output element t = fmaf(x[c], w[o][c], t) over c in order from +0.0, then + bias, then the clamp: exact bytes
    (include/lce_hip.h).  ``out``: None for a new tensor, a tensor to fill (it must not overlap an operand), False for none.
    ``out_bits``: True for new int32 [B, OH, OW, ceil(Cout/32)] bits (value < 0), a tensor to fill, False for none.  Returns
    ``(out or None, bits or None)``."""
    desc, shape = _conv1x1_check(x, w, bias, stride, activation, out, out_bits)
    return _run_windowed("conv1x1", "lce_hip_conv1x1_f32", desc, shape, x, (w, bias), out, out_bits, stream, fresh=(None,))


def _depthwise_check(x, filter, bias, stride, padding, depth_multiplier, activation, out, out_bits):
    """Argument checks of ``depthwise_conv2d`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.
    Returns (DepthwiseDesc, output shape)."""
    who = "depthwise_conv2d"
    def filter_of(cin):
        if not isinstance(depth_multiplier, (int, np.integer)) or depth_multiplier < 1:
            raise ValueError("%s: depth_multiplier must be a positive int, got %r" % (who, depth_multiplier))
        cout = cin * int(depth_multiplier)
        fs = tuple(int(v) for v in filter.shape)
        if _dtype_name(filter) != "float32" or len(fs) not in (3, 4) or fs[-1] != cout or min(fs) < 1 or (len(fs) == 4 and fs[0] != 1):
            raise ValueError("%s: filter must be float32 [1, fh, fw, %d] or [fh, fw, %d], got %s %r" % (who, cout, cout, filter.dtype, fs))
        if fs[-3] * fs[-2] * cout >= 1 << 31:
            raise ValueError("%s: a filter of 2^31 or more elements is not supported, got %r" % (who, fs))
        return cout, fs[-3], fs[-2]
    (b, h, w, cin, _, fh, fw, sh, sw), shape = _float_conv_check(who, x, filter_of, bias, stride, padding, activation, out, out_bits)
    return DepthwiseDesc(b, h, w, cin, int(depth_multiplier), fh, fw, sh, sw, int(padding), int(activation)), shape


def depthwise_conv2d(x, filter, bias=None, stride=1, padding=PADDING_SAME, depth_multiplier=1, activation=ACT_NONE, out=True,
                     out_bits=False, stream: int | None = None):
    """TFLite's builtin float DEPTHWISE_CONV_2D between binary layers (the blur of QuickNet's transition block) and the
    LceQuantize of its result, in one pass (``lce_hip_depthwise_conv2d_f32``).  ``x``: float32 NHWC on the device (or NumPy:
    copied to cuda:0 and back).  ``filter``: float32 [1, fh, fw, Cout] (or [fh, fw, Cout]), Cout = Cin x ``depth_multiplier``;
    output channel o reads input channel o // depth_multiplier.  ``bias``: float32 [Cout] or None.  ``stride``: an int or
    (height, width).  ``padding``: ``PADDING_SAME`` / ``PADDING_VALID`` with the pools' rule (taps in the padding are skipped).
    ``activation``: ``ACT_*``.  Per output element t = fmaf(x, w, t) over its in-bounds taps in raster order from +0.0, then
    + bias, then the clamp: exact bytes (include/lce_hip.h).  ``out``: True for a new tensor, a tensor to fill (it must not
    overlap an operand), False for none.  ``out_bits``: True for new int32 [B, OH, OW, ceil(Cout/32)] bits (value < 0), a
    tensor to fill, False for none.  Returns ``(out or None, bits or None)``."""
    desc, shape = _depthwise_check(x, filter, bias, stride, padding, depth_multiplier, activation, out, out_bits)
    return _run_windowed("depthwise_conv2d", "lce_hip_depthwise_conv2d_f32", desc, shape, x, (filter, bias), out, out_bits, stream)


def _conv2d_check(x, w, bias, stride, padding, activation, out, out_bits):
    """Argument checks of ``conv2d`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (Conv2dDesc, output shape)."""
    who = "conv2d"
    def filter_of(cin):
        ws = tuple(int(v) for v in w.shape)
        if _dtype_name(w) != "float32" or len(ws) != 4 or ws[3] != cin or min(ws) < 1:
            raise ValueError("%s: w must be float32 [Cout, fh, fw, %d], got %s %r" % (who, cin, w.dtype, ws))
        if ws[1] * ws[2] * cin >= 1 << 31:
            raise ValueError("%s: a filter of 2^31 or more elements per output channel is not supported, got %r" % (who, ws))
        return ws[0], ws[1], ws[2]
    (b, h, wd, cin, cout, fh, fw, sh, sw), shape = _float_conv_check(who, x, filter_of, bias, stride, padding, activation, out, out_bits)
    return Conv2dDesc(b, h, wd, cin, cout, fh, fw, sh, sw, int(padding), int(activation)), shape


def conv2d(x, w, bias=None, stride=1, padding=PADDING_SAME, activation=ACT_NONE, out=True, out_bits=False, stream: int | None = None):
    """TFLite's builtin float CONV_2D with a filter of any extent (a network's stem, or a float KxK convolution between binary
    layers) and the LceQuantize of its result, in one call (``lce_hip_conv2d_f32``).  ``x``: float32 NHWC on the device (or
    NumPy: copied to cuda:0 and back).  ``w``: float32 [Cout, fh, fw, Cin].  ``bias``: float32 [Cout] or None.  ``stride``: an
    int or (height, width).  ``padding``: ``PADDING_SAME`` / ``PADDING_VALID`` with the pools' rule (taps in the padding are
    skipped).  ``activation``: ``ACT_*``.  Per output element t = fmaf(x, w, t) over its in-bounds taps in raster order and the
    channels of a tap in order, from +0.0, then + bias, then the clamp: exact bytes (include/lce_hip.h).  ``out``: True for a
    new tensor, a tensor to fill (it must not overlap an operand), False for none.  ``out_bits``: True for new int32
    [B, OH, OW, ceil(Cout/32)] bits (value < 0), a tensor to fill, False for none.  Returns ``(out or None, bits or None)``."""
    desc, shape = _conv2d_check(x, w, bias, stride, padding, activation, out, out_bits)
    return _run_windowed("conv2d", "lce_hip_conv2d_f32", desc, shape, x, (w, bias), out, out_bits, stream)


def _conv2d_i8_quantization(who, q_in, q_out):
    """``q_in`` and ``q_out`` as (scale, zero_point) pairs of an int8 tensor: (si, zi, so, zo)."""
    vals = []
    for name, q in (("q_in", q_in), ("q_out", q_out)):
        if not isinstance(q, (tuple, list)) or len(q) != 2:
            raise ValueError("%s: %s must be (scale, zero_point), got %r" % (who, name, q))
        scale, zp = float(np.float32(q[0])), q[1]
        if not (np.isfinite(scale) and scale > 0):
            raise ValueError("%s: %s scale must be finite and positive, got %r" % (who, name, q[0]))
        if int(zp) != zp or not -128 <= int(zp) <= 127:
            raise ValueError("%s: %s zero point must be an integer in [-128, 127], got %r" % (who, name, zp))
        vals += [scale, int(zp)]
    return tuple(vals)


def _conv2d_i8_filter(who, w, cin=None):
    """``w`` is int8 [Cout, fh, fw, Cin] (``cin``: the input's channels, None: any): its four extents."""
    ws = tuple(int(v) for v in w.shape)
    if _dtype_name(w) != "int8" or len(ws) != 4 or min(ws) < 1 or (cin is not None and ws[3] != cin):
        raise ValueError("%s: w must be int8 [Cout, fh, fw, %s], got %s %r" % (who, "Cin" if cin is None else cin, w.dtype, ws))
    return ws


def conv2d_i8_prepare(w, bias, filter_scales, q_in, q_out, activation=ACT_NONE):
    """The constants of one quantized CONV_2D for ``conv2d_i8`` (``lce_hip_conv2d_i8_prepare``, host only).  ``w``: int8 NumPy
    [Cout, fh, fw, Cin] (zero point 0).  ``bias``: int32 [Cout] or None.  ``filter_scales``: one float or Cout of them.
    ``q_in``, ``q_out``: (scale, zero_point) of the input and the output tensor.  Returns ``(table, act_min, act_max)``:
    ``table`` is int32 [3, Cout] -- c[o] = bias[o] - zi * sum(w[o]), and QuantizeMultiplier(si * sw[o] / so)'s multiplier and
    exponent -- which ``conv2d_i8`` takes; the activation range is CalculateActivationRangeQuantized's at ``q_out``.  Raises
    ``LceHipError`` (ERR_UNSUPPORTED) where the reference's own int32 accumulator could overflow."""
    who = "conv2d_i8_prepare"
    cout, fh, fw, cin = _conv2d_i8_filter(who, w)
    si, zi, so, zo = _conv2d_i8_quantization(who, q_in, q_out)
    _padding_activation_check(who, None, activation)
    if bias is not None and (_dtype_name(bias) != "int32" or tuple(bias.shape) != (cout,)):
        raise ValueError("%s: bias must be int32 [%d], got %s %r" % (who, cout, bias.dtype, tuple(bias.shape)))
    scales = np.ascontiguousarray(np.atleast_1d(np.asarray(filter_scales, np.float32)))
    if scales.ndim != 1 or scales.size not in (1, cout):
        raise ValueError("%s: filter_scales must be 1 or %d scales, got shape %r" % (who, cout, scales.shape))
    wh = np.ascontiguousarray(w)
    bh = None if bias is None else np.ascontiguousarray(bias)
    # (the table depends on the filter and the quantization alone: the window of this descriptor is the filter itself)
    desc = Conv2dI8Desc(1, fh, fw, cin, cout, fh, fw, 1, 1, PADDING_VALID, int(activation), si, zi, so, zo)
    table = np.zeros((3, cout), np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    check(lib().lce_hip_conv2d_i8_prepare(C.byref(desc), _host_ptr(wh), None if bh is None else _host_ptr(bh), _host_ptr(scales),
                                          int(scales.size), _host_ptr(table), C.byref(lo), C.byref(hi)))
    return table, lo.value, hi.value


def _conv2d_i8_check(x, w, table, q_in, q_out, stride, padding, activation, out, out_bits):
    """Argument checks of ``conv2d_i8`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (Conv2dI8Desc, output shape)."""
    who = "conv2d_i8"
    _, b, h, wd, cin = _nhwc_check(who, x, ("int8",))
    cout, fh, fw, _ = _conv2d_i8_filter(who, w, cin)
    if _dtype_name(table) != "int32" or tuple(table.shape) != (3, cout):
        raise ValueError("%s: table must be int32 [3, %d] (conv2d_i8_prepare), got %s %r" % (who, cout, table.dtype, tuple(table.shape)))
    si, zi, so, zo = _conv2d_i8_quantization(who, q_in, q_out)
    sh, sw = _pair(who, "stride", stride)
    _padding_activation_check(who, padding, activation)
    oh, ow = _window_output_hw(who, (h, wd), (fh, fw), (sh, sw), padding)
    shape = (b, oh, ow, cout)
    _check_outputs(who, None if out is True else out, None if out_bits is False else out_bits, "int8", shape)
    return Conv2dI8Desc(b, h, wd, cin, cout, fh, fw, sh, sw, int(padding), int(activation), si, zi, so, zo), shape


def conv2d_i8(x, w, table, q_in, q_out, stride=1, padding=PADDING_SAME, activation=ACT_NONE, out=True, out_bits=False,
              stream: int | None = None):
    """TFLite's builtin quantized CONV_2D with a filter of any extent (the stem of an int8-converted network, the 1x1 of a
    downsampling shortcut or a transition) and the LceQuantize of its result, in one launch on the int8 matrix instruction
    (``lce_hip_conv2d_i8``).  ``x``: int8 NHWC on the device (or NumPy: copied to cuda:0 and back).  ``w``: int8
    [Cout, fh, fw, Cin].  ``table``: int32 [3, Cout] from ``conv2d_i8_prepare`` for the same filter, quantization and
    activation.  ``q_in``, ``q_out``: (scale, zero_point) of input and output.  ``stride``: an int or (height, width).
    ``padding``: ``PADDING_SAME`` / ``PADDING_VALID`` (taps in the padding are skipped).  ``activation``: ``ACT_*``.  Integer
    arithmetic, exact bytes: reference_integer_ops::ConvPerChannel in the double-rounding build (include/lce_hip.h).  ``out``:
    True for a new int8 tensor, a tensor to fill (it must not overlap an operand), False for none.  ``out_bits``: True for new
    int32 [B, OH, OW, ceil(Cout/32)] bits (value < output zero point), a tensor to fill, False for none.  Returns
    ``(out or None, bits or None)``."""
    desc, shape = _conv2d_i8_check(x, w, table, q_in, q_out, stride, padding, activation, out, out_bits)
    return _run_windowed("conv2d_i8", "lce_hip_conv2d_i8", desc, shape, x, (w, table), out, out_bits, stream)


def _depthwise_i8_filter(who, filter, depth_multiplier, cin=None):
    """``filter`` is int8 [1, fh, fw, Cout] or [fh, fw, Cout], Cout = Cin x ``depth_multiplier`` (``cin``: the input's channels,
    None: any): (Cout, fh, fw)."""
    if not isinstance(depth_multiplier, (int, np.integer)) or depth_multiplier < 1:
        raise ValueError("%s: depth_multiplier must be a positive int, got %r" % (who, depth_multiplier))
    fs = tuple(int(v) for v in filter.shape)
    bad = _dtype_name(filter) != "int8" or len(fs) not in (3, 4) or min(fs) < 1 or (len(fs) == 4 and fs[0] != 1)
    if not bad:
        bad = fs[-1] % int(depth_multiplier) != 0 if cin is None else fs[-1] != cin * int(depth_multiplier)
    if bad:
        want = "Cin x %d" % depth_multiplier if cin is None else str(cin * int(depth_multiplier))
        raise ValueError("%s: filter must be int8 [1, fh, fw, %s] or [fh, fw, %s], got %s %r" % (who, want, want, filter.dtype, fs))
    return fs[-1], fs[-3], fs[-2]


def depthwise_conv2d_i8_prepare(filter, bias, filter_scales, q_in, q_out, depth_multiplier=1, activation=ACT_NONE):
    """The constants of one quantized DEPTHWISE_CONV_2D for ``depthwise_conv2d_i8`` (``lce_hip_depthwise_conv2d_i8_prepare``, host
    only).  ``filter``: int8 NumPy [1, fh, fw, Cout] (zero point 0).  ``bias``: int32 [Cout] or None.  ``filter_scales``: one
    float or Cout of them.  ``q_in``, ``q_out``: (scale, zero_point) of the input and the output tensor.  Returns
    ``(table, act_min, act_max)``: ``table`` is int32 [3, Cout] -- bias[o] (0 without a bias), and
    QuantizeMultiplier(si * sw[o] / so)'s multiplier and exponent -- which ``depthwise_conv2d_i8`` takes; the activation range
    is CalculateActivationRangeQuantized's at ``q_out``.  Raises ``LceHipError`` (ERR_UNSUPPORTED) where the reference's own int32
    accumulator could overflow."""
    who = "depthwise_conv2d_i8_prepare"
    cout, fh, fw = _depthwise_i8_filter(who, filter, depth_multiplier)
    si, zi, so, zo = _conv2d_i8_quantization(who, q_in, q_out)
    _padding_activation_check(who, None, activation)
    if bias is not None and (_dtype_name(bias) != "int32" or tuple(bias.shape) != (cout,)):
        raise ValueError("%s: bias must be int32 [%d], got %s %r" % (who, cout, bias.dtype, tuple(bias.shape)))
    scales = np.ascontiguousarray(np.atleast_1d(np.asarray(filter_scales, np.float32)))
    if scales.ndim != 1 or scales.size not in (1, cout):
        raise ValueError("%s: filter_scales must be 1 or %d scales, got shape %r" % (who, cout, scales.shape))
    fh_ = np.ascontiguousarray(filter)
    bh = None if bias is None else np.ascontiguousarray(bias)
    # (the table depends on the filter's extents and the quantization alone: the window of this descriptor is the filter itself)
    desc = DepthwiseI8Desc(1, fh, fw, cout // int(depth_multiplier), int(depth_multiplier), fh, fw, 1, 1, PADDING_VALID, int(activation),
                           si, zi, so, zo)
    table = np.zeros((3, cout), np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    check(lib().lce_hip_depthwise_conv2d_i8_prepare(C.byref(desc), _host_ptr(fh_), None if bh is None else _host_ptr(bh),
                                                    _host_ptr(scales), int(scales.size), _host_ptr(table), C.byref(lo), C.byref(hi)))
    return table, lo.value, hi.value


def _depthwise_i8_check(x, filter, table, q_in, q_out, stride, padding, depth_multiplier, activation, out, out_bits):
    """Argument checks of ``depthwise_conv2d_i8`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.
    Returns (DepthwiseI8Desc, output shape)."""
    who = "depthwise_conv2d_i8"
    _, b, h, wd, cin = _nhwc_check(who, x, ("int8",))
    cout, fh, fw = _depthwise_i8_filter(who, filter, depth_multiplier, cin)
    if _dtype_name(table) != "int32" or tuple(table.shape) != (3, cout):
        raise ValueError("%s: table must be int32 [3, %d] (depthwise_conv2d_i8_prepare), got %s %r" % (who, cout, table.dtype,
                                                                                                      tuple(table.shape)))
    si, zi, so, zo = _conv2d_i8_quantization(who, q_in, q_out)
    sh, sw = _pair(who, "stride", stride)
    _padding_activation_check(who, padding, activation)
    oh, ow = _window_output_hw(who, (h, wd), (fh, fw), (sh, sw), padding)
    shape = (b, oh, ow, cout)
    _check_outputs(who, None if out is True else out, None if out_bits is False else out_bits, "int8", shape)
    return DepthwiseI8Desc(b, h, wd, cin, int(depth_multiplier), fh, fw, sh, sw, int(padding), int(activation), si, zi, so, zo), shape


def depthwise_conv2d_i8(x, filter, table, q_in, q_out, stride=1, padding=PADDING_SAME, depth_multiplier=1, activation=ACT_NONE, out=True,
                        out_bits=False, stream: int | None = None, path: int | None = None, report_path: bool = False):
    """TFLite's builtin quantized DEPTHWISE_CONV_2D (the blur of an int8 QuickNet's transition, the depthwise convolution of its
    stem) and the LceQuantize of its result, in one launch (``lce_hip_depthwise_conv2d_i8``).  ``x``: int8 NHWC on the device (or
    NumPy: copied to cuda:0 and back).  ``filter``: int8 [1, fh, fw, Cout] (or [fh, fw, Cout]), Cout = Cin x
    ``depth_multiplier``; output channel o reads input channel o // depth_multiplier.  ``table``: int32 [3, Cout] from
    ``depthwise_conv2d_i8_prepare`` for the same filter, quantization and activation.  ``q_in``, ``q_out``: (scale, zero_point)
    of input and output.  ``stride``: an int or (height, width).  ``padding``: ``PADDING_SAME`` / ``PADDING_VALID`` (taps in the
    padding are skipped).  ``activation``: ``ACT_*``.  Integer arithmetic, exact bytes:
    reference_integer_ops::DepthwiseConvPerChannel in the double-rounding build (include/lce_hip.h).  ``out``: True for a new
    int8 tensor, a tensor to fill (it must not overlap an operand), False for none.  ``out_bits``: True for new int32
    [B, OH, OW, ceil(Cout/32)] bits (value < output zero point), a tensor to fill, False for none.  ``path``: None for the
    entry's own choice; 0 forces the row path and 1 the 16-byte path (``lce_hip_depthwise_conv2d_i8_forced``: for tests and
    measurements; the bytes are the same).  Returns ``(out or None, bits or None)``, and with ``report_path`` a third value: 1
    when the launch took the 16-byte path, else 0."""
    import torch
    who = "depthwise_conv2d_i8"
    desc, shape = _depthwise_i8_check(x, filter, table, q_in, q_out, stride, padding, depth_multiplier, activation, out, out_bits)
    if path not in (None, 0, 1):
        raise ValueError("%s: path must be None, 0 or 1, got %r" % (who, path))
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    xd, fd, td = on_dev(x), on_dev(filter), on_dev(table)
    out_d = None if out is False else torch.empty(shape, dtype=xd.dtype, device=dev) if out is True else on_dev(out)
    bits_d = None if (out_bits is False or out_bits is None) else _new_bits(shape[:-1], shape[-1], dev) if out_bits is True else on_dev(out_bits)
    ptrs = [_dev_ptr(t) for t in (xd, fd, td, out_d, bits_d)]
    took = C.c_int32(-1)
    with torch.cuda.device(dev):
        st = C.c_void_p(_stream_or_current(stream, dev))
        if path is None:
            check(lib().lce_hip_depthwise_conv2d_i8_path(C.byref(desc), *ptrs, C.byref(took)))
            check(lib().lce_hip_depthwise_conv2d_i8(C.byref(desc), *ptrs, st))
        else:
            check(lib().lce_hip_depthwise_conv2d_i8_forced(C.byref(desc), int(path), *ptrs, st))
            took.value = int(path)
    res = _results(host, out_d, bits_d, None if out is True else out, None if out_bits is True else out_bits)
    return (*res, int(took.value)) if report_path else res


class _Pooled:
    """The shape and dtype of a pooled tensor that is never made: what the depthwise checks ask of their input."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype


def _pool_depthwise_run(who, kind, descs, shape, x, constants, out, out_bits, stream, path, report_path):
    """The run ``pool_depthwise`` and ``pool_depthwise_i8`` share: the entry's own choice of path (reported by ``..._path``) or a
    forced one."""
    import torch
    if path not in (None, 0, 1):
        raise ValueError("%s: path must be None, 0 or 1, got %r" % (who, path))
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    xd = on_dev(x)
    operands = [None if c is None else on_dev(c) for c in constants]
    out_d = None if out is False else torch.empty(shape, dtype=xd.dtype, device=dev) if out is True else on_dev(out)
    bits_d = None if (out_bits is False or out_bits is None) else _new_bits(shape[:-1], shape[-1], dev) if out_bits is True else on_dev(out_bits)
    ptrs = [_dev_ptr(t) for t in (xd, *operands, out_d, bits_d)]
    refs = [C.byref(d) for d in descs]
    took = C.c_int32(-1)
    with torch.cuda.device(dev):
        st = C.c_void_p(_stream_or_current(stream, dev))
        if path is None:
            check(getattr(lib(), "lce_hip_pool_depthwise_%s_path" % kind)(*refs, *ptrs, C.byref(took)))
            check(getattr(lib(), "lce_hip_pool_depthwise_%s" % kind)(*refs, *ptrs, st))
        else:
            check(getattr(lib(), "lce_hip_pool_depthwise_%s_forced" % kind)(*refs, int(path), *ptrs, st))
            took.value = int(path)
    res = _results(host, out_d, bits_d, None if out is True else out, None if out_bits is True else out_bits)
    return (*res, int(took.value)) if report_path else res


def pool_depthwise(x, pool_filter, filter, bias=None, pool_stride=1, pool_padding=PADDING_SAME, pool_activation=ACT_NONE, stride=1,
                   padding=PADDING_SAME, depth_multiplier=1, activation=ACT_NONE, out=True, out_bits=False, stream: int | None = None,
                   path: int | None = None, report_path: bool = False):
    """A float MAX_POOL_2D and the DEPTHWISE_CONV_2D that reads it (QuickNet's transition: pool 2x2 / 1 SAME, then the 3x3 / 2
    blur) and the LceQuantize of the result, in ONE launch that never writes the pooled tensor (``lce_hip_pool_depthwise_f32``).
    The bytes are those of ``pool2d(x, POOL_MAX, pool_filter, pool_stride, pool_padding, pool_activation)`` followed by
    ``depthwise_conv2d(pooled, filter, bias, stride, padding, depth_multiplier, activation)``; the arguments are theirs.  ``path``:
    None for the entry's own choice; 0 forces the row path (any geometry) and 1 the 16-byte path (pool stride 1 and filter <= 2 x 2,
    depthwise filter <= 3 x 3, multiplier 1, channels % 4 == 0, % 32 with bits) -- for tests and measurements, the bytes are the
    same.  Returns ``(out or None, bits or None)``, and with ``report_path`` a third value: 1 when the launch took the 16-byte path."""
    who = "pool_depthwise"
    if _dtype_name(x) != "float32":
        raise ValueError("%s: x must be a float32 NHWC tensor, got %s" % (who, x.dtype))
    pdesc, pooled = _pool2d_check(x, POOL_MAX, pool_filter, pool_stride, pool_padding, pool_activation, True, False, None, 0)
    ddesc, shape = _depthwise_check(_Pooled(pooled, x.dtype), filter, bias, stride, padding, depth_multiplier, activation, out, out_bits)
    return _pool_depthwise_run(who, "f32", (pdesc, ddesc), shape, x, (filter, bias), out, out_bits, stream, path, report_path)


def pool_depthwise_i8(x, pool_filter, filter, table, q_in, q_out, pool_stride=1, pool_padding=PADDING_SAME, pool_activation=ACT_NONE, stride=1,
                      padding=PADDING_SAME, depth_multiplier=1, activation=ACT_NONE, out=True, out_bits=False, stream: int | None = None,
                      path: int | None = None, report_path: bool = False):
    """The int8 form (``lce_hip_pool_depthwise_i8``): ``q_in`` = (scale, zero_point) is the quantization of ``x`` AND of the pooled
    tensor (TFLite's pools keep it), ``table`` comes from ``depthwise_conv2d_i8_prepare`` for the same filter, ``q_in``, ``q_out``
    and activation.  The bytes are those of ``pool2d(x, POOL_MAX, ..., scale, zero_point)`` followed by ``depthwise_conv2d_i8``;
    ``path`` and ``report_path`` as ``pool_depthwise``'s (the 16-byte path needs channels % 16 == 0)."""
    who = "pool_depthwise_i8"
    si, zi, _, _ = _conv2d_i8_quantization(who, q_in, q_out)
    if _dtype_name(x) != "int8":
        raise ValueError("%s: x must be an int8 NHWC tensor, got %s" % (who, x.dtype))
    pdesc, pooled = _pool2d_check(x, POOL_MAX, pool_filter, pool_stride, pool_padding, pool_activation, True, False, si, zi)
    ddesc, shape = _depthwise_i8_check(_Pooled(pooled, x.dtype), filter, table, q_in, q_out, stride, padding, depth_multiplier, activation, out,
                                       out_bits)
    return _pool_depthwise_run(who, "i8", (pdesc, ddesc), shape, x, (filter, table), out, out_bits, stream, path, report_path)


def _fully_connected_check(x, w, bias, activation, out):
    """Argument checks of ``fully_connected`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (FcDesc, output shape)."""
    xs, ws = tuple(int(v) for v in x.shape), tuple(int(v) for v in w.shape)
    if _dtype_name(x) != "float32" or len(xs) != 2 or min(xs) < 1:
        raise ValueError("fully_connected: x must be a non-empty float32 [batch, inputs] tensor, got %s %r" % (x.dtype, xs))
    if _dtype_name(w) != "float32" or len(ws) != 2 or ws[0] < 1 or ws[1] != xs[1]:
        raise ValueError("fully_connected: w must be float32 [outputs, %d], got %s %r" % (xs[1], w.dtype, ws))
    if bias is not None and (_dtype_name(bias) != "float32" or tuple(bias.shape) != (ws[0],)):
        raise ValueError("fully_connected: bias must be float32 [%d], got %s %r" % (ws[0], bias.dtype, tuple(bias.shape)))
    _padding_activation_check("fully_connected", None, activation)
    shape = (xs[0], ws[0])
    _check_outputs("fully_connected", out, None, "float32", shape)
    return FcDesc(xs[0], xs[1], ws[0], int(activation)), shape


def fully_connected(x, w, bias=None, activation=ACT_NONE, out=None, stream: int | None = None):
    """TFLite's builtin float FULLY_CONNECTED -- the Dense layer of a classifier head -- in one launch
    (``lce_hip_fully_connected_f32``).  ``x``: float32 [batch, inputs] on the device (or NumPy: copied to cuda:0 and back).
    ``w``: float32 [outputs, inputs].  ``bias``: float32 [outputs] or None.  ``activation``: ``ACT_*``.  Per output element
    t = fmaf(x[k], w[o][k], t) over k in order from +0.0, then + bias, then the clamp: the bytes of ``conv1x1`` on a
    [batch, 1, 1, inputs] image (include/lce_hip.h).  ``out``: None for a new tensor, or a tensor [batch, outputs] to fill (it
    must not overlap an operand).  Returns the output."""
    desc, shape = _fully_connected_check(x, w, bias, activation, out)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "fully_connected", "x's")
    xd, wd, bd = on_dev(x), on_dev(w), None if bias is None else on_dev(bias)
    out_d = torch.empty(shape, dtype=torch.float32, device=dev) if out is None else on_dev(out)
    with torch.cuda.device(dev):
        check(lib().lce_hip_fully_connected_f32(C.byref(desc), _dev_ptr(xd), _dev_ptr(wd), _dev_ptr(bd), _dev_ptr(out_d),
                                                C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, None, out)[0]


def _softmax_check(x, beta, out):
    """Argument checks of ``softmax`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.  Returns
    (rows, cols)."""
    shape = tuple(int(v) for v in x.shape)
    if _dtype_name(x) != "float32" or len(shape) < 1 or min(shape) < 1:
        raise ValueError("softmax: x must be a non-empty float32 tensor, got %s %r" % (x.dtype, shape))
    if not (np.isfinite(float(beta)) and float(beta) > 0):
        raise ValueError("softmax: beta must be finite and positive, got %r" % (beta,))
    if out is not None and out is not x:
        _check_outputs("softmax", out, None, "float32", shape)
    return int(np.prod(shape[:-1], dtype=np.int64)), shape[-1]


def softmax(x, beta: float = 1.0, out=None, stream: int | None = None):
    """TFLite's builtin float SOFTMAX over the last axis in one launch (``lce_hip_softmax_f32``), to the bytes include/lce_hip.h
    states: the row maximum, a = (x - max) * beta, the library's own exp (a Cody-Waite reduction and a polynomial, within 1 ulp),
    a sum in a fixed order, the correctly rounded division.  ``x``: float32 [..., cols] on the device (or NumPy: copied to cuda:0
    and back).  ``beta``: finite and positive.  ``out``: None for a new tensor, a tensor of x's shape to fill, or ``x`` itself
    (in place); any other overlap is refused.  Returns the output."""
    rows, cols = _softmax_check(x, beta, out)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "softmax", "x's")
    xd = on_dev(x)
    out_d = torch.empty_like(xd) if out is None else xd if out is x else on_dev(out)
    with torch.cuda.device(dev):
        check(lib().lce_hip_softmax_f32(rows, cols, float(beta), _dev_ptr(xd), _dev_ptr(out_d),
                                        C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, None, out)[0]


# ---------------------------------------------------------------------------------------
# the binarized Dense layer (include/lce_hip.h)
# ---------------------------------------------------------------------------------------
def bfc_prepare(w):
    """The sign bits and row scales of one binarized Dense layer for ``binary_fully_connected`` (``lce_hip_bfc_prepare``, host
    only).  ``w``: float32 NumPy [outputs, inputs], the weights of the converted model's float FULLY_CONNECTED: every entry of
    row o must be +s[o] or -s[o], s[o] finite with 2^-100 <= s[o] <= 2^100.  Returns ``(bits, scale)``: int32
    [outputs, ceil(inputs/32)] (LSB first, bit 1 for a negative weight, padding bits 0) and float32 [outputs].  Raises
    ``LceHipError`` (ERR_UNSUPPORTED) for other weights -- a zero, a NaN, an infinity, mixed magnitudes -- and for
    inputs >= 2^23."""
    ws = tuple(int(v) for v in w.shape)
    if not isinstance(w, np.ndarray) or _dtype_name(w) != "float32" or len(ws) != 2 or min(ws) < 1:
        raise ValueError("bfc_prepare: w must be a non-empty float32 NumPy array [outputs, inputs], got %s %r" % (getattr(w, "dtype", type(w)), ws))
    n, k = ws
    desc = BfcDesc(1, k, n, ACT_NONE)
    check(lib().lce_hip_bfc_check(C.byref(desc)))                 # (before the buffers are sized)
    wh = np.ascontiguousarray(w)
    bits, scale = np.zeros((n, bitpacked_size(k)), np.int32), np.zeros(n, np.float32)
    check(lib().lce_hip_bfc_prepare(C.byref(desc), _host_ptr(wh), _host_ptr(bits), _host_ptr(scale)))
    return bits, scale


def _bfc_check(x_bits, inputs, weight_bits, scale, bias, activation, out, out_bits):
    """Argument checks of ``binary_fully_connected`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.
    Returns (BfcDesc, output shape)."""
    who = "binary_fully_connected"
    if int(inputs) != inputs or int(inputs) < 1:
        raise ValueError("%s: inputs must be a positive integer, got %r" % (who, inputs))
    kw = bitpacked_size(int(inputs))
    xs, ws = tuple(int(v) for v in x_bits.shape), tuple(int(v) for v in weight_bits.shape)
    if _dtype_name(x_bits) != "int32" or len(xs) != 2 or xs[0] < 1 or xs[1] != kw:
        raise ValueError("%s: x_bits must be int32 [batch, %d], got %s %r" % (who, kw, x_bits.dtype, xs))
    if _dtype_name(weight_bits) != "int32" or len(ws) != 2 or ws[0] < 1 or ws[1] != kw:
        raise ValueError("%s: weight_bits must be int32 [outputs, %d], got %s %r" % (who, kw, weight_bits.dtype, ws))
    if _dtype_name(scale) != "float32" or tuple(scale.shape) != (ws[0],):
        raise ValueError("%s: scale must be float32 [%d], got %s %r" % (who, ws[0], scale.dtype, tuple(scale.shape)))
    if bias is not None and (_dtype_name(bias) != "float32" or tuple(bias.shape) != (ws[0],)):
        raise ValueError("%s: bias must be float32 [%d], got %s %r" % (who, ws[0], bias.dtype, tuple(bias.shape)))
    _padding_activation_check(who, None, activation)
    shape = (xs[0], ws[0])
    _check_outputs(who, None if out is True else out, None if out_bits is False else out_bits, "float32", shape)
    return BfcDesc(xs[0], int(inputs), ws[0], int(activation)), shape


def binary_fully_connected(x_bits, inputs, weight_bits, scale, bias=None, activation=ACT_NONE, out=True, out_bits=False,
                           stream: int | None = None):
    """A binarized Dense layer (larq's QuantDense behind a sign) and the LceQuantize of its result in one launch on the FP4 matrix
    cores (``lce_hip_binary_fully_connected``).  ``x_bits``: int32 [batch, ceil(inputs/32)] on the device (or NumPy: copied to
    cuda:0 and back), the bits of the activations (``bitpack``: bit 1 = negative).  ``weight_bits``, ``scale``: from
    ``bfc_prepare``.  ``bias``: float32 [outputs] or None.  Per output element t = the exact integer sum of a_k * w_k,
    p = t * scale[o], v = p + bias[o] (two roundings), the clamp, bit = v < 0 (include/lce_hip.h).  ``out``: True for a new
    float32 [batch, outputs] tensor, a tensor to fill (it must not overlap an operand), False for none.  ``out_bits``: True for
    new int32 [batch, ceil(outputs/32)] bits, a tensor to fill, False for none.  Returns ``(out or None, bits or None)``."""
    import torch
    who = "binary_fully_connected"
    desc, shape = _bfc_check(x_bits, inputs, weight_bits, scale, bias, activation, out, out_bits)
    host = isinstance(x_bits, np.ndarray)
    dev = torch.device("cuda:0") if host else x_bits.device
    on_dev = lambda a: _on_dev(a, dev, who, "x_bits's")
    xd, wd, sd, bd = on_dev(x_bits), on_dev(weight_bits), on_dev(scale), None if bias is None else on_dev(bias)
    out_d = None if out is False else torch.empty(shape, dtype=torch.float32, device=dev) if out is True else on_dev(out)
    bits_d = None if (out_bits is False or out_bits is None) else _new_bits(shape[:-1], shape[-1], dev) if out_bits is True else on_dev(out_bits)
    with torch.cuda.device(dev):
        check(lib().lce_hip_binary_fully_connected(C.byref(desc), _dev_ptr(xd), _dev_ptr(wd), _dev_ptr(sd), _dev_ptr(bd), _dev_ptr(out_d),
                                                   _dev_ptr(bits_d), C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, bits_d, None if out is True else out, None if out_bits is True else out_bits)


# ---------------------------------------------------------------------------------------
# the int8 classifier head and the float / int8 boundary (include/lce_hip.h)
# ---------------------------------------------------------------------------------------
SOFTMAX_I8_OUT = (1.0 / 256.0, -128)                    # the one output quantization of ``softmax_i8``


def _q1(who, name, q):
    """One (scale, zero_point) of an int8 tensor, checked as ``_conv2d_i8_quantization`` checks its two."""
    if not isinstance(q, (tuple, list)) or len(q) != 2:
        raise ValueError("%s: %s must be (scale, zero_point), got %r" % (who, name, q))
    scale, zp = float(np.float32(q[0])), q[1]
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("%s: %s scale must be finite and positive, got %r" % (who, name, q[0]))
    if int(zp) != zp or not -128 <= int(zp) <= 127:
        raise ValueError("%s: %s zero point must be an integer in [-128, 127], got %r" % (who, name, zp))
    return scale, int(zp)


def _fc_i8_weights(who, w, inputs=None):
    ws = tuple(int(v) for v in w.shape)
    if _dtype_name(w) != "int8" or len(ws) != 2 or min(ws) < 1 or (inputs is not None and ws[1] != inputs):
        raise ValueError("%s: w must be int8 [outputs, %s], got %s %r" % (who, "inputs" if inputs is None else inputs, w.dtype, ws))
    return ws


def fully_connected_i8_prepare(w, bias, weight_scales, q_in, q_out, activation=ACT_NONE):
    """The constants of one quantized FULLY_CONNECTED for ``fully_connected_i8`` (``lce_hip_fully_connected_i8_prepare``, host
    only).  ``w``: int8 NumPy [outputs, inputs] (zero point 0).  ``bias``: int32 [outputs] or None.  ``weight_scales``: one float
    or one per output.  Returns ``(table, act_min, act_max)`` as ``conv2d_i8_prepare`` does; raises ``LceHipError``
    (ERR_UNSUPPORTED) where the reference's own int32 accumulator could overflow."""
    who = "fully_connected_i8_prepare"
    n, k = _fc_i8_weights(who, w)
    (si, zi), (so, zo) = _q1(who, "q_in", q_in), _q1(who, "q_out", q_out)
    _padding_activation_check(who, None, activation)
    if bias is not None and (_dtype_name(bias) != "int32" or tuple(bias.shape) != (n,)):
        raise ValueError("%s: bias must be int32 [%d], got %s %r" % (who, n, bias.dtype, tuple(bias.shape)))
    scales = np.ascontiguousarray(np.atleast_1d(np.asarray(weight_scales, np.float32)))
    if scales.ndim != 1 or scales.size not in (1, n):
        raise ValueError("%s: weight_scales must be 1 or %d scales, got shape %r" % (who, n, scales.shape))
    wh = np.ascontiguousarray(w)
    bh = None if bias is None else np.ascontiguousarray(bias)
    desc = FcI8Desc(1, k, n, int(activation), si, zi, so, zo)
    table = np.zeros((3, n), np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    check(lib().lce_hip_fully_connected_i8_prepare(C.byref(desc), _host_ptr(wh), None if bh is None else _host_ptr(bh),
                                                   _host_ptr(scales), int(scales.size), _host_ptr(table), C.byref(lo), C.byref(hi)))
    return table, lo.value, hi.value


def _fully_connected_i8_check(x, w, table, q_in, q_out, activation, out):
    """Argument checks of ``fully_connected_i8`` on shapes and dtypes only (NumPy or torch): nothing here touches a device.
    Returns (FcI8Desc, output shape)."""
    who = "fully_connected_i8"
    xs = tuple(int(v) for v in x.shape)
    if _dtype_name(x) != "int8" or len(xs) != 2 or min(xs) < 1:
        raise ValueError("%s: x must be a non-empty int8 [batch, inputs] tensor, got %s %r" % (who, x.dtype, xs))
    n, _ = _fc_i8_weights(who, w, xs[1])
    if _dtype_name(table) != "int32" or tuple(table.shape) != (3, n):
        raise ValueError("%s: table must be int32 [3, %d] (fully_connected_i8_prepare), got %s %r" % (who, n, table.dtype, tuple(table.shape)))
    (si, zi), (so, zo) = _q1(who, "q_in", q_in), _q1(who, "q_out", q_out)
    _padding_activation_check(who, None, activation)
    shape = (xs[0], n)
    _check_outputs(who, out, None, "int8", shape)
    return FcI8Desc(xs[0], xs[1], n, int(activation), si, zi, so, zo), shape


def fully_connected_i8(x, w, table, q_in, q_out, activation=ACT_NONE, out=None, stream: int | None = None):
    """TFLite's builtin quantized FULLY_CONNECTED -- the Dense layer of an int8 classifier head -- in one launch on the int8
    matrix instruction (``lce_hip_fully_connected_i8``).  ``x``: int8 [batch, inputs] on the device (or NumPy: copied to cuda:0
    and back).  ``w``: int8 [outputs, inputs].  ``table``: int32 [3, outputs] from ``fully_connected_i8_prepare``.  The bytes
    are ``conv2d_i8``'s on a [batch, 1, 1, inputs] image.  ``out``: None for a new tensor, or an int8 tensor [batch, outputs] to
    fill.  Returns the output."""
    desc, shape = _fully_connected_i8_check(x, w, table, q_in, q_out, activation, out)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "fully_connected_i8", "x's")
    xd, wd, td = on_dev(x), on_dev(w), on_dev(table)
    out_d = torch.empty(shape, dtype=torch.int8, device=dev) if out is None else on_dev(out)
    with torch.cuda.device(dev):
        check(lib().lce_hip_fully_connected_i8(C.byref(desc), _dev_ptr(xd), _dev_ptr(wd), _dev_ptr(td), _dev_ptr(out_d),
                                               C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, None, out)[0]


def _mean_i8_desc(who, x, q_in, q_out):
    _, b, h, w, c = _nhwc_check(who, x, ("int8",))
    (si, zi), (so, zo) = _q1(who, "q_in", q_in), _q1(who, "q_out", q_out)
    return MeanI8Desc(b, h, w, c, si, zi, so, zo), (b, c)


def mean_i8_prepare(shape, q_in, q_out):
    """``lce_hip_mean_i8_prepare`` for an NHWC ``shape``: QuantizeMultiplier(si / so) as (multiplier, exponent).  Raises
    ``LceHipError`` (ERR_UNSUPPORTED) where an intermediate of the entry's arithmetic could leave int32."""
    who = "mean_i8_prepare"
    (si, zi), (so, zo) = _q1(who, "q_in", q_in), _q1(who, "q_out", q_out)
    b, h, w, c = (int(v) for v in shape)
    desc = MeanI8Desc(b, h, w, c, si, zi, so, zo)
    m, e = C.c_int32(), C.c_int32()
    check(lib().lce_hip_mean_i8_prepare(C.byref(desc), C.byref(m), C.byref(e)))
    return m.value, e.value


def mean_i8(x, q_in, q_out, out=None, stream: int | None = None):
    """TFLite's builtin int8 MEAN over height and width in one launch (``lce_hip_mean_i8``).  ``x``: int8 NHWC on the device (or
    NumPy: copied to cuda:0 and back).  Returns int8 [batch, channels]: the exact sum of x - zi, the multiplier of si / so, then
    the division by H * W rounding half away from zero (include/lce_hip.h)."""
    desc, shape = _mean_i8_desc("mean_i8", x, q_in, q_out)
    _check_outputs("mean_i8", out, None, "int8", shape)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "mean_i8", "x's")
    xd = on_dev(x)
    out_d = torch.empty(shape, dtype=torch.int8, device=dev) if out is None else on_dev(out)
    with torch.cuda.device(dev):
        check(lib().lce_hip_mean_i8(C.byref(desc), _dev_ptr(xd), _dev_ptr(out_d), C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, None, out)[0]


def softmax_i8(x, input_scale, beta: float = 1.0, q_out=SOFTMAX_I8_OUT, out=None, stream: int | None = None):
    """TFLite's builtin int8 SOFTMAX over the last axis in one launch (``lce_hip_softmax_i8``), to the bytes include/lce_hip.h
    states.  ``x``: int8 [..., cols] at scale ``input_scale`` (its zero point cancels).  The output is int8 at exactly
    (1/256, -128); any other ``q_out`` raises ``LceHipError`` (ERR_UNSUPPORTED).  ``out``: None for a new tensor, a tensor of
    x's shape to fill, or ``x`` itself (in place).  Returns the output."""
    shape = tuple(int(v) for v in x.shape)
    if _dtype_name(x) != "int8" or len(shape) < 1 or min(shape) < 1:
        raise ValueError("softmax_i8: x must be a non-empty int8 tensor, got %s %r" % (x.dtype, shape))
    if out is not None and out is not x:
        _check_outputs("softmax_i8", out, None, "int8", shape)
    rows, cols = int(np.prod(shape[:-1], dtype=np.int64)), shape[-1]
    check(lib().lce_hip_softmax_i8_check(rows, cols, float(input_scale), float(beta), float(q_out[0]), int(q_out[1])))
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, "softmax_i8", "x's")
    xd = on_dev(x)
    out_d = torch.empty_like(xd) if out is None else xd if out is x else on_dev(out)
    with torch.cuda.device(dev):
        check(lib().lce_hip_softmax_i8(rows, cols, float(input_scale), float(beta), float(q_out[0]), int(q_out[1]), _dev_ptr(xd),
                                       _dev_ptr(out_d), C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, None, out)[0]


def _quant_run(who, entry, x, in_dtype, out_dtype, q, out, stream):
    scale, zp = _q1(who, "q", q)
    shape = tuple(int(v) for v in x.shape)
    if _dtype_name(x) != in_dtype:
        raise ValueError("%s: x must be a %s tensor, got %s" % (who, in_dtype, x.dtype))
    _check_outputs(who, out, None, out_dtype, shape)
    import torch
    host = isinstance(x, np.ndarray)
    dev = torch.device("cuda:0") if host else x.device
    on_dev = lambda a: _on_dev(a, dev, who, "x's")
    xd = on_dev(x)
    out_d = torch.empty(shape, dtype=getattr(torch, out_dtype), device=dev) if out is None else on_dev(out)
    with torch.cuda.device(dev):
        check(getattr(lib(), entry)(xd.numel(), scale, zp, _dev_ptr(xd), _dev_ptr(out_d), C.c_void_p(_stream_or_current(stream, dev))))
    return _results(host, out_d, None, out)[0]


def quantize_i8(x, q, out=None, stream: int | None = None):
    """TFLite's builtin QUANTIZE float32 -> int8 at ``q`` = (scale, zero_point) (``lce_hip_quantize_f32_i8``): the IEEE division,
    roundf, the clamp in float, + zero point; a NaN gives the zero point, infinities saturate."""
    return _quant_run("quantize_i8", "lce_hip_quantize_f32_i8", x, "float32", "int8", q, out, stream)


def dequantize_i8(x, q, out=None, stream: int | None = None):
    """TFLite's builtin DEQUANTIZE int8 -> float32 at ``q`` = (scale, zero_point) (``lce_hip_dequantize_i8_f32``):
    (float)(x - zero_point) * scale, one float32 multiply."""
    return _quant_run("dequantize_i8", "lce_hip_dequantize_i8_f32", x, "int8", "float32", q, out, stream)


def bmaxpool(x, filter_height, filter_width, stride_height, stride_width, padding, stream: int | None = None, out=None):
    """LceBMaxPool2d on a CUDA int32 tensor [B,H,W,words]."""
    import torch
    assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and x.dim() == 4
    b, h, w, c = x.shape
    oh, ow = C.c_int32(), C.c_int32()
    check(lib().lce_hip_bmaxpool_output_shape(h, w, filter_height, filter_width, stride_height,
                                              stride_width, padding, C.byref(oh), C.byref(ow)))
    if out is None:
        out = torch.empty((b, oh.value, ow.value, c), dtype=torch.int32, device=x.device)
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (b, oh.value, ow.value, c)
    with torch.cuda.device(x.device):
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        check(lib().lce_hip_bmaxpool(C.c_void_p(x.data_ptr()), b, h, w, c, filter_height, filter_width,
                                     stride_height, stride_width, padding, C.c_void_p(out.data_ptr()),
                                     C.c_void_p(stream)))
    return out


# ---------------------------------------------------------------------------------------
# converter-side parameter preparation (host-only; include/lce_hip.h "lce_hip_prepare_*")
# ---------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def prepare_binary_filter(filter_hwio):
    """float HWIO +-scale filter -> (OHWI +-1 filter, post_activation_multiplier, post_activation_bias)."""
    f = _f32(filter_hwio)
    kh, kw, cin, cout = f.shape
    ohwi = np.empty((cout, kh, kw, cin), np.float32)
    mul, bias = np.empty(cout, np.float32), np.empty(cout, np.float32)
    check(lib().lce_hip_prepare_binary_filter(_host_ptr(f), kh, kw, cin, cout, _host_ptr(ohwi),
                                              _host_ptr(mul), _host_ptr(bias)))
    return ohwi, mul, bias


def prepare_fuse_post_op(op: int, value, mul, bias):
    """Fuses ``conv <op> value`` into (mul, bias); returns new arrays."""
    v = _f32(np.atleast_1d(value))
    m, b = _f32(mul).copy(), _f32(bias).copy()
    check(lib().lce_hip_prepare_fuse_post_op(op, _host_ptr(v), v.size, _host_ptr(m), _host_ptr(b), m.size))
    return m, b


def prepare_can_fuse_activation(mul, bias, padding: int, pad_values: int) -> bool:
    m, b = _f32(mul), _f32(bias)
    return bool(lib().lce_hip_prepare_can_fuse_activation(_host_ptr(m), _host_ptr(b), m.size, padding, pad_values))


def prepare_bitpacked_output(filter_ohwi, mul, bias, activation: int = ACT_NONE,
                             padding: int = PADDING_VALID, pad_values: int = 0):
    """-> (sign-flipped OHWI filter, int32 thresholds) of the bit-writing convolution."""
    f = _f32(filter_ohwi).copy()
    cout, kh, kw, cin = f.shape
    m, b = _f32(mul), _f32(bias)
    thr = np.empty(cout, np.int32)
    check(lib().lce_hip_prepare_bitpacked_output(_host_ptr(f), kh, kw, cin, cout, activation, padding, pad_values,
                                                 _host_ptr(m), _host_ptr(b), _host_ptr(thr)))
    return f, thr


def prepare_bitpack_filter(filter_ohwi):
    """float OHWI filter -> int32 [O, H, W, ceil(I/32)] (input 1 of LceBconv2d)."""
    f = _f32(filter_ohwi)
    cout, kh, kw, cin = f.shape
    words = np.empty((cout, kh, kw, (cin + 31) // 32), np.int32)
    check(lib().lce_hip_prepare_bitpack_filter(_host_ptr(f), kh, kw, cin, cout, _host_ptr(words)))
    return words
