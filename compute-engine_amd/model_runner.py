"""Run the binary sections of a converted Larq model (.tflite) on the GPU, in true batches.

Host-side counterpart of the reference's Python ``Interpreter`` for the LCE custom ops
(larq_compute_engine/tflite/python/interpreter.py:58-98, interpreter_base.py:30-95): the same
property names and the same ``predict`` contract -- a NumPy array with an implicit leading batch
dimension (or a list of arrays, one per model input) in, concatenated predictions out -- but the
reference feeds samples one at a time through a batch-1 interpreter (the converter pins the batch
to 1, mlir/tf_tfl_passes.cc:141-144) while this runner re-plans every LceBconv2d for
``batch_size`` images and keeps all intermediate tensors in HBM.

Graphs made of LCE custom ops only (LceQuantize, LceBconv2d, LceBMaxPool2d, LceDequantize) run end to end
(``predict``).  A MIXED graph -- a real converted model: float stem, batch norms / adds between binary
convolutions, float head -- is cut into its binary SECTIONS (``Interpreter.sections``: the maximal groups of LCE ops
with no builtin operator between them, include/lce_tflite_model.h); ``run_section(k, inputs)`` runs one of them on
its boundary tensors, the float operators stay with TensorFlow Lite (``predict`` on such a graph raises
``NotImplementedError`` naming the first builtin operator).
With ``elementwise_sections=True`` (``lce_tflite_model_open_ex`` with LCE_TFLITE_SECTIONS_ELEMENTWISE) the float ADD / MUL
between binary layers -- batch norm constants, residual shortcuts -- join the sections and run on the GPU as one fused pass
per chain (``lce_hip_elementwise``); a graph whose every operator then lies in a section runs through ``predict``.
With ``int8_add_sections=True`` (LCE_TFLITE_SECTIONS_INT8_ADD) the int8 residual ADD of an int8-converted network joins the
sections in the same way (``lce_hip_add_int8``: TFLite's integer arithmetic byte for byte); the two flags combine.
With ``concat_sections=True`` (LCE_TFLITE_SECTIONS_CONCAT, ``lce_tflite_model_open_opts``) the channel CONCATENATION of a
dense network (BinaryDenseNet, MeliusNet) joins them too (``lce_hip_concat``); with ``elementwise_sections`` a float dense
block is one section.
With ``pool_sections=True`` (LCE_TFLITE_SECTIONS_EXT_POOL, the 24-byte options of ``lce_tflite_model_open_opts``) the builtin
MAX_POOL_2D / AVERAGE_POOL_2D between binary layers join them (``lce_hip_pool2d``); with ``elementwise_sections`` the body of a
BinaryAlexNet is one section.
With ``conv1x1_sections=True`` (LCE_TFLITE_SECTIONS_EXT_CONV1X1, the 40-byte options) the float 1x1 CONV_2D of a transition block
or a downsampling shortcut joins them (``lce_hip_conv1x1_f32``); with ``elementwise_sections`` and ``pool_sections`` the body of
a Bi-RealNet-style or dense network is one section.
With ``depthwise_sections=True`` (LCE_TFLITE_SECTIONS_EXT_DEPTHWISE, the 56-byte options) the float DEPTHWISE_CONV_2D of
QuickNet's transition block (its 3x3 / 2 blur) joins them (``lce_hip_depthwise_conv2d_f32``); with the element-wise, pool and 1x1
flags a QuickNet body is one section.
With ``conv2d_sections=True`` (LCE_TFLITE_SECTIONS_EXT_CONV2D, the 56-byte options) a float CONV_2D of any filter extent joins
them (``lce_hip_conv2d_f32``), and with ``stem_sections=True`` (LCE_TFLITE_SECTIONS_EXT_STEM) an operator that qualifies under an
enabled flag and is ready from the start joins the first section instead of staying with the host: with every flag the stem and
the body of a converted network are ONE section fed by the image, which ``predict`` runs; only the head stays with the host.
With ``head_sections=True`` (the name ``head`` of ``lce_tflite_model_open_passes``: no bit and no size of the options struct) the
float classifier head -- MEAN over height and width, FULLY_CONNECTED, SOFTMAX -- joins them too (``lce_hip_pool2d``,
``lce_hip_fully_connected_f32``, ``lce_hip_softmax_f32``): with every flag a converted network is ONE section from the image to the
class probabilities, ``lce_only`` is true and ``predict(images)`` returns ``[N, classes]`` with nothing but the image and the
scores on the bus.  The walker carries the head's rank-2 tensors as ``[batch, 1, 1, C]``; the runner restores the file's rank.
With ``conv2d_i8_sections=True`` (the name ``conv2d_i8`` of ``lce_tflite_model_open_passes``) the quantized CONV_2D of an
int8-converted network -- its stem, the 1x1 of a downsampling shortcut or a transition -- joins them (``lce_hip_conv2d_i8``:
TFLite's integer arithmetic byte for byte on the int8 matrix instruction); with ``int8_add_sections``, ``pool_sections`` and
``stem_sections`` an int8 residual block with its shortcut, and an int8 stem with the binary layer behind it, are one section each.  Measured at batch 256 (profiles/conv2d_i8): the kernel takes 0.80 (3x3 / 2 stem), 0.41 (7x7 / 2
stem) and 0.57 (1x1 shortcut) of the float entry's time at the same shape.
With ``head_i8_sections=True`` and ``quantize_sections=True`` (the names ``head_i8`` and ``quantize``) the int8 classifier head --
MEAN, FULLY_CONNECTED, SOFTMAX on int8 tensors -- and the builtin QUANTIZE / DEQUANTIZE of the float interface join them
(``lce_hip_mean_i8``, ``lce_hip_fully_connected_i8``, ``lce_hip_softmax_i8``, ``lce_hip_quantize_f32_i8``,
``lce_hip_dequantize_i8_f32``): with every keyword an int8-converted network is ONE section too, and ``predict`` takes float
images and returns float ``[N, classes]`` on a file with a float interface, int8 on a file with an int8 interface.
With ``depthwise_i8_sections=True`` (the name ``depthwise_i8``) the quantized DEPTHWISE_CONV_2D -- QuickNet's blur and the depthwise
convolution of its stem -- joins them (``lce_hip_depthwise_conv2d_i8``: TFLite's integer arithmetic byte for byte), so an int8
QuickNet is ONE section from the float image to the float probabilities (profiles/depthwise_i8: 29 / 17 / 11 us on its three
transitions at batch 256, 53 / 29 / 16 us for the float entry).
With ``activation_sections=True``, ``reshape_sections=True`` and ``gate_sections=True`` (the names ``activation``, ``reshape`` and
``gate``) a standalone RELU / RELU_N1_TO_1 / RELU6 / LOGISTIC / PRELU, a RESHAPE that keeps the batch, and an ADD / MUL by a
``[b, 1, 1, C]`` tensor join them.  The activations and the gate are steps of the elementwise chain (``lce_hip_elementwise_ex``): the
whole tail of a ReActNet block -- batch norm, shortcut, shift, PRELU, shift and the next layer's sign bits -- is ONE pass, a
RealToBinaryNet block with its squeeze-and-excite gate is one section, and a head that flattens instead of pooling (RESHAPE,
FULLY_CONNECTED, SOFTMAX) runs on the GPU; the RESHAPE itself is a view of the same bytes.
The model file is read by the bounds-checked reader in csrc/tflite (include/lce_tflite_model.h).
"""
from __future__ import annotations

import ctypes as C
import importlib
import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

_amd = importlib.import_module(__package__ or "compute-engine_amd")
_TFL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "tflite")
_tfl = None

FLOAT32, INT32, BOOL, INT8 = 0, 2, 6, 9
SECTIONS_ELEMENTWISE = 1          # LCE_TFLITE_SECTIONS_ELEMENTWISE
SECTIONS_INT8_ADD = 2             # LCE_TFLITE_SECTIONS_INT8_ADD
SECTIONS_CONCAT = 4               # LCE_TFLITE_SECTIONS_CONCAT (lce_tflite_model_open_opts only)
SECTIONS_EXT_POOL = 1             # LCE_TFLITE_SECTIONS_EXT_POOL (sections_ext of the 24-byte options)
SECTIONS_EXT_CONV1X1 = 2          # LCE_TFLITE_SECTIONS_EXT_CONV1X1 (sections_ext of the 40-byte options)
SECTIONS_EXT_DEPTHWISE = 4        # LCE_TFLITE_SECTIONS_EXT_DEPTHWISE (sections_ext of the 56-byte options)
SECTIONS_EXT_CONV2D = 8           # LCE_TFLITE_SECTIONS_EXT_CONV2D (sections_ext of the 56-byte options)
SECTIONS_EXT_STEM = 16            # LCE_TFLITE_SECTIONS_EXT_STEM (sections_ext of the 56-byte options)
_NP = {FLOAT32: np.float32, INT32: np.int32, BOOL: np.bool_, INT8: np.int8}
LCE_OPS = ("LceQuantize", "LceDequantize", "LceBconv2d", "LceBMaxPool2d")


class _TensorInfo(C.Structure):
    _fields_ = [("type", C.c_int32), ("rank", C.c_int32), ("dims", C.c_int32 * 8), ("quantized", C.c_int32),
                ("scale", C.c_float), ("zero_point", C.c_int32), ("data", C.c_void_p), ("bytes", C.c_size_t),
                ("name", C.c_char_p)]


class _OperatorInfo(C.Structure):
    _fields_ = [("builtin_code", C.c_int32), ("custom_code", C.c_char_p), ("inputs", C.POINTER(C.c_int32)),
                ("num_inputs", C.c_int32), ("outputs", C.POINTER(C.c_int32)), ("num_outputs", C.c_int32),
                ("custom_options", C.POINTER(C.c_uint8)), ("custom_options_size", C.c_size_t)]


class _SectionInfo(C.Structure):
    _fields_ = [("ops", C.POINTER(C.c_int32)), ("num_ops", C.c_int32), ("inputs", C.POINTER(C.c_int32)), ("num_inputs", C.c_int32),
                ("outputs", C.POINTER(C.c_int32)), ("num_outputs", C.c_int32)]


class _OpenOptions(C.Structure):
    """``lce_tflite_open_options``."""
    _fields_ = [("struct_size", C.c_uint32), ("sections", C.c_uint32)]


class _OpenOptionsExt(C.Structure):
    """``lce_tflite_open_options``, the 24-byte form (``_OpenOptions`` is the first, 8-byte form)."""
    _fields_ = [("struct_size", C.c_uint32), ("sections", C.c_uint32), ("sections_ext", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class _OpenOptions40(C.Structure):
    """``lce_tflite_open_options``, the 40-byte form."""
    _fields_ = [("struct_size", C.c_uint32), ("sections", C.c_uint32), ("sections_ext", C.c_uint32), ("reserved", C.c_uint32 * 3),
                ("reserved2", C.c_uint32 * 4)]


class _OpenOptions56(C.Structure):
    """``lce_tflite_open_options``, the 56-byte form."""
    _fields_ = [("struct_size", C.c_uint32), ("sections", C.c_uint32), ("sections_ext", C.c_uint32), ("reserved", C.c_uint32 * 3),
                ("reserved2", C.c_uint32 * 4), ("reserved3", C.c_uint32 * 4)]


# THE table of the keywords of ``LceModel`` that let builtin operators join the sections, in the order their names are passed to
# ``lce_tflite_model_open_passes``: (keyword, name of the pass there, word of the options -- 0 ``sections``, 1 ``sections_ext`` --,
# bit, the smallest form of ``lce_tflite_open_options`` that carries the bit; 0: ``lce_tflite_model_open_ex`` does).  Word, bit and
# form are None for a keyword whose name only ``lce_tflite_model_open_passes`` knows.  A new pass is a row here, a row of
# ``_PASS_STATS``, a ``*_stats`` method and a sentence in ``LceModel``'s docstring.  A name newer than this table has no keyword: it
# arrives through ``LceModel(..., passes=("name",))``, which hands it to ``lce_tflite_model_open_passes`` verbatim, and its counters
# through an ordinary method (``elementwise_i8``: ``LceModel.elementwise_i8_stats``).
_PASSES = (
    ("elementwise_sections", "elementwise", 0, SECTIONS_ELEMENTWISE, 0),
    ("int8_add_sections", "int8_add", 0, SECTIONS_INT8_ADD, 0),
    ("concat_sections", "concat", 0, SECTIONS_CONCAT, 8),
    ("pool_sections", "pool", 1, SECTIONS_EXT_POOL, 24),
    ("conv1x1_sections", "conv1x1", 1, SECTIONS_EXT_CONV1X1, 40),
    ("depthwise_sections", "depthwise", 1, SECTIONS_EXT_DEPTHWISE, 56),
    ("conv2d_sections", "conv2d", 1, SECTIONS_EXT_CONV2D, 56),
    ("stem_sections", "stem", 1, SECTIONS_EXT_STEM, 56),
    ("head_sections", "head", None, None, None),
    ("conv2d_i8_sections", "conv2d_i8", None, None, None),
    ("head_i8_sections", "head_i8", None, None, None),
    ("quantize_sections", "quantize", None, None, None),
    ("depthwise_i8_sections", "depthwise_i8", None, None, None),
    ("activation_sections", "activation", None, None, None),
    ("reshape_sections", "reshape", None, None, None),
    ("gate_sections", "gate", None, None, None),
    ("binary_dense_sections", "binary_dense", None, None, None),
    ("slice_sections", "slice", None, None, None),
)
# three views of it: the keywords an options struct carries, every keyword's name, the keywords only the names reach
_SECTION_KEYWORDS = tuple((keyword, word, bit, form) for keyword, _, word, bit, form in _PASSES if word is not None)
_PASS_NAMES = {keyword: name for keyword, name, _, _, _ in _PASSES}
_NAMED_ONLY = tuple(keyword for keyword, _, word, _, _ in _PASSES if word is None)
_OPEN_OPTIONS = {C.sizeof(t): t for t in (_OpenOptions, _OpenOptionsExt, _OpenOptions40, _OpenOptions56)}
# ``lce_tflite_model_<pass>_stats`` and ``LceModel.<pass>_stats()``: the counters each reports
_PASS_STATS = {"elementwise": 3, "int8_add": 2, "concat": 2, "pool": 2, "conv1x1": 2, "depthwise": 2, "conv2d": 2, "conv_i8": 2,
               "depthwise_i8": 2, "head": 3, "head_i8": 3, "quantize": 2, "activation": 3, "gate": 2, "reshape": 2, "binary_dense": 3,
               "slice": 3}


def _section_keywords(where, sections):
    """``sections`` -- the ``**sections`` of ``where`` -- checked against ``_PASSES``: {keyword: bool} for every keyword."""
    for keyword in sections:
        if keyword not in _PASS_NAMES:
            raise TypeError("%s() got an unexpected keyword argument %r" % (where, keyword))
    return {keyword: bool(sections.get(keyword, False)) for keyword in _PASS_NAMES}


class Section:
    """A maximal group of LCE ops with no builtin operator between them: operator indices in execution order, the
    non-constant tensors it reads from outside, the tensors it must deliver (read outside it, or graph outputs)."""

    def __init__(self, info: _SectionInfo):
        self.ops = [info.ops[i] for i in range(info.num_ops)]
        self.inputs = [info.inputs[i] for i in range(info.num_inputs)]
        self.outputs = [info.outputs[i] for i in range(info.num_outputs)]

    def __repr__(self):
        return f"Section(ops={self.ops}, inputs={self.inputs}, outputs={self.outputs})"


def tflite_lib() -> C.CDLL:
    global _tfl
    if _tfl is None:
        path = os.path.join(_TFL_DIR, "liblce_tflite_ops.so")
        if not os.path.exists(path):     # a build step belongs to the build, not to an import
            raise FileNotFoundError(f"{path} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    f"(or `make -C {_TFL_DIR}`)")
        l = C.CDLL(path)
        l.lce_tflite_model_open.restype = C.c_void_p
        l.lce_tflite_model_open.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        l.lce_tflite_model_open_ex.restype = C.c_void_p
        l.lce_tflite_model_open_ex.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_char_p, C.c_size_t]
        l.lce_tflite_model_open_opts.restype = C.c_void_p
        l.lce_tflite_model_open_opts.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t]   # either form of the options
        l.lce_tflite_model_open_passes.restype = C.c_void_p
        l.lce_tflite_model_open_passes.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_size_t]
        l.lce_tflite_model_operator_reducer.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_fully_connected.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_softmax.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_pool2d.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_conv2d.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_depthwise.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_axis.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator_activation.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        for name, counters in _PASS_STATS.items():
            f = getattr(l, "lce_tflite_model_%s_stats" % name)
            f.argtypes, f.restype = [C.c_void_p] + [C.POINTER(C.c_int32)] * counters, None
        l.lce_tflite_model_elementwise_i8_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 3
        l.lce_tflite_model_elementwise_i8_stats.restype = None
        l.lce_tflite_model_gate_i8_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 3
        l.lce_tflite_model_gate_i8_stats.restype = None
        l.lce_tflite_model_transition_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 3
        l.lce_tflite_model_transition_stats.restype = None
        l.lce_tflite_model_close.argtypes = [C.c_void_p]
        for f in ("lce_tflite_model_num_tensors", "lce_tflite_model_num_operators"):
            getattr(l, f).argtypes = [C.c_void_p]
        for f in ("lce_tflite_model_inputs", "lce_tflite_model_outputs"):
            getattr(l, f).argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
        l.lce_tflite_model_tensor.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_TensorInfo)]
        l.lce_tflite_model_tensor_scales.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]
        l.lce_tflite_model_operator.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_OperatorInfo)]
        l.lce_tflite_model_bconv2d_plan.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        l.lce_tflite_option_int.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int32)]
        l.lce_tflite_model_last_error.restype = C.c_char_p
        l.lce_tflite_model_num_sections.argtypes = [C.c_void_p]
        l.lce_tflite_model_section.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_SectionInfo)]
        l.lce_tflite_model_run_section.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_void_p), C.c_void_p]
        l.lce_tflite_model_run_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]
        l.lce_tflite_model_run_stats.restype = None
        l.lce_tflite_model_use_hip_graphs.argtypes = [C.c_void_p, C.c_int32]
        l.lce_tflite_model_use_hip_graphs.restype = None
        l.lce_tflite_model_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.lce_tflite_model_graph_stats.restype = None
        l.lce_tflite_model_section_tensor_shape.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                            C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]
        _tfl = l
    return _tfl


class Tensor:
    def __init__(self, info: _TensorInfo, scales=(), quantized_dimension: int = 0):
        self.scales = tuple(scales)                       # the whole scale vector of the file (per-channel filters: one per channel)
        self.quantized_dimension = int(quantized_dimension)
        self.type = info.type
        self.shape = tuple(info.dims[i] for i in range(info.rank))
        self.scale = float(info.scale) if info.quantized else None
        self.zero_point = int(info.zero_point) if info.quantized else None
        self.name = (info.name or b"").decode()
        self.constant = bool(info.data)


class Operator:
    def __init__(self, info: _OperatorInfo, activation: int = 0, axis: int = 0, pool=(0, 0, 0, 0, 0), dilation=(1, 1),
                 depth_multiplier: int = 0):
        self.builtin_code = info.builtin_code
        self.activation = activation          # fused_activation_function of a builtin ADD / MUL / CONCATENATION / pool (0: NONE)
        self.axis = axis                      # axis of a builtin CONCATENATION as the file says (0 when absent)
        # Pool2DOptions of a builtin AVERAGE_POOL_2D / MAX_POOL_2D as the file says (all 0 when absent)
        # (a builtin CONV_2D fills padding and strides from its Conv2DOptions; its filter fields stay 0)
        self.padding, self.stride_w, self.stride_h, self.filter_width, self.filter_height = (int(v) for v in pool)
        # (a builtin DEPTHWISE_CONV_2D fills padding, strides and dilations from its DepthwiseConv2DOptions in the same way)
        self.dilation_w, self.dilation_h = (int(v) for v in dilation)   # Conv2DOptions dilation factors (1 when absent)
        self.depth_multiplier = int(depth_multiplier)   # DepthwiseConv2DOptions.depth_multiplier (0 when absent)
        self.custom_code = (info.custom_code or b"").decode()
        self.inputs = [info.inputs[i] for i in range(info.num_inputs)]
        self.outputs = [info.outputs[i] for i in range(info.num_outputs)]
        self._opts = (info.custom_options, info.custom_options_size)

    def option(self, key: str) -> Optional[int]:
        v = C.c_int32()
        rc = tflite_lib().lce_tflite_option_int(C.cast(self._opts[0], C.c_void_p), self._opts[1], key.encode(), C.byref(v))
        return None if rc else v.value


class LceModel:
    """A parsed .tflite flatbuffer (first subgraph)."""

    def __init__(self, flatbuffer: Union[bytes, str, os.PathLike], passes=(), **sections):
        """``sections``: the keywords of ``_PASSES``, each False unless given; each becomes an attribute.
        ``passes``: an iterable of pass names handed verbatim to ``lce_tflite_model_open_passes``, appended to the names of the
        keywords given and kept as ``model.passes`` (a tuple).  Names newer than ``_PASSES`` arrive this way; any name in it routes
        the constructor through ``lce_tflite_model_open_passes``, and a name the library does not know (or one given twice) raises
        ``ValueError`` with its message.  ``passes=("elementwise_i8",)``: the int8 tail of a ReActNet-style block -- ADD of a
        constant shift, PRELU, RELU / RELU_N1_TO_1 / RELU6 and the int8 -> int8 QUANTIZE, on int8 tensors -- joins the sections and a
        whole chain of them runs as ONE ``lce_hip_elementwise_i8`` launch on a table the reader prepares once per model; with
        ``int8_add_sections`` the residual ADD in front of such a chain becomes the launch's head (``elementwise_i8_stats``).
        ``passes=("gate_i8",)``: the squeeze-and-excite gate of an int8 RealToBinaryNet block -- int8 LOGISTIC (a 256-byte table,
        ``lce_hip_logistic_int8``) and int8 MUL by a [b,1,1,C] gate or a tensor (``lce_hip_mul_int8``) -- joins the sections; with
        ``int8_add_sections`` the residual ADD that alone reads the product rides in the MUL's launch (``gate_i8_stats``).
        ``passes=("transition",)``: no operator joins or leaves a section; an absorbed MAX_POOL_2D whose pooled tensor only an
        absorbed DEPTHWISE_CONV_2D of the same section reads (QuickNet's float transition) runs with it as ONE
        ``lce_hip_pool_depthwise_f32`` launch and the pooled tensor is never written (``transition_stats``); an int8 pair stays two
        launches, which measured faster than ``lce_hip_pool_depthwise_i8`` (profiles/transition/layers.txt).
        ``elementwise_sections``: float ADD / MUL between binary layers join the sections (LCE_TFLITE_SECTIONS_ELEMENTWISE,
        include/lce_tflite_model.h); the host then runs only what lies outside them.  ``int8_add_sections``: the int8
        residual ADD between binary layers joins them (LCE_TFLITE_SECTIONS_INT8_ADD).  ``concat_sections``: the channel
        CONCATENATION of a dense block joins them (LCE_TFLITE_SECTIONS_CONCAT, through ``lce_tflite_model_open_opts``).  ``pool_sections``: the
        builtin MAX_POOL_2D / AVERAGE_POOL_2D between binary layers join them (LCE_TFLITE_SECTIONS_EXT_POOL, through the
        24-byte options of ``lce_tflite_model_open_opts``).  ``conv1x1_sections``: the float 1x1 CONV_2D of a transition block or a
        downsampling shortcut joins them (LCE_TFLITE_SECTIONS_EXT_CONV1X1, through the 40-byte options).  ``depthwise_sections``: the
        float DEPTHWISE_CONV_2D of QuickNet's transition block joins them (LCE_TFLITE_SECTIONS_EXT_DEPTHWISE, through the 56-byte
        options).  ``conv2d_sections``: a float CONV_2D of any filter extent -- a network's stem -- joins them
        (LCE_TFLITE_SECTIONS_EXT_CONV2D).  ``stem_sections``: an operator that qualifies under an enabled flag and is ready from
        the start joins the first section instead of staying with the host (LCE_TFLITE_SECTIONS_EXT_STEM).  Both are bits of the
        56-byte options, which no combination of the other flags without ``depthwise_sections`` uses.  ``head_sections``: the float
        classifier head (MEAN over height and width, FULLY_CONNECTED, SOFTMAX) joins them; only then does the constructor go
        through ``lce_tflite_model_open_passes``, which names the passes -- every other combination keeps its route.
        ``conv2d_i8_sections``: the quantized CONV_2D of an int8-converted network (stem, shortcut, transition) joins them
        (``lce_hip_conv2d_i8``); it routes through ``lce_tflite_model_open_passes`` too (the name ``conv2d_i8``), and every
        combination without it keeps its route.  Its kernel takes 0.41-0.80 of the float entry's time at the same shapes (module docstring;
        profiles/conv2d_i8).  ``head_i8_sections``: the int8 classifier head (MEAN, FULLY_CONNECTED, SOFTMAX on int8 tensors)
        joins them (``lce_hip_mean_i8``, ``lce_hip_fully_connected_i8``, ``lce_hip_softmax_i8``; the name ``head_i8``).
        ``quantize_sections``: the builtin QUANTIZE float32 -> int8 and DEQUANTIZE int8 -> float32 join them (the name
        ``quantize``).  ``depthwise_i8_sections``: the quantized DEPTHWISE_CONV_2D of an int8-converted network -- QuickNet's blur
        and the depthwise convolution of its stem -- joins them (``lce_hip_depthwise_conv2d_i8``; the name ``depthwise_i8``).
        With every keyword an int8-converted network, QuickNet included, is ONE section from the image to the probabilities.
        ``activation_sections``: a standalone float RELU / RELU_N1_TO_1 / RELU6 / LOGISTIC / PRELU joins them as a step of the
        elementwise chain (``lce_hip_elementwise_ex``; the name ``activation``).  ``reshape_sections``: a RESHAPE that keeps the
        batch joins them as a view of the same bytes (the name ``reshape``).  ``gate_sections``: a float ADD / MUL of a
        ``[b, H, W, C]`` tensor by a non-constant ``[b, 1, 1, C]`` one -- a squeeze-and-excite gate -- joins them as a step of the
        same chain (the name ``gate``).  All three route through ``lce_tflite_model_open_passes``.
        ``binary_dense_sections``: a binarized Dense layer -- LceQuantize -> LceDequantize -> a float FULLY_CONNECTED whose rows
        hold only +-s -- joins them and runs on the bits as ONE ``lce_hip_binary_fully_connected`` launch on the FP4 matrix cores
        (the name ``binary_dense``); with ``head_sections`` too, the float entry takes the Dense layers this one refuses.
        ``slice_sections``: a STRIDED_SLICE / SLICE that cuts a channel window out of an image joins them (the name ``slice``);
        with ``elementwise_sections`` and ``concat_sections`` MeliusNet's improvement block -- two slices, an ADD and the
        CONCATENATION -- runs as ONE ``lce_hip_join_windows`` launch, and any other such slice as a one-window launch."""
        if not isinstance(flatbuffer, (bytes, bytearray)):
            with open(flatbuffer, "rb") as f:
                flatbuffer = f.read()
        self._data = bytes(flatbuffer)            # must outlive the handle (zero-copy reader)
        given = _section_keywords("LceModel", sections)
        self.__dict__.update(given)
        if isinstance(passes, (str, bytes)):
            raise TypeError("LceModel(): passes must be an iterable of names, not one string")
        self.passes = tuple(str(name) for name in passes)
        # a name only lce_tflite_model_open_passes knows goes there; otherwise the smallest form of the options that carries every
        # bit asked for; otherwise lce_tflite_model_open_ex
        words, size = [0, 0], 0
        for keyword, word, bit, form in _SECTION_KEYWORDS:
            if given[keyword]:
                words[word] |= bit
                size = max(size, form)
        err = C.create_string_buffer(256)
        if self.passes or any(given[keyword] for keyword in _NAMED_ONLY):
            names = ",".join([name for keyword, name, _, _, _ in _PASSES if given[keyword]] + list(self.passes))
            self._h = tflite_lib().lce_tflite_model_open_passes(self._data, len(self._data), names.encode(), err, 256)
        elif size:
            opts = _OPEN_OPTIONS[size](size, *words[:1 if size == 8 else 2])
            self._h = tflite_lib().lce_tflite_model_open_opts(self._data, len(self._data), C.byref(opts), err, 256)
        else:
            self._h = tflite_lib().lce_tflite_model_open_ex(self._data, len(self._data), words[0], err, 256)
        if not self._h:
            raise ValueError("not a readable TFLite model: " + err.value.decode(errors="replace"))
        l = tflite_lib()
        self.tensors: List[Tensor] = []
        for i in range(l.lce_tflite_model_num_tensors(self._h)):
            info = _TensorInfo()
            _amd.check(l.lce_tflite_model_tensor(self._h, i, C.byref(info)))
            qdim = C.c_int32()
            n = l.lce_tflite_model_tensor_scales(self._h, i, None, 0, C.byref(qdim))
            scales = (C.c_float * max(n, 1))()
            l.lce_tflite_model_tensor_scales(self._h, i, scales, n, None)
            self.tensors.append(Tensor(info, [float(scales[k]) for k in range(n)], qdim.value))
        self.operators: List[Operator] = []
        for i in range(l.lce_tflite_model_num_operators(self._h)):
            info = _OperatorInfo()
            _amd.check(l.lce_tflite_model_operator(self._h, i, C.byref(info)))
            act = C.c_int32()
            _amd.check(l.lce_tflite_model_operator_activation(self._h, i, C.byref(act)))
            axis = C.c_int32()
            _amd.check(l.lce_tflite_model_operator_axis(self._h, i, C.byref(axis)))
            pool = (C.c_int32 * 5)()
            _amd.check(l.lce_tflite_model_operator_pool2d(self._h, i, pool))
            conv = (C.c_int32 * 5)()
            _amd.check(l.lce_tflite_model_operator_conv2d(self._h, i, conv))
            dw = (C.c_int32 * 6)()
            _amd.check(l.lce_tflite_model_operator_depthwise(self._h, i, dw))
            if dw[3]:        # a DepthwiseConv2DOptions table: padding, strides and dilations are its own
                pool, conv = (dw[0], dw[1], dw[2], 0, 0), (0, 0, 0, dw[4], dw[5])
            self.operators.append(Operator(info, act.value, axis.value, tuple(pool), tuple(conv)[3:], dw[3]))
        buf = (C.c_int32 * 64)()
        self.inputs = [buf[i] for i in range(l.lce_tflite_model_inputs(self._h, buf, 64))]
        self.outputs = [buf[i] for i in range(l.lce_tflite_model_outputs(self._h, buf, 64))]
        self.sections: List[Section] = []
        for i in range(l.lce_tflite_model_num_sections(self._h)):
            info = _SectionInfo()
            _amd.check(l.lce_tflite_model_section(self._h, i, C.byref(info)))
            self.sections.append(Section(info))

    def close(self):
        if getattr(self, "_h", None):
            tflite_lib().lce_tflite_model_close(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int):
        if rc:
            msg = tflite_lib().lce_tflite_model_last_error().decode() or _amd.lib().lce_hip_last_error().decode()
            raise _amd.LceHipError(rc, msg)

    def section_tensor_shape(self, section: int, tensor: int, batch: int, semantics: int = _amd.SEM_OPTIMIZED):
        """([N, H, W, C], bytes) of a tensor the section reads or produces at ``batch`` images (C in words when bitpacked)."""
        dims, nbytes = (C.c_int32 * 4)(), C.c_size_t()
        self._check(tflite_lib().lce_tflite_model_section_tensor_shape(self._h, section, tensor, batch, semantics, dims, C.byref(nbytes)))
        return tuple(dims), int(nbytes.value)

    def run_section(self, section: int, batch: int, inputs_dev: Sequence[int], outputs_dev: Sequence[int], stream: int = 0,
                    semantics: int = _amd.SEM_OPTIMIZED):
        """``lce_tflite_model_run_section`` (include/lce_tflite_model.h) on raw device pointers."""
        i = (C.c_void_p * max(1, len(inputs_dev)))(*inputs_dev)
        o = (C.c_void_p * max(1, len(outputs_dev)))(*outputs_dev)
        self._check(tflite_lib().lce_tflite_model_run_section(self._h, section, batch, semantics, i, o, C.c_void_p(stream)))

    def run_stats(self):
        """(plans cached in the model, LceQuantize ops the last run folded into a convolution, bytes of intermediates)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_size_t()
        tflite_lib().lce_tflite_model_run_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def _pass_stats(self, name):
        """The counters of ``lce_tflite_model_<name>_stats``."""
        v = [C.c_int32() for _ in range(_PASS_STATS[name])]
        getattr(tflite_lib(), "lce_tflite_model_%s_stats" % name)(self._h, *[C.byref(c) for c in v])
        return tuple(int(c.value) for c in v)

    def elementwise_stats(self):
        """(lce_hip_elementwise launches, ADD / MUL operators they ran, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("elementwise")

    def int8_add_stats(self):
        """(lce_hip_add_int8 launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("int8_add")

    def concat_stats(self):
        """(lce_hip_concat launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("concat")

    def pool_stats(self):
        """(lce_hip_pool2d launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("pool")

    def conv1x1_stats(self):
        """(lce_hip_conv1x1_f32 launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("conv1x1")

    def depthwise_stats(self):
        """(lce_hip_depthwise_conv2d_f32 launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("depthwise")

    def conv2d_stats(self):
        """(lce_hip_conv2d_f32 calls, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("conv2d")

    def conv_i8_stats(self):
        """(lce_hip_conv2d_i8 launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("conv_i8")

    def depthwise_i8_stats(self):
        """(lce_hip_depthwise_conv2d_i8 launches, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("depthwise_i8")

    def head_stats(self):
        """(MEAN launches, lce_hip_fully_connected_f32 launches, lce_hip_softmax_f32 launches) of the last run."""
        return self._pass_stats("head")

    def head_i8_stats(self):
        """(lce_hip_mean_i8, lce_hip_fully_connected_i8, lce_hip_softmax_i8 launches) of the last run."""
        return self._pass_stats("head_i8")

    def quantize_stats(self):
        """(lce_hip_quantize_f32_i8 launches, lce_hip_dequantize_i8_f32 launches) of the last run."""
        return self._pass_stats("quantize")

    def activation_stats(self):
        """(lce_hip_elementwise_ex launches, operators of every kind they ran, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("activation")

    def gate_stats(self):
        """(lce_hip_elementwise_ex launches that hold a gate, LceQuantize launches they absorbed) of the last run."""
        return self._pass_stats("gate")

    def binary_dense_stats(self):
        """(lce_hip_binary_fully_connected launches, LceDequantize operators not launched because only binary Dense layers read
        them, LceQuantize launches the layers absorbed) of the last run."""
        return self._pass_stats("binary_dense")

    def slice_stats(self):
        """(lce_hip_join_windows launches, LceQuantize launches folded into them, those of the launches that took over a
        CONCATENATION) of the last run."""
        return self._pass_stats("slice")

    def elementwise_i8_stats(self):
        """(lce_hip_elementwise_i8 launches, operators of every kind they ran -- a residual ADD taken as a chain's head included --,
        LceQuantize launches they absorbed) of the last run (the pass ``elementwise_i8``, asked for through ``passes``)."""
        v = [C.c_int32() for _ in range(3)]
        tflite_lib().lce_tflite_model_elementwise_i8_stats(self._h, *[C.byref(c) for c in v])
        return tuple(int(c.value) for c in v)

    def gate_i8_stats(self):
        """(lce_hip_mul_int8 launches, MUL and residual ADD operators inside them, LceQuantize launches they absorbed) of the last
        run (the pass ``gate_i8``, asked for through ``passes``); the int8 LOGISTIC launches are not among them."""
        v = [C.c_int32() for _ in range(3)]
        tflite_lib().lce_tflite_model_gate_i8_stats(self._h, *[C.byref(c) for c in v])
        return tuple(int(c.value) for c in v)

    def transition_stats(self):
        """(lce_hip_pool_depthwise_f32 launches, the MAX_POOL_2D and DEPTHWISE_CONV_2D operators inside them, LceQuantize
        launches they absorbed) of the last run (the name ``transition``, asked for through ``passes``); such a launch is in
        neither ``pool_stats`` nor ``depthwise_stats``."""
        v = [C.c_int32() for _ in range(3)]
        tflite_lib().lce_tflite_model_transition_stats(self._h, *[C.byref(c) for c in v])
        return tuple(int(c.value) for c in v)

    def reshape_stats(self):
        """(RESHAPE operators that were a view, RESHAPE operators that cost a device-to-device copy) of the last run."""
        return self._pass_stats("reshape")

    def use_hip_graphs(self, on: bool = True):
        """``lce_tflite_model_use_hip_graphs``: run_section records a section's launches once per (batch, stream, tensor
        pointers) and replays them as one launch; needs a stream of its own (not the null stream)."""
        tflite_lib().lce_tflite_model_use_hip_graphs(self._h, 1 if on else 0)

    def graph_stats(self):
        """(recordings made, run_section calls served by one)."""
        a, b = C.c_int32(), C.c_int32()
        tflite_lib().lce_tflite_model_graph_stats(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def bconv2d_plan(self, op_index: int, batch: int, semantics: int = _amd.SEM_OPTIMIZED) -> "_amd.Bconv2dPlan":
        """A ready plan (weights set) for LceBconv2d operator ``op_index`` at the given batch size."""
        h = C.c_void_p()
        rc = tflite_lib().lce_tflite_model_bconv2d_plan(self._h, op_index, batch, semantics, C.byref(h))
        if rc:
            msg = tflite_lib().lce_tflite_model_last_error().decode() or _amd.lib().lce_hip_last_error().decode()
            raise _amd.LceHipError(rc, msg)
        out_type = self.tensors[self.operators[op_index].outputs[0]].type
        dst = {FLOAT32: _amd.F32, INT8: _amd.I8, INT32: _amd.BITPACKED}[out_type]
        cout = self.tensors[self.operators[op_index].inputs[1]].shape[0]
        return _amd.Bconv2dPlan.from_handle(h.value, dst, cout)


class Interpreter:
    """``Interpreter(flatbuffer_model, batch_size=...)`` -- see the module docstring."""

    def __init__(self, flatbuffer_model, batch_size: int = 256, device: str = "cuda:0", use_reference_bconv: bool = False,
                 passes=(), **sections):
        """``sections`` and ``passes``: the ``*_sections`` keywords and the pass names of ``LceModel``, described there (checked,
        then ignored, when a ready ``LceModel`` is passed: its own settings hold)."""
        _section_keywords("Interpreter", sections)
        self.model = (flatbuffer_model if isinstance(flatbuffer_model, LceModel)
                      else LceModel(flatbuffer_model, passes=passes, **sections))
        self.batch_size = int(batch_size)
        self.device = device
        self._sem = _amd.SEM_REFERENCE if use_reference_bconv else _amd.SEM_OPTIMIZED
        if self.model.passes or any(getattr(self.model, keyword) for keyword in _PASS_NAMES):
            # every operator outside the sections is the host's; one section over the whole graph runs like an LCE-only one
            # (when every operator lies in a section there is exactly one: two would need a builtin epoch in between)
            covered = set(self.model.sections[0].ops) if len(self.model.sections) == 1 else set()
            self._foreign = [(i, op) for i, op in enumerate(self.model.operators) if i not in covered]
        else:
            self._foreign = [(i, op) for i, op in enumerate(self.model.operators)
                             if op.builtin_code != 32 or op.custom_code not in LCE_OPS]

    @property
    def sections(self) -> List[Section]:
        """The binary sections of the graph (one covering everything for an LCE-only graph)."""
        return self.model.sections

    @property
    def lce_only(self) -> bool:
        return not self._foreign

    def _require_lce_only(self):
        if self._foreign:
            i, op = self._foreign[0]
            raise NotImplementedError(
                "only LCE custom ops run here; the model contains builtin operator %d %r (operator %d): run its %d binary "
                "section(s) with run_section() and keep the float operators in TensorFlow Lite"
                % (op.builtin_code, op.custom_code, i, len(self.model.sections)))

    # ---- the reference Interpreter's properties (interpreter_base.py:34-72) -------------------
    def _props(self, ids):
        t = [self.model.tensors[i] for i in ids]
        return t

    @property
    def input_types(self):
        return [_NP[t.type] for t in self._props(self.model.inputs)]

    @property
    def input_shapes(self):
        return [t.shape for t in self._props(self.model.inputs)]

    @property
    def input_scales(self):
        return [t.scale for t in self._props(self.model.inputs)]

    @property
    def input_zero_points(self):
        return [t.zero_point for t in self._props(self.model.inputs)]

    @property
    def output_types(self):
        return [_NP[t.type] for t in self._props(self.model.outputs)]

    @property
    def output_shapes(self):
        return [t.shape for t in self._props(self.model.outputs)]

    @property
    def output_scales(self):
        return [t.scale for t in self._props(self.model.outputs)]

    @property
    def output_zero_points(self):
        return [t.zero_point for t in self._props(self.model.outputs)]

    # ---- execution: the C entry lce_tflite_model_run_section does the work (plans cached per batch size in the model,
    # LceBconv2d + LceQuantize fused through run_dual, intermediates in buffers the model owns) -------------------------
    def _run_section_device(self, index: int, live, batch: int, wanted=None):
        """Section `index` on CUDA tensors: `live` maps tensor index -> tensor for every entry of ``sections[index].inputs``;
        returns the tensors `wanted` (default: the section's outputs) as new CUDA tensors.  Asynchronous on the current
        torch stream."""
        import torch
        sec = self.model.sections[index]
        dt = {FLOAT32: torch.float32, INT32: torch.int32, BOOL: torch.bool, INT8: torch.int8}
        outs = []
        for t in sec.outputs:
            dims, _ = self.model.section_tensor_shape(index, t, batch, self._sem)
            outs.append(torch.empty(dims, dtype=dt[self.model.tensors[t].type], device=self.device))
        ins = [live[t].contiguous() for t in sec.inputs]
        with torch.cuda.device(torch.device(self.device)):
            stream = torch.cuda.current_stream().cuda_stream
            self.model.run_section(index, batch, [x.data_ptr() for x in ins], [y.data_ptr() for y in outs], stream, self._sem)
            for x in ins:                                    # (the launches read them after this call returns)
                x.record_stream(torch.cuda.current_stream())
        # (the walker is 4-D throughout: a rank-2 tensor of the classifier head comes back in the file's rank)
        outs = [y.reshape((batch,) + tuple(self.model.tensors[t].shape[1:])) if len(self.model.tensors[t].shape) != 4 else y
                for t, y in zip(sec.outputs, outs)]
        by_index = dict(zip(sec.outputs, outs))
        return [by_index[t] for t in (sec.outputs if wanted is None else wanted)]

    def _run_ops(self, live, batch):
        """The whole graph (LCE ops only: ONE section) on device tensors; returns the graph outputs."""
        return self._run_section_device(0, live, batch, self.model.outputs)

    def run_section(self, index: int, inputs: Union[Sequence[np.ndarray], Dict[int, np.ndarray]]):
        """Runs binary section `index` of a (mixed) graph on its boundary tensors: `inputs` = one array per entry of
        ``sections[index].inputs`` in that order (or a dict tensor index -> array), each with a leading batch axis of any
        size (the plans are re-made for it); returns one NumPy array per entry of ``sections[index].outputs``.  Everything in
        between stays in HBM.  The float operators around the section are TensorFlow Lite's job."""
        import torch
        sec = self.model.sections[index]
        if isinstance(inputs, dict):
            arrs = [inputs[t] for t in sec.inputs]
        else:
            arrs = list(inputs)
        if len(arrs) != len(sec.inputs):
            raise ValueError("section %d reads %d tensor(s) %r, got %d array(s)" % (index, len(sec.inputs), sec.inputs, len(arrs)))
        live = {}
        for t, a in zip(sec.inputs, arrs):
            info = self.model.tensors[t]
            a = np.ascontiguousarray(a, dtype=_NP[info.type])
            if tuple(a.shape[1:]) != tuple(info.shape[1:]):
                raise ValueError("tensor %d (%s) has shape [batch, %s], got %r" % (t, info.name, ", ".join(map(str, info.shape[1:])), a.shape))
            live[t] = torch.from_numpy(a).to(self.device)
        batch = arrs[0].shape[0]
        if any(a.shape[0] != batch for a in arrs):
            raise ValueError("all inputs of a section share the batch dimension")
        return [y.cpu().numpy() for y in self._run_section_device(index, live, batch)]

    def _run_batch(self, inputs):
        """One batch, synchronously (kept for callers that drive batches themselves)."""
        import torch
        self._require_lce_only()
        live = {idx: torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
                for idx, arr in zip(self.model.inputs, inputs)}
        return [y.cpu().numpy() for y in self._run_ops(live, inputs[0].shape[0])]

    def _batches(self, x):
        """The reference's input forms (interpreter_base.py:10-27) -- an array with a leading sample axis, a
        list of such arrays (one per model input), or an iterator yielding ONE sample at a time (an array, or
        a list of arrays for several inputs) -- regrouped into batches of ``batch_size`` samples."""
        n_in = len(self.model.inputs)
        if isinstance(x, np.ndarray):
            x = [x]
        if isinstance(x, (list, tuple)):
            xs = list(x)
            if not xs or len(xs) != n_in:
                raise ValueError("expected one array per model input (%d)" % n_in)
            for b0 in range(0, xs[0].shape[0], self.batch_size):
                yield [a[b0:b0 + self.batch_size] for a in xs]
        elif hasattr(x, "__next__") and hasattr(x, "__iter__"):
            pending = [[] for _ in range(n_in)]
            for sample in x:
                parts = [sample] if isinstance(sample, np.ndarray) else list(sample)
                if len(parts) != n_in:
                    raise ValueError("expected one array per model input (%d)" % n_in)
                for p, a in zip(pending, parts):
                    p.append(a)
                if len(pending[0]) == self.batch_size:
                    yield [np.stack(p) for p in pending]
                    pending = [[] for _ in range(n_in)]
            if pending[0]:
                yield [np.stack(p) for p in pending]
        else:
            raise ValueError("Expected either a list of inputs or a Numpy array with implicit initial batch dimension "
                             "or an iterator yielding one of the above. Received: %r" % (x,))

    def predict(self, x, verbose: int = 0):
        """Input samples -> concatenated predictions (interpreter_base.py:74-95), ``batch_size`` samples per
        device pass instead of the reference's one.  Batches flow through a three-stage pipeline on three
        streams with page-locked staging buffers -- H2D of batch k+1 | the LCE ops of batch k | D2H of
        batch k-1 -- so the PCIe copies (40x the kernel time for a float 56x56x256 map) overlap the compute
        and each other's direction."""
        import torch
        self._require_lce_only()
        dev = torch.device(self.device)
        n_in = len(self.model.inputs)
        in_dt = [self.input_types[k] for k in range(n_in)]
        with torch.cuda.device(dev):
            s_in, s_out, s_run = torch.cuda.Stream(dev), torch.cuda.Stream(dev), torch.cuda.current_stream(dev)
            pin_in = [[None] * n_in for _ in range(2)]       # two sets of page-locked input staging buffers
            dev_in = [[None] * n_in for _ in range(2)]
            in_free = [None, None]                           # event: the ops that read dev_in[slot] have finished
            flights = []                                     # (pinned outputs, event) of the batches not yet collected
            results = None

            def collect(flight):
                nonlocal results
                outs, ev = flight
                ev.synchronize()
                arrs = [o.numpy().copy() for o in outs]
                results = [[a] for a in arrs] if results is None else [r + [a] for r, a in zip(results, arrs)]

            for k, batch in enumerate(self._batches(x)):
                slot, b = k & 1, batch[0].shape[0]
                if in_free[slot] is not None:
                    s_in.wait_event(in_free[slot])           # batch k-2's ops no longer read this slot's tensors
                    in_free[slot].synchronize()              # ... and its staging buffer has been copied out of
                live = {}
                for j, (idx, arr) in enumerate(zip(self.model.inputs, batch)):
                    arr = np.ascontiguousarray(arr, dtype=in_dt[j])
                    if pin_in[slot][j] is None or pin_in[slot][j].shape[0] < b or pin_in[slot][j].shape[1:] != arr.shape[1:]:
                        cap = (max(b, self.batch_size),) + arr.shape[1:]
                        pin_in[slot][j] = torch.empty(cap, dtype=torch.from_numpy(arr[:0]).dtype).pin_memory()
                        dev_in[slot][j] = torch.empty(cap, dtype=pin_in[slot][j].dtype, device=dev)
                    pin_in[slot][j][:b].copy_(torch.from_numpy(arr))
                    with torch.cuda.stream(s_in):
                        dev_in[slot][j][:b].copy_(pin_in[slot][j][:b], non_blocking=True)
                    live[idx] = dev_in[slot][j][:b]
                s_run.wait_stream(s_in)
                outs_dev = self._run_ops(live, b)
                done = torch.cuda.Event()
                done.record(s_run)
                in_free[slot] = done
                s_out.wait_event(done)
                outs_pin = []
                with torch.cuda.stream(s_out):
                    for y in outs_dev:
                        y.record_stream(s_out)
                        hp = torch.empty(y.shape, dtype=y.dtype).pin_memory()
                        hp.copy_(y, non_blocking=True)
                        outs_pin.append(hp)
                    ev = torch.cuda.Event()
                    ev.record(s_out)
                flights.append((outs_pin, ev))
                if len(flights) > 1:
                    collect(flights.pop(0))                  # batch k-1: its D2H overlapped this batch's H2D + ops
            for f in flights:
                collect(f)
        if results is None:
            raise ValueError("predict() needs at least one sample")
        outputs = [np.concatenate(o) for o in results]
        return outputs[0] if len(self.model.outputs) == 1 else outputs
