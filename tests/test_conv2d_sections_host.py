"""The float KxK CONV_2D and a network's stem inside the sections (LCE_TFLITE_SECTIONS_EXT_CONV2D and
LCE_TFLITE_SECTIONS_EXT_STEM, include/lce_tflite_model.h) on the CPU: the NumPy reference (tests/conv2d_ref.py) against its
definition, against torch's convolution on the CPU, against its 1x1 and depthwise siblings and against known answers worked by
hand; the partitions of the stem fixtures with and without the opt-ins; every condition that keeps a convolution with the host;
shape inference; the two bits in the 56-byte form of the options; the argument checks of lce_hip_conv2d_f32 / amd.conv2d (which
all fail before any device is touched) and the build of the new kernels.  Also the fixtures of the GPU side
(tests/test_gpu_conv2d.py)."""
import ctypes as C
import importlib
import re
import struct

import numpy as np
import pytest

import conv1x1_ref as CR
import conv2d_ref as R
import depthwise_ref as DR
import hipcc_lib as H
import oracle_lib as O
import pool_ref as PR
from section_models import (ADD, CONV_2D, DEPTHWISE_CONV_2D, F32_SPECIAL, MAX_POOL_2D, MUL, NONE, RELU, RELU6, RELU_N1_TO_1, TANH,
                            _conv, _open, _sections_of, alexnet_body_model, bconv_options, bireal_block_model, conv2d_op,
                            dense_block_model, depthwise_op, ew_op, float_fixture, float_op, mixed_model, pool_op,
                            quicknet_transition_model)
import synth
from tflite_writer import ModelBuilder

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
Conv2dDesc, conv2d_check = amd.Conv2dDesc, amd._conv2d_check      # (the binding under test: nothing here runs without it)

SAME, VALID = 0, 1
SIGN_BIT = 5
ACTS = (NONE, RELU, RELU_N1_TO_1, RELU6)
PARENT_FLAGS = dict(elementwise_sections=True, pool_sections=True, conv1x1_sections=True, depthwise_sections=True)
ALL_FLAGS = dict(conv2d_sections=True, stem_sections=True, **PARENT_FLAGS)


# ---- the reference against its definition ----------------------------------------------------------------------------------------
def grid_operands(filt, cin, cout, special=False):
    """(w [Cout, fh, fw, Cin], bias [Cout]) of the grid: ASYMMETRIC random filters of mixed magnitude.  `special`: subnormal and
    tiny weights among them, so that subnormal products and sums occur."""
    g = np.random.default_rng(filt[0] * 100000 + filt[1] * 10000 + cin * 300 + cout)
    shape = (cout, filt[0], filt[1], cin)
    w = (g.standard_normal(shape) * g.choice([1e-2, 1.0, 30.0], shape)).astype(np.float32)
    bias = g.standard_normal(cout).astype(np.float32)
    if special:
        w[::5] *= np.float32(1e-36)
        w[::3, 0, 0, 0] = F32_SPECIAL[6]
    return w, bias


def exact_and_magnitude(x, w, stride, padding):
    """(the float64 sum, the sum of |x w|) of every output element, from the definition: a plain loop over output pixels."""
    b, h, wd, cin = x.shape
    cout, fh, fw, _ = w.shape
    (oh, ph), (ow, pw) = PR.out_and_pad(h, fh, stride[0], padding), PR.out_and_pad(wd, fw, stride[1], padding)
    exact, mag = np.zeros((b, oh, ow, cout)), np.zeros((b, oh, ow, cout))
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    for oy in range(oh):
        for ox in range(ow):
            for fy in range(fh):
                for fx in range(fw):
                    y, xx = oy * stride[0] - ph + fy, ox * stride[1] - pw + fx
                    if 0 <= y < h and 0 <= xx < wd:
                        p = x64[:, y, xx, None, :] * w64[None, :, fy, fx, :]          # [B, Cout, Cin]
                        exact[:, oy, ox, :] += p.sum(axis=2)
                        mag[:, oy, ox, :] += np.abs(p).sum(axis=2)
    return exact, mag


def error_bound(steps, mag, bias):
    """`steps` roundings of at most 2^-24 of the running magnitude (<= sum |x w|) each, then the bias add's: 2^-24 of |t + bias|,
    where |t| <= (1 + steps 2^-24) sum |x w|."""
    b = 0.0 if bias is None else np.abs(bias.astype(np.float64))
    return steps * 2.0 ** -24 * mag + (0.0 if bias is None else 2.0 ** -24 * ((1 + steps * 2.0 ** -24) * mag + b))


@pytest.mark.parametrize("filt,stride,padding", [((3, 3), (2, 2), SAME), ((3, 3), (1, 1), VALID), ((5, 2), (2, 1), SAME),
                                                 ((7, 7), (2, 2), SAME), ((2, 3), (4, 3), SAME)])
def test_the_reference_against_a_float64_sum(filt, stride, padding):
    x = float_fixture((2, 9, 8, 3), 3)
    w, bias = grid_operands(filt, 3, 5)
    exact, mag = exact_and_magnitude(x, w, stride, padding)
    got = R.conv2d(x, w, bias, stride, padding)
    assert got.shape == exact.shape and got.dtype == np.float32
    steps = filt[0] * filt[1] * 3
    assert (np.abs(got.astype(np.float64) - (exact + bias.astype(np.float64))) <= error_bound(steps, mag, bias)).all()
    assert (np.abs(R.chain(x, w, stride, padding).astype(np.float64) - exact) <= error_bound(steps, mag, None)).all()


def test_the_reference_against_torchs_convolution_with_an_asymmetric_filter_and_uneven_same_padding():
    """8 columns, a filter of 5, stride 2 under SAME pad 1 in front and 2 behind (total 3): torch pads explicitly.  torch's sum
    order is its own, so the comparison is within the rounding of K steps."""
    torch = pytest.importorskip("torch")
    x = float_fixture((2, 9, 8, 4), 11)
    w, bias = grid_operands((3, 5), 4, 6)
    (oh, ph), (ow, pw) = PR.out_and_pad(9, 3, 2, SAME), PR.out_and_pad(8, 5, 2, SAME)
    assert (oh, ph, ow, pw) == (5, 1, 4, 1) and (ow - 1) * 2 + 5 - 8 - pw == 2
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).double()
    xt = torch.nn.functional.pad(xt, (pw, (ow - 1) * 2 + 5 - 8 - pw, ph, (oh - 1) * 2 + 3 - 9 - ph))
    want = torch.nn.functional.conv2d(xt, torch.from_numpy(w).permute(0, 3, 1, 2).double(), torch.from_numpy(bias).double(), stride=2)
    want = want.permute(0, 2, 3, 1).numpy()
    got = R.conv2d(x, w, bias, (2, 2), SAME)
    _, mag = exact_and_magnitude(x, w, (2, 2), SAME)
    assert got.shape == want.shape == (2, 5, 4, 6)
    assert (np.abs(got.astype(np.float64) - want) <= error_bound(3 * 5 * 4, mag, bias) + 1e-12 * mag).all()


def test_the_reference_is_its_siblings_on_their_ground():
    """A 1x1 filter: conv1x1_ref byte for byte, strides included.  One input and one output channel: depthwise_ref."""
    x = float_fixture((3, 5, 7, 33), 4, special=True)
    w, bias = grid_operands((1, 1), 33, 40, special=True)
    for stride in ((1, 1), (2, 2), (2, 1)):
        for padding in (SAME, VALID):
            a, b = R.conv2d(x, w, bias, stride, padding, RELU6), CR.conv1x1(x, w, bias, stride, CR.RELU6)
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    x = float_fixture((2, 9, 8, 1), 5, special=True)
    for filt in ((3, 3), (2, 3), (7, 7)):
        w, bias = grid_operands(filt, 1, 1, special=True)
        for stride in ((1, 1), (2, 1), (4, 3)):
            a = R.conv2d(x, w, bias, stride, SAME, RELU_N1_TO_1)
            b = DR.depthwise(x, w[0], bias, stride, SAME, 1, DR.RELU_N1_TO_1)
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- known answers, worked by hand ----------------------------------------------------------------------------------------------
TINY = np.float32(1e-30)
f = lambda *v: np.array(v, np.float32)
MINUS_ZERO = np.array([0x80000000], np.uint32).view(np.float32)[0]


def _clipped(w2):
    """A 1x2 image under a 1x3 SAME filter (pad 1 / 1).  Output 1 takes taps 0 and 1 -- fmaf(1e-30, -1e-30, +0.0) = -0.0, then
    fmaf(1e-30, -1e-30, -0.0) = -0.0 -- and its tap 2 lies in the padding: SKIPPED, the -0.0 stays.  Read as x = +0.0 it would
    give +0.0 for w2 > 0, as x = -0.0 for w2 < 0, and NaN for an infinite w2.  Output 0 takes taps 1 and 2:
    fmaf(1e-30, w2, -0.0) = 1e-30 w2, an infinity clamped to FLT_MAX (the range of NONE)."""
    x = f(TINY, TINY).reshape(1, 1, 2, 1)
    w = f(-TINY, -TINY, w2).reshape(1, 1, 3, 1)
    with np.errstate(over="ignore"):
        first = min(np.float32(TINY * np.float32(w2)), R.FLOAT_RANGE[NONE][1])
    return x, w, None, dict(stride=1, padding=SAME), np.array([first, MINUS_ZERO], np.float32).reshape(1, 1, 2, 1)


KNOWN = {
    # 1e8 + 1 rounds back to 1e8 (the grid there is 8), minus 1e8 is 0; the taps in any order that ends with the 1 give 1
    "tap_order_along_a_row": lambda: (f(1e8, 1, -1e8).reshape(1, 1, 3, 1), np.ones((1, 1, 3, 1), np.float32), None,
                                      dict(stride=1, padding=VALID), f(0).reshape(1, 1, 1, 1)),
    # raster order: 1e8 - 1e8 = 0, + 1 = 1, + 0; column-major order would go 1e8 + 1 = 1e8, - 1e8 = 0
    "tap_order_rows_then_columns": lambda: (f(1e8, -1e8, 1, 0).reshape(1, 2, 2, 1), np.ones((1, 2, 2, 1), np.float32), None,
                                            dict(stride=1, padding=VALID), f(1).reshape(1, 1, 1, 1)),
    # within a tap the channels in order: 1e8 - 1e8 + 1 = 1; then the second tap's 0 0 4: 5
    "channels_in_order_within_a_tap": lambda: (f(1e8, -1e8, 1, 0, 0, 4).reshape(1, 1, 2, 3), np.ones((1, 1, 2, 3), np.float32), None,
                                               dict(stride=1, padding=VALID), f(5).reshape(1, 1, 1, 1)),
    # w[fy][fx] = 2^(3 fy + fx) on ones: a sum names its taps.  The corner (0, 0) has taps (1,1) (1,2) (2,1) (2,2) = 16 + 32 +
    # 128 + 256; rows {1,2} {0,1,2} {0,1} give 72, 73, 9, columns {1,2} {0,1,2} {0,1} give 6, 7, 3
    "which_taps_a_corner_uses": lambda: (np.ones((1, 3, 3, 1), np.float32), (2.0 ** np.arange(9)).reshape(1, 3, 3, 1).astype(np.float32),
                                         None, dict(stride=1, padding=SAME),
                                         np.outer([72, 73, 9], [6, 7, 3]).astype(np.float32).reshape(1, 3, 3, 1)),
    # 4 rows, filter 3, stride 2: 2 outputs, total padding (2 - 1) 2 + 3 - 4 = 1, NONE in front and 1 behind.  Output 0 reads
    # rows 0 1 2 = 1 + 20 + 400, output 1 rows 2 3 and the padding = 4 + 80 (pad 1 in front would give 10 + 200 first)
    "pad_before_is_total_over_two": lambda: (f(1, 2, 4, 8).reshape(1, 4, 1, 1), f(1, 10, 100).reshape(1, 3, 1, 1), None,
                                             dict(stride=2, padding=SAME), f(421, 84).reshape(1, 2, 1, 1)),
    "minus_zero_before_a_clipped_tap_with_a_negative_weight": lambda: _clipped(-1.0),
    "minus_zero_before_a_clipped_tap_with_a_positive_weight": lambda: _clipped(1.0),
    "minus_zero_before_a_clipped_tap_with_an_infinite_weight": lambda: _clipped(np.inf),
    # K = 1 on an unclipped window: the steps beyond K must leave the -0.0 alone
    "minus_zero_across_the_k_tail": lambda: (f(TINY).reshape(1, 1, 1, 1), f(-TINY).reshape(1, 1, 1, 1), None,
                                             dict(stride=1, padding=VALID), np.array([MINUS_ZERO], np.float32).reshape(1, 1, 1, 1)),
    # the same through 3 x 3 x 3 = 27 steps (a K tail of 5) with a bias of -0.0: -0.0 + -0.0 = -0.0
    "minus_zero_through_27_steps_and_a_bias": lambda: (np.full((1, 3, 3, 3), TINY), np.full((1, 3, 3, 3), -TINY), np.array([MINUS_ZERO]),
                                                       dict(stride=1, padding=VALID), np.array([MINUS_ZERO], np.float32).reshape(1, 1, 1, 1)),
}


def known_case(name):
    x, w, bias, kw, want = KNOWN[name]()
    return (np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32),
            None if bias is None else np.ascontiguousarray(bias, np.float32), kw, np.ascontiguousarray(want, np.float32))


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers_on_the_reference(name):
    x, w, bias, kw, want = known_case(name)
    got = R.conv2d(x, w, bias, (kw["stride"],) * 2, kw["padding"])
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    if name.startswith("minus_zero_before"):
        assert got.view(np.uint32)[0, 0, 1, 0] == 0x80000000 and not np.isnan(got).any()


def test_the_padding_rule_of_the_stems():
    assert PR.out_and_pad(4, 3, 2, SAME) == (2, 0) and (2 - 1) * 2 + 3 - 4 - 0 == 1
    assert PR.out_and_pad(224, 7, 2, SAME) == (112, 2) and (112 - 1) * 2 + 7 - 224 - 2 == 3
    assert PR.out_and_pad(224, 3, 2, SAME) == (112, 0) and PR.out_and_pad(227, 11, 4, VALID) == (55, 0)
    oh, ow = C.c_int32(), C.c_int32()
    d = _desc(in_height=224, in_width=227, channels_in=3, filter_height=7, filter_width=11, stride_height=2, stride_width=4)
    assert amd.lib().lce_hip_conv2d_f32_check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (112, 57)


# ---- the fixtures of the GPU side -----------------------------------------------------------------------------------------------
def _stem_conv(b, g, src, cin, cout, filt, name):
    w = (g.standard_normal((cout, *filt, cin)) * 0.3).astype(np.float32)
    wb = g.standard_normal(cout).astype(np.float32)
    return w, wb, [src, b.tensor([cout, *filt, cin], np.float32, name, w), b.tensor([cout], np.float32, name + "b", wb)]


def _out(size, filt, stride, padding):
    return PR.out_and_pad(size, filt, stride, padding)[0]


def quicknet_stem_model(seed=0, first="conv", size=16):
    """QuickNet's stem and its first binary layer: x 16x16x3 -> CONV_2D 3x3 / 2 SAME RELU (3 -> 32) -> DEPTHWISE_CONV_2D 3x3 / 2
    SAME -> CONV_2D 1x1 (32 -> 64, bias) -> LceQuantize -> LceBconv2d (3x3, float: the graph output).  first="pool": a MAX_POOL_2D
    3x3 / 2 SAME on x 16x16x32 stands where the 3x3 convolution does (a stem the parent's kernels cover).  Returns (file, input
    tensor, output tensor, info); info["host"]: operator index -> what the host computes for it from its non-constant inputs;
    info["stem_ops"]: the stem operators in order, as (kind, constants and options...), for a host that runs them itself.  `size`:
    the input extent (tools/conv2d_sections.py measures at 224)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 701)
    C1, C2 = 32, 64
    host = {}
    h1 = _out(size, 3, 2, SAME)
    h2 = _out(h1, 3, 2, SAME)
    if first == "conv":
        x = f32([1, size, size, 3], "x")
        w0, b0, ins = _stem_conv(b, g, x, 3, C1, (3, 3), "w0")
        s = f32([1, h1, h1, C1], "s")
        k0 = conv2d_op(b, ins, [s], (2, 2), SAME, RELU)
        host[k0] = lambda v: R.conv2d(v, w0, b0, (2, 2), SAME, RELU)
        stem_ops = [("conv", w0, b0, 2, SAME, RELU)]
    else:
        x = f32([1, size, size, C1], "x")
        s = f32([1, h1, h1, C1], "s")
        k0 = pool_op(b, MAX_POOL_2D, [x], [s], (3, 3), (2, 2), SAME)
        host[k0] = lambda v: PR.pool2d(v, PR.MAX, (3, 3), (2, 2), PR.SAME)
        stem_ops = [("pool", 3, 2, SAME)]
    k = (g.standard_normal((1, 3, 3, C1)) * 0.4).astype(np.float32)
    d = f32([1, h2, h2, C1], "d")
    dw = depthwise_op(b, [s, f32([1, 3, 3, C1], "k", k)], [d], (2, 2), SAME)
    w1 = (g.standard_normal((C2, 1, 1, C1)) * 0.2).astype(np.float32)
    b1 = g.standard_normal(C2).astype(np.float32)
    t = f32([1, h2, h2, C2], "t")
    pw = conv2d_op(b, [d, f32([C2, 1, 1, C1], "w1", w1), f32([C2], "b1", b1)], [t], (1, 1), SAME)
    q = b.tensor([1, h2, h2, C2 // 32], np.int32, "q")
    b.custom_op("LceQuantize", [t], [q], b"")
    y, c0 = _conv(b, q, h2, C2, C2, seed * 10 + 1)
    stem_ops += [("depthwise", k, 2, SAME), ("conv", w1, b1, 1, SAME, NONE)]
    b.inputs, b.outputs = [x], [y]
    host.update({dw: lambda v: DR.depthwise(v, k, None, (2, 2), SAME), pw: lambda v: CR.conv1x1(v, w1, b1)})
    info = dict(host=host, stem=[k0, dw, pw], conv2d=[k0] if first == "conv" else [], convs=[c0], tensors=dict(s=s, d=d, t=t),
                shape=(size, size, 3 if first == "conv" else C1), stem_ops=stem_ops,
                stats=dict(conv2d=(1, 0) if first == "conv" else (0, 0), conv1x1=(1, 1), depthwise=(1, 0), pool=(0, 0) if first == "conv" else (1, 0)),
                parent_sections=[[3, 4]])
    return b.finish(), x, y, info


def bireal_stem_model(seed=0, size=18):
    """Bi-RealNet's stem and first block: x 18x18x3 -> CONV_2D 7x7 / 2 SAME (3 -> 64) -> MUL (c) -> ADD (c) -> MAX_POOL_2D 3x3 / 2
    SAME -> p; p -> LceQuantize -> LceBconv2d (3x3, float) -> MUL (c) -> ADD (c) -> ADD (p): the shortcut, the graph output."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 801)
    Cc = 64
    h1 = _out(size, 7, 2, SAME)
    h2 = _out(h1, 3, 2, SAME)
    x = f32([1, size, size, 3], "x")
    w0, b0, ins = _stem_conv(b, g, x, 3, Cc, (7, 7), "w0")
    s = f32([1, h1, h1, Cc], "s")
    k0 = conv2d_op(b, ins, [s], (2, 2), SAME, NONE)
    m0, a0 = g.uniform(0.5, 1.5, Cc).astype(np.float32), g.standard_normal(Cc).astype(np.float32)
    sm, sa, p = f32([1, h1, h1, Cc], "sm"), f32([1, h1, h1, Cc], "sa"), f32([1, h2, h2, Cc], "p")
    mul0 = ew_op(b, MUL, [s, f32([Cc], "m0", m0)], [sm], NONE)
    add0 = ew_op(b, ADD, [sm, f32([Cc], "a0", a0)], [sa], NONE)
    pool = pool_op(b, MAX_POOL_2D, [sa], [p], (3, 3), (2, 2), SAME)
    q = b.tensor([1, h2, h2, Cc // 32], np.int32, "q")
    b.custom_op("LceQuantize", [p], [q], b"")
    y, c0 = _conv(b, q, h2, Cc, Cc, seed * 10 + 2)
    m1, a1 = g.uniform(0.5, 1.5, Cc).astype(np.float32), g.standard_normal(Cc).astype(np.float32)
    ym, ya, out = f32([1, h2, h2, Cc], "ym"), f32([1, h2, h2, Cc], "ya"), f32([1, h2, h2, Cc], "out")
    mul1 = ew_op(b, MUL, [y, f32([Cc], "m1", m1)], [ym], NONE)
    add1 = ew_op(b, ADD, [ym, f32([Cc], "a1", a1)], [ya], NONE)
    res = ew_op(b, ADD, [ya, p], [out], NONE)
    b.inputs, b.outputs = [x], [out]
    host = {k0: lambda v: R.conv2d(v, w0, b0, (2, 2), SAME), mul0: lambda v: float_op(v, MUL, m0, NONE),
            add0: lambda v: float_op(v, ADD, a0, NONE), pool: lambda v: PR.pool2d(v, PR.MAX, (3, 3), (2, 2), PR.SAME)}
    stem_ops = [("conv", w0, b0, 2, SAME, NONE), ("mul", m0), ("add", a0), ("pool", 3, 2, SAME)]
    info = dict(host=host, stem=[k0, mul0, add0, pool], conv2d=[k0], convs=[c0], tensors=dict(s=s, p=p), shape=(size, size, 3), stem_ops=stem_ops,
                stats=dict(conv2d=(1, 0), conv1x1=(0, 0), depthwise=(0, 0), pool=(1, 1)), parent_sections=[[4, 5, 6, 7, 8]],
                body=dict(m=m1, a=a1, mul=mul1, add=add1, res=res))
    return b.finish(), x, out, info


def alexnet_stem_model(seed=0, size=27):
    """BinaryAlexNet's stem and first binary layer: x 27x27x3 -> CONV_2D 11x11 / 4 VALID (3 -> 64) -> MAX_POOL_2D 3x3 / 2 VALID ->
    MUL (c) -> ADD (c) -> LceQuantize -> LceBconv2d (3x3, float: the graph output)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 901)
    Cc = 64
    h1 = _out(size, 11, 4, VALID)
    h2 = _out(h1, 3, 2, VALID)
    x = f32([1, size, size, 3], "x")
    w0, b0, ins = _stem_conv(b, g, x, 3, Cc, (11, 11), "w0")
    s = f32([1, h1, h1, Cc], "s")
    k0 = conv2d_op(b, ins, [s], (4, 4), VALID, NONE)
    p, pm, pa = f32([1, h2, h2, Cc], "p"), f32([1, h2, h2, Cc], "pm"), f32([1, h2, h2, Cc], "pa")
    pool = pool_op(b, MAX_POOL_2D, [s], [p], (3, 3), (2, 2), VALID)
    m0, a0 = g.uniform(-1.5, 1.5, Cc).astype(np.float32), g.standard_normal(Cc).astype(np.float32)
    mul0 = ew_op(b, MUL, [p, f32([Cc], "m0", m0)], [pm], NONE)
    add0 = ew_op(b, ADD, [pm, f32([Cc], "a0", a0)], [pa], NONE)
    q = b.tensor([1, h2, h2, Cc // 32], np.int32, "q")
    b.custom_op("LceQuantize", [pa], [q], b"")
    y, c0 = _conv(b, q, h2, Cc, Cc, seed * 10 + 3)
    b.inputs, b.outputs = [x], [y]
    host = {k0: lambda v: R.conv2d(v, w0, b0, (4, 4), VALID), pool: lambda v: PR.pool2d(v, PR.MAX, (3, 3), (2, 2), PR.VALID),
            mul0: lambda v: float_op(v, MUL, m0, NONE), add0: lambda v: float_op(v, ADD, a0, NONE)}
    stem_ops = [("conv", w0, b0, 4, VALID, NONE), ("pool", 3, 2, VALID), ("mul", m0), ("add", a0)]
    info = dict(host=host, stem=[k0, pool, mul0, add0], conv2d=[k0], convs=[c0], tensors=dict(s=s, p=p), shape=(size, size, 3), stem_ops=stem_ops,
                stats=dict(conv2d=(1, 0), conv1x1=(0, 0), depthwise=(0, 0), pool=(1, 0)), parent_sections=[[4, 5]])
    return b.finish(), x, y, info


def float3x3_in_body_model(seed=0):
    """A float 3x3 convolution between binary layers: x 8x8x64 -> LceQuantize -> LceBconv2d (float) -> CONV_2D 3x3 SAME
    (64 -> 40, bias, signed results) -> LceQuantize, the graph output.  The convolution feeds ONLY the LceQuantize."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 1001)
    Cc, Co = 64, 40
    x = f32([1, 8, 8, Cc], "x")
    q0 = b.tensor([1, 8, 8, Cc // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y, c0 = _conv(b, q0, 8, Cc, Cc, seed * 10 + 4)
    w0, b0, ins = _stem_conv(b, g, y, Cc, Co, (3, 3), "w0")
    z = f32([1, 8, 8, Co], "z")
    k0 = conv2d_op(b, ins, [z], (1, 1), SAME, NONE)
    q1 = b.tensor([1, 8, 8, 2], np.int32, "q1")
    b.custom_op("LceQuantize", [z], [q1], b"")
    b.inputs, b.outputs = [x], [q1]
    info = dict(host={k0: lambda v: R.conv2d(v, w0, b0, (1, 1), SAME)}, stem=[], conv2d=[k0], convs=[c0], tensors=dict(z=z),
                shape=(8, 8, Cc), stats=dict(conv2d=(1, 1), conv1x1=(0, 0), depthwise=(0, 0), pool=(0, 0)), parent_sections=[[0, 1], [3]])
    return b.finish(), x, q1, info


STEMS = dict(quicknet=quicknet_stem_model, bireal=bireal_stem_model, alexnet=alexnet_stem_model)
FIXTURES = dict(float3x3=float3x3_in_body_model, **STEMS)


# ---- the partition --------------------------------------------------------------------------------------------------------------
def _parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_each_fixture_is_one_section_with_every_flag(name):
    data, x, out, info = FIXTURES[name]()
    model = mr.LceModel(data, **ALL_FLAGS)
    n_ops = len(model.operators)
    for k in info["conv2d"]:
        assert model.operators[k].builtin_code == CONV_2D
    assert _parts(model) == [(list(range(n_ops)), [x], [out])] and model.inputs == [x]
    assert mr.Interpreter(model).lce_only and mr.Interpreter(data, **ALL_FLAGS).lce_only
    every = mr.LceModel(data, int8_add_sections=True, concat_sections=True, **ALL_FLAGS)
    assert _parts(every) == _parts(model)
    # the parent's flags give the parent's partition: the stem is the host's, the body a section
    parent = mr.LceModel(data, **PARENT_FLAGS)
    assert [s.ops for s in parent.sections] == info["parent_sections"] and not mr.Interpreter(parent).lce_only
    for s in parent.sections:
        assert not set(s.ops) & set(info["stem"]) and not set(s.ops) & set(info["conv2d"])


def test_the_float_3x3_in_the_body_needs_the_conv2d_bit_alone():
    data, x, out, info = float3x3_in_body_model()
    (k,) = info["conv2d"]
    alone = mr.LceModel(data, conv2d_sections=True)
    assert _parts(alone) == [([0, 1, 2, 3], [x], [out])] and mr.Interpreter(alone).lce_only
    # the 1x1 bit does not take a 3x3 filter, and the stem bit is no candidate rule of its own
    for kw in (dict(conv1x1_sections=True), dict(stem_sections=True), PARENT_FLAGS, dict(stem_sections=True, **PARENT_FLAGS)):
        assert [s.ops for s in mr.LceModel(data, **kw).sections] == [[0, 1], [3]], kw


def test_stem_without_conv2d_leaves_a_3x3_stem_with_the_host_but_joins_a_stem_the_parents_kernels_cover():
    data, x, out, info = quicknet_stem_model()
    parent = _parts(mr.LceModel(data, **PARENT_FLAGS))
    # the 3x3 convolution is no candidate: it opens a builtin epoch, and what it feeds becomes ready there
    assert _parts(mr.LceModel(data, stem_sections=True, **PARENT_FLAGS)) == parent == [([3, 4], [info["tensors"]["t"]], [out])]
    # CONV2D without STEM: ready from the start is the host's
    assert _parts(mr.LceModel(data, conv2d_sections=True, **PARENT_FLAGS)) == parent
    # a stem of pool, depthwise and 1x1 alone joins under STEM, and only under STEM
    data, x, out, info = quicknet_stem_model(first="pool")
    joined = mr.LceModel(data, stem_sections=True, **PARENT_FLAGS)
    assert _parts(joined) == [([0, 1, 2, 3, 4], [x], [out])] and mr.Interpreter(joined).lce_only
    assert [s.ops for s in mr.LceModel(data, **PARENT_FLAGS).sections] == [[3, 4]]
    # STEM alone enables nothing: no operator is a candidate
    assert [s.ops for s in mr.LceModel(data, stem_sections=True).sections] == [[3, 4]]
    # only the enabled opt-ins count: without the depthwise bit the pool joins, the blur cuts, the 1x1 goes with the host
    part = mr.LceModel(data, stem_sections=True, elementwise_sections=True, pool_sections=True, conv1x1_sections=True)
    assert [s.ops for s in part.sections] == [[0], [3, 4]]


def test_a_stem_operator_that_is_no_candidate_still_opens_a_builtin_epoch():
    """x (uint8-like: int8 here) cannot feed the float convolution: a QUANTIZE-like foreign operator in front.  Built as a TANH
    convolution (no candidate) in front of a qualifying 3x3: the first is the host's, the second becomes ready in the builtin
    epoch and goes with it; the binary layer is the section."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(5)
    x = f32([1, 8, 8, 3], "x")
    _, _, ins = _stem_conv(b, g, x, 3, 8, (3, 3), "wa")
    a = f32([1, 8, 8, 8], "a")
    conv2d_op(b, ins, [a], (1, 1), SAME, TANH)
    _, _, ins = _stem_conv(b, g, a, 8, 64, (3, 3), "wb")
    s = f32([1, 8, 8, 64], "s")
    conv2d_op(b, ins, [s], (1, 1), SAME, NONE)
    q = b.tensor([1, 8, 8, 2], np.int32, "q")
    b.custom_op("LceQuantize", [s], [q], b"")
    y, _ = _conv(b, q, 8, 64, 64, 9)
    b.inputs, b.outputs = [x], [y]
    model = mr.LceModel(b.finish(), **ALL_FLAGS)
    assert [s_.ops for s_ in model.sections] == [[2, 3]] and not mr.Interpreter(model).lce_only


def test_files_without_a_qualifying_operator_keep_their_partitions():
    for data in (dense_block_model()[0], mixed_model()[0], alexnet_body_model()[0], bireal_block_model()[0], quicknet_transition_model()[0]):
        for kw in ({}, dict(elementwise_sections=True), dict(concat_sections=True, **PARENT_FLAGS)):
            want = _parts(mr.LceModel(data, **kw))
            assert _parts(mr.LceModel(data, conv2d_sections=True, **kw)) == want
            assert _parts(mr.LceModel(data, conv2d_sections=True, stem_sections=True, **kw)) == want


# ---- every condition of the candidate rule -----------------------------------------------------------------------------------------
JOINS = ["joins", "no_bias_two_inputs", "no_bias_minus_one", "stride_2", "stride_3_1", "valid", "relu6", "no_dilations", "filter_1x1",
         "filter_5x2", "filter_larger_than_the_image"]
STAYS = ["one_input", "four_inputs", "two_outputs", "int8_input", "int8_filter", "int8_output", "int32_bias", "three_d_output",
         "three_d_input", "constant_input", "filter_not_constant", "filter_3_d", "filter_zero_height", "grouped_filter",
         "filter_bytes", "bias_not_constant", "bias_length", "bias_2_d", "output_channels", "no_options", "zero_stride",
         "negative_stride", "huge_stride", "dilation_w", "dilation_h", "padding_2", "tanh", "sign_bit", "extent_off_by_one",
         "valid_extent_as_same", "depthwise_code"]


def _graph(case):
    """x -> LceQuantize -> LceBconv2d -> y -> <CONV_2D under test> -> z -> LceQuantize -> q2, with one condition of the
    candidate rule broken per case of STAYS.  Returns (file, index of the convolution)."""
    Hh, Cc, Co = 8, 64, 32
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i8 = lambda shape, name, data=None: b.tensor(shape, np.int8, name, None if data is None else data.astype(np.int8), scale=0.5, zero_point=1)
    i32 = lambda shape, name, data=None: b.tensor(shape, np.int32, name, None if data is None else data.astype(np.int32))
    ones = lambda make, shape, name: make(shape, name, np.ones(shape, np.float32))
    x = f32([1, Hh, Hh, Cc], "x")
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    y = (i8 if case == "int8_input" else f32)([Hh, Hh, Cc] if case == "three_d_input" else [1, Hh, Hh, Cc], "y")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y], bconv_options(spec))
    src = ones(f32, [1, Hh, Hh, Cc], "c") if case == "constant_input" else y
    kw, zshape, code, fshape = {}, [1, Hh, Hh, Co], CONV_2D, [Co, 3, 3, Cc]
    if case == "stride_2":
        kw, zshape = dict(stride=(2, 2)), [1, 4, 4, Co]
    elif case == "stride_3_1":
        kw, zshape = dict(stride=(3, 1)), [1, 3, 8, Co]
    elif case == "valid":
        kw, zshape = dict(padding=VALID), [1, 6, 6, Co]
    elif case == "relu6":
        kw = dict(activation=RELU6)
    elif case == "no_dilations":
        kw = dict(dilation=None)
    elif case == "filter_1x1":
        fshape = [Co, 1, 1, Cc]
    elif case == "filter_5x2":
        fshape = [Co, 5, 2, Cc]
    elif case == "filter_larger_than_the_image":
        fshape = [Co, 11, 9, Cc]
    elif case == "filter_3_d":
        fshape = [Co, 9, Cc]
    elif case == "filter_zero_height":
        fshape = [Co, 0, 3, Cc]
    elif case == "grouped_filter":
        fshape = [Co, 3, 3, Cc // 2]
    elif case == "output_channels":
        zshape = [1, Hh, Hh, Co + 1]
    elif case == "three_d_output":
        zshape = [Hh, Hh, Co]
    elif case == "no_options":
        kw = dict(options=False)
    elif case == "zero_stride":
        kw = dict(stride=(0, 1))
    elif case == "negative_stride":
        kw = dict(stride=(1, -1))
    elif case == "huge_stride":
        kw, zshape = dict(stride=(2 ** 30 + 1, 1)), [1, 1, Hh, Co]
    elif case == "dilation_w":
        kw = dict(dilation=(1, 2))
    elif case == "dilation_h":
        kw = dict(dilation=(2, 1))
    elif case == "padding_2":
        kw = dict(padding=2)
    elif case == "tanh":
        kw = dict(activation=TANH)
    elif case == "sign_bit":
        kw = dict(activation=SIGN_BIT)
    elif case == "extent_off_by_one":
        zshape = [1, Hh, Hh - 1, Co]
    elif case == "valid_extent_as_same":
        kw = dict(padding=VALID)                              # VALID gives 6 x 6; the file says 8 x 8
    elif case == "depthwise_code":
        code = DEPTHWISE_CONV_2D
    if case == "filter_not_constant":
        flt = f32(fshape, "k")
    elif case == "filter_bytes":                             # written as 3 x 2; the file's shape is patched to 3 x 3 below
        flt = b.tensor([Co, 3, 2, Cc], np.float32, "k", np.ones([Co, 3, 2, Cc], np.float32))
    else:
        flt = ones(i8 if case == "int8_filter" else f32, fshape, "k")
    kb = ones(f32, [Co], "kb")
    if case == "int32_bias":
        kb = ones(i32, [Co], "kb")
    elif case == "bias_not_constant":
        kb = f32([Co], "kb")
    elif case == "bias_length":
        kb = ones(f32, [Co - 1], "kb")
    elif case == "bias_2_d":
        kb = ones(f32, [1, Co], "kb")
    ins = [src, flt, kb]
    if case == "no_bias_two_inputs":
        ins = [src, flt]
    elif case == "no_bias_minus_one":
        ins = [src, flt, -1]
    elif case == "one_input":
        ins = [src]
    elif case == "four_inputs":
        ins = [src, flt, kb, kb]
    z = (i8 if case == "int8_output" else f32)(zshape, "z")
    outs = [z, f32(zshape, "z2")] if case == "two_outputs" else [z]
    k = conv2d_op(b, ins, outs, code=code, **kw)
    words = (zshape[-1] + 31) // 32
    q2 = b.tensor(zshape[:-1] + [words], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = [x], [q2]
    data = b.finish()
    if case == "filter_bytes":
        shape = struct.pack("<5i", 4, Co, 3, 2, Cc)
        assert data.count(shape) == 1
        data = data.replace(shape, struct.pack("<5i", 4, Co, 3, 3, Cc))
    return data, k


@pytest.mark.parametrize("case", STAYS)
def test_convolutions_that_stay_with_the_host(case):
    data, k = _graph(case)
    plain = _parts(mr.LceModel(data))
    for kw in (dict(conv2d_sections=True), ALL_FLAGS):
        try:
            model = mr.LceModel(data, **kw)
        except ValueError:                                   # (a file the reader itself refuses stays with nobody)
            assert case in ("filter_zero_height", "filter_bytes", "three_d_input")
            continue
        assert all(k not in s.ops for s in model.sections), (case, kw)
        if kw == dict(conv2d_sections=True):
            assert _parts(model) == plain


@pytest.mark.parametrize("case", JOINS)
def test_a_qualifying_convolution_joins(case):
    data, k = _graph(case)
    model = mr.LceModel(data, conv2d_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]
    assert [s.ops for s in mr.LceModel(data, **PARENT_FLAGS).sections] == ([[0, 1, 2, 3]] if case == "filter_1x1" else [[0, 1], [3]])


def test_a_1x1_filter_goes_to_the_1x1_entry_first_and_to_the_new_one_alone():
    """Precedence: with both bits a 1x1 filter is absorbed as before (kAbsorbedConv1x1: conv1x1_stats counts it on the GPU side);
    with CONV2D alone it is absorbed too.  Either way the partition is one section, and the walks infer the same shapes."""
    data, k = _graph("filter_1x1")
    both = mr.LceModel(data, conv1x1_sections=True, conv2d_sections=True)
    alone = mr.LceModel(data, conv2d_sections=True)
    old = mr.LceModel(data, conv1x1_sections=True)
    assert _parts(both) == _parts(alone) == _parts(old) == [([0, 1, 2, 3], [0], [both.outputs[0]])]
    for m in (both, alone, old):
        assert m.section_tensor_shape(0, m.operators[k].outputs[0], 3)[0] == (3, 8, 8, 32)


# ---- shape inference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
def test_section_tensor_shape_over_the_stem_tensors(batch):
    want = dict(quicknet=dict(s=(8, 8, 32), d=(4, 4, 32), t=(4, 4, 64)), bireal=dict(s=(9, 9, 64), p=(5, 5, 64)),
                alexnet=dict(s=(5, 5, 64), p=(2, 2, 64)), float3x3=dict(z=(8, 8, 40)))
    for name, make in FIXTURES.items():
        data, x, out, info = make()
        model = mr.LceModel(data, **ALL_FLAGS)
        assert model.section_tensor_shape(0, x, batch)[0] == (batch,) + info["shape"]
        for t, hwc in want[name].items():
            n = int(np.prod(hwc))
            assert model.section_tensor_shape(0, info["tensors"][t], batch) == ((batch,) + hwc, batch * n * 4), (name, t)
    for case, hwc in (("stride_2", (4, 4, 32)), ("stride_3_1", (3, 8, 32)), ("valid", (6, 6, 32)), ("filter_5x2", (8, 8, 32)),
                      ("filter_larger_than_the_image", (8, 8, 32))):
        data, k = _graph(case)
        model = mr.LceModel(data, conv2d_sections=True)
        assert model.section_tensor_shape(0, model.operators[k].outputs[0], batch)[0] == (batch,) + hwc
        assert model.section_tensor_shape(0, model.outputs[0], batch)[0] == (batch,) + hwc[:2] + (1,)


@pytest.mark.parametrize("declared", [32, 96])
def test_a_file_whose_conv_input_disagrees_with_the_inferred_shape_is_refused(declared):
    """The convolution's tensors agree with each other in the file, but the binary convolution produces 64 channels where the
    file declares `declared` for its output: the walk must fail instead of reading past (or short of) its buffer."""
    Hh, Cc = 8, 64
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x, y, z = f32([1, Hh, Hh, Cc], "x"), f32([1, Hh, Hh, declared], "y"), f32([1, Hh, Hh, 8], "z")
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y], bconv_options(spec))
    conv2d_op(b, [y, f32([8, 3, 3, declared], "k", np.ones((8, 3, 3, declared), np.float32))], [z])
    b.inputs, b.outputs = [x], [z]
    model = mr.LceModel(b.finish(), conv2d_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2]]
    with pytest.raises(amd.LceHipError, match="CONV_2D input") as e:
        model.section_tensor_shape(0, z, 2)
    assert e.value.code == amd.ERR_INVALID


# ---- lce_hip_conv2d_f32 / amd.conv2d argument checks (no device needed: they come first) ------------------------------------------
def _desc(**kw):
    d = dict(batch=2, in_height=8, in_width=8, channels_in=64, channels_out=32, filter_height=3, filter_width=3, stride_height=1,
             stride_width=1, padding=amd.PADDING_SAME, activation=amd.ACT_NONE)
    d.update(kw)
    return Conv2dDesc(*[d[n] for n, _ in Conv2dDesc._fields_])


# the input is 2 x 8 x 8 x 64 floats = 32 KiB at 65536, the filter 32 x 3 x 3 x 64 floats = 73728 bytes, the bias 128 bytes, the
# output 2 x 8 x 8 x 32 floats = 16 KiB, the bits 2 x 8 x 8 x 1 words = 512 bytes
PTRS = dict(inp=1 << 16, flt=1 << 18, bias=1 << 19, out=1 << 20, bits=1 << 21)
FAR = dict(inp=1 << 40, flt=1 << 46, out=1 << 54, bits=1 << 60)


def _c_call(desc=True, **kw):
    p = dict(PTRS)
    p.update({k: kw.pop(k) for k in list(kw) if k in PTRS})
    d = _desc(**kw)
    return amd.lib().lce_hip_conv2d_f32(C.byref(d) if desc else None, *[C.c_void_p(p[k]) for k in ("inp", "flt", "bias", "out", "bits")], None)


REFUSALS = [
    (dict(desc=False), amd.ERR_INVALID, "null desc"),
    (dict(inp=0), amd.ERR_INVALID, "null input"),
    (dict(flt=0), amd.ERR_INVALID, "null filter"),
    (dict(out=0, bits=0), amd.ERR_INVALID, "both outputs"),
    (dict(batch=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_height=-1), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_width=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(channels_in=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(channels_out=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(filter_height=0), amd.ERR_INVALID, "filter must be positive"),
    (dict(filter_width=-1), amd.ERR_INVALID, "filter must be positive"),
    (dict(stride_height=0), amd.ERR_INVALID, "stride must be positive"),
    (dict(stride_width=-1), amd.ERR_INVALID, "stride must be positive"),
    (dict(padding=2), amd.ERR_INVALID, "padding must be"),
    (dict(padding=-1), amd.ERR_INVALID, "padding must be"),
    (dict(activation=4), amd.ERR_INVALID, "unknown activation"),
    (dict(activation=-1), amd.ERR_INVALID, "unknown activation"),
    (dict(padding=amd.PADDING_VALID, filter_height=9), amd.ERR_INVALID, "empty output"),
    (dict(padding=amd.PADDING_VALID, filter_width=9), amd.ERR_INVALID, "empty output"),
    (dict(batch=2 ** 20, in_height=2 ** 6, in_width=2 ** 6, channels_in=1, channels_out=1, filter_height=1, filter_width=1, **FAR),
     amd.ERR_UNSUPPORTED, "2\\^31 pixels"),
    (dict(stride_height=2 ** 31 - 1, stride_width=2 ** 31 - 1), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(stride_width=2 ** 30 + 1), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(batch=1, channels_in=1, in_height=2 ** 30 + 1, in_width=1, stride_height=2, **FAR), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(filter_height=2 ** 15, filter_width=2 ** 15, channels_in=2, **FAR), amd.ERR_UNSUPPORTED, "2\\^31 or more elements"),
    (dict(filter_height=1, filter_width=2, channels_in=2 ** 30, batch=1, in_height=1, in_width=1, **FAR), amd.ERR_UNSUPPORTED, "2\\^31 or more elements"),
    (dict(filter_height=2 ** 31 - 1, filter_width=2 ** 31 - 1, channels_in=1, **FAR), amd.ERR_UNSUPPORTED, "2\\^31 or more elements"),
    (dict(channels_out=65535 * 128 + 1, channels_in=1, **FAR), amd.ERR_UNSUPPORTED, "output channels"),
    (dict(out=(1 << 16) + 512), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=(1 << 16) - 16), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=0, bits=(1 << 16) + 32768 - 4), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=(1 << 18) + 73728 - 4), amd.ERR_INVALID, "overlaps the filter"),
    (dict(out=0, bits=(1 << 18) - 508), amd.ERR_INVALID, "overlaps the filter"),
    (dict(out=(1 << 19) - 16380), amd.ERR_INVALID, "overlaps the bias"),
    (dict(out=0, bits=(1 << 19) + 124), amd.ERR_INVALID, "overlaps the bias"),
    (dict(bits=(1 << 20) + 16380), amd.ERR_INVALID, "outputs overlap"),
    (dict(bits=(1 << 21) + 2), amd.ERR_INVALID, "4-byte aligned"),
    (dict(inp=(1 << 16) + 1), amd.ERR_INVALID, "4-byte aligned"),
    (dict(flt=(1 << 18) + 1), amd.ERR_INVALID, "4-byte aligned"),
    (dict(bias=(1 << 19) + 2), amd.ERR_INVALID, "4-byte aligned"),
    (dict(out=(1 << 20) + 3), amd.ERR_INVALID, "4-byte aligned"),
]


@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_c_entry_refuses_bad_arguments(kw, code, msg):
    assert _c_call(**dict(kw)) == code
    assert re.search(msg, amd.lib().lce_hip_last_error().decode()), amd.lib().lce_hip_last_error()


def test_c_entry_accepts_the_edges_of_the_checks_up_to_the_device():
    """Touching ranges do not overlap; a NULL bias, either output alone, the largest stride, a filter of 2^30 elements per
    channel, the last channel count the grid reaches and every activation pass.  Without a device the accepted calls end at
    ERR_NO_DEVICE; none of them is ERR_INVALID or ERR_UNSUPPORTED."""
    edges = (dict(out=(1 << 16) + 32768), dict(out=(1 << 16) - 16384), dict(bits=(1 << 20) + 16384), dict(out=0), dict(bits=0), dict(bias=0),
             dict(out=(1 << 18) + 73728), dict(out=(1 << 19) + 128), dict(bias=0, out=1 << 19),   # (no bias: nothing there to overlap)
             dict(stride_height=2 ** 30, stride_width=2 ** 30), dict(inp=(1 << 16) + 4, flt=(1 << 18) + 4, out=(1 << 20) + 12),
             dict(activation=amd.ACT_RELU), dict(activation=amd.ACT_RELU_N1_TO_1), dict(activation=amd.ACT_RELU6),
             dict(padding=amd.PADDING_VALID, filter_height=8, filter_width=8), dict(channels_in=1), dict(channels_out=1),
             dict(filter_height=11, filter_width=9, **FAR), dict(channels_out=65535 * 128, channels_in=1, **FAR),
             dict(filter_height=2 ** 15, filter_width=2 ** 15, channels_in=1, channels_out=1, **FAR))
    oh, ow = C.c_int32(), C.c_int32()
    check = amd.lib().lce_hip_conv2d_f32_check
    for kw in edges:
        d = _desc(**{k: v for k, v in kw.items() if k not in PTRS})
        assert check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK, kw
        if amd.device_count() == 0:
            assert _c_call(**dict(kw)) == amd.ERR_NO_DEVICE, kw
    d = _desc(in_height=7, in_width=9, stride_height=2, stride_width=3)
    assert check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (4, 3)
    d = _desc(in_height=7, in_width=9, stride_height=2, stride_width=3, padding=amd.PADDING_VALID)
    assert check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (3, 3)
    assert check(C.byref(d), None, None) == amd.OK
    assert check(None, None, None) == amd.ERR_INVALID
    for kw, code, _ in REFUSALS:                             # the descriptor's refusals are the check's own
        if not set(kw) & (set(PTRS) | {"desc"}) or code == amd.ERR_UNSUPPORTED:
            d = _desc(**{k: v for k, v in kw.items() if k not in PTRS})
            assert check(C.byref(d), None, None) == code, kw


X = np.zeros((2, 8, 8, 64), np.float32)
W = np.zeros((32, 3, 3, 64), np.float32)


@pytest.mark.parametrize("x,w,kw,msg", [
    (X.astype(np.float64), W, {}, "float32 NHWC"),
    (X[0], W, {}, "NHWC"),
    (np.zeros((2, 0, 8, 64), np.float32), W, {}, "non-empty"),
    (X, W.astype(np.float64), {}, "w must be"),
    (X, np.zeros((32, 3, 3, 63), np.float32), {}, "w must be"),
    (X, np.zeros((32, 3, 3, 32), np.float32), {}, "w must be"),
    (X, np.zeros((32, 64), np.float32), {}, "w must be"),
    (X, np.zeros((32, 0, 3, 64), np.float32), {}, "w must be"),
    (X, np.zeros((0, 3, 3, 64), np.float32), {}, "w must be"),
    (X, W, dict(bias=np.zeros(31, np.float32)), "bias must be"),
    (X, W, dict(bias=np.zeros(32, np.float64)), "bias must be"),
    (X, W, dict(stride=0), "stride must be"),
    (X, W, dict(stride=(1, -1)), "stride must be"),
    (X, W, dict(stride=(2, 2, 2)), "stride must be"),
    (X, W, dict(padding=2), "padding must be"),
    (X, W, dict(activation=4), "unknown activation"),
    (X, np.zeros((32, 9, 3, 64), np.float32), dict(padding=amd.PADDING_VALID), "empty output"),
    (X, W, dict(out=False), "no output"),
    (X, W, dict(out=np.zeros((2, 8, 8, 31), np.float32)), "out must be"),
    (X, W, dict(out=np.zeros((2, 8, 8, 32), np.int8)), "out must be"),
    (X, W, dict(stride=2, out=np.zeros((2, 8, 8, 32), np.float32)), "out must be"),
    (X, W, dict(padding=amd.PADDING_VALID, out=np.zeros((2, 8, 8, 32), np.float32)), "out must be"),
    (X, W, dict(out_bits=np.zeros((2, 8, 8, 2), np.int32)), "out_bits must be"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, x, w, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    with pytest.raises(ValueError, match=msg):
        amd.conv2d(x, w, **kw)


def test_the_python_check_gives_the_descriptor_and_the_output_shape():
    d, shape = conv2d_check(X, W, np.zeros(32, np.float32), (2, 1), amd.PADDING_SAME, amd.ACT_RELU6, True, True)
    assert shape == (2, 4, 8, 32) and C.sizeof(d) == 44
    assert [getattr(d, n) for n, _ in Conv2dDesc._fields_] == [2, 8, 8, 64, 32, 3, 3, 2, 1, amd.PADDING_SAME, amd.ACT_RELU6]
    d, shape = conv2d_check(X, np.zeros((5, 8, 2, 64), np.float32), None, 3, amd.PADDING_VALID, amd.ACT_NONE, False, True)
    assert shape == (2, 1, 3, 5)


# ---- the opt-ins ----------------------------------------------------------------------------------------------------------------
def pack(size, sections, ext=0, reserved=(0,) * 11):
    """The options bytes of one of the four forms: exactly `size` bytes."""
    assert size in (8, 24, 40, 56)
    return struct.pack("<14I", size, sections, ext, *reserved)[:size]


def test_bits_8_and_16_live_in_the_56_byte_form_only():
    lib = mr.tflite_lib()
    for data in (quicknet_stem_model()[0], float3x3_in_body_model()[0]):
        for ext in range(32):
            want = _parts(mr.LceModel(data, elementwise_sections=True, pool_sections=bool(ext & 1), conv1x1_sections=bool(ext & 2),
                                      depthwise_sections=bool(ext & 4), conv2d_sections=bool(ext & 8), stem_sections=bool(ext & 16)))
            h, _ = _open(data, pack(56, 1, ext))
            assert h and _sections_of(h) == want, ext
            lib.lce_tflite_model_close(h)
        for size in (24, 40):                                # refused at the earlier sizes, alone and beside bits those know
            for ext in (8, 16, 24, 9, 17, 8 | 3, 16 | 3):
                h, err = _open(data, pack(size, 1, ext))
                assert not h and b"flags" in err, (size, ext)
            for ext in ((0, 1) if size == 24 else range(4)):  # ... which behave exactly as before
                h, _ = _open(data, pack(size, 1, ext))
                assert h and _sections_of(h) == _parts(mr.LceModel(data, elementwise_sections=True, pool_sections=bool(ext & 1),
                                                                  conv1x1_sections=bool(ext & 2))), (size, ext)
                lib.lce_tflite_model_close(h)
        for ext in (8, 16, 24):                              # size 8 reads no ext word at all
            h, _ = _open(data, pack(8, 1, ext))
            assert h and _sections_of(h) == _parts(mr.LceModel(data, elementwise_sections=True))
            lib.lce_tflite_model_close(h)
        for ext in (32, 64, 1 << 30, 1 << 31, (1 << 31) | 8, (1 << 31) | 31):          # unknown bits, and bit 31 for ever
            h, err = _open(data, pack(56, 1, ext))
            assert not h and b"flags" in err, ext
        for k in range(11):                                  # each of the eleven trailing words must be zero
            reserved = [0] * 11
            reserved[k] = 1 << (k * 2)
            h, err = _open(data, pack(56, 1, 24, reserved))
            assert not h and b"reserved" in err, k
        err = C.create_string_buffer(128)
        for flags in (8, 16, 24):                            # lce_tflite_model_open_ex is unchanged: it keeps its own mask
            assert not lib.lce_tflite_model_open_ex(data, len(data), flags, err, 128) and b"flags" in err.value
    stem = quicknet_stem_model()[0]
    one, cut = _open(stem, pack(56, 1, 31))[0], _open(stem, pack(56, 1, 7))[0]
    assert len(_sections_of(one)) == 1 and _sections_of(cut) == _parts(mr.LceModel(stem, **PARENT_FLAGS))
    lib.lce_tflite_model_close(one)
    lib.lce_tflite_model_close(cut)


def test_the_python_constructor_keeps_choosing_the_smallest_form(monkeypatch):
    data = quicknet_stem_model()[0]
    lib = mr.tflite_lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name in ("lce_tflite_model_open_ex", "lce_tflite_model_open_opts"):
                def spy(*a):
                    words = C.cast(a[2], C.POINTER(C.c_uint32)) if name.endswith("opts") else None
                    calls.append((name, a[2]) if words is None else (name, words[0], words[1], words[2] if words[0] > 8 else None))
                    return getattr(lib, name)(*a)
                return spy
            return getattr(lib, name)
    monkeypatch.setattr(mr, "tflite_lib", lambda: Spy())
    mr.LceModel(data, elementwise_sections=True)
    mr.LceModel(data, conv1x1_sections=True, pool_sections=True)
    mr.LceModel(data, conv2d_sections=True)
    mr.LceModel(data, stem_sections=True)
    mr.LceModel(data, stem_sections=True, conv1x1_sections=True)
    mr.LceModel(data, concat_sections=True, int8_add_sections=True, **ALL_FLAGS)
    mr.Interpreter(data, conv2d_sections=True, stem_sections=True)
    assert calls == [("lce_tflite_model_open_ex", 1), ("lce_tflite_model_open_opts", 40, 0, 3), ("lce_tflite_model_open_opts", 56, 0, 8),
                     ("lce_tflite_model_open_opts", 56, 0, 16), ("lce_tflite_model_open_opts", 56, 0, 18),
                     ("lce_tflite_model_open_opts", 56, 7, 31), ("lce_tflite_model_open_opts", 56, 0, 24)]


def test_the_abi():
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_conv2d_f32", "lce_hip_conv2d_f32_check"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_conv2d_stats")
    assert C.sizeof(amd.Conv2dDesc) == 44 and [n for n, _ in amd.Conv2dDesc._fields_] == [
        "batch", "in_height", "in_width", "channels_in", "channels_out", "filter_height", "filter_width", "stride_height",
        "stride_width", "padding", "activation"]
    assert (mr.SECTIONS_EXT_CONV2D, mr.SECTIONS_EXT_STEM) == (8, 16) and C.sizeof(mr._OpenOptions56) == 56


def test_stats_are_zero_before_any_run():
    model = mr.LceModel(quicknet_stem_model()[0], **ALL_FLAGS)
    assert model.conv2d_stats() == (0, 0) and model.conv1x1_stats() == (0, 0) and model.depthwise_stats() == (0, 0)
    mr.tflite_lib().lce_tflite_model_conv2d_stats(model._h, None, None)         # any pointer may be NULL
    mr.tflite_lib().lce_tflite_model_conv2d_stats(None, None, None)


# ---- the build: no scratch memory, no spills ----------------------------------------------------------------------------------------
def test_the_kernels_use_no_scratch_and_spill_nothing():
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_conv2d.hip")
    # conv2d_interior with the 16-byte and the dword load path, conv2d_border with and without the bit output
    assert len(kernels) == 4 and sum("conv2d_interior" in k for k in kernels) == 2 and sum("conv2d_border" in k for k in kernels) == 2, kernels
    for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
        assert resources[key] == ["0"] * 4, (key, resources[key])
    # interior: two tiles of 128 rows x 36 floats and 128 output pixel numbers; border: none
    lds = dict(zip(kernels, resources["LDS Size [bytes/block]"]))
    assert all(v == (str(2 * 128 * 36 * 4 + 128 * 4) if "interior" in k else "0") for k, v in lds.items()), lds
    assert "v_mfma_f32_32x32x2_f32" in mnemonics and "global_load_dwordx4" in mnemonics and "ds_read_b128" in mnemonics
    assert any(m.startswith(("v_fma_f32", "v_fmac_f32")) for m in mnemonics)
