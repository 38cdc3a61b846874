"""The float DEPTHWISE_CONV_2D of QuickNet's transition inside the sections (LCE_TFLITE_SECTIONS_EXT_DEPTHWISE,
include/lce_tflite_model.h) on the CPU: the NumPy reference (tests/depthwise_ref.py) against its definition, against torch's
grouped convolution on the CPU and against known answers worked by hand, DepthwiseConv2DOptions through the reader, the partition
with and without the opt-in, every condition that keeps a depthwise convolution with the host, the fourth (56-byte) form of the
options of lce_tflite_model_open_opts, the argument checks of lce_hip_depthwise_conv2d_f32 / amd.depthwise_conv2d (which all fail
before any device is touched) and the build of the new kernels.  Also the fixtures of the GPU side (tests/test_gpu_depthwise.py)."""
import ctypes as C
import importlib
import re
import struct

import numpy as np
import pytest

import conv1x1_ref as CR
import depthwise_ref as R
import hipcc_lib as H
import oracle_lib as O
import pool_ref as PR
from section_models import (ADD, CONV_2D, CONV_2D_OPTIONS, DEPTHWISE_CONV_2D, F32_SPECIAL, MARK, MAX_POOL_2D, MUL, NONE, RELU,
                            RELU6, RELU_N1_TO_1, TANH, _conv, _open, _sections_of, alexnet_body_model, bconv_options,
                            bireal_block_model, conv2d_op, cut_at, dense_block_model, depthwise_op, ew_op, float_fixture,
                            float_op, mixed_model, pool_op, quicknet_transition_model)
import synth
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

SAME, VALID = 0, 1
ACTS = (NONE, RELU, RELU_N1_TO_1, RELU6)
OLD_FLAGS = dict(elementwise_sections=True, pool_sections=True, conv1x1_sections=True)
ALL_FLAGS = dict(depthwise_sections=True, **OLD_FLAGS)


# ---- the reference against its definition ----------------------------------------------------------------------------------------
def grid_operands(filt, cout, special=False):
    """(w [fh, fw, Cout], bias [Cout]) of the grid: ASYMMETRIC random filters of mixed magnitude.  `special`: subnormal and tiny
    weights among them, so that subnormal products and sums occur."""
    g = np.random.default_rng(filt[0] * 10000 + filt[1] * 1000 + cout)
    shape = (filt[0], filt[1], cout)
    w = (g.standard_normal(shape) * g.choice([1e-2, 1.0, 30.0], shape)).astype(np.float32)
    bias = g.standard_normal(cout).astype(np.float32)
    if special:
        w[..., ::5] *= np.float32(1e-36)
        w[0, 0, ::3] = F32_SPECIAL[6]
    return w, bias


def exact_and_magnitude(x, w, stride, padding, m):
    """(the float64 sum, the sum of |x w|) of every output element, from the definition: a plain loop over output pixels."""
    b, h, wd, cin = x.shape
    fh, fw, cout = w.shape
    (oh, ph), (ow, pw) = PR.out_and_pad(h, fh, stride[0], padding), PR.out_and_pad(wd, fw, stride[1], padding)
    exact, mag = np.zeros((b, oh, ow, cout)), np.zeros((b, oh, ow, cout))
    xs = np.repeat(x.astype(np.float64), m, axis=3)
    for oy in range(oh):
        for ox in range(ow):
            for fy in range(fh):
                for fx in range(fw):
                    y, xx = oy * stride[0] - ph + fy, ox * stride[1] - pw + fx
                    if 0 <= y < h and 0 <= xx < wd:
                        p = xs[:, y, xx, :] * w[fy, fx].astype(np.float64)
                        exact[:, oy, ox, :] += p
                        mag[:, oy, ox, :] += np.abs(p)
    return exact, mag


def error_bound(taps, mag, bias):
    """taps roundings of at most 2^-24 of the running magnitude (<= sum |x w|) each, then the bias add's: 2^-24 of |t + bias|,
    where |t| <= (1 + taps 2^-24) sum |x w|."""
    b = 0.0 if bias is None else np.abs(bias.astype(np.float64))
    return taps * 2.0 ** -24 * mag + (0.0 if bias is None else 2.0 ** -24 * ((1 + taps * 2.0 ** -24) * mag + b))


@pytest.mark.parametrize("filt,stride,padding,m", [((3, 3), (2, 2), SAME, 1), ((3, 3), (1, 1), VALID, 1), ((5, 3), (2, 1), SAME, 1),
                                                   ((2, 2), (3, 4), SAME, 2), ((1, 1), (1, 1), SAME, 3), ((3, 3), (2, 2), SAME, 3)])
def test_the_reference_against_a_float64_sum(filt, stride, padding, m):
    x = float_fixture((2, 8, 7, 5), filt[0] * 10 + m)
    w, bias = grid_operands(filt, 5 * m)
    exact, mag = exact_and_magnitude(x, w, stride, padding, m)
    for bb in (None, bias):
        got = R.depthwise(x, w, bb, stride, padding, m)
        assert got.shape == exact.shape and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - (exact + (0.0 if bb is None else bb.astype(np.float64))))
        assert np.all(err <= error_bound(filt[0] * filt[1], mag, bb))
    assert np.abs(exact).max() > 0


@pytest.mark.parametrize("m", [1, 2])
def test_the_reference_against_torchs_grouped_convolution(m):
    """An asymmetric filter, stride 2 on EVEN extents under SAME: TFLite pads 0 in front and 1 behind (pad_before = total / 2),
    which torch is given explicitly.  A flipped or transposed tap order, or the extra row in front, would miss the bound."""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    cin = 6
    x = float_fixture((2, 8, 10, cin), 40 + m)
    w, bias = grid_operands((3, 3), cin * m)
    assert not np.allclose(w, w[::-1]) and not np.allclose(w, w[:, ::-1]) and not np.allclose(w, w.transpose(1, 0, 2))
    for stride, pads in (((2, 2), (0, 1, 0, 1)), ((1, 1), (1, 1, 1, 1))):
        (oh, ph), (ow, pw) = PR.out_and_pad(8, 3, stride[0], SAME), PR.out_and_pad(10, 3, stride[1], SAME)
        assert (ph, pw) == (pads[2], pads[0])
        xt = F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), pads)                        # (left, right, top, bottom)
        wt = torch.from_numpy(w).permute(2, 0, 1).unsqueeze(1).contiguous()              # [Cout, 1, fh, fw]: o reads group o // m
        want = F.conv2d(xt, wt, torch.from_numpy(bias), stride=stride, groups=cin).permute(0, 2, 3, 1).numpy()
        got = R.depthwise(x, w, bias, stride, SAME, m)
        assert got.shape == want.shape == (2, oh, ow, cin * m)
        _, mag = exact_and_magnitude(x, w, stride, SAME, m)
        assert np.all(np.abs(got.astype(np.float64) - want) <= error_bound(9, mag, bias))
        # the check can fail: the flipped filter is far outside the bound
        assert np.any(np.abs(R.depthwise(x, w[::-1, ::-1], bias, stride, SAME, m).astype(np.float64) - want) > error_bound(9, mag, bias))


# ---- known answers, worked by hand -------------------------------------------------------------------------------------------
P12 = np.float32(1 + 2.0 ** -12)
TINY = np.float32(1e-30)
SUB0 = np.array([0x00000001], np.uint32).view(np.float32)[0]                # the smallest subnormal
POW = (2.0 ** np.arange(9)).reshape(3, 3, 1).astype(np.float32)            # w[fy][fx] = 2^(3 fy + fx): a sum names its taps
BIG = 2.0 ** 24
# name -> (x [H, W, Cin], w [fh, fw, Cout], bias, stride, padding, multiplier, expected [OH, OW, Cout])
KNOWN = {
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 exactly: fused onto -1 it is 2^-11 + 2^-24; the rounded product is 1 + 2^-11
    "fused": ([[[-1.0], [P12]]], [[[1.0], [P12]]], None, 1, VALID, 1, [[[2.0 ** -11 + 2.0 ** -24]]]),
    # in order: 1 + 2^24 -> 2^24 (the 1 is lost), - 2^24 -> 0; any other order gives 1
    "ordered": ([[[1.0], [BIG], [-BIG]]], np.ones((1, 3, 1)), None, 1, VALID, 1, [[[0.0]]]),
    # a 2x2 filter, rows first: (0,0) (0,1) (1,0) (1,1) = 1, 2^24, -2^24, 0 -> 0; columns first: 1 - 2^24 + 2^24 = 1
    "ordered_rows": ([[[1.0], [BIG]], [[-BIG], [0.0]]], np.ones((2, 2, 1)), None, 1, VALID, 1, [[[0.0]]]),
    "minus_zero": ([[[TINY]]], [[[-TINY]]], None, 1, SAME, 1, [[[-0.0]]]),
    "minus_zero_bias": ([[[TINY]]], [[[-TINY]]], [0.0], 1, SAME, 1, [[[0.0]]]),          # -0.0 + +0.0 = +0.0
    # all ones 2x2 under SAME, stride 1: one row and column of padding in front and behind; pixel (oy, ox) uses the filter
    # rows {1,2} (oy = 0) or {0,1} (oy = 1), and the columns likewise
    "corner": (np.ones((2, 2, 1)), POW, None, 1, SAME, 1,
               [[[2 ** 4 + 2 ** 5 + 2 ** 7 + 2 ** 8], [2 ** 3 + 2 ** 4 + 2 ** 6 + 2 ** 7]],
                [[2 ** 1 + 2 ** 2 + 2 ** 4 + 2 ** 5], [2 ** 0 + 2 ** 1 + 2 ** 3 + 2 ** 4]]]),
    # stride 2: ONE row and column of padding, and it lies BEHIND (pad_before = 1 / 2 = 0): filter rows and columns {0, 1}
    "corner_stride_2": (np.ones((2, 2, 1)), POW, None, 2, SAME, 1, [[[2 ** 0 + 2 ** 1 + 2 ** 3 + 2 ** 4]]]),
    "subnormal": ([[[SUB0]]], [[[1.0]]], None, 1, SAME, 1, [[[SUB0]]]),
    # output channel o reads input channel o // 3
    "multiplier": ([[[10.0, 20.0]]], [[[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]], None, 1, SAME, 3, [[[10.0, 20.0, 30.0, 80.0, 100.0, 120.0]]]),
}


def known_case(name):
    """(x [1, H, W, Cin], w [1, fh, fw, Cout], bias or None, keyword arguments, expected float32 [1, OH, OW, Cout])."""
    x, w, bias, stride, padding, m, want = KNOWN[name]
    return (np.array(x, np.float32)[None], np.array(w, np.float32)[None], None if bias is None else np.array(bias, np.float32),
            dict(stride=stride, padding=padding, depth_multiplier=m), np.array(want, np.float32)[None])


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers_on_the_reference(name):
    x, w, bias, kw, want = known_case(name)
    got = R.depthwise(x, w, bias, **kw)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, got)
    if name == "minus_zero":
        assert got.view(np.uint32).tolist() == [[[[0x80000000]]]] and O.bitpack(got).reshape(-1).tolist() == [0]
    if name == "minus_zero_bias":
        assert got.view(np.uint32).tolist() == [[[[0]]]]
    if name == "fused":                                      # multiply, round, then add gives 2^-11
        assert np.float32(np.float32(P12 * P12) + np.float32(-1.0)) == np.float32(2.0 ** -11)
    if name.startswith("ordered"):
        assert np.float32(np.float32(1.0) + np.float32(-BIG)) + np.float32(BIG) == 1


def test_the_clamp_passes_nan_and_every_activation_clamps():
    x = float_fixture((2, 5, 7, 4), 3)
    w, bias = grid_operands((3, 3), 4)
    plain = R.depthwise(x, w, bias, (1, 1), SAME)
    for act in ACTS[1:]:
        assert np.any(R.depthwise(x, w, bias, (1, 1), SAME, 1, act) != plain)
    x[0, 0, 0, 0], x[0, 4, 6, 1] = np.nan, np.inf
    for act in ACTS:
        got = R.depthwise(x, w, None, (1, 1), SAME, 1, act)
        lo, hi = R.FLOAT_RANGE[act]
        assert np.isnan(got[0, :2, :2, 0]).all() and not np.isnan(got[0, 2:, 2:, 0]).any() and not np.isnan(got[..., 2:]).any()
        assert set(got[0, 3:, 5:, 1].reshape(-1).tolist()) <= {float(lo), float(hi)}     # an infinity is clamped, NONE included


def blur_then_binarize_model(H=8, C=64, seed=0):
    """The fold case.  x (float) -> LceQuantize -> LceBconv2d (float) -> MUL (c) -> ADD (c, RELU_N1_TO_1) -> DEPTHWISE_CONV_2D
    3x3 / 2 SAME (signed weights and a bias, so that both signs come out) -> LceQuantize -> LceBconv2d (float, the graph
    output).  The depthwise convolution feeds ONLY the LceQuantize."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 601)
    h2 = H // 2
    x = f32([1, H, H, C], "x")
    q0 = b.tensor([1, H, H, C // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y0, c0 = _conv(b, q0, H, C, C, seed * 10 + 5)
    bn_m, bn_a = g.uniform(-0.05, 0.05, C).astype(np.float32), g.standard_normal(C).astype(np.float32)
    mm, aa = f32([1, H, H, C], "mm"), f32([1, H, H, C], "aa")
    mul = ew_op(b, MUL, [y0, f32([C], "bn_m", bn_m)], [mm], NONE)
    add = ew_op(b, ADD, [mm, f32([C], "bn_a", bn_a)], [aa], RELU_N1_TO_1)
    k = g.standard_normal((1, 3, 3, C)).astype(np.float32)
    kb = (g.standard_normal(C) * 0.5).astype(np.float32)
    d = f32([1, h2, h2, C], "d")
    dw = depthwise_op(b, [aa, f32([1, 3, 3, C], "k", k), f32([C], "kb", kb)], [d], (2, 2), SAME)
    q1 = b.tensor([1, h2, h2, C // 32], np.int32, "q1")
    b.custom_op("LceQuantize", [d], [q1], b"")
    y1, c1 = _conv(b, q1, h2, C, C, seed * 10 + 6)
    b.inputs, b.outputs = [x], [y1]
    host = {mul: lambda v: float_op(v, MUL, bn_m, NONE), add: lambda v: float_op(v, ADD, bn_a, RELU_N1_TO_1),
            dw: lambda v: R.depthwise(v, k, kb, (2, 2), SAME)}
    info = dict(depthwise=dw, host=host, tensors=dict(aa=aa, d=d), size=H, channels=C, convs=[c0, c1], follows=[])
    return b.finish(), x, y1, info


FIXTURES = dict(quicknet=quicknet_transition_model, fold=blur_then_binarize_model)


# ---- the partition --------------------------------------------------------------------------------------------------------------
def _parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_each_fixture_is_one_section_with_all_flags(name):
    data, x, out, info = FIXTURES[name]()
    model = mr.LceModel(data, **ALL_FLAGS)
    n_ops = len(model.operators)
    k = info["depthwise"]
    assert model.operators[k].builtin_code == DEPTHWISE_CONV_2D and model.operators[k].depth_multiplier == 1
    assert [s.ops for s in model.sections] == [list(range(n_ops))]
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only and mr.Interpreter(data, **ALL_FLAGS).lce_only
    # without the new flag: two sections, cut at the blur (the 1x1 convolution behind it becomes ready in the host's epoch then,
    # and goes with it)
    without = mr.LceModel(data, **OLD_FLAGS)
    assert [s.ops for s in without.sections] == cut_at(n_ops, [k] + info["follows"]) and len(without.sections) == 2
    assert not mr.Interpreter(without).lce_only
    every = mr.LceModel(data, int8_add_sections=True, concat_sections=True, **ALL_FLAGS)
    assert [s.ops for s in every.sections] == [list(range(n_ops))]
    # no flags: the default partition, one section per (LceQuantize, LceBconv2d)
    plain = mr.LceModel(data)
    assert [s.ops for s in plain.sections] == [[0, 1], [k + 1 + len(info["follows"]), k + 2 + len(info["follows"])]]
    # the new flag alone: the blur joins only where it becomes ready in an LCE epoch -- behind operators the host runs it does not
    alone = mr.LceModel(data, depthwise_sections=True)
    assert all(k not in s.ops for s in alone.sections) and _parts(alone) == _parts(plain)


def test_a_stem_depthwise_stays_with_the_host_under_every_flag():
    """QuickNet's stem has a depthwise convolution too: it is ready from the start, before any LCE operator."""
    data, k = _graph("stem")
    plain = _parts(mr.LceModel(data))
    for kw in (dict(depthwise_sections=True), ALL_FLAGS, dict(int8_add_sections=True, concat_sections=True, **ALL_FLAGS)):
        model = mr.LceModel(data, **kw)
        assert all(k not in s.ops for s in model.sections) and _parts(model) == plain and not mr.Interpreter(model).lce_only


def test_files_without_a_qualifying_depthwise_keep_their_partitions():
    for data in (dense_block_model()[0], mixed_model()[0], alexnet_body_model()[0], bireal_block_model()[0]):
        for kw in ({}, dict(elementwise_sections=True), dict(concat_sections=True, **OLD_FLAGS)):
            assert _parts(mr.LceModel(data, **kw)) == _parts(mr.LceModel(data, depthwise_sections=True, **kw))


JOINS = ["joins", "no_bias_two_inputs", "no_bias_minus_one", "stride_2", "stride_3_1", "valid", "relu6", "no_dilations", "multiplier_2",
         "filter_1x1", "filter_5x3"]
STAYS = ["one_input", "four_inputs", "two_outputs", "int8_input", "int8_filter", "int8_output", "int32_bias", "three_d_output",
         "three_d_input", "constant_input", "filter_not_constant", "filter_leading_2", "filter_3_d", "filter_channels",
         "bias_not_constant", "bias_length", "bias_2_d", "output_channels", "no_options", "conv2d_options", "zero_multiplier",
         "negative_multiplier", "multiplier_mismatch", "zero_stride", "negative_stride", "huge_stride", "dilation_w", "dilation_h",
         "padding_2", "tanh", "sign_bit", "extent_off_by_one", "valid_extent_as_same", "conv_2d_code", "stem"]


def _graph(case):
    """x -> LceQuantize -> LceBconv2d -> y -> <DEPTHWISE_CONV_2D under test> -> z -> LceQuantize -> q2, with one condition of
    the candidate rule broken per case of STAYS.  Returns (file, index of the depthwise convolution)."""
    Hh, Cc = 8, 64
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i8 = lambda shape, name, data=None: b.tensor(shape, np.int8, name, data, scale=0.5, zero_point=1)
    const = lambda make, shape, name: make(shape, name, np.ones(shape, np.float32))
    x = f32([1, Hh, Hh, Cc], "x")
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    y_make = i8 if case == "int8_input" else f32
    y = y_make([Hh, Hh, Cc] if case == "three_d_input" else [1, Hh, Hh, Cc], "y")
    if case != "stem":
        b.custom_op("LceQuantize", [x], [q], b"")
        b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                    bconv_options(spec))
    src = x if case == "stem" else y
    if case == "constant_input":
        src = const(f32, [1, Hh, Hh, Cc], "c")
    kw, zshape, code, table = {}, [1, Hh, Hh, Cc], DEPTHWISE_CONV_2D, None
    flt = const(f32, [1, 3, 3, Cc], "k")
    kb = const(f32, [Cc], "kb")
    z_make, outs_extra = f32, []
    if case == "no_bias_two_inputs":
        kb = None
    elif case == "no_bias_minus_one":
        kb = -1
    elif case == "stride_2":
        kw, zshape = dict(stride=(2, 2)), [1, Hh // 2, Hh // 2, Cc]
    elif case == "stride_3_1":
        kw, zshape = dict(stride=(3, 1)), [1, 3, Hh, Cc]
    elif case == "valid":
        kw, zshape = dict(padding=VALID), [1, Hh - 2, Hh - 2, Cc]
    elif case == "relu6":
        kw = dict(activation=RELU6)
    elif case == "no_dilations":
        kw = dict(dilation=None)
    elif case == "multiplier_2":
        kw, flt, kb, zshape = dict(multiplier=2), const(f32, [1, 3, 3, 2 * Cc], "k2"), const(f32, [2 * Cc], "kb2"), [1, Hh, Hh, 2 * Cc]
    elif case == "filter_1x1":
        flt = const(f32, [1, 1, 1, Cc], "k1")
    elif case == "filter_5x3":
        kw, flt, zshape = dict(padding=VALID), const(f32, [1, 5, 3, Cc], "k53"), [1, Hh - 4, Hh - 2, Cc]
    elif case == "int8_filter":
        flt = i8([1, 3, 3, Cc], "k8", np.ones([1, 3, 3, Cc], np.int8))
    elif case == "int8_output":
        z_make = i8
    elif case == "int32_bias":
        kb = b.tensor([Cc], np.int32, "kb32", np.ones(Cc, np.int32))
    elif case == "three_d_output":
        zshape = [Hh, Hh, Cc]
    elif case == "filter_not_constant":
        flt = f32([1, 3, 3, Cc], "kv")
    elif case == "filter_leading_2":
        flt = const(f32, [2, 3, 3, Cc], "k2")
    elif case == "filter_3_d":
        flt = const(f32, [3, 3, Cc], "k3")
    elif case == "filter_channels":
        flt = const(f32, [1, 3, 3, Cc // 2], "kc")
    elif case == "bias_not_constant":
        kb = f32([Cc], "kbv")
    elif case == "bias_length":
        kb = const(f32, [Cc + 1], "kb65")
    elif case == "bias_2_d":
        kb = const(f32, [1, Cc], "kb2")
    elif case == "output_channels":
        zshape = [1, Hh, Hh, Cc * 2]
    elif case == "no_options":
        kw = dict(options=False)
    elif case == "conv2d_options":                           # a table of the wrong union type
        table = CONV_2D_OPTIONS
    elif case == "zero_multiplier":
        kw = dict(multiplier=0)
    elif case == "negative_multiplier":
        kw = dict(multiplier=-1)
    elif case == "multiplier_mismatch":                      # the filter and the output have Cin x 1 channels
        kw = dict(multiplier=2)
    elif case == "zero_stride":
        kw = dict(stride=(0, 1))
    elif case == "negative_stride":
        kw = dict(stride=(1, -1))
    elif case == "huge_stride":
        kw, zshape = dict(stride=(2 ** 31 - 1, 2 ** 31 - 1)), [1, 1, 1, Cc]
    elif case == "dilation_w":
        kw = dict(dilation=(1, 2))
    elif case == "dilation_h":
        kw = dict(dilation=(0, 1))
    elif case == "padding_2":
        kw = dict(padding=2)
    elif case == "tanh":
        kw = dict(activation=TANH)
    elif case == "sign_bit":
        kw = dict(activation=5)
    elif case == "extent_off_by_one":
        kw, zshape = dict(stride=(2, 2)), [1, Hh // 2 + 1, Hh // 2, Cc]
    elif case == "valid_extent_as_same":                     # VALID gives 6 x 6
        kw = dict(padding=VALID)
    elif case == "conv_2d_code":
        code = CONV_2D
    elif case == "two_outputs":
        outs_extra = [f32(zshape, "z2")]
    else:
        assert case in ("joins", "one_input", "four_inputs", "int8_input", "three_d_input", "constant_input", "stem"), case
    z = z_make(zshape, "z")
    ins = [src, flt] + ([] if kb is None else [kb])
    if case == "one_input":
        ins = [src]
    elif case == "four_inputs":
        ins = ins + [kb]
    if table is not None:
        k = conv2d_op(b, ins, [z], code=DEPTHWISE_CONV_2D)
    else:
        k = depthwise_op(b, ins, [z] + outs_extra, code=code, **kw)
    q2 = b.tensor(zshape[:-1] + [(zshape[-1] + 31) // 32], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = [x], [q2]
    return b.finish(), k


@pytest.mark.parametrize("case", STAYS)
def test_depthwise_convolutions_that_stay_with_the_host(case):
    data, k = _graph(case)
    model = mr.LceModel(data, int8_add_sections=True, concat_sections=True, **ALL_FLAGS)
    assert all(k not in s.ops for s in model.sections), (case, [s.ops for s in model.sections])
    assert not mr.Interpreter(model).lce_only
    assert _parts(model) == _parts(mr.LceModel(data))


@pytest.mark.parametrize("case", JOINS)
def test_a_qualifying_depthwise_convolution_joins(case):
    data, k = _graph(case)
    model = mr.LceModel(data, depthwise_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and k == 2
    assert mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]
    assert [s.ops for s in mr.LceModel(data, int8_add_sections=True, concat_sections=True, **OLD_FLAGS).sections] == [[0, 1], [3]]


# ---- the reader -----------------------------------------------------------------------------------------------------------------
def _options_model(rows):
    """One DEPTHWISE_CONV_2D per row (padding, stride_w, stride_h, depth_multiplier, activation, dilation_w, dilation_h),
    (padding, stride_w, stride_h, depth_multiplier, activation) for a table without the dilations, or None for one without an
    options table, each followed by an ADD."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, 4, 4, 4], "x")
    k = f32([1, 1, 1, 4], "k", np.ones((1, 1, 1, 4), np.float32))
    prev = x
    for n, row in enumerate(rows):
        out = f32([1, 4, 4, 4], "t%d" % n)
        if row is None:
            depthwise_op(b, [prev, k], [out], options=False)
        else:
            depthwise_op(b, [prev, k], [out], (row[2], row[1]), row[0], row[3], row[4], None if len(row) == 5 else (row[6], row[5]))
        prev = f32([1, 4, 4, 4], "u%d" % n)
        ew_op(b, ADD, [out, out], [prev], RELU)
    b.inputs, b.outputs = [x], [prev]
    return b.finish()


def test_depthwise_options_round_trip_through_the_reader():
    rows = [(VALID, 2, 3, 7, RELU6, 4, 5), (SAME, 1, 1, 1, NONE, 1, 1), None, (VALID, 2, 2, 3, RELU),
            (1, 2 ** 31 - 1, -7, -2 ** 31, 5, 0, -2 ** 31), (-1, 9, 8, 2, RELU_N1_TO_1, 7, 6)]
    model = mr.LceModel(_options_model(rows))
    convs, others = model.operators[0::2], model.operators[1::2]
    lib = mr.tflite_lib()
    v = (C.c_int32 * 6)()
    for n, (op, row) in enumerate(zip(convs, rows)):
        assert op.builtin_code == DEPTHWISE_CONV_2D
        full = None if row is None else row + (1, 1) if len(row) == 5 else row         # the schema's defaults
        want = [0, 0, 0, 0, 1, 1] if full is None else [full[0], full[1], full[2], full[3], full[5], full[6]]
        assert lib.lce_tflite_model_operator_depthwise(model._h, 2 * n, v) == amd.OK and list(v) == want, row
        assert op.activation == (0 if row is None else row[4])
        assert (op.padding, op.stride_w, op.stride_h, op.depth_multiplier, op.dilation_w, op.dilation_h) == tuple(want)
        assert (op.filter_width, op.filter_height) == (0, 0)
    for n, op in enumerate(others):                                                    # every other operator
        assert lib.lce_tflite_model_operator_depthwise(model._h, 2 * n + 1, v) == amd.OK and list(v) == [0, 0, 0, 0, 1, 1]
        assert (op.padding, op.stride_w, op.stride_h, op.depth_multiplier, op.dilation_w, op.dilation_h) == (0, 0, 0, 0, 1, 1)
        assert op.activation == RELU
    assert lib.lce_tflite_model_operator_depthwise(model._h, len(model.operators), v) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_depthwise(model._h, -1, v) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_depthwise(model._h, 0, None) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_depthwise(None, 0, v) == amd.ERR_INVALID
    # a CONV_2D's table is not a depthwise one, and the other way round
    data, k = _graph("conv2d_options")
    model = mr.LceModel(data)
    assert lib.lce_tflite_model_operator_depthwise(model._h, k, v) == amd.OK and list(v) == [0, 0, 0, 0, 1, 1]
    data, k = _graph("joins")
    w5 = (C.c_int32 * 5)()
    assert lib.lce_tflite_model_operator_conv2d(mr.LceModel(data)._h, k, w5) == amd.OK and list(w5) == [0, 0, 0, 1, 1]


def _depthwise_table(data):
    """(position of the DepthwiseConv2DOptions table whose depth_multiplier is MARK, position of the uoffset that points to it,
    position of the vtable's first slot): a vtable of seven slots (18 bytes) whose slot 3 names MARK's position."""
    at = data.index(struct.pack("<i", MARK))
    assert data.count(struct.pack("<i", MARK)) == 1
    for table in range(at - 4, max(0, at - 64), -4):
        vt = table - struct.unpack_from("<i", data, table)[0]
        if 0 <= vt < table and vt + 18 <= len(data) and struct.unpack_from("<H", data, vt)[0] == 18 and \
                table + struct.unpack_from("<H", data, vt + 4 + 2 * 3)[0] == at:
            refs = [p for p in range(0, table, 4) if p + struct.unpack_from("<I", data, p)[0] == table]
            assert len(refs) == 1
            return table, refs[0], vt + 4
    raise AssertionError("options table not found")


def test_a_truncated_or_out_of_bounds_options_table_is_refused_at_open():
    data = bytearray(_options_model([(VALID, 2, 2, MARK, NONE, 3, 3)]))
    assert mr.LceModel(bytes(data)).operators[0].depth_multiplier == MARK
    table, ref, slots = _depthwise_table(data)
    bad = []
    for target in (len(data) - 2, len(data), len(data) + 4096, 2 ** 32 - 8 - ref):   # cut short by the end of the file; beyond it
        d = bytearray(data)
        struct.pack_into("<I", d, ref, (target - ref) % 2 ** 32)
        bad.append(bytes(d))
    for soffset in (table + 8, -(len(data) + 64), 2 ** 31 - 1):                        # the table's vtable lies outside the file
        d = bytearray(data)
        struct.pack_into("<i", d, table, soffset)
        bad.append(bytes(d))
    for field in range(7):                                                             # each field far outside the file
        d = bytearray(data)
        struct.pack_into("<H", d, slots + 2 * field, 0xFFF0)
        bad.append(bytes(d))
    assert len(bad) == 14
    for d in bad:
        for kw in ({}, ALL_FLAGS):
            with pytest.raises(ValueError, match="bad DepthwiseConv2DOptions"):
                mr.LceModel(d, **kw)
    for cut in range(len(data) - 1, len(data) - 200, -7):                              # truncated files never crash
        try:
            mr.LceModel(bytes(data[:cut]), **ALL_FLAGS)
        except ValueError:
            pass


# ---- shape inference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
def test_section_tensor_shape_over_the_blurred_tensors(batch):
    data, x, out, info = quicknet_transition_model()
    model = mr.LceModel(data, **ALL_FLAGS)
    t = info["tensors"]
    assert model.section_tensor_shape(0, t["p"], batch) == ((batch, 8, 8, 32), batch * 64 * 32 * 4)
    assert model.section_tensor_shape(0, t["d"], batch) == ((batch, 4, 4, 32), batch * 16 * 32 * 4)
    assert model.section_tensor_shape(0, t["t"], batch) == ((batch, 4, 4, 64), batch * 16 * 64 * 4)
    assert model.section_tensor_shape(0, out, batch) == ((batch, 4, 4, 64), batch * 16 * 64 * 4)
    for case, want in (("stride_2", (batch, 4, 4, 64)), ("stride_3_1", (batch, 3, 8, 64)), ("valid", (batch, 6, 6, 64)),
                       ("filter_5x3", (batch, 4, 6, 64)), ("multiplier_2", (batch, 8, 8, 128))):
        data, k = _graph(case)
        model = mr.LceModel(data, depthwise_sections=True)
        assert model.section_tensor_shape(0, model.operators[k].outputs[0], batch)[0] == want
        assert model.section_tensor_shape(0, model.outputs[0], batch)[0] == want[:3] + ((want[3] + 31) // 32,)


@pytest.mark.parametrize("declared", [32, 96])
def test_a_file_whose_depthwise_input_disagrees_with_the_inferred_shape_is_refused(declared):
    """The depthwise convolution's tensors agree with each other in the file, but the binary convolution produces 64 channels
    where the file declares `declared` for its output: the walk must fail instead of reading past (or short of) its buffer."""
    Hh, Cc = 8, 64
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x, y, z = f32([1, Hh, Hh, Cc], "x"), f32([1, Hh, Hh, declared], "y"), f32([1, Hh, Hh, declared], "z")
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                bconv_options(spec))
    depthwise_op(b, [y, f32([1, 3, 3, declared], "k", np.ones((1, 3, 3, declared), np.float32))], [z])
    b.inputs, b.outputs = [x], [z]
    model = mr.LceModel(b.finish(), depthwise_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2]]
    with pytest.raises(amd.LceHipError, match="DEPTHWISE_CONV_2D input") as e:
        model.section_tensor_shape(0, z, 2)
    assert e.value.code == amd.ERR_INVALID


# ---- lce_hip_depthwise_conv2d_f32 / amd.depthwise_conv2d argument checks (no device needed: they come first) ---------------------
def _desc(**kw):
    d = dict(batch=2, in_height=8, in_width=8, channels_in=64, depth_multiplier=1, filter_height=3, filter_width=3, stride_height=1,
             stride_width=1, padding=amd.PADDING_SAME, activation=amd.ACT_NONE)
    d.update(kw)
    return amd.DepthwiseDesc(*[d[n] for n, _ in amd.DepthwiseDesc._fields_])


# the input is 2 x 8 x 8 x 64 floats = 32 KiB at 65536, the filter 3 x 3 x 64 floats = 2304 bytes, the bias 256 bytes, the output
# 2 x 8 x 8 x 64 floats = 32 KiB, the bits 2 x 8 x 8 x 2 words = 1 KiB
PTRS = dict(inp=1 << 16, flt=1 << 18, bias=1 << 19, out=1 << 20, bits=1 << 21)
FAR = dict(inp=1 << 40, flt=1 << 46, out=1 << 50, bits=1 << 60)


def _c_call(desc=True, **kw):
    p = dict(PTRS)
    p.update({k: kw.pop(k) for k in list(kw) if k in PTRS})
    d = _desc(**kw)
    return amd.lib().lce_hip_depthwise_conv2d_f32(C.byref(d) if desc else None,
                                                  *[C.c_void_p(p[k]) for k in ("inp", "flt", "bias", "out", "bits")], None)


REFUSALS = [
    (dict(desc=False), amd.ERR_INVALID, "null desc"),
    (dict(inp=0), amd.ERR_INVALID, "null input"),
    (dict(flt=0), amd.ERR_INVALID, "null filter"),
    (dict(out=0, bits=0), amd.ERR_INVALID, "both outputs"),
    (dict(batch=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_height=-1), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_width=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(channels_in=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(depth_multiplier=0), amd.ERR_INVALID, "multiplier must be positive"),
    (dict(depth_multiplier=-2), amd.ERR_INVALID, "multiplier must be positive"),
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
    (dict(batch=2 ** 20, in_height=2 ** 6, in_width=2 ** 6, channels_in=1, filter_height=1, filter_width=1, **FAR),
     amd.ERR_UNSUPPORTED, "2\\^31 pixels"),
    (dict(stride_height=2 ** 31 - 1, stride_width=2 ** 31 - 1), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(stride_width=2 ** 30 + 1), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(batch=1, channels_in=1, in_height=2 ** 30 + 1, in_width=1, stride_height=2, **FAR), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(filter_height=2 ** 15, filter_width=2 ** 15, channels_in=2, **FAR), amd.ERR_UNSUPPORTED, "2\\^31 or more elements"),
    (dict(filter_height=1, filter_width=1, channels_in=2 ** 30, depth_multiplier=2, batch=1, in_height=1, in_width=1, **FAR),
     amd.ERR_UNSUPPORTED, "2\\^31 or more elements"),
    (dict(filter_height=2 ** 31 - 1, filter_width=2 ** 31 - 1, channels_in=1, **FAR), amd.ERR_UNSUPPORTED, "2\\^31 or more elements"),
    (dict(out=(1 << 16) + 512), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=(1 << 16) - 16), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=0, bits=(1 << 16) + 32768 - 4), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=(1 << 18) + 2304 - 4), amd.ERR_INVALID, "overlaps the filter"),
    (dict(out=0, bits=(1 << 18) - 1020), amd.ERR_INVALID, "overlaps the filter"),
    (dict(out=(1 << 19) - 32764), amd.ERR_INVALID, "overlaps the bias"),
    (dict(out=0, bits=(1 << 19) + 252), amd.ERR_INVALID, "overlaps the bias"),
    (dict(bits=(1 << 20) + 32764), amd.ERR_INVALID, "outputs overlap"),
    (dict(bits=(1 << 21) + 2), amd.ERR_INVALID, "4-byte aligned"),
    (dict(inp=(1 << 16) + 1), amd.ERR_INVALID, "4-byte aligned"),
    (dict(flt=(1 << 18) + 1), amd.ERR_INVALID, "4-byte aligned"),
    (dict(bias=(1 << 19) + 2), amd.ERR_INVALID, "4-byte aligned"),
]


@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_c_entry_refuses_bad_arguments(kw, code, msg):
    assert _c_call(**dict(kw)) == code
    assert re.search(msg, amd.lib().lce_hip_last_error().decode()), amd.lib().lce_hip_last_error()


def test_c_entry_accepts_the_edges_of_the_checks_up_to_the_device():
    """Touching ranges do not overlap; a NULL bias, either output alone, the largest stride, a filter of 2^30 elements and every
    activation pass.  Without a device the accepted calls end at ERR_NO_DEVICE; none of them is ERR_INVALID or ERR_UNSUPPORTED."""
    edges = (dict(out=(1 << 16) + 32768), dict(out=(1 << 16) - 32768), dict(bits=(1 << 20) + 32768), dict(out=0), dict(bits=0), dict(bias=0),
             dict(out=(1 << 18) + 2304), dict(out=(1 << 19) + 256), dict(bias=0, out=1 << 19),   # (no bias: nothing there to overlap)
             dict(stride_height=2 ** 30, stride_width=2 ** 30), dict(inp=(1 << 16) + 4, flt=(1 << 18) + 4, out=(1 << 20) + 12),
             dict(activation=amd.ACT_RELU), dict(activation=amd.ACT_RELU_N1_TO_1), dict(activation=amd.ACT_RELU6),
             dict(padding=amd.PADDING_VALID, filter_height=8, filter_width=8), dict(channels_in=1), dict(depth_multiplier=3, **FAR),
             dict(filter_height=2 ** 15, filter_width=2 ** 15, channels_in=1, **FAR))
    oh, ow = C.c_int32(), C.c_int32()
    for kw in edges:
        d = _desc(**{k: v for k, v in kw.items() if k not in PTRS})
        assert amd.lib().lce_hip_depthwise_conv2d_f32_check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK, kw
        if amd.device_count() == 0:
            assert _c_call(**dict(kw)) == amd.ERR_NO_DEVICE, kw
    check = amd.lib().lce_hip_depthwise_conv2d_f32_check
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
W = np.zeros((1, 3, 3, 64), np.float32)


@pytest.mark.parametrize("x,w,kw,msg", [
    (X.astype(np.float64), W, {}, "float32 NHWC"),
    (X[0], W, {}, "NHWC"),
    (np.zeros((2, 0, 8, 64), np.float32), W, {}, "non-empty"),
    (X, W.astype(np.float64), {}, "filter must be"),
    (X, np.zeros((1, 3, 3, 63), np.float32), {}, "filter must be"),
    (X, np.zeros((2, 3, 3, 64), np.float32), {}, "filter must be"),
    (X, np.zeros((3, 64), np.float32), {}, "filter must be"),
    (X, np.zeros((1, 0, 3, 64), np.float32), {}, "filter must be"),
    (X, W, dict(depth_multiplier=2), "filter must be"),
    (X, W, dict(depth_multiplier=0), "depth_multiplier must be"),
    (X, W, dict(depth_multiplier=1.5), "depth_multiplier must be"),
    (X, W, dict(bias=np.zeros(63, np.float32)), "bias must be"),
    (X, W, dict(bias=np.zeros(64, np.float64)), "bias must be"),
    (X, W, dict(stride=0), "stride must be"),
    (X, W, dict(stride=(1, -1)), "stride must be"),
    (X, W, dict(stride=(2, 2, 2)), "stride must be"),
    (X, W, dict(padding=2), "padding must be"),
    (X, W, dict(activation=4), "unknown activation"),
    (X, np.zeros((1, 9, 3, 64), np.float32), dict(padding=amd.PADDING_VALID), "empty output"),
    (X, W, dict(out=False), "no output"),
    (X, W, dict(out=np.zeros((2, 8, 8, 63), np.float32)), "out must be"),
    (X, W, dict(out=np.zeros((2, 8, 8, 64), np.int8)), "out must be"),
    (X, W, dict(stride=2, out=np.zeros((2, 8, 8, 64), np.float32)), "out must be"),
    (X, W, dict(padding=amd.PADDING_VALID, out=np.zeros((2, 8, 8, 64), np.float32)), "out must be"),
    (X, W, dict(out_bits=np.zeros((2, 8, 8, 3), np.int32)), "out_bits must be"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, x, w, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    with pytest.raises(ValueError, match=msg):
        amd.depthwise_conv2d(x, w, **kw)


# ---- the opt-in -----------------------------------------------------------------------------------------------------------------
def pack(size, sections, ext=0, reserved=(0,) * 11):
    """The options bytes of one of the four forms: exactly `size` bytes."""
    assert size in (8, 24, 40, 56)
    return struct.pack("<14I", size, sections, ext, *reserved)[:size]


def test_open_opts_has_a_fourth_size():
    lib = mr.tflite_lib()
    assert [C.sizeof(t) for t in (mr._OpenOptions, mr._OpenOptionsExt, mr._OpenOptions40, mr._OpenOptions56)] == [8, 24, 40, 56]
    for data in (quicknet_transition_model()[0], blur_then_binarize_model()[0], bireal_block_model()[0], mixed_model()[0]):
        for sections in range(8):
            kw = dict(elementwise_sections=bool(sections & 1), int8_add_sections=bool(sections & 2), concat_sections=bool(sections & 4))
            want = {ext: _parts(mr.LceModel(data, pool_sections=bool(ext & 1), conv1x1_sections=bool(ext & 2),
                                            depthwise_sections=bool(ext & 4), **kw)) for ext in range(8)}
            for size, exts in ((8, (0,)), (24, (0, 1)), (40, range(4)), (56, range(8))):
                for ext in exts:                                 # the earlier forms behave as before: nothing behind them is read
                    raw = pack(size, sections, ext)
                    h, _ = _open(data, raw)
                    assert len(raw) == size and h and _sections_of(h) == want[ext], (size, sections, ext)
                    lib.lce_tflite_model_close(h)
        for size, ext in ((24, 4), (24, 5), (40, 4), (40, 7)):             # the new bit is accepted only at size 56
            h, err = _open(data, pack(size, 1, ext))
            assert not h and b"flags" in err, (size, ext)
        h, _ = _open(data, pack(8, 1, 4))                                  # (size 8 reads no ext at all)
        assert h
        lib.lce_tflite_model_close(h)
        # bits this version does not know are refused today, but only bit 31 is promised to stay refused
        for ext in (1 << 31, (1 << 31) | 4, (1 << 31) | 7):
            h, err = _open(data, pack(56, 1, ext))
            assert not h and b"flags" in err, ext
        for sections in (8, 16, 1 << 31):
            h, err = _open(data, pack(56, sections, 4))
            assert not h and b"flags" in err
        for k in range(11):                                                # each of the eleven trailing words
            reserved = [0] * 11
            reserved[k] = 1 << (k * 2)
            h, err = _open(data, pack(56, 1, 4, reserved))
            assert not h and b"reserved" in err, k
        for size in (52, 60, 72):
            raw = struct.pack("<18I", size, 1, 4, *([0] * 15))[:size]
            h, err = _open(data, raw)
            assert not h and b"struct_size" in err, size
    body = quicknet_transition_model()[0]
    one, cut = _open(body, pack(56, 1, 7))[0], _open(body, pack(40, 1, 3))[0]
    assert len(_sections_of(one)) == 1 and len(_sections_of(cut)) == 2
    lib.lce_tflite_model_close(one)
    lib.lce_tflite_model_close(cut)


def test_the_python_constructor_uses_the_56_byte_options_only_for_the_depthwise_flag(monkeypatch):
    data = quicknet_transition_model()[0]
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
    mr.LceModel(data, concat_sections=True)
    mr.LceModel(data, pool_sections=True)
    mr.LceModel(data, conv1x1_sections=True)
    mr.LceModel(data, concat_sections=True, **OLD_FLAGS)
    mr.LceModel(data, depthwise_sections=True)
    mr.LceModel(data, depthwise_sections=True, pool_sections=True)
    mr.LceModel(data, concat_sections=True, int8_add_sections=True, **ALL_FLAGS)
    assert calls == [("lce_tflite_model_open_ex", 1), ("lce_tflite_model_open_opts", 8, 4, None), ("lce_tflite_model_open_opts", 24, 0, 1),
                     ("lce_tflite_model_open_opts", 40, 0, 2), ("lce_tflite_model_open_opts", 40, 5, 3),
                     ("lce_tflite_model_open_opts", 56, 0, 4), ("lce_tflite_model_open_opts", 56, 0, 5),
                     ("lce_tflite_model_open_opts", 56, 7, 7)]


def test_the_abi():
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_depthwise_conv2d_f32", "lce_hip_depthwise_conv2d_f32_check"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    for name in ("lce_tflite_model_depthwise_stats", "lce_tflite_model_operator_depthwise"):
        assert hasattr(mr.tflite_lib(), name)
    assert C.sizeof(amd.DepthwiseDesc) == 44 and [n for n, _ in amd.DepthwiseDesc._fields_] == [
        "batch", "in_height", "in_width", "channels_in", "depth_multiplier", "filter_height", "filter_width", "stride_height",
        "stride_width", "padding", "activation"]
    assert mr.SECTIONS_EXT_DEPTHWISE == 4
    err = C.create_string_buffer(128)
    data = quicknet_transition_model()[0]
    for flags in (4, 8):                                     # open_ex keeps its own mask
        assert not mr.tflite_lib().lce_tflite_model_open_ex(data, len(data), flags, err, 128)


def test_stats_are_zero_before_any_run():
    model = mr.LceModel(quicknet_transition_model()[0], **ALL_FLAGS)
    assert model.depthwise_stats() == (0, 0) and model.conv1x1_stats() == (0, 0) and model.pool_stats() == (0, 0)
    mr.tflite_lib().lce_tflite_model_depthwise_stats(model._h, None, None)      # any pointer may be NULL
    mr.tflite_lib().lce_tflite_model_depthwise_stats(None, None, None)


# ---- the build: no scratch memory, no spills, no LDS ------------------------------------------------------------------------------
def test_the_kernels_use_no_scratch_no_lds_and_spill_nothing():
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_depthwise.hip")
    # depthwise_vec and depthwise_rows, each with and without the bit output
    assert len(kernels) == 4 and sum("depthwise_vec" in k for k in kernels) == 2 and sum("depthwise_rows" in k for k in kernels) == 2, kernels
    for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
        assert resources[key] == ["0"] * 4, (key, resources[key])
    assert resources["LDS Size [bytes/block]"] == ["0"] * 4                   # the weights come through the cache: nothing is staged
    assert "global_load_dwordx4" in mnemonics
    assert "v_fma_f32" in mnemonics or "v_pk_fma_f32" in mnemonics
