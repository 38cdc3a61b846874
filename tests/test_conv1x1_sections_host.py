"""The float 1x1 CONV_2D of transitions and shortcuts inside the sections (LCE_TFLITE_SECTIONS_EXT_CONV1X1,
include/lce_tflite_model.h) on the CPU: the NumPy reference (tests/conv1x1_ref.py) against libm's fmaf and against known
answers, Conv2DOptions through the reader, the partition with and without the opt-in, every condition that keeps a convolution
with the host, the third (40-byte) form of the options of lce_tflite_model_open_opts, the argument checks of
lce_hip_conv1x1_f32 / amd.conv1x1 (which all fail before any device is touched) and the build of the new kernel.  Also the
fixtures of the GPU side (tests/test_gpu_conv1x1.py)."""
import ctypes as C
import importlib
import re
import struct

import numpy as np
import pytest

import conv1x1_ref as R
import hipcc_lib as H
import oracle_lib as O
from section_models import (ADD, CONV_2D, DEPTHWISE_CONV_2D, F32_SPECIAL, MARK, MAX_POOL_2D, MUL, NONE, RELU, RELU6, RELU_N1_TO_1,
                            TANH, _conv, _open, _options_table, _sections_of, alexnet_body_model, bconv_options,
                            bireal_block_model, conv2d_op, cut_at, dense_block_model, ew_op, float_fixture, mixed_model, pool_op)
import synth
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

SAME, VALID = 0, 1
ACTS = (NONE, RELU, RELU_N1_TO_1, RELU6)
ALL_FLAGS = dict(elementwise_sections=True, pool_sections=True, conv1x1_sections=True)


# ---- the reference against its definition ----------------------------------------------------------------------------------------
def fma_triples(n, seed):
    """float32 triples (a, b, c) that stress a fused multiply-add: exponents over 2^+-70, sums that cancel exactly or nearly,
    half-ulp ties of the product against the addend, subnormal results, overflows and zeros of both signs."""
    g = np.random.default_rng(seed)
    mant = lambda k: (1.0 + g.integers(0, 2 ** 23, k) / 2.0 ** 23) * g.choice([-1.0, 1.0], k)
    a = (mant(n) * 2.0 ** g.integers(-70, 71, n)).astype(np.float32)
    b = (mant(n) * 2.0 ** g.integers(-70, 71, n)).astype(np.float32)
    c = (mant(n) * 2.0 ** g.integers(-70, 71, n)).astype(np.float32)
    kind = g.integers(0, 8, n)
    p = a.astype(np.float64) * b.astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        c = np.where(kind == 1, (-p).astype(np.float32), c)                                      # cancels up to the product's low bits
        c = np.where(kind == 2, (p * 2.0 ** 24).astype(np.float32), c)                           # the product is about half an ulp of c
        c = np.where(kind == 3, (p * 2.0 ** 25).astype(np.float32), c)
        small = (mant(n) * 2.0 ** g.integers(-75, -60, n)).astype(np.float32)
        a, b = np.where(kind == 4, small, a), np.where(kind == 4, small, b)                      # subnormal products
        c = np.where(kind == 4, (mant(n) * 2.0 ** g.integers(-149, -126, n)).astype(np.float32), c)
        big = (mant(n) * 2.0 ** g.integers(60, 68, n)).astype(np.float32)
        a, b = np.where(kind == 5, big, a), np.where(kind == 5, big, b)                          # overflows
        c = np.where(kind == 6, g.choice(np.array([0.0, -0.0], np.float32), n), c)
        # 12-bit factors: the product is a float32, and its negative cancels it exactly
        short = lambda k: (g.integers(2 ** 11, 2 ** 12, k) * g.choice([-1.0, 1.0], k) * 2.0 ** g.integers(-30, 31, k)).astype(np.float32)
        a, b = np.where(kind == 7, short(n), a), np.where(kind == 7, short(n), b)
        c = np.where(kind == 7, -(a * b), c)
    return a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)


def test_fma32_is_libms_fmaf():
    libm = C.CDLL("libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    a, b, c = fma_triples(6000, 1)
    extra = np.array([(1e-30, -1e-30, 0.0), (0.0, 0.0, -0.0), (-0.0, 0.0, -0.0), (-0.0, 0.0, 0.0), (1.0, 1.0, -1.0),
                      (np.inf, 0.0, 1.0), (np.inf, 1.0, -np.inf), (np.nan, 1.0, 1.0), (3e38, 2.0, -np.inf), (3e38, 2.0, -3e38),
                      (1e-45, 0.5, 0.0), (1e-45, 0.5, 1e-45), (1 + 2.0 ** -12, 1 + 2.0 ** -12, -1.0),
                      # the product lies 2^30 below the tie between c and its successor; float64 (ulp 2^48 there) rounds the sum
                      # onto the tie, which then goes to even: rounding twice gives the successor, fmaf gives c
                      (2.0 ** 38 * (1 + 2.0 ** -23), 2.0 ** 38 * (1 - 2.0 ** -23), 2.0 ** 100 * (1 + 2.0 ** -23))], np.float32)
    a, b, c = (np.concatenate([v, extra[:, k]]) for k, v in enumerate((a, b, c)))
    got = R.fma32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])
    # the triples do what they are for: subnormal and infinite results, exact zeros, and a case where rounding twice differs
    with np.errstate(over="ignore", invalid="ignore"):
        twice = (a.astype(np.float64) * b + c).astype(np.float32)
    assert np.sum((want != 0) & (np.abs(want) < 1e-38)) > 100 and np.isinf(want).sum() > 100 and np.sum(want == 0) > 100
    assert want[-1] == c[-1] and twice[-1] == np.nextafter(c[-1], np.float32(np.inf))


# (x, w, bias, the one output) -- worked by hand
P12 = np.float32(1 + 2.0 ** -12)
TINY = np.float32(1e-30)
SUB = np.array([0x00000001, 0x807FFFFF], np.uint32).view(np.float32)     # the smallest and the largest subnormal
KNOWN = [
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 exactly: fused onto -1 it is 2^-11 + 2^-24; the rounded product is 1 + 2^-11
    ("fused", [-1.0, P12], [1.0, P12], None, np.float32(2.0 ** -11 + 2.0 ** -24)),
    # in order: 1 + 2^24 -> 2^24 (the 1 is lost), - 2^24 -> 0; any other order gives 1
    ("ordered", [1.0, 2.0 ** 24, -2.0 ** 24], [1.0, 1.0, 1.0], None, np.float32(0.0)),
    ("minus_zero_1", [TINY], [-TINY], None, np.float32(-0.0)),
    # (the remaining channels carry zero products with w = +0: x < 0 there, so each is -0.0 and -0.0 + -0.0 stays -0.0)
    ("minus_zero_3", [TINY, -5.0, -7.0], [-TINY, 0.0, 0.0], None, np.float32(-0.0)),
    ("minus_zero_33", [TINY] + [-3.0] * 32, [-TINY] + [0.0] * 32, None, np.float32(-0.0)),
    ("minus_zero_bias", [TINY], [-TINY], 0.0, np.float32(0.0)),            # -0.0 + +0.0 = +0.0
    ("subnormal_0", [SUB[0]], [1.0], None, SUB[0]),
    ("subnormal_1", [SUB[1], SUB[0]], [1.0, 1.0], None, np.array([0x807FFFFE], np.uint32).view(np.float32)[0]),
]


def known_case(name):
    """(x [1,1,1,Cin], w [1,Cin], bias or None, expected float32 bits, expected bit word)."""
    _, x, w, bias, want = next(k for k in KNOWN if k[0] == name)
    want = np.float32(want)
    return (np.array(x, np.float32).reshape(1, 1, 1, -1), np.array(w, np.float32).reshape(1, -1),
            None if bias is None else np.array([bias], np.float32), int(want.view(np.uint32)), int(want < 0))


@pytest.mark.parametrize("name", [k[0] for k in KNOWN])
def test_known_answers_on_the_reference(name):
    x, w, bias, want, bit = known_case(name)
    got = R.conv1x1(x, w, bias)
    assert got.shape == (1, 1, 1, 1) and int(got.view(np.uint32)[0, 0, 0, 0]) == want
    assert O.bitpack(got).reshape(-1).tolist() == [bit]
    if name.startswith("minus_zero") and bias is None:
        assert want == 0x80000000 and bit == 0
    if name == "fused":                                      # multiply, round, then add gives 2^-11
        assert np.float32(np.float32(P12 * P12) + np.float32(-1.0)) == np.float32(2.0 ** -11)
    if name == "ordered":
        assert np.float32(np.float32(2.0 ** 24) + np.float32(-2.0 ** 24)) + np.float32(1) == 1


def test_the_padding_identities_of_the_k_tail():
    """What a kernel may feed for channels beyond Cin: fmaf(-0, +0, t) = t for every t, while fmaf(+0, +0, -0.0) = +0.0."""
    t = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -SUB[0]], np.float32)
    kept = R.fma32(np.float32(-0.0), np.float32(0.0), t)
    assert np.array_equal(kept.view(np.int32), t.view(np.int32))
    assert R.fma32(np.float32(0.0), np.float32(0.0), np.float32(-0.0)).view(np.uint32).reshape(-1).tolist() == [0]


def test_strides_select_pixels_and_the_clamp_passes_nan():
    g = np.random.default_rng(2)
    x = g.standard_normal((2, 5, 7, 3)).astype(np.float32)
    w = g.standard_normal((4, 3)).astype(np.float32)
    bias = g.standard_normal(4).astype(np.float32)
    full = R.conv1x1(x, w, bias)
    assert full.shape == (2, 5, 7, 4)
    for s in ((2, 2), (2, 1), (3, 4)):
        got = R.conv1x1(x, w, bias, s)
        assert got.shape == (2, *R.out_hw((5, 7), s), 4) and np.array_equal(got, full[:, ::s[0], ::s[1]])
    # against float64: Cin roundings of at most 2^-24 of the running magnitude each, and the bias add's
    exact = np.einsum("bhwc,oc->bhwo", x.astype(np.float64), w.astype(np.float64))
    bound = 4 * 2.0 ** -24 * (np.einsum("bhwc,oc->bhwo", np.abs(x).astype(np.float64), np.abs(w).astype(np.float64)) + np.abs(bias))
    assert np.all(np.abs(full - (exact + bias)) <= bound)
    x[0, 0, 0, 0], x[0, 0, 1, 0] = np.nan, np.inf
    for act in ACTS:
        got = R.conv1x1(x, w, None, 1, act)
        lo, hi = R.FLOAT_RANGE[act]
        assert np.isnan(got[0, 0, 0]).all() and not np.isnan(got[0, 0, 2:]).any()
        assert set(got[0, 0, 1].tolist()) <= {float(lo), float(hi)}          # an infinity is clamped, NONE included


GRID_IMAGES = [(1, 1), (5, 7), (8, 8)]
GRID_BATCHES = (1, 3)
GRID_CIN = (1, 2, 3, 31, 32, 33, 64, 65, 160)
GRID_COUT = (1, 31, 32, 33, 64, 96, 160)
GRID_STRIDES = ((1, 1), (2, 2), (2, 1))


def grid_operands(cin, cout, special=False):
    """(w, bias) of one (Cin, Cout) of the grid.  `special`: subnormal and tiny weights among them, so that subnormal products
    and sums occur."""
    g = np.random.default_rng(cin * 1000 + cout)
    w = (g.standard_normal((cout, cin)) * g.choice([1e-2, 1.0, 30.0], (cout, cin))).astype(np.float32)
    bias = g.standard_normal(cout).astype(np.float32)
    if special:
        w[g.integers(0, cout, max(1, cout // 4)), g.integers(0, cin, max(1, cout // 4))] = F32_SPECIAL[6]
        w[:, 0] *= np.float32(1e-36)
    return w, bias


def test_the_grid_fixtures_are_what_the_checks_need():
    """A fused chain differs from multiply-then-add on them, every activation clamps something, the special kind carries NaN,
    infinities and subnormal results, and negative zeros occur."""
    x = float_fixture((3, 5, 7, 33), 7)
    w, bias = grid_operands(33, 64)
    want = R.conv1x1(x, w, bias)
    t = np.zeros((x.shape[0] * 35, 64), np.float32)
    for c in range(33):
        t = (t + (x.reshape(-1, 33)[:, c:c + 1] * w[None, :, c]).astype(np.float32)).astype(np.float32)
    assert np.any((t + bias).astype(np.float32).reshape(want.shape) != want)
    for act in ACTS[1:]:
        assert np.any(R.conv1x1(x, w, bias, 1, act) != want)
    xs = float_fixture((3, 5, 7, 33), 8, special=True)
    ws, _ = grid_operands(33, 64, special=True)
    got = R.conv1x1(xs, ws)
    assert np.isnan(got).any() and np.isinf(xs).any() and np.any((got != 0) & (np.abs(got) < 1e-38))
    one = R.conv1x1(float_fixture((3, 5, 7, 1), 9, special=True), grid_operands(1, 33, special=True)[0])
    assert np.any(np.signbit(one) & (one == 0)) and np.any(~np.signbit(one) & (one == 0))


def dense_transition_model(H=8, C=64, seed=0):
    """A dense network's transition.  x (float) -> LceQuantize -> LceBconv2d (float) -> MUL (c) -> ADD (c, RELU) ->
    MAX_POOL_2D 2x2 / 2 -> CONV_2D 1x1 (C -> C/2, no bias) -> LceQuantize -> LceBconv2d (float, the graph output).  The
    convolution feeds ONLY the LceQuantize."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 401)
    h2, c2 = H // 2, C // 2
    x = f32([1, H, H, C], "x")
    q0 = b.tensor([1, H, H, C // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y0, c0 = _conv(b, q0, H, C, C, seed * 10 + 5)
    bn_m, bn_a = g.uniform(-1.5, 1.5, C).astype(np.float32), g.standard_normal(C).astype(np.float32)
    mm, aa = f32([1, H, H, C], "mm"), f32([1, H, H, C], "aa")
    mul = ew_op(b, MUL, [y0, f32([C], "bn_m", bn_m)], [mm], NONE)
    add = ew_op(b, ADD, [mm, f32([C], "bn_a", bn_a)], [aa], RELU)
    p = f32([1, h2, h2, C], "p")
    pool = pool_op(b, MAX_POOL_2D, [aa], [p], (2, 2), (2, 2), VALID)
    w = (g.standard_normal((c2, 1, 1, C)) * g.choice([-1.0, 1.0], (c2, 1, 1, C))).astype(np.float32)
    t = f32([1, h2, h2, c2], "t")
    conv = conv2d_op(b, [p, f32([c2, 1, 1, C], "w", w)], [t], (1, 1), VALID)
    q1 = b.tensor([1, h2, h2, (c2 + 31) // 32], np.int32, "q1")
    b.custom_op("LceQuantize", [t], [q1], b"")
    y1, c1 = _conv(b, q1, h2, c2, c2, seed * 10 + 6)
    b.inputs, b.outputs = [x], [y1]
    info = dict(convs=[c0, c1], bn_m=bn_m, bn_a=bn_a, mul=mul, add=add, pools=[pool], conv1x1=conv, w=w, wb=None,
                tensors=dict(aa=aa, p=p, t=t), size=H, channels=C)
    return b.finish(), x, y1, info


FIXTURES = dict(bireal=bireal_block_model, dense=dense_transition_model)


# ---- the partition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_each_fixture_is_one_section_with_the_three_flags(name):
    data, x, out, info = FIXTURES[name]()
    model = mr.LceModel(data, **ALL_FLAGS)
    n_ops = len(model.operators)
    k = info["conv1x1"]
    assert model.operators[k].builtin_code == CONV_2D
    assert [s.ops for s in model.sections] == [list(range(n_ops))]
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only and mr.Interpreter(data, **ALL_FLAGS).lce_only
    # without the conv1x1 flag: cut at the convolution, and only there
    without = mr.LceModel(data, elementwise_sections=True, pool_sections=True)
    # (the ADD that joins the shortcut becomes ready in the host's epoch then, and goes with it)
    assert [s.ops for s in without.sections] == cut_at(n_ops, [k] + ([info["join"]] if "join" in info else []))
    assert not mr.Interpreter(without).lce_only
    every = mr.LceModel(data, int8_add_sections=True, concat_sections=True, **ALL_FLAGS)
    assert [s.ops for s in every.sections] == [list(range(n_ops))]
    # the conv1x1 flag alone: the convolution joins only where it becomes ready in an LCE epoch -- behind a pool the host
    # runs it does not
    alone = mr.LceModel(data, conv1x1_sections=True)
    assert all(k not in s.ops for s in alone.sections)
    assert [(s.ops, s.inputs, s.outputs) for s in alone.sections] == [(s.ops, s.inputs, s.outputs) for s in mr.LceModel(data).sections]
    readers = [i for i, op in enumerate(model.operators) if model.operators[k].outputs[0] in op.inputs]
    assert [model.operators[i].custom_code or model.operators[i].builtin_code for i in readers] == \
        (["LceQuantize"] if name == "dense" else [ADD])


def test_files_without_a_qualifying_convolution_keep_their_partitions():
    """The mixed graph's stem CONV_2D is 3x3 without an options table; the other files have no CONV_2D."""
    for data in (dense_block_model()[0], mixed_model()[0], alexnet_body_model()[0]):
        for kw in ({}, dict(elementwise_sections=True), dict(elementwise_sections=True, concat_sections=True, pool_sections=True)):
            a, b = mr.LceModel(data, **kw), mr.LceModel(data, conv1x1_sections=True, **kw)
            assert [(s.ops, s.inputs, s.outputs) for s in a.sections] == [(s.ops, s.inputs, s.outputs) for s in b.sections]


JOINS = ["joins", "no_bias_two_inputs", "no_bias_minus_one", "stride_2", "stride_2_1_odd", "valid", "relu6", "no_dilations", "ragged_channels"]
STAYS = ["one_input", "four_inputs", "two_outputs", "int8_input", "int8_filter", "int8_output", "int32_bias", "three_d_output",
         "three_d_input", "constant_input", "filter_not_constant", "filter_3x3", "filter_2_d", "filter_cin", "bias_not_constant",
         "bias_length", "bias_2_d", "output_channels", "no_options", "zero_stride", "negative_stride", "huge_stride", "dilation_w",
         "dilation_h", "padding_2", "tanh", "sign_bit", "extent_off_by_one", "depthwise", "stem"]


def _graph(case):
    """x -> LceQuantize -> LceBconv2d -> y -> <CONV_2D under test> -> z -> LceQuantize -> q2, with one condition of the
    candidate rule broken per case of STAYS.  Returns (file, index of the convolution)."""
    Hh, Cc, Co = 8, 64, 32
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
    kw, zshape, code = {}, [1, Hh, Hh, Co], CONV_2D
    flt = const(f32, [Co, 1, 1, Cc], "k")
    kb = const(f32, [Co], "kb")
    z_make, outs_extra = f32, []
    if case == "no_bias_two_inputs":
        kb = None
    elif case == "no_bias_minus_one":
        kb = -1
    elif case == "stride_2":
        kw, zshape = dict(stride=(2, 2)), [1, Hh // 2, Hh // 2, Co]
    elif case == "stride_2_1_odd":
        kw, zshape = dict(stride=(3, 1)), [1, 3, Hh, Co]
    elif case == "valid":
        kw = dict(padding=VALID)
    elif case == "relu6":
        kw = dict(activation=RELU6)
    elif case == "no_dilations":
        kw = dict(dilation=None)
    elif case == "ragged_channels":
        flt, kb, zshape = const(f32, [33, 1, 1, Cc], "k33"), const(f32, [33], "kb33"), [1, Hh, Hh, 33]
    elif case == "int8_filter":
        flt = i8([Co, 1, 1, Cc], "k8", np.ones([Co, 1, 1, Cc], np.int8))
    elif case == "int8_output":
        z_make = i8
    elif case == "int32_bias":
        kb = b.tensor([Co], np.int32, "kb32", np.ones(Co, np.int32))
    elif case == "three_d_output":
        zshape = [Hh, Hh, Co]
    elif case == "filter_not_constant":
        flt = f32([Co, 1, 1, Cc], "kv")
    elif case == "filter_3x3":
        flt = const(f32, [Co, 3, 3, Cc], "k3")
    elif case == "filter_2_d":
        flt = const(f32, [Co, Cc], "k2")
    elif case == "filter_cin":
        flt = const(f32, [Co, 1, 1, Cc // 2], "kc")
    elif case == "bias_not_constant":
        kb = f32([Co], "kbv")
    elif case == "bias_length":
        kb = const(f32, [Co + 1], "kb33")
    elif case == "bias_2_d":
        kb = const(f32, [1, Co], "kb2")
    elif case == "output_channels":
        zshape = [1, Hh, Hh, Co * 2]
    elif case == "no_options":
        kw = dict(options=False)
    elif case == "zero_stride":
        kw = dict(stride=(0, 1))
    elif case == "negative_stride":
        kw = dict(stride=(1, -1))
    elif case == "huge_stride":
        kw, zshape = dict(stride=(2 ** 31 - 1, 2 ** 31 - 1)), [1, 1, 1, Co]
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
        kw, zshape = dict(stride=(2, 2)), [1, Hh // 2 + 1, Hh // 2, Co]
    elif case == "depthwise":
        code = DEPTHWISE_CONV_2D
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
    k = conv2d_op(b, ins, [z] + outs_extra, code=code, **kw)
    q2 = b.tensor(zshape[:-1] + [(zshape[-1] + 31) // 32], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = [x], [q2]
    return b.finish(), k


@pytest.mark.parametrize("case", STAYS)
def test_convolutions_that_stay_with_the_host(case):
    data, k = _graph(case)
    model = mr.LceModel(data, int8_add_sections=True, concat_sections=True, **ALL_FLAGS)
    assert all(k not in s.ops for s in model.sections), (case, [s.ops for s in model.sections])
    assert not mr.Interpreter(model).lce_only
    assert [(s.ops, s.inputs, s.outputs) for s in model.sections] == [(s.ops, s.inputs, s.outputs) for s in mr.LceModel(data).sections]


@pytest.mark.parametrize("case", JOINS)
def test_a_qualifying_convolution_joins(case):
    data, k = _graph(case)
    model = mr.LceModel(data, conv1x1_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and k == 2
    assert mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]
    assert [s.ops for s in mr.LceModel(data, elementwise_sections=True, int8_add_sections=True, concat_sections=True,
                                       pool_sections=True).sections] == [[0, 1], [3]]


# ---- the reader -----------------------------------------------------------------------------------------------------------------
def _options_model(rows):
    """One CONV_2D per row (padding, stride_w, stride_h, activation, dilation_w, dilation_h), (padding, stride_w, stride_h,
    activation) for a table without the dilations, or None for a convolution without an options table, each followed by an ADD."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, 4, 4, 4], "x")
    k = f32([4, 1, 1, 4], "k", np.ones((4, 1, 1, 4), np.float32))
    prev = x
    for n, row in enumerate(rows):
        out = f32([1, 4, 4, 4], "t%d" % n)
        if row is None:
            conv2d_op(b, [prev, k], [out], options=False)
        else:
            conv2d_op(b, [prev, k], [out], (row[2], row[1]), row[0], row[3], None if len(row) == 4 else (row[5], row[4]))
        prev = f32([1, 4, 4, 4], "u%d" % n)
        ew_op(b, ADD, [out, out], [prev], RELU)
    b.inputs, b.outputs = [x], [prev]
    return b.finish()


def test_conv2d_options_round_trip_through_the_reader():
    rows = [(VALID, 2, 3, RELU6, 4, 5), (SAME, 1, 1, NONE, 1, 1), None, (VALID, 2, 2, RELU), (1, 2 ** 31 - 1, -7, 5, 0, -2 ** 31),
            (-1, 9, 8, RELU_N1_TO_1, 7, 6)]
    model = mr.LceModel(_options_model(rows))
    convs, others = model.operators[0::2], model.operators[1::2]
    for op, row in zip(convs, rows):
        assert op.builtin_code == CONV_2D
        got = (op.padding, op.stride_w, op.stride_h, op.activation, op.dilation_w, op.dilation_h)
        want = (0, 0, 0, 0, 1, 1) if row is None else row + (1, 1) if len(row) == 4 else row     # the schema's defaults
        assert got == want, row
        assert (op.filter_width, op.filter_height) == (0, 0)
    for op in others:                                                                  # every other operator
        assert (op.padding, op.stride_w, op.stride_h, op.dilation_w, op.dilation_h) == (0, 0, 0, 1, 1) and op.activation == RELU
    v = (C.c_int32 * 5)()
    lib = mr.tflite_lib()
    assert lib.lce_tflite_model_operator_conv2d(model._h, 0, v) == amd.OK and list(v) == [VALID, 2, 3, 4, 5]
    assert lib.lce_tflite_model_operator_conv2d(model._h, len(model.operators), v) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_conv2d(model._h, -1, v) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_conv2d(model._h, 0, None) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_conv2d(None, 0, v) == amd.ERR_INVALID


def test_a_truncated_or_out_of_bounds_options_table_is_refused_at_open():
    data = bytearray(_options_model([(VALID, 2, 2, NONE, MARK, 3)]))
    assert mr.LceModel(bytes(data)).operators[0].dilation_w == MARK
    table, ref, slot = _options_table(data)              # (six fields like Pool2DOptions; MARK sits in field 4 as there)
    bad = []
    for target in (len(data) - 2, len(data), len(data) + 4096, 2 ** 32 - 8 - ref):   # cut short by the end of the file; beyond it
        d = bytearray(data)
        struct.pack_into("<I", d, ref, (target - ref) % 2 ** 32)
        bad.append(bytes(d))
    for soffset in (table + 8, -(len(data) + 64), 2 ** 31 - 1):                        # the table's vtable lies outside the file
        d = bytearray(data)
        struct.pack_into("<i", d, table, soffset)
        bad.append(bytes(d))
    for field in range(6):                                                             # each field far outside the file
        d = bytearray(data)
        struct.pack_into("<H", d, slot - 2 * 4 + 2 * field, 0xFFF0)
        bad.append(bytes(d))
    assert len(bad) == 13
    for d in bad:
        for kw in ({}, ALL_FLAGS):
            with pytest.raises(ValueError, match="Conv2DOptions"):
                mr.LceModel(d, **kw)


# ---- shape inference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
def test_section_tensor_shape_over_the_convolved_tensors(batch):
    data, x, out, info = bireal_block_model()
    model = mr.LceModel(data, **ALL_FLAGS)
    t = info["tensors"]
    assert model.section_tensor_shape(0, t["p"], batch) == ((batch, 4, 4, 64), batch * 16 * 64 * 4)
    assert model.section_tensor_shape(0, t["s"], batch) == ((batch, 4, 4, 128), batch * 16 * 128 * 4)
    assert model.section_tensor_shape(0, out, batch) == ((batch, 4, 4, 128), batch * 16 * 128 * 4)
    data, x, out, info = dense_transition_model()
    model = mr.LceModel(data, **ALL_FLAGS)
    assert model.section_tensor_shape(0, info["tensors"]["t"], batch) == ((batch, 4, 4, 32), batch * 16 * 32 * 4)
    for case, want in (("stride_2", (batch, 4, 4, 32)), ("stride_2_1_odd", (batch, 3, 8, 32)), ("ragged_channels", (batch, 8, 8, 33))):
        data, k = _graph(case)
        model = mr.LceModel(data, conv1x1_sections=True)
        assert model.section_tensor_shape(0, model.operators[k].outputs[0], batch)[0] == want
        assert model.section_tensor_shape(0, model.outputs[0], batch)[0] == want[:3] + ((want[3] + 31) // 32,)


@pytest.mark.parametrize("declared", [32, 96])
def test_a_file_whose_convolution_input_disagrees_with_the_inferred_shape_is_refused(declared):
    """The convolution's tensors agree with each other in the file, but the binary convolution produces 64 channels where the
    file declares `declared` for its output: the walk must fail instead of reading past (or short of) its buffer."""
    Hh, Cc = 8, 64
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x, y, z = f32([1, Hh, Hh, Cc], "x"), f32([1, Hh, Hh, declared], "y"), f32([1, Hh, Hh, 32], "z")
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                bconv_options(spec))
    conv2d_op(b, [y, f32([32, 1, 1, declared], "k", np.ones((32, 1, 1, declared), np.float32))], [z])
    b.inputs, b.outputs = [x], [z]
    model = mr.LceModel(b.finish(), conv1x1_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2]]
    with pytest.raises(amd.LceHipError, match="CONV_2D input") as e:
        model.section_tensor_shape(0, z, 2)
    assert e.value.code == amd.ERR_INVALID


# ---- lce_hip_conv1x1_f32 / amd.conv1x1 argument checks (no device needed: they come first) ----------------------------------------
def _desc(**kw):
    d = dict(batch=2, in_height=8, in_width=8, channels_in=64, channels_out=32, stride_height=1, stride_width=1, activation=amd.ACT_NONE)
    d.update(kw)
    return amd.Conv1x1Desc(*[d[n] for n, _ in amd.Conv1x1Desc._fields_])


# the input is 2 x 8 x 8 x 64 floats = 32 KiB at 4096, the filter 32 x 64 floats = 8 KiB, the bias 128 bytes, the output
# 2 x 8 x 8 x 32 floats = 16 KiB, the bits 2 x 8 x 8 words = 512 bytes
PTRS = dict(inp=4096, flt=1 << 18, bias=1 << 19, out=1 << 20, bits=1 << 21)


def _c_call(desc=True, **kw):
    p = dict(PTRS)
    p.update({k: kw.pop(k) for k in list(kw) if k in PTRS})
    d = _desc(**kw)
    return amd.lib().lce_hip_conv1x1_f32(C.byref(d) if desc else None, *[C.c_void_p(p[k]) for k in ("inp", "flt", "bias", "out", "bits")], None)


REFUSALS = [
    (dict(desc=False), amd.ERR_INVALID, "null desc"),
    (dict(inp=0), amd.ERR_INVALID, "null input"),
    (dict(flt=0), amd.ERR_INVALID, "null filter"),
    (dict(out=0, bits=0), amd.ERR_INVALID, "both outputs"),
    (dict(batch=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_height=-1), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_width=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(channels_in=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(channels_out=-3), amd.ERR_INVALID, "extents must be positive"),
    (dict(stride_height=0), amd.ERR_INVALID, "stride must be positive"),
    (dict(stride_width=-1), amd.ERR_INVALID, "stride must be positive"),
    (dict(activation=4), amd.ERR_INVALID, "unknown activation"),
    (dict(activation=-1), amd.ERR_INVALID, "unknown activation"),
    (dict(batch=2 ** 20, in_height=2 ** 6, in_width=2 ** 6, channels_in=1, channels_out=1, inp=1 << 40, out=1 << 50, bits=1 << 60),
     amd.ERR_UNSUPPORTED, "2\\^31 pixels"),
    (dict(stride_height=2 ** 31 - 1, stride_width=2 ** 31 - 1), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(stride_width=2 ** 30 + 1), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(batch=1, channels_in=1, in_height=2 ** 30 + 1, in_width=1, stride_height=2, inp=1 << 40, out=1 << 50, bits=1 << 60),
     amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(channels_out=65535 * 128 + 1, batch=1, in_height=1, in_width=1, channels_in=1, out=1 << 40, bits=1 << 50), amd.ERR_UNSUPPORTED,
     "output channels"),
    (dict(out=4096 + 512), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=4096 - 16), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=0, bits=4096 + 32768 - 4), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=(1 << 18) + 8192 - 4), amd.ERR_INVALID, "overlaps the filter"),
    (dict(out=0, bits=(1 << 18) - 508), amd.ERR_INVALID, "overlaps the filter"),
    (dict(out=(1 << 19) - 16380), amd.ERR_INVALID, "overlaps the bias"),
    (dict(out=0, bits=(1 << 19) + 124), amd.ERR_INVALID, "overlaps the bias"),
    (dict(bits=(1 << 20) + 16380), amd.ERR_INVALID, "outputs overlap"),
    (dict(bits=(1 << 21) + 2), amd.ERR_INVALID, "4-byte aligned"),
    (dict(inp=4097), amd.ERR_INVALID, "4-byte aligned"),
]


@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_c_entry_refuses_bad_arguments(kw, code, msg):
    assert _c_call(**dict(kw)) == code
    assert re.search(msg, amd.lib().lce_hip_last_error().decode()), amd.lib().lce_hip_last_error()


def test_c_entry_accepts_the_edges_of_the_checks_up_to_the_device():
    """Touching ranges do not overlap; a NULL bias, either output alone, the largest stride and every activation pass.  Without a
    device the accepted calls end at ERR_NO_DEVICE; none of them is ERR_INVALID or ERR_UNSUPPORTED."""
    edges = (dict(out=4096 + 32768), dict(out=4096 - 16384), dict(bits=(1 << 20) + 16384), dict(out=0), dict(bits=0), dict(bias=0),
             dict(out=(1 << 18) + 8192), dict(out=(1 << 19) + 128), dict(bias=0, out=1 << 19),   # (no bias: nothing there to overlap)
             dict(stride_height=2 ** 30, stride_width=2 ** 30), dict(inp=4100, flt=(1 << 18) + 4, out=(1 << 20) + 12),
             dict(activation=amd.ACT_RELU), dict(activation=amd.ACT_RELU_N1_TO_1), dict(activation=amd.ACT_RELU6),
             dict(channels_in=1, channels_out=1), dict(channels_in=2 ** 20, channels_out=1, inp=1 << 40, flt=1 << 50))
    oh, ow = C.c_int32(), C.c_int32()
    for kw in edges:
        d = _desc(**{k: v for k, v in kw.items() if k not in PTRS})
        assert amd.lib().lce_hip_conv1x1_f32_check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK, kw
        if amd.device_count() == 0:
            assert _c_call(**dict(kw)) == amd.ERR_NO_DEVICE, kw
    check = amd.lib().lce_hip_conv1x1_f32_check
    d = _desc(in_height=7, in_width=9, stride_height=2, stride_width=3)
    assert check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (4, 3)
    d = _desc(in_height=7, in_width=9, stride_height=8, stride_width=9)
    assert check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (1, 1)
    assert check(C.byref(d), None, None) == amd.OK
    assert check(None, None, None) == amd.ERR_INVALID
    for kw, code, _ in REFUSALS:                             # the descriptor's refusals are the check's own
        if not set(kw) & (set(PTRS) | {"desc"}) or code == amd.ERR_UNSUPPORTED:
            d = _desc(**{k: v for k, v in kw.items() if k not in PTRS})
            assert check(C.byref(d), None, None) == code, kw


X = np.zeros((2, 8, 8, 64), np.float32)
W = np.zeros((32, 64), np.float32)


@pytest.mark.parametrize("x,w,kw,msg", [
    (X.astype(np.float64), W, {}, "float32 NHWC"),
    (X[0], W, {}, "NHWC"),
    (np.zeros((2, 0, 8, 64), np.float32), W, {}, "non-empty"),
    (X, W.astype(np.float64), {}, "w must be"),
    (X, np.zeros((32, 63), np.float32), {}, "w must be"),
    (X, np.zeros((32, 3, 3, 64), np.float32), {}, "w must be"),
    (X, np.zeros((0, 64), np.float32), {}, "w must be"),
    (X, W, dict(bias=np.zeros(31, np.float32)), "bias must be"),
    (X, W, dict(bias=np.zeros(32, np.float64)), "bias must be"),
    (X, W, dict(stride=0), "stride must be"),
    (X, W, dict(stride=(1, -1)), "stride must be"),
    (X, W, dict(stride=(2, 2, 2)), "stride must be"),
    (X, W, dict(activation=4), "unknown activation"),
    (X, W, dict(out=False), "no output"),
    (X, W, dict(out=np.zeros((2, 8, 8, 31), np.float32)), "out must be"),
    (X, W, dict(out=np.zeros((2, 8, 8, 32), np.int8)), "out must be"),
    (X, W, dict(stride=2, out=np.zeros((2, 8, 8, 32), np.float32)), "out must be"),
    (X, W, dict(out_bits=np.zeros((2, 8, 8, 2), np.int32)), "out_bits must be"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, x, w, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    with pytest.raises(ValueError, match=msg):
        amd.conv1x1(x, w, **kw)


# ---- the opt-in -----------------------------------------------------------------------------------------------------------------
def pack(size, sections, ext=0, reserved=(0,) * 7):
    """The options bytes of one of the three forms: exactly `size` bytes."""
    assert size in (8, 24, 40)
    return struct.pack("<10I", size, sections, ext, *reserved)[:size]


def test_open_opts_has_a_third_size():
    lib = mr.tflite_lib()
    assert C.sizeof(mr._OpenOptions) == 8 and C.sizeof(mr._OpenOptionsExt) == 24 and C.sizeof(mr._OpenOptions40) == 40
    shape = lambda h: _sections_of(h)
    for data in (bireal_block_model()[0], dense_transition_model()[0], alexnet_body_model()[0], mixed_model()[0]):
        for sections in range(8):
            kw = dict(elementwise_sections=bool(sections & 1), int8_add_sections=bool(sections & 2), concat_sections=bool(sections & 4))
            want = {ext: [(s.ops, s.inputs, s.outputs) for s in mr.LceModel(data, pool_sections=bool(ext & 1), conv1x1_sections=bool(ext & 2), **kw).sections]
                    for ext in range(4)}
            h8, _ = _open(data, pack(8, sections))                         # sizes 8 and 24 behave as before: nothing behind them is read
            assert len(pack(8, sections)) == 8 and h8 and shape(h8) == want[0]
            lib.lce_tflite_model_close(h8)
            for ext in (0, 1):
                h24, _ = _open(data, pack(24, sections, ext))
                assert len(pack(24, sections, ext)) == 24 and h24 and shape(h24) == want[ext], (sections, ext)
                lib.lce_tflite_model_close(h24)
            for ext in range(4):                                           # size 40: ext 0 and 1 give the same partitions, 2 and 3 are new
                h40, _ = _open(data, pack(40, sections, ext))
                assert h40 and shape(h40) == want[ext], (sections, ext)
                lib.lce_tflite_model_close(h40)
        for ext in (2, 3):                                                 # the new bit is accepted only at size 40
            h, err = _open(data, pack(24, 1, ext))
            assert not h and b"flags" in err
        h, _ = _open(data, pack(8, 1, 2))                                  # (size 8 reads no ext at all)
        assert h
        lib.lce_tflite_model_close(h)
        for ext in (4, 6, 8, 1 << 31):
            h, err = _open(data, pack(40, 1, ext))
            assert not h and b"flags" in err, ext
        for sections in (8, 16, 1 << 31):
            h, err = _open(data, pack(40, sections, 2))
            assert not h and b"flags" in err
        for k in range(7):                                                 # each of the seven trailing words
            reserved = [0] * 7
            reserved[k] = 1 << (k * 4)
            h, err = _open(data, pack(40, 1, 2, reserved))
            assert not h and b"reserved" in err, k
        for size in (0, 4, 12, 16, 20, 28, 32, 36, 44, 48, 64):
            raw = struct.pack("<16I", size, 1, 2, *([0] * 13))[:max(size, 8)]
            h, err = _open(data, raw)
            assert not h and b"struct_size" in err, size
    body = bireal_block_model()[0]
    one, cut = _open(body, pack(40, 1, 3))[0], _open(body, pack(24, 1, 1))[0]
    assert len(shape(one)) == 1 and len(shape(cut)) == 2
    lib.lce_tflite_model_close(one)
    lib.lce_tflite_model_close(cut)


def test_the_python_constructor_uses_the_40_byte_options_only_for_the_conv1x1_flag(monkeypatch):
    data = bireal_block_model()[0]
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
    mr.LceModel(data, elementwise_sections=True, concat_sections=True, pool_sections=True, conv1x1_sections=True)
    assert calls == [("lce_tflite_model_open_ex", 1), ("lce_tflite_model_open_opts", 8, 4, None), ("lce_tflite_model_open_opts", 24, 0, 1),
                     ("lce_tflite_model_open_opts", 40, 0, 2), ("lce_tflite_model_open_opts", 40, 5, 3)]


def test_the_abi():
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_conv1x1_f32", "lce_hip_conv1x1_f32_check"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    for name in ("lce_tflite_model_conv1x1_stats", "lce_tflite_model_operator_conv2d"):
        assert hasattr(mr.tflite_lib(), name)
    assert C.sizeof(amd.Conv1x1Desc) == 32
    err = C.create_string_buffer(128)
    data = bireal_block_model()[0]
    for flags in (4, 8):                                     # open_ex keeps its own mask
        assert not mr.tflite_lib().lce_tflite_model_open_ex(data, len(data), flags, err, 128)


def test_stats_are_zero_before_any_run():
    model = mr.LceModel(bireal_block_model()[0], **ALL_FLAGS)
    assert model.conv1x1_stats() == (0, 0) and model.pool_stats() == (0, 0)
    mr.tflite_lib().lce_tflite_model_conv1x1_stats(model._h, None, None)      # any pointer may be NULL
    mr.tflite_lib().lce_tflite_model_conv1x1_stats(None, None, None)


# ---- the build: no scratch memory, no spills ----------------------------------------------------------------------------------------
def test_the_kernel_uses_no_scratch_and_spills_nothing():
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_conv1x1.hip")
    assert len(kernels) == 2 and all("conv1x1_f32" in k for k in kernels), kernels     # the 16-byte and the scalar load path
    for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
        assert resources[key] == ["0"] * 2, (key, resources[key])
    # two tiles of 128 rows x 36 floats
    assert resources["LDS Size [bytes/block]"] == [str(2 * 128 * 36 * 4)] * 2
    assert "v_mfma_f32_32x32x2_f32" in mnemonics and "global_load_dwordx4" in mnemonics and "ds_read_b128" in mnemonics
