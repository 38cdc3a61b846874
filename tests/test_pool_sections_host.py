"""Builtin 2-D pooling between binary layers inside the sections (LCE_TFLITE_SECTIONS_EXT_POOL, include/lce_tflite_model.h) on the
CPU: the arithmetic contract of lce_hip_pool2d as known answers worked by hand against the NumPy reference (tests/pool_ref.py),
the reference against itself, the partition with and without the opt-in, every condition that keeps a pool with the host,
Pool2DOptions through the reader, shape inference over the pooled tensors, the size-versioned options of
lce_tflite_model_open_opts, the argument checks of lce_hip_pool2d / amd.pool2d (which all fail before any device is touched) and
the build of the new kernels.  Also the fixtures of the GPU side (tests/test_gpu_pool.py)."""
import ctypes as C
import importlib
import mmap
import re
import struct

import numpy as np
import pytest

import hipcc_lib as H
import oracle_lib as O
import pool_ref as R
from section_models import (ADD, AVERAGE_POOL_2D, MARK, MAX_POOL_2D, NONE, RELU, RELU6, RELU_N1_TO_1, TANH, _conv, _open,
                            _options_table, _sections_of, alexnet_body_model, bconv_options, cut_at, dense_block_model, ew_op,
                            mixed_model, pool_op)
import synth
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

SAME, VALID = R.SAME, R.VALID
ACTS = (NONE, RELU, RELU_N1_TO_1, RELU6)
FLT_MAX = R.FLT_MAX


# ---- known answers, worked by hand ----------------------------------------------------------------------------------------
def test_float_average_sums_in_tap_order_with_one_rounding_per_add():
    """A 2x3 SAME window on a 1x3 image: the second filter row is padding, so the middle output has the three taps of the row.
    2^24 + 1 rounds back to 2^24 (ties to even), and again: the sequential sum is 2^24, 2^24 / 3 = 5592405.33 rounds to the
    float32 grid of 0.5: 5592405.5.  A pairwise sum would give 2^24 + (1 + 1) = 16777218 = 3 x 5592406 exactly."""
    x = np.array([2.0 ** 24, 1.0, 1.0], np.float32).reshape(1, 1, 3, 1)
    got = R.pool2d(x, R.AVERAGE, (2, 3), (1, 1), SAME)
    assert got.shape == (1, 1, 3, 1)
    assert got.reshape(-1).tolist() == [8388608.0, 5592405.5, 1.0]           # 2 taps: (2^24 + 1 -> 2^24) / 2; 3 taps; 2 taps: 2 / 2
    assert float(np.float32(2.0 ** 24 + 2.0) / np.float32(3)) == 5592406.0


# (taps n, sum a, rounded quotient): a = +-n/2 are the exact ties of an even count -- away from zero --, 9 has none
INT8_KNOWN = [(2, 1, 1), (2, -1, -1), (4, 2, 1), (4, -2, -1), (4, 1, 0), (4, -1, 0), (6, 3, 1), (6, -3, -1), (6, 2, 0), (6, -2, 0),
              (9, 4, 0), (9, -4, 0), (9, 5, 1), (9, -5, -1), (9, 13, 1), (9, 14, 2), (9, -13, -1), (9, -14, -2)]
WINDOW_OF = {2: (1, 2), 4: (2, 2), 6: (2, 3), 9: (3, 3)}


def int8_known_case(n):
    """A VALID window of n taps that is the whole image: channel k holds sum a_k in its first tap and zeros elsewhere.  Returns
    (x, filter, expected output)."""
    rows = [(a, q) for m, a, q in INT8_KNOWN if m == n]
    fh, fw = WINDOW_OF[n]
    x = np.zeros((1, fh, fw, len(rows)), np.int8)
    x[0, 0, 0, :] = [a for a, _ in rows]
    return x, (fh, fw), np.array([q for _, q in rows], np.int8).reshape(1, 1, 1, -1)


@pytest.mark.parametrize("n", sorted(WINDOW_OF))
def test_int8_average_rounds_ties_away_from_zero(n):
    x, filt, want = int8_known_case(n)
    assert np.array_equal(R.pool2d(x, R.AVERAGE, filt, (1, 1), VALID, scale=1.0, zero_point=0), want)
    # the same through C's arithmetic, written out: (a +- n/2) / n truncating
    for m, a, q in INT8_KNOWN:
        num = a + m // 2 if a > 0 else a - m // 2
        assert int(num / m) == q, (m, a)


def test_float_max_of_nan_and_minus_infinity_is_minus_flt_max():
    x = np.array([np.nan, -np.inf, -np.inf, np.nan], np.float32).reshape(1, 2, 2, 1)
    got = R.pool2d(x, R.MAX, (2, 2), (2, 2), VALID)
    assert got.shape == (1, 1, 1, 1) and got[0, 0, 0, 0] == -FLT_MAX
    # a NaN never replaces the running maximum, wherever it stands; an infinity is clamped to the range of NONE
    y = np.array([np.nan, 2.0, np.nan, -1.0, np.inf, 1.0, np.nan, np.nan], np.float32).reshape(1, 2, 2, 2)
    assert R.pool2d(y, R.MAX, (2, 2), (2, 2), VALID).reshape(-1).tolist() == [float(FLT_MAX), 2.0]


def test_quantized_activation_ranges_at_one_scale_and_zero_point():
    """scale 0.05, zero point -3: Q(0) = -3, Q(6) = -3 + 120 = 117, Q(-1) = -3 - 20 = -23, Q(1) = -3 + 20 = 17."""
    want = {NONE: (-128, 127), RELU: (-3, 127), RELU_N1_TO_1: (-23, 17), RELU6: (-3, 117)}
    for act, r in want.items():
        assert R.quantized_range(act, 0.05, -3) == r
        p = amd.add_int8_params((0.05, -3), (0.05, -3), (0.05, -3), act)     # the library's ONE copy of the computation
        assert (p["act_min"], p["act_max"]) == r
    assert R.quantized_range(RELU6, 0.01, -128) == (-128, 127)                # saturates at the type's range
    assert R.quantized_range(RELU, 0.5, 127) == (127, 127)


# ---- the reference against itself -----------------------------------------------------------------------------------------
GRID_WINDOWS = [(2, 2, 2, 2, VALID), (3, 3, 2, 2, VALID), (3, 3, 2, 2, SAME), (2, 2, 2, 2, SAME), (3, 3, 1, 1, SAME), (3, 2, 1, 2, SAME),
                (1, 1, 1, 1, VALID), "global"]
GRID_IMAGES = [(7, 7), (8, 6), (5, 9)]


def window_of(w, image):
    """(filter, stride, padding) of a grid window on `image`; "global": the filter is the whole image, VALID."""
    if w == "global":
        return tuple(image), (1, 1), VALID
    return (w[0], w[1]), (w[2], w[3]), w[4]


def explicit_windows(x, filt, stride, padding):
    """Per output pixel the list of in-bounds taps in raster order, by the definition (no slicing tricks)."""
    _, h, w, _ = x.shape
    (oh, ph), (ow, pw) = R.out_and_pad(h, filt[0], stride[0], padding), R.out_and_pad(w, filt[1], stride[1], padding)
    for oy in range(oh):
        for ox in range(ow):
            taps = [(oy * stride[0] - ph + fy, ox * stride[1] - pw + fx) for fy in range(filt[0]) for fx in range(filt[1])]
            yield oy, ox, [(y, xx) for y, xx in taps if 0 <= y < h and 0 <= xx < w]


@pytest.mark.parametrize("w", GRID_WINDOWS, ids=str)
def test_the_reference_agrees_with_the_definition(w):
    for image in GRID_IMAGES:
        filt, stride, padding = window_of(w, image)
        g = np.random.default_rng(image[0])
        x = g.standard_normal((2, *image, 3)).astype(np.float32)
        xi = g.integers(-128, 128, (2, *image, 3)).astype(np.int8)
        mx, av = R.pool2d(x, R.MAX, filt, stride, padding), R.pool2d(x, R.AVERAGE, filt, stride, padding)
        mi, ai = (R.pool2d(xi, op, filt, stride, padding, scale=1.0, zero_point=0) for op in (R.MAX, R.AVERAGE))
        seen = 0
        for oy, ox, taps in explicit_windows(x, filt, stride, padding):
            assert taps
            vals = np.stack([x[:, y, xx, :] for y, xx in taps])
            assert np.array_equal(mx[:, oy, ox, :], vals.max(axis=0))
            # float32 sequential sum against the float64 mean: n roundings of at most 2^-24 sum|x| each, and the division's
            n = len(taps)
            bound = n * 2.0 ** -23 * np.abs(vals.astype(np.float64)).sum(axis=0) / n
            assert np.all(np.abs(av[:, oy, ox, :] - vals.astype(np.float64).mean(axis=0)) <= bound)
            ivals = np.stack([xi[:, y, xx, :] for y, xx in taps]).astype(np.int64)
            assert np.array_equal(mi[:, oy, ox, :], ivals.max(axis=0))
            a = ivals.sum(axis=0)
            num = np.where(a > 0, a + n // 2, a - n // 2)
            assert np.array_equal(ai[:, oy, ox, :], np.sign(num) * (np.abs(num) // n))
            seen += 1
        assert seen == mx.shape[1] * mx.shape[2]


def test_extents_and_paddings_are_the_oracles():
    """ComputePaddingHeightWidth as the oracle computes it for a convolution of the same filter, stride and padding."""
    for size in range(1, 12):
        for f in range(1, 5):
            for s in range(1, 4):
                for padding in (SAME, VALID):
                    spec = O.ConvSpec(1, size, size + 1, 32, f, f, 32, stride_h=s, stride_w=s,
                                      padding=O.PADDING_SAME if padding == SAME else O.PADDING_VALID, pad_values=1)
                    if spec.out_h <= 0 or spec.out_w <= 0:
                        assert R.out_and_pad(size, f, s, padding)[0] <= 0
                        continue
                    assert R.out_and_pad(size, f, s, padding) == (spec.out_h, spec.pad_h), (size, f, s, padding)
                    assert R.out_and_pad(size + 1, f, s, padding) == (spec.out_w, spec.pad_w)
                    assert amd.pool2d_output_hw((size, size + 1), (f, f), (s, s), padding) == (spec.out_h, spec.out_w)


# ---- the fixtures of the GPU side -------------------------------------------------------------------------------------------
INT8_Q = (0.05, -3)                    # scale and zero point of the int8 kernel fixtures (the ranges worked out above)
F32_SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x80000001,
                        0x007FFFFF, 0x807FFFFF], np.uint32).view(np.float32)   # +-0, +-inf, NaNs, smallest / largest subnormals


def float_fixture(shape, seed, kind):
    """kind "max": normals with +-inf, NaN, +-0 and subnormals planted.  "average": finite values and subnormals.
    "average_inf": the average fixture with +-inf planted."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(shape) * g.choice([1e-3, 1.0, 3.0, 1e4], shape)).astype(np.float32)
    flat = x.reshape(-1)
    k = max(1, flat.size // 9)
    special = {"max": F32_SPECIAL, "average": F32_SPECIAL[[0, 1, 6, 7, 8, 9]], "average_inf": F32_SPECIAL[[2, 3, 6, 9]]}[kind]
    flat[g.integers(0, flat.size, k)] = special[g.integers(0, special.size, k)]
    return x


def int8_fixture(shape, seed):
    """Channels 0, 2 mod 4 within +-6 (sums land on exact ties), 1 mod 4 full range, 3 mod 4 far below the zero point (even a
    global maximum clamps under RELU)."""
    g = np.random.default_rng(seed)
    x = g.integers(-128, 128, shape).astype(np.int8)
    small = g.integers(-6, 7, shape).astype(np.int8)
    low = g.integers(-128, -99, shape).astype(np.int8)
    x[..., 0::2] = small[..., 0::2]
    x[..., 3::4] = low[..., 3::4]
    return x


def sums_and_counts(x, filt, stride, padding):
    """(int sums, tap counts) per output element."""
    taps, oh, ow = R.windows(x.shape, filt, stride, padding)
    a = np.zeros((x.shape[0], oh, ow, x.shape[3]), np.int64)
    n = np.zeros((1, oh, ow, 1), np.int64)
    for (oy, ox), (iy, ix) in taps:
        a[:, oy, ox, :] += x[:, iy, ix, :]
        n[:, oy, ox, :] += 1
    return a, np.broadcast_to(n, a.shape)


BATCHES = (1, 3)
F32_CHANNELS = dict(vector=(32, 64, 96), vector_no_bits=(4, 36), ragged=(1, 3, 33, 70))
I8_CHANNELS = dict(vector=(32, 64), vector_no_bits=(16, 48), ragged=(1, 17, 40))


def fixture_seed(image, batch, c):
    return image[0] * 10000 + image[1] * 1000 + batch * 100 + c


def grid_cases(channels):
    """(image, batch, channels) of the kernel grid on the GPU, for every window."""
    return [(image, batch, c) for image in GRID_IMAGES for batch in BATCHES for group in channels.values() for c in group]


@pytest.mark.parametrize("w", GRID_WINDOWS, ids=str)
def test_the_fixtures_are_what_the_checks_need(w):
    """Over the int8 tensors the GPU grid pools with this window: every even tap count they reach has an exact tie of each sign,
    and every activation clamps something.  Over the float ones: a window whose sequential and pairwise sums differ."""
    for image in GRID_IMAGES:
        filt, stride, padding = window_of(w, image)
        ties, clamped = {}, {(op, act): False for op in (R.MAX, R.AVERAGE) for act in ACTS[1:]}
        for im, batch, c in grid_cases(I8_CHANNELS):
            if im != image:
                continue
            x = int8_fixture((batch, *image, c), fixture_seed(image, batch, c))
            a, n = sums_and_counts(x, filt, stride, padding)
            for count in np.unique(n):
                if count % 2 == 0:
                    for sign in (1, -1):
                        hit = np.any((n == count) & (a * sign > 0) & (np.abs(a) % count == count // 2))
                        ties[(int(count), sign)] = ties.get((int(count), sign), False) or bool(hit)
            for op, act in clamped:
                free = R.pool2d(x, op, filt, stride, padding, NONE, *INT8_Q)
                clamped[(op, act)] |= bool(np.any(R.pool2d(x, op, filt, stride, padding, act, *INT8_Q) != free))
        assert all(ties.values()), (image, [k for k, v in ties.items() if not v])
        assert all(clamped.values()), (image, clamped)
        differ = False
        for im, batch, c in grid_cases(F32_CHANNELS):
            if im != image:
                continue
            shape = (batch, *image, c)
            x = float_fixture(shape, fixture_seed(image, batch, c), "average")
            assert np.isfinite(x).all() and (c < 33 or np.any((x != 0) & (np.abs(x) < 1e-38)))
            taps, oh, ow = R.windows(x.shape, filt, stride, padding)
            seq = np.zeros((batch, oh, ow, c), np.float32)
            vals = np.zeros((len(taps), batch, oh, ow, c), np.float32)
            for k, ((oy, ox), (iy, ix)) in enumerate(taps):
                seq[:, oy, ox, :] += x[:, iy, ix, :]
                vals[k][:, oy, ox, :] = x[:, iy, ix, :]
            pair = vals
            while pair.shape[0] > 1:                                         # a pairwise (tree) sum of the same taps
                if pair.shape[0] % 2:
                    pair = np.concatenate([pair, np.zeros_like(pair[:1])])
                pair = pair[0::2] + pair[1::2]
            differ = differ or bool(np.any(seq != pair[0]))
            if c >= 33:
                m = float_fixture(shape, fixture_seed(image, batch, c), "max")
                assert np.isnan(m).any() and np.isinf(m).any() and (m == 0).any() and np.any((m != 0) & (np.abs(m) < 1e-38))
                assert np.isinf(float_fixture(shape, fixture_seed(image, batch, c), "average_inf")).any()
        assert differ or len(taps) < 3, image


POOL_Q = (0.25, -3)                    # the ONE scale and zero point of the int8 body's tensors


def int8_body_model(H=15, C=64, seed=0):
    """x (int8) -> LceQuantize -> LceBconv2d (int8) -> MAX_POOL 3x3 / 2 VALID -> LceQuantize -> LceBconv2d (int8) -> AVERAGE_POOL
    2x2 / 2 SAME (RELU) -> the graph output.  The first pool feeds ONLY an LceQuantize; the second is delivered."""
    b = ModelBuilder()
    i8 = lambda shape, name: b.tensor(shape, np.int8, name, scale=POOL_Q[0], zero_point=POOL_Q[1])
    x = b.tensor([1, H, H, C], np.int8, "x", scale=0.5, zero_point=4)
    q0 = b.tensor([1, H, H, C // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y0, c0 = _conv(b, q0, H, C, C, seed * 10 + 5, out_type=np.int8, quant=POOL_Q)
    h1 = (H - 3) // 2 + 1
    p0 = i8([1, h1, h1, C], "p0")
    pool0 = pool_op(b, MAX_POOL_2D, [y0], [p0], (3, 3), (2, 2), VALID)
    q1 = b.tensor([1, h1, h1, C // 32], np.int32, "q1")
    b.custom_op("LceQuantize", [p0], [q1], b"")
    y1, c1 = _conv(b, q1, h1, C, C, seed * 10 + 6, out_type=np.int8, quant=POOL_Q)
    h2 = (h1 + 1) // 2
    p1 = i8([1, h2, h2, C], "p1")
    pool1 = pool_op(b, AVERAGE_POOL_2D, [y1], [p1], (2, 2), (2, 2), SAME, RELU)
    b.inputs, b.outputs = [x], [p1]
    info = dict(convs=[c0, c1], pools=[pool0, pool1], pooled=[p0, p1], sizes=[H, h1, h2], channels=C)
    return b.finish(), x, p1, info


def test_the_alexnet_body_is_one_section_with_both_flags():
    data, x, out, info = alexnet_body_model()
    model = mr.LceModel(data, elementwise_sections=True, pool_sections=True)
    n_ops = len(model.operators)
    assert [s.ops for s in model.sections] == [list(range(n_ops))]
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only
    assert mr.Interpreter(data, elementwise_sections=True, pool_sections=True).lce_only
    assert [model.operators[k].builtin_code for k in info["pools"]] == [MAX_POOL_2D, AVERAGE_POOL_2D]
    # without the pool flag: cut at each pool -- and the batch norm behind the first becomes ready in the host's epoch
    ew = mr.LceModel(data, elementwise_sections=True)
    assert [s.ops for s in ew.sections] == cut_at(n_ops, info["pools"] + [info["mul"], info["add"]])
    assert not mr.Interpreter(ew).lce_only
    # the pool flag alone: the MUL / ADD still cut; the flags of both words combine with the rest
    only = mr.LceModel(data, pool_sections=True)
    assert [s.ops for s in only.sections] == cut_at(n_ops, [info["mul"], info["add"]])
    assert [s.ops for s in mr.LceModel(data).sections] == cut_at(n_ops, info["pools"] + [info["mul"], info["add"]])
    every = mr.LceModel(data, elementwise_sections=True, int8_add_sections=True, concat_sections=True, pool_sections=True)
    assert [s.ops for s in every.sections] == [list(range(n_ops))]


def test_the_int8_body_is_one_section():
    data, x, out, info = int8_body_model()
    model = mr.LceModel(data, pool_sections=True)
    n_ops = len(model.operators)
    assert [s.ops for s in model.sections] == [list(range(n_ops))]
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only
    for kw in ({}, dict(elementwise_sections=True, int8_add_sections=True, concat_sections=True)):
        assert [s.ops for s in mr.LceModel(data, **kw).sections] == cut_at(n_ops, info["pools"])
    readers = lambda t: [i for i, op in enumerate(model.operators) if t in op.inputs]
    assert [len(readers(t)) for t in info["pooled"]] == [1, 0]
    assert model.operators[readers(info["pooled"][0])[0]].custom_code == "LceQuantize"


def test_the_dense_fixture_and_the_mixed_graph_keep_their_partitions():
    """Files without a qualifying pool: the flag changes nothing (the mixed graph's MAX_POOL_2D has no options table)."""
    for data in (dense_block_model()[0], mixed_model()[0]):
        for kw in ({}, dict(elementwise_sections=True), dict(elementwise_sections=True, concat_sections=True)):
            a, b = mr.LceModel(data, **kw), mr.LceModel(data, pool_sections=True, **kw)
            assert [(s.ops, s.inputs, s.outputs) for s in a.sections] == [(s.ops, s.inputs, s.outputs) for s in b.sections]


def _graph(case):
    """x -> LceQuantize -> LceBconv2d -> y -> <pool under test> -> z -> LceQuantize -> q2, with one condition of the candidate
    rule broken per case.  Returns (file, index of the pool)."""
    Hh, Cc = 8, 64
    int8 = case.startswith("int8")
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i8 = lambda shape, name, scale=0.5, zp=1: b.tensor(shape, np.int8, name, scale=scale, zero_point=zp)
    act = i8 if int8 else f32
    x = act([1, Hh, Hh, Cc], "x")
    y = act([1, Hh, Hh, Cc], "y")
    conv = lambda src, dst: b.custom_op("LceBconv2d", [src, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m),
                                                        f32([Cc], "b", bias), -1], [dst], bconv_options(spec))
    if case in ("stem", "constant"):
        # the pool reads the graph input (ready from the start: a stem operator) or a constant tensor
        src = x if case == "stem" else f32([1, Hh * 2, Hh * 2, Cc], "c", np.ones((1, Hh * 2, Hh * 2, Cc), np.float32))
        shape = [1, Hh // 2, Hh // 2, Cc] if case == "stem" else [1, Hh, Hh, Cc]
        z = f32(shape, "z")
        k = pool_op(b, MAX_POOL_2D, [src], [z])
        q = b.tensor(shape[:3] + [2], np.int32, "q")
        b.custom_op("LceQuantize", [z], [q], b"")
        spec2 = O.ConvSpec(1, shape[1], shape[1], Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
        y2 = f32(shape, "y2")
        b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y2],
                    bconv_options(spec2))
        b.inputs, b.outputs = [x], [y2]
        return b.finish(), k
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    conv(q, y)
    code, kw, zshape, ztype, src = MAX_POOL_2D, {}, [1, Hh // 2, Hh // 2, Cc], act, [y]
    if case == "wrong_type":
        ztype = i8
    elif case == "int8_scales":
        ztype = lambda shape, name: i8(shape, name, scale=0.25)
    elif case == "int8_zero_points":
        ztype = lambda shape, name: i8(shape, name, zp=2)
    elif case == "int8_unquantized":
        ztype = lambda shape, name: b.tensor(shape, np.int8, name)
    elif case == "channels":
        zshape = [1, Hh // 2, Hh // 2, Cc // 2]
    elif case == "extent_off_by_one":
        zshape = [1, Hh // 2 + 1, Hh // 2, Cc]
    elif case == "zero_stride":
        kw = dict(stride=(0, 2))
    elif case == "huge_stride":
        kw, zshape = dict(stride=(2 ** 31 - 1, 2 ** 31 - 1), padding=SAME), [1, 1, 1, Cc]
    elif case == "zero_filter":
        kw = dict(filt=(2, 0))
    elif case == "tanh":
        kw = dict(activation=TANH)
    elif case == "padding_2":
        kw = dict(padding=2)
    elif case == "no_options":
        kw = dict(options=False)
    elif case == "two_inputs":
        src = [y, y]
    elif case == "l2_pool":
        code = 11                                                     # L2_POOL_2D shares Pool2DOptions
    elif case == "three_d":
        # 3-D tensors around the pool (the convolution's output declared 3-D in the file)
        y = f32([Hh, Hh, Cc], "y3")
        b.ops.pop()
        conv(q, y)
        src, zshape = [y], [Hh // 2, Hh // 2, Cc]
    else:
        assert case in ("joins", "int8_joins", "average", "same_odd"), case
        if case == "average":
            code, kw = AVERAGE_POOL_2D, dict(activation=RELU6)
        if case == "same_odd":
            kw, zshape = dict(filt=(3, 3), stride=(3, 3), padding=SAME), [1, 3, 3, Cc]
    z = ztype(zshape, "z")
    k = pool_op(b, code, src, [z], **kw)
    q2 = b.tensor(zshape[:-1] + [(zshape[-1] + 31) // 32], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = [x], [q2]
    return b.finish(), k


@pytest.mark.parametrize("case", ["wrong_type", "int8_scales", "int8_zero_points", "int8_unquantized", "channels", "extent_off_by_one",
                                  "zero_stride", "huge_stride", "zero_filter", "tanh", "padding_2", "no_options", "two_inputs", "l2_pool", "constant",
                                  "stem", "three_d"])
def test_pools_that_stay_with_the_host(case):
    data, k = _graph(case)
    model = mr.LceModel(data, elementwise_sections=True, int8_add_sections=True, concat_sections=True, pool_sections=True)
    assert all(k not in s.ops for s in model.sections), (case, [s.ops for s in model.sections])
    assert not mr.Interpreter(model).lce_only
    assert [(s.ops, s.inputs, s.outputs) for s in model.sections] == [(s.ops, s.inputs, s.outputs) for s in mr.LceModel(data).sections]


@pytest.mark.parametrize("case", ["joins", "int8_joins", "average", "same_odd"])
def test_a_qualifying_pool_joins(case):
    data, k = _graph(case)
    model = mr.LceModel(data, pool_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and k == 2
    assert mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]
    assert [s.ops for s in mr.LceModel(data, elementwise_sections=True, int8_add_sections=True, concat_sections=True).sections] == [[0, 1], [3]]


# ---- the reader ---------------------------------------------------------------------------------------------------------------
def _options_model(rows):
    """One pool per row (code, padding, stride_w, stride_h, filter_width, filter_height, activation), or (code, None) for a pool
    without an options table, each followed by an ADD."""
    b = ModelBuilder()
    f32 = lambda shape, name: b.tensor(shape, np.float32, name)
    x = f32([1, 4, 4, 4], "x")
    prev = x
    for n, row in enumerate(rows):
        out = f32([1, 2, 2, 4], "t%d" % n)
        if row[1] is None:
            pool_op(b, row[0], [prev], [out], options=False)
        else:
            code, pad, sw, sh, fw, fh, act = row
            pool_op(b, code, [prev], [out], (fh, fw), (sh, sw), pad, act)
        prev = f32([1, 4, 4, 4], "u%d" % n)
        ew_op(b, ADD, [out, out], [prev], RELU)
    b.inputs, b.outputs = [x], [prev]
    return b.finish()


def test_pool2d_options_round_trip_through_the_reader():
    rows = [(MAX_POOL_2D, VALID, 2, 3, 4, 5, RELU6), (AVERAGE_POOL_2D, SAME, 1, 1, 2, 2, NONE), (MAX_POOL_2D, None),
            (AVERAGE_POOL_2D, 1, 2 ** 31 - 1, -7, 0, -2 ** 31, 5), (MAX_POOL_2D, -1, 9, 8, 7, 6, RELU_N1_TO_1)]
    model = mr.LceModel(_options_model(rows))
    pools, others = model.operators[0::2], model.operators[1::2]
    for op, row in zip(pools, rows):
        assert op.builtin_code == row[0]
        got = (op.padding, op.stride_w, op.stride_h, op.filter_width, op.filter_height, op.activation)
        assert got == ((0,) * 6 if row[1] is None else row[1:]), row
    for op in others:                                                                  # every other operator: 0
        assert (op.padding, op.stride_w, op.stride_h, op.filter_width, op.filter_height) == (0,) * 5 and op.activation == RELU
    v = (C.c_int32 * 5)()
    assert mr.tflite_lib().lce_tflite_model_operator_pool2d(model._h, len(model.operators), v) == amd.ERR_INVALID
    assert mr.tflite_lib().lce_tflite_model_operator_pool2d(model._h, 0, None) == amd.ERR_INVALID


def test_a_truncated_or_out_of_bounds_options_table_is_refused_at_open():
    data = bytearray(_options_model([(MAX_POOL_2D, VALID, 2, 2, 2, MARK, NONE)]))
    assert mr.LceModel(bytes(data)).operators[0].filter_height == MARK
    table, ref, slot = _options_table(data)
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
    for d in bad:
        for kw in ({}, dict(pool_sections=True)):
            with pytest.raises(ValueError, match="Pool2DOptions"):
                mr.LceModel(d, **kw)


# ---- shape inference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
def test_section_tensor_shape_over_the_pooled_tensors(batch):
    data, x, out, info = alexnet_body_model()
    model = mr.LceModel(data, elementwise_sections=True, pool_sections=True)
    c = info["channels"]
    assert info["sizes"] == [15, 7, 4]
    for t, h in zip(info["pooled"], info["sizes"][1:]):
        assert model.section_tensor_shape(0, t, batch) == ((batch, h, h, c), batch * h * h * c * 4)
    assert model.section_tensor_shape(0, out, batch) == ((batch, 4, 4, c), batch * 4 * 4 * c * 4)
    data, x, out, info = int8_body_model()
    model = mr.LceModel(data, pool_sections=True)
    for t, h in zip(info["pooled"], info["sizes"][1:]):
        assert model.section_tensor_shape(0, t, batch) == ((batch, h, h, c), batch * h * h * c)


@pytest.mark.parametrize("declared", [32, 96])
def test_a_file_whose_pool_input_disagrees_with_the_inferred_shape_is_refused(declared):
    """The pool's tensors agree with each other in the file, but the convolution produces 64 channels where the file declares
    `declared` for its output: the walk must fail instead of reading past (or short of) the convolution's buffer."""
    Hh, Cc = 8, 64
    spec = O.ConvSpec(1, Hh, Hh, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x, y, z = f32([1, Hh, Hh, Cc], "x"), f32([1, Hh, Hh, declared], "y"), f32([1, Hh // 2, Hh // 2, declared], "z")
    q = b.tensor([1, Hh, Hh, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                bconv_options(spec))
    pool_op(b, MAX_POOL_2D, [y], [z])
    b.inputs, b.outputs = [x], [z]
    model = mr.LceModel(b.finish(), pool_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2]]
    with pytest.raises(amd.LceHipError, match="pool input") as e:
        model.section_tensor_shape(0, z, 2)
    assert e.value.code == amd.ERR_INVALID


# ---- lce_hip_pool2d / amd.pool2d argument checks (no device needed: they come first) -------------------------------------------
def _desc(**kw):
    d = dict(op=amd.POOL_MAX, type=amd.F32, batch=2, in_height=8, in_width=8, channels=64, filter_height=2, filter_width=2,
             stride_height=2, stride_width=2, padding=amd.PADDING_VALID, activation=amd.ACT_NONE, scale=1.0, zero_point=0)
    d.update(kw)
    return amd.Pool2dDesc(*[d[n] for n, _ in amd.Pool2dDesc._fields_])


def _c_call(desc=True, inp=4096, out=1 << 20, bits=1 << 21, **kw):
    d = _desc(**kw)
    return amd.lib().lce_hip_pool2d(C.byref(d) if desc else None, C.c_void_p(inp), C.c_void_p(out), C.c_void_p(bits), None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(desc=False), amd.ERR_INVALID, "null desc"),
    (dict(inp=0), amd.ERR_INVALID, "null input"),
    (dict(out=0, bits=0), amd.ERR_INVALID, "both outputs"),
    (dict(batch=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_height=-1), amd.ERR_INVALID, "extents must be positive"),
    (dict(in_width=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(channels=0), amd.ERR_INVALID, "extents must be positive"),
    (dict(filter_height=0), amd.ERR_INVALID, "filter must be positive"),
    (dict(filter_width=-2), amd.ERR_INVALID, "filter must be positive"),
    (dict(stride_height=0), amd.ERR_INVALID, "stride must be positive"),
    (dict(stride_width=-1), amd.ERR_INVALID, "stride must be positive"),
    (dict(op=2), amd.ERR_INVALID, "unknown op"),
    (dict(op=-1), amd.ERR_INVALID, "unknown op"),
    (dict(type=amd.BITPACKED), amd.ERR_INVALID, "type must be"),
    (dict(type=amd.BOOL), amd.ERR_INVALID, "type must be"),
    (dict(padding=2), amd.ERR_INVALID, "padding must be"),
    (dict(activation=4), amd.ERR_INVALID, "unknown activation"),
    (dict(activation=-1), amd.ERR_INVALID, "unknown activation"),
    (dict(type=amd.I8, zero_point=128), amd.ERR_INVALID, "zero_point"),
    (dict(type=amd.I8, zero_point=-129), amd.ERR_INVALID, "zero_point"),
    (dict(type=amd.I8, scale=0.0), amd.ERR_INVALID, "scale must be"),
    (dict(type=amd.I8, scale=-1.0), amd.ERR_INVALID, "scale must be"),
    (dict(type=amd.I8, scale=float("inf")), amd.ERR_INVALID, "scale must be"),
    (dict(type=amd.I8, scale=float("nan")), amd.ERR_INVALID, "scale must be"),
    (dict(filter_height=9), amd.ERR_INVALID, "empty output"),
    (dict(filter_width=9, filter_height=1), amd.ERR_INVALID, "empty output"),
    (dict(filter_height=257, filter_width=256, padding=amd.PADDING_SAME), amd.ERR_UNSUPPORTED, "more than 65536 taps"),
    (dict(filter_height=65537, filter_width=1, padding=amd.PADDING_SAME), amd.ERR_UNSUPPORTED, "more than 65536 taps"),
    (dict(batch=2 ** 20, in_height=2 ** 6, in_width=2 ** 6, channels=1, filter_height=1, filter_width=1, stride_height=1,
          stride_width=1, inp=1 << 40, out=1 << 50, bits=1 << 60), amd.ERR_UNSUPPORTED, "2\\^31 pixels"),
    (dict(stride_height=2 ** 31 - 1, stride_width=2 ** 31 - 1, padding=amd.PADDING_SAME), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(stride_width=2 ** 30 + 1, padding=amd.PADDING_SAME), amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(batch=1, channels=1, in_height=2 ** 30 + 1, in_width=1, filter_width=1, stride_width=1, inp=1 << 40, out=1 << 50, bits=1 << 60),
     amd.ERR_UNSUPPORTED, "above 2\\^30"),
    (dict(out=4096 + 512), amd.ERR_INVALID, "overlaps the input"),                    # the input is 2 x 8 x 8 x 64 floats = 32 KiB
    (dict(out=4096 - 16), amd.ERR_INVALID, "overlaps the input"),
    (dict(out=0, bits=4096 + 32768 - 4), amd.ERR_INVALID, "overlaps the input"),
    (dict(bits=(1 << 20) + 8188), amd.ERR_INVALID, "outputs overlap"),                 # the pooled tensor is 8 KiB
    (dict(bits=(1 << 21) + 2), amd.ERR_INVALID, "4-byte aligned"),
])
def test_c_entry_refuses_bad_arguments(kw, code, msg):
    assert _c_call(**kw) == code
    assert re.search(msg, amd.lib().lce_hip_last_error().decode()), amd.lib().lce_hip_last_error()


def test_c_entry_accepts_the_edges_of_the_checks_up_to_the_device():
    """Touching ranges do not overlap; the largest filter, the extreme zero points and a 1 x 1 output pass.  Without a device
    the accepted calls end at ERR_NO_DEVICE; none of them is ERR_INVALID or ERR_UNSUPPORTED."""
    edges = (dict(out=4096 + 32768), dict(out=4096 - 8192), dict(bits=(1 << 20) + 8192), dict(out=0), dict(bits=0),
             dict(filter_height=256, filter_width=256, padding=amd.PADDING_SAME), dict(filter_height=65536, filter_width=1, padding=amd.PADDING_SAME),
             dict(filter_height=8, filter_width=8), dict(stride_height=2 ** 30, stride_width=2 ** 30, padding=amd.PADDING_SAME),
             dict(type=amd.I8, zero_point=-128, scale=1e-30), dict(type=amd.I8, zero_point=127),
             dict(op=amd.POOL_AVERAGE, activation=amd.ACT_RELU6, padding=amd.PADDING_SAME, stride_height=9, stride_width=1))
    oh, ow = C.c_int32(), C.c_int32()
    for kw in edges:
        ptrs = {k: kw[k] for k in ("out", "bits") if k in kw}
        d = _desc(**{k: v for k, v in kw.items() if k not in ptrs})
        assert amd.lib().lce_hip_pool2d_check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK, kw
        if amd.device_count() == 0:
            assert _c_call(**kw) == amd.ERR_NO_DEVICE, kw
    d = _desc(filter_height=3, filter_width=3, in_height=7, in_width=9, padding=amd.PADDING_SAME)
    assert amd.lib().lce_hip_pool2d_check(C.byref(d), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (4, 5)
    assert amd.lib().lce_hip_pool2d_check(C.byref(d), None, None) == amd.OK
    assert amd.lib().lce_hip_pool2d_check(None, None, None) == amd.ERR_INVALID


X = np.zeros((2, 8, 8, 64), np.float32)
XI = X.astype(np.int8)


@pytest.mark.parametrize("x,kw,msg", [
    (X, dict(op=2), "unknown op"),
    (X, dict(op="l2"), "unknown op"),
    (X.astype(np.float64), {}, "float32 or int8"),
    (X[0], {}, "NHWC"),
    (np.zeros((2, 0, 8, 64), np.float32), {}, "non-empty"),
    (X, dict(filter=0), "filter must be"),
    (X, dict(filter=(2, 2, 2)), "filter must be"),
    (X, dict(filter=2.0), "filter must be"),
    (X, dict(stride=(1, -1)), "stride must be"),
    (X, dict(filter=(257, 256), padding=amd.PADDING_SAME), "more than 65536 taps"),
    (X, dict(padding=2), "padding must be"),
    (X, dict(activation=4), "unknown activation"),
    (X, dict(filter=9), "empty output"),
    (X, dict(zero_point=3), "no zero point"),
    (XI, {}, "scale"),
    (XI, dict(scale=0.0), "scale"),
    (XI, dict(scale=float("nan")), "scale"),
    (XI, dict(scale=0.5, zero_point=128), "zero point"),
    (XI, dict(scale=0.5, zero_point=1.5), "zero point"),
    (X, dict(out=False), "no output"),
    (X, dict(out=np.zeros((2, 4, 4, 63), np.float32)), "out must be"),
    (X, dict(out=np.zeros((2, 4, 4, 64), np.int8)), "out must be"),
    (X, dict(out_bits=np.zeros((2, 4, 4, 3), np.int32)), "out_bits must be"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, x, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    args = dict(op=amd.POOL_MAX, filter=2, stride=2, padding=amd.PADDING_VALID)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        amd.pool2d(x, **args)


def test_open_opts_is_versioned_by_its_size():
    lib = mr.tflite_lib()
    assert C.sizeof(mr._OpenOptions) == 8 and C.sizeof(mr._OpenOptionsExt) == 24
    pack = lambda size, sections, ext=0, reserved=(0, 0, 0): struct.pack("<6I", size, sections, ext, *reserved)
    for data in (alexnet_body_model()[0], int8_body_model()[0], mixed_model()[0]):
        for sections in range(8):
            h8, _ = _open(data, pack(8, sections)[:8])                   # the first form: nothing beyond 8 bytes exists
            h24, _ = _open(data, pack(24, sections, 0))
            assert h8 and h24 and _sections_of(h8) == _sections_of(h24), sections
            hp, _ = _open(data, pack(24, sections, 1))
            assert hp
            with_pool = mr.LceModel(data, elementwise_sections=bool(sections & 1), int8_add_sections=bool(sections & 2),
                                    concat_sections=bool(sections & 4), pool_sections=True)
            assert _sections_of(hp) == [(s.ops, s.inputs, s.outputs) for s in with_pool.sections]
            for h in (h8, h24, hp):
                lib.lce_tflite_model_close(h)
        # size 8 ignores nothing: the same 8 bytes followed by what would be the pool flag still open WITHOUT it
        h, _ = _open(data, pack(8, 1, 1))
        h8, _ = _open(data, pack(8, 1)[:8])
        assert h and _sections_of(h) == _sections_of(h8)
        lib.lce_tflite_model_close(h)
        lib.lce_tflite_model_close(h8)
        for ext in (2, 3, 1 << 31):
            h, err = _open(data, pack(24, 1, ext))
            assert not h and b"flags" in err
        for sections in (8, 16, 1 << 31):
            h, err = _open(data, pack(24, sections, 1))
            assert not h and b"flags" in err
        for k in range(3):
            reserved = [0, 0, 0]
            reserved[k] = 1
            h, err = _open(data, pack(24, 1, 1, reserved))
            assert not h and b"reserved" in err
        for size in (0, 4, 12, 16, 20, 28, 32):
            h, err = _open(data, (pack(size, 1, 1) + b"\0" * 8)[:max(size, 8)])
            assert not h and b"struct_size" in err, size
    body = alexnet_body_model()[0]
    one, cut = _open(body, pack(24, 1, 1))[0], _open(body, pack(8, 1)[:8])[0]
    assert len(_sections_of(one)) == 1 and len(_sections_of(cut)) > 1
    lib.lce_tflite_model_close(one)
    lib.lce_tflite_model_close(cut)


def test_open_ex_still_refuses_the_other_bits_and_the_abi_version_stays():
    data = alexnet_body_model()[0]
    err = C.create_string_buffer(128)
    for flags in (4, 5, 7, 8):
        assert not mr.tflite_lib().lce_tflite_model_open_ex(data, len(data), flags, err, 128)
        assert b"flags" in err.value
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_pool2d", "lce_hip_pool2d_check"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    for name in ("lce_tflite_model_pool_stats", "lce_tflite_model_operator_pool2d"):
        assert hasattr(mr.tflite_lib(), name)


def test_the_python_constructor_uses_the_24_byte_options_only_for_the_pool_flag(monkeypatch):
    data = alexnet_body_model()[0]
    lib = mr.tflite_lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name in ("lce_tflite_model_open_ex", "lce_tflite_model_open_opts"):
                def spy(*a):
                    calls.append((name, C.cast(a[2], C.POINTER(C.c_uint32))[0] if name.endswith("opts") else a[2]))
                    return getattr(lib, name)(*a)
                return spy
            return getattr(lib, name)
    monkeypatch.setattr(mr, "tflite_lib", lambda: Spy())
    mr.LceModel(data, elementwise_sections=True, int8_add_sections=True)
    mr.LceModel(data, concat_sections=True)
    mr.LceModel(data, pool_sections=True)
    mr.LceModel(data, concat_sections=True, pool_sections=True)
    assert calls == [("lce_tflite_model_open_ex", 3), ("lce_tflite_model_open_opts", 8), ("lce_tflite_model_open_opts", 24),
                     ("lce_tflite_model_open_opts", 24)]


def test_stats_are_zero_before_any_run():
    model = mr.LceModel(alexnet_body_model()[0], elementwise_sections=True, pool_sections=True)
    assert model.pool_stats() == (0, 0)


# ---- the build: no scratch memory, no LDS, no spills ------------------------------------------------------------------------------
def test_the_pool_kernels_use_no_scratch_and_no_lds():
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_pool.hip")
    assert sorted(k for k in kernels if "pool" in k) == sorted(k for k in kernels), kernels
    assert len(kernels) == 12, kernels                       # vector: 2 kinds x 2 ops x with / without bits; rows: 2 kinds x 2 ops
    assert len([k for k in kernels if "pool_vec" in k]) == 8 and len([k for k in kernels if "pool_rows" in k]) == 4
    for key in H.RESOURCE_KEYS:
        assert resources[key] == ["0"] * len(kernels), (key, resources[key])
    # the vector path moves 16 bytes per lane and instruction
    assert "global_load_dwordx4" in mnemonics and "global_store_dwordx4" in mnemonics
