"""Channel CONCATENATION between binary layers inside the sections (LCE_TFLITE_SECTIONS_CONCAT, include/lce_tflite_model.h) on
the CPU: the partition with and without the opt-in, every condition that keeps a join with the host, ConcatenationOptions
through the reader, shape inference over the joined tensors, the new entry lce_tflite_model_open_opts, and the argument checks
of lce_hip_concat / amd.concat, which all fail before any device is touched.  Also the fixtures of the GPU side
(tests/test_gpu_concat.py) and of tools/concat_sections.py."""
import ctypes as C
import importlib
import re
import struct

import numpy as np
import pytest

import hipcc_lib as H
import oracle_lib as O
from section_models import (ADD, CONCATENATION, DENSE_STAGES, MUL, NONE, RELU, _conv, _sections_of, bconv_options, concat_op,
                            cut_at, dense_block_model, ew_op, joins_of, mixed_model)
import synth
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")


INT8_GROWTHS = (64, 16, 17, 31)
INT8_Q = (0.25, -3)                     # the ONE scale and zero point of every int8 LceBconv2d output and join


def int8_dense_model(H=16, C0=64, growths=INT8_GROWTHS, seed=0):
    """x (int8) -> LceQuantize -> LceBconv2d (int8) -> y0, then per layer  x -> LceQuantize -> LceBconv2d (int8, G channels) -> y;
    CONCATENATION([x, y]) -> x'  -- every join feeds the next LceQuantize directly -- and after the last join
    LceQuantize -> LceBconv2d (int8) -> the graph output, so the last join feeds ONLY an LceQuantize.  All int8 tensors behind
    the input share INT8_Q.  Returns (file, input tensor, output tensor, steps) as dense_block_model does."""
    b = ModelBuilder()
    x0 = b.tensor([1, H, H, C0], np.int8, "x", scale=0.5, zero_point=4)
    steps = []
    n = [seed * 100 + 50]

    def binary_layer(src, c, cout):
        n[0] += 1
        q = b.tensor([1, H, H, (c + 31) // 32], np.int32, "q%d" % n[0])
        b.custom_op("LceQuantize", [src], [q], b"")
        return _conv(b, q, H, c, cout, n[0], out_type=np.int8, quant=INT8_Q)

    y, info = binary_layer(x0, C0, C0)
    steps.append(dict(kind="conv", zp=4, **info))
    x, c = y, C0
    for growth in growths:
        y, info = binary_layer(x, c, growth)
        out = b.tensor([1, H, H, c + growth], np.int8, "x%d" % n[0], scale=INT8_Q[0], zero_point=INT8_Q[1])
        join = concat_op(b, [x, y], [out])
        steps.append(dict(kind="dense", convs=[info], join=join, out=out, x=x))
        x, c = out, c + growth
    y, info = binary_layer(x, c, C0)
    steps.append(dict(kind="conv", zp=INT8_Q[1], **info))
    b.inputs, b.outputs = [x0], [y]
    return b.finish(), x0, y, steps


def bn(v, m, a):
    """The float32 batch norm of a dense layer as TFLite's MUL then ADD compute it: one rounding per operator."""
    return ((v * m).astype(np.float32) + a.reshape(1, 1, 1, -1)).astype(np.float32)


def dense_reference(steps, x):
    """The float fixture composed from the oracle's LceQuantize / LceBconv2d, the one-rounding batch norm and np.concatenate.
    Returns the tensor after every step."""
    batch, after = x.shape[0], []
    for s in steps:
        conv = lambda cv, bits: O.bconv2d(cv["spec"].with_batch(batch), O.DST_F32, bits, cv["w"], cv["m"], cv["b"])
        if s["kind"] == "conv":
            x = conv(s, O.bitpack(x))
        else:
            bits = O.bitpack(bn(x, s["bn_m"], s["bn_a"]))
            x = np.concatenate([x] + [conv(cv, bits) for cv in s["convs"]], axis=-1)
        after.append(x)
    return after


def int8_dense_reference(steps, x):
    """The int8 fixture from the oracle's int8 LceBconv2d, LceQuantize at the tensor's zero point, and np.concatenate."""
    batch, after, zp = x.shape[0], [], None
    conv = lambda cv, bits: O.bconv2d(cv["spec"].with_batch(batch), O.DST_I8, bits, cv["w"], cv["m"], cv["b"],
                                      out_scale=INT8_Q[0], out_zero_point=INT8_Q[1])
    for s in steps:
        if s["kind"] == "conv":
            x = conv(s, O.bitpack(x, s["zp"]))
        else:
            x = np.concatenate([x, conv(s["convs"][0], O.bitpack(x, INT8_Q[1]))], axis=-1)
        after.append(x)
    return after


# ---- the partition ------------------------------------------------------------------------------------------------------------
def test_the_fixtures_are_what_the_checks_need():
    data, x, out, steps = dense_block_model()
    dense = [s for s in steps if s["kind"] == "dense"]
    assert len(dense) >= 6 and steps[0]["kind"] == "conv"
    assert any(s["kind"] == "conv" and s["spec"].stride_h == 2 for s in steps[1:])
    assert len({s["convs"][0]["spec"].in_h for s in dense}) == 2
    assert any(cv["spec"].channels_out % 32 for s in dense for cv in s["convs"])
    model = mr.LceModel(data)
    assert any(len(model.operators[s["join"]].inputs) == 3 for s in dense)
    assert all(model.operators[j].builtin_code == CONCATENATION for j in joins_of(steps))


def test_the_float_dense_block_is_one_section_with_both_flags():
    data, x, out, steps = dense_block_model()
    model = mr.LceModel(data, elementwise_sections=True, concat_sections=True)
    n_ops = len(model.operators)
    assert [s.ops for s in model.sections] == [list(range(n_ops))]
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only
    assert mr.Interpreter(data, elementwise_sections=True, concat_sections=True).lce_only
    # the float flag alone: cut at every join, as before the new opt-in existed -- and a batch norm that reads a joined
    # tensor becomes ready in the host's epoch, so it is the host's too (a stage's first follows an LCE operator)
    ew = mr.LceModel(data, elementwise_sections=True)
    hosts = joins_of(steps) + [i for k, s in enumerate(steps) if s["kind"] == "dense" and steps[k - 1]["kind"] == "dense"
                               for i in (s["mul"], s["add"])]
    assert [s.ops for s in ew.sections] == cut_at(n_ops, hosts)
    assert all(j not in s.ops for j in joins_of(steps) for s in ew.sections) and not mr.Interpreter(ew).lce_only
    h = mr.tflite_lib().lce_tflite_model_open_ex(data, len(data), mr.SECTIONS_ELEMENTWISE, None, 0)
    assert _sections_of(h) == [(s.ops, s.inputs, s.outputs) for s in ew.sections]
    mr.tflite_lib().lce_tflite_model_close(h)
    # the new flag alone: the MUL / ADD still cut
    only = mr.LceModel(data, concat_sections=True)
    foreign = [i for i, op in enumerate(only.operators) if op.builtin_code in (ADD, MUL)]
    assert [s.ops for s in only.sections] == cut_at(n_ops, foreign)
    assert not mr.Interpreter(only).lce_only
    # no flag: cut at every builtin operator
    assert [s.ops for s in mr.LceModel(data).sections] == cut_at(n_ops, foreign + joins_of(steps))


def test_the_int8_dense_block_is_one_section():
    data, x, out, steps = int8_dense_model()
    model = mr.LceModel(data, int8_add_sections=True, concat_sections=True)
    n_ops = len(model.operators)
    assert [s.ops for s in model.sections] == [list(range(n_ops))]
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data, concat_sections=True).sections] == [list(range(n_ops))]
    assert [s.ops for s in mr.LceModel(data, int8_add_sections=True).sections] == cut_at(n_ops, joins_of(steps))
    assert [s.ops for s in mr.LceModel(data).sections] == cut_at(n_ops, joins_of(steps))
    # the last join feeds only an LceQuantize; the others an LceQuantize and the next join
    readers = lambda t: [i for i, op in enumerate(model.operators) if t in op.inputs]
    dense = [s for s in steps if s["kind"] == "dense"]
    assert [len(readers(s["out"])) for s in dense] == [2] * (len(dense) - 1) + [1]
    assert model.operators[readers(dense[-1]["out"])[0]].custom_code == "LceQuantize"


def _graph(case):
    """x -> LceQuantize -> LceBconv2d -> y -> CONCATENATION([y, other]) -> z -> LceQuantize -> q2, with one condition of the
    candidate rule broken per case.  Returns (file, index of the join)."""
    H, Cc = 8, 64
    int8 = case.startswith("int8")
    spec = O.ConvSpec(1, H, H, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i8 = lambda shape, name, scale=0.5, zp=1: b.tensor(shape, np.int8, name, scale=scale, zero_point=zp)
    act = i8 if int8 else f32
    x = act([1, H, H, Cc], "x")
    inputs = [x]
    q = b.tensor([1, H, H, 2], np.int32, "q")
    y = act([1, H, H, Cc], "y")
    conv = lambda src: b.custom_op("LceBconv2d", [src, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1],
                                   [y], bconv_options(spec))
    if case == "outside":
        # CONCATENATION(x, x2): both operands come from outside; it is ready from the start and is a stem operator
        x2 = f32([1, H, H, Cc], "x2")
        z = f32([1, H, H, 2 * Cc], "z")
        k = concat_op(b, [x, x2], [z])
        q4 = b.tensor([1, H, H, 4], np.int32, "q4")
        b.custom_op("LceQuantize", [z], [q4], b"")
        spec2 = O.ConvSpec(1, H, H, 2 * Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
        _, w2, m2, b2 = synth.conv_inputs(spec2, 6)
        b.custom_op("LceBconv2d", [q4, b.tensor(w2.shape, np.int32, "w", w2), f32([Cc], "m", m2), f32([Cc], "b", b2), -1], [y],
                    bconv_options(spec2))
        b.inputs, b.outputs = [x, x2], [y]
        return b.finish(), k
    b.custom_op("LceQuantize", [x], [q], b"")
    conv(q)
    others, zc, axis, activation = [x], 2 * Cc, 3, NONE
    if case == "axis1":
        axis = 1
    elif case == "axis0":
        axis = 0
    elif case == "minus1":
        axis = -1
    elif case == "relu":
        activation = RELU
    elif case == "constant":
        others = [f32([1, H, H, Cc], "c", np.ones((1, H, H, Cc), np.float32))]
    elif case == "nine":
        others, zc = [x] * 8, 9 * Cc
    elif case == "h_mismatch":
        others = [f32([1, H // 2, H, Cc], "x2")]
        inputs.append(others[0])
    elif case == "sum":
        zc = 2 * Cc - 28
    elif case == "mixed":
        others = [i8([1, H, H, Cc], "x2")]
        inputs.append(others[0])
    elif case == "int8_scales":
        others = [i8([1, H, H, Cc], "x2", scale=0.25)]
        inputs.append(others[0])
    elif case == "int8_zero_points":
        others = [i8([1, H, H, Cc], "x2", zp=2)]
        inputs.append(others[0])
    elif case == "int8_no_quantization":
        others = [b.tensor([1, H, H, Cc], np.int8, "x2")]
        inputs.append(others[0])
    else:
        assert case in ("joins", "int8_joins"), case
    z = act([1, H, H, zc], "z")
    k = concat_op(b, [y] + others, [z], axis, activation)
    q2 = b.tensor([1, H, H, (zc + 31) // 32], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = inputs, [q2]
    return b.finish(), k


@pytest.mark.parametrize("case", ["axis1", "axis0", "relu", "constant", "nine", "h_mismatch", "sum", "mixed", "int8_scales",
                                  "int8_zero_points", "int8_no_quantization", "outside"])
def test_joins_that_stay_with_the_host(case):
    data, k = _graph(case)
    model = mr.LceModel(data, elementwise_sections=True, int8_add_sections=True, concat_sections=True)
    assert all(k not in s.ops for s in model.sections), (case, [s.ops for s in model.sections])
    assert not mr.Interpreter(model).lce_only
    assert [(s.ops, s.inputs, s.outputs) for s in model.sections] == [(s.ops, s.inputs, s.outputs) for s in mr.LceModel(data).sections]


@pytest.mark.parametrize("case", ["joins", "minus1", "int8_joins"])
def test_a_qualifying_join_joins(case):
    data, k = _graph(case)
    model = mr.LceModel(data, concat_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and k == 2
    assert mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]
    assert [s.ops for s in mr.LceModel(data, elementwise_sections=True, int8_add_sections=True).sections] == [[0, 1], [3]]


# ---- the reader ---------------------------------------------------------------------------------------------------------------
def _axis_model(axes):
    b = ModelBuilder()
    f32 = lambda shape, name: b.tensor(shape, np.float32, name)
    x = f32([1, 2, 2, 4], "x")
    prev = x
    for n, axis in enumerate(axes):
        out = f32([1, 2, 2, 8], "t%d" % n)
        concat_op(b, [prev, prev], [out], axis, n % 4)
        prev = f32([1, 2, 2, 4], "u%d" % n)
        ew_op(b, ADD, [out, out], [prev], RELU)
    b.inputs, b.outputs = [x], [prev]
    return b.finish()


def test_axis_and_activation_round_trip_through_the_reader():
    axes = (3, -1, 0, None, 1, -4, 2 ** 31 - 1)
    model = mr.LceModel(_axis_model(axes))
    joins = model.operators[0::2]
    assert [op.axis for op in joins] == [0 if a is None else a for a in axes]
    assert [op.activation for op in joins] == [0 if a is None else n % 4 for n, a in enumerate(axes)]
    assert [op.axis for op in model.operators[1::2]] == [0] * len(axes)                 # every other operator: 0
    assert [op.activation for op in model.operators[1::2]] == [RELU] * len(axes)
    axis = C.c_int32()
    assert mr.tflite_lib().lce_tflite_model_operator_axis(model._h, len(model.operators), C.byref(axis)) == amd.ERR_INVALID
    assert mr.tflite_lib().lce_tflite_model_operator_axis(model._h, 0, None) == amd.ERR_INVALID


MARK = 0x5A6B7C4D


def _options_table(data):
    """(position of the ConcatenationOptions table whose axis is MARK, position of the uoffset that points to it)."""
    at = data.index(struct.pack("<i", MARK))
    assert data.count(struct.pack("<i", MARK)) == 1
    table = at - 4
    refs = [p for p in range(0, table, 4) if p + struct.unpack_from("<I", data, p)[0] == table]
    assert len(refs) == 1
    return table, refs[0]


def test_a_truncated_or_out_of_bounds_options_table_is_refused_at_open():
    data = bytearray(_axis_model((MARK,)))
    assert mr.LceModel(bytes(data)).operators[0].axis == MARK
    table, ref = _options_table(data)
    bad = []
    for target in (len(data) - 2, len(data), len(data) + 4096, 2 ** 32 - 8 - ref):   # cut short by the end of the file; beyond it
        d = bytearray(data)
        struct.pack_into("<I", d, ref, (target - ref) % 2 ** 32)
        bad.append(bytes(d))
    for soffset in (table + 8, -(len(data) + 64), 2 ** 31 - 1):                        # the table's vtable lies outside the file
        d = bytearray(data)
        struct.pack_into("<i", d, table, soffset)
        bad.append(bytes(d))
    d = bytearray(data)
    vtable = table - struct.unpack_from("<i", data, table)[0]
    struct.pack_into("<H", d, vtable + 4, 0xFFF0)                                      # field 0 (axis) far outside the file
    bad.append(bytes(d))
    for d in bad:
        for kw in ({}, dict(concat_sections=True)):
            with pytest.raises(ValueError, match="ConcatenationOptions"):
                mr.LceModel(d, **kw)


# ---- shape inference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
def test_section_tensor_shape_over_the_joined_tensors(batch):
    data, x, out, steps = dense_block_model()
    model = mr.LceModel(data, elementwise_sections=True, concat_sections=True)
    h, c = 16, 64
    for s in steps:
        if s["kind"] == "conv":
            h, c = s["spec"].out_h, s["spec"].channels_out
            continue
        for cv in s["convs"]:
            g = cv["spec"].channels_out
            assert model.section_tensor_shape(0, cv["y"], batch) == ((batch, h, h, g), batch * h * h * g * 4)
        c += sum(cv["spec"].channels_out for cv in s["convs"])
        assert model.section_tensor_shape(0, s["out"], batch) == ((batch, h, h, c), batch * h * h * c * 4), s["join"]
    assert (h, c) == (8, 288)
    data, x, out, steps = int8_dense_model()
    model = mr.LceModel(data, concat_sections=True)
    c = 64
    for s in steps:
        if s["kind"] == "dense":
            c += s["convs"][0]["spec"].channels_out
            assert model.section_tensor_shape(0, s["out"], batch) == ((batch, 16, 16, c), batch * 16 * 16 * c), s["join"]
    assert c == 64 + sum(INT8_GROWTHS)


@pytest.mark.parametrize("declared", [32, 96])
def test_a_file_whose_join_inputs_disagree_with_the_inferred_shapes_is_refused(declared):
    """The join's tensors agree with each other in the file, but the convolution produces 64 channels where the file declares
    `declared` for its output: the walk must fail instead of reading past (or short of) the convolution's buffer."""
    H, Cc = 8, 64
    spec = O.ConvSpec(1, H, H, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x, y, z = f32([1, H, H, Cc], "x"), f32([1, H, H, declared], "y"), f32([1, H, H, Cc + declared], "z")
    q = b.tensor([1, H, H, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                bconv_options(spec))
    concat_op(b, [x, y], [z])
    b.inputs, b.outputs = [x], [z]
    model = mr.LceModel(b.finish(), concat_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2]]
    with pytest.raises(amd.LceHipError, match="CONCATENATION input") as e:
        model.section_tensor_shape(0, z, 2)
    assert e.value.code == amd.ERR_INVALID


# ---- lce_hip_concat / amd.concat argument checks (no device needed: they come first) -------------------------------------------
def _c_call(type=amd.F32, channels=(64, 64), n=None, rows=4, zero_point=0, out=1 << 20, bits=1 << 21, inputs=None):
    k = len(channels)
    ptrs = (C.c_void_p * max(1, k))(*(inputs if inputs is not None else [4096 * (i + 1) for i in range(k)]))
    ch = (C.c_int32 * max(1, k))(*channels)
    return amd.lib().lce_hip_concat(type, ptrs, ch, k if n is None else n, rows, zero_point, C.c_void_p(out), C.c_void_p(bits), None)


@pytest.mark.parametrize("kw,msg", [
    (dict(channels=(64,)), "num_inputs"),
    (dict(channels=(8,) * 9), "num_inputs"),
    (dict(n=0), "num_inputs"),
    (dict(n=-1), "num_inputs"),
    (dict(channels=(64, 0)), "channels must be positive"),
    (dict(channels=(-4, 64)), "channels must be positive"),
    (dict(channels=(2 ** 30, 2 ** 30)), "2\\^31"),
    (dict(type=amd.BOOL), "type"),
    (dict(type=7), "type"),
    (dict(type=amd.BITPACKED), "no bit output"),
    (dict(out=0, bits=0), "both outputs"),
    (dict(type=amd.I8, zero_point=128), "zero point"),
    (dict(type=amd.I8, zero_point=-129), "zero point"),
    (dict(zero_point=1), "zero point"),
    (dict(type=amd.BITPACKED, bits=0, zero_point=1), "zero point"),
    (dict(inputs=[4096, 0]), "null"),
    (dict(out=4096 + 512), "overlaps input 0"),                     # inside input 0: 4 rows x 64 floats = 1024 bytes
    (dict(out=8192 - 16), "overlaps input 1"),                      # ends inside input 1
    (dict(inputs=[4096, (1 << 20) + 2044]), "overlaps input 1"),    # the joined tensor is 2048 bytes
    (dict(out=0, bits=4096 + 1020), "overlaps input 0"),
    (dict(bits=(1 << 20) + 2044), "outputs overlap"),
])
def test_c_entry_refuses_bad_arguments(kw, msg):
    assert _c_call(**kw) == amd.ERR_INVALID
    assert re.search(msg, amd.lib().lce_hip_last_error().decode())


def test_c_entry_accepts_the_edges_of_the_checks_up_to_the_device():
    """Touching ranges do not overlap, one input may appear twice, and zero rows is a no-op even with null pointers.  Without a
    device the accepted calls end at ERR_NO_DEVICE; none of them is ERR_INVALID."""
    assert _c_call(rows=0) == amd.OK
    assert _c_call(rows=0, out=0, bits=0, inputs=[0, 0]) == amd.OK
    assert _c_call(type=amd.I8, rows=0, zero_point=-128) == amd.OK
    if amd.device_count() == 0:
        for kw in (dict(out=4096 + 1024, inputs=[4096, 1 << 22]), dict(inputs=[4096, 4096]), dict(type=amd.I8, zero_point=127),
                   dict(type=amd.BITPACKED, bits=0), dict(bits=0), dict(out=0)):
            assert _c_call(**kw) == amd.ERR_NO_DEVICE, kw


X = np.zeros((2, 3, 64), np.float32)


@pytest.mark.parametrize("tensors,kw,msg", [
    ([X], {}, "2..8 tensors"),
    ([X] * 9, {}, "2..8 tensors"),
    ([X, X.astype(np.float64)], {}, "tensor 1 must be float32"),
    ([X.astype(np.float64)] * 2, {}, "float32, int8 or int32"),
    ([X, np.zeros((2, 4, 64), np.float32)], {}, "tensor 1 must be"),
    ([X, np.zeros((2, 3, 0), np.float32)], {}, "tensor 1 must be"),
    ([X.astype(np.int32)] * 2, dict(out_bits=True), "no bit output"),
    ([X, X], dict(zero_point=3), "zero point"),
    ([X.astype(np.int8)] * 2, dict(zero_point=128), "zero point"),
    ([X, X], dict(out=False), "no output"),
    ([X, X], dict(out=np.zeros((2, 3, 127), np.float32)), "out must be"),
    ([X, X], dict(out=np.zeros((2, 3, 128), np.int8)), "out must be"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, tensors, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    with pytest.raises(ValueError, match=msg):
        amd.concat(tensors, **kw)


def test_open_opts():
    lib = mr.tflite_lib()
    files = [mixed_model()[0], dense_block_model()[0], int8_dense_model()[0]]
    size = C.sizeof(mr._OpenOptions)
    assert size == 8
    for data in files:
        for sections in range(8):
            h = lib.lce_tflite_model_open_opts(data, len(data), C.byref(mr._OpenOptions(size, sections)), None, 0)
            assert h, sections
            if sections < 4:                                   # exactly lce_tflite_model_open_ex with the same value
                h2 = lib.lce_tflite_model_open_ex(data, len(data), sections, None, 0)
                assert h2 and _sections_of(h) == _sections_of(h2)
                lib.lce_tflite_model_close(h2)
            lib.lce_tflite_model_close(h)
        for sections in (8, 16, 12, 1 << 31):
            err = C.create_string_buffer(128)
            assert not lib.lce_tflite_model_open_opts(data, len(data), C.byref(mr._OpenOptions(size, sections)), err, 128)
            assert b"flags" in err.value or b"sections" in err.value
        for wrong in (0, 4, 12, 16):
            err = C.create_string_buffer(128)
            assert not lib.lce_tflite_model_open_opts(data, len(data), C.byref(mr._OpenOptions(wrong, 4)), err, 128)
            assert b"struct_size" in err.value
    err = C.create_string_buffer(128)
    assert not lib.lce_tflite_model_open_opts(files[0], len(files[0]), None, err, 128) and b"options" in err.value
    assert not lib.lce_tflite_model_open_opts(None, 0, C.byref(mr._OpenOptions(size, 4)), err, 128) and b"null buffer" in err.value
    assert not lib.lce_tflite_model_open_opts(b"junk", 4, C.byref(mr._OpenOptions(size, 4)), err, 128)


def test_open_ex_still_refuses_the_new_bit_and_the_abi_version_stays():
    data = dense_block_model()[0]
    err = C.create_string_buffer(128)
    for flags in (4, 5, 7):
        assert not mr.tflite_lib().lce_tflite_model_open_ex(data, len(data), flags, err, 128)
        assert b"flags" in err.value
    assert amd.lib().lce_hip_abi_version() == 3
    assert "lce_hip_concat" in amd.ABI_SYMBOLS and hasattr(amd.lib(), "lce_hip_concat")


def test_the_python_constructor_uses_open_opts_only_for_the_new_flag(monkeypatch):
    data = dense_block_model()[0]
    lib = mr.tflite_lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name in ("lce_tflite_model_open_ex", "lce_tflite_model_open_opts"):
                calls.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(mr, "tflite_lib", lambda: Spy())
    mr.LceModel(data, elementwise_sections=True, int8_add_sections=True)
    assert calls == ["lce_tflite_model_open_ex"]
    del calls[:]
    mr.LceModel(data, concat_sections=True)
    assert calls == ["lce_tflite_model_open_opts"]


def test_stats_are_zero_before_any_run():
    model = mr.LceModel(dense_block_model()[0], elementwise_sections=True, concat_sections=True)
    assert model.concat_stats() == (0, 0)


# ---- the build: no scratch memory, no LDS, no scalar-memory writes -------------------------------------------------------------
NEW_SOURCES = ("lce_kernels_join.h", "lce_tu_join.hip")


def test_the_new_sources_hold_no_scalar_memory_write():
    assert not H.sources_with_scalar_memory_writes(NEW_SOURCES)


def test_the_concat_kernels_use_no_scratch_and_no_lds():
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_join.hip")
    assert sorted(k for k in kernels if "join" in k) == sorted(k for k in kernels), kernels
    # vector: float with and without bits, each with and without an addend; int8 with and without bits; rows: float with and
    # without an addend; int8
    assert len(kernels) == 9, kernels
    for key in H.RESOURCE_KEYS:
        assert resources[key] == ["0"] * len(kernels), (key, resources[key])
    assert not [m for m in mnemonics if H.scalar_memory_write(m)]
    # the vector path moves 16 bytes per lane and instruction
    assert "global_load_dwordx4" in mnemonics and "global_store_dwordx4" in mnemonics
