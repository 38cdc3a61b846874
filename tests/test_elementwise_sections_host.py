"""Float ADD / MUL between binary layers inside the sections (LCE_TFLITE_SECTIONS_ELEMENTWISE, include/lce_tflite_model.h) on the
CPU: the partition with and without the flag, which builtin operators stay with the host, AddOptions / MulOptions activations
through the reader, shape inference over the absorbed tensors, and the argument checks of lce_hip_elementwise /
amd.elementwise, which all fail before any device is touched.  The GPU side is tests/test_gpu_elementwise.py."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import hipcc_lib as H
import oracle_lib as O
from section_models import (ADD, BODY, CONV_2D, MUL, NONE, RELU, RELU6, RELU_N1_TO_1, SUB, TANH, bconv_options, body_model, ew_op,
                            layer, mixed_model)
import synth
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")


def test_partition_of_the_mixed_graph_with_and_without_the_flag():
    data, t, _ = mixed_model()
    plain = mr.LceModel(data)
    assert [s.ops for s in plain.sections] == [[1, 2], [4, 5], [7, 8, 9, 10, 12]]      # unchanged by default
    ew = mr.LceModel(data, elementwise_sections=True)
    assert [s.ops for s in ew.sections] == [[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]]
    assert ew.sections[0].inputs == [t["s"]]
    assert ew.sections[0].outputs == [t["y3"], t["d2"]]
    assert not mr.Interpreter(data, elementwise_sections=True).lce_only       # the stem CONV_2D and MAX_POOL_2D remain
    assert not mr.Interpreter(data).lce_only


def _graph(case):
    """x -> [ADD stem] -> LceQuantize -> LceBconv2d -> y -> <op under test> -> z -> LceQuantize -> q2.  Returns (file, index
    of the op under test)."""
    H, C = 8, 64
    spec = O.ConvSpec(1, H, H, C, 3, 3, C, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, H, H, C], "x")
    cC = f32([C], "cC", np.ones(C, np.float32))
    src, tested = x, None
    if case == "stem":
        s = f32([1, H, H, C], "s")
        tested = ew_op(b, ADD, [x, cC], [s], NONE)
        src = s
    q = b.tensor([1, H, H, 2], np.int32, "q")
    y_type = np.int8 if case == "int8" else np.float32
    y = b.tensor([1, H, H, C], y_type, "y", scale=0.5 if case == "int8" else None, zero_point=0 if case == "int8" else None)
    b.custom_op("LceQuantize", [src], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([C], "m", m), f32([C], "b", bias), -1], [y],
                bconv_options(spec))
    z = b.tensor([1, H, H, C], y_type, "z", scale=0.5 if case == "int8" else None, zero_point=0 if case == "int8" else None)
    if case == "broadcast":
        k = ew_op(b, ADD, [y, f32([1, H, 1, C], "cH", np.ones((1, H, 1, C), np.float32))], [z], NONE)
    elif case == "int8":
        k = ew_op(b, ADD, [y, b.tensor([C], np.int8, "c8", np.ones(C, np.int8), scale=0.5, zero_point=0)], [z], NONE)
    elif case == "sub":
        k = ew_op(b, SUB, [y, cC], [z], None)
    elif case == "tanh":
        k = ew_op(b, ADD, [y, cC], [z], TANH)
    else:                                       # "stem" and the positive control "joins"
        k = ew_op(b, ADD, [y, cC], [z], RELU)
    q2 = b.tensor([1, H, H, 2], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = [x], [q2]
    return b.finish(), (tested if case == "stem" else k)


@pytest.mark.parametrize("case", ["broadcast", "int8", "sub", "tanh", "stem"])
def test_builtin_ops_that_stay_with_the_host(case):
    data, k = _graph(case)
    model = mr.LceModel(data, elementwise_sections=True)
    assert all(k not in s.ops for s in model.sections), (case, [s.ops for s in model.sections])
    assert not mr.Interpreter(model).lce_only


def test_a_qualifying_add_joins_and_the_graph_becomes_lce_only():
    data, k = _graph("joins")
    model = mr.LceModel(data, elementwise_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and k == 2
    assert mr.Interpreter(model).lce_only
    assert not mr.Interpreter(data).lce_only                       # the default is unchanged
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]


def test_a_residual_from_a_builtin_op_outside_is_a_section_input():
    """x -> CONV_2D (host) -> s;  s -> LceQuantize -> LceBconv2d -> y;  ADD(y, s) joins, s is read from outside."""
    H, C = 8, 64
    spec = O.ConvSpec(1, H, H, C, 3, 3, C, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 6)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x, s, y, r = f32([1, H, H, 3], "x"), f32([1, H, H, C], "s"), f32([1, H, H, C], "y"), f32([1, H, H, C], "r")
    q = b.tensor([1, H, H, 2], np.int32, "q")
    b.builtin_op(CONV_2D, [x, f32([C, 3, 3, 3], "k", np.ones((C, 3, 3, 3), np.float32)), f32([C], "kb", np.zeros(C, np.float32))], [s])
    b.custom_op("LceQuantize", [s], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([C], "m", m), f32([C], "b", bias), -1], [y],
                bconv_options(spec))
    ew_op(b, ADD, [y, s], [r], None)
    b.inputs, b.outputs = [x], [r]
    model = mr.LceModel(b.finish(), elementwise_sections=True)
    assert [(sec.ops, sec.inputs, sec.outputs) for sec in model.sections] == [([1, 2, 3], [s], [r])]


def test_add_and_mul_activations_round_trip_through_the_reader():
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, 2, 2, 4], "x")
    c = f32([4], "c", np.ones(4, np.float32))
    want = []
    prev = x
    for code in (ADD, MUL):
        for act in (None, NONE, RELU, RELU_N1_TO_1, RELU6, TANH, 5):
            out = f32([1, 2, 2, 4], "t%d" % len(want))
            ew_op(b, code, [prev, c], [out], act)
            want.append(0 if act is None else act)
            prev = out
    b.builtin_op(CONV_2D, [prev, c, c], [f32([1, 2, 2, 4], "z")])   # no options at all
    want.append(0)
    b.inputs, b.outputs = [x], [prev]
    model = mr.LceModel(b.finish())
    assert [op.activation for op in model.operators] == want


def test_section_tensor_shape_over_the_absorbed_tensors_at_batch_3():
    data, t, p = mixed_model()
    model = mr.LceModel(data, elementwise_sections=True)
    for name in ("y0", "r0", "y1", "r1"):
        assert model.section_tensor_shape(0, t[name], 3) == ((3, 10, 10, 64), 3 * 10 * 10 * 64 * 4), name
    assert model.section_tensor_shape(0, t["y3"], 3)[0] == (3, 5, 5, 32)
    assert model.section_tensor_shape(0, t["d2"], 3)[0] == (3, 10, 10, 96)


def test_the_body_graph_is_one_section():
    data, x, out, info, outs = body_model()
    model = mr.LceModel(data, elementwise_sections=True)
    assert len(model.sections) == 1 and model.sections[0].ops == list(range(len(model.operators)))
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only
    # default mode: one (LceQuantize, LceBconv2d) section per layer, the ADD / MUL between them on the host
    plain = mr.LceModel(data)
    assert len(plain.sections) == len(BODY) and all(len(s.ops) == 2 for s in plain.sections)
    assert model.section_tensor_shape(0, out, 256)[0] == (256, 14, 14, 256)


def test_open_ex_refuses_unknown_flags():
    data, _, _ = mixed_model()
    err = C.create_string_buffer(128)
    assert not mr.tflite_lib().lce_tflite_model_open_ex(data, len(data), 6, err, 128)
    assert b"flags" in err.value


# ---- lce_hip_elementwise / amd.elementwise argument checks (no device needed: they come first) --------------------------
def _c_call(steps, n=None, rows=4, channels=64, out=1, bits=1, x=16):
    arr = (amd.EwStep * max(1, len(steps)))(*[amd.EwStep(*s) for s in steps])
    return amd.lib().lce_hip_elementwise(C.c_void_p(x), rows, channels, arr, len(steps) if n is None else n,
                                         C.c_void_p(out), C.c_void_p(bits), None)


@pytest.mark.parametrize("steps,n,kw,msg", [
    ([(0, 0, 0, 1.0, 0)], 0, {}, "num_steps"),
    ([(0, 0, 0, 1.0, 0)] * 9, None, {}, "num_steps"),
    ([(2, 0, 0, 1.0, 0)], None, {}, "unknown op"),
    ([(0, 3, 0, 1.0, 0)], None, {}, "unknown operand"),
    ([(0, 0, 0, 1.0, 4)], None, {}, "unknown activation"),
    ([(0, 1, 0, 0.0, 0)], None, {}, "null operand"),
    ([(1, 2, 0, 0.0, 0)], None, {}, "null operand"),
    ([(0, 0, 0, 1.0, 0)], None, dict(out=0, bits=0), "both outputs"),
    ([(0, 0, 0, 1.0, 0)], None, dict(channels=1 << 31), "2\\^31"),
])
def test_c_entry_refuses_bad_arguments(steps, n, kw, msg):
    assert _c_call(steps, n, **kw) == amd.ERR_INVALID
    assert re.search(msg, amd.lib().lce_hip_last_error().decode())


def test_c_entry_empty_tensors_are_a_no_op():
    assert _c_call([(0, 0, 0, 1.0, 0)], rows=0) == amd.OK
    assert _c_call([(1, 0, 0, 2.0, 3)], channels=0) == amd.OK


@pytest.mark.parametrize("steps,kw,msg", [
    ([], {}, "steps"),
    ([("add", 1.0, amd.ACT_NONE)] * 9, {}, "steps"),
    ([("sub", 1.0, amd.ACT_NONE)], {}, "unknown op"),
    ([("add", 1.0, 7)], {}, "unknown activation"),
    ([("add", None, amd.ACT_NONE)], {}, "no operand"),
    ([("add", np.zeros(5, np.float32), amd.ACT_NONE)], {}, "operand shape"),
    ([("mul", np.zeros((2, 3, 64), np.float64), amd.ACT_NONE)], {}, "float32"),
    ([("add", 1.0, amd.ACT_NONE)], dict(out=False), "no output"),
    ([("add", 1.0, amd.ACT_NONE)], dict(out=np.zeros((2, 3, 63), np.float32)), "out must be"),
    ([("add", 1.0, amd.ACT_NONE)], dict(out_bits=np.zeros((2, 3, 3), np.int32)), "out_bits must be"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, steps, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    with pytest.raises(ValueError, match=msg):
        amd.elementwise(np.zeros((2, 3, 64), np.float32), steps, **kw)
    with pytest.raises(ValueError, match="float32"):
        amd.elementwise(np.zeros((2, 3, 64), np.float64), [("add", 1.0, amd.ACT_NONE)])


# ---- the build: no scratch memory, no scalar-memory writes -----------------------------------------------------------------
NEW_SOURCES = ("lce_kernels_eltwise.h", "lce_tu_eltwise.hip")


def test_the_new_sources_hold_no_scalar_memory_write():
    assert not H.sources_with_scalar_memory_writes(NEW_SOURCES)


def test_the_elementwise_kernels_use_no_scratch_and_no_lds():
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_eltwise.hip")
    assert sorted(k for k in kernels if "eltwise" in k) == sorted(k for k in kernels), kernels
    assert len(kernels) == 2, kernels
    for key in H.RESOURCE_KEYS:
        assert resources[key] == ["0", "0"], (key, resources[key])
    assert not [m for m in mnemonics if H.scalar_memory_write(m)]
    # one rounding per op: the float adds and multiplies are not contracted (the only fma forms are the 64-bit division's)
    assert "v_add_f32_e32" in mnemonics and "v_mul_f32_e32" in mnemonics
