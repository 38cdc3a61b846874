"""The int8 residual ADD between binary layers (lce_hip_add_int8, LCE_TFLITE_SECTIONS_INT8_ADD) on the CPU: TFLite's Prepare
against the NumPy restatement (tests/int8_add_ref.py), the restatement against the specification's known answers, the partition
with and without the flag, which int8 operators stay with the host, shape inference over the absorbed tensors, the argument
checks that come before any device call, and the build of the new sources.  The GPU side is tests/test_gpu_int8_add.py."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import hipcc_lib as H
import int8_add_ref as R
import oracle_lib as O
from section_models import ADD, MUL, NONE, RELU, RELU6, RELU_N1_TO_1, TANH, bconv_options, ew_op, mixed_model
import synth
from tflite_writer import ModelBuilder

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

EQUAL_SCALES = (0.5, 1, 0.5, 2, 0.7, 3)
RATIO_2_12 = (1.0, 4, 2.0 ** -12, -9, 1.0, 0)
# no cheap form applies: an output shift of 0 (the sum saturates almost everywhere), an input multiplier that quantizes to 0
NO_CHEAP_FORM = ((1.0, 0, 1.0, 0, 3e-6, 0), (1.0, 0, 2.0 ** -40, 0, 1.0, 0))


# ---- the restatement against the known answers ----------------------------------------------------------------------------
@pytest.mark.parametrize("q,act,want", [
    (R.SET_A, R.ACT_NONE, ((20, 1073741824, 0, 1593432776, -1, 1508064419, -19, -128, 127), 14, -513522, "05f28dfe", 0.039)),
    (R.SET_A, R.ACT_RELU, ((20, 1073741824, 0, 1593432776, -1, 1508064419, -19, -7, 127), 7, 1243568, "4ed62da3", 0.519)),
    (R.SET_B, R.ACT_NONE, ((20, 1073741824, -1, 1073741824, 0, 1434701836, -18, -128, 127), 0, -2019054, "00071e0d", 0.318)),
    (R.SET_C, R.ACT_NONE, ((20, 1867377040, -1, 1073741824, 0, 1593294349, -19, -128, 127), 0, -44439, "ec19eaad", 0.081)),
])
def test_the_restatement_reproduces_the_known_answers(q, act, want):
    params, diff, total, crc, sat = R.table_row(q, act)
    assert (params, diff, total, crc) == want[:4]
    assert round(sat, 3) == want[4]


def test_set_a_has_pairs_that_differ_from_real_rounding():
    """So a float shortcut in the kernel cannot pass the GPU test that uses set A."""
    x1, x2 = R.all_pairs()
    assert np.count_nonzero(R.add_q(x1, x2, R.SET_A) != R.real_rounding(x1, x2, R.SET_A)) >= 1


# ---- lce_hip_add_int8_prepare -------------------------------------------------------------------------------------------
def c_prepare(q, act=0):
    p = amd.AddInt8Params()
    code = amd.lib().lce_hip_add_int8_prepare(C.byref(amd.AddInt8Desc(*q, act)), C.byref(p))
    return code, tuple(getattr(p, n) for n in R.PARAM_NAMES)


@pytest.mark.parametrize("q", [R.SET_A, R.SET_B, R.SET_C, EQUAL_SCALES, RATIO_2_12, *NO_CHEAP_FORM])
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_RELU_N1_TO_1, R.ACT_RELU6])
def test_prepare_equals_the_restatement(q, act):
    assert c_prepare(q, act) == (amd.OK, R.prepare(*q, act))


def test_prepare_equals_the_restatement_on_random_sets():
    for k, q in enumerate(R.random_sets(300, seed=1)):
        act = k % 4
        assert c_prepare(q, act) == (amd.OK, R.prepare(*q, act)), (q, act)
        assert amd.add_int8_params(q[0:2], q[2:4], q[4:6], act)["out_multiplier"] == R.prepare(*q, act)[5]


@pytest.mark.parametrize("q,act,msg", [
    ((0.0, 0, 1.0, 0, 1.0, 0), 0, "in1_scale must be finite and positive"),
    ((1.0, 0, -1.0, 0, 1.0, 0), 0, "in2_scale must be finite and positive"),
    ((1.0, 0, 1.0, 0, float("inf"), 0), 0, "out_scale must be finite and positive"),
    ((1.0, 0, float("nan"), 0, 1.0, 0), 0, "in2_scale must be finite and positive"),
    ((1.0, 128, 1.0, 0, 1.0, 0), 0, r"in1_zero_point must be in \[-128, 127\]"),
    ((1.0, 0, 1.0, -129, 1.0, 0), 0, r"in2_zero_point must be in \[-128, 127\]"),
    ((1.0, 0, 1.0, 0, 1.0, 300), 0, r"out_zero_point must be in \[-128, 127\]"),
    ((1.0, 0, 1.0, 0, 1.0, 0), 4, "unknown activation 4"),
    ((1.0, 0, 1.0, 0, 1.0, 0), -1, "unknown activation -1"),
    ((1.0, 0, 1.0, 0, 1e-7, 0), 0, r"real multiplier of out is .* not in \(0, 1\)"),
])
def test_prepare_refusals(q, act, msg):
    code, _ = c_prepare(q, act)
    assert code == amd.ERR_INVALID
    assert re.search(msg, amd.lib().lce_hip_last_error().decode())
    # the launch refuses the same, before it looks at a pointer (these are not addresses of anything)
    assert amd.lib().lce_hip_add_int8(C.byref(amd.AddInt8Desc(*q, act)), C.c_void_p(16), C.c_void_p(32), 4, 64,
                                      C.c_void_p(48), C.c_void_p(64), None) == amd.ERR_INVALID
    assert re.search(msg, amd.lib().lce_hip_last_error().decode())


def test_both_outputs_null_is_refused_and_empty_tensors_are_a_no_op():
    d = amd.AddInt8Desc(*R.SET_A, 0)
    call = lambda rows, ch, out, bits: amd.lib().lce_hip_add_int8(C.byref(d), C.c_void_p(16), C.c_void_p(32), rows, ch,
                                                                  C.c_void_p(out), C.c_void_p(bits), None)
    assert call(4, 64, 0, 0) == amd.ERR_INVALID
    assert "both outputs are null" in amd.lib().lce_hip_last_error().decode()
    assert call(0, 64, 48, 64) == amd.OK
    assert call(4, 0, 48, 64) == amd.OK


# ---- the variant chooser (the proof runs on the host) ---------------------------------------------------------------------
def chosen(q, act=0):
    return amd.add_int8_params(q[0:2], q[2:4], q[4:6], act)["variant"]


def test_the_chooser_picks_by_proof():
    assert chosen(R.SET_A) == amd.ADD_INT8_SPLIT and chosen(R.SET_C) == amd.ADD_INT8_SPLIT
    assert chosen(R.SET_B) == amd.ADD_INT8_SHIFT                      # 0.0157 / 0.0314 is exactly 1/2 in float32
    assert chosen(EQUAL_SCALES) == amd.ADD_INT8_SHIFT and chosen(RATIO_2_12) == amd.ADD_INT8_SHIFT
    for q in NO_CHEAP_FORM:
        assert chosen(q) == amd.ADD_INT8_LITERAL, q
    # a variant that is not proven for a parameter set is refused when forced (before any pointer or device is touched)
    d = amd.AddInt8Desc(*R.SET_A, 0)
    args = (C.c_void_p(16), C.c_void_p(32), 4, 64, C.c_void_p(48), C.c_void_p(64), None)
    assert amd.lib().lce_hip_add_int8_forced(C.byref(d), amd.ADD_INT8_SHIFT, *args) == amd.ERR_INVALID
    assert "not proven" in amd.lib().lce_hip_last_error().decode()
    assert amd.lib().lce_hip_add_int8_forced(C.byref(d), 3, *args) == amd.ERR_INVALID
    assert "unknown variant" in amd.lib().lce_hip_last_error().decode()


# ---- the partition ------------------------------------------------------------------------------------------------------------
# (H, C, Cout, stride, shortcut) per layer: a Bi-RealNet style body on the int8 output path, batch norm folded into LceBconv2d
INT8_BODY = ((56, 64, 64, 1, True), (56, 64, 64, 1, True), (56, 64, 128, 2, False), (28, 128, 128, 1, True),
             (28, 128, 128, 1, True), (28, 128, 256, 2, False), (14, 256, 256, 1, True))


def int8_body_model(layers=INT8_BODY, seed=0, acts=(NONE, RELU, NONE, RELU6, NONE, NONE, RELU_N1_TO_1)):
    """r (int8 [1,H,W,C]) -> per layer LceQuantize -> LceBconv2d (int8 out) [-> ADD(y, r) int8] -> the last tensor (graph
    output).  Returns (file, input tensor, output tensor, per-layer dicts with the ADD's six quantization numbers)."""
    b = ModelBuilder()
    g = synth.rng(seed + 77)
    quant = lambda: (float(np.float32(g.uniform(0.15, 0.6))), int(g.integers(-20, 21)))
    H, C0 = layers[0][0], layers[0][1]
    q_r = quant()
    x = b.tensor([1, H, H, C0], np.int8, "x", scale=q_r[0], zero_point=q_r[1])
    r, info = x, []
    f32 = lambda shape, name, data: b.tensor(shape, np.float32, name, data)
    for k, (h, c, cout, stride, shortcut) in enumerate(layers):
        spec = O.ConvSpec(1, h, h, c, 3, 3, cout, stride_h=stride, stride_w=stride, padding=O.PADDING_SAME, pad_values=1)
        _, w, m, bias = synth.conv_inputs(spec, seed + 10 * k + 1)
        m = (m * np.float32(0.05)).astype(np.float32)
        oh = spec.out_h
        q_y = quant()
        qt = b.tensor([1, h, h, (c + 31) // 32], np.int32, "q%d" % k)
        y = b.tensor([1, oh, oh, cout], np.int8, "y%d" % k, scale=q_y[0], zero_point=q_y[1])
        b.custom_op("LceQuantize", [r], [qt], b"")
        b.custom_op("LceBconv2d", [qt, b.tensor(w.shape, np.int32, "w%d" % k, w), f32([cout], "m%d" % k, m),
                                   f32([cout], "b%d" % k, bias), -1], [y], bconv_options(spec))
        li = dict(spec=spec, shortcut=shortcut, y=y, q_y=q_y, act=acts[k % len(acts)])
        if shortcut:
            q_s = quant()
            s = b.tensor([1, oh, oh, cout], np.int8, "r%d" % k, scale=q_s[0], zero_point=q_s[1])
            li["add"] = ew_op(b, ADD, [y, r], [s], li["act"])
            li["q"] = (q_y[0], q_y[1], q_r[0], q_r[1], q_s[0], q_s[1])
            r, q_r = s, q_s
        else:
            r, q_r = y, q_y
        li["out"] = r
        info.append(li)
    b.inputs, b.outputs = [x], [r]
    return b.finish(), x, r, info


def test_the_int8_body_is_one_section_with_the_flag_and_unchanged_without():
    data, x, out, info = int8_body_model()
    assert len(info) >= 6 and any(not li["shortcut"] and li["spec"].stride_h == 2 for li in info)
    model = mr.LceModel(data, int8_add_sections=True)
    assert len(model.sections) == 1 and model.sections[0].ops == list(range(len(model.operators)))
    assert model.sections[0].inputs == [x] and model.sections[0].outputs == [out]
    assert mr.Interpreter(model).lce_only
    assert mr.Interpreter(data, int8_add_sections=True).lce_only
    # the default partition: cut at every ADD (what lce_tflite_model_open gives, and gave before the flag existed)
    adds = [li["add"] for li in info if li["shortcut"]]
    want, cur = [], []
    for i in range(len(model.operators)):
        if i in adds:
            want.append(cur)
            cur = []
        else:
            cur.append(i)
    want = [s for s in want + [cur] if s]
    plain = mr.LceModel(data)
    assert [s.ops for s in plain.sections] == want and len(want) == len(adds)
    assert not mr.Interpreter(data).lce_only
    # the float flag alone leaves an int8 ADD with the host
    assert [s.ops for s in mr.LceModel(data, elementwise_sections=True).sections] == want
    # both flags: the int8 body is still one section
    both = mr.LceModel(data, elementwise_sections=True, int8_add_sections=True)
    assert [s.ops for s in both.sections] == [list(range(len(model.operators)))]


def test_the_flags_of_open_ex():
    data, _, _ = mixed_model()
    lib = mr.tflite_lib()
    for flags in (2, 3):
        h = lib.lce_tflite_model_open_ex(data, len(data), flags, None, 0)
        assert h
        lib.lce_tflite_model_close(h)
    for flags in (4, 6, 8):
        err = C.create_string_buffer(128)
        assert not lib.lce_tflite_model_open_ex(data, len(data), flags, err, 128)
        assert b"flags" in err.value
    # a float graph is partitioned by the int8 flag exactly as by none, and by both flags exactly as by the float flag
    sections = lambda **kw: [(s.ops, s.inputs, s.outputs) for s in mr.LceModel(data, **kw).sections]
    assert sections(int8_add_sections=True) == sections()
    assert sections(int8_add_sections=True, elementwise_sections=True) == sections(elementwise_sections=True)


def _graph(case):
    """x (int8) -> LceQuantize -> LceBconv2d (int8) -> y -> <op under test>(y, x or other) -> z -> LceQuantize -> q2.
    Returns (file, index of the op under test)."""
    H, Cc = 8, 64
    spec = O.ConvSpec(1, H, H, Cc, 3, 3, Cc, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i8 = lambda shape, name, data=None, scale=0.5, zp=1: b.tensor(shape, np.int8, name, data, scale=scale, zero_point=zp)
    x = i8([1, H, H, Cc], "x")
    q = b.tensor([1, H, H, 2], np.int32, "q")
    y = i8([1, H, H, Cc], "y", scale=0.25, zp=-2)
    z = i8([1, H, H, Cc], "z", scale=0.6, zp=3)
    inputs = [x]
    if case == "outside":
        # ADD(x, x2): both operands come from outside; it is ready from the start and is a stem operator
        x2 = i8([1, H, H, Cc], "x2")
        inputs.append(x2)
        k = ew_op(b, ADD, [x, x2], [z], NONE)
        b.custom_op("LceQuantize", [z], [q], b"")
        b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                    bconv_options(spec))
        b.inputs, b.outputs = inputs, [y]
        return b.finish(), k
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                bconv_options(spec))
    if case == "constant":
        k = ew_op(b, ADD, [y, i8([1, H, H, Cc], "c", np.ones((1, H, H, Cc), np.int8))], [z], NONE)
    elif case == "broadcast":
        x2 = i8([1, 1, 1, Cc], "x2")
        inputs.append(x2)
        k = ew_op(b, ADD, [y, x2], [z], NONE)
    elif case == "mul":
        k = ew_op(b, MUL, [y, x], [z], NONE)
    elif case == "tanh":
        k = ew_op(b, ADD, [y, x], [z], TANH)
    elif case == "no_quantization":
        x2 = b.tensor([1, H, H, Cc], np.int8, "x2")
        inputs.append(x2)
        k = ew_op(b, ADD, [y, x2], [z], NONE)
    elif case == "float_input":
        x2 = f32([1, H, H, Cc], "x2")
        inputs.append(x2)
        k = ew_op(b, ADD, [y, x2], [z], NONE)
    elif case == "refused_by_prepare":
        z = i8([1, H, H, Cc], "z2", scale=1e-8, zp=3)           # the output multiplier would exceed 1
        k = ew_op(b, ADD, [y, x], [z], NONE)
    else:                                                          # the positive control "joins"
        k = ew_op(b, ADD, [y, x], [z], RELU)
    q2 = b.tensor([1, H, H, 2], np.int32, "q2")
    b.custom_op("LceQuantize", [z], [q2], b"")
    b.inputs, b.outputs = inputs, [q2]
    return b.finish(), k


@pytest.mark.parametrize("case", ["constant", "broadcast", "mul", "tanh", "no_quantization", "float_input", "outside",
                                  "refused_by_prepare"])
def test_int8_operators_that_stay_with_the_host(case):
    data, k = _graph(case)
    model = mr.LceModel(data, int8_add_sections=True)
    assert all(k not in s.ops for s in model.sections), (case, [s.ops for s in model.sections])
    assert not mr.Interpreter(model).lce_only
    assert [s.ops for s in model.sections] == [s.ops for s in mr.LceModel(data).sections]


def test_a_qualifying_int8_add_joins():
    data, k = _graph("joins")
    model = mr.LceModel(data, int8_add_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3]] and k == 2
    assert mr.Interpreter(model).lce_only
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3]]
    assert [s.ops for s in mr.LceModel(data, elementwise_sections=True).sections] == [[0, 1], [3]]


def test_section_tensor_shape_over_the_absorbed_tensors_at_another_batch():
    data, x, out, info = int8_body_model()
    model = mr.LceModel(data, int8_add_sections=True)
    for li in info:
        oh, cout = li["spec"].out_h, li["spec"].channels_out
        assert model.section_tensor_shape(0, li["y"], 5) == ((5, oh, oh, cout), 5 * oh * oh * cout), li
        assert model.section_tensor_shape(0, li["out"], 5) == ((5, oh, oh, cout), 5 * oh * oh * cout), li
    assert model.section_tensor_shape(0, out, 256)[0] == (256, 14, 14, 256)


def test_a_file_whose_add_inputs_disagree_with_the_inferred_shapes_is_refused():
    """The ADD's tensors agree with each other in the file, but the convolution (stride 2) produces a smaller tensor than the
    file declares for it: the walk must fail instead of reading past the convolution's buffer."""
    H, Cc = 8, 64
    spec = O.ConvSpec(1, H, H, Cc, 3, 3, Cc, stride_h=2, stride_w=2, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, 5)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i8 = lambda name: b.tensor([1, H, H, Cc], np.int8, name, scale=0.5, zero_point=1)
    x, y, z = i8("x"), i8("y"), i8("z")                        # y is declared 8x8; the convolution infers 4x4
    q = b.tensor([1, H, H, 2], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    b.custom_op("LceBconv2d", [q, b.tensor(w.shape, np.int32, "w", w), f32([Cc], "m", m), f32([Cc], "b", bias), -1], [y],
                bconv_options(spec))
    ew_op(b, ADD, [y, x], [z], NONE)
    b.inputs, b.outputs = [x], [z]
    model = mr.LceModel(b.finish(), int8_add_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2]]
    with pytest.raises(amd.LceHipError, match="int8 ADD input"):
        model.section_tensor_shape(0, z, 2)


# ---- amd.add_int8 argument checks (no device needed: they come first) --------------------------------------------------------
X = np.zeros((2, 3, 64), np.int8)
QA = dict(q1=R.SET_A[0:2], q2=R.SET_A[2:4], q_out=R.SET_A[4:6])


@pytest.mark.parametrize("x1,x2,kw,msg", [
    (X.astype(np.float32), X, {}, "x1 must be an int8"),
    (X, X.astype(np.uint8), {}, "x2 must be int8"),
    (X, np.zeros((2, 3, 32), np.int8), {}, "x2 must be int8 of x1's shape"),
    (X, X, dict(out=False), "no output requested"),
    (X, X, dict(out=np.zeros((2, 3, 63), np.int8)), "out must be"),
    (X, X, dict(out=np.zeros((2, 3, 64), np.int32)), "out must be"),
    (X, X, dict(out_bits=np.zeros((2, 3, 3), np.int32)), "out_bits must be"),
    (X, X, dict(q1=(0.0, 0)), "q1 scale"),
    (X, X, dict(q2=(float("nan"), 0)), "q2 scale"),
    (X, X, dict(q_out=(0.5, 128)), "q_out zero point"),
    (X, X, dict(q1=(0.5, 1.5)), "q1 zero point"),
    (X, X, dict(q1=0.5), r"q1 must be \(scale, zero_point\)"),
    (X, X, dict(activation=4), "unknown activation"),
    (X, X, dict(variant=3), "unknown variant"),
])
def test_python_checks_fail_before_any_device_call(monkeypatch, x1, x2, kw, msg):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(amd, "lib", no_device)
    with pytest.raises(ValueError, match=msg):
        amd.add_int8(x1, x2, **{**QA, **kw})


# ---- the build -------------------------------------------------------------------------------------------------------------------
NEW_SOURCES = ("lce_kernels_eltwise_i8.h", "lce_tu_eltwise_i8.hip")


def test_the_new_sources_hold_no_scalar_memory_write():
    assert not H.sources_with_scalar_memory_writes(NEW_SOURCES)


def test_the_int8_add_kernels_use_no_scratch_and_no_lds():
    kernels, resources, text, mnemonics = H.compile_unit("lce_tu_eltwise_i8.hip")
    # the unit emits only its own kernels: a flat and a row kernel per variant
    assert sorted(k for k in kernels if "add_i8_flat" in k or "add_i8_rows" in k) == sorted(kernels), kernels
    assert len(kernels) == 6 and len(set(kernels)) == 6, kernels
    for key in H.RESOURCE_KEYS:
        assert resources[key] == ["0"] * 6, (key, resources[key])
    assert not [m for m in mnemonics if H.scalar_memory_write(m)]
    assert not [m for m in mnemonics if m.startswith("ds_") or m.startswith("scratch_")], mnemonics
    # the cheap variants hold ONE 64-bit multiply-add per element and no slow 32-bit multiply; the literal one holds six
    body = lambda v: text.split("_ZN3lce11add_i8_flatILi%dEEEvNS_9AddI8ArgsEm:" % v)[1].split(".Lfunc_end")[0]
    count = lambda v, m: len(re.findall(r"^\s+" + m + r"\b", body(v), re.M))
    for v in (amd.ADD_INT8_SPLIT, amd.ADD_INT8_SHIFT):
        assert 64 <= count(v, "v_mad_i64_i32") <= 66, (v, count(v, "v_mad_i64_i32"))       # 64 elements per lane and iteration
        assert count(v, "v_mul_lo_u32") == 0 and count(v, "v_mul_hi_i32") == 0 and count(v, "v_mul_hi_u32") == 0
    assert count(amd.ADD_INT8_LITERAL, "v_mad_i64_i32") >= 6 * 64
