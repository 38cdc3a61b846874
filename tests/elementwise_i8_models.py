"""Fixtures of the int8 elementwise chain in the model reader ("elementwise_i8" of lce_tflite_model_open_passes), built with
tests/tflite_writer.py: a two-block int8 ReActNet-style body, a requantize -> CONCATENATION join, a standalone int8 RELU6, one
file per rule of the predicate, and the NumPy side of each builtin operator they hold (tests/elementwise_i8_ref.py).  No tests here."""
import numpy as np

import elementwise_i8_ref as E
import synth
from activation_models import LOGISTIC, PRELU, RELU6_OP, RELU_N1_TO_1_OP, RELU_OP, _quantize
from section_models import ADD, MUL, NONE, RELU, RELU6, _conv, concat_op, ew_op
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

QUANTIZE = 114
UINT8, INT16 = 3, 7
NAMES = "int8_add,concat,elementwise_i8"


def _q(g, lo=0.02, hi=0.1):
    return (float(np.float32(g.uniform(lo, hi))), int(g.integers(-20, 21)))


def _i8(b, H, C, name, q):
    return b.tensor([1, H, H, C], np.int8, name, scale=q[0], zero_point=q[1])


def _const(b, shape, name, values, q):
    return b.tensor(list(shape), np.int8, name, np.asarray(values, np.int8).reshape(shape), scale=q[0], zero_point=q[1])


def reactnet_i8_model(seed=0, H=8, C=64, blocks=2, act=NONE):
    """x (int8 [1,H,H,C]) -> per block: LceQuantize, LceBconv2d 3x3 (int8 out), ADD (the shortcut), ADD (shift [C]), PRELU (alpha
    [1,1,C]), ADD (shift [1,1,1,C]) -> the next block.  Returns (file, x, output, info): info["host"] lists, per builtin operator,
    (operator, kind, input tensors, output tensor, step of elementwise_i8_ref or the residual ADD's six numbers)."""
    b = ModelBuilder()
    g = synth.rng(seed + 7)
    q_r = _q(g)
    x = _i8(b, H, C, "x", q_r)
    r, host, tails, convs = x, [], [], []
    for n in range(blocks):
        q, kq = _quantize(b, r, H, C, str(n))
        q_y = _q(g)
        y, ci = _conv(b, q, H, C, C, seed + 10 * n + 1, out_type=np.int8, quant=q_y)
        convs.append(ci)
        qs = [_q(g, 0.03, 0.15) for _ in range(4)]
        t = [_i8(b, H, C, "t%d_%d" % (n, k), qs[k]) for k in range(4)]
        q_k1, q_a, q_k2 = _q(g, 0.01, 0.05), (float(np.float32(g.uniform(0.004, 0.012))), int(g.integers(-5, 6))), _q(g, 0.01, 0.05)
        shift1, shift2 = g.integers(-128, 128, C).astype(np.int8), g.integers(-128, 128, C).astype(np.int8)
        alpha = g.integers(-128, 128, C).astype(np.int8)
        ops = [ew_op(b, ADD, [y, r], [t[0]], act),
               ew_op(b, ADD, [t[0], _const(b, [C], "shift1_%d" % n, shift1, q_k1)], [t[1]], NONE),
               b.builtin_op(PRELU, [t[1], _const(b, [1, 1, C], "alpha%d" % n, alpha, q_a)], [t[2]]),
               ew_op(b, ADD, [_const(b, [1, 1, 1, C], "shift2_%d" % n, shift2, q_k2), t[2]], [t[3]], RELU6 if n == 0 else NONE)]
        head = (q_y[0], q_y[1], q_r[0], q_r[1], qs[0][0], qs[0][1])
        steps = [("add", shift1, q_k1, qs[1], NONE), ("prelu", alpha, q_a, qs[2]), ("add", shift2, q_k2, qs[3], RELU6 if n == 0 else NONE)]
        host.append((ops[0], "residual", [y, r], t[0], (head, act)))
        q_in = qs[0]
        for k, st in enumerate(steps):
            host.append((ops[k + 1], "step", [t[k]], t[k + 1], (st, q_in)))
            q_in = qs[k + 1]
        tails.append(dict(quantize=kq, ops=ops, tensors=t, y=y, head=head, steps=steps, q_y=q_y))
        r, q_r = t[3], qs[3]
    b.inputs, b.outputs = [x], [r]
    return b.finish(), x, r, dict(host=host, tails=tails, convs=convs, shape=(H, H, C))


def requantize_concat_model(seed=0, H=8, C=64):
    """x (int8) -> LceQuantize -> two LceBconv2d (int8 out, C and 32 channels, different scales) -> QUANTIZE of the second to the
    first's scale -> CONCATENATION -> LceQuantize -> LceBconv2d (the output).  Returns (file, x, output, info)."""
    b = ModelBuilder()
    g = synth.rng(seed + 11)
    q_x, q_a, q_b = _q(g), _q(g), _q(g, 0.12, 0.3)
    x = _i8(b, H, C, "x", q_x)
    q, _ = _quantize(b, x, H, C, "0")
    ya, _ = _conv(b, q, H, C, C, seed + 1, out_type=np.int8, quant=q_a)
    yb, _ = _conv(b, q, H, C, 32, seed + 2, out_type=np.int8, quant=q_b)
    yb2 = _i8(b, H, 32, "yb_requantized", q_a)
    k_rq = b.builtin_op(QUANTIZE, [yb], [yb2])
    j = _i8(b, H, C + 32, "joined", q_a)
    k_cat = concat_op(b, [ya, yb2], [j])
    q2, _ = _quantize(b, j, H, C + 32, "1")
    out, _ = _conv(b, q2, H, C + 32, C, seed + 3, out_type=np.int8, quant=_q(g))
    b.inputs, b.outputs = [x], [out]
    host = [(k_rq, "step", [yb], yb2, (("requantize", q_a), q_b)), (k_cat, "concat", [ya, yb2], j, None)]
    return b.finish(), x, out, dict(host=host, requantize=k_rq, concat=k_cat, shape=(H, H, C))


def relu6_model(seed=0, H=8, C=64, code=RELU6_OP):
    """x (int8) -> LceQuantize -> LceBconv2d (int8 out) -> RELU6 (its own output quantization) -> LceQuantize -> LceBconv2d."""
    b = ModelBuilder()
    g = synth.rng(seed + 13)
    q_y, q_z = (0.05, -4), (0.0235, -128)
    x = _i8(b, H, C, "x", _q(g))
    q, _ = _quantize(b, x, H, C, "0")
    y, _ = _conv(b, q, H, C, C, seed + 1, out_type=np.int8, quant=q_y)
    z = _i8(b, H, C, "z", q_z)
    k = b.builtin_op(code, [y], [z])
    q2, _ = _quantize(b, z, H, C, "1")
    out, _ = _conv(b, q2, H, C, C, seed + 2, out_type=np.int8, quant=_q(g))
    b.inputs, b.outputs = [x], [out]
    act = {RELU_OP: RELU, RELU_N1_TO_1_OP: 2, RELU6_OP: RELU6}[code]
    return b.finish(), x, out, dict(host=[(k, "step", [y], z, (("clamp", q_z, act), q_y))], relu=k, shape=(H, H, C))


def host_op(kind, inputs, params):
    """The NumPy side of one builtin operator of the fixtures: `inputs` are its non-constant int8 input arrays."""
    if kind == "residual":
        q, act = params
        return E.ar.add_q(inputs[0], inputs[1], q, act)
    if kind == "step":
        st, q_in = params
        return E.apply_step(np.asarray(inputs[0]).astype(np.int64), st, q_in)[0].astype(np.int8)
    if kind == "concat":
        return np.concatenate(inputs, axis=-1)
    raise ValueError(kind)


# ---- one file per rule: x -> LceQuantize -> LceBconv2d (int8) -> y -> THE operator -> out, `case` naming what is wrong with it -------
REFUSALS = ("mul_int8", "logistic_int8", "alpha_hwc", "alpha_not_constant", "per_channel_constant", "per_channel_alpha", "uint8", "int16",
            "rank2", "add_two_tensors_no_int8_add", "add_multiplier", "zero_point_300", "two_scales_output", "quantize_from_float",
            "constant_of_other_length", "relu_overflow")
CONTROLS = ("add_c", "add_111c", "add_1", "add_scalar", "add_constant_first", "prelu_c", "prelu_11c", "prelu_111c", "prelu_1", "relu",
            "relu_n1_to_1", "relu6", "requantize")


def _set_quant(b, t, scales, zero_points):
    b.tensors[t].fields[4] = _Table({2: _Vector("f", [float(s) for s in scales]), 3: _Vector("q", [int(z) for z in zero_points])})


def single_op_model(case, seed=0, H=4, C=32):
    """Returns (file, index of the operator under test, (kind, params) for host_op or None).  A name of REFUSALS: the operator the
    predicate or its prepare step leaves with the host; a name of CONTROLS: a well-formed one, which the name takes."""
    b = ModelBuilder()
    g = synth.rng(seed + 91)
    q_y, q_o, q_k = (0.05, -3), (0.07, 4), (0.02, 1)
    x = b.tensor([1, H, H, C], np.float32, "x")
    q, _ = _quantize(b, x, H, C, "0")
    y, _ = _conv(b, q, H, C, C, seed + 1, out_type=np.int8, quant=q_y)
    inputs, ref = [x], None
    out = _i8(b, H, C, "out", q_o)
    kvals = g.integers(-128, 128, C).astype(np.int8)
    if case in ("add_c", "add_111c", "add_1", "add_scalar", "add_constant_first", "per_channel_constant", "add_multiplier", "zero_point_300",
                "two_scales_output", "uint8", "int16", "constant_of_other_length"):
        shape = {"add_111c": [1, 1, 1, C], "add_1": [1], "add_scalar": [], "constant_of_other_length": [C // 2]}.get(case, [C])
        n = int(np.prod(shape)) if shape else 1
        k = _const(b, shape or [1], "k", kvals[:n], q_k)
        if not shape:
            b.tensors[k].fields[0] = _Vector("i", [])                # (the writer takes no data for a 0-d shape: declared afterwards)
        if case == "per_channel_constant":
            _set_quant(b, k, [0.02] * C, [0] * C)
        if case == "add_multiplier":
            _set_quant(b, out, [1e-8], [0])
        if case == "zero_point_300":
            _set_quant(b, out, [q_o[0]], [300])
        if case == "two_scales_output":
            _set_quant(b, out, [q_o[0], q_o[0]], [q_o[1], q_o[1]])
        if case in ("uint8", "int16"):
            b.tensors[out].fields[1] = _Scalar("b", UINT8 if case == "uint8" else INT16)
        op = ew_op(b, ADD, [k, y] if case == "add_constant_first" else [y, k], [out], RELU)
        ref = ("step", (("add", kvals[:n] if n > 1 else np.int8(kvals[0]), q_k, q_o, RELU), q_y))
    elif case == "add_two_tensors_no_int8_add":
        other = _i8(b, H, C, "other", q_k)
        inputs.append(other)
        op = ew_op(b, ADD, [y, other], [out], NONE)
    elif case == "mul_int8":
        op = ew_op(b, MUL, [y, _const(b, [C], "k", kvals, q_k)], [out], NONE)
    elif case == "logistic_int8":
        _set_quant(b, out, [1.0 / 256], [-128])
        op = b.builtin_op(LOGISTIC, [y], [out])
    elif case in ("prelu_c", "prelu_11c", "prelu_111c", "prelu_1", "alpha_hwc", "per_channel_alpha"):
        shape = {"prelu_c": [C], "prelu_111c": [1, 1, 1, C], "prelu_1": [1], "alpha_hwc": [H, H, C]}.get(case, [1, 1, C])
        n = int(np.prod(shape))
        a = g.integers(-128, 128, n).astype(np.int8)
        alpha = _const(b, shape, "alpha", a, (0.01, 2))
        if case == "per_channel_alpha":
            _set_quant(b, alpha, [0.01] * C, [0] * C)
        op = b.builtin_op(PRELU, [y, alpha], [out])
        ref = ("step", (("prelu", a if n > 1 else np.int8(a[0]), (0.01, 2), q_o), q_y))
    elif case == "alpha_not_constant":
        alpha = b.tensor([1, 1, C], np.int8, "alpha", scale=0.01, zero_point=2)
        inputs.append(alpha)
        op = b.builtin_op(PRELU, [y, alpha], [out])
    elif case in ("relu", "relu_n1_to_1", "relu6", "relu_overflow"):
        code, act = {"relu": (RELU_OP, 1), "relu_n1_to_1": (RELU_N1_TO_1_OP, 2), "relu6": (RELU6_OP, 3), "relu_overflow": (RELU_OP, 1)}[case]
        if case == "relu_overflow":
            _set_quant(b, out, [q_y[0] * 2.0 ** -25], [0])           # (v - zi) * 2^26 leaves int32: prepare refuses
        op = b.builtin_op(code, [y], [out])
        ref = ("step", (("clamp", q_o, act), q_y))
    elif case == "requantize":
        op = b.builtin_op(QUANTIZE, [y], [out])
        ref = ("step", (("requantize", q_o), q_y))
    elif case == "quantize_from_float":
        f = b.tensor([1, H, H, C], np.float32, "f")
        inputs.append(f)
        op = b.builtin_op(QUANTIZE, [f], [out])
    elif case == "rank2":
        # a rank-2 int8 ADD: no LceBconv2d output is rank 2, so it reads a graph input
        b2 = ModelBuilder()
        v = b2.tensor([1, C], np.int8, "v", scale=q_y[0], zero_point=q_y[1])
        o2 = b2.tensor([1, C], np.int8, "out", scale=q_o[0], zero_point=q_o[1])
        op = ew_op(b2, ADD, [v, _const(b2, [C], "k", kvals, q_k)], [o2], NONE)
        b2.inputs, b2.outputs = [v], [o2]
        return b2.finish(), op, None
    else:
        raise ValueError(case)
    b.inputs, b.outputs = inputs, [out]
    return b.finish(), op, ref if case in CONTROLS else None
