"""Fixtures of the int8 squeeze-and-excite gate in the model reader ("gate_i8" of lce_tflite_model_open_passes), built with
int8_conv_models.QModelBuilder: a RealToBinary-style int8 body of gated blocks with its NumPy forward (the oracle's LceBconv2d,
tests/head_i8_ref.py, tests/int8_add_ref.py, tests/gate_i8_ref.py), and one file per rule of the two predicates.  No tests here."""
import numpy as np

import gate_i8_ref as G
import head_i8_ref as H8
import int8_add_ref as ar
import int8_conv_models as M
import oracle_lib as O
import synth
from activation_models import LOGISTIC, RESHAPE, _quantize
from elementwise_i8_models import INT16, UINT8, _const, _i8, _set_quant
from head_models import fc_op, mean_op
from section_models import ADD, MUL, NONE, RELU, RELU6, ew_op
from tflite_writer import _Scalar

NAMES = "head_i8,reshape,int8_add,gate_i8"
Q_GATE = G.LOGISTIC_OUT


def realtobinary_i8_model(seed=0, H=8, C=64, hidden=8, blocks=2, act=NONE, add_act=NONE, side_reader=False):
    """x (int8 [1,H,H,C]) -> per block: LceQuantize, LceBconv2d 3x3 (int8 out) -> y;  MEAN(y) [1,C] -> FULLY_CONNECTED (RELU,
    C -> hidden) -> FULLY_CONNECTED (hidden -> C) -> LOGISTIC [1,C] -> RESHAPE [1,1,1,C] -> gate;  MUL(y, gate) -> ADD(product,
    block input) -> the next block (whose LceQuantize reads the sum).  Returns (file, x, output, info); info["blocks"] holds each
    block's operator indices, tensors and constants.  `side_reader`: every product is also read by a second ADD (product + block
    input -> a graph output of its own), so that no MUL's product has a single reader (the NumPy forward does not cover it)."""
    b = M.QModelBuilder()
    g = synth.rng(seed + 17)
    sides = []
    q_r = (0.05, -4)
    x = _i8(b, H, C, "x", q_r)
    r, infos = x, []
    i8 = lambda shape, name, q: b.tensor(shape, np.int8, name, scale=q[0], zero_point=q[1])
    for n in range(blocks):
        q, kq = _quantize(b, r, H, C, str(n))
        q_y = (float(np.float32(g.uniform(0.03, 0.06))), int(g.integers(-10, 11)))
        y, cv = M._bconv_int8(b, q, H, C, C, seed * 10 + n + 1, 1, q_y)
        q_pool, q_h1, q_h2 = (float(np.float32(q_y[0] / 2)), int(g.integers(-5, 6))), (0.02, -128), (0.03, int(g.integers(-10, 11)))
        w1, b1, sw1 = M.conv_constants(hidden, (1, 1), C, seed + 31 + n, q_pool, q_h1, True)
        w2, b2, sw2 = M.conv_constants(C, (1, 1), hidden, seed + 41 + n, q_h1, q_h2, True)
        w1, w2 = w1.reshape(hidden, C), w2.reshape(C, hidden)
        pooled, h1, h2 = i8([1, C], "pooled%d" % n, q_pool), i8([1, hidden], "h1_%d" % n, q_h1), i8([1, C], "h2_%d" % n, q_h2)
        s, gate = i8([1, C], "sigmoid%d" % n, Q_GATE), i8([1, 1, 1, C], "gate%d" % n, Q_GATE)
        q_m = (float(np.float32(q_y[0] * g.uniform(0.6, 0.9))), int(g.integers(-10, 11)))
        q_o = (float(np.float32((q_m[0] + q_r[0]) * g.uniform(0.7, 1.0))), int(g.integers(-10, 11)))
        m, out = _i8(b, H, C, "scaled%d" % n, q_m), _i8(b, H, C, "sum%d" % n, q_o)
        k_mean = mean_op(b, [y, b.tensor([2], np.int32, "axis%d" % n, np.array([1, 2], np.int32))], [pooled], False)
        k_fc1 = fc_op(b, [pooled, b.qtensor(w1.shape, np.int8, "w1_%d" % n, w1, np.atleast_1d(sw1), [0] * np.atleast_1d(sw1).size, 0),
                          b.tensor([hidden], np.int32, "b1_%d" % n, b1)], [h1], RELU)
        k_fc2 = fc_op(b, [h1, b.qtensor(w2.shape, np.int8, "w2_%d" % n, w2, np.atleast_1d(sw2), [0] * np.atleast_1d(sw2).size, 0),
                          b.tensor([C], np.int32, "b2_%d" % n, b2)], [h2], NONE)
        k_log = b.builtin_op(LOGISTIC, [h2], [s])
        k_rs = b.builtin_op(RESHAPE, [s, b.tensor([4], np.int32, "gate_shape%d" % n, np.array([1, 1, 1, C], np.int32))], [gate])
        # (the gate stands in slot 0 in the second block, and the product in the ADD's slot 1)
        k_mul = ew_op(b, MUL, [y, gate] if n % 2 == 0 else [gate, y], [m], act)
        k_add = ew_op(b, ADD, [m, r] if n % 2 == 0 else [r, m], [out], add_act)
        k_side = None
        if side_reader:
            sides.append(_i8(b, H, C, "side%d" % n, q_o))
            k_side = ew_op(b, ADD, [m, r], [sides[-1]], NONE)
        infos.append(dict(side=k_side, quantize=kq, conv=kq + 1, cv=cv, mean=k_mean, fc1=k_fc1, fc2=k_fc2, logistic=k_log, reshape=k_rs, mul=k_mul, add=k_add,
                          w1=w1, b1=b1, sw1=sw1, w2=w2, b2=b2, sw2=sw2, q_in=q_r, q_y=q_y, q_pool=q_pool, q_h1=q_h1, q_h2=q_h2, q_m=q_m,
                          q_o=q_o, act=act, add_act=add_act,
                          tensors=dict(y=y, pooled=pooled, h1=h1, h2=h2, sigmoid=s, gate=gate, product=m, sum=out)))
        r, q_r = out, q_o
    b.inputs, b.outputs = [x], [r] + sides
    return b.finish(), x, r, dict(blocks=infos, shape=(H, H, C))


def realtobinary_i8_forward(x, info):
    """The NumPy forward of realtobinary_i8_model on x int8 [batch, H, H, C]; returns (output, {tensor: array} of every block)."""
    v = np.asarray(x, np.int8)
    vals = {}
    for bi in info["blocks"]:
        n, C = v.shape[0], v.shape[-1]
        y = M.bconv_int8(bi["cv"], O.bitpack(v, bi["q_in"][1]))
        pooled = H8.mean_i8(y, bi["q_y"], bi["q_pool"]).reshape(n, C)
        h1 = H8.fully_connected_i8(pooled, bi["w1"], bi["b1"], bi["sw1"], bi["q_pool"], bi["q_h1"], RELU)
        h2 = H8.fully_connected_i8(h1, bi["w2"], bi["b2"], bi["sw2"], bi["q_h1"], bi["q_h2"], NONE)
        gate = G.logistic_q(h2, bi["q_h2"])
        rows = y.shape[1] * y.shape[2]
        out = G.mul_add_q(y.reshape(n * rows, C), gate, v.reshape(n * rows, C), bi["q_y"], Q_GATE, bi["q_m"], bi["act"], bi["q_in"],
                          bi["q_o"], bi["add_act"], rows).reshape(y.shape)
        t = bi["tensors"]
        vals.update({t["y"]: y, t["pooled"]: pooled, t["h2"]: h2, t["sigmoid"]: gate, t["sum"]: out})
        v = out
    return v, vals


# ---- one file per rule: x -> LceQuantize -> LceBconv2d (int8) -> y -> THE operator -> out, `case` naming it ---------------------------
CONTROLS = ("mul_tensor", "mul_gate_slot1", "mul_gate_slot0", "mul_relu", "mul_relu_n1_to_1", "mul_relu6", "logistic_rank4", "logistic_rank2")
REFUSALS = ("mul_constant", "mul_bc_operand", "mul_per_channel_input", "mul_uint8", "mul_zero_point_300", "mul_overflow",
            "logistic_other_output", "logistic_uint8", "logistic_zero_point_300", "logistic_per_channel_input")


def single_op_model(case, seed=0, H=4, C=32):
    """Returns (file, index of the operator under test, graph inputs, ref): ref(values of the graph inputs behind x ..., y) is
    the operator's NumPy result for a name of CONTROLS, None for a name of REFUSALS (what the predicates or their prepare steps
    leave with the host)."""
    b = M.QModelBuilder()
    g = synth.rng(seed + 23)
    q_y, q_o, q_g = (0.05, -3), (0.04, 4), Q_GATE
    x = b.tensor([1, H, H, C], np.float32, "x")
    q, _ = _quantize(b, x, H, C, "0")
    y, _ = M._bconv_int8(b, q, H, C, C, seed + 1, 1, q_y)
    inputs, ref = [x], None
    if case.startswith("mul"):
        out = _i8(b, H, C, "out", q_o)
        act = {"mul_relu": RELU, "mul_relu_n1_to_1": 2, "mul_relu6": RELU6}.get(case, NONE)
        if case == "mul_constant":
            other = _const(b, [C], "k", g.integers(-128, 128, C).astype(np.int8), q_g)
        elif case == "mul_tensor":
            other = _i8(b, H, C, "other", q_g)
        elif case == "mul_bc_operand":
            other = b.tensor([1, C], np.int8, "other", scale=q_g[0], zero_point=q_g[1])
        else:
            other = b.tensor([1, 1, 1, C], np.int8, "gate", scale=q_g[0], zero_point=q_g[1])
        if case != "mul_constant":
            inputs.append(other)
        if case == "mul_per_channel_input":
            _set_quant(b, other, [q_g[0]] * C, [q_g[1]] * C)
        if case == "mul_uint8":
            b.tensors[out].fields[1] = _Scalar("b", UINT8)
        if case == "mul_zero_point_300":
            _set_quant(b, out, [q_o[0]], [300])
        if case == "mul_overflow":
            _set_quant(b, out, [1e-9], [0])                          # the products times 2^18 leave int32: prepare refuses
        op = ew_op(b, MUL, [other, y] if case == "mul_gate_slot0" else [y, other], [out], act)
        if case in CONTROLS:
            rpi = 0 if case == "mul_tensor" else H * H
            ref = lambda o, yv: G.mul_q(yv.reshape(-1, C), o.reshape(-1, C), q_y, q_g, q_o, act, rpi).reshape(yv.shape)
    elif case == "logistic_rank2":
        # no LceBconv2d output is rank 2: the LOGISTIC reads the [1, C] MEAN of y (head_i8 takes the MEAN)
        pooled = b.tensor([1, C], np.int8, "pooled", scale=q_y[0], zero_point=q_y[1])
        mean_op(b, [y, b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [pooled], False)
        out = b.tensor([1, C], np.int8, "out", scale=q_g[0], zero_point=q_g[1])
        op = b.builtin_op(LOGISTIC, [pooled], [out])
        ref = lambda yv: G.logistic_q(H8.mean_i8(yv, q_y, q_y).reshape(yv.shape[0], C), q_y)
    else:
        out = _i8(b, H, C, "out", q_g)
        if case == "logistic_other_output":
            _set_quant(b, out, [1.0 / 128], [-128])
        if case == "logistic_uint8":
            b.tensors[out].fields[1] = _Scalar("b", UINT8)
        if case == "logistic_zero_point_300":
            _set_quant(b, out, [q_g[0]], [300])
        if case == "logistic_per_channel_input":
            _set_quant(b, y, [q_y[0]] * C, [q_y[1]] * C)
        op = b.builtin_op(LOGISTIC, [y], [out])
        if case in CONTROLS:
            ref = lambda yv: G.logistic_q(yv, q_y)
    b.inputs, b.outputs = inputs, [out]
    assert (ref is not None) == (case in CONTROLS), case
    return b.finish(), op, inputs, ref
