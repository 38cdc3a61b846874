"""Fixture models of the int8 classifier head and the float / int8 boundary, shared by tests/test_head_i8_host.py and
tests/test_gpu_head_i8.py, built with int8_conv_models.QModelBuilder and the head's option tables of tests/head_models.py: (a) a
head alone -- MEAN -> FULLY_CONNECTED -> SOFTMAX -> DEQUANTIZE on an int8 map -- and (b) a whole small int8 network with a float
interface, each with its host-side operators (the NumPy restatements of tests/head_i8_ref.py) and an oracle closure.  No tests
here."""
import numpy as np

import conv2d_i8_ref as R
import head_i8_ref as H
import int8_conv_models as M
import oracle_lib as O
from head_models import fc_op, mean_op, softmax_op
from section_models import NONE, SAME, conv2d_op

QUANTIZE, DEQUANTIZE = 114, 6              # schema.fbs BuiltinOperator
Q_PROBS = H.SOFTMAX_OUT
EVERY_FLAG = dict(head_i8_sections=True, quantize_sections=True, **M.ALL_FLAGS)


def head_i8(b, src, q_src, hw, c, classes, seed, per_channel=True, keep_dims=False, beta=1.0, activation=NONE, bias=True,
            q_pooled=(0.021, 3), q_logits=(0.11, 12), q_probs=Q_PROBS, weight_zero_points=None, dequantize=True):
    """MEAN -> FULLY_CONNECTED (c -> classes) -> SOFTMAX (-> DEQUANTIZE) behind the int8 tensor `src` [1, hw, hw, c] at `q_src`.
    Returns (the last tensor, info)."""
    i8 = lambda shape, name, q: b.tensor(shape, np.int8, name, scale=q[0], zero_point=q[1])
    w4, wb, sw = M.conv_constants(classes, (1, 1), c, seed + 31, q_pooled, q_logits, per_channel)
    w = w4.reshape(classes, c)
    wb = wb if bias else None
    t_axis = b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))
    pooled = i8([1, 1, 1, c] if keep_dims else [1, c], "pooled", q_pooled)
    k_mean = mean_op(b, [src, t_axis], [pooled], keep_dims)
    logits, probs = i8([1, classes], "logits", q_logits), i8([1, classes], "probabilities", q_probs)
    zps = [0] * np.atleast_1d(sw).size if weight_zero_points is None else weight_zero_points
    ins = [pooled, b.qtensor(w.shape, np.int8, "dense_w", w, np.atleast_1d(sw), zps, 0)]
    ins += [b.tensor([classes], np.int32, "dense_b", wb)] if bias else []
    k_fc = fc_op(b, ins, [logits], activation)
    k_sm = softmax_op(b, [logits], [probs], beta)
    host = {k_mean: lambda v: H.mean_i8(v, q_src, q_pooled).reshape((v.shape[0], 1, 1, c) if keep_dims else (v.shape[0], c)),
            k_fc: lambda v: H.fully_connected_i8(v.reshape(v.shape[0], c), w, wb, sw, q_pooled, q_logits, activation),
            k_sm: lambda v: H.softmax_i8(v, q_logits[0], beta)}
    last, k_dq = probs, None
    if dequantize:
        last = b.tensor([1, classes], np.float32, "scores")
        k_dq = b.builtin_op(DEQUANTIZE, [probs], [last])
        host[k_dq] = lambda v: H.dequantize(v, *q_probs)

    def forward(v):
        for k in (k_mean, k_fc, k_sm) + ((k_dq,) if dequantize else ()):
            v = host[k](v)
        return v
    return last, dict(mean=k_mean, fc=k_fc, softmax=k_sm, dequantize=k_dq, host=host, forward=forward, w=w, wb=wb, sw=sw, q_src=q_src,
                      q_pooled=q_pooled, q_logits=q_logits, beta=beta, classes=classes, tensors=dict(pooled=pooled, logits=logits, probs=probs))


def head_only_fixture(per_channel=True, seed=0, H_=5, C=40, classes=7, **kw):
    """(a) x int8 [1, 5, 5, 40] -> MEAN -> FULLY_CONNECTED (40 -> 7, RELU-free) -> SOFTMAX (beta 0.5) -> DEQUANTIZE: every operator
    is the new passes'.  Returns (file, input tensor, output tensor, info)."""
    b = M.QModelBuilder()
    q_x = (0.05, -4)
    x = b.tensor([1, H_, H_, C], np.int8, "x", scale=q_x[0], zero_point=q_x[1])
    out, hi = head_i8(b, x, q_x, H_, C, classes, seed, per_channel, beta=kw.pop("beta", 0.5), **kw)
    b.inputs, b.outputs = [x], [out]
    info = dict(shape=(H_, H_, C), head=hi, host=hi["host"], oracle=hi["forward"], ops=4 if hi["dequantize"] is not None else 3,
                in_dtype=np.int8, out_dtype=np.float32 if hi["dequantize"] is not None else np.int8)
    return b.finish(), x, out, info


def network_fixture(per_channel=True, seed=0, H_=17, cout=64, classes=10, float_interface=True):
    """(b) image float32 [1, 17, 17, 3] -> 0 QUANTIZE -> 1 CONV_2D 3x3 / 2 SAME int8 (3 -> 64, + bias; no activation, so that the signs the binary layer reads depend on the image) -> 2 LceQuantize ->
    3 LceBconv2d 3x3 (64 -> 64, int8) -> 4 MEAN -> 5 FULLY_CONNECTED (64 -> 10) -> 6 SOFTMAX -> 7 DEQUANTIZE -> float32 [1, 10].
    With float_interface False the QUANTIZE and the DEQUANTIZE are left out: int8 in, int8 out.  Returns (file, input tensor,
    output tensor, info)."""
    b = M.QModelBuilder()
    q_x, q_c, q_y = (0.02, -128), (0.05, -9), (0.04, 2)
    h2 = (H_ + 1) // 2
    host = {}
    xq = None
    if float_interface:
        x = b.tensor([1, H_, H_, 3], np.float32, "image")
        xq = b.tensor([1, H_, H_, 3], np.int8, "image_q", scale=q_x[0], zero_point=q_x[1])
        k_q = b.builtin_op(QUANTIZE, [x], [xq])
        host[k_q] = lambda v: H.quantize(v, *q_x)
    else:
        x = xq = b.tensor([1, H_, H_, 3], np.int8, "image_q", scale=q_x[0], zero_point=q_x[1])
    w, bias, sw = M.conv_constants(cout, (3, 3), 3, seed + 7, q_x, q_c, per_channel)
    c = b.tensor([1, h2, h2, cout], np.int8, "c", scale=q_c[0], zero_point=q_c[1])
    conv = conv2d_op(b, [xq, M.filter_tensor(b, w, sw), b.tensor([cout], np.int32, "wb", bias)], [c], (2, 2), SAME, NONE)
    host[conv] = lambda v: R.conv2d_i8(v, w, bias, sw, q_x, q_c, (2, 2), SAME, R.NONE)
    q0 = b.tensor([1, h2, h2, cout // 32], np.int32, "q0")
    k_lq = b.custom_op("LceQuantize", [c], [q0], b"")
    y, cv = M._bconv_int8(b, q0, h2, cout, cout, seed * 10 + 2, 1, q_y)
    out, hi = head_i8(b, y, q_y, h2, cout, classes, seed, per_channel, dequantize=float_interface, q_pooled=(0.01, 3), q_logits=(0.02, 12))
    host.update(hi["host"])
    b.inputs, b.outputs = [x], [out]

    def oracle(v):
        if float_interface:
            v = H.quantize(v, *q_x)
        return hi["forward"](M.bconv_int8(cv, O.bitpack(host[conv](v), q_c[1])))
    n_ops = len(b.ops)
    info = dict(shape=(H_, H_, 3), conv=conv, head=hi, host=host, oracle=oracle, ops=n_ops, body=[k_lq, k_lq + 1],
                in_dtype=np.float32 if float_interface else np.int8, out_dtype=np.float32 if float_interface else np.int8, q_x=q_x,
                body_out=y)
    return b.finish(), x, out, info


FIXTURES = {"head_per_channel": lambda: head_only_fixture(True), "head_per_tensor": lambda: head_only_fixture(False),
            "network_per_channel": lambda: network_fixture(True), "network_per_tensor": lambda: network_fixture(False),
            "network_int8_interface": lambda: network_fixture(True, float_interface=False)}


def fixture_input(info, batch, seed=0):
    """A seeded input batch of the fixture: int8 over the whole range, or float images in [0, 5) (0.02 x 255 = 5.1 is the
    QUANTIZE's range)."""
    g = np.random.default_rng(seed + 77)
    if info["in_dtype"] == np.int8:
        return g.integers(-128, 128, (batch,) + info["shape"], dtype=np.int64).astype(np.int8)
    return (g.uniform(-0.2, 5.3, (batch,) + info["shape"])).astype(np.float32)
