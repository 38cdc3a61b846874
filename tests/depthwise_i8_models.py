"""Fixture models with a quantized builtin DEPTHWISE_CONV_2D, shared by tests/test_depthwise_i8_host.py and
tests/test_gpu_depthwise_i8.py, built with int8_conv_models.QModelBuilder: (a) an int8 QuickNet transition with the fixed blur,
(b) an int8 stem with a depthwise convolution, and (c) a whole small int8 network with a float interface -- head_i8_models'
network with (b) in front of its body and (a) behind it -- each with its host-side operators (the NumPy restatements), an oracle
closure, the partition under every earlier name and the expected counters.  No tests here."""
import numpy as np

import conv2d_i8_ref as CR
import depthwise_i8_ref as R
import head_i8_models as HM
import head_i8_ref as H
import int8_add_ref as A
import int8_conv_models as M
import oracle_lib as O
import pool_ref as PR
from depthwise_ref import BLUR
from section_models import ADD, MAX_POOL_2D, NONE, RELU, SAME, conv2d_op, depthwise_op, ew_op, pool_op

EARLIER = dict(HM.EVERY_FLAG)                                      # every name the library knew before depthwise_i8
EVERY_FLAG = dict(depthwise_i8_sections=True, **EARLIER)
BLUR_SCALE = 0.25 / 127.0
BLUR_Q = np.rint(BLUR / np.float32(BLUR_SCALE)).astype(np.int8)    # [[32 64 32] [64 127 64] [32 64 32]]


def depthwise_filter_tensor(b, w, sw, name="dw", zero_points=None, quantized_dimension=3):
    """The constant int8 filter [1, fh, fw, Cout] with its scale vector `sw` (1 or Cout scales) along dimension 3."""
    return M.filter_tensor(b, w, sw, name, zero_points, quantized_dimension)


def depthwise_constants(cout, filt, seed, q_in, q_out, per_channel):
    """Seeded int8 filter [1, fh, fw, Cout], int32 bias and filter scales whose outputs spread over the int8 range."""
    w4, bias, sw = M.conv_constants(cout, filt, 1, seed, q_in, q_out, per_channel)         # [Cout, fh, fw, 1]
    return np.ascontiguousarray(w4.transpose(3, 1, 2, 0)), bias, sw


def _i8(b, shape, name, q):
    return b.tensor(shape, np.int8, name, scale=q[0], zero_point=q[1])


def transition_part(b, x, q_x, Hx, C, seed, per_channel, tag=""):
    """Behind the int8 tensor `x` [1, Hx, Hx, C] at q_x: LceQuantize -> LceBconv2d 3x3 (C -> C, int8) -> ADD int8 (+ x, RELU) ->
    MAX_POOL_2D 2x2 / 1 SAME -> DEPTHWISE_CONV_2D 3x3 / 2 SAME (the blur, round(w / (0.25 / 127)), no bias) -> CONV_2D 1x1 int8
    (C -> 2C, + bias) -> LceQuantize -> LceBconv2d 3x3 (2C -> 2C, int8).  Returns (output tensor, its quantization, part)."""
    q_y, q_r, q_d, q_t, q_o = (0.04, 3), (0.06, -20), (0.06, -18), (0.05, -6), (0.045, 4)
    h2, c2 = (Hx + 1) // 2, 2 * C
    q0 = b.tensor([1, Hx, Hx, C // 32], np.int32, "tq0" + tag)
    k0 = b.custom_op("LceQuantize", [x], [q0], b"")
    y, cv0 = M._bconv_int8(b, q0, Hx, C, C, seed * 10 + 3, 1, q_y)
    r = _i8(b, [1, Hx, Hx, C], "r" + tag, q_r)
    add = ew_op(b, ADD, [y, x], [r], RELU)
    p = _i8(b, [1, Hx, Hx, C], "p" + tag, q_r)
    pool = pool_op(b, MAX_POOL_2D, [r], [p], (2, 2), (1, 1), SAME)
    blur = np.ascontiguousarray(np.broadcast_to(BLUR_Q[None, :, :, None], (1, 3, 3, C)))
    # (a converter writes one scale, or the same one per channel; the per-channel file varies them a little so that a channel
    # that took its neighbour's multiplier would show)
    sb = np.float32(BLUR_SCALE) * (1 + np.arange(C, dtype=np.float32) / (4 * C)) if per_channel else np.array([BLUR_SCALE], np.float32)
    d = _i8(b, [1, h2, h2, C], "d" + tag, q_d)
    dw = depthwise_op(b, [p, depthwise_filter_tensor(b, blur, sb, "blur" + tag)], [d], (2, 2), SAME)
    w, bias, sw = M.conv_constants(c2, (1, 1), C, seed + 5, q_d, q_t, per_channel)
    t = _i8(b, [1, h2, h2, c2], "t" + tag, q_t)
    conv = conv2d_op(b, [d, M.filter_tensor(b, w, sw, "w" + tag), b.tensor([c2], np.int32, "wb" + tag, bias)], [t], (1, 1), SAME)
    q1 = b.tensor([1, h2, h2, c2 // 32], np.int32, "tq1" + tag)
    k1 = b.custom_op("LceQuantize", [t], [q1], b"")
    out, cv1 = M._bconv_int8(b, q1, h2, c2, c2, seed * 10 + 4, 1, q_o)
    q_add = (q_y[0], q_y[1], q_x[0], q_x[1], q_r[0], q_r[1])
    host = {add: lambda a, c: A.add_q(a, c, q_add, A.ACT_RELU),
            pool: lambda v: PR.pool2d(v, PR.MAX, (2, 2), (1, 1), SAME, NONE, q_r[0], q_r[1]),
            dw: lambda v: R.depthwise_i8(v, blur, None, sb, q_r, q_d, (2, 2), SAME),
            conv: lambda v: CR.conv2d_i8(v, w, bias, sw, q_d, q_t, (1, 1), SAME)}

    def forward(v):
        v = host[pool](host[add](M.bconv_int8(cv0, O.bitpack(v, q_x[1])), v))
        return M.bconv_int8(cv1, O.bitpack(host[conv](host[dw](v)), q_t[1]))
    return out, q_o, dict(host=host, forward=forward, depthwise=dw, conv=conv, add=add, pool=pool, first=k0, last=k1 + 1, blur=blur, sb=sb,
                          q_in=q_r, q_out=q_d, size=h2, channels=c2)


def stem_part(b, x, q_x, Hx, seed, per_channel, tag=""):
    """Behind the int8 image `x` [1, Hx, Hx, 3] at q_x: CONV_2D 3x3 / 2 SAME int8 (3 -> 16, + bias) -> DEPTHWISE_CONV_2D 3x3 / 2 SAME
    with depth multiplier 2 (16 -> 32, seeded weights, + bias, RELU) -> CONV_2D 1x1 int8 (32 -> 64, + bias) -> LceQuantize ->
    LceBconv2d 3x3 (64 -> 64, int8).  Returns (output tensor, its quantization, part)."""
    q_c, q_d, q_t, q_y = (0.05, -9), (0.04, -128), (0.05, 7), (0.04, 2)
    h2, h4 = (Hx + 1) // 2, ((Hx + 1) // 2 + 1) // 2
    w0, b0, s0 = M.conv_constants(16, (3, 3), 3, seed + 7, q_x, q_c, per_channel)
    c = _i8(b, [1, h2, h2, 16], "c" + tag, q_c)
    conv0 = conv2d_op(b, [x, M.filter_tensor(b, w0, s0, "w0" + tag), b.tensor([16], np.int32, "b0" + tag, b0)], [c], (2, 2), SAME, NONE)
    wd, bd, sd = depthwise_constants(32, (3, 3), seed + 8, q_c, q_d, per_channel)
    bd = bd + np.int32(12000)                                        # (a RELU on a sum centred at 0 would zero half of the map)
    d = _i8(b, [1, h4, h4, 32], "sd" + tag, q_d)
    dw = depthwise_op(b, [c, depthwise_filter_tensor(b, wd, sd, "wd" + tag), b.tensor([32], np.int32, "bd" + tag, bd)], [d], (2, 2), SAME, 2, RELU)
    w1, b1, s1 = M.conv_constants(64, (1, 1), 32, seed + 9, q_d, q_t, per_channel)
    t = _i8(b, [1, h4, h4, 64], "st" + tag, q_t)
    conv1 = conv2d_op(b, [d, M.filter_tensor(b, w1, s1, "w1" + tag), b.tensor([64], np.int32, "b1" + tag, b1)], [t], (1, 1), SAME, NONE)
    q0 = b.tensor([1, h4, h4, 2], np.int32, "sq0" + tag)
    k0 = b.custom_op("LceQuantize", [t], [q0], b"")
    y, cv = M._bconv_int8(b, q0, h4, 64, 64, seed * 10 + 2, 1, q_y)
    host = {conv0: lambda v: CR.conv2d_i8(v, w0, b0, s0, q_x, q_c, (2, 2), SAME, CR.NONE),
            dw: lambda v: R.depthwise_i8(v, wd, bd, sd, q_c, q_d, (2, 2), SAME, 2, R.RELU),
            conv1: lambda v: CR.conv2d_i8(v, w1, b1, s1, q_d, q_t, (1, 1), SAME, CR.NONE)}

    def forward(v):
        return M.bconv_int8(cv, O.bitpack(host[conv1](host[dw](host[conv0](v))), q_t[1]))
    return y, q_y, dict(host=host, forward=forward, depthwise=dw, conv=conv0, conv1=conv1, last=k0 + 1, w=wd, bias=bd, sw=sd, q_in=q_c,
                        q_out=q_d, size=h4)


def transition_fixture(per_channel=True, seed=0, Hx=8, C=32):
    """(a) an int8 QuickNet transition on x int8 [1, 8, 8, 32]: 0 LceQuantize, 1 LceBconv2d, 2 ADD, 3 MAX_POOL_2D, 4 the blur,
    5 CONV_2D 1x1, 6 LceQuantize, 7 LceBconv2d.  Returns (file, input tensor, output tensor, info)."""
    b = M.QModelBuilder()
    q_x = (0.05, -4)
    x = _i8(b, [1, Hx, Hx, C], "x", q_x)
    out, _, part = transition_part(b, x, q_x, Hx, C, seed, per_channel)
    b.inputs, b.outputs = [x], [out]
    info = dict(part, shape=(Hx, Hx, C), oracle=part["forward"], ops=8, in_dtype=np.int8, out_dtype=np.int8, depthwises=[part["depthwise"]],
                plain=[[0, 1], [6, 7]], parent_sections=[[0, 1, 2, 3], [6, 7]],
                stats=dict(depthwise_i8=(1, 0), conv_i8=(1, 1), int8_add=(1, 0), pool=(1, 0)))
    return b.finish(), x, out, info


def stem_fixture(per_channel=True, seed=0, Hx=17):
    """(b) an int8 stem on x int8 [1, 17, 17, 3]: 0 CONV_2D 3x3 / 2, 1 DEPTHWISE_CONV_2D 3x3 / 2 (multiplier 2, bias, RELU),
    2 CONV_2D 1x1, 3 LceQuantize, 4 LceBconv2d.  Returns (file, input tensor, output tensor, info)."""
    b = M.QModelBuilder()
    q_x = (0.02, -128)
    x = _i8(b, [1, Hx, Hx, 3], "x", q_x)
    out, _, part = stem_part(b, x, q_x, Hx, seed, per_channel)
    b.inputs, b.outputs = [x], [out]
    info = dict(part, shape=(Hx, Hx, 3), oracle=part["forward"], ops=5, in_dtype=np.int8, out_dtype=np.int8, depthwises=[part["depthwise"]],
                plain=[[3, 4]], parent_sections=[[0], [3, 4]],
                stats=dict(depthwise_i8=(1, 0), conv_i8=(2, 1), int8_add=(0, 0), pool=(0, 0)))
    return b.finish(), x, out, info


def network_fixture(per_channel=True, seed=0, Hx=33, classes=10):
    """(c) image float32 [1, 33, 33, 3] -> 0 QUANTIZE -> the stem of (b) (1 .. 5: 17 x 17 x 16, 9 x 9 x 32, 9 x 9 x 64) -> the
    transition of (a) on 64 channels (6 .. 13: 5 x 5 x 128) -> 14 MEAN -> 15 FULLY_CONNECTED (128 -> 10) -> 16 SOFTMAX ->
    17 DEQUANTIZE -> float32 [1, 10].  Returns (file, input tensor, output tensor, info)."""
    b = M.QModelBuilder()
    q_x = (0.02, -128)
    x = b.tensor([1, Hx, Hx, 3], np.float32, "image")
    xq = _i8(b, [1, Hx, Hx, 3], "image_q", q_x)
    k_q = b.builtin_op(HM.QUANTIZE, [x], [xq])
    y, q_y, stem = stem_part(b, xq, q_x, Hx, seed, per_channel, "_s")
    z, q_z, tr = transition_part(b, y, q_y, stem["size"], 64, seed + 1, per_channel, "_t")
    out, head = HM.head_i8(b, z, q_z, tr["size"], tr["channels"], classes, seed, per_channel, q_pooled=(0.01, 3), q_logits=(0.02, 12))
    b.inputs, b.outputs = [x], [out]
    host = {k_q: lambda v: H.quantize(v, *q_x), **stem["host"], **tr["host"], **head["host"]}

    def oracle(v):
        return head["forward"](tr["forward"](stem["forward"](H.quantize(v, *q_x))))
    n = len(b.ops)
    dws = [stem["depthwise"], tr["depthwise"]]
    # under every earlier name the file is cut exactly at the two depthwise operators: what becomes ready behind a host operator
    # and is no LCE operator stays with the host until the next LceQuantize
    info = dict(shape=(Hx, Hx, 3), host=host, oracle=oracle, ops=n, head=head, in_dtype=np.float32, out_dtype=np.float32, depthwises=dws,
                parent_sections=[[0, 1], [4, 5, 6, 7, 8, 9], [12, 13, 14, 15, 16, 17]],
                stats=dict(depthwise_i8=(2, 0), conv_i8=(3, 2), int8_add=(1, 0), pool=(1, 0)))
    return b.finish(), x, out, info


FIXTURES = {"transition_per_channel": lambda: transition_fixture(True), "transition_per_tensor": lambda: transition_fixture(False),
            "stem_per_channel": lambda: stem_fixture(True), "stem_per_tensor": lambda: stem_fixture(False),
            "network_per_channel": lambda: network_fixture(True), "network_per_tensor": lambda: network_fixture(False)}
fixture_input = HM.fixture_input
