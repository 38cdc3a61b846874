"""Builders for the classifier head on tests/tflite_writer.py -- MEAN, FULLY_CONNECTED and SOFTMAX with their options tables, as
section_models.pool_op writes Pool2DOptions -- and the fixture models of the head tests with their restated references.  No tests
here."""
import numpy as np

import conv2d_ref as KR
import head_ref as HR
import oracle_lib as O
import synth
from section_models import ADD, MUL, NONE, RELU, SAME, conv2d_op, float_op, layer
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

# schema.fbs BuiltinOperator / BuiltinOptions
FULLY_CONNECTED, SOFTMAX, MEAN, TANH_OP = 9, 25, 40, 28
FULLY_CONNECTED_OPTIONS, SOFTMAX_OPTIONS, REDUCER_OPTIONS = 8, 9, 27

ALL_FLAGS = dict(elementwise_sections=True, pool_sections=True, conv1x1_sections=True, depthwise_sections=True,
                 conv2d_sections=True, stem_sections=True)
EVERY_FLAG = dict(head_sections=True, **ALL_FLAGS)


def _op(b, code, inputs, outputs, options_type=None, table=None):
    fields = {0: _Scalar("I", b._code(None, code)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if table is not None:
        fields[3] = _Scalar("B", options_type)
        fields[4] = _Table(table)
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


def mean_op(b: ModelBuilder, inputs, outputs, keep_dims=False, options=True) -> int:
    """A builtin MEAN with its ReducerOptions table (0 keep_dims) -- or without one when options is False."""
    return _op(b, MEAN, inputs, outputs, REDUCER_OPTIONS, {0: _Scalar("B", 1 if keep_dims else 0)} if options else None)


def fc_op(b: ModelBuilder, inputs, outputs, activation=NONE, weights_format=0, keep_num_dims=False, options=True) -> int:
    """A builtin FULLY_CONNECTED with its FullyConnectedOptions table (0 fused_activation_function, 1 weights_format,
    2 keep_num_dims) -- or without one when options is False."""
    table = {0: _Scalar("b", activation), 1: _Scalar("b", weights_format), 2: _Scalar("B", 1 if keep_num_dims else 0)}
    return _op(b, FULLY_CONNECTED, inputs, outputs, FULLY_CONNECTED_OPTIONS, table if options else None)


def softmax_op(b: ModelBuilder, inputs, outputs, beta=1.0, options=True) -> int:
    """A builtin SOFTMAX with its SoftmaxOptions table (0 beta) -- or without one when options is False."""
    return _op(b, SOFTMAX, inputs, outputs, SOFTMAX_OPTIONS, {0: _Scalar("f", beta)} if options else None)


def head(b, src, hw, c, classes, seed, keep_dims=False, beta=1.0, activation=NONE, bias=True, axis=(1, 2)):
    """MEAN over `axis` -> FULLY_CONNECTED (c -> classes) -> SOFTMAX behind the 4-D tensor `src` [1, hw, hw, c].  Returns (the
    probabilities' tensor, info)."""
    g = synth.rng(seed + 901)
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    w = (g.standard_normal((classes, c)) * 0.3).astype(np.float32)
    wb = g.standard_normal(classes).astype(np.float32) if bias else None
    t_axis = b.tensor([len(axis)], np.int32, "axis", np.array(axis, np.int32))
    pooled = f32([1, 1, 1, c] if keep_dims else [1, c], "pooled")
    k_mean = mean_op(b, [src, t_axis], [pooled], keep_dims)
    logits, probs = f32([1, classes], "logits"), f32([1, classes], "probabilities")
    ins = [pooled, f32([classes, c], "dense_w", w)] + ([f32([classes], "dense_b", wb)] if bias else [])
    k_fc = fc_op(b, ins, [logits], activation)
    k_sm = softmax_op(b, [logits], [probs], beta)
    return probs, dict(mean=k_mean, fc=k_fc, softmax=k_sm, w=w, wb=wb, beta=beta, activation=activation, keep_dims=keep_dims,
                       tensors=dict(pooled=pooled, logits=logits, probs=probs), classes=classes)


def head_forward(v, hi):
    """The restated head on the float32 map `v` [B, H, W, C]."""
    pooled = HR.mean_hw(v)
    return HR.softmax(HR.fully_connected(pooled, hi["w"], hi["wb"], hi["activation"]), hi["beta"])


def quicknet_head_model(seed=0, keep_dims=False, H=8, classes=10):
    """A QuickNet-shaped network: x [1, H, H, 3] -> CONV_2D 3x3 SAME RELU (3 -> 32, bias: the stem) -> a binary layer 32 -> 32 with
    batch norm and the residual ADD -> a binary layer 32 -> 64 / 2 with batch norm and RELU -> MEAN -> FULLY_CONNECTED (64 ->
    classes, bias) -> SOFTMAX.  Returns (file, input tensor, output tensor, info)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 801)
    x = f32([1, H, H, 3], "image")
    w0 = (g.standard_normal((32, 3, 3, 3)) * 0.5).astype(np.float32)
    b0 = g.standard_normal(32).astype(np.float32)
    s = f32([1, H, H, 32], "stem")
    k0 = conv2d_op(b, [x, f32([32, 3, 3, 3], "stem_w", w0), f32([32], "stem_b", b0)], [s], (1, 1), SAME, RELU)
    r1, l1 = layer(b, s, H, 32, 32, seed + 11, 1, True, NONE)
    r2, l2 = layer(b, r1, H, 32, 64, seed + 21, 2, False, RELU)
    probs, hi = head(b, r2, H // 2, 64, classes, seed, keep_dims)
    b.inputs, b.outputs = [x], [probs]
    info = dict(stem=k0, w0=w0, b0=b0, layers=[l1, l2], head=hi, shape=(H, H, 3), body_out=r2, classes=classes)
    return b.finish(), x, probs, info


def body_forward(x, info):
    """The restated stem and body of quicknet_head_model: the float map that feeds the head."""
    v = KR.conv2d(x, info["w0"], info["b0"], (1, 1), KR.SAME, KR.RELU)
    for li in info["layers"]:
        y = O.bconv2d(li["spec"].with_batch(x.shape[0]), O.DST_F32, O.bitpack(v), li["w"], li["m"], li["b"])
        t = float_op(y, MUL, li["bn_m"], NONE)
        if li["residual"]:
            t = float_op(float_op(t, ADD, li["bn_a"].reshape(1, 1, 1, -1), NONE), ADD, v, li["act"])
        else:
            t = float_op(t, ADD, li["bn_a"].reshape(1, 1, 1, -1), li["act"])
        v = t
    return v


def quicknet_forward(x, info):
    return head_forward(body_forward(x, info), info["head"])


def head_only_model(seed=0, H=5, C=40, classes=7):
    """x [1, H, H, C] -> TANH (an operator of the host: no pass takes it) -> MEAN -> FULLY_CONNECTED -> SOFTMAX: the head is a
    section of its own, which starts at the MEAN.  Returns (file, input tensor, output tensor, info)."""
    b = ModelBuilder()
    x = b.tensor([1, H, H, C], np.float32, "x")
    t = b.tensor([1, H, H, C], np.float32, "t")
    k = b.builtin_op(TANH_OP, [x], [t])
    probs, hi = head(b, t, H, C, classes, seed, activation=RELU, beta=0.5)
    b.inputs, b.outputs = [x], [probs]
    return b.finish(), x, probs, dict(tanh=k, t=t, head=hi, shape=(H, H, C))
