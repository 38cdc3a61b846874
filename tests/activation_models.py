"""Builders for the standalone activations, RESHAPE and the per-image gate on tests/tflite_writer.py, the three fixture networks
of their tests -- a ReActNet-style pair of blocks, a RealToBinary-style gated block, a head that flattens -- with their restated
references, and one file per refusal of the three predicates.  No tests here."""
import numpy as np

import activation_ref as AR
import head_models as HM
import head_ref as HR
import oracle_lib as O
import synth
from section_models import ADD, MUL, NONE, RELU, _conv, ew_op
from tflite_writer import ModelBuilder

# schema.fbs BuiltinOperator
LOGISTIC, RELU_OP, RELU_N1_TO_1_OP, RELU6_OP, RESHAPE, TANH_OP, PRELU = 14, 19, 20, 21, 22, 28, 54
ACTIVATION_CODES = dict(LOGISTIC=14, RELU=19, RELU_N1_TO_1=20, RELU6=21, RESHAPE=22, PRELU=54)

OLD_NAMES = ("elementwise", "int8_add", "concat", "pool", "conv1x1", "depthwise", "conv2d", "stem", "head", "conv2d_i8", "head_i8",
             "quantize", "depthwise_i8")
NEW_NAMES = ("activation", "reshape", "gate")
OLD_KEYWORDS = dict(int8_add_sections=True, concat_sections=True, conv2d_i8_sections=True, head_i8_sections=True, quantize_sections=True,
                    depthwise_i8_sections=True, **HM.EVERY_FLAG)
NEW_KEYWORDS = dict(activation_sections=True, reshape_sections=True, gate_sections=True)


def _quantize(b, src, H, C, tag):
    q = b.tensor([1, H, H, (C + 31) // 32], np.int32, "q" + tag)
    k = b.custom_op("LceQuantize", [src], [q], b"")
    return q, k


def reactnet_model(seed=0, H=8, C=64, blocks=2):
    """x [1,H,H,C] -> per block: LceQuantize, LceBconv2d 3x3 (float), MUL and ADD (batch norm), ADD (the shortcut), ADD (shift),
    PRELU (alpha [1,1,C]), ADD (shift) -> the next block.  Returns (file, x, output, info): info["blocks"] holds each block's
    constants and operator indices, info["kinds"] what partition_ref calls each operator under the OLD names."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, H, H, C], "x")
    r, infos, kinds = x, [], []
    for n in range(blocks):
        g = synth.rng(seed + 50 * n + 7)
        q, kq = _quantize(b, r, H, C, str(n))
        y, ci = _conv(b, q, H, C, C, seed + 10 * n + 1)
        consts = dict(bn_m=g.uniform(0.5, 1.5, C), bn_a=g.standard_normal(C), shift1=g.standard_normal(C) * 0.5,
                      alpha=g.uniform(-0.5, 1.5, C), shift2=g.standard_normal(C) * 0.5)
        consts = {k: v.astype(np.float32) for k, v in consts.items()}
        t = [f32([1, H, H, C], "t%d_%d" % (n, k)) for k in range(6)]
        ops = [ew_op(b, MUL, [y, f32([C], "bn_m%d" % n, consts["bn_m"])], [t[0]], NONE),
               ew_op(b, ADD, [t[0], f32([C], "bn_a%d" % n, consts["bn_a"])], [t[1]], NONE),
               ew_op(b, ADD, [t[1], r], [t[2]], NONE),
               ew_op(b, ADD, [t[2], f32([C], "shift1_%d" % n, consts["shift1"])], [t[3]], NONE),
               b.builtin_op(PRELU, [t[3], f32([1, 1, C], "alpha%d" % n, consts["alpha"].reshape(1, 1, C))], [t[4]]),
               ew_op(b, ADD, [t[4], f32([C], "shift2_%d" % n, consts["shift2"])], [t[5]], NONE)]
        kinds += ["LceQuantize", "LceBconv2d", "elementwise", "elementwise", "elementwise", "elementwise", None, "elementwise"]
        infos.append(dict(conv=ci, quantize=kq, ops=ops, tensors=t, **consts))
        r = t[5]
    b.inputs, b.outputs = [x], [r]
    return b.finish(), x, r, dict(blocks=infos, kinds=kinds, shape=(H, H, C))


def reactnet_forward(x, info):
    v = np.asarray(x, np.float32)
    for bi in info["blocks"]:
        ci = bi["conv"]
        y = O.bconv2d(ci["spec"].with_batch(v.shape[0]), O.DST_F32, O.bitpack(v), ci["w"], ci["m"], ci["b"])
        v = AR.chain(y, [(AR.MUL, bi["bn_m"], NONE), (AR.ADD, bi["bn_a"], NONE), (AR.ADD, v, NONE), (AR.ADD, bi["shift1"], NONE),
                         (AR.PRELU, bi["alpha"], NONE), (AR.ADD, bi["shift2"], NONE)])
    return v


def gated_model(seed=0, H=8, C=64, hidden=8):
    """A RealToBinary-style block: x [1,H,H,C] -> LceQuantize -> LceBconv2d (float) -> y;  y -> MEAN keep_dims -> FULLY_CONNECTED
    (RELU, C -> hidden) -> FULLY_CONNECTED (hidden -> C) -> LOGISTIC -> RESHAPE [1,1,1,C] -> g;  MUL(y, g) -> ADD(x) -> out.
    Returns (file, x, output, info)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 333)
    x = f32([1, H, H, C], "x")
    q, kq = _quantize(b, x, H, C, "0")
    y, ci = _conv(b, q, H, C, C, seed + 1)
    w1, b1 = (g.standard_normal((hidden, C)) * 0.2).astype(np.float32), g.standard_normal(hidden).astype(np.float32)
    w2, b2 = (g.standard_normal((C, hidden)) * 0.5).astype(np.float32), g.standard_normal(C).astype(np.float32)
    pooled, h1, h2 = f32([1, 1, 1, C], "pooled"), f32([1, hidden], "h1"), f32([1, C], "h2")
    s, gate, m, out = f32([1, C], "sigmoid"), f32([1, 1, 1, C], "gate"), f32([1, H, H, C], "scaled"), f32([1, H, H, C], "out")
    k_mean = HM.mean_op(b, [y, b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [pooled], keep_dims=True)
    k_fc1 = HM.fc_op(b, [pooled, f32([hidden, C], "w1", w1), f32([hidden], "b1", b1)], [h1], RELU)
    k_fc2 = HM.fc_op(b, [h1, f32([C, hidden], "w2", w2), f32([C], "b2", b2)], [h2], NONE)
    k_log = b.builtin_op(LOGISTIC, [h2], [s])
    k_rs = b.builtin_op(RESHAPE, [s, b.tensor([4], np.int32, "gate_shape", np.array([1, 1, 1, C], np.int32))], [gate])
    k_mul = ew_op(b, MUL, [y, gate], [m], NONE)
    k_add = ew_op(b, ADD, [m, x], [out], NONE)
    b.inputs, b.outputs = [x], [out]
    kinds = ["LceQuantize", "LceBconv2d", "mean", "fully_connected", "fully_connected", None, None, None, "elementwise"]
    return b.finish(), x, out, dict(conv=ci, w1=w1, b1=b1, w2=w2, b2=b2, kinds=kinds, shape=(H, H, C),
                                    ops=dict(mean=k_mean, fc1=k_fc1, fc2=k_fc2, logistic=k_log, reshape=k_rs, mul=k_mul, add=k_add))


def gated_forward(x, info):
    x = np.asarray(x, np.float32)
    ci = info["conv"]
    y = O.bconv2d(ci["spec"].with_batch(x.shape[0]), O.DST_F32, O.bitpack(x), ci["w"], ci["m"], ci["b"])
    pooled = HR.mean_hw(y)
    h2 = HR.fully_connected(HR.fully_connected(pooled, info["w1"], info["b1"], HR.RELU), info["w2"], info["b2"])
    gate = AR.logistic(h2).reshape(x.shape[0], 1, 1, -1)
    return AR.chain(y, [(AR.MUL, gate, NONE), (AR.ADD, x, NONE)])


def flatten_head_model(seed=0, H=4, C=32, classes=10, deliver_flat=False):
    """x [1,H,H,C] -> LceQuantize -> LceBconv2d (float) -> RESHAPE [1, H*H*C] -> FULLY_CONNECTED -> SOFTMAX: a head that flattens
    instead of pooling.  `deliver_flat`: the flattened tensor is a graph output too (the RESHAPE then costs a copy).  Returns (file,
    x, outputs, info)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 444)
    K = H * H * C
    x = f32([1, H, H, C], "x")
    q, kq = _quantize(b, x, H, C, "0")
    y, ci = _conv(b, q, H, C, C, seed + 1)
    w, wb = (g.standard_normal((classes, K)) * 0.05).astype(np.float32), g.standard_normal(classes).astype(np.float32)
    flat, logits, probs = f32([1, K], "flat"), f32([1, classes], "logits"), f32([1, classes], "probabilities")
    k_rs = b.builtin_op(RESHAPE, [y, b.tensor([2], np.int32, "flat_shape", np.array([-1, K], np.int32))], [flat])
    k_fc = HM.fc_op(b, [flat, f32([classes, K], "dense_w", w), f32([classes], "dense_b", wb)], [logits], NONE)
    k_sm = HM.softmax_op(b, [logits], [probs], 1.0)
    b.inputs, b.outputs = [x], [probs] + ([flat] if deliver_flat else [])
    kinds = ["LceQuantize", "LceBconv2d", None, "fully_connected", "softmax"]
    return b.finish(), x, list(b.outputs), dict(conv=ci, w=w, wb=wb, kinds=kinds, shape=(H, H, C), flat=flat,
                                                ops=dict(reshape=k_rs, fc=k_fc, softmax=k_sm))


def flatten_head_forward(x, info):
    """(probabilities, the flattened map)"""
    x = np.asarray(x, np.float32)
    ci = info["conv"]
    y = O.bconv2d(ci["spec"].with_batch(x.shape[0]), O.DST_F32, O.bitpack(x), ci["w"], ci["m"], ci["b"])
    flat = y.reshape(x.shape[0], -1)
    return HR.softmax(HR.fully_connected(flat, info["w"], info["wb"])), flat


def graph_of(data_model):
    """(ops, constants, outputs) of an mr.LceModel in partition_ref's plain lists."""
    ops = [(list(o.inputs), list(o.outputs)) for o in data_model.operators]
    constants = {i for i, t in enumerate(data_model.tensors) if t.constant}
    return ops, constants, set(data_model.outputs)


# ---- one file per refusal: x -> LceQuantize -> LceBconv2d -> y -> THE operator -> out, `case` naming what is wrong with it ---------
REFUSALS = ("alpha_hwc", "prelu_int8", "logistic_int8", "reshape_folds_batch", "reshape_dynamic_shape", "gate_rank2_operand", "add_rank2")
CONTROLS = ("prelu", "logistic", "reshape", "gate")


def single_op_model(case, seed=0, H=4, C=32):
    """Returns (file, index of the operator under test).  A name of REFUSALS: the operator no predicate takes; a name of CONTROLS: its
    well-formed twin, which the new names do take."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 91)
    x = f32([1, H, H, C], "x")
    q, _ = _quantize(b, x, H, C, "0")
    int8 = case.endswith("_int8")
    y, _ = _conv(b, q, H, C, C, seed + 1, **(dict(out_type=np.int8, quant=(0.05, -3)) if int8 else {}))
    inputs = [x]
    if case in ("alpha_hwc", "prelu", "prelu_int8"):
        shape = [H, H, C] if case == "alpha_hwc" else [1, 1, C]
        kw = dict(scale=0.05, zero_point=-3) if int8 else {}
        out = b.tensor([1, H, H, C], np.int8 if int8 else np.float32, "out", **kw)
        alpha = (b.tensor(shape, np.int8, "alpha", g.integers(-100, 100, shape).astype(np.int8), scale=0.01, zero_point=0) if int8
                 else f32(shape, "alpha", g.uniform(-1, 1, shape).astype(np.float32)))
        k = b.builtin_op(PRELU, [y, alpha], [out])
    elif case in ("logistic", "logistic_int8"):
        out = b.tensor([1, H, H, C], np.int8, "out", scale=1.0 / 256, zero_point=-128) if int8 else f32([1, H, H, C], "out")
        k = b.builtin_op(LOGISTIC, [y], [out])
    elif case in ("reshape", "reshape_folds_batch", "reshape_dynamic_shape"):
        shape = [H, H * C] if case == "reshape_folds_batch" else [1, H * H * C]
        out = f32(shape, "out")
        if case == "reshape_dynamic_shape":
            shape_t = b.tensor([2], np.int32, "shape")               # no data: computed at run time
            inputs.append(shape_t)
        else:
            shape_t = b.tensor([2], np.int32, "shape", np.array(shape, np.int32))
        k = b.builtin_op(RESHAPE, [y, shape_t], [out])
    elif case in ("gate", "gate_rank2_operand"):
        gate = f32([1, C] if case == "gate_rank2_operand" else [1, 1, 1, C], "gate")
        inputs.append(gate)
        out = f32([1, H, H, C], "out")
        k = ew_op(b, MUL, [y, gate], [out], NONE)
    elif case == "add_rank2":
        pooled, out = f32([1, C], "pooled"), f32([1, C], "out")
        HM.mean_op(b, [y, b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [pooled])
        k = ew_op(b, ADD, [pooled, f32([C], "bias", g.standard_normal(C).astype(np.float32))], [out], NONE)
    else:
        raise ValueError(case)
    b.inputs, b.outputs = inputs, [out]
    return b.finish(), k
