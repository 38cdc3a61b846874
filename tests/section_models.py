"""Model builders shared by the tests of the GPU sections: the operator builders on tests/tflite_writer.py, the fixture models
that more than one test file uses, the helpers that open a model through the C ABI and read its sections, and the schema's
operator, option and activation codes.  No tests here."""
import ctypes as C
import importlib
import mmap
import struct

import numpy as np

import conv1x1_ref as CR
import depthwise_ref as DR
import flexbuf
import oracle_lib as O
import pool_ref as PR
import synth
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

# schema.fbs BuiltinOperator
ADD, AVERAGE_POOL_2D, CONCATENATION, CONV_2D, DEPTHWISE_CONV_2D, MAX_POOL_2D, MUL, SUB = 0, 1, 2, 3, 4, 17, 18, 41
# schema.fbs BuiltinOptions
CONV_2D_OPTIONS, DEPTHWISE_CONV_2D_OPTIONS, POOL_2D_OPTIONS, CONCATENATION_OPTIONS, ADD_OPTIONS, MUL_OPTIONS = 1, 2, 5, 10, 11, 21
# schema.fbs ActivationFunctionType
NONE, RELU, RELU_N1_TO_1, RELU6, TANH = 0, 1, 2, 3, 4
# schema.fbs Padding
SAME, VALID = 0, 1


def bconv_options(spec: O.ConvSpec) -> bytes:
    return flexbuf.bconv2d_options(channels_in=spec.channels_in, dilation_height_factor=spec.dilation_h,
                                   dilation_width_factor=spec.dilation_w, fused_activation_function=spec.activation,
                                   pad_values=spec.pad_values, padding=spec.padding, stride_height=spec.stride_h,
                                   stride_width=spec.stride_w)


def small_model(seed=0):
    """float in -> LceQuantize -> LceBconv2d(float) -> LceQuantize -> LceBconv2d(bitpacked, RELU)
    -> LceBMaxPool2d -> LceBconv2d(int8) ; second output: LceDequantize of the pooled bits."""
    H, C0 = 12, 64
    s1 = O.ConvSpec(1, H, H, C0, 3, 3, 96, padding=O.PADDING_SAME, pad_values=1)
    s2 = O.ConvSpec(1, H, H, 96, 3, 3, 40, 1, 2, 2, 1, 1, O.PADDING_VALID, 0, O.ACT_RELU)
    oh = s2.out_h
    s3 = O.ConvSpec(1, oh // 2, oh // 2, 40, 1, 1, 33)
    _, w1, m1, b1 = synth.conv_inputs(s1, seed + 1)
    _, w2, m2, b2 = synth.conv_inputs(s2, seed + 2)
    _, w3, m3, b3 = synth.conv_inputs(s3, seed + 3)
    thr2 = O.thresholds_converter(s2, m2, b2)
    sc3, zp3 = synth.int8_quant_params(seed + 3)
    b = ModelBuilder()
    t_in = b.tensor([1, H, H, C0], np.float32, "input")
    t_q1 = b.tensor([1, H, H, 2], np.int32, "q1")
    t_w1 = b.tensor(w1.shape, np.int32, "w1", w1)
    t_m1 = b.tensor([96], np.float32, "m1", m1)
    t_b1 = b.tensor([96], np.float32, "b1", b1)
    t_y1 = b.tensor([1, H, H, 96], np.float32, "y1")
    t_q2 = b.tensor([1, H, H, 3], np.int32, "q2")
    t_w2 = b.tensor(w2.shape, np.int32, "w2", w2)
    t_t2 = b.tensor([40], np.int32, "thr2", thr2)
    t_y2 = b.tensor([1, oh, oh, 2], np.int32, "y2")
    t_p = b.tensor([1, oh // 2, oh // 2, 2], np.int32, "pooled")
    t_w3 = b.tensor(w3.shape, np.int32, "w3", w3)
    t_m3 = b.tensor([33], np.float32, "m3", m3)
    t_b3 = b.tensor([33], np.float32, "b3", b3)
    t_y3 = b.tensor([1, oh // 2, oh // 2, 33], np.int8, "y3", scale=float(sc3), zero_point=zp3)
    t_d = b.tensor([1, oh // 2, oh // 2, 40], np.float32, "dequantized")
    b.inputs, b.outputs = [t_in], [t_y3, t_d]
    b.custom_op("LceQuantize", [t_in], [t_q1], b"")
    b.custom_op("LceBconv2d", [t_q1, t_w1, t_m1, t_b1, -1], [t_y1], bconv_options(s1))
    b.custom_op("LceQuantize", [t_y1], [t_q2], b"")
    b.custom_op("LceBconv2d", [t_q2, t_w2, -1, -1, t_t2], [t_y2], bconv_options(s2))
    b.custom_op("LceBMaxPool2d", [t_y2], [t_p], flexbuf.bmaxpool_options(2, 2, 2, 2, O.PADDING_VALID))
    b.custom_op("LceBconv2d", [t_p, t_w3, t_m3, t_b3, -1], [t_y3], bconv_options(s3))
    b.custom_op("LceDequantize", [t_p], [t_d], b"")
    params = dict(s1=s1, s2=s2, s3=s3, w=(w1, w2, w3), m=(m1, m2, m3), b=(b1, b2, b3), thr2=thr2, q3=(sc3, zp3))
    return b.finish(), params


def oracle_forward(x, p):
    n = x.shape[0]
    s1, s2, s3 = (s.with_batch(n) for s in (p["s1"], p["s2"], p["s3"]))
    y1 = O.bconv2d(s1, O.DST_F32, O.bitpack(x), p["w"][0], p["m"][0], p["b"][0])
    y2 = O.bconv2d(s2, O.DST_BITPACKED, O.bitpack(y1), p["w"][1], thresholds=p["thr2"])
    pooled = O.bmaxpool(y2, 2, 2, 2, 2, O.PADDING_VALID)
    y3 = O.bconv2d(s3, O.DST_I8, pooled, p["w"][2], p["m"][2], p["b"][2], out_scale=float(p["q3"][0]),
                   out_zero_point=p["q3"][1])
    return y3, O.unpack(pooled, 40, np.float32)


def mixed_model(seed=0):
    """A QuickNet-shaped mixed graph (float stem, residual ADDs between binary convolutions, float pooling head):

        x --CONV_2D(builtin stem)--> s --LceQuantize--> q0 --LceBconv2d(float)--> y0 --ADD(s)--> r0
          r0 --LceQuantize--> q1 --LceBconv2d(float)--> y1 --ADD(r0)--> r1
          r1 --LceQuantize--> q2 --LceBconv2d(bitpacked)--> b2 --LceBMaxPool2d--> p2 --LceBconv2d(float)--> y3 --MAX_POOL_2D--> out
          b2 --LceDequantize--> d2 (second graph output)

    Binary sections: {Quantize, Bconv} (s -> y0), {Quantize, Bconv} (r0 -> y1), {Quantize, Bconv, BMaxPool, Bconv, Dequantize}
    (r1 -> y3, d2)."""
    H, C = 10, 64
    s_a = O.ConvSpec(1, H, H, C, 3, 3, C, padding=O.PADDING_SAME, pad_values=1)
    s_c = O.ConvSpec(1, H, H, C, 3, 3, 96, padding=O.PADDING_SAME, pad_values=1, activation=O.ACT_RELU)
    s_d = O.ConvSpec(1, H // 2, H // 2, 96, 3, 3, 32, padding=O.PADDING_SAME, pad_values=1)
    _, w0, m0, b0 = synth.conv_inputs(s_a, seed + 1)
    _, w1, m1, b1 = synth.conv_inputs(s_a, seed + 2)
    _, w2, m2, b2 = synth.conv_inputs(s_c, seed + 3)
    _, w3, m3, b3 = synth.conv_inputs(s_d, seed + 4)
    thr2 = O.thresholds_converter(s_c, m2, b2)
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    i32 = lambda shape, name, data=None: b.tensor(shape, np.int32, name, data)
    x = f32([1, H, H, 3], "image")
    k = f32([C, 3, 3, 3], "stem_filter", synth.rng(seed).standard_normal((C, 3, 3, 3)).astype(np.float32))
    kb = f32([C], "stem_bias", np.zeros(C, np.float32))
    s = f32([1, H, H, C], "stem")
    q0, y0, r0 = i32([1, H, H, 2], "q0"), f32([1, H, H, C], "y0"), f32([1, H, H, C], "r0")
    q1, y1, r1 = i32([1, H, H, 2], "q1"), f32([1, H, H, C], "y1"), f32([1, H, H, C], "r1")
    q2, bb2, p2 = i32([1, H, H, 2], "q2"), i32([1, H, H, 3], "b2"), i32([1, H // 2, H // 2, 3], "p2")
    y3, out, d2 = f32([1, H // 2, H // 2, 32], "y3"), f32([1, 2, 2, 32], "pooled"), f32([1, H, H, 96], "d2")
    tw = [i32(w.shape, "w%d" % i, w) for i, w in enumerate((w0, w1, w2, w3))]
    tm = [f32([len(m)], "m%d" % i, m) for i, m in enumerate((m0, m1, m2, m3))]
    tb = [f32([len(v)], "b%d" % i, v) for i, v in enumerate((b0, b1, b2, b3))]
    tthr = i32([96], "thr2", thr2)
    b.inputs, b.outputs = [x], [out, d2]
    b.builtin_op(CONV_2D, [x, k, kb], [s])                                             # 0
    b.custom_op("LceQuantize", [s], [q0], b"")                                         # 1
    b.custom_op("LceBconv2d", [q0, tw[0], tm[0], tb[0], -1], [y0], bconv_options(s_a))  # 2
    b.builtin_op(ADD, [y0, s], [r0])                                                   # 3
    b.custom_op("LceQuantize", [r0], [q1], b"")                                        # 4
    b.custom_op("LceBconv2d", [q1, tw[1], tm[1], tb[1], -1], [y1], bconv_options(s_a))  # 5
    b.builtin_op(ADD, [y1, r0], [r1])                                                  # 6
    b.custom_op("LceQuantize", [r1], [q2], b"")                                        # 7
    b.custom_op("LceBconv2d", [q2, tw[2], -1, -1, tthr], [bb2], bconv_options(s_c))     # 8
    b.custom_op("LceBMaxPool2d", [bb2], [p2], flexbuf.bmaxpool_options(2, 2, 2, 2, O.PADDING_VALID))   # 9
    b.custom_op("LceBconv2d", [p2, tw[3], tm[3], tb[3], -1], [y3], bconv_options(s_d))  # 10
    b.builtin_op(MAX_POOL_2D, [y3], [out])                                             # 11
    b.custom_op("LceDequantize", [bb2], [d2], b"")                                     # 12
    ids = dict(s=s, y0=y0, r0=r0, y1=y1, r1=r1, y3=y3, d2=d2, b2=bb2)
    params = dict(specs=(s_a, s_a, s_c, s_d), w=(w0, w1, w2, w3), m=(m0, m1, m2, m3), b=(b0, b1, b2, b3), thr2=thr2)
    return b.finish(), ids, params


def ew_op(b: ModelBuilder, code: int, inputs, outputs, activation=None) -> int:
    """A builtin operator with an AddOptions / MulOptions table (fields 3/4 of Operator) -- or none when activation is None."""
    fields = {0: _Scalar("I", b._code(None, code)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if activation is not None:
        fields[3] = _Scalar("B", MUL_OPTIONS if code == MUL else ADD_OPTIONS)
        fields[4] = _Table({0: _Scalar("b", activation)})
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


def layer(b, r_prev, H, C, cout, seed, stride=1, residual=True, act=RELU):
    """One QuickNet-style binary layer: LceQuantize -> LceBconv2d (3x3 SAME, float) -> MUL (BN) -> ADD (BN) [-> ADD residual].
    Returns (output tensor, the layer's constants)."""
    spec = O.ConvSpec(1, H, H, C, 3, 3, cout, stride_h=stride, stride_w=stride, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, seed)
    g = synth.rng(seed + 1000)
    bn_m = g.uniform(0.5, 1.5, cout).astype(np.float32)
    bn_a = g.standard_normal(cout).astype(np.float32)
    oh = spec.out_h
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    q = b.tensor([1, H, H, (C + 31) // 32], np.int32, "q%d" % seed)
    tw = b.tensor(w.shape, np.int32, "w%d" % seed, w)
    y, mm, a = f32([1, oh, oh, cout], "y%d" % seed), f32([1, oh, oh, cout], "bnm%d" % seed), f32([1, oh, oh, cout], "bna%d" % seed)
    b.custom_op("LceQuantize", [r_prev], [q], b"")
    b.custom_op("LceBconv2d", [q, tw, f32([cout], "m%d" % seed, m), f32([cout], "b%d" % seed, bias), -1], [y], bconv_options(spec))
    ew_op(b, MUL, [y, f32([cout], "bn_mul%d" % seed, bn_m)], [mm], NONE)
    if not residual:
        ew_op(b, ADD, [mm, f32([1, 1, 1, cout], "bn_add%d" % seed, bn_a.reshape(1, 1, 1, cout))], [a], act)
        return a, dict(spec=spec, w=w, m=m, b=bias, bn_m=bn_m, bn_a=bn_a, residual=False, act=act)
    ew_op(b, ADD, [mm, f32([1, 1, 1, cout], "bn_add%d" % seed, bn_a.reshape(1, 1, 1, cout))], [a], NONE)
    r = f32([1, oh, oh, cout], "r%d" % seed)
    ew_op(b, ADD, [a, r_prev], [r], act)
    return r, dict(spec=spec, w=w, m=m, b=bias, bn_m=bn_m, bn_a=bn_a, residual=True, act=act)


# the QuickNet body the GPU tests and tools/elementwise_sections.py use: (H, C, Cout, stride, residual) per layer
BODY = ((56, 64, 64, 1, True), (56, 64, 64, 1, True), (56, 64, 128, 2, False), (28, 128, 128, 1, True),
        (28, 128, 256, 2, False), (14, 256, 256, 1, True))


def body_model(layers=BODY, seed=0):
    """x (float [1,H,W,C]) -> the layers -> the last layer's float output (graph output).  Returns (file, x, output, layer list,
    the tensor each layer's chain writes)."""
    b = ModelBuilder()
    H, C = layers[0][0], layers[0][1]
    x = b.tensor([1, H, H, C], np.float32, "x")
    r, info, outs = x, [], []
    for k, (h, c, cout, stride, residual) in enumerate(layers):
        r, li = layer(b, r, h, c, cout, seed + 10 * k + 1, stride, residual, RELU if k % 2 else NONE)
        info.append(li)
        outs.append(r)
    b.inputs, b.outputs = [x], [r]
    return b.finish(), x, r, info, outs


def concat_op(b: ModelBuilder, inputs, outputs, axis=3, activation=NONE) -> int:
    """A builtin CONCATENATION with its ConcatenationOptions table (0 axis, 1 fused_activation_function) -- or without one
    when axis is None."""
    fields = {0: _Scalar("I", b._code(None, CONCATENATION)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if axis is not None:
        fields[3] = _Scalar("B", CONCATENATION_OPTIONS)
        fields[4] = _Table({0: _Scalar("i", axis), 1: _Scalar("b", activation)})
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


def _conv(b, src_bits, H, C, cout, seed, stride=1, out_type=np.float32, quant=None, k=3):
    """LceBconv2d (k x k SAME, one-padding) on the bitpacked tensor `src_bits`; returns (output tensor, its constants)."""
    spec = O.ConvSpec(1, H, H, C, k, k, cout, stride_h=stride, stride_w=stride, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, seed)
    if quant is not None:
        m = (m * np.float32(0.05)).astype(np.float32)
    oh = spec.out_h
    kw = {} if quant is None else dict(scale=quant[0], zero_point=quant[1])
    y = b.tensor([1, oh, oh, cout], out_type, "y%d" % seed, **kw)
    f32 = lambda shape, name, data: b.tensor(shape, np.float32, name, data)
    b.custom_op("LceBconv2d", [src_bits, b.tensor(w.shape, np.int32, "w%d" % seed, w), f32([cout], "m%d" % seed, m),
                               f32([cout], "b%d" % seed, bias), -1], [y], bconv_options(spec))
    return y, dict(spec=spec, w=w, m=m, b=bias, y=y)


# growth per dense layer of the two stages (a tuple: several convolutions of one layer, joined at once); 10 is ragged
DENSE_STAGES = ((64, 10, (32, 32)), (64, 32, 64))


def dense_block_model(H=16, C0=64, stages=DENSE_STAGES, transition=128, seed=0):
    """x (float [1,H,H,C0]) -> LceQuantize -> LceBconv2d -> y0, then per dense layer
         x -> MUL (bn) -> ADD (bn) -> LceQuantize -> LceBconv2d (3x3, C -> G, float) [x n] -> CONCATENATION([x, y...]) -> x'
    at two resolutions with a stride-2 binary layer (LceQuantize -> LceBconv2d) between them; the last x' is the graph output.
    Returns (file, input tensor, output tensor, steps): steps is the program in order -- dicts with kind "conv" (the leading
    and the stride-2 layer), or "dense" (bn_m, bn_a, mul / add / join: operator indices, convs, out: joined tensor)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x0 = f32([1, H, H, C0], "x")
    steps = []
    n = [seed * 100]

    def binary_layer(src, h, c, cout, stride):
        n[0] += 1
        q = b.tensor([1, h, h, (c + 31) // 32], np.int32, "q%d" % n[0])
        b.custom_op("LceQuantize", [src], [q], b"")
        y, info = _conv(b, q, h, c, cout, n[0], stride)
        steps.append(dict(kind="conv", **info))
        return y

    x, h, c = binary_layer(x0, H, C0, C0, 1), H, C0
    for s, growths in enumerate(stages):
        if s:
            x, h, c = binary_layer(x, h, c, transition, 2), h // 2, transition
        for growth in growths:
            n[0] += 1
            g = synth.rng(n[0] + 1000)
            bn_m = g.uniform(0.5, 1.5, c).astype(np.float32)
            bn_a = g.standard_normal(c).astype(np.float32)
            mm, a = f32([1, h, h, c], "bnm%d" % n[0]), f32([1, h, h, c], "bna%d" % n[0])
            mul = ew_op(b, MUL, [x, f32([c], "bn_mul%d" % n[0], bn_m)], [mm], NONE)
            add = ew_op(b, ADD, [mm, f32([1, 1, 1, c], "bn_add%d" % n[0], bn_a.reshape(1, 1, 1, c))], [a], NONE)
            q = b.tensor([1, h, h, (c + 31) // 32], np.int32, "q%d" % n[0])
            b.custom_op("LceQuantize", [a], [q], b"")
            convs = []
            for j, cout in enumerate(growth if isinstance(growth, tuple) else (growth,)):
                n[0] += 1
                convs.append(_conv(b, q, h, c, cout, n[0], k=3 if j == 0 else 1)[1])
            c2 = c + sum(cv["spec"].channels_out for cv in convs)
            out = f32([1, h, h, c2], "x%d" % n[0])
            join = concat_op(b, [x] + [cv["y"] for cv in convs], [out], axis=3 if len(steps) % 2 else -1)
            steps.append(dict(kind="dense", bn_m=bn_m, bn_a=bn_a, convs=convs, join=join, out=out, x=x, mul=mul, add=add))
            x, c = out, c2
    b.inputs, b.outputs = [x0], [x]
    return b.finish(), x0, x, steps


def joins_of(steps):
    return [s["join"] for s in steps if s["kind"] == "dense"]


def cut_at(n_ops, cuts):
    """Operator runs between the operators `cuts`: the partition of a chain-like graph whose only foreign operators they are."""
    want, cur = [], []
    for i in range(n_ops):
        if i in cuts:
            want.append(cur)
            cur = []
        else:
            cur.append(i)
    return [s for s in want + [cur] if s]


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def _sections_of(handle):
    lib = mr.tflite_lib()
    out = []
    for i in range(lib.lce_tflite_model_num_sections(handle)):
        info = mr._SectionInfo()
        assert lib.lce_tflite_model_section(handle, i, C.byref(info)) == amd.OK
        s = mr.Section(info)
        out.append((s.ops, s.inputs, s.outputs))
    return out


def pool_op(b: ModelBuilder, code, inputs, outputs, filt=(2, 2), stride=(2, 2), padding=VALID, activation=NONE, options=True) -> int:
    """A builtin pool with its Pool2DOptions table (0 padding, 1 stride_w, 2 stride_h, 3 filter_width, 4 filter_height,
    5 fused_activation_function) -- or without one when options is False."""
    fields = {0: _Scalar("I", b._code(None, code)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if options:
        fields[3] = _Scalar("B", POOL_2D_OPTIONS)
        fields[4] = _Table({0: _Scalar("b", padding), 1: _Scalar("i", stride[1]), 2: _Scalar("i", stride[0]),
                            3: _Scalar("i", filt[1]), 4: _Scalar("i", filt[0]), 5: _Scalar("b", activation)})
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


# ---- the partition ------------------------------------------------------------------------------------------------------------
def alexnet_body_model(H=15, C=64, seed=0):
    """x (float) -> LceQuantize -> LceBconv2d (float) -> MAX_POOL 3x3 / 2 VALID -> MUL (c) -> ADD (c) -> LceQuantize ->
    LceBconv2d (float) -> AVERAGE_POOL 2x2 / 2 SAME -> LceQuantize -> LceBconv2d (float, the graph output).  Returns (file,
    input tensor, output tensor, info): info holds the convolutions' constants, the batch norm and the operator indices."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    quant = lambda src, h, name: b.tensor([1, h, h, C // 32], np.int32, name)
    x = f32([1, H, H, C], "x")
    q0 = quant(x, H, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y0, c0 = _conv(b, q0, H, C, C, seed * 10 + 1)
    h1 = (H - 3) // 2 + 1
    p0 = f32([1, h1, h1, C], "p0")
    pool0 = pool_op(b, MAX_POOL_2D, [y0], [p0], (3, 3), (2, 2), VALID)
    g = synth.rng(seed + 77)
    bn_m, bn_a = g.uniform(-1.5, 1.5, C).astype(np.float32), g.standard_normal(C).astype(np.float32)
    mm, aa = f32([1, h1, h1, C], "mm"), f32([1, h1, h1, C], "aa")
    mul = ew_op(b, MUL, [p0, f32([C], "bn_m", bn_m)], [mm], NONE)
    add = ew_op(b, ADD, [mm, f32([C], "bn_a", bn_a)], [aa], NONE)
    q1 = quant(aa, h1, "q1")
    b.custom_op("LceQuantize", [aa], [q1], b"")
    y1, c1 = _conv(b, q1, h1, C, C, seed * 10 + 2)
    h2 = (h1 + 1) // 2
    p1 = f32([1, h2, h2, C], "p1")
    pool1 = pool_op(b, AVERAGE_POOL_2D, [y1], [p1], (2, 2), (2, 2), SAME, RELU6)
    q2 = quant(p1, h2, "q2")
    b.custom_op("LceQuantize", [p1], [q2], b"")
    y2, c2 = _conv(b, q2, h2, C, C, seed * 10 + 3)
    b.inputs, b.outputs = [x], [y2]
    info = dict(convs=[c0, c1, c2], bn_m=bn_m, bn_a=bn_a, pools=[pool0, pool1], mul=mul, add=add, pooled=[p0, p1], sizes=[H, h1, h2],
                channels=C)
    return b.finish(), x, y2, info


MARK = 0x5A6B7C4D


def _options_table(data):
    """(position of the Pool2DOptions table whose filter_height is MARK, position of the uoffset that points to it, position of
    the vtable slot of filter_height)."""
    at = data.index(struct.pack("<i", MARK))
    assert data.count(struct.pack("<i", MARK)) == 1
    for table in range(at - 4, max(0, at - 64), -4):                                  # the table start: its vtable names `at`
        vt = table - struct.unpack_from("<i", data, table)[0]
        if 0 <= vt < table and vt + 14 <= len(data) and struct.unpack_from("<H", data, vt)[0] == 16 and \
                table + struct.unpack_from("<H", data, vt + 4 + 2 * 4)[0] == at:
            refs = [p for p in range(0, table, 4) if p + struct.unpack_from("<I", data, p)[0] == table]
            assert len(refs) == 1
            return table, refs[0], vt + 4 + 2 * 4
    raise AssertionError("options table not found")


# ---- the opt-in -----------------------------------------------------------------------------------------------------------------
def _open(data, raw):
    """lce_tflite_model_open_opts on the options bytes `raw`, placed so that they END at a page that cannot be read: a read
    beyond them faults.  Returns (handle or None, message)."""
    page = mmap.PAGESIZE
    m = mmap.mmap(-1, 2 * page)
    view = (C.c_char * (2 * page)).from_buffer(m)
    base = C.addressof(view)
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    at = base + page - len(raw)
    C.memmove(at, raw, len(raw))
    assert libc.mprotect(base + page, page, 0) == 0, C.get_errno()
    try:
        err = C.create_string_buffer(128)
        h = mr.tflite_lib().lce_tflite_model_open_opts(data, len(data), C.c_void_p(at), err, 128)
    finally:
        assert libc.mprotect(base + page, page, mmap.PROT_READ | mmap.PROT_WRITE) == 0
        del view
        m.close()
    return h, err.value


def conv2d_op(b: ModelBuilder, inputs, outputs, stride=(1, 1), padding=SAME, activation=NONE, dilation=(1, 1), options=True,
              code=CONV_2D) -> int:
    """A builtin CONV_2D with its Conv2DOptions table (0 padding, 1 stride_w, 2 stride_h, 3 fused_activation_function,
    4 dilation_w_factor, 5 dilation_h_factor) -- without the dilations when dilation is None (the schema's default 1 holds), or
    without a table when options is False.  stride and dilation are (height, width)."""
    fields = {0: _Scalar("I", b._code(None, code)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if options:
        t = {0: _Scalar("b", padding), 1: _Scalar("i", stride[1]), 2: _Scalar("i", stride[0]), 3: _Scalar("b", activation)}
        if dilation is not None:
            t[4], t[5] = _Scalar("i", dilation[1]), _Scalar("i", dilation[0])
        fields[3] = _Scalar("B", CONV_2D_OPTIONS)
        fields[4] = _Table(t)
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


# ---- the fixtures of the GPU side -----------------------------------------------------------------------------------------------
F32_SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x80000001,
                        0x007FFFFF, 0x807FFFFF], np.uint32).view(np.float32)   # +-0, +-inf, NaNs, smallest / largest subnormals


def float_fixture(shape, seed, special=False):
    """Mixed-magnitude normals (products and sums round at every step).  `special`: every third pixel scaled into the
    subnormals (subnormal inputs and results), +-0 and subnormals planted everywhere, +-inf and NaN in every third pixel."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(shape) * g.choice([1e-3, 1.0, 3.0, 1e4], shape)).astype(np.float32)
    if special:
        rows = x.reshape(-1, shape[-1])
        rows[1::3] *= np.float32(1e-41)
        k = max(1, rows.size // 9)
        r, c = g.integers(0, rows.shape[0], k), g.integers(0, shape[-1], k)
        v = F32_SPECIAL[g.integers(0, F32_SPECIAL.size, k)]
        keep = (r % 3 == 0) | np.isfinite(v)
        rows[r[keep], c[keep]] = v[keep]
    return x


def bireal_block_model(H=8, C=64, seed=0):
    """A Bi-RealNet-style downsampling block.  x (float) -> LceQuantize -> LceBconv2d (float) -> r;
    main: r -> LceQuantize -> LceBconv2d 3x3 / 2 (C -> 2C) -> MUL (c) -> ADD (c) -> aa;
    shortcut: r -> AVERAGE_POOL_2D 2x2 / 2 -> CONV_2D 1x1 (C -> 2C) + bias -> s;
    ADD (aa, s) -> LceQuantize -> LceBconv2d (float, the graph output).  Returns (file, input tensor, output tensor, info)."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 301)
    h2, c2 = H // 2, 2 * C
    x = f32([1, H, H, C], "x")
    q0 = b.tensor([1, H, H, C // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    r, c0 = _conv(b, q0, H, C, C, seed * 10 + 1)
    q1 = b.tensor([1, H, H, C // 32], np.int32, "q1")
    b.custom_op("LceQuantize", [r], [q1], b"")
    y1, c1 = _conv(b, q1, H, C, c2, seed * 10 + 2, stride=2)
    bn_m, bn_a = g.uniform(-1.5, 1.5, c2).astype(np.float32), g.standard_normal(c2).astype(np.float32)
    mm, aa = f32([1, h2, h2, c2], "mm"), f32([1, h2, h2, c2], "aa")
    mul = ew_op(b, MUL, [y1, f32([c2], "bn_m", bn_m)], [mm], NONE)
    add = ew_op(b, ADD, [mm, f32([c2], "bn_a", bn_a)], [aa], NONE)
    p = f32([1, h2, h2, C], "p")
    pool = pool_op(b, AVERAGE_POOL_2D, [r], [p], (2, 2), (2, 2), VALID)
    w = (g.standard_normal((c2, 1, 1, C)) * 0.2).astype(np.float32)
    wb = (g.standard_normal(c2) * 8).astype(np.float32)
    s = f32([1, h2, h2, c2], "s")
    conv = conv2d_op(b, [p, f32([c2, 1, 1, C], "w", w), f32([c2], "wb", wb)], [s], (1, 1), SAME)
    rr = f32([1, h2, h2, c2], "rr")
    join = ew_op(b, ADD, [aa, s], [rr], NONE)
    q2 = b.tensor([1, h2, h2, c2 // 32], np.int32, "q2")
    b.custom_op("LceQuantize", [rr], [q2], b"")
    y2, c3 = _conv(b, q2, h2, c2, c2, seed * 10 + 3)
    b.inputs, b.outputs = [x], [y2]
    info = dict(convs=[c0, c1, c3], bn_m=bn_m, bn_a=bn_a, mul=mul, add=add, pools=[pool], conv1x1=conv, join=join, w=w, wb=wb,
                tensors=dict(r=r, p=p, s=s, aa=aa, rr=rr), size=H, channels=C)
    return b.finish(), x, y2, info


def depthwise_op(b: ModelBuilder, inputs, outputs, stride=(1, 1), padding=SAME, multiplier=1, activation=NONE, dilation=(1, 1),
                 options=True, code=DEPTHWISE_CONV_2D) -> int:
    """A builtin DEPTHWISE_CONV_2D with its DepthwiseConv2DOptions table (0 padding, 1 stride_w, 2 stride_h, 3 depth_multiplier,
    4 fused_activation_function, 5 dilation_w_factor, 6 dilation_h_factor) -- without the dilations when dilation is None (the
    schema's default 1 holds), or without a table when options is False.  stride and dilation are (height, width)."""
    fields = {0: _Scalar("I", b._code(None, code)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if options:
        t = {0: _Scalar("b", padding), 1: _Scalar("i", stride[1]), 2: _Scalar("i", stride[0]), 3: _Scalar("i", multiplier),
             4: _Scalar("b", activation)}
        if dilation is not None:
            t[5], t[6] = _Scalar("i", dilation[1]), _Scalar("i", dilation[0])
        fields[3] = _Scalar("B", DEPTHWISE_CONV_2D_OPTIONS)
        fields[4] = _Table(t)
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


def float_op(v, op, operand, act):
    """TFLite's float MUL / ADD: one rounding, then the clamp (std::max / std::min: a NaN passes)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return DR.clamp((v * operand if op == MUL else v + operand).astype(np.float32), act)


# ---- the fixtures of the GPU side -----------------------------------------------------------------------------------------------
def quicknet_transition_model(H=8, C=32, seed=0):
    """A QuickNet residual layer and the transition behind it.  x (float) -> LceQuantize -> LceBconv2d (3x3, float) -> MUL (c)
    -> ADD (c) -> ADD (x, RELU) -> MAX_POOL_2D 2x2 / 1 SAME -> DEPTHWISE_CONV_2D 3x3 / 2 SAME (the blur [1 2 1] x [1 2 1] / 16,
    no bias) -> CONV_2D 1x1 (C -> 2C, with bias: the folded batch norm) -> LceQuantize -> LceBconv2d (3x3, float) -> MUL (c) ->
    ADD (c), the graph output.  This layer order is QuickNet's as remembered (its transition: ReLU, max pool, blur pool, pointwise
    convolution, batch norm); larq_zoo was not available to check it against.  Returns (file, input tensor, output tensor, info);
    info["host"]: operator index -> what the host computes for it from its non-constant inputs."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 501)
    h2, c2 = H // 2, 2 * C
    x = f32([1, H, H, C], "x")
    q0 = b.tensor([1, H, H, (C + 31) // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y0, c0 = _conv(b, q0, H, C, C, seed * 10 + 1)
    bn_m, bn_a = g.uniform(0.5, 1.5, C).astype(np.float32), g.standard_normal(C).astype(np.float32)
    mm, aa, r = f32([1, H, H, C], "mm"), f32([1, H, H, C], "aa"), f32([1, H, H, C], "r")
    mul = ew_op(b, MUL, [y0, f32([C], "bn_m", bn_m)], [mm], NONE)
    add = ew_op(b, ADD, [mm, f32([C], "bn_a", bn_a)], [aa], NONE)
    res = ew_op(b, ADD, [aa, x], [r], RELU)
    p = f32([1, H, H, C], "p")
    pool = pool_op(b, MAX_POOL_2D, [r], [p], (2, 2), (1, 1), SAME)
    blur = np.ascontiguousarray(np.broadcast_to(DR.BLUR[None, :, :, None], (1, 3, 3, C)))
    d = f32([1, h2, h2, C], "d")
    dw = depthwise_op(b, [p, f32([1, 3, 3, C], "blur", blur)], [d], (2, 2), SAME)
    w = (g.standard_normal((c2, 1, 1, C)) * 0.2).astype(np.float32)
    wb = (g.standard_normal(c2) * 2).astype(np.float32)
    t = f32([1, h2, h2, c2], "t")
    conv = conv2d_op(b, [d, f32([c2, 1, 1, C], "w", w), f32([c2], "wb", wb)], [t], (1, 1), SAME)
    q1 = b.tensor([1, h2, h2, c2 // 32], np.int32, "q1")
    b.custom_op("LceQuantize", [t], [q1], b"")
    y1, c1 = _conv(b, q1, h2, c2, c2, seed * 10 + 2)
    bn_m2, bn_a2 = g.uniform(0.5, 1.5, c2).astype(np.float32), g.standard_normal(c2).astype(np.float32)
    mm2, out = f32([1, h2, h2, c2], "mm2"), f32([1, h2, h2, c2], "out")
    mul2 = ew_op(b, MUL, [y1, f32([c2], "bn_m2", bn_m2)], [mm2], NONE)
    add2 = ew_op(b, ADD, [mm2, f32([c2], "bn_a2", bn_a2)], [out], NONE)
    b.inputs, b.outputs = [x], [out]
    host = {mul: lambda v: float_op(v, MUL, bn_m, NONE), add: lambda v: float_op(v, ADD, bn_a, NONE),
            res: lambda a, s: float_op(a, ADD, s, RELU), pool: lambda v: PR.pool2d(v, PR.MAX, (2, 2), (1, 1), PR.SAME),
            dw: lambda v: DR.depthwise(v, blur, None, (2, 2), SAME), conv: lambda v: CR.conv1x1(v, w, wb),
            mul2: lambda v: float_op(v, MUL, bn_m2, NONE), add2: lambda v: float_op(v, ADD, bn_a2, NONE)}
    info = dict(depthwise=dw, conv1x1=conv, host=host, tensors=dict(r=r, p=p, d=d, t=t), size=H, channels=C, convs=[c0, c1],
                follows=[conv], w=w, wb=wb)
    return b.finish(), x, out, info
