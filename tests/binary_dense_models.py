"""Builders for networks with binarized Dense layers on tests/tflite_writer.py -- the graph the converter leaves of larq's
QuantDense behind a sign: LceQuantize -> LceDequantize -> a float FULLY_CONNECTED whose row o holds only +-s[o] -- with a NumPy
forward pass for each (tests/binary_dense_ref.py, tests/head_ref.py), and one file per refusal of the predicate.  No tests
here."""
import numpy as np

import binary_dense_ref as R
import head_models as HM
import head_ref as HR
import oracle_lib as O
import synth
from activation_models import RESHAPE, TANH_OP
from section_models import NONE, RELU, _conv
from tflite_writer import ModelBuilder

KEYWORDS = dict(reshape_sections=True, binary_dense_sections=True)
KEYWORDS_HEAD = dict(head_sections=True, **KEYWORDS)


def dense_weights(g, k, n, scales="mixed", bias=True):
    """(+-s weights float32 [n, k], s [n], bias [n] or None).  `scales`: "pow2" (exact powers of two), "mixed" (any float)."""
    sign = 1 - 2 * g.integers(0, 2, (n, k))
    if scales == "pow2":
        s = np.exp2(g.integers(-6, 3, n)).astype(np.float32)
    else:
        s = g.uniform(0.01, 0.2, n).astype(np.float32)
    w = (sign * s[:, None]).astype(np.float32)
    return w, s, (g.standard_normal(n).astype(np.float32) if bias else None)


def _sign_pair(b, src, k, tag, rank4=False, dq_type=np.float32, dq_quant=None):
    """src (float [1, k] or [1, 1, 1, k]) -> LceQuantize -> LceDequantize; returns (bits tensor, dequantized tensor, op indices)."""
    lead = [1, 1, 1] if rank4 else [1]
    q = b.tensor(lead + [R.words_of(k)], np.int32, "bits" + tag)
    kw = {} if dq_quant is None else dict(scale=dq_quant[0], zero_point=dq_quant[1])
    d = b.tensor(lead + [k], dq_type, "sign" + tag, **kw)
    kq = b.custom_op("LceQuantize", [src], [q], b"")
    kd = b.custom_op("LceDequantize", [q], [d], b"")
    return q, d, (kq, kd)


def _dense(b, src, w, bias, activation, tag):
    n, k = w.shape
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    out = f32([1, n], "dense" + tag)
    ins = [src, f32([n, k], "w" + tag, w)] + ([f32([n], "b" + tag, bias)] if bias is not None else [])
    return out, HM.fc_op(b, ins, [out], activation)


def _tail(b, src, widths, classes, seed, scales="mixed", first_act=RELU):
    """Behind the float tensor `src` [1, widths[0]]: per hidden width LceQuantize -> LceDequantize -> FC(+-s, bias; the first with
    `first_act`), then the same into `classes`, then SOFTMAX.  Returns (probabilities' tensor, info).  (Behind a RELU every sign
    is +1 -- a clamped value is +0.0, whose bit must be 0 --, so the layers after it see one constant input; body_tail_model
    has no activation there and its deeper layers depend on the image.)"""
    g = synth.rng(seed + 1201)
    layers, cur = [], src
    sizes = list(widths) + [classes]
    for n, (k, nout) in enumerate(zip(sizes[:-1], sizes[1:])):
        w, s, wb = dense_weights(g, k, nout, scales)
        q, d, (kq, kd) = _sign_pair(b, cur, k, str(n))
        act = first_act if n == 0 else NONE
        out, kf = _dense(b, d, w, wb, act, str(n))
        layers.append(dict(w=w, s=s, wb=wb, act=act, k=k, n=nout, bits=q, sign=d, out=out, quantize=kq, dequantize=kd, fc=kf))
        cur = out
    probs = b.tensor([1, classes], np.float32, "probabilities")
    ksm = HM.softmax_op(b, [cur], [probs], 1.0)
    return probs, dict(layers=layers, softmax=ksm, logits=cur, probs=probs)


def tail_forward(flat, info):
    """(logits, probabilities, per-layer outputs) of the tail on the float [B, K] input."""
    v, outs = np.asarray(flat, np.float32), []
    for L in info["layers"]:
        wb, s = R.prepare(L["w"])
        v, _ = R.binary_fully_connected(bits_of(v), wb, s, L["wb"], L["k"], L["act"])
        outs.append(v)
    return v, HR.softmax(v), outs


def alexnet_tail_model(seed=0, H=3, C=20, widths=(70, 33), classes=10, scales="mixed"):
    """A BinaryAlexNet-style tail: float image [1, H, H, C] -> RESHAPE [1, H*H*C] -> LceQuantize -> LceDequantize -> FC(+-s, bias,
    RELU) -> LceQuantize -> LceDequantize -> FC -> LceQuantize -> LceDequantize -> FC -> SOFTMAX.  Returns (file, x, outputs, info)."""
    b = ModelBuilder()
    K = H * H * C
    x = b.tensor([1, H, H, C], np.float32, "image")
    flat = b.tensor([1, K], np.float32, "flat")
    k_rs = b.builtin_op(RESHAPE, [x, b.tensor([2], np.int32, "flat_shape", np.array([-1, K], np.int32))], [flat])
    probs, info = _tail(b, flat, (K,) + tuple(widths), classes, seed, scales)
    b.inputs, b.outputs = [x], [probs]
    info.update(reshape=k_rs, flat=flat, shape=(H, H, C), body=None)
    return b.finish(), x, [probs], info


def body_tail_model(seed=0, H=4, C=32, widths=(40,), classes=10):
    """The same tail (its first Dense layer without the RELU) behind a small LceBconv2d body: x [1, H, H, C] -> LceQuantize -> LceBconv2d 3x3 (float) -> RESHAPE -> the
    tail.  Returns (file, x, outputs, info)."""
    b = ModelBuilder()
    K = H * H * C
    x = b.tensor([1, H, H, C], np.float32, "x")
    q0 = b.tensor([1, H, H, R.words_of(C)], np.int32, "q_body")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y, ci = _conv(b, q0, H, C, C, seed + 1)
    flat = b.tensor([1, K], np.float32, "flat")
    k_rs = b.builtin_op(RESHAPE, [y, b.tensor([2], np.int32, "flat_shape", np.array([-1, K], np.int32))], [flat])
    probs, info = _tail(b, flat, (K,) + tuple(widths), classes, seed + 5, first_act=NONE)
    b.inputs, b.outputs = [x], [probs]
    info.update(reshape=k_rs, flat=flat, shape=(H, H, C), body=ci)
    return b.finish(), x, [probs], info


def flat_of(x, info):
    """The float [B, K] tensor that feeds the tail of alexnet_tail_model / body_tail_model."""
    x = np.asarray(x, np.float32)
    if info["body"] is not None:
        ci = info["body"]
        x = O.bconv2d(ci["spec"].with_batch(x.shape[0]), O.DST_F32, O.bitpack(x), ci["w"], ci["m"], ci["b"])
    return x.reshape(x.shape[0], -1)


def second_reader_model(seed=0, K=70, N=33):
    """x [1, K] -> LceQuantize -> LceDequantize -> d;  FC(+-s)(d) -> out0;  d is ALSO a graph output, so it must still be written.
    The graph begins at its rank-2 input.  Returns (file, x, outputs [out0, d], info); info["t"] is the section's input."""
    b = ModelBuilder()
    g = synth.rng(seed + 1301)
    x = t = b.tensor([1, K], np.float32, "x")
    q, d, (kq, kd) = _sign_pair(b, t, K, "0")
    w, s, wb = dense_weights(g, K, N)
    out, kf = _dense(b, d, w, wb, NONE, "0")
    b.inputs, b.outputs = [x], [out, d]
    return b.finish(), x, [out, d], dict(t=t, bits=q, sign=d, w=w, s=s, wb=wb, k=K, n=N, quantize=kq, dequantize=kd, fc=kf)


def second_reader_forward(t, info):
    """(out0, d) from the section's input t."""
    t = np.asarray(t, np.float32)
    bits = O.bitpack(t.reshape(t.shape[0], 1, 1, -1)).reshape(t.shape[0], -1)
    wb, s = R.prepare(info["w"])
    v, _ = R.binary_fully_connected(bits, wb, s, info["wb"], info["k"], NONE)
    return v, R.unpack_signs(bits, info["k"]).astype(np.float32)


def value_and_bits_model(seed=0, K=65, N=40, N2=12):
    """x [1, K] -> LceQuantize -> LceDequantize -> FC(+-s) -> h;  h is a graph output AND feeds LceQuantize -> LceDequantize
    -> FC(+-s) -> out1: the first launch needs both the value and the bits.  The graph begins at its rank-2 input.  Returns
    (file, x, outputs [h, out1], info); info["t"] is the section's input."""
    b = ModelBuilder()
    g = synth.rng(seed + 1401)
    x = t = b.tensor([1, K], np.float32, "x")
    layers, cur = [], t
    for n, (k, nout) in enumerate(((K, N), (N, N2))):
        w, s, wb = dense_weights(g, k, nout)
        q, d, (kq, kd) = _sign_pair(b, cur, k, str(n))
        out, kf = _dense(b, d, w, wb, NONE, str(n))
        layers.append(dict(w=w, s=s, wb=wb, act=NONE, k=k, n=nout, bits=q, sign=d, out=out, quantize=kq, dequantize=kd, fc=kf))
        cur = out
    b.inputs, b.outputs = [x], [layers[0]["out"], layers[1]["out"]]
    return b.finish(), x, list(b.outputs), dict(t=t, layers=layers)


def value_and_bits_forward(t, info):
    _, _, outs = tail_forward(t, dict(layers=info["layers"]))
    return outs[0], outs[1]


def shared_reader_model(seed=0, K=70, N=33, N2=9):
    """x [1, K] -> LceQuantize -> LceDequantize -> d;  FC(+-s)(d) -> out0, a binary Dense layer;  FC(mixed magnitudes)(d) -> out1,
    which only `head` takes: d has one `binary_dense` reader and one other reader in the SAME section, so it must still be
    written.  Returns (file, x, outputs [out0, out1], info)."""
    b = ModelBuilder()
    g = synth.rng(seed + 1601)
    x = b.tensor([1, K], np.float32, "x")
    q, d, (kq, kd) = _sign_pair(b, x, K, "0")
    w, s, wb = dense_weights(g, K, N)
    out0, kf = _dense(b, d, w, wb, NONE, "0")
    w2, b2 = (g.standard_normal((N2, K)) * 0.1).astype(np.float32), g.standard_normal(N2).astype(np.float32)
    out1, kf2 = _dense(b, d, w2, b2, NONE, "1")
    b.inputs, b.outputs = [x], [out0, out1]
    return b.finish(), x, [out0, out1], dict(t=x, bits=q, sign=d, w=w, s=s, wb=wb, k=K, n=N, w2=w2, b2=b2, n2=N2, quantize=kq,
                                             dequantize=kd, fc=kf, fc_head=kf2)


def shared_reader_forward(t, info):
    """(out0, out1) from the section's input t."""
    out0, sign = second_reader_forward(t, info)
    return out0, HR.fully_connected(sign, info["w2"], info["b2"])


def bits_of(v):
    """LceQuantize of a float [B, K] tensor: int32 [B, ceil(K/32)]."""
    v = np.asarray(v, np.float32)
    return O.bitpack(v.reshape(v.shape[0], 1, 1, -1)).reshape(v.shape[0], -1)


REFUSALS = ("mixed_magnitudes", "zero_weight", "not_dequantize", "int8_dequantize", "rank4_hw")


def refusal_model(case, seed=0, K=64, N=10):
    """x -> TANH -> [the sign] -> FULLY_CONNECTED -> out, with ONE thing that keeps the Dense layer from `binary_dense` (`head`
    still takes it where it can).  Returns (file, x, out, info) with info["fc"] the operator and info["head"] whether `head`'s
    FULLY_CONNECTED row takes it."""
    assert case in REFUSALS
    b = ModelBuilder()
    g = synth.rng(seed + 1501)
    w, s, wb = dense_weights(g, K, N)
    if case == "mixed_magnitudes":
        w[3, 5] = np.nextafter(w[3, 5], np.float32(np.inf), dtype=np.float32)
    if case == "zero_weight":
        w[2, 7] = 0.0
    head = True
    if case == "rank4_hw":
        # a [1, 2, 2, K/4] input: FULLY_CONNECTED flattens it, but its bits are not one row of ceil(K/32) words
        x = b.tensor([1, 2, 2, K // 4], np.float32, "x")
        t = b.tensor([1, 2, 2, K // 4], np.float32, "t")
        b.builtin_op(TANH_OP, [x], [t])
        q = b.tensor([1, 2, 2, R.words_of(K // 4)], np.int32, "bits")
        d = b.tensor([1, 2, 2, K // 4], np.float32, "sign")
        b.custom_op("LceQuantize", [t], [q], b"")
        b.custom_op("LceDequantize", [q], [d], b"")
    else:
        x = b.tensor([1, K], np.float32, "x")
        t = b.tensor([1, K], np.float32, "t")
        b.builtin_op(TANH_OP, [x], [t])
        if case == "not_dequantize":
            d = t
        elif case == "int8_dequantize":
            # the sign as int8 (+-1 at scale 1): the FULLY_CONNECTED behind it is not a float one at all
            _, d, _ = _sign_pair(b, t, K, "0", dq_type=np.int8, dq_quant=(1.0, 0))
            head = False
        else:
            _, d, _ = _sign_pair(b, t, K, "0")
    out, kf = _dense(b, d, w, wb, NONE, "0")
    b.inputs, b.outputs = [x], [out]
    return b.finish(), x, out, dict(fc=kf, head=head, w=w, wb=wb)
