"""A seeded generator of random mixed float / int8 / bitpacked networks over every operator the section runner takes, for
tests/test_random_models_host.py and tests/test_gpu_random_models.py.  No tests here.

`build(seed)` grows a DAG of typed tensors -- kinds f32, i8 (scale, zero point) and bits -- one operator at a time, each a
transition the kind allows (the table in `_Gen.step`), evaluates every operator on the seed's own input as it goes (the NumPy
restatements of tests/*_ref.py and the oracle), and calibrates each operator's constants on those values so that int8 tensors
spread over their range and bit tensors stay mixed.  The operators are then written in a random topological order.  A seed is a
case; a failing case is named by its seed.

The constants come from the fixtures' routines (synth.conv_inputs, int8_conv_models.conv_constants,
depthwise_i8_models.depthwise_constants, head_models.head, head_i8_models.head_i8); the calibration only rescales their filter scales
and re-centres their biases on the values the operator really sees.  LceBconv2d is written here and not through
section_models._conv / int8_conv_models._bconv_int8, which know square maps only; the layout of its operands is theirs."""
import functools
import os

import numpy as np

import conv1x1_ref as C1
import conv2d_i8_ref as CI
import conv2d_ref as KR
import depthwise_i8_models as DM
import depthwise_i8_ref as DI
import depthwise_ref as DR
import flexbuf
import head_i8_models as HIM
import head_i8_ref as HI
import head_models as HM
import head_ref as HR
import int8_add_ref as A
import int8_conv_models as M
import oracle_lib as O
import partition_ref as P
import pool_ref as PR
import synth
from tflite_writer import _Vector
from section_models import (ADD, AVERAGE_POOL_2D, MAX_POOL_2D, MUL, NONE, RELU, RELU6, RELU_N1_TO_1, SAME, VALID, bconv_options, concat_op,
                            conv2d_op, depthwise_op, ew_op, float_op, pool_op)

# every keyword of model_runner.LceModel: depthwise_i8_models.EVERY_FLAG holds the int8 names, head_models.EVERY_FLAG the float ones
EVERY_FLAG = dict(DM.EVERY_FLAG, concat_sections=True, **HM.EVERY_FLAG)
# the keyword that enables each pass
FLAG_OF = dict(elementwise="elementwise_sections", int8_add="int8_add_sections", concat="concat_sections", pool="pool_sections",
               conv1x1="conv1x1_sections", depthwise="depthwise_sections", conv2d="conv2d_sections", conv_i8="conv2d_i8_sections",
               depthwise_i8="depthwise_i8_sections", mean="head_sections", fully_connected="head_sections", softmax="head_sections",
               mean_i8="head_i8_sections", fully_connected_i8="head_i8_sections", softmax_i8="head_i8_sections",
               quantize="quantize_sections", dequantize="quantize_sections")
assert set(FLAG_OF) == set(P.PASSES) and set(FLAG_OF.values()) | {"stem_sections"} == set(EVERY_FLAG)
CHANNELS = (16, 32, 33, 40, 64, 70, 96)
FEATURES = "abcdefghijk"
# what (h) asks of the joins, counted apart: 4 or more inputs, exactly LCE_HIP_CONCAT_MAX_INPUTS, one tensor listed twice, and a
# float / int8 join with an input whose channel count is no multiple of 32 (the inputs then start off a word of the folded bits)
JOIN_FEATURES = ("h_wide", "h_max", "h_dup", "h_ragged_f32", "h_ragged_i8")
ACTS = (NONE, RELU, RELU_N1_TO_1, RELU6)
CONCAT_MAX = 8                                                       # LCE_HIP_CONCAT_MAX_INPUTS


def f32(v):
    return float(np.float32(v))


class _T:
    """A live tensor: kind 'f32' | 'i8' | 'bits', NHWC extents (c: channels, also for bits), its quantization, its value on the
    seed's input, and how it is used."""

    def __init__(self, n, kind, val, c, q=None, rank2=False, keep_dims=False):
        self.n, self.kind, self.val, self.c, self.q, self.rank2, self.keep_dims = n, kind, val, c, q, rank2, keep_dims
        self.h, self.w = (1, 1) if rank2 else val.shape[1:3]
        self.readers, self.output, self.producer = [], False, None

    @property
    def shape(self):
        if self.rank2 and not self.keep_dims:
            return [1, self.c]
        return [1, self.h, self.w, (self.c + 31) // 32 if self.kind == "bits" else self.c]

    @property
    def dtype(self):
        return dict(f32=np.float32, i8=np.int8, bits=np.int32)[self.kind]

    def negative(self):
        """The share of elements LceQuantize would give the bit 1."""
        return float(np.mean(self.val < (self.q[1] if self.kind == "i8" else 0)))

    def balanced(self):
        return self.kind != "bits" and not self.rank2 and 0.3 <= self.negative() <= 0.7


class _Node:
    def __init__(self, name, alts, ins, out, emit, fn):
        self.name, self.alts, self.ins, self.out, self.emit, self.fn = name, alts, ins, out, emit, fn
        self.after = None                                              # an operator the file order puts in front of this one


def ones_share(words, c):
    """The share of 1 bits among the `c` valid channels of a bitpacked tensor."""
    u = np.ascontiguousarray(words).view(np.uint32)
    bits = ((u[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(u.shape[:-1] + (-1,))[..., :c]
    return float(bits.mean())


class _Gen:
    def __init__(self, seed):
        self.seed = seed
        self.g = np.random.default_rng(seed)
        self.tensors, self.nodes = [], []
        self.features = {k: 0 for k in FEATURES}
        g = self.g
        self.batch = int(g.choice([1, 3, 8]))
        self.images = self.batch + 2
        self.budget = int(g.integers(6, 21))
        self.head = bool(g.integers(0, 2))
        self.budget = max(self.budget, 8) if self.head else self.budget
        # the rarer graph shapes are drawn on purpose: a chain past the cap (e), a chain operand written late (f), a residual chain (i)
        # ... and a join of 4 to LCE_HIP_CONCAT_MAX_INPUTS inputs (w)
        self.want = {k for k in "efiw" if g.random() < 0.3}
        self.budget = max(self.budget, 15) if "e" in self.want else self.budget
        h = int(g.integers(5, 13))
        w = h if g.random() < 0.3 else int(g.integers(5, 13))
        c = int(g.choice((3,) + CHANNELS))
        shape = (self.images, h, w, c)
        if g.random() < 0.55:
            x = g.uniform(-1.5, 1.5, shape).astype(np.float32)
            x.reshape(-1)[g.integers(0, x.size, 6)] = np.float32(-0.0)
            self.x = self.new("f32", x, c)
        else:
            q = (f32(g.uniform(0.02, 0.05)), int(g.choice([-128, -4, 0, 7, 127])))
            x = g.integers(-128, 128, shape, dtype=np.int64).astype(np.int8)
            x.reshape(-1)[:2] = (-128, 127)
            self.x = self.new("i8", x, c, q)

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------------
    def new(self, kind, val, c, q=None, **kw):
        t = _T(len(self.tensors), kind, val, c, q, **kw)
        self.tensors.append(t)
        return t

    def left(self):
        return self.budget - len(self.nodes) - ((4 if self.head else 0))

    def op(self, name, ins, kind, c, emit, fn, q=None, alts=None, **kw):
        with np.errstate(all="ignore"):
            val = fn(*[t.val for t in ins])
        out = self.new(kind, val, c, q, **kw)
        out.producer = len(self.nodes)
        for t in ins:
            t.readers.append(len(self.nodes))
        alts = alts if alts is not None else ([(FLAG_OF[name], name)] if name in FLAG_OF else [])
        self.nodes.append(_Node(name, alts, ins, out, emit, fn))
        return out

    def pick_act(self, real, allowed=ACTS):
        """An activation that clamps less than 30 % of `real` (the float values behind a tensor) on either side."""
        ok = [a for a in allowed if a == NONE or
              (a == RELU and np.mean(real < 0) < 0.3) or (a == RELU6 and np.mean(real < 0) < 0.3 and np.mean(real > 6) < 0.3) or
              (a == RELU_N1_TO_1 and np.mean(real < -1) < 0.3 and np.mean(real > 1) < 0.3)]
        return int(self.g.choice(ok)) if self.g.random() < 0.6 else NONE

    # ---- the LCE operators ------------------------------------------------------------------------------------------------------------
    def lceq(self, t):
        zp = t.q[1] if t.kind == "i8" else 0
        return self.op("LceQuantize", [t], "bits", t.c, lambda b, i, o: b.custom_op("LceQuantize", i, [o], b""), lambda v: O.bitpack(v, zp))

    def lcedq(self, t):
        c = t.c
        return self.op("LceDequantize", [t], "f32", c, lambda b, i, o: b.custom_op("LceDequantize", i, [o], b""),
                       lambda v: O.unpack(v, c, np.float32))

    def bmaxpool(self, t):
        g = self.g
        fh, fw, sh, sw, pad = [(2, 2, 2, 2, O.PADDING_VALID), (2, 2, 1, 1, O.PADDING_SAME), (1, 2, 1, 2, O.PADDING_VALID)][int(g.integers(0, 3))]
        fn = lambda v: O.bmaxpool(v, fh, fw, sh, sw, pad)
        if not 0.22 <= ones_share(fn(t.val), t.c) <= 0.78:
            return None
        return self.op("LceBMaxPool2d", [t], "bits", t.c,
                       lambda b, i, o: b.custom_op("LceBMaxPool2d", i, [o], flexbuf.bmaxpool_options(fh, fw, sh, sw, pad)), fn)

    def bconv(self, t, dst, cout=None, k=None, stride=None, ones=0.5, pad=None, q=None):
        """LceBconv2d on the bit tensor `t` to a float, int8 or bitpacked output.  synth.conv_inputs' weights and multipliers; the
        bias (and for int8 the multiplier's size) calibrated on the accumulators the operator sees: a float or int8 output is
        centred per channel, a bitpacked one has the share `ones` of 1 bits per channel."""
        g = self.g
        k = k or int(g.choice([1, 3, 3]))
        stride = stride or int(g.choice([1, 1, 2]))
        cout = cout or int(g.choice(CHANNELS))
        pad = pad or ((O.PADDING_VALID, 0) if (g.random() < 0.3 and min(t.h, t.w) >= k) else (O.PADDING_SAME, 1))
        act = O.ACT_RELU if (dst != O.DST_BITPACKED and g.random() < 0.12) else O.ACT_NONE
        spec = O.ConvSpec(1, t.h, t.w, t.c, k, k, cout, 1, stride, stride, 1, 1, pad[0], pad[1], act)
        _, wts, mul, bias = synth.conv_inputs(spec, int(g.integers(0, 9999)), negative_mul_fraction=0.2)
        plain = O.ConvSpec(self.images, t.h, t.w, t.c, k, k, cout, 1, stride, stride, 1, 1, pad[0], pad[1], O.ACT_NONE)   # (no clamp)
        acc = O.bconv2d(plain, O.DST_F32, t.val, wts, np.ones(cout, np.float32), np.zeros(cout, np.float32))
        rows = acc.reshape(-1, cout).astype(np.float64)
        thr = None
        if dst == O.DST_I8:
            q = q or (f32(g.uniform(0.02, 0.08)), int(g.integers(-20, 21)))
            mul = (np.sign(mul) * g.uniform(0.6, 1.4, cout) * 40.0 * q[0] / max(rows.std(), 1.0)).astype(np.float32)
            bias = (-mul * rows.mean(0) + g.uniform(-5, 5, cout) * q[0] + (30 * q[0] if act else 0)).astype(np.float32)
        elif dst == O.DST_F32:
            bias = (-mul * np.median(rows, 0) + g.uniform(-0.5, 0.5, cout) + (np.abs(mul) * rows.std(0) if act else 0)).astype(np.float32)
        else:
            y = rows * mul
            bias = (-np.quantile(y, ones, axis=0) + 1e-3).astype(np.float32)
            thr = O.thresholds_converter(spec, mul, bias)
        kw = dict(out_scale=q[0], out_zero_point=q[1]) if q else {}
        fn = lambda v: O.bconv2d(spec.with_batch(v.shape[0]), dst, v, wts, mul, bias, thr, **kw)

        def emit(b, i, o):
            tw = b.tensor(wts.shape, np.int32, "bw", wts)
            if dst == O.DST_BITPACKED:
                return b.custom_op("LceBconv2d", i + [tw, -1, -1, b.tensor([cout], np.int32, "thr", thr)], [o], bconv_options(spec))
            return b.custom_op("LceBconv2d", i + [tw, b.tensor([cout], np.float32, "bm", mul), b.tensor([cout], np.float32, "bb", bias), -1],
                               [o], bconv_options(spec))
        return self.op("LceBconv2d", [t], ("f32", "i8", "bits")[dst], cout, emit, fn, q)

    # ---- the float / int8 boundary ------------------------------------------------------------------------------------------------------
    def quantize(self, t):
        lo, hi = np.quantile(t.val[np.isfinite(t.val)], [0.01, 0.99])
        scale = f32(max(hi - lo, 1e-3) / 215.0)
        q = (scale, int(np.clip(np.rint(-108 - lo / scale), -128, 127)))
        return self.op("quantize", [t], "i8", t.c, lambda b, i, o: b.builtin_op(HIM.QUANTIZE, i, [o]), lambda v: HI.quantize(v, *q), q)

    def dequantize(self, t, **kw):
        q = t.q
        return self.op("dequantize", [t], "f32", t.c, lambda b, i, o: b.builtin_op(HIM.DEQUANTIZE, i, [o]), lambda v: HI.dequantize(v, *q), **kw)

    # ---- float passes -------------------------------------------------------------------------------------------------------------------
    def ew(self, t, other=None, code=None, act=None, centre=False):
        """One ADD / MUL on the float tensor `t`: with the tensor `other`, or with a scalar or per-channel constant."""
        g = self.g
        code = code if code is not None else int(g.choice([ADD, MUL]))
        if other is not None:
            if code == MUL and float(np.abs(t.val).max()) * float(np.abs(other.val).max()) > 1e6:
                code = ADD
            act = self.pick_act(float_op(t.val, code, other.val, NONE)) if act is None else act
            first = g.random() < 0.5
            ins = [t, other] if first else [other, t]
            fn = (lambda a, c: float_op(a, code, c, act)) if first else (lambda c, a: float_op(a, code, c, act))
            return self.op("elementwise", ins, "f32", t.c, lambda b, i, o: ew_op(b, code, i, [o], act), fn)
        form = int(g.integers(0, 4))                                   # [], [1], [C], [1, 1, 1, C]
        n = 1 if form < 2 else t.c
        if centre:                                                     # a batch norm's shift: the result is centred per channel
            code, form, n, act = ADD, 2 + int(g.integers(0, 2)), t.c, NONE
            const = (-np.median(t.val.reshape(-1, t.c), 0)).astype(np.float32)
        elif code == MUL:
            const = (g.uniform(0.5, 1.5, n) * g.choice([-1, 1, 1, 1], n)).astype(np.float32)
        else:
            const = g.standard_normal(n).astype(np.float32)
        shape = [[], [1], [t.c], [1, 1, 1, t.c]][form]
        operand = const.reshape(shape) if form != 1 else const
        act = self.pick_act(float_op(t.val, code, const, NONE)) if act is None else act
        first = g.random() < 0.7
        fn = lambda a: float_op(a, code, const, act)

        def emit(b, i, o):
            k = b.tensor(shape or [1], np.float32, "k", operand.reshape(shape or [1]))
            if not shape:                                              # a rank-0 constant: the writer's helper makes rank 1 of it
                b.tensors[k].fields[0] = _Vector("i", [])
            return ew_op(b, code, i + [k] if first else [k] + i, [o], act)
        return self.op("elementwise", [t], "f32", t.c, emit, fn)

    def window(self, t, filters=((2, 2), (3, 3), (2, 3), (3, 1))):
        g = self.g
        filt = filters[int(g.integers(0, len(filters)))]
        stride = [(1, 1), (1, 1), (2, 2), (2, 1)][int(g.integers(0, 4))]
        padding = VALID if (g.random() < 0.35 and t.h >= filt[0] and t.w >= filt[1]) else SAME
        return filt, stride, padding

    def pool(self, t, same_shape=False):
        g = self.g
        filt, stride, padding = self.window(t)
        if same_shape:
            stride, padding = (1, 1), SAME
        op = int(g.integers(0, 2))                                     # PR.MAX, PR.AVERAGE
        code = MAX_POOL_2D if op == PR.MAX else AVERAGE_POOL_2D
        if t.kind == "f32":
            act = self.pick_act(PR.pool2d(t.val, op, filt, stride, padding))
            fn = lambda v: PR.pool2d(v, op, filt, stride, padding, act)
        else:
            s, z = t.q
            real = (PR.pool2d(t.val, op, filt, stride, padding, NONE, s, z).astype(np.float32) - z) * s
            act = self.pick_act(real)
            fn = lambda v: PR.pool2d(v, op, filt, stride, padding, act, s, z)
        return self.op("pool", [t], t.kind, t.c, lambda b, i, o: pool_op(b, code, i, [o], filt, stride, padding, act), fn, t.q)

    def float_bias(self, chain, cout, bias):
        """(bias or None, activation): the bias centres each channel of `chain`, the convolution's sums before it."""
        g = self.g
        if not bias:
            return None, self.pick_act(chain)
        act = int(g.choice(ACTS)) if g.random() < 0.5 else NONE
        rows = chain.reshape(-1, cout)
        shift = {NONE: 0.0, RELU: 1.0, RELU6: 1.0, RELU_N1_TO_1: 0.0}[act] * rows.std(0)
        return (-np.median(rows, 0) + shift + g.uniform(-0.2, 0.2, cout)).astype(np.float32), act

    def conv1x1(self, t):
        g = self.g
        cout = int(g.choice(CHANNELS))
        w = (g.standard_normal((cout, 1, 1, t.c)) * 0.2).astype(np.float32)
        stride = [(1, 1), (1, 1), (2, 2), (1, 2)][int(g.integers(0, 4))]
        bias, act = self.float_bias(C1.conv1x1(t.val, w, None, stride), cout, g.random() < 0.7)
        pad = int(g.integers(0, 2))

        def emit(b, i, o):
            ins = i + [b.tensor(w.shape, np.float32, "w", w)] + ([b.tensor([cout], np.float32, "wb", bias)] if bias is not None else [])
            return conv2d_op(b, ins, [o], stride, pad, act)
        alts = [(FLAG_OF["conv1x1"], "conv1x1"), (FLAG_OF["conv2d"], "conv2d")]
        return self.op("conv1x1", [t], "f32", cout, emit, lambda v: C1.conv1x1(v, w, bias, stride, act), alts=alts)

    def conv2d(self, t):
        g = self.g
        cout = int(g.choice([16, 32, 33]))
        filt, stride, padding = self.window(t, ((3, 3), (2, 3), (5, 5), (1, 3)) if t.c == 3 else ((3, 3), (2, 3), (1, 3)))
        w = (g.standard_normal((cout, filt[0], filt[1], t.c)) * 0.3).astype(np.float32)
        bias, act = self.float_bias(KR.chain(t.val, w, stride, padding), cout, g.random() < 0.7)

        def emit(b, i, o):
            ins = i + [b.tensor(w.shape, np.float32, "w", w)] + ([b.tensor([cout], np.float32, "wb", bias)] if bias is not None else [-1])
            return conv2d_op(b, ins, [o], stride, padding, act)
        return self.op("conv2d", [t], "f32", cout, emit, lambda v: KR.conv2d(v, w, bias, stride, padding, act))

    def depthwise(self, t):
        g = self.g
        m = int(g.choice([1, 1, 2, 3])) if t.c <= 40 else 1
        cout = t.c * m
        filt, stride, padding = self.window(t)
        w = (g.standard_normal((1, filt[0], filt[1], cout)) * 0.4).astype(np.float32)
        bias, act = self.float_bias(DR.chain(t.val, w, stride, padding, m), cout, g.random() < 0.6)

        def emit(b, i, o):
            ins = i + [b.tensor(w.shape, np.float32, "dw", w)] + ([b.tensor([cout], np.float32, "db", bias)] if bias is not None else [])
            return depthwise_op(b, ins, [o], stride, padding, m, act)
        return self.op("depthwise", [t], "f32", cout, emit, lambda v: DR.depthwise(v, w, bias, stride, padding, m, act))

    def concat(self, ts):
        kind, q = ts[0].kind, ts[0].q
        axis = int(self.g.choice([3, -1]))
        c = sum(t.c for t in ts)
        return self.op("concat", ts, kind, c, lambda b, i, o: concat_op(b, i, [o], axis), lambda *v: np.concatenate(v, axis=3), q)

    # ---- int8 passes ----------------------------------------------------------------------------------------------------------------------
    def int8_add(self, a, c):
        g = self.g
        real = (a.val.astype(np.float64) - a.q[1]) * a.q[0] + (c.val.astype(np.float64) - c.q[1]) * c.q[0]
        lo, hi = np.quantile(real, [0.005, 0.995])
        scale = f32(max(hi - lo, 1e-3) / 235.0)
        act = self.pick_act(real)
        zp = int(np.clip(np.rint(-118 - lo / scale), -128, 127))
        q = (scale, zp)
        q6 = (a.q[0], a.q[1], c.q[0], c.q[1], scale, zp)
        return self.op("int8_add", [a, c], "i8", a.c, lambda b, i, o: ew_op(b, ADD, i, [o], act), lambda u, v: A.add_q(u, v, q6, act), q)

    def q_for(self, act):
        """(output quantization, the level above its zero point on which the sums are centred) for a quantized convolution."""
        g = self.g
        if act == RELU:
            return (f32(g.uniform(0.02, 0.06)), int(g.integers(-128, -89))), 55
        if act == RELU6:
            return (f32(g.uniform(0.021, 0.0235)), -128), 110
        if act == RELU_N1_TO_1:
            return (f32(g.uniform(0.0072, 0.0078)), int(g.integers(-3, 4))), 0
        return (f32(g.uniform(0.02, 0.06)), int(g.integers(-20, 21))), 0

    def calibrate(self, acc, bias, sw, s_in, q_out, centre):
        """int8_conv_models.conv_constants' filter scales `sw` rescaled so that acc + bias spreads over about +-40 levels of the
        output, and its bias (when there is one) shifted so that each channel is centred `centre` levels above the zero point."""
        cout = acc.shape[-1]
        rows = acc.reshape(-1, cout).astype(np.float64) + (0 if bias is None else bias.astype(np.float64))
        rel = np.broadcast_to(sw / sw.mean(), (cout,)).astype(np.float64)
        spread = (rows * rel - (rows * rel).mean(0) * (bias is not None)).std()
        mult = rel * 40.0 / max(spread, 1.0)
        if bias is not None:
            bias = (bias + np.rint(centre / mult - rows.mean(0))).astype(np.int32)
        else:
            q_out = (q_out[0], int(np.clip(q_out[1] + centre - np.rint((rows * mult).mean()), -100, 100)))
        sw = (mult[:sw.size] * q_out[0] / s_in).astype(np.float32)
        return bias, sw, q_out

    def conv_i8(self, t):
        g = self.g
        cout = int(g.choice(CHANNELS))
        filt, stride, padding = self.window(t, ((1, 1), (1, 1), (3, 3), (2, 3)))
        per_channel, has_bias = bool(g.integers(0, 2)), g.random() < 0.7
        act = int(g.choice(ACTS)) if (has_bias and g.random() < 0.5) else NONE
        q_out, centre = self.q_for(act)
        w, bias, sw = M.conv_constants(cout, filt, t.c, int(g.integers(0, 9999)), t.q, q_out, per_channel)
        bias, sw, q_out = self.calibrate(CI.accumulate(t.val, w, t.q[1], stride, padding), bias if has_bias else None, sw, t.q[0], q_out, centre)
        q_in = t.q

        def emit(b, i, o):
            ins = i + [M.filter_tensor(b, w, sw)] + ([b.tensor([cout], np.int32, "wb", bias)] if has_bias else [])
            return conv2d_op(b, ins, [o], stride, padding, act)
        return self.op("conv_i8", [t], "i8", cout, emit, lambda v: CI.conv2d_i8(v, w, bias, sw, q_in, q_out, stride, padding, act), q_out)

    def depthwise_i8(self, t):
        g = self.g
        m = int(g.choice([1, 1, 2, 3])) if t.c <= 40 else 1
        cout = t.c * m
        filt, stride, padding = self.window(t)
        per_channel, has_bias = bool(g.integers(0, 2)), g.random() < 0.7
        act = int(g.choice(ACTS)) if (has_bias and g.random() < 0.5) else NONE
        q_out, centre = self.q_for(act)
        w, bias, sw = DM.depthwise_constants(cout, filt, int(g.integers(0, 9999)), t.q, q_out, per_channel)
        bias, sw, q_out = self.calibrate(DI.accumulate(t.val, w, t.q[1], stride, padding, m), bias if has_bias else None, sw, t.q[0], q_out, centre)
        q_in = t.q

        def emit(b, i, o):
            ins = i + [DM.depthwise_filter_tensor(b, w, sw)] + ([b.tensor([cout], np.int32, "db", bias)] if has_bias else [])
            return depthwise_op(b, ins, [o], stride, padding, m, act)
        return self.op("depthwise_i8", [t], "i8", cout, emit,
                       lambda v: DI.depthwise_i8(v, w, bias, sw, q_in, q_out, stride, padding, m, act), q_out)

    # ---- the heads --------------------------------------------------------------------------------------------------------------------------
    def float_head(self, t):
        g = self.g
        classes, keep, beta = int(g.integers(5, 17)), bool(g.integers(0, 2)), f32(g.choice([0.5, 1.0, 2.0]))
        act, has_bias = int(g.choice([NONE, NONE, RELU])), g.random() < 0.7
        hi = HM.head(HM.ModelBuilder(), 0, t.h, t.c, classes, int(g.integers(0, 999)), keep, beta, act, has_bias)[1]
        w, wb = hi["w"], hi["wb"]
        c = t.c

        def emit_mean(b, i, o):
            return HM.mean_op(b, i + [b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [o], keep)

        def emit_fc(b, i, o):
            ins = i + [b.tensor([classes, c], np.float32, "dense_w", w)] + ([b.tensor([classes], np.float32, "dense_b", wb)] if has_bias else [])
            return HM.fc_op(b, ins, [o], act)
        pooled = self.op("mean", [t], "f32", c, emit_mean, lambda v: HR.mean_hw(v, keep), rank2=True, keep_dims=keep)
        logits = self.op("fully_connected", [pooled], "f32", classes, emit_fc, lambda v: HR.fully_connected(v, w, wb, act), rank2=True)
        return self.op("softmax", [logits], "f32", classes, lambda b, i, o: HM.softmax_op(b, i, [o], beta), lambda v: HR.softmax(v, beta), rank2=True)

    def int8_head(self, t):
        g = self.g
        classes, keep, beta = int(g.integers(7, 17)), bool(g.integers(0, 2)), f32(g.choice([0.5, 1.0]))
        per_channel, has_bias = bool(g.integers(0, 2)), g.random() < 0.7
        c, q_src = t.c, t.q
        real = (t.val.astype(np.float64) - q_src[1]).mean((1, 2)) * q_src[0]
        lo, hi = real.min(), real.max()
        s = f32(max(hi - lo, 1e-3) / 200.0)
        q_pooled = (s, int(np.clip(np.rint(-100 - lo / s), -128, 127)))
        q_logits = (f32(g.uniform(0.03, 0.06)), int(g.integers(-15, 16)))
        scratch = M.QModelBuilder()
        src = scratch.tensor([1, t.h, t.w, c], np.int8, "src", scale=q_src[0], zero_point=q_src[1])
        hi_ = HIM.head_i8(scratch, src, q_src, t.h, c, classes, int(g.integers(0, 999)), per_channel, keep, beta, NONE, has_bias, q_pooled, q_logits)[1]
        w, wb, sw, host = hi_["w"], hi_["wb"], np.atleast_1d(hi_["sw"]), hi_["host"]
        # (the logits' spread: conv_constants sizes its scales for inputs over the whole int8 range; the pooled map is calibrated to that)

        def emit_mean(b, i, o):
            return HM.mean_op(b, i + [b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [o], keep)

        def emit_fc(b, i, o):
            ins = i + [b.qtensor(w.shape, np.int8, "dense_w", w, sw, [0] * sw.size, 0)] + ([b.tensor([classes], np.int32, "dense_b", wb)] if has_bias else [])
            return HM.fc_op(b, ins, [o], NONE)
        pooled = self.op("mean_i8", [t], "i8", c, emit_mean, host[hi_["mean"]], q_pooled, rank2=True, keep_dims=keep)
        logits = self.op("fully_connected_i8", [pooled], "i8", classes, emit_fc, host[hi_["fc"]], q_logits, rank2=True)
        probs = self.op("softmax_i8", [logits], "i8", classes, lambda b, i, o: HM.softmax_op(b, i, [o], beta), host[hi_["softmax"]], HIM.Q_PROBS, rank2=True)
        return self.dequantize(probs, rank2=True)

    # ---- growth -------------------------------------------------------------------------------------------------------------------------------
    def same_map(self, t, kind=None):
        return [u for u in self.tensors if u.kind == (kind or t.kind) and not u.rank2 and u.c != 3 and (u.h, u.w) == (t.h, t.w) and (t.kind != "i8" or u.q == t.q)]

    def fold_variants(self, p):
        """Behind the balanced pass output `p`: the reader patterns FoldQuantize has branches for (features a to d)."""
        if not p.balanced() or self.left() < 1:
            return
        r = self.g.random()
        self.lceq(p)
        if 0.3 <= r < 0.5:
            p.output = True
        elif 0.5 <= r < 0.75 and self.left() >= 1:
            self.lceq(p)
        elif 0.75 <= r and self.left() >= 1:
            (self.pool(p) if self.g.random() < 0.5 or p.kind == "i8" else self.ew(p))

    def branches(self, bits):
        """(g) two LceBconv2d off one bit tensor, joined by an ADD (float, int8) or a CONCATENATION (any kind)."""
        g = self.g
        dst = int(g.choice([O.DST_F32, O.DST_I8, O.DST_BITPACKED]))
        join_add = dst != O.DST_BITPACKED and g.random() < 0.5
        k, stride = int(g.choice([1, 3])), int(g.choice([1, 1, 2]))
        c1 = int(g.choice([32, 64] if dst == O.DST_BITPACKED else CHANNELS))
        c2 = c1 if join_add else int(g.choice([32, 64, 96] if dst == O.DST_BITPACKED else CHANNELS))
        y1 = self.bconv(bits, dst, c1, k, stride, pad=(O.PADDING_SAME, 1))
        # (an int8 join needs ONE quantization: the second branch is written at the first one's)
        y2 = self.bconv(bits, dst, c2, k, stride, pad=(O.PADDING_SAME, 1), q=None if join_add else y1.q)
        if (y1.h, y1.w) != (y2.h, y2.w):
            return y2
        if join_add:
            return self.ew(y1, y2, ADD) if dst == O.DST_F32 else self.int8_add(y1, y2)
        return self.concat([y1, y2] + ([y1] if g.random() < 0.3 else []))

    def residual(self, t):
        """(i) an int8 residual chain: t -> LceQuantize -> LceBconv2d (int8) -> ADD with t, twice when there is room."""
        for _ in range(2):
            if self.left() < 3 or not t.balanced():
                return t
            y = self.bconv(self.lceq(t), O.DST_I8, t.c, 3, 1, pad=(O.PADDING_SAME, 1))
            if (y.h, y.w) != (t.h, t.w):
                return y
            t = self.int8_add(y, t) if self.g.random() < 0.5 else self.int8_add(t, y)
            self.features["i"] += 1
        return t

    def late_operand(self, t):
        """(f) t -> ADD / MUL (constant) -> ADD / MUL with a pool of t that the file order puts behind the first of the two."""
        v = self.ew(t)
        first = len(self.nodes) - 1
        side = self.pool(t, same_shape=True)
        self.nodes[side.producer].after = first
        return self.ew(v, side)

    def chain(self, t, long=None):
        """(e) an ADD / MUL chain of 1 to 10 steps; a step may take a tensor that a side branch produces, which the file order may
        put behind the chain's first operator (f)."""
        g = self.g
        long = self.left() >= 9 and (g.random() < 0.75 if long is None else long)   # past the cap: constants and the chain's own source only
        length = int(g.integers(9, 11)) if long else int(min(g.integers(1, 9), self.left()))
        v, src = t, t
        for k in range(length):
            r = g.random()
            if long:
                v = self.ew(v, src) if (r < 0.15 and k) else self.ew(v, centre=(k == length - 1 and r < 0.6))
                continue
            if r < 0.4 and k and k != 8 and self.left() >= 2:
                v = self.ew(v, self.pool(src, same_shape=True))
            elif r < 0.5:
                peers = [u for u in self.same_map(v) if u.c == v.c and u is not v]
                v = self.ew(v, peers[int(g.integers(0, len(peers)))]) if peers else self.ew(v)
            elif r < 0.55:
                v = self.ew(v, v, ADD)
            else:
                v = self.ew(v, centre=(k == length - 1 and g.random() < 0.6))
            if self.left() < 1:
                break
        return v

    def join(self, t):
        """(h) a CONCATENATION of 2 to 8 inputs of t's kind and map, one of them possibly listed twice; ragged channel counts."""
        g = self.g
        pool = self.same_map(t)
        if t.kind == "bits":
            pool = [u for u in pool if u.c % 32 == 0]
        while len(pool) < 3 and self.left() >= 2 and t.kind != "bits":
            pool.append(self.pool(t, same_shape=True) if (t.kind == "i8" or g.random() < 0.5) else self.ew(t))
        n = int(g.integers(2, CONCAT_MAX + 1)) if g.random() < 0.4 else int(g.integers(2, 4))
        if len(pool) < 1 or (t.kind == "bits" and t.c % 32):
            return None
        ts = [t] + [pool[int(g.integers(0, len(pool)))] for _ in range(n - 1)]
        return self.concat(ts)

    def wide_join(self, t):
        """(h) a CONCATENATION of 4 to LCE_HIP_CONCAT_MAX_INPUTS inputs, half of the time exactly that many: `t`, one to three cheap
        tensors of its map and quantization (a pool at stride 1, a float ADD / MUL), and repeats of them in a random order."""
        g = self.g
        n = CONCAT_MAX if g.random() < 0.5 else int(g.integers(4, CONCAT_MAX))
        ts = [t]
        for _ in range(int(min(g.integers(1, 4), self.left() - 1))):
            ts.append(self.pool(t, same_shape=True) if (t.kind == "i8" or g.random() < 0.5) else self.ew(t))
        ts += [ts[int(g.integers(0, len(ts)))] for _ in range(n - len(ts))]
        return self.concat([ts[k] for k in g.permutation(len(ts))])

    def step(self):
        """One round of the growth: a tensor, and one transition its kind allows (the table)."""
        g = self.g
        fresh = [t for t in self.tensors if not t.readers and not t.output and not t.rank2]
        live = [t for t in self.tensors if not t.rank2]
        t = fresh[int(g.integers(0, len(fresh)))] if fresh and g.random() < 0.85 else live[int(g.integers(0, len(live)))]
        r, out = g.random(), None
        floats = [u for u in fresh if u.kind == "f32" and u.c != 3]
        if "e" in self.want and floats and self.left() >= 9:
            self.want.discard("e")
            out = self.chain(floats[0], long=True)
        elif "f" in self.want and floats and self.left() >= 3:
            self.want.discard("f")
            out = self.late_operand(floats[0])
        elif "i" in self.want and self.left() >= 3 and any(u.kind == "i8" and u.c != 3 and u.balanced() for u in fresh):
            self.want.discard("i")
            out = self.residual([u for u in fresh if u.kind == "i8" and u.c != 3 and u.balanced()][0])
        elif "w" in self.want and self.left() >= 2 and any(u.kind != "bits" and 3 < u.c <= 96 for u in fresh):
            self.want.discard("w")
            out = self.wide_join([u for u in fresh if u.kind != "bits" and 3 < u.c <= 96][0])
        elif t.kind == "bits":
            if r < 0.25 and self.left() >= 3:
                out = self.branches(t)
            elif r < 0.30:
                out = self.lcedq(t)
            elif r < 0.34 and t.c % 32 == 0:
                out = self.join(t)
            elif r < 0.5 and self.left() >= 2 and min(t.h, t.w) >= 4:
                y = self.bconv(t, O.DST_BITPACKED, ones=0.73)
                out = self.bmaxpool(y) if min(y.h, y.w) >= 2 else None
            else:
                out = self.bconv(t, int(g.choice([O.DST_F32, O.DST_F32, O.DST_I8, O.DST_I8, O.DST_BITPACKED])))
                if out.kind != "bits" and out.balanced() and g.random() < 0.25 and self.left() >= 2:
                    self.lceq(out), self.lceq(out)
        elif t.c == 3:                                             # three channels: a stem's convolution only
            out = (self.conv2d(t) if g.random() < 0.7 else self.depthwise(t)) if t.kind == "f32" else \
                (self.conv_i8(t) if g.random() < 0.7 else self.depthwise_i8(t))
        elif t.kind == "f32":
            heavy = t.c * 6 <= 240
            if t.c > 192 and 0.58 <= r:                            # a wide join's result: no float convolution over it, no join
                r = 0.85 if r < 0.8 else 0.55
            if r < 0.22 and t.balanced():
                out = self.lceq(t)
            elif r < 0.30:
                out = self.quantize(t)
            elif r < 0.52:
                out = self.chain(t)
            elif r < 0.58:
                out = self.pool(t)
            elif r < 0.70:
                out = self.conv1x1(t)
            elif r < 0.80 and heavy:
                out = self.conv2d(t)
            elif r < 0.88:
                out = self.depthwise(t)
            else:
                out = self.join(t)
        else:
            if r < 0.2 and t.balanced():
                out = self.lceq(t)
            elif r < 0.28:
                out = self.dequantize(t)
            elif r < 0.46:
                out = self.residual(t)
            elif r < 0.52:
                peers = [u for u in self.tensors if u.kind == "i8" and not u.rank2 and u is not t and (u.h, u.w, u.c) == (t.h, t.w, t.c)]
                out = self.int8_add(t, peers[int(g.integers(0, len(peers)))]) if peers else self.pool(t)
            elif r < 0.58:
                out = self.pool(t)
            elif r < 0.72:
                out = self.conv_i8(t)
            elif r < 0.9:
                out = self.depthwise_i8(t)
            elif t.c <= 192:
                out = self.join(t)
            else:
                out = self.pool(t)
        if out is not None and out.producer is not None and out.kind != "bits" and self.nodes[out.producer].name in P.FOLDING and g.random() < 0.6:
            self.fold_variants(out)

    def grow(self):
        g = self.g
        while self.left() >= 1:
            self.step()
        if self.head:
            ends = [t for t in self.tensors if t.kind != "bits" and not t.rank2 and t.c != 3 and not t.readers] or \
                   [t for t in self.tensors if t.kind != "bits" and not t.rank2 and t.c != 3]
            if ends:
                kind = "i8" if (g.random() < 0.5 and any(t.kind == "i8" for t in ends)) else ends[int(g.integers(0, len(ends)))].kind
                ends = [t for t in ends if t.kind == kind]
                t = ends[int(g.integers(0, len(ends)))]
                (self.float_head if t.kind == "f32" else self.int8_head)(t)
        for t in self.tensors:
            if not t.readers and t is not self.x:
                t.output = True

    # ---- the file -------------------------------------------------------------------------------------------------------------------------------
    def order(self):
        """A random topological order of the operators."""
        g = self.g
        waiting = {k: {t.producer for t in n.ins if t.producer is not None} for k, n in enumerate(self.nodes)}
        order = []
        while waiting:
            ready = sorted(k for k, deps in waiting.items() if not deps)
            ready = [k for k in ready if self.nodes[k].after is None or self.nodes[k].after in order] or ready
            k = ready[int(g.integers(0, len(ready)))]
            order.append(k)
            del waiting[k]
            for deps in waiting.values():
                deps.discard(k)
        return order

    def write(self):
        b = M.QModelBuilder()
        F = {}
        for t in self.tensors:
            kw = dict(scale=t.q[0], zero_point=t.q[1]) if t.kind == "i8" else {}
            F[t.n] = b.tensor(t.shape, t.dtype, "t%d" % t.n, **kw)
        order = self.order()
        for k in order:
            n = self.nodes[k]
            at = n.emit(b, [F[t.n] for t in n.ins], F[n.out.n])
            assert at == len(b.ops) - 1
        b.inputs = [F[self.x.n]]
        b.outputs = [F[t.n] for t in self.tensors if t.output]
        return b, F, order


def _tensor_lists(b):
    return [(list(op.fields[1].items), list(op.fields[2].items)) for op in b.ops]


@functools.lru_cache(maxsize=None)
def build(seed):
    """The model of `seed`: a dict with data (the file), x (the seed's input: batch + 2 images), batch, input / outputs (tensor
    indices), ops [(inputs, outputs)], constants, names (per operator: its LCE name, or the pass that takes it with every flag),
    alts (per operator: [(keyword, pass)] in the library's priority order), forward(x) -> {tensor: array}, host {operator:
    closure over its non-constant inputs}, kinds(flags), types {tensor: 'f32' | 'i8' | 'bits'}, channels, features, nan_ok."""
    gen = _Gen(seed)
    gen.grow()
    b, F, order = gen.write()
    nodes = [gen.nodes[k] for k in order]
    ops = _tensor_lists(b)
    live = {F[t.n] for t in gen.tensors}
    constants = {t for ins, _ in ops for t in ins if t >= 0 and t not in live}
    wiring = [([F[t.n] for t in n.ins], F[n.out.n], n.fn) for n in nodes]
    for (ins, out, _), (all_ins, outs) in zip(wiring, ops):
        assert ins == [t for t in all_ins if t in live] and outs == [out]
    x_t = F[gen.x.n]

    def forward(x):
        vals = {x_t: x}
        with np.errstate(all="ignore"):
            for ins, out, fn in wiring:
                vals[out] = fn(*[vals[t] for t in ins])
        return vals

    def kinds(flags):
        return [n.name if n.name in P.LCE_OPS else next((kind for flag, kind in n.alts if flags.get(flag)), None) for n in nodes]
    readers = P.readers_of(ops)
    features = dict(gen.features)
    # (e) and (f) are read off the restated walk of the one section: a chain that ran into the cap, a chain that stopped at an
    # operand the file order put further down
    one = P.partition(ops, kinds(EVERY_FLAG), constants, [F[t.n] for t in gen.tensors if t.output], True)
    bit_tensors = {F[t.n] for t in gen.tensors if t.kind == "bits"}
    walks = [P.expected_counters(s, ops, kinds(EVERY_FLAG), constants, bit_tensors) for s in one]
    chains = [c for wk in walks for c in wk["chains"]]
    features["e"] = sum(1 for _, why in chains if why == "cap")
    features["f"] = sum(1 for _, why in chains if why == "operand")
    # (a) to (d) and (j) are read off the graph: the readers of every tensor a folding pass or an LceBconv2d writes
    outputs = set(b.outputs)
    for k, n in enumerate(nodes):
        t = ops[k][1][0]
        rd = readers.get(t, [])
        quants = [r for r in rd if nodes[r].name == "LceQuantize"]
        is_pass = n.name in P.FOLDING and t not in bit_tensors
        features["a"] += is_pass and len(rd) == 1 and len(quants) == 1 and t not in outputs
        features["b"] += is_pass and len(rd) == 1 and len(quants) == 1 and t in outputs
        features["c"] += (is_pass or (n.name == "LceBconv2d" and t not in bit_tensors)) and len(quants) >= 2
        features["d"] += is_pass and len(quants) >= 1 and any(nodes[r].name in P.PASSES for r in rd)
    # (g), (h) and (k) too: two LceBconv2d that read one bit tensor and whose results meet in one ADD or CONCATENATION; the joins
    # and what their input lists hold; model outputs of more than one kind
    types = {F[t.n]: t.kind for t in gen.tensors}
    channels = {F[t.n]: t.c for t in gen.tensors}
    source = {ops[k][1][0]: ops[k][0][0] for k, n in enumerate(nodes) if n.name == "LceBconv2d"}
    features.update(g=0, h=0, k=int(len({types[t] for t in outputs}) > 1), **{name: 0 for name in JOIN_FEATURES})
    for k, n in enumerate(nodes):
        if n.name not in ("elementwise", "int8_add", "concat"):
            continue
        ins = [t for t in ops[k][0] if t >= 0 and t not in constants]
        branches = sorted({t for t in ins if t in source})
        features["g"] += any(source[a] == source[c] for a in branches for c in branches if a < c)
        if n.name == "concat":
            ragged = any(channels[t] % 32 for t in ins)
            features["h"] += 1
            features["h_wide"] += len(ins) >= 4
            features["h_max"] += len(ins) == CONCAT_MAX
            features["h_dup"] += len(set(ins)) < len(ins)
            features["h_ragged_f32"] += ragged and types[ins[0]] == "f32"
            features["h_ragged_i8"] += ragged and types[ins[0]] == "i8"
    features["j"] = int(any(nodes[r].name != "LceQuantize" for r in readers.get(x_t, [])))
    features = {k: int(v) for k, v in features.items()}
    x = gen.x.val
    only_quantize = all(nodes[r].name == "LceQuantize" for r in readers.get(x_t, [])) and gen.x.kind == "f32"
    if only_quantize:
        x = x.copy()
        x[0, 0, 0, :3] = (np.nan, np.inf, -np.inf)
    return dict(seed=seed, data=b.finish(), x=x, batch=gen.batch, input=x_t, outputs=list(b.outputs), ops=ops, constants=constants,
                names=kinds(EVERY_FLAG), alts=[n.alts for n in nodes], forward=forward, host={k: fn for k, (_, _, fn) in enumerate(wiring)},
                kinds=kinds, types={F[t.n]: t.kind for t in gen.tensors}, channels={F[t.n]: t.c for t in gen.tensors}, features=features,
                bit_tensors=bit_tensors, chains=chains, nan_ok=only_quantize)


def violations(info):
    """The conditions on a draw, checked on the reference alone: every float tensor finite (but for the special values planted in
    an input that only LceQuantize reads), every int8 tensor spread (32 distinct values, or half as many as it has elements when it
    has fewer than 64; no value on more than half of them), every bit tensor with 20 % to 80 % ones, and outputs that differ
    between image 0 and image 1.  Returns the list of what fails: empty for a kept seed."""
    bad = []
    vals = info["forward"](info["x"])
    for t, v in sorted(vals.items()):
        kind = info["types"][t]
        if kind == "f32":
            if not np.isfinite(v).all() and not (t == info["input"] and info["nan_ok"]):
                bad.append("tensor %d is not finite" % t)
        elif kind == "i8":
            values, counts = np.unique(v, return_counts=True)
            if values.size < (32 if v.size >= 64 else (v.size + 1) // 2):
                bad.append("int8 tensor %d takes %d values" % (t, values.size))
            if counts.max() > v.size / 2:
                bad.append("int8 tensor %d holds one value in %d of %d places" % (t, counts.max(), v.size))
        else:
            share = ones_share(v, info["channels"][t])
            if not 0.2 <= share <= 0.8:
                bad.append("bit tensor %d has %.0f %% ones" % (t, 100 * share))
    for t in info["outputs"]:
        if np.array_equal(vals[t][0].view(np.uint8), vals[t][1].view(np.uint8)):
            bad.append("output %d is the same for images 0 and 1" % t)
    if not 6 <= len(info["ops"]) <= 20:
        bad.append("%d operators" % len(info["ops"]))
    return bad


# The suite's cases: the seeds of range(CANDIDATES) that meet the conditions (tests/test_random_models_host.py checks that this is
# the list, so a dropped seed is dropped by the conditions and by nothing else).
CANDIDATES = 56
SEEDS = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 18, 19, 20, 22, 23, 24, 25, 27, 28, 29, 30, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41,
         42, 43, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55)


def fuzz_seeds():
    """Freshly drawn seeds for a longer hunt, kept under the same conditions (see _fuzz)."""
    return _fuzz()[0]


def fuzz_dropped():
    """(how many freshly drawn seeds the conditions dropped, how many were drawn): the cap of one in four holds for them too."""
    return _fuzz()[1:]


@functools.lru_cache(maxsize=None)
def _fuzz():
    """Read as tests/test_gpu_model_random.py reads them: either variable starts a hunt, LCE_FUZZ_EXAMPLES (default 80) draws
    from LCE_FUZZ_SEED (default 0).  With neither the suite is the fixed list."""
    if "LCE_FUZZ_SEED" not in os.environ and "LCE_FUZZ_EXAMPLES" not in os.environ:
        return [], 0, 0
    base, count = int(os.environ.get("LCE_FUZZ_SEED", "0")), int(os.environ.get("LCE_FUZZ_EXAMPLES", "80"))
    start = 1000003 * (base + 1)
    kept = [s for s in range(start, start + max(count, 0)) if not violations(build(s))]
    print("random_models: %d fuzz seeds drawn from %d, %d dropped by the conditions" % (count, start, count - len(kept)))
    return kept, max(count, 0) - len(kept), max(count, 0)


def cut_flags(seed):
    """The seed's own subset of the keywords: every keyword but a random third of them (at least one is dropped), which cuts the
    file into sections at places no fixture has them."""
    g = np.random.default_rng(seed + 100003)
    names = sorted(EVERY_FLAG)
    dropped = [n for n in names if g.random() < 0.35] or [names[int(g.integers(0, len(names)))]]
    return {n: True for n in names if n not in dropped}


def reference_partition(info, flags):
    """partition_ref's sections of the seed's file under `flags`."""
    return P.partition(info["ops"], info["kinds"](flags), info["constants"], info["outputs"], bool(flags.get("stem_sections")))


def expected_stats(info, flags=None, section=0):
    """What the *_stats() entries and run_stats()[1] report after a run of `section` under `flags` (default: every keyword),
    keyed as the tests read them."""
    flags = EVERY_FLAG if flags is None else flags
    kinds = info["kinds"](flags)
    c = P.expected_counters(reference_partition(info, flags)[section], info["ops"], kinds, info["constants"], info["bit_tensors"])
    n, f = c["passes"], c["folded"]
    pair = lambda k: (n[k], f[k])
    return dict(elementwise=(n["elementwise"], c["ew_ops"], f["elementwise"]), int8_add=pair("int8_add"), concat=pair("concat"), pool=pair("pool"),
                conv1x1=pair("conv1x1"), depthwise=pair("depthwise"), conv2d=pair("conv2d"), conv_i8=pair("conv_i8"),
                depthwise_i8=pair("depthwise_i8"), head=(n["mean"], n["fully_connected"], n["softmax"]),
                head_i8=(n["mean_i8"], n["fully_connected_i8"], n["softmax_i8"]), quantize=(n["quantize"], n["dequantize"]),
                fused_quantize=c["conv_quantize"])


def model_stats(model):
    """The same dict read from a model_runner.LceModel after a run."""
    return dict(elementwise=model.elementwise_stats(), int8_add=model.int8_add_stats(), concat=model.concat_stats(), pool=model.pool_stats(),
                conv1x1=model.conv1x1_stats(), depthwise=model.depthwise_stats(), conv2d=model.conv2d_stats(), conv_i8=model.conv_i8_stats(),
                depthwise_i8=model.depthwise_i8_stats(), head=model.head_stats(), head_i8=model.head_i8_stats(), quantize=model.quantize_stats(),
                fused_quantize=model.run_stats()[1])


def run_cut(info, sections, x, run_section):
    """The seed's file cut into `sections` [(operators, inputs, outputs)]: every operator outside them through info["host"] in
    NumPy, every section through run_section(index, [input arrays]) -> [output arrays], each as soon as what it reads is there
    (a section's first operator may stand in the file in front of a host operator another of its members waits for).  Returns
    tensor -> array for every tensor that crossed the host."""
    ops, constants = info["ops"], info["constants"]
    variable = lambda i: [t for t in ops[i][0] if t >= 0 and t not in constants]
    inside = {i for members, _, _ in sections for i in members}
    units = [("host", i) for i in range(len(ops)) if i not in inside] + [("section", k) for k in range(len(sections))]
    live = {info["input"]: x}
    while units:
        ready = [u for u in units if all(t in live for t in (variable(u[1]) if u[0] == "host" else sections[u[1]][1]))]
        assert ready, "the cut cannot be scheduled"
        for what, k in ready:
            if what == "host":
                live[ops[k][1][0]] = info["host"][k](*[live[t] for t in variable(k)])
            else:
                live.update(zip(sections[k][2], run_section(k, [live[t] for t in sections[k][1]])))
            units.remove((what, k))
    return live
