"""Builders for the channel slices of MeliusNet's improvement block on tests/tflite_writer.py -- STRIDED_SLICE with its
StridedSliceOptions table attached as head_models.fc_op attaches its own, and SLICE -- and the fixture models of the slice tests.
Every operator a builder adds is recorded with its NumPy restatement, so one evaluator gives the forward pass of every fixture
and what the host does for the operators outside the sections.  No tests here."""
import numpy as np

import int8_add_ref as R
import oracle_lib as O
import synth
from section_models import ADD, MUL, NONE, RELU, _conv, concat_op, ew_op, float_op
from tflite_writer import ModelBuilder, _Scalar, _Table, _Vector

# schema.fbs BuiltinOperator / BuiltinOptions
STRIDED_SLICE, SLICE = 45, 65
STRIDED_SLICE_OPTIONS = 32
INT8_Q = (0.25, -3)                     # the ONE scale and zero point of every int8 tensor behind the input
INPUT_Q = (0.5, 4)
GROWTH = 64                             # channels of every binary layer's output, and of the window the improvement block updates
FLOAT_NAMES = dict(elementwise_sections=True, concat_sections=True, slice_sections=True)
INT8_NAMES = dict(int8_add_sections=True, concat_sections=True, slice_sections=True)


def strided_slice_op(b: ModelBuilder, inputs, outputs, begin_mask=0, end_mask=0, ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=0,
                     offset=False, options=True) -> int:
    """A builtin STRIDED_SLICE with its StridedSliceOptions table (0 begin_mask, 1 end_mask, 2 ellipsis_mask, 3 new_axis_mask,
    4 shrink_axis_mask, 5 offset) -- or without one when options is False."""
    fields = {0: _Scalar("I", b._code(None, STRIDED_SLICE)), 1: _Vector("i", list(inputs)), 2: _Vector("i", list(outputs))}
    if options:
        fields[3] = _Scalar("B", STRIDED_SLICE_OPTIONS)
        fields[4] = _Table({0: _Scalar("i", begin_mask), 1: _Scalar("i", end_mask), 2: _Scalar("i", ellipsis_mask),
                            3: _Scalar("i", new_axis_mask), 4: _Scalar("i", shrink_axis_mask), 5: _Scalar("B", 1 if offset else 0)})
    b.ops.append(_Table(fields))
    return len(b.ops) - 1


def resolve(extent, begin, end, begin_masked=False, end_masked=False):
    """The (begin, count) of a stride-1 range, by Python's own slicing."""
    r = range(extent)[None if begin_masked else begin:None if end_masked else end]
    return (r.start, len(r)) if len(r) else (0, 0)


class Net:
    """A ModelBuilder that records, per operator, (its non-constant inputs, its output, its NumPy restatement)."""

    def __init__(self, dtype=np.float32, H=8, C0=64, seed=0, batch=1):
        self.b = ModelBuilder()
        self.i8 = np.dtype(dtype) == np.int8
        self.dtype, self.H, self.batch = dtype, H, batch
        self.n = seed * 100
        self.run = {}                       # operator -> (input tensors, output tensor, function of the input arrays)
        self.zp, self.channels = {}, {}
        self.kinds = {}                     # operator -> a word for what it is ("slice", "improve_add", "join", ...)
        self.x0 = self.tensor(C0, "x", INPUT_Q)

    def tensor(self, c, name, q=INT8_Q, h=None):
        h = self.H if h is None else h
        kw = dict(scale=q[0], zero_point=q[1]) if self.i8 else {}
        t = self.b.tensor([self.batch, h, h, c], self.dtype, name, **kw)
        self.zp[t], self.channels[t] = (q[1] if self.i8 else 0), c
        return t

    def record(self, op, ins, out, fn, kind):
        self.run[op] = (list(ins), out, fn)
        self.kinds[op] = kind
        return out

    def binary(self, src, cout=GROWTH):
        """LceQuantize -> LceBconv2d (3x3 SAME, one-padding) of `src`."""
        self.n += 1
        c = self.channels[src]
        q = self.b.tensor([self.batch, self.H, self.H, (c + 31) // 32], np.int32, "q%d" % self.n)
        zp = self.zp[src]
        self.record(self.b.custom_op("LceQuantize", [src], [q], b""), [src], q, lambda v: O.bitpack(v, zp), "quantize")
        y, cv = _conv(self.b, q, self.H, c, cout, self.n, out_type=self.dtype, quant=INT8_Q if self.i8 else None)
        self.zp[y], self.channels[y] = (INT8_Q[1] if self.i8 else 0), cout
        if self.i8:
            fn = lambda bits: O.bconv2d(cv["spec"].with_batch(bits.shape[0]), O.DST_I8, bits, cv["w"], cv["m"], cv["b"], out_scale=INT8_Q[0],
                                        out_zero_point=INT8_Q[1])
        else:
            fn = lambda bits: O.bconv2d(cv["spec"].with_batch(bits.shape[0]), O.DST_F32, bits, cv["w"], cv["m"], cv["b"])
        return self.record(len(self.b.ops) - 1, [q], y, fn, "bconv")

    def bn(self, src):
        """The float batch norm in front of an LceQuantize: MUL by [C], ADD of [1,1,1,C]."""
        self.n += 1
        c = self.channels[src]
        g = synth.rng(self.n + 1000)
        m, a = g.uniform(0.5, 1.5, c).astype(np.float32), g.standard_normal(c).astype(np.float32)
        f32 = lambda shape, name, data: self.b.tensor(shape, np.float32, name, data)
        mm, out = self.tensor(c, "bnm%d" % self.n), self.tensor(c, "bna%d" % self.n)
        self.record(ew_op(self.b, MUL, [src, f32([c], "bn_mul%d" % self.n, m)], [mm], NONE), [src], mm, lambda v: float_op(v, MUL, m, NONE), "bn")
        return self.record(ew_op(self.b, ADD, [mm, f32([1, 1, 1, c], "bn_add%d" % self.n, a.reshape(1, 1, 1, c))], [out], NONE), [mm], out,
                           lambda v: float_op(v, ADD, a.reshape(1, 1, 1, -1), NONE), "bn")

    def slice(self, src, begin, count, form="masked"):
        """The channels [begin, begin + count) of `src`, written in one of the forms a converter may choose: `masked` (axes 0..2
        masked on both sides), `negative` (the channel range counted from the end, its end masked), `plain` (every index written
        out) or `slice` (the builtin SLICE with sizes of -1 for the whole axes)."""
        self.n += 1
        c, H, B = self.channels[src], self.H, self.batch
        i32 = lambda name, v: self.b.tensor([4], np.int32, "%s%d" % (name, self.n), np.array(v, np.int32))
        out = self.tensor(count, "window%d" % self.n, (INT8_Q[0], self.zp[src]))
        if form == "slice":
            op = self.b.builtin_op(SLICE, [src, i32("begin", [0, 0, 0, begin]), i32("size", [-1, H, -1, count])], [out])
        else:
            if form == "masked":
                v, masks = ([5, 7, -2, begin], [1, 2, 3, begin + count]), (7, 7)
            elif form == "negative":
                v, masks = ([0, 0, 0, begin - c], [B, H, H, 0]), (0, 8)
                assert begin + count == c
            else:
                v, masks = ([0, 0, 0, begin], [B, H, H, begin + count]), (0, 0)
            op = strided_slice_op(self.b, [src, i32("begin", v[0]), i32("end", v[1]), i32("strides", [1, 1, 1, 1])], [out], masks[0], masks[1])
        return self.record(op, [src], out, lambda x: np.ascontiguousarray(x[..., begin:begin + count]), "slice")

    def add(self, t1, t2, act=NONE, kind="add"):
        """TFLite's ADD of two tensors of one shape: float32 (one rounding, then the activation) or int8 (its integer arithmetic)."""
        self.n += 1
        out = self.tensor(self.channels[t1], "sum%d" % self.n)
        if self.i8:
            q = (INT8_Q[0], self.zp[t1], INT8_Q[0], self.zp[t2]) + INT8_Q
            fn = lambda a, c: R.add_q(a, c, q, act)
        else:
            fn = lambda a, c: float_op(a, ADD, c, act)
        return self.record(ew_op(self.b, ADD, [t1, t2], [out], act), [t1, t2], out, fn, kind)

    def scale(self, src, factor):
        """MUL by a scalar constant: an operator of the elementwise chain."""
        self.n += 1
        out = self.tensor(self.channels[src], "scaled%d" % self.n)
        k = self.b.tensor([1], np.float32, "factor%d" % self.n, np.array([factor], np.float32))
        return self.record(ew_op(self.b, MUL, [src, k], [out], NONE), [src], out, lambda v: float_op(v, MUL, np.float32(factor), NONE), "scale")

    def concat(self, ts, kind="join"):
        self.n += 1
        out = self.tensor(sum(self.channels[t] for t in ts), "joined%d" % self.n)
        return self.record(concat_op(self.b, ts, [out]), ts, out, lambda *xs: np.concatenate(xs, axis=-1), kind)

    def dense(self, x):
        """A dense block: CONCATENATION([x, LceBconv2d(LceQuantize(BN(x)))])."""
        return self.concat([x, self.binary(x if self.i8 else self.bn(x))], "dense_join")

    def improve(self, x, forms=("masked", "negative"), act=NONE, scaled=False):
        """MeliusNet's improvement block: the last GROWTH channels of x get LceBconv2d(LceQuantize(BN(x))) added."""
        c = self.channels[x]
        w = self.binary(x if self.i8 else self.bn(x))
        f = self.slice(x, 0, c - GROWTH, forms[0])
        t = self.slice(x, c - GROWTH, GROWTH, forms[1])
        if scaled:
            w = self.scale(w, 0.5)
        return self.concat([f, self.add(t, w, act, "improve_add")], "improve_join")

    def finish(self, outputs):
        self.b.inputs, self.b.outputs = [self.x0], list(outputs)
        return self.b.finish()

    def ops_of(self, *kinds):
        return [k for k, v in sorted(self.kinds.items()) if v in kinds]

    def forward(self, x):
        """tensor -> array for every tensor of the graph, from the input `x`."""
        live = {self.x0: x}
        for op in sorted(self.run):
            ins, out, fn = self.run[op]
            live[out] = fn(*[live[t] for t in ins])
        return live


def meliusnet_model(dtype=np.float32, H=8, seed=0, forms=("masked", "negative")):
    """A MeliusNet-style body: x [1,H,H,64] -> a binary layer, then twice { dense block, improvement block }: the channels go
    64 -> 128 -> 128 -> 192 -> 192.  float32: a batch norm (MUL, ADD) stands in front of every LceQuantize and the last joined
    tensor is the graph output.  int8: every LceQuantize reads the joined tensor directly, the ADD is TFLite's int8 ADD -- so the `f`
    slice folds into the join and the `b` slice runs standalone into the ADD -- and a last binary layer reads the last join.
    Returns (file, net, output tensor)."""
    net = Net(dtype, H, seed=seed)
    x = net.binary(net.x0)
    for _ in range(2):
        x = net.improve(net.dense(x), forms)
    if net.i8:
        x = net.binary(x)
    return net.finish([x]), net, x


def variant_model(case, seed=0):
    """One improvement-shaped block behind a binary layer 64 -> 128, bent one way each.  Returns (file, net, graph outputs).
      quantize_reader  a slice read only by an LceQuantize (-> LceBconv2d)
      delivered        CONCATENATION([b, f]) with f a graph output too
      two_readers      f is read by the CONCATENATION and by an LceQuantize (-> LceBconv2d, a second output)
      relu_add         the improvement block with a fused RELU on its ADD
      chain_addend     the improvement block whose addend comes from a MUL of the elementwise chain
      slice_op         the improvement block with builtin SLICE operators
      plain            the improvement block with every index written out"""
    net = Net(np.float32, seed=seed)
    x = net.binary(net.x0, 2 * GROWTH)
    if case == "quantize_reader":
        outs = [net.binary(net.slice(x, GROWTH, GROWTH))]
    elif case == "delivered":
        f, t = net.slice(x, 0, GROWTH), net.slice(x, GROWTH, GROWTH, "negative")
        outs = [net.concat([t, f]), f]
    elif case == "two_readers":
        f, t = net.slice(x, 0, GROWTH), net.slice(x, GROWTH, GROWTH)
        outs = [net.concat([f, t]), net.binary(f)]
    elif case == "relu_add":
        outs = [net.improve(x, act=RELU)]
    elif case == "chain_addend":
        outs = [net.improve(x, scaled=True)]
    elif case == "slice_op":
        outs = [net.improve(x, forms=("slice", "slice"))]
    elif case == "plain":
        outs = [net.improve(x, forms=("plain", "plain"))]
    else:
        raise KeyError(case)
    return net.finish(outs), net, outs


VARIANTS = ("quantize_reader", "delivered", "two_readers", "relu_add", "chain_addend", "slice_op", "plain")
# (lce_hip_join_windows launches, LceQuantize folded, those that took over a CONCATENATION), lce_hip_concat launches and
# lce_hip_elementwise launches a run of each variant makes with `elementwise,concat,slice`
VARIANT_STATS = dict(quantize_reader=((1, 1, 0), 0, 0), delivered=((2, 0, 1), 0, 0), two_readers=((2, 1, 1), 0, 0),
                     relu_add=((2, 0, 1), 0, 2), chain_addend=((2, 0, 1), 0, 2), slice_op=((1, 0, 1), 0, 1), plain=((1, 0, 1), 0, 1))

REFUSALS = ("stride_2", "window_on_h", "batch_range", "shrink_mask", "ellipsis_mask", "new_axis_mask", "offset_true", "length_3",
            "dynamic_begin", "declared_output", "int32_tensor", "constant_input", "no_options", "empty_window", "slice_negative_begin",
            "slice_past_the_end", "slice_dynamic_size", "requantizing")
CONTROLS = ("masked", "negative", "plain", "slice", "slice_to_the_end", "int8", "one_channel", "clamped")


def single_op_model(case, H=4, C=96):
    """x (the graph input) -> STRIDED_SLICE / SLICE -> y -> LceQuantize -> the graph output: with `stem` and `slice` named the
    section holds both operators when the slice qualifies and the LceQuantize alone when it does not.  Returns (file, the
    slice's operator index, the window (begin, count) a qualifying slice cuts)."""
    b = ModelBuilder()
    B = 2 if case == "batch_range" else 1
    dtype = np.int32 if case == "int32_tensor" else np.int8 if case in ("int8", "requantizing") else np.float32
    q = dict(scale=0.5, zero_point=3) if dtype == np.int8 else {}
    data = np.zeros((B, H, H, C), np.float32) if case == "constant_input" else None
    x = b.tensor([B, H, H, C], dtype, "x", data, **q)
    i32 = lambda name, v: b.tensor([len(v)], np.int32, name, np.array(v, np.int32))
    begin, end, strides = [0, 0, 0, 32], [B, H, H, 64], [1, 1, 1, 1]
    masks, opt, shape, extra_inputs = dict(), True, [B, H, H, 32], []
    window = (32, 32)
    code = SLICE if case.startswith("slice") else STRIDED_SLICE
    if case == "stride_2":
        strides, shape = [1, 1, 1, 2], [B, H, H, 16]
    elif case == "window_on_h":
        begin, end, shape = [0, 1, 0, 0], [B, 3, H, C], [B, 2, H, C]
    elif case == "batch_range":
        end, shape = [1, H, H, 64], [1, H, H, 32]
    elif case == "shrink_mask":
        masks = dict(shrink_axis_mask=1)
    elif case == "ellipsis_mask":
        masks = dict(ellipsis_mask=2)
    elif case == "new_axis_mask":
        masks = dict(new_axis_mask=1)
    elif case == "offset_true":
        masks = dict(offset=True)
    elif case == "length_3":
        begin, end, strides = begin[1:], end[1:], strides[1:]
    elif case == "declared_output":
        shape = [B, H, H, 31]
    elif case == "no_options":
        opt = False
    elif case == "empty_window":
        begin, end, shape = [0, 0, 0, 64], [B, H, H, 64], [B, H, H, 1]
    elif case == "requantizing":
        q = dict(scale=0.25, zero_point=3)
    elif case == "masked":
        begin, end, masks = [3, -1, 9, 32], [0, 0, 0, 64], dict(begin_mask=7, end_mask=7)
    elif case == "negative":
        begin, end, masks, shape, window = [0, 0, 0, -32], [B, H, H, 0], dict(end_mask=8), [B, H, H, 32], (C - 32, 32)
    elif case == "one_channel":
        begin, end, shape, window = [0, 0, 0, C - 1], [B, H, H, C], [B, H, H, 1], (C - 1, 1)
    elif case == "clamped":
        begin, end, shape, window = [-9, 0, 0, -500], [B + 7, 1000, H, 500], [B, H, H, C], (0, C)
    elif case == "slice":
        end = [B, H, H, 32]                                           # (SLICE's third operand is the size)
    elif case == "slice_to_the_end":
        end, shape, window = [-1, -1, -1, -1], [B, H, H, C - 32], (32, C - 32)
    elif case == "slice_negative_begin":
        begin, end = [0, 0, 0, -64], [B, H, H, 32]
    elif case == "slice_past_the_end":
        begin, end, shape = [0, 0, 0, 80], [B, H, H, 32], [B, H, H, 16]
    elif case in ("slice_dynamic_size", "dynamic_begin"):
        pass
    y = b.tensor(shape, dtype, "y", **q)
    t_begin = b.tensor([4], np.int32, "begin") if case == "dynamic_begin" else i32("begin", begin)
    t_end = b.tensor([4], np.int32, "size") if case == "slice_dynamic_size" else i32("end", end)
    if case in ("dynamic_begin", "slice_dynamic_size"):
        extra_inputs = [t_begin if case == "dynamic_begin" else t_end]
    if code == SLICE:
        k = b.builtin_op(SLICE, [x, t_begin, t_end], [y])
    else:
        k = strided_slice_op(b, [x, t_begin, t_end, i32("strides", strides)], [y], options=opt, **masks)
    bits = b.tensor(shape[:3] + [(shape[3] + 31) // 32], np.int32, "bits")
    b.custom_op("LceQuantize", [y], [bits], b"")
    b.inputs, b.outputs = ([] if case == "constant_input" else [x]) + extra_inputs, [bits]
    return b.finish(), k, window
