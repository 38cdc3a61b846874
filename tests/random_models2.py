"""The second generation of tests/random_models.py, for tests/test_v2_random_models_host.py and tests/test_gpu_random_models2.py: the
same seeded generator of random mixed float / int8 / bitpacked networks, growing over all 25 rows of the library's pass table and
the "transition" fusion.  No tests here.

`_Gen2` subclasses `_Gen` and leaves it untouched (tests/golden/random_models_gen1_digests.json holds generation 1's files).  Its
growth table offers every transition of the old one (`_Gen.step`) and, counted as features like a-k:
  l  a standalone float activation (RELU, RELU_N1_TO_1, RELU6, LOGISTIC, PRELU) inside an ADD / MUL chain;
  m  a per-image float gate: MEAN -> (FULLY_CONNECTED | 1x1 CONV_2D) -> LOGISTIC (-> RESHAPE) -> MUL / ADD onto the image, and the
     1x1-image case where the gate is a tensor operand;
  n  a RESHAPE that flattens into the float or int8 head, or whose result is a model output;
  o  a binary Dense layer: LceQuantize -> LceDequantize -> FULLY_CONNECTED on +-s weights (powers of two: the bytes then do not
     depend on whether `binary_dense` or `head` takes the layer), with the variants skipped / second reader / refused / ragged;
  p  MeliusNet's improvement block on float and int8 tensors: a channel window, an ADD onto it, the CONCATENATION that reassembles;
  q  an int8 chain of ADD constant / PRELU / RELU* / QUANTIZE, behind a residual ADD (the head) or not, folding or not;
  r  the int8 gate: MEAN -> (FULLY_CONNECTED | CONV_2D) -> LOGISTIC -> MUL, a MUL of two tensors, each with or without a rider ADD;
  s  the transition: MAX_POOL_2D 2x2 / 1 SAME -> DEPTHWISE_CONV_2D 3x3 / 2 and its neighbours that do not fuse.
Every value is evaluated while growing with the NumPy restatements of the passes' own tests, and the constants are calibrated on
the values the operator really sees.  A file holds 6 to 24 operators (generation 1: 20; a gate block alone is six)."""
import functools
import os

import numpy as np

import activation_models as AM
import activation_ref as AR
import binary_dense_models as BM
import binary_dense_ref as BR
import conv1x1_ref as C1
import conv2d_i8_ref as CI
import elementwise_i8_ref as E
import gate_i8_ref as G
import head_i8_models as HIM
import head_i8_ref as HI
import head_models as HM
import head_ref as HR
import int8_add_ref as A
import int8_conv_models as M
import oracle_lib as O
import partition_ref as P
import partition_ref2 as P2
import pool_ref as PR
import random_models as RM
import slice_models as SM
from random_models import f32
from section_models import (ADD, AVERAGE_POOL_2D, MAX_POOL_2D, MUL, NONE, RELU, RELU6, RELU_N1_TO_1, SAME, VALID, concat_op, conv2d_op, ew_op,
                            float_op, pool_op)
from tflite_writer import _Scalar, _Table, _Vector

# the keywords of model_runner.LceModel and the three names that arrive through passes=
PASS_NAMES = ("elementwise_i8", "gate_i8", "transition")
EVERY_FLAG = dict(RM.EVERY_FLAG, activation_sections=True, reshape_sections=True, gate_sections=True, binary_dense_sections=True,
                  slice_sections=True, **{n: True for n in PASS_NAMES})
FLAG_OF = dict(RM.FLAG_OF, activation="activation_sections", reshape="reshape_sections", gate="gate_sections", binary_dense="binary_dense_sections",
               slice="slice_sections", elementwise_i8="elementwise_i8", logistic_i8="gate_i8", mul_i8="gate_i8")
assert set(FLAG_OF) == set(P2.PASSES) and len(P2.PASSES) == 25 and set(FLAG_OF.values()) | {"stem_sections", "transition"} == set(EVERY_FLAG)
CHANNELS = RM.CHANNELS + (48, 80)
FEATURES = RM.FEATURES + "lmnopqrs"
JOIN_FEATURES = RM.JOIN_FEATURES
# the fusing and the non-fusing variants of o, q, r and s, each counted apart
CLAMPS = ("q_relu", "q_relu_n1_to_1", "q_relu6")                      # the int8 chain's three clamp steps: each in at least one kept seed
VARIANTS = ("l_cap", "o_skipped", "o_second_reader", "o_refused", "o_ragged", "q_head", "q_no_head", "q_fold", "r_gate", "r_tensor", "r_rider", "r_no_rider",
            "s_fused", "s_average", "s_second_reader", "s_delivered", "s_int8", "s_row")
MUST = ("s0", "s1", "s5", "s3", "s2", "p_f32", "p_i8", "o2", "o3", "q_head", "q_no_head", "s5")
ACTIVATION_KINDS = ("relu", "relu_n1_to_1", "relu6", "logistic", "prelu")
MAX_OPS = 24
QUANTIZE_OP = 114


def model_args(flags):
    """(passes, keywords) for model_runner.LceModel / Interpreter from a dict over EVERY_FLAG's names."""
    return tuple(n for n in PASS_NAMES if flags.get(n)), {k: True for k, v in flags.items() if v and k not in PASS_NAMES}


class _T2(RM._T):
    @property
    def shape(self):
        c = (self.c + 31) // 32 if self.kind == "bits" else self.c
        return [1, c] if (self.rank2 and not self.keep_dims) else [1, self.h, self.w, c]


class _Gen2(RM._Gen):
    def __init__(self, seed):
        self.seed = seed
        self.g = g = np.random.default_rng(seed)
        self.tensors, self.nodes = [], []
        self.features = {k: 0 for k in FEATURES}
        self.features.update({k: 0 for k in VARIANTS + CLAMPS})
        self.batch = int(g.choice([1, 3, 8]))
        self.images = self.batch + 2
        self.budget = int(g.integers(6, MAX_OPS + 1))
        self.head = bool(g.integers(0, 2))
        self.budget = max(self.budget, 8) if self.head else self.budget
        self.want = {k for k in "efiw" if g.random() < (0.5 if k == "w" else 0.3)}
        self.want2 = [k for k in g.permutation(list("lmnopqrs")) if g.random() < (0.8 if k == "o" else 0.9 if k == "s" else 0.6 if k in "mp" else 0.25 if k == "n" else 0.4)]
        # the seed's own block, grown first while there is room: the variants of o, p, q and s take turns with the seed, so that each is
        # met across the kept seeds whatever the other draws do
        self.must = MUST[seed % len(MUST)]
        self.budget = max(self.budget, 14)
        self.long_l = g.random() < 0.3                                 # (l) a chain with activations that runs past the cap
        self.budget = max(self.budget, 18) if "e" in self.want else self.budget
        self.budget = max(self.budget, 20) if self.long_l else self.budget
        self.budget = max(self.budget, 10 + 2 * len(self.want2)) if self.want2 else self.budget
        self.budget = min(self.budget, MAX_OPS)
        self._window = None
        h = int(g.integers(5, 13))
        w = h if g.random() < 0.3 else int(g.integers(5, 13))
        c = int(g.choice((3, 3) + CHANNELS))
        shape = (self.images, h, w, c)
        if g.random() < 0.5:
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
        t = _T2(len(self.tensors), kind, val, c, q, **kw)
        self.tensors.append(t)
        return t

    def op(self, name, ins, kind, c, emit, fn, q=None, alts=None, **kw):
        if alts is None and name not in RM.FLAG_OF and name in FLAG_OF:
            alts = [(FLAG_OF[name], name)]
        out = super().op(name, ins, kind, c, emit, fn, q, alts, **kw)
        # (on a 1 x 1 image an ADD / MUL of two tensors is also what the "gate" row takes, behind the "elementwise" row)
        if name == "elementwise" and len(ins) == 2 and (out.h, out.w) == (1, 1) and len(out.shape) == 4:
            self.nodes[-1].alts = list(self.nodes[-1].alts) + [(FLAG_OF["gate"], "gate")]
        return out

    def bconv(self, t, dst, cout=None, *a, **kw):
        return super().bconv(t, dst, cout or int(self.g.choice(CHANNELS)), *a, **kw)

    def lceq(self, t):
        zp = t.q[1] if t.kind == "i8" else 0
        return self.op("LceQuantize", [t], "bits", t.c, lambda b, i, o: b.custom_op("LceQuantize", i, [o], b""), lambda v: O.bitpack(v, zp),
                       rank2=t.rank2, keep_dims=t.keep_dims)

    def lcedq(self, t):
        c = t.c
        return self.op("LceDequantize", [t], "f32", c, lambda b, i, o: b.custom_op("LceDequantize", i, [o], b""),
                       lambda v: O.unpack(v, c, np.float32), rank2=t.rank2, keep_dims=t.keep_dims)

    def window(self, t, filters=((2, 2), (3, 3), (2, 3), (3, 1))):
        if self._window is not None:
            forced, self._window = self._window, None
            return forced
        return super().window(t, filters)

    def pool(self, t, same_shape=False, force=None):
        """_Gen.pool, with `force` = (PR.MAX | PR.AVERAGE, filter, stride, padding) for the transition block."""
        g = self.g
        filt, stride, padding = self.window(t)
        if same_shape:
            stride, padding = (1, 1), SAME
        op = int(g.integers(0, 2))
        if force is not None:
            op, filt, stride, padding = force
        code = MAX_POOL_2D if op == PR.MAX else AVERAGE_POOL_2D
        if t.kind == "f32":
            act = NONE if force else self.pick_act(PR.pool2d(t.val, op, filt, stride, padding))
            fn = lambda v: PR.pool2d(v, op, filt, stride, padding, act)
        else:
            s, z = t.q
            real = (PR.pool2d(t.val, op, filt, stride, padding, NONE, s, z).astype(np.float32) - z) * s
            act = NONE if force else self.pick_act(real)
            fn = lambda v: PR.pool2d(v, op, filt, stride, padding, act, s, z)
        return self.op("pool", [t], t.kind, t.c, lambda b, i, o: pool_op(b, code, i, [o], filt, stride, padding, act), fn, t.q)

    def const_i8(self, b, shape, values, q, name="k"):
        k = b.tensor(list(shape) or [1], np.int8, name, np.asarray(values, np.int8).reshape(list(shape) or [1]), scale=q[0], zero_point=q[1])
        if not shape:
            b.tensors[k].fields[0] = _Vector("i", [])                  # (the writer takes no data for a 0-d shape: declared afterwards)
        return k

    # ---- (l) standalone float activations ------------------------------------------------------------------------------------------
    def activation(self, t, kind=None):
        g = self.g
        kind = kind or str(g.choice(ACTIVATION_KINDS))
        c = t.c
        if kind == "prelu":
            form = int(g.integers(0, 5))
            n = c if form < 3 else 1
            alpha = (g.uniform(0.1, 1.5, n) * g.choice([-1, 1, 1, 1], n)).astype(np.float32)
            shape = [[c], [1, 1, c], [1, 1, 1, c], [1], []][form]
            fn = lambda v: AR.prelu(v, alpha if n > 1 else alpha[0])

            def emit(b, i, o):
                k = b.tensor(shape or [1], np.float32, "alpha", alpha.reshape(shape or [1]))
                if not shape:
                    b.tensors[k].fields[0] = _Vector("i", [])
                return b.builtin_op(AM.PRELU, i + [k], [o])
        elif kind == "logistic":
            fn, emit = AR.logistic, (lambda b, i, o: b.builtin_op(AM.LOGISTIC, i, [o]))
        else:
            code, act = dict(relu=(AM.RELU_OP, RELU), relu_n1_to_1=(AM.RELU_N1_TO_1_OP, RELU_N1_TO_1), relu6=(AM.RELU6_OP, RELU6))[kind]
            fn, emit = (lambda v: AR.clamp(v, act)), (lambda b, i, o: b.builtin_op(code, i, [o]))
        return self.op("activation", [t], "f32", c, emit, fn, rank2=t.rank2, keep_dims=t.keep_dims)

    def activation_chain(self, t, long=None):
        """(l) an ADD / MUL chain with activation steps in it: short, or past the cap with activations on both sides of the cut;
        its last step may centre the result so that an LceQuantize behind it stays mixed."""
        g = self.g
        long = (self.left() >= 10 and g.random() < 0.45) if long is None else long
        length = 10 if long else int(min(g.integers(2, 7), self.left()))
        centre = g.random() < 0.7
        v, kinds = t, list(g.permutation(ACTIVATION_KINDS))
        for k in range(length):
            r = g.random()
            if k == length - 1 and centre and length > 1:
                v = self.ew(v, centre=True)
            elif r < 0.45 or (long and k in (0, 4, 8)) or (k == 0 and length == 2):
                v = self.activation(v, str(kinds[k % 5]))
            elif r < 0.55 and k:
                v = self.ew(v, t)
            else:
                v = self.ew(v)
        self.features["l"] += 1
        if v.balanced() and self.left() >= 1 and g.random() < 0.7:
            self.fold_variants(v)
        elif g.random() < 0.3:
            v.output = True
        return v

    # ---- (m) the per-image float gate ------------------------------------------------------------------------------------------------
    def mean(self, t, keep):
        def emit(b, i, o):
            return HM.mean_op(b, i + [b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [o], keep)
        return self.op("mean", [t], "f32", t.c, emit, lambda v: HR.mean_hw(v, keep), rank2=True, keep_dims=keep)

    def dense(self, t, n, w, wb, act=NONE, name="fully_connected", alts=None, fn=None):
        """A float FULLY_CONNECTED on the rank-2 or [b,1,1,K] tensor `t`."""
        k = t.c

        def emit(b, i, o):
            ins = i + [b.tensor([n, k], np.float32, "dense_w", w)] + ([b.tensor([n], np.float32, "dense_b", wb)] if wb is not None else [])
            return HM.fc_op(b, ins, [o], act)
        fn = fn or (lambda v: HR.fully_connected(v.reshape(v.shape[0], -1), w, wb, act))
        return self.op(name, [t], "f32", n, emit, fn, alts=alts, rank2=True)

    def reshape(self, t, rank2_shape=None):
        """RESHAPE that keeps the batch: an image or a [b,1,1,C] tensor to [b, K], or a [b, C] tensor to [b,1,1,C]."""
        k = int(np.prod(t.val.shape[1:])) if t.kind != "bits" else None
        to_gate = t.rank2 and not t.keep_dims
        shape = [1, 1, 1, k] if to_gate else [-1, k]
        fn = (lambda v: v.reshape(v.shape[0], 1, 1, -1)) if to_gate else (lambda v: v.reshape(v.shape[0], -1))
        with_shape = self.g.random() < 0.8

        def emit(b, i, o):
            return b.builtin_op(AM.RESHAPE, i + ([b.tensor([len(shape)], np.int32, "shape", np.array(shape, np.int32))] if with_shape else []), [o])
        return self.op("reshape", [t], t.kind, k, emit, fn, t.q, rank2=True, keep_dims=to_gate)

    def float_gate(self, t):
        g = self.g
        c = t.c
        variant = int(g.integers(0, 4))
        keep = variant != 1
        pooled = self.mean(t, keep)
        h = pooled
        if variant == 1:
            w, wb = (g.standard_normal((c, c)) * 3.0 / np.sqrt(c)).astype(np.float32), g.standard_normal(c).astype(np.float32)
            h = self.dense(pooled, c, w, wb)
        elif variant == 2:
            w, wb = (g.standard_normal((c, 1, 1, c)) * 3.0 / np.sqrt(c)).astype(np.float32), g.standard_normal(c).astype(np.float32)

            def emit(b, i, o):
                return conv2d_op(b, i + [b.tensor(w.shape, np.float32, "w", w), b.tensor([c], np.float32, "wb", wb)], [o], (1, 1), SAME, NONE)
            alts = [(FLAG_OF["conv1x1"], "conv1x1"), (FLAG_OF["conv2d"], "conv2d")]
            h = self.op("conv1x1", [pooled], "f32", c, emit, lambda v: C1.conv1x1(v, w, wb, (1, 1), NONE), alts=alts, rank2=True, keep_dims=True)
        s = self.activation(h, "logistic")
        gate = self.reshape(s) if not s.keep_dims else s
        code = int(g.choice([MUL, MUL, ADD]))
        first = g.random() < 0.6
        self.features["m"] += 1
        if variant == 3:                                               # the 1 x 1 image: the gate is an ordinary tensor operand
            ins = [pooled, gate] if first else [gate, pooled]
            fn = (lambda a, k: float_op(a, code, k, NONE)) if first else (lambda k, a: float_op(a, code, k, NONE))
            return self.op("elementwise", ins, "f32", c, lambda b, i, o: ew_op(b, code, i, [o], NONE), fn, rank2=True, keep_dims=True)
        act = self.pick_act(float_op(t.val, code, gate.val, NONE))
        ins = [t, gate] if first else [gate, t]
        fn = (lambda a, k: float_op(a, code, k, act)) if first else (lambda k, a: float_op(a, code, k, act))
        # (on a map that has shrunk to 1 x 1 the gate is a tensor operand and the "elementwise" row takes the operator first)
        out = self.op("elementwise" if (t.h, t.w) == (1, 1) else "gate", ins, "f32", c, lambda b, i, o: ew_op(b, code, i, [o], act), fn)
        if out.balanced() and self.left() >= 1 and g.random() < 0.6:
            self.fold_variants(out)
        return out

    # ---- (n) RESHAPE into a head, or delivered -------------------------------------------------------------------------------------------
    def flat_head(self, t):
        """RESHAPE [b, H W C] -> FULLY_CONNECTED -> SOFTMAX on a float or an int8 image (int8: -> DEQUANTIZE)."""
        g = self.g
        flat = self.reshape(t)
        k, classes, beta = flat.c, int(g.integers(5, 17)), f32(g.choice([0.5, 1.0]))
        self.features["n"] += 1
        if t.kind == "f32":
            w, wb = (g.standard_normal((classes, k)) * 1.5 / np.sqrt(k)).astype(np.float32), g.standard_normal(classes).astype(np.float32)
            logits = self.dense(flat, classes, w, wb)
            return self.op("softmax", [logits], "f32", classes, lambda b, i, o: HM.softmax_op(b, i, [o], beta), lambda v: HR.softmax(v, beta), rank2=True)
        per_channel = bool(g.integers(0, 2))
        q_logits = (f32(g.uniform(0.03, 0.06)), int(g.integers(-15, 16)))
        logits = self.dense_i8(flat, classes, q_logits, per_channel)
        probs = self.op("softmax_i8", [logits], "i8", classes, lambda b, i, o: HM.softmax_op(b, i, [o], beta),
                        lambda v: HI.softmax_i8(v, logits.q[0], beta), HIM.Q_PROBS, rank2=True)
        return self.dequantize(probs, rank2=True)

    def dense_i8(self, t, n, q_out, per_channel, act=NONE):
        """An int8 FULLY_CONNECTED on the rank-2 or [b,1,1,K] int8 tensor `t`, calibrated like the int8 convolutions."""
        g = self.g
        k, q_in = t.c, t.q
        w4, bias, sw = M.conv_constants(n, (1, 1), k, int(g.integers(0, 9999)), q_in, q_out, per_channel)
        acc = CI.accumulate(t.val.reshape(t.val.shape[0], 1, 1, k), w4, q_in[1], (1, 1), VALID)
        bias, sw, q_out = self.calibrate(acc, bias, sw, q_in[0], q_out, 0)
        w, sw = w4.reshape(n, k), np.atleast_1d(sw)

        def emit(b, i, o):
            return HM.fc_op(b, i + [b.qtensor(w.shape, np.int8, "dense_w", w, sw, [0] * sw.size, 0), b.tensor([n], np.int32, "dense_b", bias)], [o], act)
        fn = lambda v: HI.fully_connected_i8(v.reshape(v.shape[0], k), w, bias, sw, q_in, q_out, act)
        return self.op("fully_connected_i8", [t], "i8", n, emit, fn, q_out, rank2=True)

    # ---- (o) the binary Dense layer --------------------------------------------------------------------------------------------------
    def binary_layer(self, d, n, act=NONE):
        """FULLY_CONNECTED on +-s weights (s a power of two) behind the LceDequantize output `d`."""
        w, s, wb = BM.dense_weights(self.g, d.c, n, "pow2", bias=self.g.random() < 0.8)
        bits_w, scale = BR.prepare(w)
        k = d.c
        fn = lambda v: BR.binary_fully_connected(BR.pack_signs(np.signbit(v.reshape(v.shape[0], k))), bits_w, scale, wb, k, act)[0]
        alts = [(FLAG_OF["binary_dense"], "binary_dense"), (FLAG_OF["fully_connected"], "fully_connected")]
        return self.dense(d, n, w, wb, act, "binary_dense", alts, fn)

    def refused_layer(self, d, n):
        """The same with one weight of another magnitude: BinaryDensePrepare refuses it and the head's row takes it."""
        w, s, wb = BM.dense_weights(self.g, d.c, n, "pow2")
        w[n // 2, d.c // 3] *= np.float32(0.5)
        self.features["o_refused"] += 1
        return self.dense(d, n, w, wb)

    def binary_dense(self, t, variant=None):
        g = self.g
        if not t.balanced():
            t = self.ew(t, centre=True)
        pooled = self.mean(t, bool(g.integers(0, 2)))
        if not 0.25 <= float(np.mean(pooled.val < 0)) <= 0.75:
            return pooled
        d = self.lcedq(self.lceq(pooled))
        n = int(g.choice([10, 33, 40, 64]))
        variant = (self.seed + self.features["o"]) % 4 if variant is None else variant   # (the variants rotate with the seed)
        self.features["o"] += 1
        self.features["o_ragged"] += bool(d.c % 32 or n % 32)
        if variant == 3:
            return self.refused_layer(d, n)
        y = self.binary_layer(d, n)
        if variant == 1 and self.left() >= 1:                          # a second binary Dense layer on the same signs
            self.binary_layer(d, int(g.choice([12, 32])))
        if variant == 2:                                               # a second reader of another kind
            self.features["o_second_reader"] += 1
            if g.random() < 0.5 or self.left() < 1:
                d.output = True
            else:
                self.refused_layer(d, 9)
        if self.left() >= 3 and 0.25 <= float(np.mean(y.val < 0)) <= 0.75 and g.random() < 0.6:   # a hidden layer: only its bits are written
            y = self.binary_layer(self.lcedq(self.lceq(y)), int(g.choice([7, 16])))
        if self.left() >= 1 and g.random() < 0.5:
            y = self.op("softmax", [y], "f32", y.c, lambda b, i, o: HM.softmax_op(b, i, [o], 1.0), lambda v: HR.softmax(v, 1.0), rank2=True)
        return y

    # ---- (p) MeliusNet's improvement block ---------------------------------------------------------------------------------------------
    def slice(self, t, begin, count, form=None):
        g = self.g
        c, H, W = t.c, t.h, t.w
        forms = ["masked", "plain", "slice"] + (["negative"] if begin + count == c else [])
        form = form or forms[int(g.integers(0, len(forms)))]

        def emit(b, i, o):
            i32 = lambda name, v: b.tensor([4], np.int32, name, np.array(v, np.int32))
            if form == "slice":
                return b.builtin_op(SM.SLICE, i + [i32("begin", [0, 0, 0, begin]), i32("size", [-1, H, -1, count])], [o])
            if form == "masked":
                v, masks = ([5, 7, -2, begin], [1, 2, 3, begin + count]), (7, 7)
            elif form == "negative":
                v, masks = ([0, 0, 0, begin - c], [1, H, W, 0]), (0, 8)
            else:
                v, masks = ([0, 0, 0, begin], [1, H, W, begin + count]), (0, 0)
            return SM.strided_slice_op(b, i + [i32("begin", v[0]), i32("end", v[1]), i32("strides", [1, 1, 1, 1])], [o], masks[0], masks[1])
        assert SM.resolve(c, begin, begin + count) == (begin, count)
        return self.op("slice", [t], t.kind, count, emit, lambda x: np.ascontiguousarray(x[..., begin:begin + count]), t.q)

    def int8_add_at(self, a, c, q):
        """The int8 ADD of two tensors written at the quantization `q` (a join needs ONE quantization)."""
        q6 = (a.q[0], a.q[1], c.q[0], c.q[1], q[0], q[1])
        return self.op("int8_add", [a, c], "i8", a.c, lambda b, i, o: ew_op(b, ADD, i, [o], NONE), lambda u, v: A.add_q(u, v, q6, NONE), q)

    def improvement(self, t, full=False):
        g = self.g
        c = t.c
        counts = [n for n in (16, 32, 20, 12) if n < c]
        count = counts[int(g.integers(0, len(counts)))]
        begin = c - count
        self.features["p"] += 1
        if self.left() < 6 or not t.balanced() or (g.random() < 0.3 and not full):   # a lone window: delivered, folded, or read twice
            begin = int(g.choice([0, begin, (c - count) // 2]))
            s = self.slice(t, begin, count)
            r = g.random()
            if r < 0.35 or self.left() < 1:
                s.output = True
            elif s.balanced():
                self.lceq(s)
                if r > 0.7 and self.left() >= 1:
                    self.pool(s, same_shape=True)
            return s
        dst = O.DST_F32 if t.kind == "f32" else O.DST_I8
        y = self.bconv(self.lceq(t), dst, count, 3, 1, pad=(O.PADDING_SAME, 1), q=t.q)
        s = self.slice(t, begin, count)
        if g.random() < 0.2:
            s.output = True                                            # a second reader: the window is written after all
        a = (self.ew(s, y, ADD, NONE) if g.random() < 0.8 else self.ew(y, s, ADD)) if t.kind == "f32" else self.int8_add_at(s, y, t.q)
        rest = self.slice(t, 0, begin)
        out = self.concat([rest, a])
        if out.balanced() and self.left() >= 1 and g.random() < 0.6:
            self.fold_variants(out)
        return out

    # ---- (q) the int8 elementwise chain ---------------------------------------------------------------------------------------------------
    def i8_step(self, t, kind, up=None, act=None):
        g = self.g
        (si, zi), c = t.q, t.c
        real = (t.val.astype(np.float64) - zi) * si
        low, high = float(np.mean(t.val < zi)), 0.0
        near = lambda: int(np.clip(zi + g.integers(-8, 9), -120, 120))
        if kind == "clamp":
            acts = [a for a, ok in ((RELU, low < 0.3), (RELU_N1_TO_1, np.mean(np.abs(real) > 1) < 0.3), (RELU6, low < 0.3 and np.mean(real > 6) < 0.3)) if ok]
            acts = [act] if act in acts else acts
            if not acts:
                kind = "requantize"
        per = bool(g.integers(0, 2))
        n = c if per else 1
        shape = ([[c], [1, 1, 1, c]] if per else [[1], []])[int(g.integers(0, 2))]
        if kind == "add":
            up = g.random() < 0.4 if up is None else up                # a shift that leaves few values below the zero point: a RELU may follow
            while True:
                sk, zk = f32(si * (g.uniform(1.2, 1.6) if up else g.uniform(0.5, 1.5))), int(g.integers(-10, 11))
                # (up: the shift that leaves about an eighth of the values below the zero point, and a little per channel)
                need = max(-float(np.quantile(t.val.astype(np.float64) - zi, 0.12)), 0.0) * si / sk
                k = np.clip(zk + np.rint(need) + g.integers(0, 7, n), -128, 127).astype(np.int8) if up else g.integers(-25, 26, n).astype(np.int8)
                so, zo = f32(si * g.uniform(1.0, 1.25)), (int(np.clip(zi - g.integers(30, 60), -128, 127)) if up else near())
                try:
                    A.prepare(si, zi, sk, zk, so, zo, NONE)
                    break
                except ValueError:
                    continue
            st = ("add", k if per else np.int8(k[0]), (sk, zk), (so, zo), NONE)
            emit = lambda b, i, o: ew_op(b, ADD, (i + [self.const_i8(b, shape, k, (sk, zk))])[::int(g_first)], [o], NONE)
            g_first = 1 if g.random() < 0.7 else -1
        elif kind == "prelu":
            sa, za = f32(0.01), int(g.integers(-5, 6))
            alpha = (za + g.integers(30, 121, n)).astype(np.int8)
            so, zo = f32(si * g.uniform(0.8, 1.2)), near()
            st = ("prelu", alpha if per else np.int8(alpha[0]), (sa, za), (so, zo))
            shape = [1, 1, c] if (per and g.random() < 0.4) else shape
            emit = lambda b, i, o: b.builtin_op(AM.PRELU, i + [self.const_i8(b, shape, alpha, (sa, za), "alpha")], [o])
        elif kind == "clamp":
            act = int(acts[int(g.integers(0, len(acts)))])
            so, zo = f32(si * g.uniform(0.9, 1.1)), near()
            st = ("clamp", (so, zo), act)
            code = {RELU: AM.RELU_OP, RELU_N1_TO_1: AM.RELU_N1_TO_1_OP, RELU6: AM.RELU6_OP}[act]
            emit = lambda b, i, o: b.builtin_op(code, i, [o])
        else:
            so, zo = f32(si * g.uniform(0.7, 1.5)), int(g.integers(-20, 21))
            st = ("requantize", (so, zo))
            emit = lambda b, i, o: b.builtin_op(QUANTIZE_OP, i, [o])
        q_in = t.q
        fn = lambda x: E.apply_step(np.asarray(x).astype(np.int64), st, q_in)[0].astype(np.int8)
        return self.op("elementwise_i8", [t], "i8", c, emit, fn, (so, zo))

    def int8_chain(self, t, mode=None):
        g = self.g
        self.features["q"] += 1
        mode = (self.seed + self.features["q"]) % 3 if mode is None else mode          # 0: a head ADD read twice, 1: RELU_N1_TO_1, 2: a head
        n1 = mode == 1 and self.left() >= 3 and t.balanced()
        if not n1 and self.left() >= 5 and t.balanced() and g.random() < 0.9:   # behind a residual ADD: the chain's head, unless it is read twice
            y = self.bconv(self.lceq(t), O.DST_I8, t.c, 3, 1, pad=(O.PADDING_SAME, 1))
            t = self.int8_add(y, t) if g.random() < 0.5 else self.int8_add(t, y)
            if mode == 0:
                if g.random() < 0.5 or self.left() < 2:
                    t.output = True
                else:
                    side = self.pool(t, same_shape=True)
                    if side.balanced() and self.left() >= 3:
                        self.lceq(side)
        v = t
        if n1:
            # (RELU_N1_TO_1 clamps real values at +-1: it is drawn where the tensor's scale keeps most of them inside)
            q = (f32(g.uniform(0.012, 0.018)), int(g.integers(-10, 11)))
            v = self.i8_step(self.bconv(self.lceq(t), O.DST_I8, t.c, 3, 1, pad=(O.PADDING_SAME, 1), q=q), "clamp", act=RELU_N1_TO_1)
        for _ in range(int(min(g.integers(1, 5), max(self.left(), 1)))):
            kind = str(g.choice(["add", "prelu", "clamp", "requantize"]))
            if kind == "clamp" and float(np.mean(v.val < v.q[1])) >= 0.3 and self.left() >= 2:
                v = self.i8_step(v, "add", up=True)                    # (a RELU of a centred tensor would put half of it on one value)
            v = self.i8_step(v, kind)
        if v.balanced() and self.left() >= 1 and g.random() < 0.6:
            self.lceq(v)
        return v

    # ---- (r) the int8 gate ------------------------------------------------------------------------------------------------------------------
    def mul_i8(self, x, operand, per_image):
        g = self.g
        q1, q2 = x.q, operand.q
        if per_image:
            qo = (f32(q1[0] * g.uniform(0.55, 0.8)), int(np.clip(q1[1] + g.integers(-6, 7), -128, 127)))
        else:
            p = (x.val.astype(np.float64) - q1[1]) * (operand.val.astype(np.float64) - q2[1])
            qo = (f32(q1[0] * q2[0] * max(p.std(), 1.0) / 40.0), int(g.integers(-10, 11)))
        c, rows = x.c, x.h * x.w
        first = g.random() < 0.5 or not per_image                      # (a TENSOR operand is input 1)

        def ref(a, k):
            return G.mul_q(a.reshape(-1, c), k.reshape(-1, c), q1, q2, qo, NONE, rows if per_image else 0).reshape(a.shape)
        ins = [x, operand] if first else [operand, x]
        fn = ref if first else (lambda k, a: ref(a, k))
        return self.op("mul_i8", ins, "i8", c, lambda b, i, o: ew_op(b, MUL, i, [o], NONE), fn, qo)

    def int8_gate(self, t):
        g = self.g
        c, q_src = t.c, t.q
        self.features["r"] += 1
        if (self.seed + self.features["r"]) % 5 < 3 and self.left() >= 5 and t.balanced():
            self.features["r_gate"] += 1
            keep = bool(g.integers(0, 2))
            real = (t.val.astype(np.float64) - q_src[1]).mean((1, 2)) * q_src[0]
            s = f32(max(real.max() - real.min(), 1e-3) / 200.0)
            q_pool = (s, int(np.clip(np.rint(-100 - real.min() / s), -128, 127)))

            def emit_mean(b, i, o):
                return HM.mean_op(b, i + [b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))], [o], keep)
            shape = (lambda v: (v.shape[0], 1, 1, c)) if keep else (lambda v: (v.shape[0], c))
            pooled = self.op("mean_i8", [t], "i8", c, emit_mean, lambda v: HI.mean_i8(v, q_src, q_pool).reshape(shape(v)), q_pool, rank2=True, keep_dims=keep)
            q_h = (f32(g.uniform(0.04, 0.07)), int(g.integers(-10, 11)))
            if keep and g.random() < 0.6:                              # a 1 x 1 CONV_2D on the [b,1,1,C] tensor
                per_channel = bool(g.integers(0, 2))
                w, bias, sw = M.conv_constants(c, (1, 1), c, int(g.integers(0, 9999)), q_pool, q_h, per_channel)
                bias, sw, q_h = self.calibrate(CI.accumulate(pooled.val, w, q_pool[1], (1, 1), SAME), bias, sw, q_pool[0], q_h, 0)

                def emit(b, i, o):
                    return conv2d_op(b, i + [M.filter_tensor(b, w, sw), b.tensor([c], np.int32, "wb", bias)], [o], (1, 1), SAME, NONE)
                h = self.op("conv_i8", [pooled], "i8", c, emit, lambda v: CI.conv2d_i8(v, w, bias, sw, q_pool, q_h, (1, 1), SAME, NONE), q_h,
                            rank2=True, keep_dims=True)
            else:
                h = self.dense_i8(pooled, c, q_h, bool(g.integers(0, 2)))
            q_hh = h.q
            sig = self.op("logistic_i8", [h], "i8", c, lambda b, i, o: b.builtin_op(AM.LOGISTIC, i, [o]), lambda v: G.logistic_q(v, q_hh), G.LOGISTIC_OUT,
                          rank2=True, keep_dims=h.keep_dims)
            gate = sig if sig.keep_dims else self.reshape(sig)
            m = self.mul_i8(t, gate, True)
        else:
            self.features["r_tensor"] += 1
            peers = [u for u in self.tensors if u.kind == "i8" and not u.rank2 and u is not t and (u.h, u.w, u.c) == (t.h, t.w, t.c)]
            other = peers[int(g.integers(0, len(peers)))] if peers and g.random() < 0.6 else self.pool(t, same_shape=True)
            m = self.mul_i8(t, other, False)
        if self.left() < 1:
            return m
        if (self.seed + self.features["r"]) % 3 == 0:                  # the product has another reader: no rider
            self.features["r_no_rider"] += 1
            if g.random() < 0.5 or self.left() < 2:
                m.output = True
            else:
                self.pool(m, same_shape=True)
        out = self.int8_add(m, t) if g.random() < 0.5 else self.int8_add(t, m)
        if out.balanced() and self.left() >= 1 and g.random() < 0.5:
            self.lceq(out)
        return out

    # ---- (s) the transition --------------------------------------------------------------------------------------------------------------------
    def transition(self, t, variant=None):
        g = self.g
        self.features["s"] += 1
        variant = ((0, 1, 5, 3, 2)[(self.seed + self.features["s"]) % 5] if variant is None else variant) if t.kind == "f32" else 4
        row = variant == 5 and min(t.h, t.w) >= 4
        op = PR.AVERAGE if variant == 1 else PR.MAX
        p = self.pool(t, force=(op, (3, 3), (2, 2), SAME) if row else (op, (2, 2), (1, 1), SAME))
        if variant == 1 and p.balanced() and self.left() >= 3 and g.random() < 0.6:
            self.lceq(p)                                               # (an AVERAGE pool never fuses: this LceQuantize folds into its launch)
        if variant == 2 and self.left() >= 2:
            if p.balanced():
                self.lceq(p)                                           # (the second reader folds into the pool's own launch)
            else:
                self.ew(p).output = True
        if variant == 3:
            p.output = True
        self._window = ((5, 5), (1, 1), SAME) if row else ((3, 3), (2, 2), SAME)
        d = self.depthwise(p) if t.kind == "f32" else self.depthwise_i8(p)
        self._window = None
        if d.balanced() and self.left() >= 1 and g.random() < 0.6:
            self.fold_variants(d)
        return d

    # ---- growth ---------------------------------------------------------------------------------------------------------------------------------
    def new_step(self):
        """One of the blocks l to s on a tensor that suits it; False when none was grown."""
        g = self.g
        if not (self.want2 or g.random() < 0.2):
            return False
        k = self.want2.pop(0) if self.want2 else str(g.choice(list("lmmoopqrs")))
        images = [t for t in self.tensors if not t.rank2 and t.c != 3 and t.kind != "bits"]
        fresh = [t for t in images if not t.readers and not t.output]
        pick = lambda ts: ts[int(g.integers(0, len(ts)))] if ts else None
        # (a tensor that one of the newer passes made is taken first, half of the time: the blocks then read each other)
        newer = [t for t in fresh if t.producer is not None and self.nodes[t.producer].name in P2.NEW] if g.random() < 0.35 else []
        of = lambda kind, ok=lambda t: True: pick([t for t in newer if t.kind == kind and ok(t)]) or pick([t for t in fresh if t.kind == kind and ok(t)]) or \
            pick([t for t in images if t.kind == kind and ok(t)])
        ft, it = of("f32"), of("i8")
        if k in "qr" and it is None and ft is not None and self.left() >= 4:
            it = self.quantize(of("f32", lambda t: t.balanced()) or ft)
        n = len(self.nodes)
        if k == "l" and ft is not None and self.left() >= 2:
            self.activation_chain(ft)
        elif k == "m" and ft is not None and self.left() >= 5:
            self.float_gate(ft)
        elif k == "n" and self.left() >= 1:
            t = pick([t for t in images if t.h * t.w * t.c <= 4096])
            if t is not None:
                self.reshape(t).output = True
                self.features["n"] += 1
        elif k == "o" and ft is not None and self.left() >= 5:
            self.binary_dense(ft)
        elif k == "p" and self.left() >= 1:
            wide = lambda t: 33 <= t.c <= 96
            kind = "f32" if (g.random() < 0.5 or it is None) else "i8"
            t = of(kind, lambda t: wide(t) and t.balanced()) or of(kind, wide)
            if t is not None:
                self.improvement(t)
        elif k == "q" and it is not None and self.left() >= 1:
            self.int8_chain(it)
        elif k == "r" and it is not None and self.left() >= 3:
            self.int8_gate(of("i8", lambda t: t.balanced()) or it)
        elif k == "s" and self.left() >= 2:
            t = of("f32", lambda t: min(t.h, t.w) >= 3) if (g.random() < 0.93 or it is None) else of("i8", lambda t: min(t.h, t.w) >= 3)
            if t is not None:
                self.transition(t)
        return len(self.nodes) > n

    def grow_must(self):
        """The seed's own block (MUST) on a fresh tensor that suits it; False while there is none."""
        fresh = [t for t in self.tensors if not t.rank2 and t.c != 3 and t.kind != "bits" and not t.readers and not t.output]
        first = lambda kind, ok=lambda t: True: next((t for t in fresh if t.kind == kind and ok(t)), None)
        k = self.must
        wide = lambda t: 33 <= t.c <= 96 and t.balanced()
        t = first("f32", lambda t: min(t.h, t.w) >= 4) if k[0] == "s" else first("f32" if k == "p_f32" else "i8", wide) if k[0] == "p" else \
            first("f32") if k[0] == "o" else first("i8", lambda t: t.balanced())
        if t is None:
            return False
        if k[0] == "s":
            self.transition(t, int(k[1]))
        elif k[0] == "p":
            self.improvement(t, full=True)
        elif k[0] == "o":
            self.binary_dense(t, int(k[1]))
        else:
            self.int8_chain(t, 2 if k == "q_head" else 0)
        return True

    def grow(self):
        g = self.g
        while self.left() >= 1:
            # (the chain past the cap needs nine operators: it is grown before the newer blocks use the room up)
            floats = [t for t in self.tensors if t.kind == "f32" and t.c != 3 and not t.rank2 and not t.readers and not t.output]
            early = "e" in self.want and self.left() >= 9 and floats
            if self.must and self.left() >= 7 and self.grow_must():
                self.must = None
            elif self.long_l and self.left() >= 11 and floats:           # (and so is the one with activations on both sides of the cut)
                self.long_l = False
                self.activation_chain(floats[0], long=True)
            elif early or not self.new_step():
                self.step()                                            # (generation 1's transitions)
        if self.head:
            ends = [t for t in self.tensors if t.kind != "bits" and not t.rank2 and t.c != 3 and not t.readers] or \
                   [t for t in self.tensors if t.kind != "bits" and not t.rank2 and t.c != 3]
            if ends:
                kind = "i8" if (g.random() < 0.5 and any(t.kind == "i8" for t in ends)) else ends[int(g.integers(0, len(ends)))].kind
                ends = [t for t in ends if t.kind == kind]
                ends = [t for t in ends if t.balanced()] or ends       # (a map far off its zero point saturates the pooled tensor)
                t = ends[int(g.integers(0, len(ends)))]
                if t.h * t.w * t.c <= 4096 and g.random() < 0.5:
                    self.flat_head(t)                                  # (n) the head that flattens instead of pooling
                else:
                    (self.float_head if t.kind == "f32" else self.int8_head)(t)
        for t in self.tensors:
            if not t.readers and t is not self.x:
                t.output = True


def _attrs(b):
    """Per operator of the builder: dict(code=its builtin code, None for a custom operator; act=the fused activation its options
    table holds, None without one), read from what the writer recorded."""
    out = []
    for op in b.ops:
        custom, code = b.codes[op.fields[0].value]
        table = op.fields.get(4)
        act = None
        if custom is None and isinstance(table, _Table):
            slot = {ADD: 0, MUL: 0, MAX_POOL_2D: 5, AVERAGE_POOL_2D: 5}.get(code)
            act = table.fields[slot].value if slot is not None and isinstance(table.fields.get(slot), _Scalar) else None
        out.append(dict(code=None if custom is not None else code, act=act))
    return out


def walk(info, flags=None, section=0):
    """partition_ref2's counters of `section` of the seed's file under `flags` (default: everything)."""
    flags = EVERY_FLAG if flags is None else flags
    kinds = info["kinds"](flags)
    sections = reference_partition(info, flags)
    return P2.expected_counters(sections[section], info["ops"], kinds, info["constants"], info["attrs"], info["types"], info["dims"],
                                bool(flags.get("transition")))


@functools.lru_cache(maxsize=None)
def build(seed):
    """random_models.build for generation 2: the same dict, with attrs and dims (what partition_ref2 reads besides the wiring),
    walk (the restated counters of the one section), pairs (the ordered pairs of different newer passes in a producer-to-reader
    relation) and the features a-k, h_*, l-s and VARIANTS."""
    gen = _Gen2(seed)
    gen.grow()
    b, F, order = gen.write()
    nodes = [gen.nodes[k] for k in order]
    ops = RM._tensor_lists(b)
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
    types = {F[t.n]: t.kind for t in gen.tensors}
    channels = {F[t.n]: t.c for t in gen.tensors}
    dims = {F[t.n]: list(t.shape) for t in gen.tensors}
    outputs = set(b.outputs)
    info = dict(seed=seed, data=b.finish(), x=gen.x.val, batch=gen.batch, input=x_t, outputs=list(b.outputs), ops=ops, constants=constants,
                names=kinds(EVERY_FLAG), alts=[n.alts for n in nodes], forward=forward, host={k: fn for k, (_, _, fn) in enumerate(wiring)},
                kinds=kinds, types=types, channels=channels, dims=dims, attrs=_attrs(b), bit_tensors={t for t, k in types.items() if k == "bits"})
    names = info["names"]
    readers = P.readers_of(ops)
    features = dict(gen.features)
    one = walk(info)
    info["walk"] = one
    chains = one["chains"]
    info["chains"] = chains
    # (e), (f) and what the walk decided are read off the restated walk of the one section
    features["e"] = sum(1 for _, why in chains if why == "cap")
    features["f"] = sum(1 for _, why in chains if why == "operand")
    features["l"] = sum(1 for ks, _ in chains if "activation" in ks and ("elementwise" in ks or "gate" in ks))
    features.update(o_skipped=one["dequantize_skipped"], q_head=one["heads"], r_rider=one["riders"], s_fused=one["transition"][0], p_join=one["joins"])
    # a chain that ran into the cap and holds an activation, continued by a chain that holds one too
    for ks, why, members in zip([c[0] for c in chains], [c[1] for c in chains], one["chain_ops"]):
        behind = [m for m in one["chain_ops"] if ops[members[-1]][1][0] in ops[m[0]][0]]
        features["l_cap"] += why == "cap" and "activation" in ks and any("activation" in [names[j] for j in m] for m in behind)
    # the variants of o, q and r are read off the graph: who reads what
    made_by = {ops[k][1][0]: k for k in range(len(ops))}
    features.update({k: 0 for k in ("o_second_reader", "o_refused", "o_ragged", "q_no_head", "r_gate", "r_tensor", "r_no_rider") + CLAMPS})
    features["q_fold"] = one["folded"]["elementwise_i8"]
    for k, name in enumerate(names):
        t = ops[k][1][0]
        rd = readers.get(t, [])
        shared = len(rd) > 1 or t in outputs
        var = [u for u in ops[k][0] if u >= 0 and u not in constants]
        if nodes[k].name == "LceDequantize" and any(names[r] == "binary_dense" for r in rd):
            features["o_second_reader"] += t in outputs or any(names[r] != "binary_dense" for r in rd)
        if name == "fully_connected" and var[0] in made_by and nodes[made_by[var[0]]].name == "LceDequantize":
            features["o_refused"] += 1
        if name == "binary_dense":
            features["o_ragged"] += bool(channels[var[0]] % 32 or channels[t] % 32)
        if name == "int8_add" and any(names[r] == "elementwise_i8" for r in rd):
            features["q_no_head"] += shared
        if name == "mul_i8":
            features["r_gate" if P2.gate_slot(ops[k][0], t, dims) is not None and dims[t][1] * dims[t][2] > 1 else "r_tensor"] += 1
            features["r_no_rider"] += shared and any(names[r] == "int8_add" for r in rd)
        if name == "elementwise_i8":
            clamp = {AM.RELU_OP: "q_relu", AM.RELU_N1_TO_1_OP: "q_relu_n1_to_1", AM.RELU6_OP: "q_relu6"}.get(info["attrs"][k]["code"])
            if clamp:
                features[clamp] += 1
    bit_tensors = info["bit_tensors"]
    for k, n in enumerate(nodes):
        t = ops[k][1][0]
        rd = readers.get(t, [])
        quants = [r for r in rd if nodes[r].name == "LceQuantize"]
        is_pass = names[k] in P2.FOLDING and t not in bit_tensors
        features["a"] += is_pass and len(rd) == 1 and len(quants) == 1 and t not in outputs
        features["b"] += is_pass and len(rd) == 1 and len(quants) == 1 and t in outputs
        features["c"] += (is_pass or (n.name == "LceBconv2d" and t not in bit_tensors)) and len(quants) >= 2
        features["d"] += is_pass and len(quants) >= 1 and any(names[r] in P2.PASSES for r in rd)
        if n.name == "pool" and types[t] != "bits" and info["attrs"][k]["code"] is not None:
            dw = [r for r in rd if names[r] in ("depthwise", "depthwise_i8")]
            fused = t in one["elided"]
            features["s_average"] += bool(dw) and info["attrs"][k]["code"] == AVERAGE_POOL_2D and types[t] == "f32"
            features["s_int8"] += bool(dw) and types[t] == "i8" and info["attrs"][k]["code"] == MAX_POOL_2D and len(rd) == 1
            blur = bool(dw) and info["attrs"][k]["code"] == MAX_POOL_2D and types[t] == "f32"
            features["s_second_reader"] += blur and len(rd) > 1
            features["s_delivered"] += blur and t in outputs
            features["s_row"] += fused and tuple(dims[ops[k][0][0]][1:3]) != tuple(dims[t][1:3])
    source = {ops[k][1][0]: ops[k][0][0] for k, n in enumerate(nodes) if n.name == "LceBconv2d"}
    features.update(g=0, h=0, k=int(len({types[t] for t in outputs}) > 1), **{name: 0 for name in JOIN_FEATURES})
    for k, n in enumerate(nodes):
        if names[k] not in ("elementwise", "int8_add", "concat"):
            continue
        ins = [t for t in ops[k][0] if t >= 0 and t not in constants]
        branches = sorted({t for t in ins if t in source})
        features["g"] += any(source[a] == source[c] for a in branches for c in branches if a < c)
        if names[k] == "concat":
            ragged = any(channels[t] % 32 for t in ins)
            features["h"] += 1
            features["h_wide"] += len(ins) >= 4
            features["h_max"] += len(ins) == RM.CONCAT_MAX
            features["h_dup"] += len(set(ins)) < len(ins)
            features["h_ragged_f32"] += ragged and types[ins[0]] == "f32"
            features["h_ragged_i8"] += ragged and types[ins[0]] == "i8"
    features["j"] = int(any(nodes[r].name != "LceQuantize" for r in readers.get(x_t, [])))
    info["features"] = {k: int(v) for k, v in features.items()}
    # producer -> reader pairs of two different newer passes (the name "transition" stands for a pool or depthwise it fused)
    newer = lambda k: "transition" if (names[k] in ("pool", "depthwise") and (ops[k][1][0] in one["elided"] or ops[k][0][0] in one["elided"])) \
        else (names[k] if names[k] in P2.NEW else None)
    info["pairs"] = sorted({(newer(k), newer(r)) for k in range(len(ops)) for r in readers.get(ops[k][1][0], [])
                            if newer(k) and newer(r) and newer(k) != newer(r)})
    x = gen.x.val
    only_quantize = all(nodes[r].name == "LceQuantize" for r in readers.get(x_t, [])) and gen.x.kind == "f32"
    if only_quantize:
        x = x.copy()
        x[0, 0, 0, :3] = (np.nan, np.inf, -np.inf)
    info.update(x=x, nan_ok=only_quantize)
    return info


def violations(info):
    """random_models.violations, unchanged but for the bound on the operators: 6 to MAX_OPS = 24 (generation 1: 20; a gate block
    alone is six operators)."""
    bad = [b for b in RM.violations(info) if not b.endswith(" operators")]
    if not 6 <= len(info["ops"]) <= MAX_OPS:
        bad.append("%d operators" % len(info["ops"]))
    return bad


# The suite's cases: the seeds of range(CANDIDATES) that meet the conditions (tests/test_v2_random_models_host.py checks that this is
# the list, so a dropped seed is dropped by the conditions and by nothing else).
CANDIDATES = 72
SEEDS = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 33, 34, 35, 36, 38, 39, 40, 41, 42, 43, 44, 45, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 62, 63, 65, 66, 67, 69, 70, 71)


def fuzz_seeds():
    return _fuzz()[0]


def fuzz_dropped():
    return _fuzz()[1:]


@functools.lru_cache(maxsize=None)
def _fuzz():
    """As random_models._fuzz: LCE_FUZZ_SEED / LCE_FUZZ_EXAMPLES start a hunt over freshly drawn generation-2 seeds."""
    if "LCE_FUZZ_SEED" not in os.environ and "LCE_FUZZ_EXAMPLES" not in os.environ:
        return [], 0, 0
    base, count = int(os.environ.get("LCE_FUZZ_SEED", "0")), int(os.environ.get("LCE_FUZZ_EXAMPLES", "80"))
    start = 2000003 * (base + 1)
    kept = [s for s in range(start, start + max(count, 0)) if not violations(build(s))]
    print("random_models2: %d fuzz seeds drawn from %d, %d dropped by the conditions" % (count, start, count - len(kept)))
    return kept, max(count, 0) - len(kept), max(count, 0)


def cut_flags(seed):
    """The seed's own subset of the keywords AND the three passes= names: all but a random third (at least one is dropped)."""
    g = np.random.default_rng(seed + 200003)
    names = sorted(EVERY_FLAG)
    dropped = [n for n in names if g.random() < 0.35] or [names[int(g.integers(0, len(names)))]]
    return {n: True for n in names if n not in dropped}


def reference_partition(info, flags):
    return P2.partition(info["ops"], info["kinds"](flags), info["constants"], info["outputs"], bool(flags.get("stem_sections")))


def expected_stats(info, flags=None, section=0):
    """random_models.expected_stats plus the eight newer tuples, as model_runner.LceModel documents them."""
    c = walk(info, flags, section)
    n, f = c["passes"], c["folded"]
    pair = lambda k: (n[k], f[k])
    return dict(elementwise=(n["elementwise"], c["ew_ops"], f["elementwise"]), int8_add=pair("int8_add"), concat=pair("concat"), pool=pair("pool"),
                conv1x1=pair("conv1x1"), depthwise=pair("depthwise"), conv2d=pair("conv2d"), conv_i8=pair("conv_i8"),
                depthwise_i8=pair("depthwise_i8"), head=(n["mean"], n["fully_connected"], n["softmax"]),
                head_i8=(n["mean_i8"], n["fully_connected_i8"], n["softmax_i8"]), quantize=(n["quantize"], n["dequantize"]),
                fused_quantize=c["conv_quantize"],
                activation=(n["activation"], c["ex_ops"], f["activation"]), gate=pair("gate"), reshape=(c["views"], c["copies"]),
                binary_dense=(n["binary_dense"], c["dequantize_skipped"], f["binary_dense"]), slice=(n["slice"], f["slice"], c["joins"]),
                elementwise_i8=(n["elementwise_i8"], c["ew_i8_ops"], f["elementwise_i8"]), gate_i8=(n["mul_i8"], c["gate_i8_ops"], f["mul_i8"]),
                transition=c["transition"])


def model_stats(model):
    """The same dict read from a model_runner.LceModel after a run."""
    return dict(RM.model_stats(model), activation=model.activation_stats(), gate=model.gate_stats(), reshape=model.reshape_stats(),
                binary_dense=model.binary_dense_stats(), slice=model.slice_stats(), elementwise_i8=model.elementwise_i8_stats(),
                gate_i8=model.gate_i8_stats(), transition=model.transition_stats())


run_cut = RM.run_cut
