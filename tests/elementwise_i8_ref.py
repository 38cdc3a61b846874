"""The int8 elementwise chain of include/lce_hip.h (lce_hip_elementwise_i8) restated in NumPy int64 from the header's statement:
the head ADD and the constant ADD are tests/int8_add_ref.py's, PRELU, CLAMP and REQUANTIZE are MBQM(x, m, e) + zo with their own
real multipliers.  ``chain`` applies the steps to a tensor element by element -- it never builds a table -- so the library's table,
its kernels and the model reader are all compared against arithmetic that shares no code with them.  ``real_step`` is one step in
float64, for the deviation the header quotes.  No tests here."""
import numpy as np

import int8_add_ref as ar

ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6 = 0, 1, 2, 3


def mbqm(x, m: int, e: int):
    """MultiplyByQuantizedMultiplier: RDivPOT(SRDHM(x * 2^max(e,0), m), max(-e,0)) on int64 arrays holding int32 values."""
    x = np.asarray(x, np.int64) * np.int64(1 << max(e, 0))
    assert np.all(np.abs(x) <= (1 << 31) - 1), "an intermediate left int32"
    return ar.rdivpot(ar.srdhm(x, m), max(-e, 0))


def f32(v):
    return np.float32(v)


def step_multipliers(kind, si, so, sa=None):
    """The (m, e) pairs of a PRELU (two), CLAMP or REQUANTIZE (one) step."""
    if kind == "prelu":
        r1 = f32(si) / f32(so)
        r2 = f32(f32(si) * f32(sa)) / f32(so)
        return ar.quantize_multiplier(float(r1)), ar.quantize_multiplier(float(r2))
    if kind == "clamp":
        return (ar.quantize_multiplier(float(f32(si) / f32(so))),)
    return (ar.quantize_multiplier(float(f32(si)) / float(f32(so))),)


def apply_step(v, st, q_in):
    """One step on an int64 array v [..., C] of int8 values; returns (int64 values, (scale, zero point) of the result)."""
    si, zi = q_in
    kind = st[0]
    if kind == "add":
        _, k, (sk, zk), (so, zo), act = st
        k = np.asarray(k, np.int64)
        p = ar.prepare(si, zi, sk, zk, so, zo, act)
        return ar.add(v, np.broadcast_to(k, v.shape), zi, zk, zo, p).astype(np.int64), (so, zo)
    if kind == "prelu":
        _, alpha, (sa, za), (so, zo) = st
        (m1, e1), (m2, e2) = step_multipliers("prelu", si, so, sa)
        d = v - zi
        alpha = np.broadcast_to(np.asarray(alpha, np.int64), v.shape)
        pos = mbqm(np.where(d >= 0, d, 0), m1, e1)
        neg = mbqm(np.where(d < 0, d * (alpha - za), 0), m2, e2)
        return np.clip(np.where(d >= 0, pos, neg) + zo, -128, 127), (so, zo)
    if kind == "clamp":
        _, (so, zo), act = st
        ((m, e),) = step_multipliers("clamp", si, so)
        lo, hi = ar.activation_range(act, so, zo)
        return np.minimum(hi, np.maximum(lo, mbqm(v - zi, m, e) + zo)), (so, zo)
    if kind == "requantize":
        _, (so, zo) = st
        ((m, e),) = step_multipliers("requantize", si, so)
        return np.clip(mbqm(v - zi, m, e) + zo, -128, 127), (so, zo)
    raise ValueError("unknown step %r" % (kind,))


def chain(x, q_in, steps, addend=None, head=None):
    """The chain on int8 x [..., C]: returns (int8 out, int32 bits at the last step's zero point)."""
    v = np.asarray(x).astype(np.int64)
    q = q_in
    if head is not None:
        q_add, q_out = head[0], head[1]
        act = head[2] if len(head) == 3 else ACT_NONE
        p = ar.prepare(q[0], q[1], q_add[0], q_add[1], q_out[0], q_out[1], act)
        v = ar.add(v, np.asarray(addend), q[1], q_add[1], q_out[1], p).astype(np.int64)
        q = q_out
    for st in steps:
        v, q = apply_step(v, st, q)
    out = v.astype(np.int8)
    return out, ar.bitpack(out, q[1])


def table(channels, q_in, steps):
    """What lce_hip_elementwise_i8_prepare must write, from ``chain`` on all 256 values of every channel: uint8 [R, 256]."""
    per_channel = any(st[0] in ("add", "prelu") and np.ndim(st[1]) > 0 for st in steps)
    rows = channels if per_channel else 1
    x = np.broadcast_to(np.arange(-128, 128, dtype=np.int64).astype(np.int8)[:, None], (256, channels))
    out, _ = chain(x, q_in, steps)
    return np.ascontiguousarray(out[:, :rows].T).view(np.uint8)


def real_step(v, st, q_in):
    """One step in float64 with ONE rounding (half away from zero) and the same clamp: what the integer arithmetic approximates.
    Returns the UNROUNDED real result in units of the output's LSB, clamped to the step's range (so that a deviation is |int - real|)."""
    si, zi = float(f32(q_in[0])), q_in[1]
    v = np.asarray(v, np.float64)
    kind = st[0]
    lo, hi = -128, 127
    if kind == "add":
        _, k, (sk, zk), (so, zo), act = st
        so = float(f32(so))
        r = (si * (v - zi) + float(f32(sk)) * (np.asarray(k, np.float64) - zk)) / so + zo
        lo, hi = ar.activation_range(act, so, zo)
    elif kind == "prelu":
        _, alpha, (sa, za), (so, zo) = st
        so = float(f32(so))
        d = v - zi
        r = np.where(d >= 0, si * d, si * d * float(f32(sa)) * (np.asarray(alpha, np.float64) - za)) / so + zo
    elif kind == "clamp":
        _, (so, zo), act = st
        so = float(f32(so))
        r = si * (v - zi) / so + zo
        lo, hi = ar.activation_range(act, so, zo)
    else:
        _, (so, zo) = st
        r = si * (v - zi) / float(f32(so)) + zo
    return np.minimum(hi, np.maximum(lo, r))


# ---- seeded draws -------------------------------------------------------------------------------------------------------------------
def _scale(g, lo=1e-3, hi=1.0):
    return float(np.float32(np.exp(g.uniform(np.log(lo), np.log(hi)))))


def _zp(g):
    return int(g.choice([-128, 127, 0, int(g.integers(-128, 128)), int(g.integers(-20, 21))]))


def draw_step(g, kind, q_in, channels, per_channel):
    """One step of `kind` whose parameters the library accepts, for the input quantization q_in."""
    si = q_in[0]
    for _ in range(1000):
        zo = _zp(g)
        if kind == "add":
            sk, so = _scale(g), _scale(g, 2e-3, 2.0)
            zk = _zp(g)
            act = int(g.integers(0, 4))
            try:
                ar.prepare(si, q_in[1], sk, zk, so, zo, act)
            except ValueError:
                continue
            k = g.integers(-128, 128, channels).astype(np.int8) if per_channel else np.int8(g.integers(-128, 128))
            return ("add", k, (sk, zk), (so, zo), act)
        # a ratio on either side of 1: both signs of e
        so = float(np.float32(si * np.exp(g.uniform(np.log(1 / 64), np.log(64)))))
        if kind == "prelu":
            sa, za = _scale(g, 1e-3, 0.05), _zp(g)
            if per_channel:
                alpha = g.integers(-128, 128, channels).astype(np.int8)
                alpha[0] = za                                         # alpha == za: the negative side is flat
            else:
                alpha = np.int8(g.choice([za, -128, 127, int(g.integers(-128, 128))]))
            return ("prelu", alpha, (sa, za), (so, zo))
        if kind == "clamp":
            return ("clamp", (so, zo), int(g.integers(0, 4)))
        return ("requantize", (so, zo))
    raise AssertionError("no acceptable parameters drawn")


def draw_chain(g, channels, num_steps, per_channel=True, kinds=("add", "prelu", "clamp", "requantize")):
    """(q_in, steps): a chain of num_steps steps; with per_channel False every operand is a scalar (R = 1)."""
    q = (_scale(g), _zp(g))
    q_in, steps = q, []
    for _ in range(num_steps):
        kind = str(g.choice(kinds))
        st = draw_step(g, kind, q, channels, per_channel and bool(g.integers(0, 4)))
        steps.append(st)
        q = st[3] if kind in ("add", "prelu") else st[1]
    return q_in, steps


def draw_head(g, q_in):
    """(q_addend, q_out, act) of a head ADD the library accepts."""
    while True:
        h = ((_scale(g), _zp(g)), (_scale(g, 2e-3, 2.0), _zp(g)), int(g.integers(0, 4)))
        try:
            ar.prepare(q_in[0], q_in[1], h[0][0], h[0][1], h[1][0], h[1][1], h[2])
            return h
        except ValueError:
            continue


def reactnet_tail(g, channels):
    """The chain the feature is for: (q_in, head, steps) of ADD shortcut -> ADD shift -> PRELU -> ADD shift."""
    q_in = (_scale(g, 0.02, 0.1), _zp(g))
    head = draw_head(g, q_in)
    q = head[1]
    steps = []
    for kind in ("add", "prelu", "add"):
        st = draw_step(g, kind, q, channels, True)
        steps.append(st)
        q = st[3]
    return q_in, head, steps
