"""TensorFlow Lite's builtin int8 ADD restated in NumPy from its definition (the double-rounding build): Prepare's parameters
(QuantizeMultiplier, CalculateActivationRangeQuantized) and reference_integer_ops::Add per element
(SaturatingRoundingDoublingHighMul, RoundingDivideByPOT).  This is what lce_hip_add_int8 must reproduce byte for byte; it is
NOT the correctly rounded (s1 (x1 - z1) + s2 (x2 - z2)) / so, which ``real_rounding`` gives for comparison."""
import math
import zlib

import numpy as np

ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6 = 0, 1, 2, 3
LEFT_SHIFT = 20
PARAM_NAMES = ("left_shift", "in1_multiplier", "in1_shift", "in2_multiplier", "in2_shift", "out_multiplier", "out_shift",
               "act_min", "act_max")

# the known answers of the feature's specification: (s1, z1, s2, z2, so, zo).  Each scale is the float32 nearest the decimal.
SET_A = (0.05, -3, 0.0371, 5, 0.0712, -7)
SET_B = (0.0157, -128, 0.0314, 0, 0.0235, -128)
SET_C = (0.02, 0, 0.023, 0, 0.031, 0)


def round_half_away(v: float) -> int:
    """std::round / TfLiteRound."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def quantize_multiplier(d: float):
    """QuantizeMultiplier (tensorflow/lite/kernels/internal/quantization_util.cc): d = m * 2^(e - 31), m in [2^30, 2^31)."""
    if d == 0.0:
        return 0, 0
    q, e = math.frexp(d)
    m = round_half_away(q * float(1 << 31))
    assert m <= (1 << 31)
    if m == (1 << 31):
        m //= 2
        e += 1
    if e < -31:
        e, m = 0, 0
    return int(m), int(e)


def activation_range(activation: int, so, zo: int):
    """CalculateActivationRangeQuantized for int8: Q(f) = zo + round(f / so), the division in float32."""
    so = np.float32(so)

    def q(f):
        return int(zo) + round_half_away(float(np.float32(f) / so))
    lo, hi = -128, 127
    if activation == ACT_RELU:
        lo = max(lo, q(0.0))
    elif activation == ACT_RELU6:
        lo, hi = max(lo, q(0.0)), min(hi, q(6.0))
    elif activation == ACT_RELU_N1_TO_1:
        lo, hi = max(lo, q(-1.0)), min(hi, q(1.0))
    elif activation != ACT_NONE:
        raise ValueError("unknown activation %r" % (activation,))
    return lo, hi


def prepare(s1, z1, s2, z2, so, zo, activation=ACT_NONE):
    """The nine numbers of lce_hip_add_int8_params, in PARAM_NAMES order.  Raises ValueError when a real multiplier is not in
    (0, 1)."""
    s1, s2, so = float(np.float32(s1)), float(np.float32(s2)), float(np.float32(so))
    twice_max = 2.0 * max(s1, s2)
    reals = (s1 / twice_max, s2 / twice_max, twice_max / (float(1 << LEFT_SHIFT) * so))
    for r in reals:
        if not 0.0 < r < 1.0:
            raise ValueError("real multiplier %r is not in (0, 1)" % r)
    (m1, e1), (m2, e2), (mo, eo) = (quantize_multiplier(r) for r in reals)
    lo, hi = activation_range(activation, so, zo)
    return (LEFT_SHIFT, m1, e1, m2, e2, mo, eo, lo, hi)


def srdhm(a, b: int):
    """SaturatingRoundingDoublingHighMul on int64 arrays holding int32 values."""
    a = np.asarray(a, np.int64)
    p = a * np.int64(b)
    nudge = np.where(p >= 0, np.int64(1 << 30), np.int64(1 - (1 << 30)))
    t = p + nudge
    q = np.where(t >= 0, t >> 31, -((-t) >> 31))          # C++ truncating division by 2^31
    return np.where((a == -(1 << 31)) & (b == -(1 << 31)), np.int64((1 << 31) - 1), q)


def rdivpot(x, n: int):
    """RoundingDivideByPOT on int64 arrays holding int32 values, 0 <= n <= 31."""
    x = np.asarray(x, np.int64)
    mask = np.int64((1 << n) - 1)
    rem = x & mask
    thr = (mask >> 1) + (x < 0)
    return (x >> n) + (rem > thr)


def add(x1, x2, z1, z2, zo, params):
    """reference_integer_ops::Add on int8 arrays; `params` from ``prepare``."""
    ls, m1, e1, m2, e2, mo, eo, lo, hi = params
    x1, x2 = np.asarray(x1), np.asarray(x2)
    if x1.size > (1 << 22):                                   # (int64 temporaries: a large tensor goes in pieces)
        f1, f2 = x1.reshape(-1), x2.reshape(-1)
        parts = [add(f1[k:k + (1 << 22)], f2[k:k + (1 << 22)], z1, z2, zo, params) for k in range(0, f1.size, 1 << 22)]
        return np.concatenate(parts).reshape(x1.shape)
    a = (np.asarray(x1, np.int64) - z1) << ls
    b = (np.asarray(x2, np.int64) - z2) << ls
    sa = rdivpot(srdhm(a, m1), -e1)
    sb = rdivpot(srdhm(b, m2), -e2)
    raw = rdivpot(srdhm(sa + sb, mo), -eo) + zo
    return np.minimum(hi, np.maximum(lo, raw)).astype(np.int8)


def add_q(x1, x2, q, activation=ACT_NONE):
    """``add`` from the six quantization numbers q = (s1, z1, s2, z2, so, zo)."""
    return add(x1, x2, q[1], q[3], q[5], prepare(*q, activation))


def all_pairs():
    """Every (x1, x2) pair as two [256, 256] int8 tensors: x1 along axis 0, both from -128 to 127."""
    v = np.arange(-128, 128, dtype=np.int64).astype(np.int8)
    return np.ascontiguousarray(np.broadcast_to(v[:, None], (256, 256))), np.ascontiguousarray(np.broadcast_to(v[None, :], (256, 256)))


def real_rounding(x1, x2, q, activation=ACT_NONE):
    """round_half_away((s1 (x1 - z1) + s2 (x2 - z2)) / so) + zo in double, clamped to the same activation range."""
    s1, z1, s2, z2, so, zo = q
    s1, s2, so = float(np.float32(s1)), float(np.float32(s2)), float(np.float32(so))
    lo, hi = activation_range(activation, so, zo)
    v = (s1 * (np.asarray(x1, np.float64) - z1) + s2 * (np.asarray(x2, np.float64) - z2)) / so
    r = np.where(v >= 0, np.floor(np.abs(v) + 0.5), -np.floor(np.abs(v) + 0.5)).astype(np.int64) + zo
    return np.minimum(hi, np.maximum(lo, r)).astype(np.int8)


def table_row(q, activation=ACT_NONE):
    """One row of the known-answer table: (params, bytes that differ from real rounding, sum, CRC-32 hex, saturated share)."""
    x1, x2 = all_pairs()
    p = prepare(*q, activation)
    t = add(x1, x2, q[1], q[3], q[5], p)
    diff = int(np.count_nonzero(t != real_rounding(x1, x2, q, activation)))
    sat = float(np.mean((t == p[7]) | (t == p[8])))
    return p, diff, int(t.astype(np.int64).sum()), "%08x" % (zlib.crc32(t.tobytes()) & 0xFFFFFFFF), sat


def bitpack(out, zo: int):
    """LceQuantize of an int8 tensor at zero point zo: bit = out < zo, LSB first, ceil(C/32) int32 words per row."""
    out = np.asarray(out)
    C = out.shape[-1]
    words = (C + 31) // 32
    neg = np.zeros(out.shape[:-1] + (words * 32,), np.uint64)
    neg[..., :C] = out.astype(np.int64) < zo
    w = (neg.reshape(out.shape[:-1] + (words, 32)) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


def random_sets(n: int, seed: int = 0):
    """n seeded parameter sets with scales in [1e-3, 1] (log-uniform) and zero points in [-128, 127] whose three real
    multipliers lie in (0, 1)."""
    g = np.random.default_rng(seed)
    sets = []
    while len(sets) < n:
        s = np.exp(g.uniform(np.log(1e-3), np.log(1.0), 3)).astype(np.float32)
        z = g.integers(-128, 128, 3)
        q = (float(s[0]), int(z[0]), float(s[1]), int(z[1]), float(s[2]), int(z[2]))
        try:
            prepare(*q)
        except ValueError:
            continue
        sets.append(q)
    return sets
