"""The int8 squeeze-and-excite gate of include/lce_hip.h (lce_hip_mul_int8, lce_hip_logistic_int8) restated in NumPy int64 /
float32 from the header's statement: MUL is MBQM((x1 - z1)(x2 - z2), m, e) + zo with (m, e) of the float32 s1 * s2 / so, the ADD
behind it is tests/int8_add_ref.py's on the MUL's int8 result, LOGISTIC is a table of the library's stated float LOGISTIC
(tests/activation_ref.py).  Nothing here shares code with the library.  ``real_mul`` and ``real_logistic`` are the real-valued
results in float64, for the deviation the header quotes.  No tests here."""
import numpy as np

import activation_ref
import elementwise_i8_ref as er
import int8_add_ref as ar

ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6 = 0, 1, 2, 3
LOGISTIC_OUT = (1.0 / 256.0, -128)
f32 = np.float32


def mul_params(q1, q2, qo, act=ACT_NONE):
    """(multiplier, shift, act_min, act_max) of the MUL: the real multiplier in float32, left to right, then widened."""
    real = f32(f32(q1[0]) * f32(q2[0])) / f32(qo[0])
    m, e = ar.quantize_multiplier(float(real))
    lo, hi = ar.activation_range(act, qo[0], qo[1])
    return m, e, lo, hi


def broadcast_gate(x, operand, rows_per_image=0):
    """The operand at every element of x [rows, C]: a tensor of x's shape, or a gate [rows / rows_per_image, C] whose element
    (n, c) serves the rows n * rows_per_image .. of image n."""
    x, operand = np.asarray(x), np.asarray(operand)
    if operand.shape == x.shape and not rows_per_image:
        return operand
    assert rows_per_image and x.shape[0] % rows_per_image == 0 and operand.shape == (x.shape[0] // rows_per_image, x.shape[1])
    return np.repeat(operand, rows_per_image, axis=0)


def mul_q(x, operand, q1, q2, qo, act=ACT_NONE, rows_per_image=0):
    """The int8 MUL of x [rows, C] by a tensor or a per-image gate; int8."""
    m, e, lo, hi = mul_params(q1, q2, qo, act)
    g = broadcast_gate(x, operand, rows_per_image)
    p = (np.asarray(x, np.int64) - q1[1]) * (np.asarray(g, np.int64) - q2[1])
    return np.minimum(hi, np.maximum(lo, er.mbqm(p, m, e) + qo[1])).astype(np.int8)


def mul_add_q(x, operand, addend, q1, q2, qo, act, q_addend, q_sum, add_act=ACT_NONE, rows_per_image=0):
    """MUL, then int8_add_ref's ADD of (the product at qo, the addend at q_addend) to q_sum; int8."""
    p = mul_q(x, operand, q1, q2, qo, act, rows_per_image)
    return ar.add_q(p, np.asarray(addend), (qo[0], qo[1], q_addend[0], q_addend[1], q_sum[0], q_sum[1]), add_act)


def logistic_table(q_in):
    """uint8 [256]: table[v + 128] is the int8 LOGISTIC, as a byte, of the value v at q_in; the output is at (1/256, -128)."""
    si, zi = f32(q_in[0]), int(q_in[1])
    v = np.arange(-128, 128, dtype=np.int64)
    x = (si * (v - zi).astype(np.float32)).astype(np.float32)
    y = (activation_ref.logistic(x) * f32(256)).astype(np.float32).astype(np.float64)
    r = np.floor(y + 0.5).astype(np.int64) - 128          # round half away from zero: y >= 0
    return np.clip(r, -128, 127).astype(np.int8).view(np.uint8)


def logistic_q(x, q_in):
    return logistic_table(q_in)[np.asarray(x, np.int64) + 128].view(np.int8)


def real_mul(x1, x2, q1, q2, qo, act=ACT_NONE):
    """s1 s2 (x1 - z1)(x2 - z2) / so + zo in float64 (not rounded), clamped to the activation range."""
    s1, s2, so = float(f32(q1[0])), float(f32(q2[0])), float(f32(qo[0]))
    lo, hi = ar.activation_range(act, qo[0], qo[1])
    v = s1 * s2 * (np.asarray(x1, np.float64) - q1[1]) * (np.asarray(x2, np.float64) - q2[1]) / so + qo[1]
    return np.clip(v, lo, hi)


def real_logistic(q_in):
    """256 / (1 + exp(-x)) - 128 in float64 for every int8 input at q_in, clamped to [-128, 127]."""
    x = float(f32(q_in[0])) * (np.arange(-128, 128, dtype=np.float64) - q_in[1])
    return np.clip(256.0 / (1.0 + np.exp(-x)) - 128.0, -128, 127)


def mul_draws(n, seed=0):
    """n seeded (q1, q2, qo) with the output scale chosen so that the products span most of the int8 range without sitting on its
    bounds: so is s1 s2 times the largest |(x1 - z1)(x2 - z2)| over 60 to 150 and the output zero point lies in [-30, 30], so only
    the largest products of a draw reach a clamp bound."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = np.exp(g.uniform(np.log(1e-3), np.log(1.0), 2)).astype(np.float32)
        z = [int(v) for v in g.integers(-128, 128, 2)] + [int(g.integers(-30, 31))]
        big = max(abs(-128 - z[0]), abs(127 - z[0])) * max(abs(-128 - z[1]), abs(127 - z[1]))
        so = f32(float(s[0]) * float(s[1]) * big / g.uniform(60.0, 150.0))
        out.append(((float(s[0]), z[0]), (float(s[1]), z[1]), (float(so), z[2])))
    return out
