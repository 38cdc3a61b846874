"""NumPy restatements of the int8 classifier head and the float / int8 boundary as include/lce_hip.h states them:
lce_hip_fully_connected_i8 (tests/conv2d_i8_ref.py on the one-pixel image), lce_hip_mean_i8 (the gemmlowp steps of
tests/int8_add_ref.py, then the division rounding half away from zero), lce_hip_softmax_i8 (the stated exp and the fixed-order
sum of tests/head_ref.py), lce_hip_quantize_f32_i8 and lce_hip_dequantize_i8_f32; and the float64 answers they are measured
against.  No tests here."""
import numpy as np

import conv2d_i8_ref as CR
import head_ref as HR
from int8_add_ref import quantize_multiplier, rdivpot, srdhm

NONE, RELU, RELU_N1_TO_1, RELU6 = CR.NONE, CR.RELU, CR.RELU_N1_TO_1, CR.RELU6
INT32_MAX = (1 << 31) - 1
SOFTMAX_OUT = (1.0 / 256.0, -128)


def fully_connected_i8(x, w, bias, weight_scales, q_in, q_out, activation=NONE):
    """x: int8 [B, K]; w: int8 [N, K]; bias: int32 [N] or None -> int8 [B, N]: lce_hip_conv2d_i8 on [B, 1, 1, K] with a 1x1 filter."""
    x, w = np.asarray(x), np.asarray(w)
    y = CR.conv2d_i8(x.reshape(x.shape[0], 1, 1, x.shape[1]), w.reshape(w.shape[0], 1, 1, w.shape[1]), bias, weight_scales, q_in, q_out,
                     (1, 1), CR.VALID, activation)
    return y.reshape(x.shape[0], w.shape[0])


def fc_table(w, bias, weight_scales, si, zi, so):
    """What lce_hip_fully_connected_i8_prepare writes: conv2d_i8_ref.table of the 1x1 filter."""
    w = np.asarray(w)
    return CR.table(w.reshape(w.shape[0], 1, 1, w.shape[1]), bias, weight_scales, si, zi, so)


def mean_multiplier(si, so):
    """(m, e) = QuantizeMultiplier((double)si / (double)so), the scales float32."""
    return quantize_multiplier(float(np.float32(si)) / float(np.float32(so)))


def mean_bound_ok(n: int, e: int) -> bool:
    """lce_hip_mean_i8_prepare's bound: 255 n 2^max(e, 0) + n/2 <= 2^31 - 1."""
    left = max(e, 0)
    return left < 31 and ((255 * n) << left) + n // 2 <= INT32_MAX


def trunc_div(a, n: int):
    """C++ int division (truncating) of an int64 array by n > 0."""
    a = np.asarray(a, np.int64)
    return np.where(a >= 0, a // n, -((-a) // n))


def mean_i8(x, q_in, q_out):
    """x: int8 [B, H, W, C] -> int8 [B, C]."""
    x = np.asarray(x)
    assert x.dtype == np.int8 and x.ndim == 4
    (si, zi), (so, zo) = q_in, q_out
    n = x.shape[1] * x.shape[2]
    m, e = mean_multiplier(si, so)
    if not mean_bound_ok(n, e):
        raise ValueError("an intermediate could leave int32: n = %d, e = %d" % (n, e))
    acc = (x.astype(np.int64) - int(zi)).sum(axis=(1, 2))
    t = rdivpot(srdhm(acc << max(e, 0), m), max(-e, 0))
    q = np.where(t > 0, trunc_div(t + n // 2, n), trunc_div(t - n // 2, n))
    return np.minimum(127, np.maximum(-128, q + int(zo))).astype(np.int8)


def mean_exact(x, q_in, q_out):
    """The real-valued answer in output units before the zero point: acc si / (n so), float64 (acc exact)."""
    x = np.asarray(x)
    n = x.shape[1] * x.shape[2]
    acc = (x.astype(np.int64) - int(q_in[1])).sum(axis=(1, 2)).astype(np.float64)
    return acc * float(np.float32(q_in[0])) / (n * float(np.float32(q_out[0])))


def round_half_away(v):
    """std::round on a float array."""
    v = np.asarray(v)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def roundf32(t):
    """roundf on a float32 array, without a float add that could round: trunc, then the exact remainder against 0.5."""
    t = np.asarray(t, np.float32)
    r = np.trunc(t)
    rest = np.abs(t - r)                   # exact: t and trunc(t) share an exponent range in which the difference is representable
    return (r + np.where(rest >= np.float32(0.5), np.sign(t), np.float32(0))).astype(np.float32)


def softmax_i8(q, input_scale, beta=1.0):
    """q: int8 [..., cols] -> int8 of the same shape at (1/256, -128)."""
    q = np.asarray(q)
    assert q.dtype == np.int8
    rows = q.reshape(-1, q.shape[-1]).astype(np.int32)
    d = rows - rows.max(axis=1, keepdims=True)
    sb = np.float32(np.float32(input_scale) * np.float32(beta))
    a = (d.astype(np.float32) * sb).astype(np.float32)
    e = HR.exp32(a)
    p = (e / HR.wave_sum(e)[:, None]).astype(np.float32)
    t = (p * np.float32(256.0)).astype(np.float32)
    v = np.minimum(roundf32(t).astype(np.int32) - 128, 127)
    return v.astype(np.int8).reshape(q.shape)


def softmax_exact(q, input_scale, beta=1.0):
    """256 * softmax in float64: what the output's integer (before - 128) approximates."""
    rows = np.asarray(q).reshape(-1, np.shape(q)[-1]).astype(np.float64)
    a = (rows - rows.max(axis=1, keepdims=True)) * (float(np.float32(input_scale)) * float(np.float32(beta)))
    e = np.exp(a)
    return (256.0 * e / e.sum(axis=1, keepdims=True)).reshape(np.shape(q))


def quantize(x, scale, zp):
    """float32 -> int8: the IEEE float32 division, roundf, the clamp in float, + zp; a NaN gives zp."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (x / np.float32(scale)).astype(np.float32)
        nan = np.isnan(t)
        fin = np.where(np.isinf(t) | nan, np.float32(0), t)
        r = np.where(np.isinf(t), t, roundf32(fin))
        r = np.minimum(np.maximum(r, np.float32(-128 - zp)), np.float32(127 - zp))
        return (np.where(nan, np.float32(0), r).astype(np.int32) + int(zp)).astype(np.int8)


def dequantize(q, scale, zp):
    """int8 -> float32: (float)(q - zp) * scale, one float32 multiply."""
    return ((np.asarray(q).astype(np.int32) - int(zp)).astype(np.float32) * np.float32(scale)).astype(np.float32)
