"""NumPy reference of lce_hip_conv2d_i8 (include/lce_hip.h): TFLite's reference_integer_ops::ConvPerChannel (groups 1,
dilation 1) in its default (double-rounding) build.  Per output element: acc = sum over the in-bounds taps and the channels of
(x - zi) * w, exact (taps in the padding are skipped); + bias[o]; MultiplyByQuantizedMultiplier with
(m[o], e[o]) = QuantizeMultiplier(si * sw[o] / so) in double; + zo; the clamp to CalculateActivationRangeQuantized at (so, zo).
The gemmlowp steps, QuantizeMultiplier and the activation range are tests/int8_add_ref.py's; the window is
tests/depthwise_ref.py's taps with the pools' extents and padding (tests/conv2d_ref.py)."""
import numpy as np

from conv2d_ref import SAME, VALID, out_and_pad, taps  # noqa: F401  (re-exported)
from int8_add_ref import ACT_NONE, ACT_RELU, ACT_RELU6, ACT_RELU_N1_TO_1, activation_range, bitpack, quantize_multiplier, rdivpot, srdhm  # noqa: F401

NONE, RELU, RELU_N1_TO_1, RELU6 = ACT_NONE, ACT_RELU, ACT_RELU_N1_TO_1, ACT_RELU6
INT32_MAX = (1 << 31) - 1


def _pair(stride):
    return (stride, stride) if isinstance(stride, int) else tuple(stride)


def accumulate(x, w, zi, stride=(1, 1), padding=SAME):
    """x: int8 [B, H, W, Cin]; w: int8 [Cout, fh, fw, Cin].  The exact sum over the in-bounds taps: int64 [B, OH, OW, Cout]."""
    x, w = np.asarray(x), np.asarray(w)
    assert x.dtype == np.int8 and w.dtype == np.int8 and w.ndim == 4 and w.shape[3] == x.shape[3]
    tp, oh, ow = taps(x.shape[1:3], w.shape[1:3], _pair(stride), padding)
    assert oh > 0 and ow > 0
    xs = x.astype(np.int64) - int(zi)
    acc = np.zeros((x.shape[0], oh, ow, w.shape[0]), np.int64)
    for fy, fx, (oy, ox), (iy, ix) in tp:
        acc[:, oy, ox, :] += xs[:, iy, ix, :] @ w[:, fy, fx, :].astype(np.int64).T
    return acc


def scales_of(filter_scales, cout):
    s = np.atleast_1d(np.asarray(filter_scales, np.float32))
    assert s.ndim == 1 and s.size in (1, cout)
    return np.broadcast_to(s, (cout,))


def multipliers(si, filter_scales, so, cout):
    """(m[o], e[o]) = QuantizeMultiplier((double)si * (double)sw[o] / (double)so), the scales float32: two int lists."""
    si, so = float(np.float32(si)), float(np.float32(so))
    pairs = [quantize_multiplier(si * float(s) / so) for s in scales_of(filter_scales, cout)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def requantize(acc, m: int, e: int):
    """MultiplyByQuantizedMultiplier on an int64 array holding int32 values: RDivPOT(SRDHM(acc * 2^max(e, 0), m), max(-e, 0))."""
    acc = np.asarray(acc, np.int64)
    shifted = acc << max(e, 0)
    assert shifted.size == 0 or (shifted.max() <= INT32_MAX and shifted.min() >= -INT32_MAX - 1), "the reference itself would overflow"
    return rdivpot(srdhm(shifted, m), max(-e, 0))


def table(w, bias, filter_scales, si, zi, so):
    """What lce_hip_conv2d_i8_prepare writes: int32 [3, Cout] = c[o] = bias[o] - zi * sum(w[o]), m[o], e[o].  Raises ValueError
    where the library answers LCE_HIP_ERR_UNSUPPORTED."""
    w = np.asarray(w)
    cout, K = w.shape[0], int(np.prod(w.shape[1:]))
    b = np.zeros(cout, np.int64) if bias is None else np.asarray(bias, np.int64)
    bound = 255 * 128 * K + int(np.abs(b).max(initial=0))
    if bound > INT32_MAX:
        raise ValueError("the accumulator bound %d exceeds 2^31 - 1" % bound)
    m, e = multipliers(si, filter_scales, so, cout)
    for o in range(cout):
        if e[o] > 0 and (bound << e[o]) > INT32_MAX:
            raise ValueError("channel %d: the bound %d times 2^%d exceeds 2^31 - 1" % (o, bound, e[o]))
    c = b - int(zi) * w.reshape(cout, -1).astype(np.int64).sum(1)
    assert np.abs(c).max(initial=0) <= INT32_MAX
    return np.stack([c, np.asarray(m, np.int64), np.asarray(e, np.int64)]).astype(np.int32)


def finish(acc, bias, filter_scales, q_in, q_out, activation=NONE):
    """Bias, requantization, zero point and clamp on ``accumulate``'s result: int8."""
    (si, _), (so, zo) = q_in, q_out
    cout = acc.shape[-1]
    m, e = multipliers(si, filter_scales, so, cout)
    acc = np.asarray(acc, np.int64) + (0 if bias is None else np.asarray(bias, np.int64))
    v = np.empty_like(acc)
    for o in range(cout):
        v[..., o] = requantize(acc[..., o], m[o], e[o])
    lo, hi = activation_range(activation, so, zo)
    return np.minimum(hi, np.maximum(lo, v + int(zo))).astype(np.int8)


def conv2d_i8(x, w, bias, filter_scales, q_in, q_out, stride=(1, 1), padding=SAME, activation=NONE):
    """lce_hip_conv2d_i8 on NumPy arrays: int8 [B, OH, OW, Cout]."""
    return finish(accumulate(x, w, q_in[1], stride, padding), bias, filter_scales, q_in, q_out, activation)


def accumulate_float64(x, w, zi, stride=(1, 1), padding=SAME):
    """The cross-check of ``accumulate``: a float64 convolution of (x - zi) zero-padded, written without the taps (exact at
    these magnitudes: every partial sum is an integer below 2^53)."""
    x, w = np.asarray(x), np.asarray(w)
    (sh, sw), (fh, fw) = _pair(stride), w.shape[1:3]
    (oh, ph), (ow, pw) = out_and_pad(x.shape[1], fh, sh, padding), out_and_pad(x.shape[2], fw, sw, padding)
    xp = np.zeros((x.shape[0], max((oh - 1) * sh + fh, ph + x.shape[1]), max((ow - 1) * sw + fw, pw + x.shape[2]), x.shape[3]), np.float64)
    xp[:, ph:ph + x.shape[1], pw:pw + x.shape[2], :] = x.astype(np.float64) - float(zi)
    out = np.zeros((x.shape[0], oh, ow, w.shape[0]), np.float64)
    wf = w.astype(np.float64).reshape(w.shape[0], -1)
    for oy in range(oh):
        for ox in range(ow):
            win = xp[:, oy * sh:oy * sh + fh, ox * sw:ox * sw + fw, :].reshape(x.shape[0], -1)
            out[:, oy, ox, :] = win @ wf.T
    return out
