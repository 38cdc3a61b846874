"""NumPy reference of lce_hip_depthwise_conv2d_i8 (include/lce_hip.h): TFLite's reference_integer_ops::DepthwiseConvPerChannel
(dilation 1) in its default (double-rounding) build.  Output channel o reads input channel o // depth_multiplier.  Per output
element: acc = sum over the in-bounds taps of (x - zi) * w[fy][fx][o], exact (taps in the padding are skipped, the filter index
is the unclipped one); + bias[o]; MultiplyByQuantizedMultiplier with (m[o], e[o]) = QuantizeMultiplier(si * sw[o] / so) in
double; + zo; the clamp to CalculateActivationRangeQuantized at (so, zo).  The multipliers, the requantization and the finish are
tests/conv2d_i8_ref.py's, the window is tests/conv2d_ref.py's taps."""
import numpy as np

from conv2d_i8_ref import (INT32_MAX, NONE, RELU, RELU6, RELU_N1_TO_1, SAME, VALID, activation_range, bitpack, finish, multipliers,  # noqa: F401
                           out_and_pad, requantize)
from conv2d_ref import taps


def _pair(stride):
    return (stride, stride) if isinstance(stride, int) else tuple(stride)


def _filter(w):
    w = np.asarray(w)
    assert w.dtype == np.int8 and w.ndim in (3, 4) and (w.ndim == 3 or w.shape[0] == 1)
    return w.reshape(w.shape[-3:])


def accumulate(x, w, zi, stride=(1, 1), padding=SAME, depth_multiplier=1):
    """x: int8 [B, H, W, Cin]; w: int8 [1, fh, fw, Cout] (or [fh, fw, Cout]).  The exact sum over the in-bounds taps: int64
    [B, OH, OW, Cout]."""
    x, w, m = np.asarray(x), _filter(w), int(depth_multiplier)
    assert x.dtype == np.int8 and w.shape[2] == x.shape[3] * m
    tp, oh, ow = taps(x.shape[1:3], w.shape[:2], _pair(stride), padding)
    assert oh > 0 and ow > 0
    xs = x.astype(np.int64) - int(zi)
    xs = xs if m == 1 else np.repeat(xs, m, axis=3)          # output channel o reads input channel o // m
    acc = np.zeros((x.shape[0], oh, ow, w.shape[2]), np.int64)
    for fy, fx, (oy, ox), (iy, ix) in tp:
        acc[:, oy, ox, :] += xs[:, iy, ix, :] * w[fy, fx].astype(np.int64)
    return acc


def table(w, bias, filter_scales, si, so):
    """What lce_hip_depthwise_conv2d_i8_prepare writes: int32 [3, Cout] = bias[o] (0 without a bias), m[o], e[o].  Raises
    ValueError where the library answers LCE_HIP_ERR_UNSUPPORTED: the bounds of tests/conv2d_i8_ref.py's table with K = fh x fw."""
    w = _filter(w)
    cout, K = w.shape[2], w.shape[0] * w.shape[1]
    b = np.zeros(cout, np.int64) if bias is None else np.asarray(bias, np.int64)
    bound = 255 * 128 * K + int(np.abs(b).max(initial=0))
    if bound > INT32_MAX:
        raise ValueError("the accumulator bound %d exceeds 2^31 - 1" % bound)
    m, e = multipliers(si, filter_scales, so, cout)
    for o in range(cout):
        if e[o] > 0 and (bound << e[o]) > INT32_MAX:
            raise ValueError("channel %d: the bound %d times 2^%d exceeds 2^31 - 1" % (o, bound, e[o]))
    return np.stack([b, np.asarray(m, np.int64), np.asarray(e, np.int64)]).astype(np.int32)


def depthwise_i8(x, w, bias, filter_scales, q_in, q_out, stride=(1, 1), padding=SAME, depth_multiplier=1, activation=NONE):
    """lce_hip_depthwise_conv2d_i8 on NumPy arrays: int8 [B, OH, OW, Cout]."""
    return finish(accumulate(x, w, q_in[1], stride, padding, depth_multiplier), bias, filter_scales, q_in, q_out, activation)


def accumulate_float64(x, w, zi, stride=(1, 1), padding=SAME, depth_multiplier=1):
    """The cross-check of ``accumulate``: a float64 depthwise convolution of (x - zi) zero-padded, written without the taps (exact
    at these magnitudes: every partial sum is an integer below 2^53)."""
    x, w, m = np.asarray(x), _filter(w), int(depth_multiplier)
    (sh, sw), (fh, fw) = _pair(stride), w.shape[:2]
    (oh, ph), (ow, pw) = out_and_pad(x.shape[1], fh, sh, padding), out_and_pad(x.shape[2], fw, sw, padding)
    cout = w.shape[2]
    xp = np.zeros((x.shape[0], max((oh - 1) * sh + fh, ph + x.shape[1]), max((ow - 1) * sw + fw, pw + x.shape[2]), cout), np.float64)
    xp[:, ph:ph + x.shape[1], pw:pw + x.shape[2], :] = np.repeat(x.astype(np.float64) - float(zi), m, axis=3)
    out = np.zeros((x.shape[0], oh, ow, cout), np.float64)
    wf = w.astype(np.float64)
    for oy in range(oh):
        for ox in range(ow):
            out[:, oy, ox, :] = (xp[:, oy * sh:oy * sh + fh, ox * sw:ox * sw + fw, :] * wf[None]).sum(axis=(1, 2))
    return out
