"""NumPy reference of lce_hip_depthwise_conv2d_f32 (include/lce_hip.h): TFLite's float reference_ops::DepthwiseConv as a
contracting build computes it.  Output channel o reads input channel o // depth_multiplier.  Per output element, over its
in-bounds taps in raster order (filter row, then filter column; taps in the padding are skipped, the filter index is the
unclipped one): t = +0.0f; t = fmaf(x, w[fy][fx][o], t); then t + bias[o] (skipped without a bias); then the clamp to the
activation range.  Extents and padding are the pools' (tests/pool_ref.py); the fmaf is tests/conv1x1_ref.py's, which is checked
against libm."""
import numpy as np

from conv1x1_ref import FLOAT_RANGE, NONE, RELU, RELU6, RELU_N1_TO_1, clamp, fma32  # noqa: F401  (re-exported)
from pool_ref import SAME, VALID, out_and_pad  # noqa: F401

BLUR = (np.outer([1, 2, 1], [1, 2, 1]) / 16.0).astype(np.float32)      # QuickNet's fixed [1 2 1] x [1 2 1] / 16


def taps(in_hw, filt, stride, padding):
    """Per filter tap (fy, fx) in raster order that lies inside the image for some output: (fy, fx, output rows and columns as
    slices, input rows and columns as slices).  Also the output extents."""
    (h, w), (fh, fw), (sh, sw) = in_hw, filt, stride
    (oh, ph), (ow, pw) = out_and_pad(h, fh, sh, padding), out_and_pad(w, fw, sw, padding)

    def span(n_out, size, f, s, p):                          # outputs o with 0 <= o * s - p + f < size
        lo = max(0, -((f - p) // s))                         # ceil((p - f) / s)
        hi = min(n_out, (size - 1 + p - f) // s + 1)
        return lo, max(lo, hi)
    out = []
    for fy in range(fh):
        y0, y1 = span(oh, h, fy, sh, ph)
        for fx in range(fw):
            x0, x1 = span(ow, w, fx, sw, pw)
            if y1 > y0 and x1 > x0:
                iy, ix = y0 * sh - ph + fy, x0 * sw - pw + fx
                out.append((fy, fx, (slice(y0, y1), slice(x0, x1)),
                            (slice(iy, iy + (y1 - y0 - 1) * sh + 1, sh), slice(ix, ix + (x1 - x0 - 1) * sw + 1, sw))))
    return out, oh, ow


def chain(x, w, stride=(1, 1), padding=SAME, depth_multiplier=1):
    """x: float32 [B, H, W, Cin]; w: float32 [fh, fw, Cout] (or [1, fh, fw, Cout]).  The fmaf chain alone, before bias and
    clamp: float32 [B, OH, OW, Cout]."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    w = w.reshape(w.shape[-3:])
    m = int(depth_multiplier)
    assert w.shape[2] == x.shape[3] * m
    stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
    tp, oh, ow = taps(x.shape[1:3], w.shape[:2], stride, padding)
    assert oh > 0 and ow > 0
    xm = x if m == 1 else np.repeat(x, m, axis=3)            # output channel o reads input channel o // m
    t = np.zeros((x.shape[0], oh, ow, w.shape[2]), np.float32)
    for fy, fx, (oy, ox), (iy, ix) in tp:
        t[:, oy, ox, :] = fma32(xm[:, iy, ix, :], w[fy, fx][None, None, None, :], t[:, oy, ox, :])
    return t


def finish(t, bias=None, activation=NONE):
    """The bias add (one float32 add, skipped without a bias) and the clamp on a chain's result."""
    if bias is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (t + np.asarray(bias, np.float32)[None, None, None, :]).astype(np.float32)
    return clamp(t, activation)


def depthwise(x, w, bias=None, stride=(1, 1), padding=SAME, depth_multiplier=1, activation=NONE):
    """lce_hip_depthwise_conv2d_f32 on NumPy arrays."""
    return finish(chain(x, w, stride, padding, depth_multiplier), bias, activation)
