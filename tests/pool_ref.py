"""NumPy reference of lce_hip_pool2d (include/lce_hip.h): TFLite's builtin MAX_POOL_2D / AVERAGE_POOL_2D as its reference
kernels compute them, restated.  One loop over the filter taps (fy, fx) in raster order on whole-tensor slices: float32
accumulation for AVERAGE (one rounding per add, in tap order), a per-output count of in-bounds taps, a truncating integer
division for int8, then the clamp to the activation range.  Taps in the padding are excluded."""
import numpy as np

SAME, VALID = 0, 1
MAX, AVERAGE = 0, 1
NONE, RELU, RELU_N1_TO_1, RELU6 = range(4)
FLT_MAX = np.float32(3.4028234663852886e38)
FLOAT_RANGE = {NONE: (-FLT_MAX, FLT_MAX), RELU: (np.float32(0), FLT_MAX), RELU_N1_TO_1: (np.float32(-1), np.float32(1)),
               RELU6: (np.float32(0), np.float32(6))}


def out_and_pad(size, filt, stride, padding):
    """(output extent, padding in front) of one axis: ComputeOutSize and ComputePaddingHeightWidth's total // 2."""
    out = (size + stride - 1) // stride if padding == SAME else (size + stride - filt) // stride
    return out, max(0, (out - 1) * stride + filt - size) // 2


def quantized_range(activation, scale, zero_point):
    """CalculateActivationRangeQuantized for int8: Q(f) = zero_point + round(f / scale), the division in float32 and the
    rounding half away from zero (TfLiteRound)."""
    def q(f):
        r = np.float32(f) / np.float32(scale)
        return int(zero_point) + int(np.sign(r) * np.floor(np.abs(np.float64(r)) + 0.5))
    lo, hi = -128, 127
    if activation == RELU:
        lo = max(lo, q(0.0))
    elif activation == RELU6:
        lo, hi = max(lo, q(0.0)), min(hi, q(6.0))
    elif activation == RELU_N1_TO_1:
        lo, hi = max(lo, q(-1.0)), min(hi, q(1.0))
    return lo, hi


def windows(shape, filt, stride, padding):
    """Per tap (fy, fx) in raster order: (output rows oy0:oy1, output columns ox0:ox1, input slices) for which the tap lies
    inside the image, plus the output extents."""
    _, h, w, _ = shape
    (fh, fw), (sh, sw) = filt, stride
    (oh, ph), (ow, pw) = out_and_pad(h, fh, sh, padding), out_and_pad(w, fw, sw, padding)

    def span(n_out, size, f, s, p):                      # outputs o with 0 <= o * s - p + f < size
        lo = max(0, -((f - p) // s))                     # ceil((p - f) / s)
        hi = min(n_out, (size - 1 + p - f) // s + 1)
        return lo, max(lo, hi)
    taps = []
    for fy in range(fh):
        y0, y1 = span(oh, h, fy, sh, ph)
        for fx in range(fw):
            x0, x1 = span(ow, w, fx, sw, pw)
            if y1 > y0 and x1 > x0:
                iy, ix = y0 * sh - ph + fy, x0 * sw - pw + fx
                taps.append(((slice(y0, y1), slice(x0, x1)),
                             (slice(iy, iy + (y1 - y0 - 1) * sh + 1, sh), slice(ix, ix + (x1 - x0 - 1) * sw + 1, sw))))
    return taps, oh, ow


def pool2d(x, op, filt, stride, padding, activation=NONE, scale=None, zero_point=0):
    """x: float32 or int8 [B, H, W, C].  Returns the pooled tensor of x's dtype."""
    x = np.asarray(x)
    b, _, _, c = x.shape
    taps, oh, ow = windows(x.shape, filt, stride, padding)
    assert oh > 0 and ow > 0
    count = np.zeros((1, oh, ow, 1), np.int32)
    is_float = x.dtype == np.float32
    if op == MAX:
        acc = np.full((b, oh, ow, c), -FLT_MAX if is_float else -128, np.float32 if is_float else np.int32)
    else:
        acc = np.zeros((b, oh, ow, c), np.float32 if is_float else np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for (oy, ox), (iy, ix) in taps:
            v = x[:, iy, ix, :]
            if not is_float:
                v = v.astype(np.int32)
            if op == MAX:
                a = acc[:, oy, ox, :]
                acc[:, oy, ox, :] = np.where(a < v, v, a)             # m = (m < x) ? x : m: a NaN never replaces m
            else:
                acc[:, oy, ox, :] = acc[:, oy, ox, :] + v             # float32: one rounding per add, in tap order
            count[:, oy, ox, :] += 1
        if is_float:
            r = acc if op == MAX else (acc / count.astype(np.float32)).astype(np.float32)
            lo, hi = FLOAT_RANGE[activation]
            r = np.where(r < lo, lo, r)                               # std::max(r, lo): a NaN passes
            return np.where(hi < r, hi, r).astype(np.float32)         # std::min(r, hi)
    if op == AVERAGE:
        n = np.broadcast_to(count, acc.shape).astype(np.int64)
        a = acc.astype(np.int64)
        num = np.where(a > 0, a + n // 2, a - n // 2)
        acc = (np.sign(num) * (np.abs(num) // n)).astype(np.int32)    # C's truncating division
    lo, hi = quantized_range(activation, scale, zero_point)
    return np.clip(acc, lo, hi).astype(np.int8)
