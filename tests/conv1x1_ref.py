"""NumPy reference of lce_hip_conv1x1_f32 (include/lce_hip.h): the float 1x1 CONV_2D as a contracting build of TFLite's
reference_ops::Conv computes it.  Per output element, over input channels c = 0 .. Cin-1 in order: t = +0.0f;
t = fmaf(x[c], w[o][c], t); then t + bias[o] (skipped without a bias); then the clamp to the activation range.

NumPy has no fmaf, and float32(float64(a) * b + c) rounds twice.  ``fma32`` rounds the float64 sum to ODD first: the product of
two float32 is exact in float64 (48 significant bits, exponents within range), s = p + c is the correctly rounded sum, TwoSum
gives its exact error e, and where the sum was inexact and s's last mantissa bit is 0, s moves one ulp towards e -- the
neighbour with an odd last bit.  A round-to-odd result in 53 bits rounds to 24 bits (and to the float32 subnormals) exactly as
the unrounded sum does."""
import numpy as np

NONE, RELU, RELU_N1_TO_1, RELU6 = range(4)
FLT_MAX = np.float32(3.4028234663852886e38)
FLOAT_RANGE = {NONE: (-FLT_MAX, FLT_MAX), RELU: (np.float32(0), FLT_MAX), RELU_N1_TO_1: (np.float32(-1), np.float32(1)),
               RELU6: (np.float32(0), np.float32(6))}


def fma32(a, b, c):
    """Element-wise fmaf(a, b, c) of float32 arrays (broadcasting): ONE rounding of a * b + c to float32."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a * b                                            # exact
        s = p + c
        bb = s - p                                           # TwoSum (Knuth): s + e == p + c exactly
        e = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        move = (e != 0) & np.isfinite(s) & even              # (a NaN e compares unequal, but then s is not finite)
        towards = np.where(e > 0, np.inf, -np.inf)
        s = np.where(move, np.nextafter(s, towards), s)
        return s.astype(np.float32)


def out_hw(in_hw, stride):
    """A 1x1 filter has no padding taps: SAME and VALID both give ceil(in / stride)."""
    return tuple((i + s - 1) // s for i, s in zip(in_hw, stride))


def chain(x, w):
    """x [M, Cin], w [Cout, Cin] -> [M, Cout]: the fmaf chain over the channels in order, from +0.0."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    t = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for c in range(x.shape[1]):
        t = fma32(x[:, c:c + 1], w[None, :, c], t)
    return t


def clamp(t, activation):
    lo, hi = FLOAT_RANGE[activation]
    with np.errstate(invalid="ignore"):
        t = np.where(t < lo, lo, t)                          # std::max(t, lo): a NaN passes, -0.0 stays
        return np.where(hi < t, hi, t).astype(np.float32)    # std::min(t, hi)


def conv1x1(x, w, bias=None, stride=(1, 1), activation=NONE):
    """x: float32 [B, H, W, Cin]; w: float32 [Cout, Cin] (or [Cout, 1, 1, Cin]); bias: float32 [Cout] or None.  Returns float32
    [B, ceil(H / sh), ceil(W / sw), Cout]."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32).reshape(np.shape(w)[0], -1)
    stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
    xs = x[:, ::stride[0], ::stride[1], :]
    t = chain(xs.reshape(-1, x.shape[3]), w)
    if bias is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            t = t + np.asarray(bias, np.float32)[None, :]    # one float32 add
    return clamp(t, activation).reshape(xs.shape[:3] + (w.shape[0],))
