"""NumPy float32 restatements of the classifier head as include/lce_hip.h states it: MEAN over height and width (the AVERAGE
pool whose filter is the image, tests/pool_ref.py), lce_hip_fully_connected_f32 (the fmaf chain of tests/conv1x1_ref.py) and
lce_hip_softmax_f32 (its own exp and its own order of the sum).  No tests here."""
import numpy as np

import conv1x1_ref as CR
import pool_ref as PR

NONE, RELU, RELU_N1_TO_1, RELU6 = range(4)
LOG2E = np.float32(1.44269502)
LN2_HI = np.float32(0.693145751953125)
LN2_LO = np.float32(1.42860676e-06)
EXP_COEFFS = tuple(np.float32(c) for c in (1.38888892e-03, 8.33333377e-03, 4.16666679e-02, 1.66666672e-01, 0.5, 1.0, 1.0))
EXP_LEAD = np.float32(1.98412701e-04)
TWO_M64 = np.float32(2.0 ** -64)


def mean_hw(x, keep_dims=False):
    """x: float32 [B, H, W, C] -> [B, C] (or [B, 1, 1, C]): the sum over the pixels in raster order from +0.0f, one rounding per
    add, then one division by H * W."""
    x = np.asarray(x, np.float32)
    y = PR.pool2d(x, PR.AVERAGE, x.shape[1:3], (1, 1), PR.VALID)
    return y if keep_dims else y.reshape(x.shape[0], x.shape[3])


def fully_connected(x, w, bias=None, activation=NONE):
    """x: float32 [B, K]; w: float32 [N, K]; bias: float32 [N] or None -> [B, N]."""
    t = CR.chain(np.asarray(x, np.float32).reshape(np.shape(x)[0], -1), w)
    if bias is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            t = t + np.asarray(bias, np.float32)[None, :]    # one float32 add
    return CR.clamp(t, activation)


def exp32(a):
    """The stated exp of lce_hip_softmax_f32, element-wise on a float32 array of arguments <= 0."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        live = a >= np.float32(-104)                         # false for a < -104, -inf and NaN
        x = np.where(live, np.minimum(a, np.float32(0)), np.float32(0)).astype(np.float32)
        n = np.rint(x * LOG2E).astype(np.float32)            # to nearest even
        r = CR.fma32(n, -LN2_HI, x)
        r = CR.fma32(n, -LN2_LO, r)
        p = np.full(x.shape, EXP_LEAD, np.float32)
        for c in EXP_COEFFS:
            p = CR.fma32(p, r, c)
        ni = n.astype(np.int32)
        low = ni < -125
        bits = np.ascontiguousarray(p).view(np.uint32) + ((ni + np.where(low, 64, 0)).astype(np.int32) << 23).astype(np.uint32)
        e = (bits.view(np.float32) * np.where(low, TWO_M64, np.float32(1))).astype(np.float32)
        return np.where(live, e, np.float32(0)).astype(np.float32)


def wave_sum(e):
    """e: float32 [rows, cols] -> [rows]: partial sum l adds e[l], e[l + 64], ... in order from +0.0f, then the butterfly
    s[l] = s[l] + s[l ^ d] for d = 32 .. 1."""
    e = np.asarray(e, np.float32)
    s = np.zeros((e.shape[0], 64), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(0, e.shape[1], 64):
            part = e[:, j:j + 64]
            s[:, :part.shape[1]] = s[:, :part.shape[1]] + part
        lanes = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, lanes ^ d]).astype(np.float32)
    return s[:, 0]


def softmax(x, beta=1.0):
    """x: float32 [..., cols] -> the same shape."""
    x = np.asarray(x, np.float32)
    rows = x.reshape(-1, x.shape[-1])
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        m = rows.max(axis=1, keepdims=True)
        a = ((rows - m).astype(np.float32) * np.float32(beta)).astype(np.float32)
        e = exp32(a)
        return (e / wave_sum(e)[:, None]).astype(np.float32).reshape(x.shape)
