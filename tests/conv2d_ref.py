"""NumPy reference of lce_hip_conv2d_f32 (include/lce_hip.h): TFLite's float reference_ops::Conv (groups 1, dilation 1) as a
contracting build computes it.  Per output element, over its in-bounds taps in raster order (filter row, then filter column;
taps in the padding are skipped, the filter index is the unclipped one) and within a tap over c = 0 .. Cin-1 in order:
t = +0.0f; t = fmaf(x[iy][ix][c], w[o][fy][fx][c], t); then t + bias[o] (skipped without a bias); then the clamp to the
activation range.  The fmaf is tests/conv1x1_ref.py's, the taps are tests/depthwise_ref.py's, extents and padding are the
pools' (tests/pool_ref.py)."""
import numpy as np

from conv1x1_ref import FLOAT_RANGE, NONE, RELU, RELU6, RELU_N1_TO_1, clamp, fma32  # noqa: F401  (re-exported)
from depthwise_ref import finish, taps  # noqa: F401
from pool_ref import SAME, VALID, out_and_pad  # noqa: F401


def chain(x, w, stride=(1, 1), padding=SAME):
    """x: float32 [B, H, W, Cin]; w: float32 [Cout, fh, fw, Cin].  The fmaf chain alone, before bias and clamp: float32
    [B, OH, OW, Cout]."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    assert w.ndim == 4 and w.shape[3] == x.shape[3]
    stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
    tp, oh, ow = taps(x.shape[1:3], w.shape[1:3], stride, padding)
    assert oh > 0 and ow > 0
    t = np.zeros((x.shape[0], oh, ow, w.shape[0]), np.float32)
    for fy, fx, (oy, ox), (iy, ix) in tp:
        for c in range(x.shape[3]):
            t[:, oy, ox, :] = fma32(x[:, iy, ix, c:c + 1], w[None, None, None, :, fy, fx, c], t[:, oy, ox, :])
    return t


def conv2d(x, w, bias=None, stride=(1, 1), padding=SAME, activation=NONE):
    """lce_hip_conv2d_f32 on NumPy arrays."""
    return finish(chain(x, w, stride, padding), bias, activation)
