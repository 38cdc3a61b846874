"""NumPy float32 restatements of lce_hip_elementwise_ex as include/lce_hip.h states it: the ADD / MUL steps of
lce_hip_elementwise (one rounding per op, then the activation's clamp as compares and selects), the per-image operand, CLAMP,
PRELU and LOGISTIC -- the last on tests/head_ref.py's exp32, the E(a) of the softmax.  No tests here."""
import numpy as np

import conv1x1_ref as CR
import head_ref as HR

NONE, RELU, RELU_N1_TO_1, RELU6 = range(4)
ADD, MUL, CLAMP, PRELU, LOGISTIC = "add", "mul", "clamp", "prelu", "logistic"
ONE = np.float32(1)


def clamp(v, activation):
    """The activation's clamp: v < lo ? lo : v, then hi < v ? hi : v.  RELU(-0.0) = -0.0 and a NaN passes."""
    return CR.clamp(np.asarray(v, np.float32), activation)


def prelu(v, alpha):
    """v >= 0 ? v : fl(v * alpha); alpha a float32 scalar or [C] (broadcast over the last axis).  -0.0 stays (-0.0 >= 0); a NaN
    takes the multiply and stays NaN."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.where(v >= np.float32(0), v, (v * np.asarray(alpha, np.float32)).astype(np.float32)).astype(np.float32)


def logistic(x):
    """x >= 0: e = E(-x), y = 1 / fl(1 + e);  x < 0: e = E(x), y = e / fl(1 + e);  a NaN passes unchanged (its bytes too)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        pos = x >= np.float32(0)
        e = HR.exp32(np.where(pos, -x, x).astype(np.float32))
        d = (ONE + e).astype(np.float32)
        y = (np.where(pos, ONE, e).astype(np.float32) / d).astype(np.float32)
    out = y.copy()
    nan = np.isnan(x)
    out[nan] = x[nan]
    return out


def chain(x, steps):
    """x: float32 [batch, ..., C]; steps: (op, operand, activation) as compute-engine_amd.elementwise_ex takes them -- an ADD / MUL
    operand is a float, a [C] array, an array of x's shape or a per-image [batch, 1, ..., 1, C] array (NumPy's broadcast IS the
    stated indexing for each of them)."""
    v = np.asarray(x, np.float32)
    for op, operand, act in steps:
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            if op in (ADD, MUL):
                o = np.asarray(operand, np.float32)
                v = clamp((v * o if op == MUL else v + o).astype(np.float32), act)
            elif op == CLAMP:
                v = clamp(v, act)
            elif op == PRELU:
                v = prelu(v, operand)
            elif op == LOGISTIC:
                v = logistic(v)
            else:
                raise ValueError(op)
    return v
