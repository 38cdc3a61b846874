"""NumPy restatement of the binarized Dense layer as include/lce_hip.h states it (lce_hip_bfc_prepare and
lce_hip_binary_fully_connected): an int64 dot product of +-1, one float32 multiply, one float32 add, the clamp, the bit rule.  No
tests here."""
import numpy as np

NONE, RELU, RELU_N1_TO_1, RELU6 = range(4)
ACTIVATIONS = (NONE, RELU, RELU_N1_TO_1, RELU6)
FLT_MAX = np.float32(np.finfo(np.float32).max)
RANGES = {NONE: (-FLT_MAX, FLT_MAX), RELU: (np.float32(0), FLT_MAX), RELU_N1_TO_1: (np.float32(-1), np.float32(1)),
          RELU6: (np.float32(0), np.float32(6))}


def words_of(n):
    return (int(n) + 31) // 32


def pack_signs(neg):
    """neg: bool [..., C], True where the value is negative -> int32 [..., ceil(C/32)], LSB first, padding bits 0."""
    neg = np.asarray(neg, bool)
    c = neg.shape[-1]
    padded = np.zeros(neg.shape[:-1] + (words_of(c) * 32,), np.uint64)
    padded[..., :c] = neg
    w = (padded.reshape(neg.shape[:-1] + (words_of(c), 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return w.astype(np.uint32).view(np.int32)


def unpack_signs(bits, c):
    """int32 [..., ceil(c/32)] -> int64 [..., c] of +1 (bit 0) and -1 (bit 1)."""
    u = np.ascontiguousarray(bits).view(np.uint32)
    b = (u[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return 1 - 2 * b.reshape(u.shape[:-1] + (-1,))[..., :c].astype(np.int64)


def prepare(w):
    """w: float32 [N, K] -> (bits int32 [N, ceil(K/32)], scale float32 [N]), or None where lce_hip_bfc_prepare refuses: a row
    whose magnitudes differ, a zero, a NaN, an infinity, a scale outside [2^-100, 2^100], K >= 2^23."""
    w = np.asarray(w, np.float32)
    if w.shape[1] >= 1 << 23:
        return None
    with np.errstate(invalid="ignore"):
        s = np.abs(w[:, 0])
        if not np.all((s >= np.float32(2.0 ** -100)) & (s <= np.float32(2.0 ** 100))):
            return None
        if not np.all(np.abs(w) == s[:, None]):
            return None
    return pack_signs(np.signbit(w)), s.astype(np.float32)


def clamp(v, activation):
    """std::max(v, lo) = v < lo ? lo : v, then std::min: a NaN passes, -0.0 stays -0.0."""
    lo, hi = RANGES[activation]
    with np.errstate(invalid="ignore"):
        v = np.where(v < lo, lo, v).astype(np.float32)
        return np.where(hi < v, hi, v).astype(np.float32)


def dot(in_bits, weight_bits, k):
    """t [B, N] int64: the sum of a_k * w_k over k < K."""
    return unpack_signs(in_bits, k) @ unpack_signs(weight_bits, k).T


def binary_fully_connected(in_bits, weight_bits, scale, bias, k, activation=NONE):
    """in_bits int32 [B, ceil(K/32)], weight_bits int32 [N, ceil(K/32)], scale float32 [N], bias float32 [N] or None ->
    (v float32 [B, N], bits int32 [B, ceil(N/32)])."""
    t = dot(in_bits, weight_bits, k).astype(np.float32)         # exact: |t| <= K < 2^23; zero is +0.0f
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = (t * np.asarray(scale, np.float32)[None, :]).astype(np.float32)
        if bias is not None:
            v = (v + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
        v = clamp(v, activation)
        return v, pack_signs(v < np.float32(0))
