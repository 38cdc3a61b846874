"""The window sets the window join (lce_hip_join_windows) is tested on, their operands and the NumPy reference.  Shared by
tests/test_join_hostsim.py and tests/test_gpu_join_windows.py.  No tests here."""
import numpy as np

import oracle_lib as O
from test_gpu_concat import patterns

# (pitches of the source tensors, [(source, begin, count, has an addend)]).  Channel counts are elements.
VEC_F32 = {                                  # every begin / count / pitch a multiple of 4 floats; with bits, the sum one of 32
    "192:0+128,128+64a": ((192,), [(0, 0, 128, False), (0, 128, 64, True)]),      # the improvement block at C = 192
    "320:0+256,256+64a": ((320,), [(0, 0, 256, False), (0, 256, 64, True)]),
    "128:64+64": ((128,), [(0, 64, 64, False)]),                                  # a channel slice alone
    "160:32+96": ((160,), [(0, 32, 96, False)]),
    "8x32of3": ((64, 96, 128), [(0, 0, 32, False), (1, 16, 32, True), (0, 16, 32, False), (2, 96, 32, False), (1, 32, 32, False),
                                (0, 32, 32, True), (2, 0, 32, False), (0, 8, 32, False)]),   # one tensor four times, overlapping
}
ROW_F32 = {
    "70:3+31": ((70,), [(0, 3, 31, False)]),
    "70:0+1,69+1": ((70,), [(0, 0, 1, False), (0, 69, 1, False)]),
    "64:1+32a": ((64,), [(0, 1, 32, True)]),                                       # aligned but for a begin of 1
    "68:0+36,36+32a": ((68,), [(0, 0, 36, False), (0, 36, 32, True)]),            # 16-byte chunks, but the bits straddle rows
}
VEC_I8 = {
    "192:0+128,128+64": ((192,), [(0, 0, 128, False), (0, 128, 64, False)]),
    "48:16+32": ((48,), [(0, 16, 32, False)]),
    "64,32:32+32,0+16,16+16": ((64, 32), [(0, 32, 32, False), (1, 0, 16, False), (1, 16, 16, False)]),
}
ROW_I8 = {
    "48:16+17": ((48,), [(0, 16, 17, False)]),
    "70:0+1,69+1": ((70,), [(0, 0, 1, False), (0, 69, 1, False)]),
}


def dense(*channels):
    """Whole tensors of `channels` joined: lce_hip_concat's launch, begin 0 and count = pitch."""
    return tuple(channels), [(k, 0, c, False) for k, c in enumerate(channels)]


def twice(c):
    """One tensor of `c` channels joined to itself."""
    return (c,), [(0, 0, c, False), (0, 0, c, False)]


# the dense joins tests/test_gpu_concat.py runs on the GPU, by the path they take
DENSE_VEC_F32 = {"dense:64x64": dense(64, 64), "dense:256x64x64": dense(256, 64, 64), "dense:8x32": dense(*(32,) * 8), "dense:64twice": twice(64)}
DENSE_ROW_F32 = {"dense:1x31": dense(1, 31), "dense:33x64x7": dense(33, 64, 7), "dense:63x1": dense(63, 1), "dense:7twice": twice(7)}
DENSE_VEC_I8 = {"dense:16x16": dense(16, 16), "dense:128x64": dense(128, 64), "dense:64twice": twice(64)}
DENSE_ROW_I8 = {"dense:48x17": dense(48, 17), "dense:5x3": dense(5, 3), "dense:7twice": twice(7)}
# bitpacked int32 words: 4-byte elements through the float kind, no bit output
DENSE_WORDS = {"words:4x8x4": (dense(4, 8, 4), True), "words:1x3": (dense(1, 3), False)}      # (case, takes the 16-byte path)


def build(kind, case, rows, seed):
    """The windows of `case` on random operands: [(source [rows, pitch], begin, count, addend [rows, count] or None)].  Float
    operands are random 32-bit patterns with the special values planted (tests/test_gpu_concat.py)."""
    pitches, wins = case
    g = np.random.default_rng(seed)
    if kind == "f32":
        srcs = [patterns(rows, p, seed + 31 * k).view(np.float32) for k, p in enumerate(pitches)]
    else:
        srcs = [g.integers(-128, 128, (rows, p), dtype=np.int64).astype(np.int8) for p in pitches]
    out = []
    for k, (s, b, c, add) in enumerate(wins):
        a = patterns(rows, c, seed + 1000 + 17 * k).view(np.float32) if add and kind == "f32" else None
        out.append((srcs[s], b, c, a))
    return out


def reference(windows):
    """(the joined tensor, a mask of the positions whose value is a float32 SUM that came out a NaN).  Copies keep their bits."""
    parts, nan = [], []
    for t, b, c, a in windows:
        w = np.ascontiguousarray(t[:, b:b + c])
        if a is None:
            parts.append(w)
            nan.append(np.zeros(w.shape, bool))
        else:
            with np.errstate(all="ignore"):
                s = (w + a).astype(np.float32)
            parts.append(s)
            nan.append(np.isnan(s))
    return np.concatenate(parts, axis=-1), np.concatenate(nan, axis=-1)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_joined(got, want, nan, what=""):
    """Equal bits everywhere but where the reference's sum is a NaN: there a NaN (its payload is unspecified)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if nan.any():
        assert np.isnan(got[nan]).all(), what
    assert np.array_equal(raw(got)[~nan], raw(want)[~nan]), what


def want_bits(want, zero_point=0):
    return O.bitpack(want, zero_point)          # (a NaN is not below zero, whatever its payload)
