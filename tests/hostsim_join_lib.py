"""Loader of tests/hostsim_join (the real kernel bodies of csrc/lce_kernels_join.h on the CPU) and the one call the suite makes
of it: a launch of the window join on exact-size buffers between guard bytes.  No tests here."""
import ctypes as C
import os

import numpy as np

import hostsim_lib

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_join")
MARK = 0x5A
_lib = None


def lib():
    """tests/hostsim_join/liblce_hostsim_join.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        l = hostsim_lib.load(DIR, "liblce_hostsim_join.so")
        l.lce_hostsim_join.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        _lib = l
    return _lib


def Placed(shape, dtype, offset, data=None):
    """hostsim_lib.Placed with every guard byte MARK."""
    return hostsim_lib.Placed(shape, dtype, offset, np.frombuffer(bytes([MARK]) * np.dtype(dtype).itemsize, dtype)[0], data)


def sim(windows, zero_point=0, value=True, bits=True, cap=2048, offset=0):
    """One simulated launch of lce_hip_join_windows on `windows` [(array [rows, pitch], begin, count, addend or None)].  Returns
    (out or None, bits or None, took the 16-byte path).  Every source, addend and output is an exact-size buffer `offset` bytes
    behind a 16-byte boundary; an array that appears in several windows is placed once; the guards around the outputs are
    checked."""
    n = len(windows)
    dtype = windows[0][0].dtype
    kind = {np.dtype(np.float32): 0, np.dtype(np.int8): 1}[dtype]
    rows = windows[0][0].shape[0]
    placed = {}

    def once(a):
        if id(a) not in placed:
            placed[id(a)] = Placed(a.shape, a.dtype, offset, a)
        return placed[id(a)].view.ctypes.data

    src, add = (C.c_void_p * n)(), (C.c_void_p * n)()
    pitch, begin, count = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    for k, (t, b, c, a) in enumerate(windows):
        src[k], pitch[k], begin[k], count[k] = once(t), t.shape[1], b, c
        add[k] = None if a is None else once(a)
    total = sum(w[2] for w in windows)
    out = Placed((rows, total), dtype, offset) if value else None
    ob = Placed((rows, (total + 31) // 32), np.int32, offset - offset % 4) if bits else None
    vec = lib().lce_hostsim_join(kind, n, src, pitch, begin, count, add, rows, zero_point, None if out is None else out.view.ctypes.data,
                                 None if ob is None else ob.view.ctypes.data, cap)
    for p in (out, ob):
        assert p is None or p.intact(), "a write outside an output buffer"
    return None if out is None else out.view.copy(), None if ob is None else ob.view.copy(), bool(vec)
