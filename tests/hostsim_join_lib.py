"""Loader of tests/hostsim_join (the real kernel bodies of csrc/lce_kernels_join.h on the CPU) and the one call the suite makes
of it: a launch of the window join on exact-size buffers between guard bytes.  No tests here."""
import ctypes as C
import os
import subprocess

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_join")
GUARD = 64                                  # guard bytes on either side of every buffer
MARK = 0x5A
_lib = None


def lib():
    """tests/hostsim_join/liblce_hostsim_join.so, brought up to date with the kernel header first (as tests/hostsim_lib.py does:
    among pytest-xdist workers one builds and the others wait)."""
    global _lib
    if _lib is None:
        import fcntl
        with open(os.path.join(DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.run(["make", "-C", DIR], check=True, capture_output=True)
        l = C.CDLL(os.path.join(DIR, "liblce_hostsim_join.so"))
        l.lce_hostsim_join.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        _lib = l
    return _lib


class Placed:
    """An exact-size array whose first byte lies `offset` bytes behind a 16-byte boundary, between GUARD bytes of MARK on either
    side: a write past an end is seen by intact()."""

    def __init__(self, shape, dtype, offset, data=None):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.buf = np.full(n + 2 * GUARD + 32, MARK, np.uint8)
        self.start = GUARD + (-(self.buf.ctypes.data + GUARD)) % 16 + offset
        self.n = n
        self.view = self.buf[self.start:self.start + n].view(dtype).reshape(shape)
        assert self.view.ctypes.data % 16 == offset
        if data is not None:
            self.view[...] = data

    def intact(self):
        return bool(np.all(self.buf[:self.start] == MARK) and np.all(self.buf[self.start + self.n:] == MARK))


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
