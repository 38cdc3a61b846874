"""Loader of tests/hostsim_binary_dense (the real kernel body of csrc/lce_kernels_bfc.h on the CPU) and the one call the suite
makes of it: a launch of binary_fully_connected on exact-size buffers.  No tests here."""
import ctypes as C
import os
import subprocess

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_binary_dense")
OUT_MARK = np.float32(-7.5)
BITS_MARK = np.int32(0x5A5A5A5A)
_lib = None


def lib():
    """tests/hostsim_binary_dense/liblce_hostsim_binary_dense.so, brought up to date with the kernel headers first (as
    tests/hostsim_lib.py does: among pytest-xdist workers one builds and the others wait)."""
    global _lib
    if _lib is None:
        import fcntl
        with open(os.path.join(DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.run(["make", "-C", DIR], check=True, capture_output=True)
        l = C.CDLL(os.path.join(DIR, "liblce_hostsim_binary_dense.so"))
        l.lce_hostsim_binary_fully_connected.argtypes = [C.c_void_p] * 7 + [C.c_int32]
        _lib = l
    return _lib


def placed(a, offset):
    """A copy of `a` that starts `offset` bytes behind a 16-byte boundary, exact in size."""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    view = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    view[...] = a
    return view


def sim(in_bits, weight_bits, scale, bias, k, activation=0, value=True, bits=True, cap=1 << 20, offset=0):
    """(v or None, bits or None, took the 16-byte path) of one launch on EXACT-size operands; the bit operands start `offset` bytes
    behind a 16-byte boundary."""
    a, w = placed(np.asarray(in_bits, np.int32), offset), placed(np.asarray(weight_bits, np.int32), offset)
    s = np.ascontiguousarray(scale, np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    m, n = a.shape[0], w.shape[0]
    assert a.shape[1] == w.shape[1] == (k + 31) // 32 and s.shape == (n,)
    d = (C.c_int32 * 4)(m, k, n, activation)
    out = np.full((m, n), OUT_MARK, np.float32) if value else None
    ob = np.full((m, (n + 31) // 32), BITS_MARK, np.int32) if bits else None
    vec = lib().lce_hostsim_binary_fully_connected(d, a.ctypes.data, w.ctypes.data, s.ctypes.data, None if b is None else b.ctypes.data,
                                                   None if out is None else out.ctypes.data, None if ob is None else ob.ctypes.data, cap)
    return out, ob, bool(vec)
