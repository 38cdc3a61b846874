"""Loader of tests/hostsim_binary_dense (the real kernel body of csrc/lce_kernels_bfc.h on the CPU) and the one call the suite
makes of it: a launch of binary_fully_connected on exact-size buffers.  No tests here."""
import ctypes as C
import os

import numpy as np

import hostsim_lib
from hostsim_lib import placed

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_binary_dense")
OUT_MARK = np.float32(-7.5)
BITS_MARK = np.int32(0x5A5A5A5A)
_lib = None


def lib():
    """tests/hostsim_binary_dense/liblce_hostsim_binary_dense.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        l = hostsim_lib.load(DIR, "liblce_hostsim_binary_dense.so")
        l.lce_hostsim_binary_fully_connected.argtypes = [C.c_void_p] * 7 + [C.c_int32]
        _lib = l
    return _lib


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
