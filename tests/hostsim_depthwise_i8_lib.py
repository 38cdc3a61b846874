"""Loader of tests/hostsim_depthwise_i8 (the real kernel bodies of csrc/lce_kernels_depthwise_i8.h on the CPU) and the one call the
suites make of it: one launch, on the path the entry's rule picks or forced onto the row path.  No tests here."""
import ctypes as C
import os
import subprocess

import numpy as np

import depthwise_i8_ref as R
from depthwise_i8_cases import BITS_MARK, OUT_MARK
from hostsim_conv2d_i8_lib import placed

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_depthwise_i8")
_lib = None


def lib():
    """tests/hostsim_depthwise_i8/liblce_hostsim_depthwise_i8.so, brought up to date with the kernel headers first (as
    tests/hostsim_lib.py does: among pytest-xdist workers one builds and the others wait)."""
    global _lib
    if _lib is None:
        import fcntl
        with open(os.path.join(DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.run(["make", "-C", DIR], check=True, capture_output=True)
        _lib = C.CDLL(os.path.join(DIR, "liblce_hostsim_depthwise_i8.so"))
        _lib.lce_hostsim_depthwise_i8.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int32]
    return _lib


def sim(x, w, bias, sw, q_in, q_out, stride, padding, m, act, want_out=True, want_bits=True, offset=0, path=None, cap=3):
    """(out, bits, took the 16-byte path); an output that was not asked for keeps its marks.  `offset`: input, filter and output
    lie that many bytes behind a 16-byte boundary.  `path`: None for the entry's rule, 0 for the row path."""
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    w = np.asarray(w).reshape((1,) + np.asarray(w).shape[-3:])
    x, w = placed(x, offset), placed(w, offset)
    (oh, ph), (ow, pw) = R.out_and_pad(x.shape[1], w.shape[1], st[0], padding), R.out_and_pad(x.shape[2], w.shape[2], st[1], padding)
    table = placed(np.ascontiguousarray(R.table(w, bias, sw, q_in[0], q_out[0])), 0)
    lo, hi = R.activation_range(act, q_out[0], q_out[1])
    d = (C.c_int32 * 17)(*x.shape, m, w.shape[1], w.shape[2], st[0], st[1], oh, ow, ph, pw, q_in[1], q_out[1], lo, hi)
    cout = w.shape[3]
    out = placed(np.full((x.shape[0], oh, ow, cout), OUT_MARK, np.int8), offset)
    bits = np.full((x.shape[0], oh, ow, (cout + 31) // 32), BITS_MARK, np.int32)
    vec = lib().lce_hostsim_depthwise_i8(d, x.ctypes.data, w.ctypes.data, table.ctypes.data, out.ctypes.data if want_out else None,
                                         bits.ctypes.data if want_bits else None, -1 if path is None else int(path), cap)
    return out, bits, bool(vec)
