"""Loader of tests/hostsim_conv2d_i8 (the real kernel body of csrc/lce_kernels_conv2d_i8.h on the CPU) and the two calls the
suites make of it: one launch of the kernel, and the requantization function of its epilogue.  No tests here."""
import ctypes as C
import os

import numpy as np

import hostsim_lib
from hostsim_lib import placed

import conv2d_i8_ref as R
from conv2d_i8_cases import BITS_MARK, OUT_MARK

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_conv2d_i8")
_lib = None


def lib():
    """tests/hostsim_conv2d_i8/liblce_hostsim_conv2d_i8.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        _lib = hostsim_lib.load(DIR, "liblce_hostsim_conv2d_i8.so")
        _lib.lce_hostsim_conv2d_i8.argtypes = [C.c_void_p] * 6 + [C.c_int32]
        _lib.lce_hostsim_conv2d_i8_requantize.argtypes = [C.c_int64] + [C.c_void_p] * 4
        _lib.lce_hostsim_conv2d_i8_requantize.restype = None
    return _lib


def requantize(acc, m, e):
    """conv2d_i8_requantize, the function of the kernel's epilogue compiled for the host, element by element."""
    acc, m, e = (np.ascontiguousarray(a, np.int32) for a in (acc, m, e))
    out = np.empty(acc.shape, np.int32)
    lib().lce_hostsim_conv2d_i8_requantize(acc.size, acc.ctypes.data, m.ctypes.data, e.ctypes.data, out.ctypes.data)
    return out


def sim(x, w, bias, sw, q_in, q_out, stride, padding, act, want_out=True, want_bits=True, offset=0, cap=3):
    """(out, bits, took the 16-byte path); an output that was not asked for keeps its marks."""
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    x, w = placed(x, offset), placed(w, offset)
    oh, ow = R.out_and_pad(x.shape[1], w.shape[1], st[0], padding)[0], R.out_and_pad(x.shape[2], w.shape[2], st[1], padding)[0]
    table = np.ascontiguousarray(R.table(w, bias, sw, q_in[0], q_in[1], q_out[0]))
    lo, hi = R.activation_range(act, q_out[0], q_out[1])
    d = (C.c_int32 * 15)(*x.shape, w.shape[0], w.shape[1], w.shape[2], st[0], st[1], oh, ow, q_in[1], q_out[1], lo, hi)
    out = np.full((x.shape[0], oh, ow, w.shape[0]), OUT_MARK, np.int8)
    bits = np.full((x.shape[0], oh, ow, (w.shape[0] + 31) // 32), BITS_MARK, np.int32)
    vec = lib().lce_hostsim_conv2d_i8(d, x.ctypes.data, w.ctypes.data, table.ctypes.data, out.ctypes.data if want_out else None,
                                      bits.ctypes.data if want_bits else None, cap)
    return out, bits, bool(vec)
