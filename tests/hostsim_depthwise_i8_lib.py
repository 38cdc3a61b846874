"""Loader of tests/hostsim_depthwise_i8 (the real kernel bodies of csrc/lce_kernels_depthwise_i8.h on the CPU) and the one call the
suites make of it: one launch, on the path the entry's rule picks or forced onto the row path.  No tests here."""
import ctypes as C
import os

import numpy as np

import depthwise_i8_ref as R
import hostsim_lib
from depthwise_i8_cases import BITS_MARK, OUT_MARK
from hostsim_lib import placed

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_depthwise_i8")
_lib = None


def lib():
    """tests/hostsim_depthwise_i8/liblce_hostsim_depthwise_i8.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        _lib = hostsim_lib.load(DIR, "liblce_hostsim_depthwise_i8.so")
        _lib.lce_hostsim_depthwise_i8.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int32]
    return _lib


def sim(x, w, bias, sw, q_in, q_out, stride, padding, m, act, want_out=True, want_bits=True, offset=0, path=None, cap=3, offsets=None, seen=None):
    """(out, bits, took the 16-byte path); an output that was not asked for keeps its marks.  `offset`: input, filter and output
    lie that many bytes behind a 16-byte boundary; `offsets`: input, filter, table and output each by its own.  `path`: None for
    the entry's rule, 0 for the row path.  `seen`: a dict that receives the operands as the launch saw them."""
    ox, ow_, ot, oo = offsets or (offset, offset, 0, offset)
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    w = np.asarray(w).reshape((1,) + np.asarray(w).shape[-3:])
    x, w = placed(x, ox), placed(w, ow_)
    (oh, ph), (ow, pw) = R.out_and_pad(x.shape[1], w.shape[1], st[0], padding), R.out_and_pad(x.shape[2], w.shape[2], st[1], padding)
    table = placed(np.ascontiguousarray(R.table(w, bias, sw, q_in[0], q_out[0])), ot)
    lo, hi = R.activation_range(act, q_out[0], q_out[1])
    d = (C.c_int32 * 17)(*x.shape, m, w.shape[1], w.shape[2], st[0], st[1], oh, ow, ph, pw, q_in[1], q_out[1], lo, hi)
    cout = w.shape[3]
    out = placed(np.full((x.shape[0], oh, ow, cout), OUT_MARK, np.int8), oo)
    bits = np.full((x.shape[0], oh, ow, (cout + 31) // 32), BITS_MARK, np.int32)
    vec = lib().lce_hostsim_depthwise_i8(d, x.ctypes.data, w.ctypes.data, table.ctypes.data, out.ctypes.data if want_out else None,
                                         bits.ctypes.data if want_bits else None, -1 if path is None else int(path), cap)
    if seen is not None:
        seen.update(x=x, w=w, third=table, out=out if want_out else None, bits=bits if want_bits else None)
    assert vec >= 0, "the padding the product's fill derives is not (%d, %d)" % (ph, pw)
    return out, bits, bool(vec)
