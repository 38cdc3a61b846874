"""Loader of tests/hostsim_eltwise (the real kernel bodies of csrc/lce_kernels_eltwise.h on the CPU) and the one call the suite
makes of it: a launch of the chain on exact-size buffers between guard words.  No tests here."""
import ctypes as C
import importlib
import os

import numpy as np

import hostsim_lib
from hostsim_lib import Placed

amd = importlib.import_module("compute-engine_amd")
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_eltwise")
OUT_MARK = np.float32(777)
BITS_MARK = np.uint32(0x5A5A5A5A)
_lib = None


def lib():
    """tests/hostsim_eltwise/liblce_hostsim_eltwise.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        l = hostsim_lib.load(DIR, "liblce_hostsim_eltwise.so")
        l.lce_hostsim_eltwise.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_int32]
        l.lce_hostsim_logistic.argtypes, l.lce_hostsim_logistic.restype = [C.c_void_p, C.c_void_p, C.c_int64], None
        _lib = l
    return _lib


def sim_logistic(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    lib().lce_hostsim_logistic(x.ctypes.data, y.ctypes.data, x.size)
    return y


def sim_chain(x, steps, want_out=True, want_bits=True, cap=2048, offset=0, ex=1, in_place=False):
    """One simulated launch of the chain `steps` (as compute-engine_amd.elementwise_ex takes them) on x [batch, ..., C].  Returns
    (out or None, bits or None, took the flat path).  Every operand and output is an exact-size buffer `offset` floats behind a
    16-byte boundary; the guards around the outputs are checked."""
    x = np.asarray(x, np.float32)
    kinds = amd._ew_ex_check(x, steps, None if want_out else False, True if want_bits else None)
    channels = x.shape[-1]
    rows = x.size // channels
    nan = np.float32(np.nan)
    xin = Placed(x.shape, np.float32, 4 * offset, nan, x)
    out = xin if in_place else Placed(x.shape, np.float32, 4 * offset, OUT_MARK) if want_out else None
    bits = Placed(x.shape[:-1] + ((channels + 31) // 32,), np.uint32, 4 * offset, BITS_MARK) if want_bits else None
    n = len(steps)
    keep = []
    values = (C.c_void_p * n)()
    ops, operands, acts = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    scalars = (C.c_float * n)()
    for k, ((op, operand, act), kind) in enumerate(zip(steps, kinds)):
        ops[k], operands[k], acts[k] = amd._EW_EX_OPS[op], kind, act
        if kind == amd.EW_SCALAR:
            scalars[k] = 0.0 if operand is None else float(operand)
        else:
            p = Placed(np.shape(operand), np.float32, 4 * offset, nan, operand)
            keep.append(p)
            values[k] = p.view.ctypes.data
    flat = lib().lce_hostsim_eltwise(rows, channels, rows // x.shape[0], n, ops, operands, values, scalars, acts, xin.view.ctypes.data,
                                     out.view.ctypes.data if out is not None else None, bits.view.ctypes.data if bits is not None else None,
                                     cap, ex)
    for p in (out, bits):
        assert p is None or p.intact(), "a write outside an output buffer"
    return (None if out is None else out.view.copy(), None if bits is None else bits.view.copy().view(np.int32), bool(flat))
