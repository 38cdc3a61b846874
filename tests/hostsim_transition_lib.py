"""Loader of tests/hostsim_transition (the real kernel bodies of csrc/lce_kernels_transition.h on the CPU) and the two calls the suite
makes of it: one fused launch, float32 or int8, on the path the entry's rule picks or forced onto the row path.  No tests here."""
import ctypes as C
import os

import numpy as np

import hostsim_lib
from hostsim_lib import placed

import depthwise_i8_ref as DI
import pool_ref as P
from transition_cases import BITS_MARK, OUT_MARK_F32, OUT_MARK_I8

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_transition")
_lib = None


def lib():
    """tests/hostsim_transition/liblce_hostsim_transition.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        _lib = hostsim_lib.load(DIR, "liblce_hostsim_transition.so")
        _lib.lce_hostsim_transition_f32.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32]
        _lib.lce_hostsim_transition_i8.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32]
    return _lib


def geometry(shape, pool, filt, stride, padding, m):
    """The 21 ints both launches take, and the output shape."""
    (qh, pph), (qw, ppw) = (P.out_and_pad(shape[1 + k], pool["filter"][k], pool["stride"][k], pool["padding"]) for k in (0, 1))
    (oh, ph), (ow, pw) = (P.out_and_pad((qh, qw)[k], filt[k], stride[k], padding) for k in (0, 1))
    d = (C.c_int32 * 21)(*shape, m, *pool["filter"], *pool["stride"], pph, ppw, qh, qw, *filt, *stride, ph, pw, oh, ow)
    return d, (shape[0], oh, ow, shape[3] * m)


def _ptr(a):
    return None if a is None else a.ctypes.data


def sim_f32(x, pool, w, bias, stride, padding, m, act, want_out=True, want_bits=True, path=None, offset=0, cap=3, place_x=None, offsets=None,
            seen=None):
    """(out, bits, took the 16-byte path); an output that was not asked for keeps its marks.  `offset`: input, filter, bias and output
    lie that many bytes (a multiple of 4) behind a 16-byte boundary; `offsets`: each of the four by its own.  `place_x`: a placement of
    the input of the caller's own.  `seen`: a dict that receives the operands as the launch saw them."""
    ox, ow_, ot, oo = offsets or (offset,) * 4
    w = np.asarray(w, np.float32).reshape((1,) + np.asarray(w).shape[-3:])
    d, shape = geometry(x.shape, pool, w.shape[1:3], stride, padding, m)
    x = placed(x, ox) if place_x is None else place_x(x)
    w, bias = placed(w, ow_), None if bias is None else placed(np.asarray(bias, np.float32), ot)
    rng = (C.c_float * 4)(*P.FLOAT_RANGE[pool.get("activation", P.NONE)], *P.FLOAT_RANGE[act])
    out = placed(np.full(shape, OUT_MARK_F32, np.float32), oo)
    bits = np.full(shape[:3] + ((shape[3] + 31) // 32,), BITS_MARK, np.int32)
    vec = lib().lce_hostsim_transition_f32(d, rng, _ptr(x), _ptr(w), _ptr(bias), _ptr(out) if want_out else None,
                                           _ptr(bits) if want_bits else None, -1 if path is None else int(path), cap)
    if seen is not None:
        seen.update(x=x, w=w, third=bias, out=out if want_out else None, bits=bits if want_bits else None)
    assert vec >= 0, "the paddings the product's fill derives are not NumPy's"
    return out, bits, bool(vec)


def sim_i8(x, pool, w, bias, sw, q_out, stride, padding, m, act, want_out=True, want_bits=True, path=None, offset=0, cap=3, offsets=None, seen=None):
    ox, ow_, ot, oo = offsets or (offset, offset, 0, offset)
    w = np.asarray(w).reshape((1,) + np.asarray(w).shape[-3:])
    d, shape = geometry(x.shape, pool, w.shape[1:3], stride, padding, m)
    x, w = placed(x, ox), placed(w, ow_)
    table = placed(np.ascontiguousarray(DI.table(w, bias, sw, pool["scale"], q_out[0])), ot)
    lo, hi = DI.activation_range(act, q_out[0], q_out[1])
    plo, phi = P.quantized_range(pool.get("activation", P.NONE), pool["scale"], pool["zero_point"])
    q = (C.c_int32 * 6)(pool["zero_point"], q_out[1], lo, hi, plo, phi)
    out = placed(np.full(shape, OUT_MARK_I8, np.int8), oo)
    bits = np.full(shape[:3] + ((shape[3] + 31) // 32,), BITS_MARK, np.int32)
    vec = lib().lce_hostsim_transition_i8(d, q, _ptr(x), _ptr(w), _ptr(table), _ptr(out) if want_out else None,
                                          _ptr(bits) if want_bits else None, -1 if path is None else int(path), cap)
    if seen is not None:
        seen.update(x=x, w=w, third=table, out=out if want_out else None, bits=bits if want_bits else None)
    assert vec >= 0, "the paddings the product's fill derives are not NumPy's"
    return out, bits, bool(vec)
