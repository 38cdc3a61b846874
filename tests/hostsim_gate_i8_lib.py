"""Loader of tests/hostsim_gate_i8 (the real kernel bodies of csrc/lce_kernels_mul_i8.h on the CPU) and the one call the suite makes
of it: a launch of the int8 gate MUL, as lce_hip_mul_int8_path describes it, on exact-size buffers between guard bytes.  No tests
here."""
import ctypes as C
import importlib
import os

import numpy as np

import hostsim_lib

from hostsim_eltwise_i8_lib import Placed

amd = importlib.import_module("compute-engine_amd")
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_gate_i8")
_lib = None


def lib():
    """tests/hostsim_gate_i8/liblce_hostsim_gate_i8.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        l = hostsim_lib.load(DIR, "liblce_hostsim_gate_i8.so")
        l.lce_hostsim_gate_i8.restype = C.c_int
        l.lce_hostsim_gate_i8.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32] + \
                                         [C.c_void_p] * 5 + [C.c_int32] * 4
        _lib = l
    return _lib


def sim_mul(x, operand, q_x, q_operand, q_out, act=0, rows_per_image=0, addend=None, add=None, want_out=True, want_bits=True,
            cap=None, offset=0, bits_offset=0, in_place=None, literal_add=False):
    """One simulated launch of the MUL on x [rows, C] (int8).  ``operand``: [rows, C], or with ``rows_per_image`` the gate
    [rows / rows_per_image, C].  ``addend`` with ``add = (q_addend, q_sum[, act])``: the residual ADD.  Layout and grid are what
    lce_hip_mul_int8_path reports for the buffers' addresses (`cap`: at most this many blocks, so that waves stride).  `offset`:
    bytes behind a 16-byte boundary of every int8 tensor of x's shape; `bits_offset`: words behind one of the bit output.
    `in_place`: None, "x" or "addend".  `literal_add`: the ADD's LITERAL kernel (right for every parameter set, on the same
    parameters and input order) instead of the variant the entry chose.  Returns (out or None, bits or None, launch dict)."""
    x = np.ascontiguousarray(x, np.int8)
    operand = np.ascontiguousarray(operand, np.int8)
    rows, channels = x.shape
    per_image = bool(rows_per_image)
    d = amd._mul_int8_desc("sim_mul", q_x, q_operand, q_out, act, per_image, add)
    p = amd.mul_int8_params(q_x, q_operand, q_out, act, add)
    xin = Placed(x.size, offset, 0x11, x)
    gate = Placed(operand.size, 0 if per_image else offset, 0x66, operand)
    ad = None if addend is None else Placed(x.size, offset, 0x22, np.ascontiguousarray(addend, np.int8))
    out = {None: Placed(x.size, offset, 0x44) if want_out else None, "x": xin, "addend": ad}[in_place]
    wpr = (channels + 31) // 32
    bits = Placed(rows * wpr * 4, 4 * bits_offset, 0x5A) if want_bits else None
    ptr = lambda b: None if b is None else b.ptr
    L = amd.MulInt8Launch()
    amd.check(amd.lib().lce_hip_mul_int8_path(C.byref(d), rows, channels, rows_per_image, xin.ptr, gate.ptr, ptr(ad), ptr(out),
                                              ptr(bits), C.byref(L)))
    launch = {n: int(getattr(L, n)) for n, t in amd.MulInt8Launch._fields_ if t is C.c_int32}
    mp = (C.c_int32 * 7)(q_x[1], q_operand[1], q_out[1], p["multiplier"], p["shift"], p["act_min"], p["act_max"])
    # the ADD runs the variant the entry chose, on the entry's own kernel parameters and input order
    ap = None if add is None else L.add_args
    blocks = launch["blocks"] if cap is None else min(cap, launch["blocks"])
    launch["blocks_run"] = blocks
    rc = lib().lce_hostsim_gate_i8(mp, ap, 0 if literal_add and add is not None else launch["add_variant"], launch["product_first"], rows, channels, rows_per_image, int(per_image),
                                   xin.ptr, gate.ptr, ptr(ad), ptr(out), ptr(bits), launch["flat"], blocks,
                                   64 * launch["waves_per_block"], launch["mul_variant"])
    assert rc == 0, "the simulation has no such variant"
    for b in (xin, gate, ad, out, bits):
        assert b is None or b.intact(), "a write outside a buffer"
    if in_place != "x":
        assert np.array_equal(xin.view.view(np.int8).reshape(x.shape), x), "the input was written"
    if in_place != "addend" and ad is not None:
        assert np.array_equal(ad.view.view(np.int8).reshape(x.shape), addend), "the addend was written"
    assert np.array_equal(gate.view.view(np.int8).reshape(operand.shape), operand), "the operand was written"
    return (None if out is None else out.view.view(np.int8).reshape(x.shape).copy(),
            None if bits is None else bits.view.view(np.int32).reshape(rows, wpr).copy(), launch)
