"""Loader of tests/hostsim_head_i8 (the real kernel bodies of csrc/lce_kernels_head_i8.h on the CPU) and the calls the suites make
of it: one launch of each kernel on exact-size buffers, and the value functions of the epilogues element by element.  No tests
here."""
import ctypes as C
import os

import numpy as np

import hostsim_lib

import conv2d_i8_ref as CR
import head_i8_ref as H
from hostsim_lib import placed

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_head_i8")
OUT_MARK = np.int8(0x5A)
_lib = None


def lib():
    """tests/hostsim_head_i8/liblce_hostsim_head_i8.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        l = hostsim_lib.load(DIR, "liblce_hostsim_head_i8.so")
        l.lce_hostsim_fully_connected_i8.argtypes = [C.c_void_p] * 5 + [C.c_int32]
        l.lce_hostsim_mean_i8.argtypes, l.lce_hostsim_mean_i8.restype = [C.c_void_p] * 3 + [C.c_int32], None
        l.lce_hostsim_softmax_i8.argtypes = [C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int32]
        l.lce_hostsim_softmax_i8.restype = None
        l.lce_hostsim_quant_i8.argtypes = [C.c_int32, C.c_int64, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        l.lce_hostsim_quant_i8.restype = None
        l.lce_hostsim_fc_i8_value.argtypes = [C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]
        l.lce_hostsim_mean_i8_value.argtypes = [C.c_int64, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]
        l.lce_hostsim_softmax_i8_exp.argtypes = [C.c_int64, C.c_void_p, C.c_float, C.c_void_p]
        l.lce_hostsim_softmax_i8_value.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        l.lce_hostsim_quantize_value.argtypes = [C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_void_p]
        l.lce_hostsim_dequantize_value.argtypes = [C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_void_p]
        for f in ("fc_i8_value", "mean_i8_value", "softmax_i8_exp", "softmax_i8_value", "quantize_value", "dequantize_value"):
            getattr(l, "lce_hostsim_" + f).restype = None
        _lib = l
    return _lib


def sim_fc(x, w, bias, sw, q_in, q_out, act=H.NONE, offset=0, cap=3):
    """(out, took the 16-byte path) of one launch of fully_connected_i8 on EXACT-size operands placed `offset` bytes behind a
    16-byte boundary (an access past an end lands in another allocation's bytes or faults under a checker)."""
    x, w = placed(x, offset), placed(w, offset)
    table = np.ascontiguousarray(H.fc_table(w, bias, sw, q_in[0], q_in[1], q_out[0]))
    lo, hi = CR.activation_range(act, q_out[0], q_out[1])
    d = (C.c_int32 * 6)(x.shape[0], x.shape[1], w.shape[0], q_out[1], lo, hi)
    out = np.full((x.shape[0], w.shape[0]), OUT_MARK, np.int8)
    vec = lib().lce_hostsim_fully_connected_i8(d, x.ctypes.data, w.ctypes.data, table.ctypes.data, out.ctypes.data, cap)
    return out, bool(vec)


def sim_mean(x, q_in, q_out, cap=3):
    x = np.ascontiguousarray(x)
    m, e = H.mean_multiplier(q_in[0], q_out[0])
    d = (C.c_int32 * 7)(x.shape[0], x.shape[1] * x.shape[2], x.shape[3], q_in[1], q_out[1], m, e)
    out = np.full((x.shape[0], x.shape[3]), OUT_MARK, np.int8)
    lib().lce_hostsim_mean_i8(d, x.ctypes.data, out.ctypes.data, cap)
    return out


def sim_softmax(q, input_scale, beta=1.0, cap=3):
    q = np.ascontiguousarray(q)
    out = np.full(q.shape, OUT_MARK, np.int8)
    lib().lce_hostsim_softmax_i8(q.size // q.shape[-1], q.shape[-1], float(input_scale), float(beta), q.ctypes.data, out.ctypes.data, cap)
    return out


def sim_quantize(x, scale, zp, cap=3):
    x = np.ascontiguousarray(x, np.float32)
    out = np.full(x.shape, OUT_MARK, np.int8)
    lib().lce_hostsim_quant_i8(1, x.size, float(scale), int(zp), x.ctypes.data, out.ctypes.data, cap)
    return out


def sim_dequantize(q, scale, zp, cap=3):
    q = np.ascontiguousarray(q, np.int8)
    out = np.full(q.shape, np.float32(-7.5), np.float32)
    lib().lce_hostsim_quant_i8(0, q.size, float(scale), int(zp), q.ctypes.data, out.ctypes.data, cap)
    return out


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def fc_value(acc, cst, m, e, zo, lo, hi):
    acc, cst, m, e = (_i32(a) for a in (acc, cst, m, e))
    out = np.empty(acc.shape, np.int32)
    lib().lce_hostsim_fc_i8_value(acc.size, acc.ctypes.data, cst.ctypes.data, m.ctypes.data, e.ctypes.data, zo, lo, hi, out.ctypes.data)
    return out


def mean_value(acc, m, e, n, zo):
    acc = _i32(acc)
    out = np.empty(acc.shape, np.int32)
    lib().lce_hostsim_mean_i8_value(acc.size, acc.ctypes.data, m, e, n, zo, out.ctypes.data)
    return out


def softmax_exp(d, sb):
    d = _i32(d)
    out = np.empty(d.shape, np.float32)
    lib().lce_hostsim_softmax_i8_exp(d.size, d.ctypes.data, float(sb), out.ctypes.data)
    return out


def softmax_value(e, s):
    e, s = np.ascontiguousarray(e, np.float32), np.ascontiguousarray(s, np.float32)
    out = np.empty(e.shape, np.int32)
    lib().lce_hostsim_softmax_i8_value(e.size, e.ctypes.data, s.ctypes.data, out.ctypes.data)
    return out


def quantize_value(x, scale, zp):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.int32)
    lib().lce_hostsim_quantize_value(x.size, x.ctypes.data, float(scale), int(zp), out.ctypes.data)
    return out


def dequantize_value(q, scale, zp):
    q = _i32(q)
    out = np.empty(q.shape, np.float32)
    lib().lce_hostsim_dequantize_value(q.size, q.ctypes.data, float(scale), int(zp), out.ctypes.data)
    return out
