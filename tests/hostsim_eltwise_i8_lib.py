"""Loader of tests/hostsim_eltwise_i8 (the real kernel bodies of csrc/lce_kernels_eltwise_i8_chain.h on the CPU) and the one call the
suite makes of it: a launch of a chain, as lce_hip_elementwise_i8_path describes it, on exact-size buffers between guard bytes.  No
tests here."""
import ctypes as C
import importlib
import os

import numpy as np

import hostsim_lib

amd = importlib.import_module("compute-engine_amd")
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_eltwise_i8")
_lib = None


def lib():
    """tests/hostsim_eltwise_i8/liblce_hostsim_eltwise_i8.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        l = hostsim_lib.load(DIR, "liblce_hostsim_eltwise_i8.so")
        l.lce_hostsim_eltwise_i8.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p] + [C.c_int32] * 5
        _lib = l
    return _lib


def Placed(nbytes, offset, mark, data=None):
    """`nbytes` guarded bytes `offset` bytes behind a 16-byte boundary (hostsim_lib.Placed)."""
    return hostsim_lib.Placed((nbytes,), np.uint8, offset, mark, None if data is None else np.ascontiguousarray(data).view(np.uint8))


def sim_chain(x, q_in, steps, addend=None, head=None, want_out=True, want_bits=True, path=None, cap=None, offset=0, bits_offset=0,
              in_place=None):
    """One simulated launch of the chain on x [rows, C] (int8).  The table is the product's own (elementwise_i8_prepare); path,
    layout, grid, block size and LDS bytes are what lce_hip_elementwise_i8_path reports for the buffers' addresses (`path`: None for
    the entry's rule or an EW_I8_PATH_* to force; `cap`: at most this many blocks, so that waves stride).  `offset`: bytes behind a
    16-byte boundary of every int8 buffer; `bits_offset`: words behind one of the bit output.  `in_place`: None, "in" or "addend".
    Returns (out or None, bits or None, launch dict)."""
    x = np.ascontiguousarray(x, np.int8)
    rows, channels = x.shape
    table = amd.elementwise_i8_prepare(channels, q_in, steps, head=head)
    desc, keep = amd._ew_i8_desc("sim_chain", channels, q_in, steps, head)
    xin = Placed(x.size, offset, 0x11, x)
    add = None if addend is None else Placed(x.size, offset, 0x22, np.ascontiguousarray(addend, np.int8))
    tab = Placed(table.size, 0, 0x33, table)
    out = {None: Placed(x.size, offset, 0x44) if want_out else None, "in": xin, "addend": add}[in_place]
    wpr = (channels + 31) // 32
    bits = Placed(rows * wpr * 4, 4 * bits_offset, 0x5A) if want_bits else None
    L = amd.EwI8Launch()
    amd.check(amd.lib().lce_hip_elementwise_i8_path(C.byref(desc), rows, xin.ptr, None if add is None else add.ptr, tab.ptr,
                                                    None if out is None else out.ptr, None if bits is None else bits.ptr,
                                                    -1 if path is None else path, C.byref(L)))
    launch = {n: int(getattr(L, n)) for n, _ in amd.EwI8Launch._fields_}
    hp = None
    if head is not None:
        p = amd.add_int8_params(q_in, head[0], head[1], head[2] if len(head) == 3 else 0)
        hp = (C.c_int32 * 11)(q_in[1], p["in1_multiplier"], -p["in1_shift"], head[0][1], p["in2_multiplier"], -p["in2_shift"],
                              head[1][1], p["out_multiplier"], -p["out_shift"], p["act_min"], p["act_max"])
    last = steps[-1]
    zo_last = (last[3] if last[0] in ("add", "prelu") else last[1])[1]
    blocks = launch["blocks"] if cap is None else min(cap, launch["blocks"])
    launch["blocks_run"] = blocks
    bad = lib().lce_hostsim_eltwise_i8(hp, rows, channels, xin.ptr, None if add is None else add.ptr, tab.ptr, zo_last,
                                       None if out is None else out.ptr, None if bits is None else bits.ptr, launch["path"],
                                       launch["flat"], blocks, 64 * launch["waves_per_block"], launch["lds_bytes"])
    assert not bad, "a write outside the block's LDS"
    for p in (xin, add, tab, out, bits):
        assert p is None or p.intact(), "a write outside a buffer"
    if in_place != "in":
        assert np.array_equal(xin.view.view(np.int8).reshape(x.shape), x), "the input was written"
    assert np.array_equal(tab.view, table.reshape(-1)), "the table was written"
    return (None if out is None else out.view.view(np.int8).reshape(x.shape).copy(),
            None if bits is None else bits.view.view(np.int32).reshape(rows, wpr).copy(), launch)
