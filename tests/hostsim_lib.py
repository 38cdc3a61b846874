"""ctypes binding of tests/hostsim/liblce_hostsim.so: the REAL kernel bodies
(compute-engine_amd/csrc/lce_kernels.h) and the REAL planner (lce_plan.cpp) executed
thread by thread on the CPU.  Test infrastructure only -- it lets the CPU-only suite check
index / padding / grouping / epilogue logic before any GPU minute is spent."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_lib = None


class Desc(C.Structure):
    """lce_hip_bconv2d_desc (include/lce_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "in_height", "in_width", "channels_in", "filter_height", "filter_width",
        "channels_out", "groups", "stride_height", "stride_width", "dilation_height",
        "dilation_width", "padding", "pad_values", "activation", "dst_type", "semantics")] + [
        ("out_scale", C.c_float), ("out_zero_point", C.c_int32)]


def make_desc(spec: O.ConvSpec, dst_type: int, out_scale: float = 1.0, out_zero_point: int = 0) -> Desc:
    return Desc(spec.batch, spec.in_h, spec.in_w, spec.channels_in, spec.filter_h, spec.filter_w,
                spec.channels_out, spec.groups, spec.stride_h, spec.stride_w, spec.dilation_h,
                spec.dilation_w, spec.padding, spec.pad_values, spec.activation, dst_type,
                spec.semantics, float(out_scale), int(out_zero_point))


def load(directory: str, library: str) -> C.CDLL:
    """`library` of the host simulation in `directory`, brought up to date with the kernel headers first (among pytest-xdist
    workers one builds and the others wait).  Every tests/hostsim_*_lib.py loads its library through this."""
    import fcntl
    with open(os.path.join(directory, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", directory], check=True, capture_output=True)
    return C.CDLL(os.path.join(directory, library))


def placed(a, offset=0):
    """A copy of `a`, exact in size, whose first byte lies `offset` bytes behind a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = np.zeros(a.nbytes + 32, np.uint8)
    start = (-buf.ctypes.data) % 16 + offset
    v = buf[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    v[...] = a
    assert v.ctypes.data % 16 == offset
    return v


GUARD = 64                                  # guard bytes on either side of a Placed buffer


class Placed:
    """An exact-size array of `shape` and `dtype` whose first byte lies `offset` bytes behind a 16-byte boundary, between GUARD bytes
    on either side.  The guards hold `mark`, an element of `dtype`, and so does the array unless `data` is given: a read past an end
    meets the mark (a NaN for floats that ask for it), a write past an end is seen by intact()."""

    def __init__(self, shape, dtype, offset, mark, data=None):
        dt = np.dtype(dtype)
        self.n = int(np.prod(shape)) * dt.itemsize
        self.buf = np.zeros(self.n + 2 * GUARD + 32, np.uint8)
        self.start = GUARD + (-(self.buf.ctypes.data + GUARD)) % 16 + offset
        pattern = np.array([mark]).astype(dt).view(np.uint8)
        self.buf[...] = pattern[(np.arange(self.buf.size) - self.start) % dt.itemsize]
        self.marks = self.buf.copy()
        self.view = self.buf[self.start:self.start + self.n].view(dt).reshape(shape)
        assert self.view.ctypes.data % 16 == offset
        if data is not None:
            self.view[...] = np.ascontiguousarray(data).view(dt).reshape(shape)

    @property
    def ptr(self):
        return self.view.ctypes.data

    def intact(self):
        end = self.start + self.n
        return np.array_equal(self.buf[:self.start], self.marks[:self.start]) and np.array_equal(self.buf[end:], self.marks[end:])


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = load(_DIR, "liblce_hostsim.so")
        _lib.hostsim_last_error.restype = C.c_char_p
        _lib.hostsim_fastdiv.restype = C.c_uint32
    return _lib


def check_round_sat_i8():
    """(number of floats where the kernels' 4-instruction int8 rounding differs from
    saturate(roundf(y)), bits of the first such float) over ALL 2^32 bit patterns but NaNs."""
    l = lib()
    l.hostsim_check_round_sat_i8.restype = C.c_uint64
    first = C.c_uint32(0)
    return int(l.hostsim_check_round_sat_i8(C.byref(first))), first.value


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def option_string(options: dict) -> bytes:
    """{"engine": "stream", "compute_units": 4} -> b"engine=stream;compute_units=4": plan options as hostsim_bconv2d and
    hostsim_plan_estimate take them (the keys and values of lce_hip_bconv2d_plan_set_option, include/lce_hip.h)."""
    return ";".join("%s=%s" % kv for kv in options.items()).encode()


# Where a plan made here differs from a C-ABI plan by default: consecutive segments on the streaming kernel unless a test asks for
# interleaved runs (a C-ABI plan's stream_interleave is "auto": the cost estimate decides).
DEFAULT_OPTIONS = {"stream_interleave": 0}


def bconv2d(spec: O.ConvSpec, dst_type: int, inp, filt, post_mul=None, post_bias=None,
            thresholds=None, out_scale=1.0, out_zero_point=0, kernel="auto", tile=(0, 0),
            max_batch=0, engine="valu", sign_words=None, options=None, out=None):
    """options: plan options by key, e.g. {"compute_units": 4, "stream_rows": 2}, on top of DEFAULT_OPTIONS and of engine / kernel /
    tile (shorthands for three of them; tile (0, 0) = auto).
    sign_words: an int32 array [B,OH,OW,ceil(Cout/32)] that receives the float output's sign bits (the
    matrix-core kernels' second output; stays untouched when the chosen kernel variant cannot write it).
    out: a C-contiguous array of the output's shape and type to write into (e.g. a view into a guarded buffer) instead of a new one."""
    inp = np.ascontiguousarray(inp, np.int32)
    filt = np.ascontiguousarray(filt, np.int32)
    mul = None if post_mul is None else np.ascontiguousarray(post_mul, np.float32)
    bias = None if post_bias is None else np.ascontiguousarray(post_bias, np.float32)
    thr = None if thresholds is None else np.ascontiguousarray(thresholds, np.int32)
    dt = {O.DST_F32: np.float32, O.DST_I8: np.int8, O.DST_BITPACKED: np.int32}[dst_type]
    if out is None:
        out = np.full(spec.output_shape(dst_type), 0x55, dtype=np.uint8).astype(dt) if dt == np.int8 \
            else np.full(spec.output_shape(dst_type), -7, dtype=dt)
    assert out.dtype == dt and out.shape == tuple(spec.output_shape(dst_type)) and out.flags.c_contiguous
    name = C.create_string_buffer(128)
    d = make_desc(spec, dst_type, out_scale, out_zero_point)
    opts = {**DEFAULT_OPTIONS, "engine": engine, "kernel": kernel, "tile": "%dx%d" % tuple(tile) if tile[0] else "auto", **(options or {})}
    rc = lib().hostsim_bconv2d(C.byref(d), option_string(opts), _p(filt), _p(mul), _p(bias), _p(thr), _p(inp), _p(out),
                               _p(sign_words), max_batch, name, 128)
    if rc != 0:
        raise RuntimeError(lib().hostsim_last_error().decode())
    return out, name.value.decode()


def last_int8_floor() -> int:
    """1: the last convolution's int8 rounding ran as floor(x + 0.5) (the planner proved it equal to round-half-away on that plan),
    0: as round-half-away, -1: not an int8 plan of the streaming / pointwise kernels."""
    return int(lib().hostsim_last_int8_floor())


def last_int8_adjusted() -> int:
    """Channels of the last int8 plan that the planner's proof of the one-instruction forms gave neighbouring parameters (lce_plan.cpp, prepare_int8_epilogue)."""
    return int(lib().hostsim_last_int8_adjusted())


def bitpack(x: np.ndarray, zero_point: int = 0, force_rows: bool = False) -> np.ndarray:
    x = np.ascontiguousarray(x)
    cols = x.shape[-1]
    rows = int(np.prod(x.shape[:-1], dtype=np.int64)) if x.ndim > 1 else 1
    out = np.full(x.shape[:-1] + ((cols + 31) // 32,), -1, np.int32)
    t = {np.dtype(np.float32): 0, np.dtype(np.int8): 1, np.dtype(np.bool_): 3, np.dtype(np.uint8): 3}[x.dtype]
    lib().hostsim_bitpack(t, _p(x), C.c_uint64(rows), C.c_uint64(cols), C.c_int32(zero_point),
                          _p(out), int(force_rows))
    return out


def unpack(words: np.ndarray, cols: int, dtype, scale=1.0, zero_point=0) -> np.ndarray:
    words = np.ascontiguousarray(words, np.int32)
    rows = int(np.prod(words.shape[:-1], dtype=np.int64)) if words.ndim > 1 else 1
    out = np.empty(words.shape[:-1] + (cols,), dtype=dtype)
    t = {np.dtype(np.float32): 0, np.dtype(np.int8): 1, np.dtype(np.bool_): 3}[np.dtype(dtype)]
    lib().hostsim_unpack(t, _p(words), C.c_uint64(rows), C.c_uint64(cols), C.c_float(scale),
                         C.c_int32(zero_point), _p(out))
    return out


def bmaxpool(x, fh, fw, sh, sw, padding):
    x = np.ascontiguousarray(x, np.int32)
    b, h, w, c = x.shape
    oh = (h + sh - 1) // sh if padding == O.PADDING_SAME else (h + sh - fh) // sh
    ow = (w + sw - 1) // sw if padding == O.PADDING_SAME else (w + sw - fw) // sw
    out = np.empty((b, oh, ow, c), np.int32)
    lib().hostsim_bmaxpool(_p(x), b, h, w, c, fh, fw, sh, sw, padding, _p(out))
    return out


def fastdiv(n: int, d: int) -> int:
    return lib().hostsim_fastdiv(C.c_uint32(n), C.c_uint32(d))
