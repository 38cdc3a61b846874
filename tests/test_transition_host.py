"""lce_hip_pool_depthwise_f32 / lce_hip_pool_depthwise_i8 without a GPU: every refusal of the two host-only checks (what either
entry's own check refuses, a pool of the wrong type, a depthwise input that is not the pool's output, a quantization that differs,
AVERAGE as unsupported), the refusals of the run entries that come before any device call (null pointers, overlap), the rule of
`_path` against its statement, and the Python wrappers' argument checks.  The GPU side is tests/test_gpu_transition.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

amd = importlib.import_module("compute-engine_amd")

SAME, VALID = amd.PADDING_SAME, amd.PADDING_VALID


def pool_desc(type=amd.F32, op=amd.POOL_MAX, shape=(2, 8, 8, 32), filt=(2, 2), stride=(1, 1), padding=SAME, act=amd.ACT_NONE, scale=0.05, zp=-3):
    return amd.Pool2dDesc(op, type, *shape, *filt, *stride, padding, act, scale, zp)


def dw_desc(shape=(2, 8, 8, 32), m=1, filt=(3, 3), stride=(2, 2), padding=SAME, act=amd.ACT_NONE):
    return amd.DepthwiseDesc(*shape, m, *filt, *stride, padding, act)


def dw8_desc(shape=(2, 8, 8, 32), m=1, filt=(3, 3), stride=(2, 2), padding=SAME, act=amd.ACT_NONE, q_in=(0.05, -3), q_out=(0.04, 5)):
    return amd.DepthwiseI8Desc(*shape, m, *filt, *stride, padding, act, q_in[0], q_in[1], q_out[0], q_out[1])


def check(kind, pool, dw):
    h, w = C.c_int32(-1), C.c_int32(-1)
    rc = getattr(amd.lib(), "lce_hip_pool_depthwise_%s_check" % kind)(None if pool is None else C.byref(pool), None if dw is None else C.byref(dw),
                                                                    C.byref(h), C.byref(w))
    return rc, (h.value, w.value), amd.lib().lce_hip_last_error().decode()


def test_the_symbols_are_declared_and_exported():
    """Fails without the feature."""
    for name in ("lce_hip_pool_depthwise_f32", "lce_hip_pool_depthwise_f32_check", "lce_hip_pool_depthwise_f32_path", "lce_hip_pool_depthwise_f32_forced",
                 "lce_hip_pool_depthwise_i8", "lce_hip_pool_depthwise_i8_check", "lce_hip_pool_depthwise_i8_path", "lce_hip_pool_depthwise_i8_forced"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)


def test_the_checks_accept_a_quicknet_transition_and_report_the_blurred_extents():
    assert check("f32", pool_desc(), dw_desc())[:2] == (amd.OK, (4, 4))
    assert check("i8", pool_desc(amd.I8), dw8_desc())[:2] == (amd.OK, (4, 4))
    # odd extents, a VALID 3x3 / 2 pool (7 x 9 -> 3 x 4) and a 5x5 / 2 SAME depthwise window behind it with a multiplier
    assert check("f32", pool_desc(shape=(1, 7, 9, 5), filt=(3, 3), stride=(2, 2), padding=VALID), dw_desc((1, 3, 4, 5), 2, (5, 5)))[:2] == (amd.OK, (2, 2))
    # the extents are nullable
    assert amd.lib().lce_hip_pool_depthwise_f32_check(C.byref(pool_desc()), C.byref(dw_desc()), None, None) == amd.OK


REFUSALS_F32 = {
    "null pool": (None, dw_desc(), amd.ERR_INVALID, "null desc"),
    "null depthwise": (pool_desc(), None, amd.ERR_INVALID, "null desc"),
    "pool: unknown op": (pool_desc(op=7), dw_desc(), amd.ERR_INVALID, "unknown op"),
    "pool: type": (pool_desc(type=amd.BITPACKED), dw_desc(), amd.ERR_INVALID, "type must be"),
    "pool: extent": (pool_desc(shape=(2, 0, 8, 32)), dw_desc(), amd.ERR_INVALID, "extents must be positive"),
    "pool: filter": (pool_desc(filt=(0, 2)), dw_desc(), amd.ERR_INVALID, "filter must be positive"),
    "pool: stride": (pool_desc(stride=(1, -1)), dw_desc(), amd.ERR_INVALID, "stride must be positive"),
    "pool: padding": (pool_desc(padding=2), dw_desc(), amd.ERR_INVALID, "padding must be"),
    "pool: activation": (pool_desc(act=9), dw_desc(), amd.ERR_INVALID, "unknown activation"),
    "pool: empty output": (pool_desc(filt=(9, 9), padding=VALID), dw_desc(), amd.ERR_INVALID, "empty output"),
    "pool: taps": (pool_desc(filt=(300, 300)), dw_desc(), amd.ERR_UNSUPPORTED, "taps"),
    "depthwise: multiplier": (pool_desc(), dw_desc(m=0), amd.ERR_INVALID, "depth multiplier"),
    "depthwise: filter": (pool_desc(), dw_desc(filt=(3, 0)), amd.ERR_INVALID, "filter must be positive"),
    "depthwise: stride": (pool_desc(), dw_desc(stride=(0, 2)), amd.ERR_INVALID, "stride must be positive"),
    "depthwise: padding": (pool_desc(), dw_desc(padding=-1), amd.ERR_INVALID, "padding must be"),
    "depthwise: activation": (pool_desc(), dw_desc(act=4), amd.ERR_INVALID, "unknown activation"),
    "depthwise: empty output": (pool_desc(), dw_desc(filt=(9, 9), padding=VALID), amd.ERR_INVALID, "empty output"),
    "depthwise: stride above 2^30": (pool_desc(), dw_desc(stride=((1 << 30) + 1, 1)), amd.ERR_UNSUPPORTED, "2\\^30"),
    "an int8 pool": (pool_desc(amd.I8), dw_desc(), amd.ERR_INVALID, "the pool's type must be float32"),
    "another batch": (pool_desc(), dw_desc((3, 8, 8, 32)), amd.ERR_INVALID, "is not the pool's output"),
    "another height": (pool_desc(), dw_desc((2, 7, 8, 32)), amd.ERR_INVALID, "is not the pool's output"),
    "another width": (pool_desc(stride=(1, 2)), dw_desc(), amd.ERR_INVALID, "is not the pool's output"),
    "other channels": (pool_desc(), dw_desc((2, 8, 8, 16)), amd.ERR_INVALID, "is not the pool's output"),
    "AVERAGE": (pool_desc(op=amd.POOL_AVERAGE), dw_desc(), amd.ERR_UNSUPPORTED, "only a MAX pool"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS_F32))
def test_each_refusal_of_the_float_check(name):
    import re
    pool, dw, code, word = REFUSALS_F32[name]
    rc, _, message = check("f32", pool, dw)
    assert rc == code and re.search(word, message), (name, rc, message)


def test_the_refusals_of_the_int8_check():
    for pool, dw, code, word in (
            (pool_desc(amd.I8), dw8_desc(), amd.OK, ""),
            (pool_desc(amd.F32), dw8_desc(), amd.ERR_INVALID, "the pool's type must be int8"),
            (pool_desc(amd.I8, zp=200), dw8_desc(), amd.ERR_INVALID, "zero_point"),
            (pool_desc(amd.I8, scale=0.0), dw8_desc(), amd.ERR_INVALID, "scale"),
            (pool_desc(amd.I8), dw8_desc(q_out=(float("inf"), 0)), amd.ERR_INVALID, "scale"),
            (pool_desc(amd.I8), dw8_desc(q_in=(0.05, -4)), amd.ERR_INVALID, "quantization"),
            (pool_desc(amd.I8), dw8_desc(q_in=(0.050001, -3)), amd.ERR_INVALID, "quantization"),
            (pool_desc(amd.I8), dw8_desc((2, 8, 9, 32)), amd.ERR_INVALID, "is not the pool's output"),
            (pool_desc(amd.I8, op=amd.POOL_AVERAGE), dw8_desc(), amd.ERR_UNSUPPORTED, "only a MAX pool"),
            (None, dw8_desc(), amd.ERR_INVALID, "null desc"), (pool_desc(amd.I8), None, amd.ERR_INVALID, "null desc")):
        rc, _, message = check("i8", pool, dw)
        assert rc == code and (rc == amd.OK or word in message), (rc, message, word)


def _buffers(dtype, shape=(2, 8, 8, 32), out_shape=(2, 4, 4, 32), filt=(3, 3), offset=0):
    """Host arrays standing in for device operands (the host-only entries look at addresses alone): 16-byte aligned but for
    `offset` bytes."""
    def placed(n):
        raw = np.zeros(n * np.dtype(dtype).itemsize + 32, np.uint8)
        start = (-raw.ctypes.data) % 16 + offset
        return raw[start:start + n * np.dtype(dtype).itemsize]
    x, w, out = placed(int(np.prod(shape))), placed(filt[0] * filt[1] * out_shape[3]), placed(int(np.prod(out_shape)))
    third = np.zeros(3 * out_shape[3] + 4, np.int32) if dtype == np.int8 else placed(out_shape[3])
    bits = np.zeros(int(np.prod(out_shape[:3])) * ((out_shape[3] + 31) // 32), np.int32)
    return x, w, third, out, bits


def path_of(kind, pool, dw, bufs, want_out=True, want_bits=True):
    x, w, third, out, bits = bufs
    took = C.c_int32(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = getattr(amd.lib(), "lce_hip_pool_depthwise_%s_path" % kind)(C.byref(pool), C.byref(dw), p(x), p(w), p(third), p(out) if want_out else None,
                                                                   p(bits) if want_bits else None, C.byref(took))
    return rc, took.value, amd.lib().lce_hip_last_error().decode()


def test_the_path_rule_is_the_stated_one():
    """1 (the 16-byte path) needs: multiplier 1; channels % 4 (float) / % 16 (int8), % 32 with bits; everything 16-byte aligned; pool
    stride 1 x 1 and filter <= 2 x 2; depthwise filter <= 3 x 3.  Anything else is 0 (the rows)."""
    assert path_of("f32", pool_desc(), dw_desc(), _buffers(np.float32))[:2] == (amd.OK, 1)
    assert path_of("i8", pool_desc(amd.I8), dw8_desc(), _buffers(np.int8))[:2] == (amd.OK, 1)
    # channels: 36 float channels are chunks but no words; 48 int8 channels alike; 33 are neither
    for kind, dtype, c, bits, want in (("f32", np.float32, 36, False, 1), ("f32", np.float32, 36, True, 0), ("f32", np.float32, 33, False, 0),
                                       ("i8", np.int8, 48, False, 1), ("i8", np.int8, 48, True, 0), ("i8", np.int8, 40, False, 0)):
        pool = pool_desc(amd.I8 if kind == "i8" else amd.F32, shape=(2, 8, 8, c))
        dw = (dw8_desc if kind == "i8" else dw_desc)((2, 8, 8, c))
        assert path_of(kind, pool, dw, _buffers(dtype, (2, 8, 8, c), (2, 4, 4, c)), want_bits=bits)[:2] == (amd.OK, want), (kind, c, bits)
    # alignment
    assert path_of("f32", pool_desc(), dw_desc(), _buffers(np.float32, offset=4))[:2] == (amd.OK, 0)
    assert path_of("i8", pool_desc(amd.I8), dw8_desc(), _buffers(np.int8, offset=1))[:2] == (amd.OK, 0)
    # the geometry class
    for pool_kw, dw_kw, out_hw, want in ((dict(filt=(1, 2)), dict(), (4, 4), 1), (dict(filt=(1, 1)), dict(filt=(1, 1), stride=(1, 1)), (8, 8), 1),
                                         (dict(filt=(3, 2)), dict(), (4, 4), 0), (dict(filt=(2, 2), stride=(2, 2)), dict(shape=(2, 4, 4, 32)), (2, 2), 0),
                                         (dict(), dict(filt=(5, 5)), (4, 4), 0), (dict(), dict(filt=(3, 4)), (4, 4), 0)):
        pool, dw = pool_desc(**pool_kw), dw_desc(**dw_kw)
        bufs = _buffers(np.float32, out_shape=(2,) + out_hw + (32,), filt=dw_kw.get("filt", (3, 3)))
        assert path_of("f32", pool, dw, bufs)[:2] == (amd.OK, want), (pool_kw, dw_kw)
    # a depth multiplier
    assert path_of("f32", pool_desc(), dw_desc(m=2), _buffers(np.float32, out_shape=(2, 4, 4, 64)))[:2] == (amd.OK, 0)


def test_the_run_entries_refuse_before_any_device_call():
    """Null pointers, overlap and misalignment are found on addresses alone: no device is needed to be refused."""
    x, w, bias, out, bits = _buffers(np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    run = lambda *a: (amd.lib().lce_hip_pool_depthwise_f32(C.byref(pool_desc()), C.byref(dw_desc()), *[p(t) for t in a], None),
                      amd.lib().lce_hip_last_error().decode())
    for args, word in (((None, w, bias, out, bits), "null input"), ((x, None, bias, out, bits), "null filter"), ((x, w, bias, None, None), "both outputs"),
                       ((x, w, bias, x[64:], None), "overlaps the input"), ((x, w, bias, None, w), "overlaps the filter"),
                       ((x, w, bias, None, bias), "overlaps the bias"), ((x, w, bias, out, out[16:]), "two outputs overlap"),
                       ((x[2:], w, bias, out, None), "4-byte aligned")):
        rc, message = run(*args)
        assert rc == amd.ERR_INVALID and word in message, (rc, message, word)
    rc = amd.lib().lce_hip_pool_depthwise_f32(C.byref(pool_desc(op=amd.POOL_AVERAGE)), C.byref(dw_desc()), p(x), p(w), None, p(out), None, None)
    assert rc == amd.ERR_UNSUPPORTED
    x, w, table, out, bits = _buffers(np.int8)
    run8 = lambda *a: (amd.lib().lce_hip_pool_depthwise_i8(C.byref(pool_desc(amd.I8)), C.byref(dw8_desc()), *[p(t) for t in a], None),
                       amd.lib().lce_hip_last_error().decode())
    for args, word in (((x, w, None, out, bits), "null table"), ((x, w, table, table.view(np.int8), None), "overlaps the table"),
                       ((x, w, table, x, None), "overlaps the input"), ((x, w, table, None, table), "overlaps the table"),
                       ((x, w, table.view(np.int8)[1:], out, None), "table_dev must be 4-byte aligned")):
        rc, message = run8(*args)
        assert rc == amd.ERR_INVALID and word in message, (rc, message, word)
    took = C.c_int32()
    assert amd.lib().lce_hip_pool_depthwise_f32_path(C.byref(pool_desc()), C.byref(dw_desc()), p(x), p(w), None, p(out), None, None) == amd.ERR_INVALID
    for bad in (-1, 2):
        assert amd.lib().lce_hip_pool_depthwise_f32_forced(C.byref(pool_desc()), C.byref(dw_desc()), bad, p(x), p(w), None, p(out), None, None) == amd.ERR_INVALID
        assert "unknown path" in amd.lib().lce_hip_last_error().decode()


def test_the_python_wrappers_check_their_arguments_without_a_device():
    x = np.zeros((2, 8, 8, 32), np.float32)
    w = np.zeros((1, 3, 3, 32), np.float32)
    for kw, word in ((dict(pool_filter=(0, 2)), "filter"), (dict(pool_padding=3), "padding"), (dict(filter=w[..., :16]), "filter must be float32"),
                     (dict(bias=np.zeros(3, np.float32)), "bias"), (dict(stride=0), "stride"), (dict(out=False), "no output"), (dict(path=2), "path")):
        args = dict(dict(x=x, pool_filter=(2, 2), filter=w, stride=2), **kw)
        with pytest.raises(ValueError, match=word):
            amd.pool_depthwise(**args)
    with pytest.raises(ValueError, match="float32"):
        amd.pool_depthwise(x.astype(np.int8), (2, 2), w)
    with pytest.raises(ValueError, match="int8"):
        amd.pool_depthwise_i8(x, (2, 2), w.astype(np.int8), np.zeros((3, 32), np.int32), (0.5, 0), (0.5, 0))
    with pytest.raises(ValueError, match="table"):
        amd.pool_depthwise_i8(x.astype(np.int8), (2, 2), w.astype(np.int8), np.zeros((3, 16), np.int32), (0.5, 0), (0.5, 0))
