"""The int8 classifier head and the float / int8 boundary (lce_hip_fully_connected_i8, lce_hip_mean_i8, lce_hip_softmax_i8,
lce_hip_quantize_f32_i8, lce_hip_dequantize_i8_f32; "head_i8" and "quantize" of lce_tflite_model_open_passes) on the CPU: the NumPy
restatements (tests/head_i8_ref.py) against float64 and hand-worked answers; every refusal of the check, prepare and run entries
and the edge of each overflow bound; the value functions of the kernels' epilogues, compiled for the host, against the
restatements on 10^5 random inputs; and the partitions of the fixtures of tests/head_i8_models.py with and without the names."""
import ctypes as C
import importlib

import numpy as np
import pytest

import conv2d_i8_ref as CR
import head_i8_cases as K
import head_i8_models as HM
import head_i8_ref as H
import head_models as FHM
import hostsim_head_i8_lib as S
import int8_conv_models as M
from head_models import fc_op, softmax_op
from test_head_sections_host import NO_HEAD

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")


# ---- the restatements against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(K.MEAN_SETS)))
def test_the_mean_is_the_rounded_exact_mean_up_to_its_two_roundings(case):
    """Two roundings -- the multiplier's (at most half a unit of acc si / so: 0.5 / n output units) and the division's -- so the
    byte may differ from round-half-away(acc si / (n so)) by at most 1, and only within 0.5 / n + 1e-6 of a tie."""
    h, w, c, q_in, q_out = K.MEAN_SETS[case]
    x = K.mean_input(h, w, c, 4, case)
    got = H.mean_i8(x, q_in, q_out).astype(np.int64)
    exact = H.mean_exact(x, q_in, q_out)
    want = np.clip(H.round_half_away(exact) + q_out[1], -128, 127).astype(np.int64)
    off = got != want
    print("mean set %d: %d elements, %d differ" % (case, got.size, int(off.sum())))
    assert np.abs(got - want).max() <= 1
    to_tie = np.abs(np.abs(exact - np.floor(exact)) - 0.5)
    assert np.all(to_tie[off] <= 0.5 / (h * w) + 1e-6)
    assert got.shape == (4, c) and (np.unique(got).size > 3 or h * w == 1)
    if q_in == q_out and h * w == 1:
        assert np.array_equal(got, x.reshape(4, c))                       # one pixel at equal quantization: the identity


@pytest.mark.parametrize("case", range(len(K.SOFTMAX_SETS)))
def test_the_softmax_is_the_rounded_float64_softmax_up_to_float_error(case):
    """p * 256 carries at most about 1.2e-4 of float32 error (E within 1 ulp, a sum of up to 1000 terms, a division, a
    multiply): the byte may differ from round(256 softmax) by at most 1, and only within 2^-10 of a tie."""
    scale, beta, cols = K.SOFTMAX_SETS[case]
    q = K.softmax_input(64, cols, 100 + case)
    got = H.softmax_i8(q, scale, beta).astype(np.int64)
    exact = H.softmax_exact(q, scale, beta)
    want = np.minimum(H.round_half_away(exact) - 128, 127).astype(np.int64)
    off = got != want
    to_tie = np.abs(np.abs(exact - np.floor(exact)) - 0.5)
    print("softmax set %d: %d elements, %d differ, closest to a tie %.2e" % (case, got.size, int(off.sum()), to_tie.min()))
    assert np.abs(got - want).max() <= 1 and np.all(to_tie[off] <= 2.0 ** -10)
    assert np.unique(got).size > 3                                            # not degenerate
    if 255 * scale * beta > np.log(cols) + 6:                                 # the one-hot row is one-hot in probabilities too
        assert got[-1].max() == 127 and np.sort(got[-1])[-2] == -128
    if case == 4:
        assert exact[-1].max() > 255.5                                        # round gives 256: the clamp at 127 is what keeps it a byte
    assert got.min() >= -128 and got.dtype == np.int64


def test_the_fully_connected_restatement_is_the_one_pixel_convolution():
    """Against an independent statement: the integer matrix product of (x - zi) and w, then conv2d_i8_ref.finish."""
    for k, (batch, kk, n) in enumerate([(3, 70, 33), (17, 512, 10), (1, 1, 1)]):
        x, w, bias, sw, q_in, q_out = K.fc_operands(batch, kk, n, k, K.ZIS[k], per_channel=k != 1, bias=k != 2)
        acc = (x.astype(np.int64) - q_in[1]) @ w.astype(np.int64).T
        want = CR.finish(acc, bias, sw, q_in, q_out, K.ACTS[k])
        got = H.fully_connected_i8(x, w, bias, sw, q_in, q_out, K.ACTS[k])
        assert np.array_equal(got, want)
        image = CR.conv2d_i8(x.reshape(batch, 1, 1, kk), w.reshape(n, 1, 1, kk), bias, sw, q_in, q_out, (1, 1), CR.SAME, K.ACTS[k])
        assert np.array_equal(got, image.reshape(batch, n))
        if batch * n > 50:
            assert np.unique(got).size > 20


def test_quantize_and_dequantize_by_hand():
    f = lambda *v: np.array(v, np.float32)
    # scale 0.5, zero point 3: t = 2 x.  Exact halves of both signs go AWAY from zero: 0.25 -> 0.5 -> 1, -0.25 -> -1, 0.75 -> 1.5 -> 2
    assert H.quantize(f(0.25, -0.25, 0.75, -0.75, 1.25, 0.0, -0.0, 0.2, -0.2), 0.5, 3).tolist() == [4, 2, 5, 1, 6, 3, 3, 3, 3]
    # the clamp edges: r in [-128 - zp, 127 - zp] = [-131, 124]: 62 -> 124 -> 127; 62.25 -> 124.5 -> 125 -> clamped; -65.5 -> -131 -> -128
    assert H.quantize(f(62.0, 62.25, 61.5, -65.5, -65.75, -65.0), 0.5, 3).tolist() == [127, 127, 126, -128, -128, -127]
    # NaN gives the zero point, the infinities and what is beyond int32 saturate
    assert H.quantize(f(np.nan, np.inf, -np.inf, 3e9, -3e9, 1e38), 0.5, 3).tolist() == [3, 127, -128, 127, -128, 127]
    assert H.quantize(f(np.nan, 0.0), 0.5, -128).tolist() == [-128, -128] and H.quantize(f(np.nan), 2.0, 127).tolist() == [127]
    # just below a half stays down: 0.49999997f is the float before 0.5
    assert H.quantize(f(0.49999997, 0.5, 1.5, 2.5), 1.0, 0).tolist() == [0, 1, 2, 3]
    # dequantize: (q - zp) * scale in one float32 multiply = the double product rounded once
    q = np.arange(-128, 128).astype(np.int8)
    for scale, zp in ((0.05, -4), (0.0157, -128), (1.0 / 256.0, -128), (1.0, 127)):
        d = H.dequantize(q, scale, zp)
        ref = ((q.astype(np.float64) - zp) * float(np.float32(scale))).astype(np.float32)
        assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), ref.view(np.uint32))
    assert H.dequantize(np.array([-128, 127, 3], np.int8), 0.5, 3).tolist() == [-65.5, 62.0, 0.0]


@pytest.mark.parametrize("scale,zp", [(0.05, -4), (0.0157, -128), (1.0 / 256.0, -128)])
def test_quantize_of_dequantize_is_the_identity_on_all_256_bytes(scale, zp):
    q = np.arange(-128, 128).astype(np.int8)
    assert np.array_equal(H.quantize(H.dequantize(q, scale, zp), scale, zp), q)
    assert np.array_equal(S.quantize_value(S.dequantize_value(q, scale, zp), scale, zp), q.astype(np.int32))


# ---- the value functions the kernels run, compiled for the host ------------------------------------------------------------------------
def test_the_kernels_requantizing_epilogues_equal_the_restatements_on_1e5_inputs():
    g = np.random.default_rng(5)
    total = 0
    for _ in range(100):
        m, e = int(g.integers(1 << 30, 1 << 31)), int(g.integers(-31, 8))
        lim = (H.INT32_MAX >> max(e, 0)) // 2                   # acc + cst stays inside what prepare guarantees
        acc, cst = g.integers(-lim, lim + 1, 1000), g.integers(-lim, lim + 1, 1000)
        zo, act = int(g.integers(-128, 128)), int(g.integers(0, 4))
        lo, hi = CR.activation_range(act, 0.05, zo)
        want = np.clip(CR.requantize(acc + cst, m, e) + zo, lo, hi)
        assert np.array_equal(S.fc_value(acc, cst, np.full(1000, m), np.full(1000, e), zo, lo, hi), want), (m, e)
        total += 1000
    assert total >= 10 ** 5
    total = 0
    for _ in range(100):
        n = int(g.integers(1, 3000))
        m, e = H.quantize_multiplier(float(np.exp(g.uniform(np.log(0.01), np.log(60.0)))))
        if not H.mean_bound_ok(n, e):
            continue
        zo = int(g.integers(-128, 128))
        acc = np.concatenate([g.integers(-255 * n, 255 * n + 1, 1000), [0, 255 * n, -255 * n, n // 2, -(n // 2), 1, -1]])
        t = CR.requantize(acc, m, e)
        q = np.where(t > 0, H.trunc_div(t + n // 2, n), H.trunc_div(t - n // 2, n))
        assert np.array_equal(S.mean_value(acc, m, e, n, zo), np.clip(q + zo, -128, 127)), (n, m, e)
        total += acc.size
    assert total >= 5 * 10 ** 4


def test_the_kernels_softmax_and_boundary_functions_equal_the_restatements_on_1e5_inputs():
    g = np.random.default_rng(6)
    d = -g.integers(0, 256, 100000)
    for sb in (0.05, 0.003, 1.0, 0.41):
        want = H.HR.exp32((d.astype(np.float32) * np.float32(sb)).astype(np.float32))
        assert np.array_equal(S.softmax_exp(d, sb).view(np.uint32), want.view(np.uint32))
    e = g.uniform(0, 1, 100000).astype(np.float32)
    e[:4] = [1.0, 0.0, 0.001953125, 0.005859375]                       # with s = 1: 256, 0, an exact half (0.5 -> 1), 1.5 -> 2
    s = np.maximum(e, g.uniform(1, 50, 100000).astype(np.float32))
    s[:4] = 1.0
    t = ((e / s).astype(np.float32) * np.float32(256)).astype(np.float32)
    want = np.minimum(H.roundf32(t).astype(np.int32) - 128, 127)
    got = S.softmax_value(e, s)
    assert np.array_equal(got, want) and got[:4].tolist() == [127, -128, -127, -126]
    x = (g.standard_normal(100000) * 4).astype(np.float32)
    x[:8] = [np.nan, np.inf, -np.inf, 0.025, -0.025, 0.075, 1e30, -1e30]
    for scale, zp in ((0.05, -4), (0.0157, -128), (1.0, 127)):
        assert np.array_equal(S.quantize_value(x, scale, zp), H.quantize(x, scale, zp).astype(np.int32))
        q = g.integers(-128, 128, 100000)
        assert np.array_equal(S.dequantize_value(q, scale, zp).view(np.uint32), H.dequantize(q.astype(np.int8), scale, zp).view(np.uint32))


# ---- check and prepare -----------------------------------------------------------------------------------------------------------------
def fc_desc(batch=2, inputs=8, outputs=4, act=amd.ACT_NONE, q_in=(0.5, 0), q_out=(0.5, 0)):
    return amd.FcI8Desc(batch, inputs, outputs, act, q_in[0], q_in[1], q_out[0], q_out[1])


def mean_desc(batch=2, h=7, w=7, c=8, q_in=(0.5, 0), q_out=(0.5, 0)):
    return amd.MeanI8Desc(batch, h, w, c, q_in[0], q_in[1], q_out[0], q_out[1])


def last():
    return amd.lib().lce_hip_last_error().decode()


def c_fc_prepare(d, w, bias, sw):
    table = np.zeros((3, d.outputs), np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    sw = np.ascontiguousarray(np.atleast_1d(sw), np.float32)
    rc = amd.lib().lce_hip_fully_connected_i8_prepare(C.byref(d), w.ctypes.data, None if bias is None else bias.ctypes.data, sw.ctypes.data,
                                                      sw.size, table.ctypes.data, C.byref(lo), C.byref(hi))
    return rc, last(), table, lo.value, hi.value


def test_fc_prepare_equals_the_restatement_and_the_conv_entrys_table():
    g = np.random.default_rng(12)
    for n in range(40):
        k, cout = int(g.integers(1, 600)), int(g.integers(1, 40))
        zi, zo, act = int(g.integers(-128, 128)), int(g.integers(-128, 128)), int(g.integers(0, 4))
        si, so = (float(np.float32(np.exp(g.uniform(np.log(1e-3), np.log(1.0))))) for _ in range(2))
        w = g.integers(-128, 128, (cout, k), dtype=np.int64).astype(np.int8)
        bias = None if n % 3 == 0 else g.integers(-(1 << 20), 1 << 20, cout, dtype=np.int64).astype(np.int32)
        sw = np.exp(g.uniform(np.log(1e-4), np.log(0.5), cout if n % 2 else 1)).astype(np.float32)
        rc, msg, table, lo, hi = c_fc_prepare(fc_desc(1, k, cout, act, (si, zi), (so, zo)), w, bias, sw)
        try:
            want = H.fc_table(w, bias, sw, si, zi, so)
        except ValueError:
            assert rc == amd.ERR_UNSUPPORTED and "channel" in msg, msg
            continue
        assert rc == amd.OK, msg
        assert np.array_equal(table, want) and (lo, hi) == CR.activation_range(act, so, zo)
        py = amd.fully_connected_i8_prepare(w, bias, sw, (si, zi), (so, zo), act)
        assert np.array_equal(py[0], want) and py[1:] == (lo, hi)
        conv = amd.conv2d_i8_prepare(w.reshape(cout, 1, 1, k), bias, sw, (si, zi), (so, zo), act)
        assert np.array_equal(conv[0], table) and conv[1:] == (lo, hi)


def test_the_fc_overflow_bound_just_under_and_just_over():
    assert 255 * 128 * 65793 + 127 == 2 ** 31 - 1
    for k, bias, ok in ((65793, None, True), (65793, [5, -127], True), (65793, [5, -128], False), (65794, None, False)):
        w = np.ones((2, k), np.int8)
        b = None if bias is None else np.array(bias, np.int32)
        rc, msg, table, _, _ = c_fc_prepare(fc_desc(1, k, 2), w, b, 2.0 ** -20)
        if ok:
            assert rc == amd.OK and table[0].tolist() == ([0, 0] if b is None else bias), msg
        else:
            assert rc == amd.ERR_UNSUPPORTED and "channel %d" % (1 if bias else 0) in msg and "exceeds 2^31 - 1" in msg, msg
    lib = amd.lib()
    assert lib.lce_hip_fully_connected_i8_check(C.byref(fc_desc(1, 65793, 2))) == amd.OK
    assert lib.lce_hip_fully_connected_i8_check(C.byref(fc_desc(1, 65794, 2))) == amd.ERR_UNSUPPORTED and "65794" in last()
    # a left shift: K = 1, bound 32640; e = 17 overflows, e = 16 passes
    w = np.ones((3, 1), np.int8)
    rc, msg, _, _, _ = c_fc_prepare(fc_desc(1, 1, 3, q_in=(1.0, 0), q_out=(1.0, 0)), w, None, [1.0, 0.75 * 2.0 ** 17, 1.0])
    assert rc == amd.ERR_UNSUPPORTED and "channel 1" in msg and "2^17" in msg, msg
    assert c_fc_prepare(fc_desc(1, 1, 3, q_in=(1.0, 0), q_out=(1.0, 0)), w, None, [1.0, 0.75 * 2.0 ** 16, 1.0])[0] == amd.OK


def test_the_fc_entries_refuse_what_is_malformed():
    lib = amd.lib()
    for d, msg in ((fc_desc(batch=0), "extents must be positive"), (fc_desc(inputs=0), "extents must be positive"), (fc_desc(outputs=-1), "extents"),
                   (fc_desc(act=4), "unknown activation"), (fc_desc(q_in=(0.0, 0)), "input_scale must be finite and positive"),
                   (fc_desc(q_in=(float("nan"), 0)), "input_scale"), (fc_desc(q_out=(float("inf"), 0)), "output_scale must be finite"),
                   (fc_desc(q_out=(-0.5, 0)), "output_scale"), (fc_desc(q_in=(0.5, 128)), "input_zero_point must be in"),
                   (fc_desc(q_out=(0.5, -129)), "output_zero_point must be in")):
        assert lib.lce_hip_fully_connected_i8_check(C.byref(d)) == amd.ERR_INVALID and msg in last(), last()
    assert lib.lce_hip_fully_connected_i8_check(None) == amd.ERR_INVALID and "null desc" in last()
    assert lib.lce_hip_fully_connected_i8_check(C.byref(fc_desc(batch=2 ** 31 - 1, inputs=1, outputs=2 ** 31 - 1))) == amd.ERR_UNSUPPORTED and "tiles" in last()
    w, sw = np.ones((4, 8), np.int8), np.full(4, 0.5, np.float32)
    table, lo, hi = np.zeros((3, 4), np.int32), C.c_int32(), C.c_int32()
    good = dict(d=fc_desc(), w=w.ctypes.data, b=None, s=sw.ctypes.data, n=4, t=table.ctypes.data, lo=C.byref(lo), hi=C.byref(hi))

    def call(**kw):
        a = {**good, **kw}
        rc = lib.lce_hip_fully_connected_i8_prepare(C.byref(a["d"]) if a["d"] is not None else None, a["w"], a["b"], a["s"], a["n"], a["t"], a["lo"], a["hi"])
        return rc, last()
    assert call()[0] == amd.OK
    for kw, msg in ((dict(d=None), "null desc"), (dict(w=None), "null weights"), (dict(s=None), "null weight scales"), (dict(t=None), "null result"),
                    (dict(lo=None), "null result"), (dict(hi=None), "null result"), (dict(n=2), "2 scales"), (dict(n=0), "0 scales"),
                    (dict(d=fc_desc(q_in=(0.0, 0))), "input_scale"), (dict(d=fc_desc(q_out=(0.5, 200))), "output_zero_point"),
                    (dict(d=fc_desc(outputs=0)), "extents must be positive"), (dict(d=fc_desc(act=9)), "unknown activation")):
        rc, text = call(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_fully_connected_i8"), (kw, text)
    bad = sw.copy()
    bad[2] = np.inf
    rc, text = call(s=bad.ctypes.data)
    assert rc == amd.ERR_INVALID and "channel 2" in text


def test_mean_prepare_and_the_edge_of_its_bound():
    lib = amd.lib()
    m, e = C.c_int32(), C.c_int32()
    prep = lambda d: (lib.lce_hip_mean_i8_prepare(C.byref(d), C.byref(m), C.byref(e)), last(), m.value, e.value)
    g = np.random.default_rng(2)
    for _ in range(50):
        si, so = (float(np.float32(np.exp(g.uniform(np.log(1e-3), np.log(1.0))))) for _ in range(2))
        h, w = int(g.integers(1, 40)), int(g.integers(1, 40))
        rc, msg, mm, ee = prep(mean_desc(1, h, w, 3, (si, 0), (so, 0)))
        want = H.mean_multiplier(si, so)
        if H.mean_bound_ok(h * w, want[1]):
            assert rc == amd.OK and (mm, ee) == want, msg
            assert amd.mean_i8_prepare((1, h, w, 3), (si, 0), (so, 0)) == want
        else:
            assert rc == amd.ERR_UNSUPPORTED and "could leave int32" in msg
    # e <= 0 (a multiplier below 1; 0.5 = 2^30 x 2^(0 - 31)): 255 n + n / 2 <= 2^31 - 1 holds up to n = 8405024 and fails at 8405025
    half = dict(q_in=(0.25, 0), q_out=(0.5, 0))
    assert H.mean_multiplier(0.25, 0.5) == (1 << 30, 0)
    assert 255 * 8405024 + 8405024 // 2 <= 2 ** 31 - 1 < 255 * 8405025 + 8405025 // 2
    assert prep(mean_desc(1, 8405024, 1, 1, **half))[0] == amd.OK and prep(mean_desc(1, 2, 4202512, 1, **half))[0] == amd.OK
    rc, msg, _, _ = prep(mean_desc(1, 8405025, 1, 1, **half))
    assert rc == amd.ERR_UNSUPPORTED and "8405025" in msg
    # equal scales: the multiplier 1 = 2^30 x 2^(1 - 31) has e = 1, a left shift of one: 510 n + n / 2 <= 2^31 - 1 up to n = 4206628
    assert H.mean_multiplier(0.5, 0.5) == (1 << 30, 1) and H.mean_bound_ok(4206628, 1) and not H.mean_bound_ok(4206629, 1)
    assert prep(mean_desc(1, 4206628, 1, 1))[0] == amd.OK and prep(mean_desc(1, 4206629, 1, 1))[0] == amd.ERR_UNSUPPORTED
    assert prep(mean_desc(1, 46341, 46341, 1))[0] == amd.ERR_UNSUPPORTED                # n beyond int32
    # a left shift: si / so = 1.5 x 2^10 has e = 11: 255 x 49 x 2^11 = 25589760 passes; si / so = 1.5 x 2^17 (e = 18) does not
    assert H.mean_multiplier(1536.0, 1.0)[1] == 11 and prep(mean_desc(1, 7, 7, 1, (1536.0, 0), (1.0, 0)))[0] == amd.OK
    assert H.mean_multiplier(196608.0, 1.0)[1] == 18 and not H.mean_bound_ok(49, 18)
    rc, msg, _, _ = prep(mean_desc(1, 7, 7, 1, (196608.0, 0), (1.0, 0)))
    assert rc == amd.ERR_UNSUPPORTED and "e = 18" in msg
    # the exact edge at e = 17 (a multiplier in [2^16, 2^17)): 255 n 2^17 + n / 2 <= 2^31 - 1 up to n = 64
    assert H.mean_bound_ok(64, 17) and not H.mean_bound_ok(65, 17) and H.mean_multiplier(98304.0, 1.0)[1] == 17
    assert prep(mean_desc(1, 8, 8, 1, (98304.0, 0), (1.0, 0)))[0] == amd.OK
    assert prep(mean_desc(1, 5, 13, 1, (98304.0, 0), (1.0, 0)))[0] == amd.ERR_UNSUPPORTED
    assert prep(mean_desc(1, 1, 1, 1, (1e30, 0), (1e-30, 0)))[0] == amd.ERR_UNSUPPORTED  # an exponent beyond any shift
    for d, text in ((mean_desc(batch=0), "extents must be positive"), (mean_desc(h=0), "extents"), (mean_desc(c=-3), "extents"),
                    (mean_desc(q_in=(0.0, 0)), "input_scale must be finite and positive"), (mean_desc(q_out=(float("nan"), 0)), "output_scale"),
                    (mean_desc(q_in=(0.5, -129)), "input_zero_point must be in"), (mean_desc(q_out=(0.5, 128)), "output_zero_point must be in")):
        assert lib.lce_hip_mean_i8_check(C.byref(d)) == amd.ERR_INVALID and text in last(), last()
        assert prep(d)[0] == amd.ERR_INVALID
    assert lib.lce_hip_mean_i8_check(None) == amd.ERR_INVALID and lib.lce_hip_mean_i8_prepare(C.byref(mean_desc()), None, C.byref(e)) == amd.ERR_INVALID
    assert lib.lce_hip_mean_i8_check(C.byref(mean_desc(2 ** 31 - 1, 2 ** 15, 2 ** 15, 2 ** 10))) == amd.ERR_UNSUPPORTED and "2^60" in last()


def test_the_softmax_check():
    lib = amd.lib()
    chk = lambda rows=4, cols=10, si=0.1, beta=1.0, so=1.0 / 256.0, zo=-128: (lib.lce_hip_softmax_i8_check(rows, cols, si, beta, so, zo), last())
    assert chk()[0] == amd.OK
    for kw, msg in ((dict(rows=0), "rows and cols must be positive"), (dict(cols=0), "rows and cols"), (dict(si=0.0), "input_scale must be finite and positive"),
                    (dict(si=float("inf")), "input_scale"), (dict(beta=-1.0), "beta must be finite and positive"), (dict(beta=float("nan")), "beta"),
                    (dict(so=0.0), "output_scale must be finite and positive"), (dict(zo=-129), "output_zero_point must be in"), (dict(zo=128), "output_zero_point")):
        rc, text = chk(**kw)
        assert rc == amd.ERR_INVALID and msg in text, (kw, text)
    for kw in (dict(so=1.0 / 128.0), dict(zo=0), dict(so=float(np.nextafter(np.float32(1.0 / 256.0), np.float32(1)))), dict(zo=-127)):
        rc, text = chk(**kw)
        assert rc == amd.ERR_UNSUPPORTED and "exactly (1/256, -128)" in text, (kw, text)
    assert chk(cols=2 ** 31)[0] == amd.ERR_UNSUPPORTED and chk(rows=2 ** 40, cols=2 ** 21)[0] == amd.ERR_UNSUPPORTED
    assert chk(rows=2 ** 40, cols=2 ** 20)[0] == amd.OK


def test_the_run_entries_refuse_before_any_device_call():
    """The checks on pointers, overlap and alignment come before the device is asked for: made-up addresses never reach it."""
    lib = amd.lib()
    p = lambda v: None if v is None else C.c_void_p(v)
    d = fc_desc(batch=16, inputs=64, outputs=32)                    # in: 1024 B, weights: 2048 B, table: 384 B, out: 512 B

    def fc(x=1 << 20, w=2 << 20, t=3 << 20, o=4 << 20, dd=d):
        return lib.lce_hip_fully_connected_i8(C.byref(dd) if dd is not None else None, p(x), p(w), p(t), p(o), None), last()
    for kw, msg in ((dict(dd=None), "null desc"), (dict(x=None), "null input"), (dict(w=None), "null weights"), (dict(t=None), "null table"),
                    (dict(o=None), "null output"), (dict(o=(1 << 20) + 1023), "an output overlaps the input"),
                    (dict(o=(2 << 20) - 511), "an output overlaps the filter"), (dict(o=(3 << 20) + 383), "the output overlaps the table"),
                    (dict(t=(3 << 20) + 2), "table_dev must be 4-byte aligned"), (dict(dd=fc_desc(q_in=(0.5, 300))), "input_zero_point"),
                    (dict(dd=fc_desc(q_out=(0.0, 0))), "output_scale"), (dict(dd=fc_desc(act=7)), "unknown activation")):
        rc, text = fc(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_fully_connected_i8:"), (kw, text)
    rc, text = fc(dd=fc_desc(inputs=65794))
    assert rc == amd.ERR_UNSUPPORTED and "65794" in text
    md = mean_desc(2, 7, 7, 8)                                      # in: 784 B, out: 16 B

    def mean(x=1 << 20, o=2 << 20, dd=md):
        return lib.lce_hip_mean_i8(C.byref(dd) if dd is not None else None, p(x), p(o), None), last()
    for kw, msg in ((dict(dd=None), "null desc"), (dict(x=None), "null input"), (dict(o=None), "null output"),
                    (dict(o=(1 << 20) + 783), "the output overlaps the input"), (dict(o=(1 << 20) - 15), "overlaps"),
                    (dict(dd=mean_desc(q_in=(0.5, 128))), "input_zero_point"), (dict(dd=mean_desc(q_out=(-1.0, 0))), "output_scale")):
        rc, text = mean(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_mean_i8:"), (kw, text)
    assert mean(dd=mean_desc(1, 4206629, 1, 1))[0] == amd.ERR_UNSUPPORTED

    def softmax(x=1 << 20, o=2 << 20, rows=4, cols=10, si=0.1, beta=1.0, so=1.0 / 256.0, zo=-128):
        return lib.lce_hip_softmax_i8(rows, cols, si, beta, so, zo, p(x), p(o), None), last()
    for kw, msg in ((dict(x=None), "null input"), (dict(o=None), "null output"), (dict(o=(1 << 20) + 39), "partly overlaps"),
                    (dict(o=(1 << 20) + 1), "partly overlaps"), (dict(si=0.0), "input_scale"), (dict(beta=0.0), "beta"), (dict(zo=200), "output_zero_point")):
        rc, text = softmax(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_softmax_i8:"), (kw, text)
    assert softmax(so=0.5)[0] == amd.ERR_UNSUPPORTED

    def quant(entry, n=100, scale=0.5, zp=0, x=1 << 20, o=2 << 20):
        return getattr(lib, entry)(n, scale, zp, p(x), p(o), None), last()
    for entry, fbytes in (("lce_hip_quantize_f32_i8", "x"), ("lce_hip_dequantize_i8_f32", "o")):
        for kw, msg in ((dict(x=None), "null input"), (dict(o=None), "null output"), (dict(scale=0.0), "scale must be finite and positive"),
                        (dict(scale=float("nan")), "scale"), (dict(zp=128), "zero_point must be in"), (dict(zp=-129), "zero_point"),
                        ({fbytes: (3 << 20) + 2}, "float pointer must be 4-byte aligned"),
                        (dict(o=(1 << 20) + (396 if fbytes == "x" else 96)), "the output overlaps the input")):
            rc, text = quant(entry, **kw)
            assert rc == amd.ERR_INVALID and msg in text and text.startswith(entry + ":"), (entry, kw, text)
        assert quant(entry, n=2 ** 61)[0] == amd.ERR_UNSUPPORTED
        assert quant(entry, n=0)[0] == amd.OK                        # nothing to do: no device is asked for
    # the int8 operands need no alignment: odd addresses pass every host check.  Only where there is no device to launch on: there
    # the call ends at the device query (made-up addresses must never reach a kernel)
    if amd.device_count() == 0:
        assert fc(x=(1 << 20) + 1, w=(2 << 20) + 3, o=(4 << 20) + 5)[0] == amd.ERR_NO_DEVICE
        assert mean(x=(1 << 20) + 1, o=(2 << 20) + 3)[0] == amd.ERR_NO_DEVICE
        assert softmax(x=(1 << 20) + 1, o=(2 << 20) + 3)[0] == amd.ERR_NO_DEVICE and softmax(o=1 << 20)[0] == amd.ERR_NO_DEVICE   # in place
        assert quant("lce_hip_quantize_f32_i8", o=(2 << 20) + 1)[0] == amd.ERR_NO_DEVICE
        assert quant("lce_hip_dequantize_i8_f32", x=(1 << 20) + 1)[0] == amd.ERR_NO_DEVICE


def test_python_checks_fail_before_any_device_call():
    x, w, t = np.zeros((2, 8), np.int8), np.zeros((4, 8), np.int8), np.zeros((3, 4), np.int32)
    q = ((0.5, 0), (0.5, 0))
    for args, kw, msg in (((x.astype(np.float32), w, t, *q), {}, "x must be a non-empty int8"), ((x, w.astype(np.float32), t, *q), {}, "w must be int8"),
                          ((x, w[:, :7], t, *q), {}, "w must be int8"), ((x, w, t[:2], *q), {}, "table must be int32"),
                          ((x, w, t, (0.5,), q[1]), {}, "q_in must be"), ((x, w, t, q[0], (0.5, 300)), {}, "zero point"),
                          ((x, w, t, *q), dict(activation=7), "activation"), ((x, w, t, *q), dict(out=np.zeros((2, 4), np.float32)), "out must be int8")):
        with pytest.raises(ValueError, match=msg):
            amd.fully_connected_i8(*args, **kw)
    with pytest.raises(ValueError, match="bias must be int32"):
        amd.fully_connected_i8_prepare(w, np.zeros(4, np.float32), 0.5, *q)
    with pytest.raises(ValueError, match="weight_scales"):
        amd.fully_connected_i8_prepare(w, None, [0.5, 0.5], *q)
    with pytest.raises(ValueError, match="int8 NHWC"):
        amd.mean_i8(np.zeros((2, 8), np.int8), *q)
    with pytest.raises(ValueError, match="non-empty int8"):
        amd.softmax_i8(np.zeros((2, 8), np.float32), 0.1)
    with pytest.raises(amd.LceHipError, match="exactly"):
        amd.softmax_i8(np.zeros((2, 8), np.int8), 0.1, q_out=(0.5, 0))
    with pytest.raises(ValueError, match="float32"):
        amd.quantize_i8(np.zeros(4, np.int8), (0.5, 0))
    with pytest.raises(ValueError, match="int8"):
        amd.dequantize_i8(np.zeros(4, np.float32), (0.5, 0))
    with pytest.raises(ValueError, match="scale must be finite"):
        amd.quantize_i8(np.zeros(4, np.float32), (0.0, 0))


def test_the_abi_grew_by_ten_symbols_and_keeps_its_version():
    assert amd.lib().lce_hip_abi_version() == 3
    names = ("lce_hip_fully_connected_i8", "lce_hip_fully_connected_i8_check", "lce_hip_fully_connected_i8_prepare", "lce_hip_mean_i8",
             "lce_hip_mean_i8_check", "lce_hip_mean_i8_prepare", "lce_hip_softmax_i8", "lce_hip_softmax_i8_check", "lce_hip_quantize_f32_i8",
             "lce_hip_dequantize_i8_f32")
    for name in names:
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_head_i8_stats") and hasattr(mr.tflite_lib(), "lce_tflite_model_quantize_stats")


# ---- the partitions ---------------------------------------------------------------------------------------------------------------------
def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


@pytest.mark.parametrize("name", sorted(HM.FIXTURES))
def test_each_fixture_is_one_section_with_every_name(name):
    data, x, out, info = HM.FIXTURES[name]()
    one = mr.LceModel(data, **HM.EVERY_FLAG)
    assert parts(one) == [(list(range(info["ops"])), [x], [out])]
    it = mr.Interpreter(data, **HM.EVERY_FLAG)
    assert it.lce_only and len(it.sections) == 1
    assert it.input_types == [info["in_dtype"]] and it.output_types == [info["out_dtype"]]
    dims, nbytes = one.section_tensor_shape(0, out, 3)
    classes = info["head"]["classes"]
    assert dims == (3, 1, 1, classes) and nbytes == 3 * classes * (4 if info["out_dtype"] == np.float32 else 1)
    assert one.head_i8_stats() == (0, 0, 0) and one.quantize_stats() == (0, 0)              # nothing has run
    # without the two names nothing of the head or the boundary joins: the partition of the parent
    parent = mr.LceModel(data, **M.ALL_FLAGS)
    new = {info["head"][k] for k in ("mean", "fc", "softmax", "dequantize") if info["head"][k] is not None}
    assert not any(set(ops) & new for ops, _, _ in parts(parent)) and not mr.Interpreter(parent).lce_only
    # the names one at a time
    only_head = parts(mr.LceModel(data, head_i8_sections=True, **M.ALL_FLAGS))
    assert [info["head"][k] for k in ("mean", "fc", "softmax")] == only_head[-1][0][-3:]
    only_quant = parts(mr.LceModel(data, quantize_sections=True, **M.ALL_FLAGS))
    assert not any(info["head"]["mean"] in ops for ops, _, _ in only_quant)


def test_the_head_alone_needs_no_lce_operator_and_no_stem_flag():
    data, x, out, info = HM.head_only_fixture()
    assert parts(mr.LceModel(data, head_i8_sections=True, quantize_sections=True)) == [([0, 1, 2, 3], [x], [out])]
    assert parts(mr.LceModel(data, head_i8_sections=True)) == [([0, 1, 2], [x], [info["head"]["tensors"]["probs"]])]
    assert parts(mr.LceModel(data)) == [] and parts(mr.LceModel(data, quantize_sections=True)) == []
    # a QUANTIZE at the graph's input joins under `stem`, as any enabled opt-in does
    data, x, out, info = HM.network_fixture()
    no_stem = {k: v for k, v in HM.EVERY_FLAG.items() if k != "stem_sections"}
    assert parts(mr.LceModel(data, **no_stem))[0][0] == [2, 3, 4, 5, 6, 7]
    lib, err = mr.tflite_lib(), C.create_string_buffer(256)
    h = lib.lce_tflite_model_open_passes(data, len(data), b"quantize,head_i8,conv2d_i8,stem", err, 256)
    assert h and lib.lce_tflite_model_num_sections(h) == 1
    lib.lce_tflite_model_close(h)
    assert not lib.lce_tflite_model_open_passes(data, len(data), b"head_i8,stem,head_i8", err, 256) and b"'head_i8' is named twice" in err.value
    assert not lib.lce_tflite_model_open_passes(data, len(data), b"quantise", err, 256) and b"unknown name 'quantise'" in err.value


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_without_the_names_the_int8_fixtures_partition_as_the_parent_did(name):
    data, x, out, info = M.FIXTURES[name]()
    assert [s.ops for s in mr.LceModel(data).sections] == info["plain"]
    assert [s.ops for s in mr.LceModel(data, **info["parent_flags"]).sections] == info["parent_sections"]
    assert [s.ops for s in mr.LceModel(data, **M.ALL_FLAGS).sections] == [list(range(info["ops"]))]
    # ... and with them too: these files have no head and no boundary operator
    for flags in ({}, info["parent_flags"], M.ALL_FLAGS):
        assert parts(mr.LceModel(data, head_i8_sections=True, quantize_sections=True, **flags)) == parts(mr.LceModel(data, **flags))


@pytest.mark.parametrize("name", ["quicknet_head", "quicknet_head_keep_dims", "head_only"] + sorted(NO_HEAD))
def test_the_names_move_nothing_on_a_float_file(name):
    """No new predicate takes a float MEAN / FULLY_CONNECTED / SOFTMAX, and no float file here has a QUANTIZE / DEQUANTIZE."""
    data = {"quicknet_head": lambda: FHM.quicknet_head_model(), "quicknet_head_keep_dims": lambda: FHM.quicknet_head_model(keep_dims=True),
            "head_only": lambda: FHM.head_only_model(), **NO_HEAD}[name]()[0]
    for flags in ({}, dict(head_sections=True), dict(int8_add_sections=True, concat_sections=True, **FHM.ALL_FLAGS),
                  dict(int8_add_sections=True, concat_sections=True, conv2d_i8_sections=True, **FHM.EVERY_FLAG)):
        without = mr.LceModel(data, **flags)
        with_names = mr.LceModel(data, head_i8_sections=True, quantize_sections=True, **flags)
        assert parts(with_names) == parts(without)
        assert mr.Interpreter(with_names).lce_only == mr.Interpreter(without).lce_only
    if name == "quicknet_head":
        n = len(mr.LceModel(data).operators)
        assert [s.ops for s in mr.LceModel(data, **FHM.EVERY_FLAG).sections] == [list(range(n))]       # the parent's one section


def _violation(case):
    """The head-alone fixture with one rule broken; returns (file, the operator that must stay with the host, the head's info)."""
    kw = {}
    if case == "softmax_output_scale":
        kw["q_probs"] = (1.0 / 128.0, -128)
    if case == "softmax_output_zero_point":
        kw["q_probs"] = (1.0 / 256.0, 0)
    if case == "weight_zero_point":
        kw["weight_zero_points"] = [0, 0, 1, 0, 0, 0, 0]
    data, x, out, info = HM.head_only_fixture(**kw)
    return data, info["head"]["softmax" if case.startswith("softmax") else "fc"], info["head"]


@pytest.mark.parametrize("case", ["softmax_output_scale", "softmax_output_zero_point", "weight_zero_point"])
def test_a_candidate_that_fails_stays_with_the_host(case):
    data, k, hi = _violation(case)
    model = mr.LceModel(data, **HM.EVERY_FLAG)
    assert not any(k in s.ops for s in model.sections) and not mr.Interpreter(model).lce_only
    assert any(hi["mean"] in s.ops for s in model.sections)                                   # the rest still joins


def test_a_hybrid_or_malformed_fully_connected_stays_with_the_host():
    """float input with int8 weights (hybrid), per-channel scales along the wrong dimension, a float bias, shuffled weights, a bias
    beyond the accumulator bound: none joins; the plain operator does."""
    def build(case):
        b = M.QModelBuilder()
        q_x, q_y = (0.05, -4), (0.04, 3)
        x = b.tensor([1, 16], np.float32 if case == "hybrid" else np.int8, "x", **({} if case == "hybrid" else dict(scale=q_x[0], zero_point=q_x[1])))
        w = np.ones((4, 16), np.int8)
        sw = [0.01] * 4
        wt = b.qtensor(w.shape, np.int8, "w", w, sw, [0] * 4, 1 if case == "quantized_dimension_1" else 0)
        bias = np.array([0, 2 ** 31 - 1, 0, 0] if case == "bias_overflow" else [1, 2, 3, 4], np.int32)
        bt = b.tensor([4], np.float32, "b", bias.astype(np.float32)) if case == "float_bias" else b.tensor([4], np.int32, "b", bias)
        y = b.tensor([1, 4], np.float32 if case == "hybrid" else np.int8, "y", **({} if case == "hybrid" else dict(scale=q_y[0], zero_point=q_y[1])))
        k = fc_op(b, [x, wt, bt], [y], weights_format=1 if case == "shuffled" else 0, options=case != "no_options")
        p = b.tensor([1, 4], np.int8, "p", scale=1.0 / 256.0, zero_point=-128)
        if case != "hybrid":
            softmax_op(b, [y], [p])
        b.inputs, b.outputs = [x], [y if case == "hybrid" else p]
        return b.finish(), k
    data, k = build("plain")
    assert [s.ops for s in mr.LceModel(data, head_i8_sections=True).sections] == [[0, 1]]
    for case in ("hybrid", "quantized_dimension_1", "float_bias", "shuffled", "no_options", "bias_overflow"):
        data, k = build(case)
        for flags in (dict(head_i8_sections=True), dict(head_i8_sections=True, head_sections=True, quantize_sections=True, stem_sections=True)):
            assert not any(k in s.ops for s in mr.LceModel(data, **flags).sections), case


def test_a_requantizing_quantize_and_other_types_stay_with_the_host():
    b = M.QModelBuilder()
    x = b.tensor([1, 4, 4, 8], np.int8, "x", scale=0.05, zero_point=-4)
    y = b.tensor([1, 4, 4, 8], np.int8, "y", scale=0.1, zero_point=3)
    k_rq = b.builtin_op(HM.QUANTIZE, [x], [y])                                               # int8 -> int8: a requantization
    z = b.tensor([1, 4, 4, 8], np.float32, "z")
    k_dq = b.builtin_op(HM.DEQUANTIZE, [y], [z])
    z2 = b.tensor([1, 4, 4, 8], np.int8, "z2", scale=0.1, zero_point=200)                    # a zero point that is no int8
    k_bad = b.builtin_op(HM.QUANTIZE, [z], [z2])
    b.inputs, b.outputs = [x], [z2]
    model = mr.LceModel(b.finish(), quantize_sections=True, stem_sections=True, head_i8_sections=True)
    assert [s.ops for s in model.sections] == [] or not any(k in s.ops for s in model.sections for k in (k_rq, k_bad))
