"""The quantized DEPTHWISE_CONV_2D inside the sections (lce_hip_depthwise_conv2d_i8, "depthwise_i8" of
lce_tflite_model_open_passes) on the CPU: the NumPy restatement (tests/depthwise_i8_ref.py) against a float64 sum and against known
answers worked by hand; the grid's operands against the spread they promise; lce_hip_depthwise_conv2d_i8_prepare's table against
the restatement, every refusal of the entries with its message, and the overflow bounds at their edges; and the partitions of the
fixtures of tests/depthwise_i8_models.py with and without the new name."""
import ctypes as C
import importlib

import numpy as np
import pytest

import depthwise_i8_models as DM
import depthwise_i8_ref as R
import head_i8_models as HM
import int8_conv_models as M
import section_models as SM
from depthwise_i8_cases import GRID, KNOWN, expect_vec, operands, run_grid
from section_models import NONE, SAME, depthwise_op
from test_head_sections_host import NO_HEAD

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,cin,m", GRID)
def test_the_accumulation_equals_a_float64_sum_over_the_zero_padded_image(filt, cin, m):
    n = 0
    for image, stride, padding, zi in (((5, 7), (1, 1), R.SAME, 5), ((9, 8), (2, 2), R.SAME, -128), ((9, 8), (4, 3), R.VALID, 127),
                                       ((1, 1), (1, 1), R.SAME, -3)):
        if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
            continue
        x, w, _, _, _, _ = operands((2, *image, cin), filt, m, 31 * cin + image[0], zi, stride=stride, padding=padding)
        acc = R.accumulate(x, w, zi, stride, padding, m)
        ref = R.accumulate_float64(x, w, zi, stride, padding, m)
        assert acc.shape == ref.shape and np.abs(ref).max() < 2.0 ** 53 and np.array_equal(acc.astype(np.float64), ref)
        n += 1
    assert n >= 3


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_restatement_gives_the_known_answers(name):
    k = KNOWN[name]
    got = R.depthwise_i8(k["x"], k["w"], k["bias"], k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], k["m"], k["act"])
    assert got.dtype == np.int8 and np.array_equal(got, k["want"]), (got, k["want"])


def test_the_known_answers_cover_what_they_claim():
    m = lambda k: R.multipliers(k["q_in"][0], k["sw"], k["q_out"][0], 1)
    assert m(KNOWN["ties"]) == ([1 << 30], [-1]) and m(KNOWN["e_positive"]) == ([1 << 30], [2]) and m(KNOWN["multiplier_2"]) == ([1 << 30], [1])
    assert m(KNOWN["zi_minus_128"]) == ([1 << 30], [-7]) and m(KNOWN["zi_127"]) == ([1 << 30], [-9])
    assert KNOWN["zi_minus_128"]["q_in"][1] == -128 and KNOWN["zi_127"]["q_in"][1] == 127
    assert KNOWN["zi_minus_128"]["want"].min() == -128 and KNOWN["zi_minus_128"]["want"].max() == 127 and KNOWN["zi_127"]["want"].max() == 127
    assert {k["m"] for k in KNOWN.values()} == {1, 2, 3} and {"activation_%d" % a for a in range(4)} <= set(KNOWN)
    # the skipped taps of the corner: read as x = 0 they would change the answer
    for name in ("corner_same_pad", "corner_two_channels"):
        k = KNOWN[name]
        zero_padded = np.zeros((1, 4, 4, k["x"].shape[3]), np.int8)
        zero_padded[:, 1:3, 1:3] = k["x"]
        wrong = R.depthwise_i8(zero_padded, k["w"], None, k["sw"], k["q_in"], k["q_out"], 1, R.VALID)
        assert wrong.shape == k["want"].shape and not np.array_equal(wrong[..., 0], k["want"][..., 0])
    # a channel that read its neighbour's input or weights would show in the two-channel corner and in the mappings
    k = KNOWN["multiplier_3"]
    assert not np.array_equal(R.depthwise_i8(k["x"][..., ::-1], k["w"], None, k["sw"], k["q_in"], k["q_out"], 1, R.VALID, 3), k["want"])


def test_the_reference_meets_the_grids_assertions_on_every_case():
    """run_grid on the reference itself: every case with at least 64 output elements holds 16 distinct values or more and fewer
    than half of its bytes on a clamp bound (spread_check), so a kernel that writes a constant cannot pass the grid; and the
    rotations reach every input zero point, activation, output combination, scale kind and placement."""
    seen = set()

    def run(x, w, b, sw, q_in, q_out, stride, padding, m, act, want_out=True, want_bits=True, offset=0, path=None):
        want = R.depthwise_i8(x, w, b, sw, q_in, q_out, stride, padding, m, act)
        seen.add((q_in[1], act, b is None, want_out, want_bits, offset, np.atleast_1d(sw).size > 1 or w.shape[-1] == 1))
        vec = path is None and expect_vec(w.shape[-1], m, offset, want_out, want_bits)
        return (want if want_out else None), (R.bitpack(want, q_out[1]) if want_bits else None), vec
    total = 0
    for filt, cin, m in GRID:
        n, vecs = run_grid(run, filt, cin, m)
        assert n >= 9 and (vecs > 0) == (m == 1 and cin % 16 == 0)
        total += n
    assert total == 630
    assert {s[0] for s in seen} == {0, -128, 127, 5, -3} and {s[1] for s in seen} == {0, 1, 2, 3} and {s[2] for s in seen} == {False, True}
    assert {s[3:5] for s in seen} == {(True, True), (False, True), (True, False)} and {s[5] for s in seen} == {0, 1}
    assert {s[6] for s in seen} == {False, True}


# ---- prepare ------------------------------------------------------------------------------------------------------------------------
def desc(cin=4, m=1, filt=(3, 3), image=(9, 9), stride=(1, 1), padding=amd.PADDING_SAME, act=amd.ACT_NONE, q_in=(0.5, 0), q_out=(0.5, 0), batch=1):
    return amd.DepthwiseI8Desc(batch, image[0], image[1], cin, m, filt[0], filt[1], stride[0], stride[1], padding, act, q_in[0], q_in[1],
                               q_out[0], q_out[1])


def c_prepare(d, w, bias, sw):
    """(status, message, table, act_min, act_max) of lce_hip_depthwise_conv2d_i8_prepare on NumPy constants."""
    cout = d.channels_in * d.depth_multiplier
    table = np.zeros((3, cout), np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    sw = np.ascontiguousarray(np.atleast_1d(sw), np.float32)
    rc = amd.lib().lce_hip_depthwise_conv2d_i8_prepare(C.byref(d), w.ctypes.data, None if bias is None else bias.ctypes.data, sw.ctypes.data,
                                                       sw.size, table.ctypes.data, C.byref(lo), C.byref(hi))
    return rc, amd.lib().lce_hip_last_error().decode(), table, lo.value, hi.value


def test_prepare_equals_the_restatement_on_random_constants():
    g = np.random.default_rng(11)
    oks = 0
    for n in range(60):
        filt, cin, m = (int(g.integers(1, 8)), int(g.integers(1, 8))), int(g.integers(1, 40)), int(g.integers(1, 4))
        cout = cin * m
        zi, zo, act = int(g.integers(-128, 128)), int(g.integers(-128, 128)), int(g.integers(0, 4))
        si, so = (float(np.float32(np.exp(g.uniform(np.log(1e-3), np.log(1.0))))) for _ in range(2))
        w = g.integers(-128, 128, (1, *filt, cout), dtype=np.int64).astype(np.int8)
        bias = None if n % 3 == 0 else g.integers(-(1 << 20), 1 << 20, cout, dtype=np.int64).astype(np.int32)
        sw = np.exp(g.uniform(np.log(1e-4), np.log(0.5), cout if n % 2 else 1)).astype(np.float32)
        d = desc(cin, m, filt, (9, 9), q_in=(si, zi), q_out=(so, zo), act=act)
        rc, msg, table, lo, hi = c_prepare(d, w, bias, sw)
        try:
            want = R.table(w, bias, sw, si, so)
        except ValueError:
            assert rc == amd.ERR_UNSUPPORTED and "channel" in msg, msg
            continue
        assert rc == amd.OK, msg
        assert np.array_equal(table, want) and (lo, hi) == R.activation_range(act, so, zo)
        assert np.array_equal(table[0], np.zeros(cout, np.int32) if bias is None else bias)          # row 0 is the bias itself
        py = amd.depthwise_conv2d_i8_prepare(w, bias, sw, (si, zi), (so, zo), m, act)
        assert np.array_equal(py[0], want) and py[1:] == (lo, hi)
        oks += 1
    assert oks >= 40


def test_the_table_is_the_one_the_convolutions_prepare_makes_of_the_same_multipliers():
    """QuantizeMultiplier and the activation range are the routine lce_hip_conv2d_i8_prepare runs: on a one-channel filter with
    zi = 0 (nothing to fold) the two tables are the same bytes."""
    g = np.random.default_rng(5)
    for _ in range(20):
        si, so, sw = (float(np.float32(np.exp(g.uniform(np.log(1e-3), np.log(1.0))))) for _ in range(3))
        w = g.integers(-128, 128, (1, 3, 3, 1), dtype=np.int64).astype(np.int8)
        bias = g.integers(-1000, 1000, 1, dtype=np.int64).astype(np.int32)
        a = amd.depthwise_conv2d_i8_prepare(w, bias, sw, (si, 0), (so, 3), 1, amd.ACT_RELU6)
        b = amd.conv2d_i8_prepare(w, bias, sw, (si, 0), (so, 3), amd.ACT_RELU6)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_the_overflow_bounds_at_their_edges():
    """255 x 128 x K + B against 2^31 - 1 with K = fh x fw: K = 65793 = 241 x 273 passes without a bias (2147483520) and with
    |bias| = 127, fails with 128, naming the channel; K = 65794 = 2 x 67 x 491 fails.  The channel count does not enter: K is
    the taps of ONE channel."""
    assert 241 * 273 == 65793 and 134 * 491 == 65794 and 255 * 128 * 65793 + 127 == 2 ** 31 - 1 and 255 * 128 * 65794 > 2 ** 31 - 1
    for filt, bias, ok in (((241, 273), None, True), ((241, 273), [5, -127], True), ((241, 273), [5, -128], False), ((134, 491), None, False)):
        w = np.ones((1, *filt, 2), np.int8)
        b = None if bias is None else np.array(bias, np.int32)
        rc, msg, table, _, _ = c_prepare(desc(2, 1, filt, filt, padding=amd.PADDING_VALID), w, b, 2.0 ** -20)
        if ok:
            assert rc == amd.OK and table[0].tolist() == ([0, 0] if b is None else bias), msg
        else:
            assert rc == amd.ERR_UNSUPPORTED and msg.startswith("lce_hip_depthwise_conv2d_i8_prepare") and "exceeds 2^31 - 1" in msg, msg
            assert "channel %d" % (1 if bias else 0) in msg, msg
    # many channels of few taps are far inside: 3 x 3 x 65794 channels
    assert c_prepare(desc(65794, 1, (3, 3), (3, 3)), np.ones((1, 3, 3, 65794), np.int8), None, 2.0 ** -20)[0] == amd.OK
    # a left shift: K = 1, bound 32640; multiplier 0.75 x 2^17 has e = 17: 32640 x 2^17 > 2^31 - 1, while e = 16 passes
    w = np.ones((1, 1, 1, 3), np.int8)
    rc, msg, _, _, _ = c_prepare(desc(3, 1, (1, 1), (1, 1), q_in=(1.0, 0), q_out=(1.0, 0)), w, None, [1.0, 0.75 * 2.0 ** 17, 1.0])
    assert rc == amd.ERR_UNSUPPORTED and "channel 1" in msg and "2^17" in msg, msg
    assert c_prepare(desc(3, 1, (1, 1), (1, 1), q_in=(1.0, 0), q_out=(1.0, 0)), w, None, [1.0, 0.75 * 2.0 ** 16, 1.0])[0] == amd.OK
    # ... and with a bias just inside and just outside: (32640 + B) x 2^16 <= 2^31 - 1 needs B <= 127
    assert (32640 + 127) << 16 <= 2 ** 31 - 1 < (32640 + 128) << 16
    for B, want in ((127, amd.OK), (128, amd.ERR_UNSUPPORTED)):
        rc, msg, _, _, _ = c_prepare(desc(3, 1, (1, 1), (1, 1), q_in=(1.0, 0), q_out=(1.0, 0)), w, np.array([0, 0, -B], np.int32),
                                     [1.0, 0.75 * 2.0 ** 16, 1.0])
        assert rc == want and (want == amd.OK or "channel 1" in msg), msg


BAD_DESCS = ((dict(q_in=(0.0, 0)), "input_scale must be finite and positive"), (dict(q_in=(float("inf"), 0)), "input_scale must be finite and positive"),
             (dict(q_out=(float("nan"), 0)), "output_scale must be finite and positive"), (dict(q_out=(-1.0, 0)), "output_scale must be finite and positive"),
             (dict(q_in=(0.5, 128)), "input_zero_point must be in"), (dict(q_out=(0.5, -129)), "output_zero_point must be in"),
             (dict(cin=0), "extents must be positive"), (dict(batch=0), "extents must be positive"), (dict(m=0), "the depth multiplier must be positive"),
             (dict(filt=(0, 3)), "the filter must be positive"), (dict(stride=(1, 0)), "the stride must be positive"),
             (dict(padding=2), "padding must be SAME or VALID"), (dict(act=4), "unknown activation"),
             (dict(filt=(10, 10), padding=amd.PADDING_VALID), "empty output"))


def test_check_refuses_what_the_float_entry_refuses_and_bad_quantization():
    oh, ow = C.c_int32(), C.c_int32()
    lib = amd.lib()
    assert lib.lce_hip_depthwise_conv2d_i8_check(C.byref(desc(stride=(2, 2))), C.byref(oh), C.byref(ow)) == amd.OK and (oh.value, ow.value) == (5, 5)
    assert lib.lce_hip_depthwise_conv2d_i8_check(C.byref(desc()), None, None) == amd.OK
    assert lib.lce_hip_depthwise_conv2d_i8_check(None, None, None) == amd.ERR_INVALID and "null desc" in lib.lce_hip_last_error().decode()
    for kw, msg in BAD_DESCS:
        rc = lib.lce_hip_depthwise_conv2d_i8_check(C.byref(desc(**kw)), C.byref(oh), C.byref(ow))
        text = lib.lce_hip_last_error().decode()
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_depthwise_conv2d_i8:"), (kw, text)
        if "q_in" not in kw and "q_out" not in kw:                   # the float entry refuses the same geometry
            f = amd.DepthwiseDesc(*[getattr(desc(**kw), n) for n, _ in amd.DepthwiseDesc._fields_])
            assert lib.lce_hip_depthwise_conv2d_f32_check(C.byref(f), C.byref(oh), C.byref(ow)) == amd.ERR_INVALID
            assert msg in lib.lce_hip_last_error().decode()
    for kw, msg in ((dict(image=((1 << 30) + 1, 1), filt=(1, 1)), "above 2^30"), (dict(cin=1 << 28, filt=(3, 3)), "a filter of 2^31 or more elements"),
                    (dict(batch=1 << 16, image=(1 << 8, 1 << 8), filt=(1, 1)), "fewer than 2^31 pixels")):
        rc = lib.lce_hip_depthwise_conv2d_i8_check(C.byref(desc(**kw)), C.byref(oh), C.byref(ow))
        assert rc == amd.ERR_UNSUPPORTED and msg in lib.lce_hip_last_error().decode(), (kw, lib.lce_hip_last_error())
    assert C.sizeof(amd.DepthwiseDesc) == 44 and C.sizeof(amd.DepthwiseI8Desc) == 60       # the float struct keeps its size


def test_prepare_refuses_what_is_malformed():
    w, sw = np.ones((1, 3, 3, 4), np.int8), np.full(4, 0.5, np.float32)
    table, lo, hi = np.zeros((3, 4), np.int32), C.c_int32(), C.c_int32()
    good = dict(d=desc(), w=w.ctypes.data, b=None, s=sw.ctypes.data, n=4, t=table.ctypes.data, lo=C.byref(lo), hi=C.byref(hi))
    call = lambda **kw: (lambda a: (amd.lib().lce_hip_depthwise_conv2d_i8_prepare(C.byref(a["d"]) if a["d"] is not None else None, a["w"], a["b"],
                                                                                  a["s"], a["n"], a["t"], a["lo"], a["hi"]),
                                    amd.lib().lce_hip_last_error().decode()))({**good, **kw})
    assert call()[0] == amd.OK and call(n=1)[0] == amd.OK
    for kw, msg in ((dict(d=None), "null desc"), (dict(w=None), "null filter"), (dict(s=None), "null filter scales"), (dict(t=None), "null result"),
                    (dict(lo=None), "null result"), (dict(hi=None), "null result"), (dict(n=2), "2 scales"), (dict(n=0), "0 scales"),
                    (dict(d=desc(m=2), n=4), "4 scales")) + tuple((dict(d=desc(**kw)), msg) for kw, msg in BAD_DESCS):
        rc, text = call(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_depthwise_conv2d_i8_prepare"), (kw, text)
    for bad_value in (0.0, -0.5, float("inf"), float("nan")):
        bad = sw.copy()
        bad[2] = bad_value
        rc, text = call(s=bad.ctypes.data)
        assert rc == amd.ERR_INVALID and "channel 2" in text and "finite and positive" in text


def test_the_run_entries_refuse_before_any_device_call():
    """The checks on pointers, overlap and alignment come before the device is asked for: made-up addresses never reach it."""
    d = desc(cin=64, image=(8, 8), batch=2)                          # in: 8192 B, filter: 576 B, table: 768 B, out: 8192 B, bits: 1024 B
    lib = amd.lib()
    p = lambda v: None if v is None else C.c_void_p(v)
    took = C.c_int32(-1)

    def call(entry="", x=1 << 20, w=2 << 20, t=3 << 20, o=4 << 20, b=5 << 20, dd=d, path=None):
        args = [C.byref(dd) if dd is not None else None] + ([path] if entry == "_forced" else []) + [p(x), p(w), p(t), p(o), p(b)]
        args += [C.byref(took)] if entry == "_path" else [None]
        rc = getattr(lib, "lce_hip_depthwise_conv2d_i8" + entry)(*args)
        return rc, lib.lce_hip_last_error().decode()
    for entry, extra in (("", {}), ("_path", {}), ("_forced", dict(path=0))):
        for kw, msg in ((dict(dd=None), "null desc"), (dict(x=None), "null input"), (dict(w=None), "null filter"), (dict(t=None), "null table"),
                        (dict(o=None, b=None), "both outputs are null"), (dict(o=(1 << 20) + 8191), "an output overlaps the input"),
                        (dict(b=(2 << 20) + 572), "an output overlaps the filter"), (dict(o=(3 << 20) - 1), "an output overlaps the table"),
                        (dict(b=(4 << 20) + 8188), "the two outputs overlap"), (dict(b=(5 << 20) + 2), "out_bits_dev must be 4-byte aligned"),
                        (dict(t=(3 << 20) + 1), "table_dev must be 4-byte aligned"), (dict(dd=desc(q_in=(0.5, 300))), "input_zero_point"),
                        (dict(dd=desc(act=9)), "unknown activation")):
            rc, text = call(entry, **kw, **extra)
            assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_depthwise_conv2d_i8%s:" % entry), (entry, kw, text)
    # the path: 64 channels, everything 16-byte aligned -> the 16-byte path; a 1-byte offset of any of the four, a multiplier, a
    # ragged channel count, or bits on channels % 32 != 0 -> the row path.  Host only: nothing runs
    path_of = lambda **kw: (call("_path", **kw)[0], took.value)
    assert path_of() == (amd.OK, 1) and path_of(b=None) == (amd.OK, 1) and path_of(o=None) == (amd.OK, 1)
    for kw in (dict(x=(1 << 20) + 1), dict(w=(2 << 20) + 1), dict(o=(4 << 20) + 1), dict(t=(3 << 20) + 4), dict(dd=desc(cin=32, m=2, image=(8, 8), batch=2)),
               dict(dd=desc(cin=63, image=(8, 8), batch=2)), dict(dd=desc(cin=48, image=(8, 8), batch=2))):
        assert path_of(**kw) == (amd.OK, 0), kw
    assert path_of(dd=desc(cin=48, image=(8, 8), batch=2), b=None) == (amd.OK, 1)
    assert call("_path", x=1 << 20)[0] == amd.OK
    rc = lib.lce_hip_depthwise_conv2d_i8_path(C.byref(d), p(1 << 20), p(2 << 20), p(3 << 20), p(4 << 20), p(5 << 20), None)
    assert rc == amd.ERR_INVALID and "null path" in lib.lce_hip_last_error().decode()
    # forcing: an unknown path, and the 16-byte path where the operands do not qualify
    for path in (-1, 2):
        rc, text = call("_forced", path=path)
        assert rc == amd.ERR_INVALID and "unknown path" in text
    rc, text = call("_forced", path=1, x=(1 << 20) + 1)
    assert rc == amd.ERR_INVALID and "the 16-byte path needs" in text
    # the int8 operands need no alignment: odd addresses pass every host check.  Only where there is no device to launch on: there
    # the call ends at the device query (made-up addresses must never reach a kernel)
    if amd.device_count() == 0:
        rc, text = call(x=(1 << 20) + 1, w=(2 << 20) + 3, o=(4 << 20) + 5)
        assert rc == amd.ERR_NO_DEVICE, text


def test_python_checks_fail_before_any_device_call():
    x, w, t = np.zeros((1, 5, 5, 4), np.int8), np.zeros((1, 3, 3, 4), np.int8), np.zeros((3, 4), np.int32)
    q = ((0.5, 0), (0.5, 0))
    for args, kw, msg in (((x.astype(np.float32), w, t, *q), {}, "x must be a non-empty int8 NHWC"), ((x, w.astype(np.float32), t, *q), {}, "filter must be int8"),
                          ((x, w[..., :2], t, *q), {}, "filter must be int8"), ((x, np.zeros((2, 3, 3, 4), np.int8), t, *q), {}, "filter must be int8"),
                          ((x, w, t, *q), dict(depth_multiplier=2), "filter must be int8"), ((x, w, t, *q), dict(depth_multiplier=0), "depth_multiplier"),
                          ((x, w, t[:2], *q), {}, "table must be int32"), ((x, w, t, (0.5,), q[1]), {}, "q_in must be"),
                          ((x, w, t, (0.5, 200), q[1]), {}, "zero point"), ((x, w, t, q[0], (0.0, 0)), {}, "scale must be finite"),
                          ((x, w, t, *q), dict(stride=0), "stride"), ((x, w, t, *q), dict(padding=3), "padding"),
                          ((x, w, t, *q), dict(activation=7), "activation"), ((x, w, t, *q), dict(out=False), "no output requested"),
                          ((x, w, t, *q), dict(out=np.zeros((1, 5, 5, 4), np.float32)), "out must be int8"), ((x, w, t, *q), dict(path=2), "path must be")):
        with pytest.raises(ValueError, match=msg):
            amd.depthwise_conv2d_i8(*args, **kw)
    with pytest.raises(ValueError, match="bias must be int32"):
        amd.depthwise_conv2d_i8_prepare(w, np.zeros(4, np.float32), 0.5, *q)
    with pytest.raises(ValueError, match="filter_scales"):
        amd.depthwise_conv2d_i8_prepare(w, None, [0.5, 0.5], *q)
    with pytest.raises(ValueError, match="filter must be int8"):
        amd.depthwise_conv2d_i8_prepare(w, None, 0.5, *q, depth_multiplier=3)


def test_the_abi_grew_by_five_symbols_and_keeps_its_version():
    """Fails without the feature: none of the symbols exists there."""
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_depthwise_conv2d_i8", "lce_hip_depthwise_conv2d_i8_check", "lce_hip_depthwise_conv2d_i8_prepare",
                 "lce_hip_depthwise_conv2d_i8_path", "lce_hip_depthwise_conv2d_i8_forced"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_depthwise_i8_stats")
    assert "depthwise_i8_sections" in mr._NAMED_ONLY and mr._PASS_NAMES["depthwise_i8_sections"] == "depthwise_i8" and mr._PASS_STATS["depthwise_i8"] == 2


# ---- the partition --------------------------------------------------------------------------------------------------------------------
def ops(model):
    return [s.ops for s in model.sections]


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


@pytest.mark.parametrize("name", sorted(DM.FIXTURES))
def test_each_fixture_is_one_section_with_the_name_and_cut_at_the_depthwise_operators_without(name):
    data, x, out, info = DM.FIXTURES[name]()
    one = mr.LceModel(data, **DM.EVERY_FLAG)
    assert ops(one) == [list(range(info["ops"]))] and one.sections[0].inputs == [x] and one.sections[0].outputs == [out]
    it = mr.Interpreter(data, **DM.EVERY_FLAG)
    assert it.lce_only and len(it.sections) == 1
    # with every earlier name: the recorded parent partition, which no section of crosses a depthwise operator, and predict() refuses
    parent = mr.LceModel(data, **DM.EARLIER)
    assert ops(parent) == info["parent_sections"]
    covered = {k for s in ops(parent) for k in s}
    for k in info["depthwises"]:
        assert k not in covered and parent.operators[k].builtin_code == SM.DEPTHWISE_CONV_2D
        assert all(not (min(s) < k < max(s)) for s in ops(parent))
    assert not mr.Interpreter(data, **DM.EARLIER).lce_only
    if "plain" in info:
        assert ops(mr.LceModel(data)) == info["plain"]
    # every float opt-in leaves an int8 DEPTHWISE_CONV_2D with the host
    floats = dict(elementwise_sections=True, concat_sections=True, conv1x1_sections=True, depthwise_sections=True, conv2d_sections=True,
                  head_sections=True)
    assert ops(mr.LceModel(data, **floats, **DM.EARLIER)) == info["parent_sections"]
    # the per-channel file carries Cout scales along dimension 3, the per-tensor file one
    for k in info["depthwises"]:
        flt = one.tensors[one.operators[k].inputs[1]]
        assert flt.shape[0] == 1 and len(flt.scales) == (flt.shape[3] if name.endswith("per_channel") else 1)
        assert flt.quantized_dimension == 3
    # at another batch the section's shapes follow
    dims, nbytes = one.section_tensor_shape(0, out, 3)
    assert dims[0] == 3 and tuple(d for d in dims[1:] if d != 1) == tuple(d for d in one.tensors[out].shape[1:] if d != 1)   # (rank 2 is carried as [b, 1, 1, C])


def test_the_blur_of_the_fixture_is_the_quantized_one_two_one_filter():
    assert DM.BLUR_Q.tolist() == [[32, 64, 32], [64, 127, 64], [32, 64, 32]]
    assert np.abs(DM.BLUR_Q * DM.BLUR_SCALE - np.outer([1, 2, 1], [1, 2, 1]) / 16.0).max() <= DM.BLUR_SCALE / 2 + 1e-9
    # on a constant map the blur returns the constant (its taps sum to 511 x 0.25 / 127 = 1.006), also at the border, where the
    # padding taps are skipped and NOT renormalised: a corner of a 3x3 / 2 SAME blur on an even extent sees all nine taps or fewer
    x = np.full((1, 8, 8, 32), 30, np.int8)
    blur = np.broadcast_to(DM.BLUR_Q[None, :, :, None], (1, 3, 3, 32))
    y = R.depthwise_i8(x, blur, None, DM.BLUR_SCALE, (0.06, -20), (0.06, -20), (2, 2), R.SAME)
    assert y.shape == (1, 4, 4, 32) and (y[0, :3, :3] == 30).all() and (y[0, 3, 3] < 30).all()


def test_the_name_alone_needs_the_stem_flag_for_a_stem_and_an_lce_epoch_for_a_transition():
    data, _, _, info = DM.stem_fixture()
    assert ops(mr.LceModel(data, depthwise_i8_sections=True)) == info["plain"]
    assert ops(mr.LceModel(data, depthwise_i8_sections=True, stem_sections=True)) == info["plain"]        # (its input is the host's CONV_2D's)
    assert ops(mr.LceModel(data, depthwise_i8_sections=True, conv2d_i8_sections=True, stem_sections=True)) == [[0, 1, 2, 3, 4]]
    data, _, _, info = DM.transition_fixture()
    assert ops(mr.LceModel(data, depthwise_i8_sections=True)) == info["plain"]
    # behind the pool of the earlier names the blur joins, and the 1x1 behind it with conv2d_i8
    assert ops(mr.LceModel(data, depthwise_i8_sections=True, int8_add_sections=True, pool_sections=True)) == [[0, 1, 2, 3, 4], [6, 7]]


def test_the_pass_name_of_open_passes():
    """Fails without the feature: the parent refuses the name."""
    data, _, _, _ = DM.stem_fixture()
    lib, err = mr.tflite_lib(), C.create_string_buffer(256)
    h = lib.lce_tflite_model_open_passes(data, len(data), b"stem,conv2d_i8,depthwise_i8", err, 256)
    assert h, err.value
    assert lib.lce_tflite_model_num_sections(h) == 1
    lib.lce_tflite_model_close(h)
    assert not lib.lce_tflite_model_open_passes(data, len(data), b"depthwise_i8,stem,depthwise_i8", err, 256)
    assert b"'depthwise_i8' is named twice" in err.value
    assert not lib.lce_tflite_model_open_passes(data, len(data), b"depthwise_int8", err, 256) and b"unknown name 'depthwise_int8'" in err.value
    # no bit and no struct size enables it: every bit of the 56-byte options leaves the file cut
    every = dict(elementwise_sections=True, int8_add_sections=True, concat_sections=True, pool_sections=True, conv1x1_sections=True,
                 depthwise_sections=True, conv2d_sections=True, stem_sections=True)
    assert ops(mr.LceModel(data, **every)) == ops(mr.LceModel(data, stem_sections=True))


@pytest.mark.parametrize("name", sorted(NO_HEAD))
def test_the_name_moves_nothing_on_the_float_fixtures(name):
    data = NO_HEAD[name]()[0]
    for flags in ({}, dict(stem_sections=True), dict(elementwise_sections=True, pool_sections=True, conv1x1_sections=True, depthwise_sections=True,
                                                      conv2d_sections=True, stem_sections=True, head_sections=True), DM.EARLIER):
        without, with_name = mr.LceModel(data, **flags), mr.LceModel(data, depthwise_i8_sections=True, **flags)
        assert parts(with_name) == parts(without)
        assert with_name.depthwise_i8_stats() == (0, 0)


@pytest.mark.parametrize("name", sorted(M.FIXTURES) + sorted(HM.FIXTURES))
def test_the_name_moves_nothing_on_the_earlier_int8_fixtures(name):
    data = (M.FIXTURES[name] if name in M.FIXTURES else HM.FIXTURES[name])()[0]
    for flags in ({}, M.ALL_FLAGS, HM.EVERY_FLAG):
        assert parts(mr.LceModel(data, depthwise_i8_sections=True, **flags)) == parts(mr.LceModel(data, **flags))


def _graph(case):
    """x (float) -> 0 LceQuantize -> 1 LceBconv2d (int8; float for `hybrid`) -> r -> 2 DEPTHWISE_CONV_2D 3x3 (64 -> 64 m), varied by
    `case` -> s -> 3 LceQuantize.  Returns (file, index of the DEPTHWISE_CONV_2D)."""
    b = M.QModelBuilder()
    q_r, q_s = (0.05, -4), (0.04, 3)
    x = b.tensor([1, 6, 6, 64], np.float32, "x")
    q0 = b.tensor([1, 6, 6, 2], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    hybrid = case == "hybrid"
    r = SM._conv(b, q0, 6, 64, 64, 1)[0] if hybrid else M._bconv_int8(b, q0, 6, 64, 64, 1, 1, q_r)[0]
    m = 2 if case in ("multiplier_2", "multiplier_mismatch") else 1
    cout = 64 * m
    w, bias, sw = DM.depthwise_constants(cout, (3, 3), 3, q_r, q_s, per_channel=True)
    kw = dict(zero_points=[0] * 5 + [1] + [0] * (cout - 6)) if case == "filter_zero_point" else {}
    if case == "two_scales":
        sw, kw = sw[:2], dict(zero_points=[0, 0])
    if case == "per_tensor":
        sw = sw[:1]
    if case == "leading_extent_2":
        w = np.concatenate([w, w], 0)
    flt = DM.depthwise_filter_tensor(b, w, sw, quantized_dimension=0 if case == "quantized_dimension_0" else 3, **kw)
    bt = b.tensor([cout], np.float32, "wb", bias.astype(np.float32)) if case == "float_bias" else b.tensor([cout], np.int32, "wb", bias)
    ins = [r, flt] if case == "no_bias" else [r, flt, -1] if case == "bias_minus_1" else [r, flt, bt]
    shape = [1, 6, 6, cout]
    if hybrid:
        s = b.tensor(shape, np.float32, "s")
    else:
        s = b.tensor(shape, np.int8, "s", scale=q_s[0], zero_point=200 if case == "output_zero_point_200" else q_s[1])
    dw = depthwise_op(b, ins, [s], (1, 1), SAME, 1 if case == "multiplier_mismatch" else m, NONE,
                      dilation=(2, 2) if case == "dilation_2" else (1, 1), options=case != "no_options")
    q1 = b.tensor([1, 6, 6, cout // 32], np.int32, "q1")
    b.custom_op("LceQuantize", [s], [q1], b"")
    b.inputs, b.outputs = [x], [q1]
    return b.finish(), dw


@pytest.mark.parametrize("case", ["dilation_2", "hybrid", "filter_zero_point", "quantized_dimension_0", "two_scales", "float_bias", "no_options",
                                  "multiplier_mismatch", "leading_extent_2", "output_zero_point_200"])
def test_what_the_candidate_refuses_stays_with_the_host(case):
    data, dw = _graph(case)
    every = dict(DM.EVERY_FLAG, depthwise_sections=True, elementwise_sections=True)
    assert ops(mr.LceModel(data, **every)) == [[0, 1], [3]] == ops(mr.LceModel(data))


@pytest.mark.parametrize("case", ["plain", "per_tensor", "no_bias", "bias_minus_1", "multiplier_2"])
def test_what_the_candidate_accepts_joins(case):
    data, dw = _graph(case)
    assert ops(mr.LceModel(data, depthwise_i8_sections=True)) == [[0, 1, 2, 3]] and ops(mr.LceModel(data)) == [[0, 1], [3]]
    assert ops(mr.LceModel(data, **DM.EARLIER)) == [[0, 1], [3]]


def test_constants_that_prepare_refuses_stay_with_the_host():
    """A bias beyond the accumulator bound: the reference's own int32 accumulator could overflow."""
    for bias_1, joins in ((2 ** 31 - 1, False), (1000, True)):
        b = M.QModelBuilder()
        x = b.tensor([1, 4, 4, 4], np.int8, "x", scale=0.5, zero_point=0)
        w = np.ones((1, 1, 1, 4), np.int8)
        s = b.tensor([1, 4, 4, 4], np.int8, "s", scale=0.5, zero_point=0)
        bias = np.array([0, bias_1, 0, 0], np.int32)
        depthwise_op(b, [x, DM.depthwise_filter_tensor(b, w, [2.0 ** -20]), b.tensor([4], np.int32, "wb", bias)], [s], (1, 1), SAME)
        q = b.tensor([1, 4, 4, 1], np.int32, "q")
        b.custom_op("LceQuantize", [s], [q], b"")
        b.inputs, b.outputs = [x], [q]
        assert ops(mr.LceModel(b.finish(), depthwise_i8_sections=True, stem_sections=True)) == ([[0, 1]] if joins else [[1]])
