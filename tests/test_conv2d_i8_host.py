"""The quantized CONV_2D inside the sections (lce_hip_conv2d_i8, "conv2d_i8" of lce_tflite_model_open_passes) on the CPU: the
NumPy restatement (tests/conv2d_i8_ref.py) against a float64 convolution and against known answers worked by hand;
lce_hip_conv2d_i8_prepare's table against the restatement and every refusal of the three entries with its status; the
requantization function of the kernel's epilogue, compiled for the host, against the restatement; the reader on per-channel
files; and the partitions of the fixtures of tests/int8_conv_models.py with and without the new pass."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

import conv2d_i8_ref as R
import int8_conv_models as M
from conv2d_i8_cases import GRID, KNOWN, REQUANT_KNOWN, operands
from section_models import (ADD, CONV_2D, NONE, SAME, alexnet_body_model, bconv_options, bireal_block_model, conv2d_op, dense_block_model,
                            quicknet_transition_model)
from hostsim_conv2d_i8_lib import requantize

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,cin", GRID)
def test_the_accumulation_equals_a_float64_convolution_of_the_zero_padded_image(filt, cin):
    n = 0
    for image, stride, padding, zi in (((5, 7), (1, 1), R.SAME, 5), ((9, 8), (2, 2), R.SAME, -128), ((9, 8), (4, 3), R.VALID, 127),
                                       ((1, 1), (1, 1), R.SAME, -3)):
        if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
            continue
        x, w, _, _, _, _ = operands((2, *image, cin), filt, 5, 31 * cin + image[0], zi)
        acc = R.accumulate(x, w, zi, stride, padding)
        ref = R.accumulate_float64(x, w, zi, stride, padding)
        assert acc.shape == ref.shape and np.abs(ref).max() < 2.0 ** 53 and np.array_equal(acc.astype(np.float64), ref)
        n += 1
    assert n >= 3


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_restatement_gives_the_known_answers(name):
    k = KNOWN[name]
    got = R.conv2d_i8(k["x"], k["w"], k["bias"], k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], k["act"])
    assert got.dtype == np.int8 and np.array_equal(got, k["want"]), (got, k["want"])


def test_the_known_answers_cover_what_they_claim():
    m = lambda k: R.multipliers(k["q_in"][0], k["sw"], k["q_out"][0], 1)
    assert m(KNOWN["ties"]) == ([1 << 30], [-1]) and m(KNOWN["e_zero"]) == ([1 << 30], [0])
    assert m(KNOWN["e_positive"]) == ([1 << 30], [2]) and m(KNOWN["e_minus_31"]) == ([1 << 30], [-31])
    assert m(KNOWN["corner_same_pad"]) == ([1 << 30], [-2])
    assert KNOWN["zi_minus_128"]["want"].min() == -128 and KNOWN["zi_127"]["want"].max() == 127       # both clamp ends
    # the skipped taps of the corner: read as x = 0 they would change the answer
    k = KNOWN["corner_same_pad"]
    zero_padded = np.zeros((1, 4, 4, 1), np.int8)
    zero_padded[:, 1:3, 1:3] = k["x"]
    wrong = R.conv2d_i8(zero_padded, k["w"], None, k["sw"], k["q_in"], k["q_out"], 1, R.VALID)
    assert wrong.shape == k["want"].shape and not np.array_equal(wrong, k["want"])
    # ... and staged as x = zi they are the skip
    zi_padded = np.full((1, 4, 4, 1), k["q_in"][1], np.int8)
    zi_padded[:, 1:3, 1:3] = k["x"]
    assert np.array_equal(R.conv2d_i8(zi_padded, k["w"], None, k["sw"], k["q_in"], k["q_out"], 1, R.VALID), k["want"])
    assert [R.activation_range(a, 0.05, -10) for a in (R.NONE, R.RELU, R.RELU_N1_TO_1, R.RELU6)] == [(-128, 127), (-10, 127), (-30, 10), (-10, 110)]


def test_the_grid_operands_spread_over_the_int8_range():
    for filt, cin in GRID:
        x, w, bias, sw, q_in, q_out = operands((3, 5, 7, cin), filt, 33, 1)
        y = R.conv2d_i8(x, w, bias, sw, q_in, q_out)
        sat = np.mean((y == 127) | (y == -128))
        assert 0 < sat < 0.3 and np.unique(y).size > 100, (filt, cin, sat)


# ---- the requantization the kernel runs -----------------------------------------------------------------------------------------------
def test_the_requantization_restated_gives_the_known_answers():
    for acc, m, e, want in REQUANT_KNOWN:
        if abs(acc) << max(e, 0) <= R.INT32_MAX:
            assert int(R.requantize(np.array([acc]), m, e)[0]) == want, (acc, m, e)


def test_the_kernels_requantization_equals_the_restatement_on_a_million_triples():
    g = np.random.default_rng(3)
    edge_m = [0, 1 << 30, (1 << 30) + 1, (1 << 31) - 1, 1518500250]
    edge_e = [-31, -30, -8, -1, 0, 1, 7, 30]
    pairs = [(m, e) for m in edge_m for e in edge_e]
    while len(pairs) < 1000:
        pairs.append((int(g.integers(1 << 30, 1 << 31)), int(g.integers(-31, 31))))
    total = 0
    for m, e in pairs:
        lim = R.INT32_MAX >> max(e, 0)                       # what lce_hip_conv2d_i8_prepare guarantees: acc * 2^e fits
        acc = np.concatenate([g.integers(-lim - 1, lim + 1, 1000), [0, 1, -1, lim, -lim - 1, lim // 2, -(lim // 2) - 1]]).astype(np.int64)
        got = requantize(acc, np.full(acc.shape, m), np.full(acc.shape, e))
        assert np.array_equal(got, R.requantize(acc, m, e)), (m, e)
        total += acc.size
    assert total >= 10 ** 6


# ---- prepare ------------------------------------------------------------------------------------------------------------------------
def desc(cout=4, filt=(3, 3), cin=3, image=(9, 9), stride=(1, 1), padding=amd.PADDING_SAME, act=amd.ACT_NONE, q_in=(0.5, 0), q_out=(0.5, 0), batch=1):
    return amd.Conv2dI8Desc(batch, image[0], image[1], cin, cout, filt[0], filt[1], stride[0], stride[1], padding, act, q_in[0], q_in[1],
                            q_out[0], q_out[1])


def c_prepare(d, w, bias, sw):
    """(status, message, table, act_min, act_max) of lce_hip_conv2d_i8_prepare on NumPy constants."""
    cout = d.channels_out
    table = np.zeros((3, cout), np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    sw = np.ascontiguousarray(np.atleast_1d(sw), np.float32)
    rc = amd.lib().lce_hip_conv2d_i8_prepare(C.byref(d), w.ctypes.data, None if bias is None else bias.ctypes.data, sw.ctypes.data, sw.size,
                                             table.ctypes.data, C.byref(lo), C.byref(hi))
    return rc, amd.lib().lce_hip_last_error().decode(), table, lo.value, hi.value


def test_prepare_equals_the_restatement_on_random_constants():
    g = np.random.default_rng(11)
    for n in range(60):
        filt, cin, cout = (int(g.integers(1, 8)), int(g.integers(1, 8))), int(g.integers(1, 70)), int(g.integers(1, 40))
        zi, zo, act = int(g.integers(-128, 128)), int(g.integers(-128, 128)), int(g.integers(0, 4))
        si, so = (float(np.float32(np.exp(g.uniform(np.log(1e-3), np.log(1.0))))) for _ in range(2))
        w = g.integers(-128, 128, (cout, *filt, cin), dtype=np.int64).astype(np.int8)
        bias = None if n % 3 == 0 else g.integers(-(1 << 20), 1 << 20, cout, dtype=np.int64).astype(np.int32)
        sw = np.exp(g.uniform(np.log(1e-4), np.log(0.5), cout if n % 2 else 1)).astype(np.float32)
        d = desc(cout, filt, cin, (9, 9), q_in=(si, zi), q_out=(so, zo), act=act)
        rc, msg, table, lo, hi = c_prepare(d, w, bias, sw)
        try:
            want = R.table(w, bias, sw, si, zi, so)
        except ValueError:
            assert rc == amd.ERR_UNSUPPORTED and "channel" in msg, msg
            continue
        assert rc == amd.OK, msg
        assert np.array_equal(table, want) and (lo, hi) == R.activation_range(act, so, zo)
        py = amd.conv2d_i8_prepare(w, bias, sw, (si, zi), (so, zo), act)
        assert np.array_equal(py[0], want) and py[1:] == (lo, hi)


def test_the_overflow_bound_just_under_and_just_over():
    """255 x 128 x K + B against 2^31 - 1: K = 65793 passes without a bias (2147483520) and with |bias| = 127, fails with 128;
    K = 65794 fails."""
    assert 255 * 128 * 65793 + 127 == 2 ** 31 - 1 and 255 * 128 * 65794 > 2 ** 31 - 1
    for cin, bias, ok in ((65793, None, True), (65793, [5, -127], True), (65793, [5, -128], False), (65794, None, False)):
        w = np.ones((2, 1, 1, cin), np.int8)
        b = None if bias is None else np.array(bias, np.int32)
        rc, msg, table, _, _ = c_prepare(desc(2, (1, 1), cin, (1, 1)), w, b, 2.0 ** -20)
        if ok:
            assert rc == amd.OK and table[0].tolist() == ([0, 0] if b is None else bias), msg
        else:
            assert rc == amd.ERR_UNSUPPORTED and "channel %d" % (1 if bias else 0) in msg and "exceeds 2^31 - 1" in msg, msg
    # the check of the run entry has the K bound too: beyond it no table exists
    oh, ow = C.c_int32(), C.c_int32()
    assert amd.lib().lce_hip_conv2d_i8_check(C.byref(desc(2, (1, 1), 65793, (1, 1))), C.byref(oh), C.byref(ow)) == amd.OK
    assert amd.lib().lce_hip_conv2d_i8_check(C.byref(desc(2, (1, 1), 65794, (1, 1))), C.byref(oh), C.byref(ow)) == amd.ERR_UNSUPPORTED
    # a left shift: K = 1, bound 32640; multiplier 0.75 x 2^17 has e = 17: 32640 x 2^17 > 2^31 - 1, while e = 16 passes
    w = np.ones((3, 1, 1, 1), np.int8)
    rc, msg, _, _, _ = c_prepare(desc(3, (1, 1), 1, (1, 1), q_in=(1.0, 0), q_out=(1.0, 0)), w, None, [1.0, 0.75 * 2.0 ** 17, 1.0])
    assert rc == amd.ERR_UNSUPPORTED and "channel 1" in msg and "2^17" in msg, msg
    assert R.quantize_multiplier(0.75 * 2.0 ** 17)[1] == 17 and R.quantize_multiplier(0.75 * 2.0 ** 16)[1] == 16 and 32640 << 16 <= 2 ** 31 - 1
    assert c_prepare(desc(3, (1, 1), 1, (1, 1), q_in=(1.0, 0), q_out=(1.0, 0)), w, None, [1.0, 0.75 * 2.0 ** 16, 1.0])[0] == amd.OK


def test_prepare_refuses_what_is_malformed():
    w, sw = np.ones((4, 3, 3, 3), np.int8), np.full(4, 0.5, np.float32)
    table, lo, hi = np.zeros((3, 4), np.int32), C.c_int32(), C.c_int32()
    good = dict(d=desc(), w=w.ctypes.data, b=None, s=sw.ctypes.data, n=4, t=table.ctypes.data, lo=C.byref(lo), hi=C.byref(hi))
    call = lambda **kw: (lambda a: (amd.lib().lce_hip_conv2d_i8_prepare(C.byref(a["d"]) if a["d"] is not None else None, a["w"], a["b"], a["s"],
                                                                        a["n"], a["t"], a["lo"], a["hi"]),
                                    amd.lib().lce_hip_last_error().decode()))({**good, **kw})
    assert call()[0] == amd.OK
    for kw, msg in ((dict(d=None), "null desc"), (dict(w=None), "null filter"), (dict(s=None), "null filter scales"), (dict(t=None), "null result"),
                    (dict(lo=None), "null result"), (dict(hi=None), "null result"), (dict(n=2), "2 scales"), (dict(n=0), "0 scales"),
                    (dict(d=desc(q_in=(0.0, 0))), "input_scale must be finite and positive"),
                    (dict(d=desc(q_in=(float("inf"), 0))), "input_scale must be finite and positive"),
                    (dict(d=desc(q_out=(float("nan"), 0))), "output_scale must be finite and positive"),
                    (dict(d=desc(q_out=(-1.0, 0))), "output_scale must be finite and positive"),
                    (dict(d=desc(q_in=(0.5, 128))), "input_zero_point must be in"), (dict(d=desc(q_out=(0.5, -129))), "output_zero_point must be in"),
                    (dict(d=desc(cout=0)), "extents must be positive"), (dict(d=desc(filt=(0, 3))), "the filter must be positive"),
                    (dict(d=desc(stride=(1, 0))), "the stride must be positive"), (dict(d=desc(padding=2)), "padding must be SAME or VALID"),
                    (dict(d=desc(act=4)), "unknown activation"), (dict(d=desc(filt=(10, 10), padding=amd.PADDING_VALID)), "empty output")):
        rc, text = call(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_conv2d_i8_prepare"), (kw, text)
    bad = sw.copy()
    bad[2] = 0.0
    rc, text = call(s=bad.ctypes.data)
    assert rc == amd.ERR_INVALID and "channel 2" in text


def test_the_run_entry_refuses_before_any_device_call():
    """The checks on pointers, overlap and alignment come before the device is asked for: made-up addresses never reach it."""
    d = desc(cout=64, cin=64, image=(8, 8), batch=2)               # in: 8192 B, filter: 36864 B, table: 768 B, out: 8192 B, bits: 1024 B
    lib = amd.lib()
    p = lambda v: None if v is None else C.c_void_p(v)
    def call(x=1 << 20, w=2 << 20, t=3 << 20, o=4 << 20, b=5 << 20, dd=d):
        rc = lib.lce_hip_conv2d_i8(C.byref(dd) if dd is not None else None, p(x), p(w), p(t), p(o), p(b), None)
        return rc, lib.lce_hip_last_error().decode()
    for kw, msg in ((dict(dd=None), "null desc"), (dict(x=None), "null input"), (dict(w=None), "null filter"), (dict(t=None), "null table"),
                    (dict(o=None, b=None), "both outputs are null"), (dict(o=(1 << 20) + 8191), "an output overlaps the input"),
                    (dict(b=(2 << 20) + 36860), "an output overlaps the filter"), (dict(o=(3 << 20) - 1), "an output overlaps the table"),
                    (dict(b=(4 << 20) + 8188), "the two outputs overlap"), (dict(b=(5 << 20) + 2), "out_bits_dev must be 4-byte aligned"),
                    (dict(t=(3 << 20) + 1), "table_dev must be 4-byte aligned"), (dict(dd=desc(q_in=(0.5, 300))), "input_zero_point"),
                    (dict(dd=desc(act=9)), "unknown activation")):
        rc, text = call(**kw)
        assert rc == amd.ERR_INVALID and msg in text and text.startswith("lce_hip_conv2d_i8:"), (kw, text)
    rc, text = call(dd=desc(cin=65794, filt=(1, 1), image=(1, 1)))
    assert rc == amd.ERR_UNSUPPORTED and "65794" in text
    # the int8 operands need no alignment: odd addresses pass every host check.  Only where there is no device to launch on: there
    # the call ends at the device query (made-up addresses must never reach a kernel)
    if amd.device_count() == 0:
        rc, text = call(x=(1 << 20) + 1, w=(2 << 20) + 3, o=(4 << 20) + 5)
        assert rc == amd.ERR_NO_DEVICE, text


def test_python_checks_fail_before_any_device_call():
    x, w, t = np.zeros((1, 5, 5, 3), np.int8), np.zeros((4, 3, 3, 3), np.int8), np.zeros((3, 4), np.int32)
    q = ((0.5, 0), (0.5, 0))
    for args, kw, msg in (((x.astype(np.float32), w, t, *q), {}, "x must be a non-empty int8 NHWC"), ((x, w.astype(np.float32), t, *q), {}, "w must be int8"),
                          ((x, w[..., :2], t, *q), {}, "w must be int8"), ((x, w, t[:2], *q), {}, "table must be int32"),
                          ((x, w, t, (0.5,), q[1]), {}, "q_in must be"), ((x, w, t, (0.5, 200), q[1]), {}, "zero point"),
                          ((x, w, t, q[0], (0.0, 0)), {}, "scale must be finite"), ((x, w, t, *q), dict(stride=0), "stride"),
                          ((x, w, t, *q), dict(padding=3), "padding"), ((x, w, t, *q), dict(activation=7), "activation"),
                          ((x, w, t, *q), dict(out=False), "no output requested"),
                          ((x, w, t, *q), dict(out=np.zeros((1, 5, 5, 4), np.float32)), "out must be int8")):
        with pytest.raises(ValueError, match=msg):
            amd.conv2d_i8(*args, **kw)
    with pytest.raises(ValueError, match="bias must be int32"):
        amd.conv2d_i8_prepare(w, np.zeros(4, np.float32), 0.5, *q)
    with pytest.raises(ValueError, match="filter_scales"):
        amd.conv2d_i8_prepare(w, None, [0.5, 0.5], *q)


def test_the_abi_grew_by_three_symbols_and_keeps_its_version():
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_conv2d_i8", "lce_hip_conv2d_i8_check", "lce_hip_conv2d_i8_prepare"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_conv_i8_stats") and hasattr(mr.tflite_lib(), "lce_tflite_model_tensor_scales")


# ---- the reader -----------------------------------------------------------------------------------------------------------------------
def _one_filter_file(scales, zero_points, qdim):
    b = M.QModelBuilder()
    w = np.arange(4 * 2, dtype=np.int8).reshape(4, 1, 1, 2)
    t = b.qtensor(w.shape, np.int8, "w", w, scales, zero_points, qdim)
    x = b.tensor([1, 2, 2, 2], np.int8, "x", scale=0.25, zero_point=-7)
    b.inputs, b.outputs = [x], [x]
    return b.finish(), t, x


def test_the_reader_keeps_the_scale_vector_and_the_quantized_dimension():
    scales = [0.5, 0.25, 0.125, 2.0]
    data, t, x = _one_filter_file(scales, [0, 0, 0, 0], 3)
    m = mr.LceModel(data)
    assert m.tensors[t].scales == tuple(scales) and m.tensors[t].quantized_dimension == 3
    assert m.tensors[t].scale == 0.5 and m.tensors[t].zero_point == 0                  # `scale` stays the first element
    assert m.tensors[x].scales == (0.25,) and m.tensors[x].quantized_dimension == 0 and m.tensors[x].zero_point == -7
    data, t, _ = _one_filter_file(scales, None, None)                                  # no zero points, no quantized_dimension field
    m = mr.LceModel(data)
    assert m.tensors[t].scales == tuple(scales) and m.tensors[t].quantized_dimension == 0
    lib, n = mr.tflite_lib(), C.c_int32(7)
    two = (C.c_float * 2)()
    assert lib.lce_tflite_model_tensor_scales(m._h, t, two, 2, C.byref(n)) == 4 and list(two) == [0.5, 0.25] and n.value == 0
    assert lib.lce_tflite_model_tensor_scales(m._h, 99, None, 0, None) == -1 and lib.lce_tflite_model_tensor_scales(None, 0, None, 0, None) == -1


def test_a_truncated_scale_vector_is_refused():
    """The scale vector's element count is raised beyond the end of the file: the reader refuses the file instead of reading on."""
    scales = [0.5, 0.25, 0.125, 2.0]
    data, _, _ = _one_filter_file(scales, [0, 0, 0, 0], 0)
    payload = struct.pack("<I4f", 4, *scales)
    at = data.index(payload)
    assert data.count(payload) == 1
    for count in (len(data), 0x7fffffff, 0xffffffff, (len(data) - at - 4) // 4 + 1):
        bad = data[:at] + struct.pack("<I", count) + data[at + 4:]
        with pytest.raises(ValueError, match="QuantizationParameters.scale"):
            mr.LceModel(bad)
    cut = data[:at + 4 + 8]                                                              # the file ends inside the vector
    with pytest.raises(ValueError):
        mr.LceModel(cut)


# ---- the partition --------------------------------------------------------------------------------------------------------------------
def ops(model):
    return [s.ops for s in model.sections]


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_each_fixture_is_one_section_with_the_pass_and_cut_as_today_without(name):
    data, x, out, info = M.FIXTURES[name]()
    one = mr.LceModel(data, **M.ALL_FLAGS)
    assert ops(one) == [list(range(info["ops"]))] and one.sections[0].inputs == [x] and one.sections[0].outputs == [out]
    it = mr.Interpreter(data, **M.ALL_FLAGS)
    assert it.lce_only and len(it.sections) == 1
    # without conv2d_i8: the parent's partitions, through the parent's routes
    assert ops(mr.LceModel(data)) == info["plain"] and ops(mr.LceModel(data, **info["parent_flags"])) == info["parent_sections"]
    assert not mr.Interpreter(data, **info["parent_flags"]).lce_only
    # every float opt-in and the head leave an int8 CONV_2D with the host
    floats = dict(elementwise_sections=True, concat_sections=True, conv1x1_sections=True, depthwise_sections=True, conv2d_sections=True,
                  head_sections=True)
    assert ops(mr.LceModel(data, **floats, **info["parent_flags"])) == info["parent_sections"]
    # the per-channel file carries Cout scales, the per-tensor file one
    flt = one.tensors[one.operators[info["conv"]].inputs[1]]
    assert len(flt.scales) == (flt.shape[0] if name.endswith("per_channel") else 1) and np.allclose(flt.scales, info["sw"], rtol=0, atol=0)
    # at another batch the section's shapes follow
    dims, nbytes = one.section_tensor_shape(0, out, 3)
    assert dims[0] == 3 and dims[1:] == tuple(one.tensors[out].shape[1:]) and nbytes == int(np.prod(dims))


def test_the_shortcut_fixtures_host_pool_is_the_rounded_mean():
    """The oracle side of the fixture: AVERAGE_POOL_2D 2x2 / 2 on int8 is the sum of four plus or minus 2, divided by 4 towards zero."""
    _, _, _, info = M.shortcut_fixture()
    x = np.random.default_rng(1).integers(-128, 128, (2, 8, 8, 64), dtype=np.int64).astype(np.int8)
    s = x.astype(np.int64).reshape(2, 4, 2, 4, 2, 64).sum(axis=(2, 4))
    num = np.where(s > 0, s + 2, s - 2)
    want = (np.sign(num) * (np.abs(num) // 4)).astype(np.int8)
    assert np.array_equal(info["host"][info["pool"]](x), want) and np.abs(want.astype(int)).max() < 128


def test_the_pass_alone_needs_the_stem_flag_for_a_stem_and_an_lce_epoch_for_a_shortcut():
    data, _, _, info = M.stem_fixture()
    assert ops(mr.LceModel(data, conv2d_i8_sections=True)) == info["plain"]
    assert ops(mr.LceModel(data, conv2d_i8_sections=True, stem_sections=True)) == [[0, 1, 2]]
    data, _, _, info = M.shortcut_fixture()
    assert ops(mr.LceModel(data, conv2d_i8_sections=True)) == info["plain"]


def test_the_pass_name_of_open_passes():
    data, _, _, _ = M.stem_fixture()
    lib, err = mr.tflite_lib(), C.create_string_buffer(256)
    h = lib.lce_tflite_model_open_passes(data, len(data), b"stem,conv2d_i8", err, 256)
    assert h and lib.lce_tflite_model_num_sections(h) == 1
    lib.lce_tflite_model_close(h)
    assert not lib.lce_tflite_model_open_passes(data, len(data), b"conv2d_i8,stem,conv2d_i8", err, 256) and b"'conv2d_i8' is named twice" in err.value
    assert not lib.lce_tflite_model_open_passes(data, len(data), b"conv2d_int8", err, 256) and b"unknown name 'conv2d_int8'" in err.value


def test_the_pass_alone_moves_nothing_on_the_float_fixtures():
    from test_conv2d_sections_host import FIXTURES as FLOAT_FIXTURES
    files = [f()[0] for f in (alexnet_body_model, bireal_block_model, quicknet_transition_model, dense_block_model)]
    files += [FLOAT_FIXTURES[n]()[0] for n in sorted(FLOAT_FIXTURES)]
    for data in files:
        assert ops(mr.LceModel(data, conv2d_i8_sections=True)) == ops(mr.LceModel(data))
        with_stem = ops(mr.LceModel(data, conv2d_i8_sections=True, stem_sections=True))
        assert with_stem == ops(mr.LceModel(data, stem_sections=True))


def _graph(case):
    """x (float) -> 0 LceQuantize -> 1 LceBconv2d (int8) -> r -> 2 CONV_2D 3x3 int8 (64 -> 4), varied by `case` -> s -> 3 LceQuantize.
    Returns (file, index of the CONV_2D)."""
    b = M.QModelBuilder()
    q_r, q_s = (0.05, -4), (0.04, 3)
    x = b.tensor([1, 6, 6, 64], np.float32, "x")
    q0 = b.tensor([1, 6, 6, 2], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    r, _ = M._bconv_int8(b, q0, 6, 64, 64, 1, 1, q_r)
    cin = 32 if case == "grouped" else 64
    w, bias, sw = M.conv_constants(4, (3, 3), cin, 3, q_r, q_s, per_channel=True)
    kw = dict(zero_points=[0, 0, 1, 0]) if case == "filter_zero_point" else {}
    if case == "two_scales":
        sw, kw = sw[:2], dict(zero_points=[0, 0])
    if case == "per_tensor":
        sw = sw[:1]
    flt = M.filter_tensor(b, w, sw, quantized_dimension=3 if case == "quantized_dimension_3" else 0, **kw)
    bt = b.tensor([4], np.float32, "wb", bias.astype(np.float32)) if case == "float_bias" else b.tensor([4], np.int32, "wb", bias)
    ins = [r, flt] if case == "no_bias" else [r, flt, -1] if case == "bias_minus_1" else [r, flt, bt]
    s_kw = dict(scale=q_s[0], zero_point=200 if case == "output_zero_point_200" else q_s[1])
    s = b.tensor([1, 6, 6, 4], np.int8, "s", **s_kw)
    conv = conv2d_op(b, ins, [s], (1, 1), SAME, NONE, dilation=(2, 2) if case == "dilation_2" else (1, 1), options=case != "no_options")
    q1 = b.tensor([1, 6, 6, 1], np.int32, "q1")
    b.custom_op("LceQuantize", [s], [q1], b"")
    b.inputs, b.outputs = [x], [q1]
    return b.finish(), conv


@pytest.mark.parametrize("case", ["filter_zero_point", "two_scales", "quantized_dimension_3", "float_bias", "dilation_2", "grouped", "no_options",
                                  "output_zero_point_200"])
def test_what_the_candidate_refuses_stays_with_the_host(case):
    data, conv = _graph(case)
    assert ops(mr.LceModel(data, **M.ALL_FLAGS)) == [[0, 1], [3]] == ops(mr.LceModel(data))


@pytest.mark.parametrize("case", ["plain", "per_tensor", "no_bias", "bias_minus_1"])
def test_what_the_candidate_accepts_joins(case):
    data, conv = _graph(case)
    assert ops(mr.LceModel(data, conv2d_i8_sections=True)) == [[0, 1, 2, 3]] and ops(mr.LceModel(data)) == [[0, 1], [3]]


def test_constants_that_prepare_refuses_stay_with_the_host():
    """A bias beyond the accumulator bound: the reference's own int32 accumulator could overflow."""
    b = M.QModelBuilder()
    x = b.tensor([1, 4, 4, 8], np.int8, "x", scale=0.5, zero_point=0)
    w = np.ones((4, 1, 1, 8), np.int8)
    s = b.tensor([1, 4, 4, 4], np.int8, "s", scale=0.5, zero_point=0)
    bias = np.array([0, 2 ** 31 - 1, 0, 0], np.int32)
    conv2d_op(b, [x, M.filter_tensor(b, w, [2.0 ** -20]), b.tensor([4], np.int32, "wb", bias)], [s], (1, 1), SAME)
    q = b.tensor([1, 4, 4, 1], np.int32, "q")
    b.custom_op("LceQuantize", [s], [q], b"")
    b.inputs, b.outputs = [x], [q]
    assert ops(mr.LceModel(b.finish(), conv2d_i8_sections=True, stem_sections=True)) == [[1]]
