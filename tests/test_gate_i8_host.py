"""Host-only checks of the int8 gate's entries (lce_hip_mul_int8_prepare, lce_hip_mul_int8_path, lce_hip_logistic_int8_prepare):
the parameters and the LOGISTIC table against the NumPy restatement (tests/gate_i8_ref.py), every refusal with the field it names,
and the deviation from the real-valued result that include/lce_hip.h quotes.  No GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gate_i8_ref as G
import int8_add_ref as ar

amd = importlib.import_module("compute-engine_amd")
DRAWS = G.mul_draws(300, 2024)


def _logistic_draws(n, seed):
    """Input scales up to 0.02: |x| stays below 5.1, so few of the 256 results reach a clamp bound."""
    g = np.random.default_rng(seed)
    return [(float(np.float32(np.exp(g.uniform(np.log(1e-3), np.log(0.02))))), int(g.integers(-128, 128))) for _ in range(n)]


LOGISTIC_DRAWS = _logistic_draws(300, 7)


def _add_for(qo, seed):
    g = np.random.default_rng(seed)
    q_ad = (float(np.float32(qo[0] * g.uniform(0.5, 2.0))), int(g.integers(-128, 128)))
    return q_ad, (float(np.float32((qo[0] + q_ad[0]) * g.uniform(0.6, 1.2))), int(g.integers(-60, 60)))


def test_prepare_against_the_restatement_for_300_draws():
    for k, (q1, q2, qo) in enumerate(DRAWS):
        act = k % 4
        q_ad, q_sum = _add_for(qo, k)
        p = amd.mul_int8_params(q1, q2, qo, act, add=(q_ad, q_sum, (k // 4) % 4))
        assert (p["multiplier"], p["shift"], p["act_min"], p["act_max"]) == G.mul_params(q1, q2, qo, act), (k, q1, q2, qo)
        want = ar.prepare(qo[0], qo[1], q_ad[0], q_ad[1], q_sum[0], q_sum[1], (k // 4) % 4)
        assert tuple(p["add"][n] for n in ar.PARAM_NAMES) == want
        assert "add" not in amd.mul_int8_params(q1, q2, qo, act)


def test_the_logistic_table_against_the_restatement_for_300_draws():
    for q in LOGISTIC_DRAWS + [(0.05, 3), (0.1, -128), (1.0, 127), (3.0, 0)]:
        assert np.array_equal(amd.logistic_int8_table(q), G.logistic_table(q)), q


def test_the_logistic_table_is_monotone_and_centred():
    t = amd.logistic_int8_table((0.02, 5)).view(np.int8).astype(int)
    assert np.all(np.diff(t) >= 0) and t[5 + 128] == 0 and t[0] < -100 and t[-1] > 100


def _desc(**kw):
    d = amd._mul_int8_desc("t", (0.05, 3), (1 / 256, -128), (0.04, -5), 0, kw.pop("per_image", False),
                           kw.pop("add", ((0.03, 1), (0.06, 2), 0)))
    for k, v in kw.items():
        if k == "reserved":
            d.reserved[1] = v
        else:
            setattr(d, k, v)
    return d


def _refused(call, *names):
    with pytest.raises(amd.LceHipError) as e:
        amd.check(call())
    assert e.value.code == amd.ERR_INVALID
    for n in names:
        assert n in str(e.value), str(e.value)


REFUSED_FIELDS = [
    ("in1_scale", 0.0, ("in1_scale",)), ("in1_scale", float("nan"), ("in1_scale",)), ("in2_scale", float("inf"), ("in2_scale",)),
    ("in2_scale", -1.0, ("in2_scale",)), ("out_scale", 0.0, ("out_scale",)),
    ("in1_zero_point", 300, ("in1_zero_point",)), ("in2_zero_point", -129, ("in2_zero_point",)), ("out_zero_point", 128, ("out_zero_point",)),
    ("activation", 4, ("unknown activation",)), ("activation", -1, ("unknown activation",)),
    ("operand", 1, ("operand kind",)), ("operand", 0, ("operand kind",)), ("operand", 4, ("operand kind",)),
    ("has_add", 2, ("has_add",)), ("reserved", 1, ("reserved",)),
    ("addend_scale", 0.0, ("add", "in2_scale")), ("addend_zero_point", 200, ("add", "in2_zero_point")),
    ("add_scale", float("nan"), ("add", "out_scale")), ("add_zero_point", -200, ("add", "out_zero_point")),
    ("add_activation", 7, ("add", "unknown activation")),
    ("add_scale", 1e-9, ("add", "real multiplier of out")),
]


def test_prepare_refuses_and_names_the_field():
    for field, value, names in REFUSED_FIELDS:
        d, p = _desc(**{field: value}), amd.MulInt8Params()
        _refused(lambda: amd.lib().lce_hip_mul_int8_prepare(C.byref(d), C.byref(p)), "lce_hip_mul_int8_prepare", *names)


def test_the_add_refusals_are_add_int8_prepares_own():
    """The same parameters through lce_hip_add_int8_prepare give the same sentence after the entry's name."""
    d, p = _desc(add_scale=1e-9), amd.MulInt8Params()
    with pytest.raises(amd.LceHipError) as e1:
        amd.check(amd.lib().lce_hip_mul_int8_prepare(C.byref(d), C.byref(p)))
    with pytest.raises(amd.LceHipError) as e2:
        amd.add_int8_params((0.04, -5), (0.03, 1), (1e-9, 2))
    assert str(e1.value).split("add: ")[1] == str(e2.value).split("lce_hip_add_int8_prepare: ")[1]


def test_a_multiplier_that_could_leave_int32_is_refused():
    p = amd.MulInt8Params()
    d = _desc(out_scale=1e-9, has_add=0)                      # s1 s2 / so = 195 312: 65 025 * 2^18 is beyond int32
    _refused(lambda: amd.lib().lce_hip_mul_int8_prepare(C.byref(d), C.byref(p)), "int32")
    d = _desc(in1_scale=1e-30, in2_scale=1e-30, has_add=0)    # the float32 product is 0
    _refused(lambda: amd.lib().lce_hip_mul_int8_prepare(C.byref(d), C.byref(p)), "real multiplier")
    _refused(lambda: amd.lib().lce_hip_mul_int8_prepare(None, C.byref(p)), "null")
    _refused(lambda: amd.lib().lce_hip_mul_int8_prepare(C.byref(d), None), "null")


def test_the_launch_refuses_before_any_pointer_is_touched():
    """The pointers below are not addresses of anything: a refusal that came after a read of them would be a crash."""
    L, call = amd.MulInt8Launch(), amd.lib().lce_hip_mul_int8
    x, g, a, o, b = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    gate, tensor = _desc(per_image=True), _desc()
    _refused(lambda: call(C.byref(gate), x, g, a, 6, 32, 0, o, b, None), "rows_per_image")
    _refused(lambda: call(C.byref(gate), x, g, a, 6, 32, 4, o, b, None), "rows_per_image", "divide")
    _refused(lambda: call(C.byref(tensor), x, g, a, 6, 32, 4, o, b, None), "rows_per_image", "divide")
    _refused(lambda: call(C.byref(gate), x, g, a, 6, 32, 3, None, None, None), "both outputs")
    _refused(lambda: call(C.byref(gate), x, g, None, 6, 32, 3, o, b, None), "addend_dev", "has_add")
    _refused(lambda: call(C.byref(_desc(add=None)), x, g, a, 6, 32, 0, o, b, None), "addend_dev", "without")
    _refused(lambda: call(C.byref(gate), None, g, a, 6, 32, 3, o, b, None), "null input")
    _refused(lambda: call(C.byref(gate), x, None, a, 6, 32, 3, o, b, None), "null input")
    _refused(lambda: call(C.byref(gate), x, g, a, 6, 32, 3, o, b + 2, None), "out_bits_dev")
    _refused(lambda: call(C.byref(_desc(activation=9)), x, g, a, 6, 32, 0, o, b, None), "unknown activation")
    _refused(lambda: amd.lib().lce_hip_mul_int8_path(C.byref(gate), 6, 32, 0, x, g, a, o, b, C.byref(L)), "rows_per_image")
    _refused(lambda: amd.lib().lce_hip_mul_int8_path(C.byref(gate), 6, 32, 3, x, g, a, o, b, None), "null")
    # zero rows or channels is a no-op, with null pointers too
    amd.check(call(C.byref(gate), None, None, None, 0, 32, 3, None, None, None))
    amd.check(call(C.byref(gate), None, None, None, 6, 0, 3, None, None, None))


def test_the_path_reports_the_layout_the_grid_and_the_add_variant():
    L = amd.MulInt8Launch()
    path = amd.lib().lce_hip_mul_int8_path
    d = _desc(per_image=True)
    want_variant = amd.add_int8_params((0.04, -5), (0.03, 1), (0.06, 2))["variant"]
    for channels, off, flat in ((64, 0, 1), (48, 0, 1), (16, 0, 1), (64, 1, 0), (40, 0, 0), (33, 0, 0)):
        amd.check(path(C.byref(d), 147, channels, 49, 0x1000 + off, 0x2000, 0x3000, 0x4000, 0x5004, C.byref(L)))
        assert (L.flat, L.waves_per_block, L.add_variant, L.mul_variant) == (flat, 4, want_variant, 1), channels
        tasks = (147 * (channels // 16) + 255) // 256 if flat else 147 * ((channels + 63) // 64)
        assert L.blocks == max(1, (tasks + 3) // 4)
    amd.check(path(C.byref(d), 256 * 56 * 56, 64, 56 * 56, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, C.byref(L)))
    assert L.blocks == 2048 and L.flat == 1                    # capped: the waves stride over the rest
    amd.check(path(C.byref(_desc(add=None)), 147, 64, 0, 0x1000, 0x2000, None, 0x4000, None, C.byref(L)))
    assert L.add_variant == -1
    for gate_off in (4, 8):                                    # the gate's pointer counts for the layout too
        amd.check(path(C.byref(d), 147, 64, 49, 0x1000, 0x2000 + gate_off, 0x3000, 0x4000, 0x5000, C.byref(L)))
        assert L.flat == 0


def test_logistic_refuses_any_other_output_quantization():
    for q_out in ((1 / 128, -128), (1 / 256, 0), (1 / 256, -127), (0.00390624, -128)):
        with pytest.raises(amd.LceHipError) as e:
            amd.logistic_int8_table((0.05, 0), q_out)
        assert e.value.code == amd.ERR_INVALID and "(1/256, -128)" in str(e.value), q_out


def test_logistic_refuses_a_bad_input_quantization():
    for q_in, name in (((0.0, 0), "in_scale"), ((float("nan"), 0), "in_scale"), ((0.1, 300), "in_zero_point")):
        with pytest.raises(amd.LceHipError) as e:
            amd.logistic_int8_table(q_in)
        assert e.value.code == amd.ERR_INVALID and name in str(e.value), q_in


def test_logistic_launch_refusals():
    call = amd.lib().lce_hip_logistic_int8
    _refused(lambda: call(0x1000, 0x2000, 3, 64, None, None, None), "both outputs")
    _refused(lambda: call(0x1000, None, 3, 64, 0x3000, None, None), "in_dev is null")
    _refused(lambda: call(None, 0x2000, 3, 64, 0x3000, None, None), "table_dev is null")
    _refused(lambda: call(0x1002, 0x2000, 3, 64, 0x3000, None, None), "table_dev")
    _refused(lambda: call(0x1000, 0x2000, 3, 1 << 22, 0x3000, None, None), "channels", "2^22")   # the chain entry's bound
    amd.check(call(None, None, 0, 64, None, None, None))


# ---- the deviation the header quotes ----

def test_mul_deviates_from_the_real_product_by_little_more_than_half_an_lsb():
    """All 65 536 pairs of 300 draws against s1 s2 (x1 - z1)(x2 - z2) / so + zo in float64, clamped the same way.  The draws'
    output scales let the products span the int8 range without sitting on its bounds: that is asserted on the reference alone.
    Measured: 0.5039 LSB.  MBQM rounds twice, but a product of two int8 differences that fits int8 has a real multiplier of a
    hundredth or less, so the first rounding is worth 2^-7 of the second's unit; held at the measured value rounded up.
    The figure is the restatement's (gate_i8_ref.mul_q): the library has no host entry that multiplies.  What ties it to the
    library is byte equality -- the parameters (test_prepare_against_the_restatement_for_300_draws, the same draws), the kernel
    bodies on the CPU (tests/test_gate_i8_hostsim.py) and the GPU (tests/test_gpu_gate_i8.py)."""
    x1, x2 = ar.all_pairs()
    worst, at_bound, total = 0.0, 0, 0
    for k, (q1, q2, qo) in enumerate(DRAWS):
        act = 0 if k % 8 else 1 + (k // 8) % 3
        ref = G.mul_q(x1, x2, q1, q2, qo, act).astype(np.int64)
        lo, hi = ar.activation_range(act, qo[0], qo[1])
        if act == 0:
            at_bound += int(np.count_nonzero((ref == lo) | (ref == hi)))
            total += ref.size
        worst = max(worst, float(np.max(np.abs(ref - G.real_mul(x1, x2, q1, q2, qo, act)))))
    print("MUL: largest deviation %.4f LSB; %.2f %% of the outputs at a clamp bound" % (worst, 100.0 * at_bound / total))
    assert at_bound < 0.10 * total
    assert worst <= 0.51


def test_logistic_deviates_from_the_real_sigmoid_by_at_most_half_an_lsb():
    """The LIBRARY's table (lce_hip_logistic_int8_prepare) against float64; the draw condition on the restatement alone."""
    worst, at_bound = 0.0, 0
    for q in LOGISTIC_DRAWS:
        ref = G.logistic_table(q).view(np.int8).astype(np.int64)
        at_bound += int(np.count_nonzero((ref == -128) | (ref == 127)))
        got = amd.logistic_int8_table(q).view(np.int8).astype(np.int64)
        worst = max(worst, float(np.max(np.abs(got - G.real_logistic(q)))))
    print("LOGISTIC: largest deviation %.4f LSB; %.2f %% at a clamp bound" % (worst, 100.0 * at_bound / (256 * len(LOGISTIC_DRAWS))))
    assert at_bound < 0.10 * 256 * len(LOGISTIC_DRAWS)
    assert worst <= 0.51


def test_the_fast_mul_variant_is_chosen_only_where_it_is_proven():
    """Every draw (real multipliers of a hundredth and less, e <= -6) takes the fast variant; a multiplier of 1/2 and above (e >= 0)
    does not meet its precondition and takes the literal one."""
    L, path = amd.MulInt8Launch(), amd.lib().lce_hip_mul_int8_path
    for q1, q2, qo in DRAWS[:60]:
        d = amd._mul_int8_desc("t", q1, q2, qo, 0, False, None)
        amd.check(path(C.byref(d), 8, 64, 0, 0x1000, 0x2000, None, 0x4000, None, C.byref(L)))
        assert L.mul_variant == 1 and amd.mul_int8_params(q1, q2, qo)["shift"] <= -1
    for so, variant in ((0.08, 0), (0.3, 0), (0.6, 1)):
        d = amd._mul_int8_desc("t", (0.5, 3), (0.5, -4), (so, 5), 0, False, None)
        amd.check(path(C.byref(d), 8, 64, 0, 0x1000, 0x2000, None, 0x4000, None, C.byref(L)))
        assert L.mul_variant == variant, so
