"""The int8 elementwise chain (lce_hip_elementwise_i8) on the CPU: lce_hip_elementwise_i8_prepare's table against the NumPy
restatement of the header's arithmetic (tests/elementwise_i8_ref.py) for all 256 inputs of every channel, every refusal with its
message, each step kind against the real-valued result, and the launch geometry the entry reports.  The kernels run in
tests/test_elementwise_i8_hostsim.py (CPU) and tests/test_gpu_elementwise_i8.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import elementwise_i8_ref as E

amd = importlib.import_module("compute-engine_amd")

KINDS = ("add", "prelu", "clamp", "requantize")
# The largest |integer result - real-valued result| of one step alone, in LSB of the step's output, measured by
# test_one_step_against_the_real_valued_result over its draws (0.5000, 0.7498, 0.7495, 0.7497) and quoted in include/lce_hip.h: the
# ADD rounds once at a precision of 2^-20 LSB and once at the end; MBQM rounds the doubling high product and then the shift, which
# can stack a half and a quarter.
MEASURED_LSB = {"add": 0.51, "prelu": 0.75, "clamp": 0.75, "requantize": 0.75}


def test_the_symbols_are_exported():
    """Fails without the feature: none of the symbols exists there."""
    for name in ("lce_hip_elementwise_i8_check", "lce_hip_elementwise_i8_table_size", "lce_hip_elementwise_i8_prepare",
                 "lce_hip_elementwise_i8", "lce_hip_elementwise_i8_path", "lce_hip_elementwise_i8_forced"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    assert amd.lib().lce_hip_abi_version() == 3
    assert C.sizeof(amd.EwI8Step) == 48 and C.sizeof(amd.EwI8Desc) == 40 + 8 * 48 + 8


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _chains():
    """A few hundred seeded chains: 1 to 8 steps, per-channel and scalar-only, every kind and activation."""
    g = np.random.default_rng(20260)
    out = []
    for n in range(260):
        channels = int(g.choice([1, 3, 8, 17]))
        steps_n = 1 if n % 5 == 0 else 8 if n % 5 == 1 else int(g.integers(2, 8))
        per_channel = n % 4 != 3
        out.append((channels, per_channel) + E.draw_chain(g, channels, steps_n, per_channel))
    return out


CHAINS = _chains()


def test_the_draws_cover_what_they_must():
    zps, acts, es, alphas, lengths, scalar_only = set(), set(), set(), set(), set(), 0
    for channels, per_channel, q_in, steps in CHAINS:
        lengths.add(len(steps))
        scalar_only += not per_channel
        q = q_in
        zps.add(q[1])
        for st in steps:
            if st[0] == "add":
                acts.add(st[4]); zps.add(st[3][1]); q = st[3]
            elif st[0] == "prelu":
                (_, e1), (_, e2) = E.step_multipliers("prelu", q[0], st[3][0], st[2][0])
                es.add(np.sign(e1))
                a = np.atleast_1d(np.asarray(st[1], np.int64)) - st[2][1]
                alphas |= {int(np.sign(v)) for v in a}
                q = st[3]
            else:
                ((_, e),) = E.step_multipliers(st[0], q[0], st[1][0])
                es.add(np.sign(e))
                if st[0] == "clamp":
                    acts.add(st[2])
                q = st[1]
            zps.add(q[1])
    assert {-128, 127} <= zps and acts == {0, 1, 2, 3} and {-1, 1} <= es and alphas == {-1, 0, 1}
    assert {1, 8} <= lengths and scalar_only >= 50


def test_the_table_equals_the_restatement_for_every_input_of_every_channel():
    for channels, per_channel, q_in, steps in CHAINS:
        got = amd.elementwise_i8_prepare(channels, q_in, steps)
        want = E.table(channels, q_in, steps)
        assert got.shape == want.shape and got.shape[0] == (channels if any(np.ndim(s[1]) > 0 for s in steps if s[0] in ("add", "prelu")) else 1)
        assert np.array_equal(got, want), (channels, q_in, steps)
        if not per_channel:
            assert got.shape[0] == 1


def test_a_head_does_not_change_the_table_but_moves_its_input_quantization():
    g = np.random.default_rng(5)
    q_in, head, steps = E.reactnet_tail(g, 8)
    with_head = amd.elementwise_i8_prepare(8, q_in, steps, head=head)
    assert np.array_equal(with_head, E.table(8, head[1], steps))
    assert np.array_equal(with_head, amd.elementwise_i8_prepare(8, head[1], steps))


# ---- one step against real arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_step_against_the_real_valued_result(kind):
    g = np.random.default_rng(KINDS.index(kind))
    v = np.arange(-128, 128, dtype=np.int64)[:, None]
    worst = 0.0
    for _ in range(300):
        q_in = (E._scale(g), E._zp(g))
        st = E.draw_step(g, kind, q_in, 4, True)
        got = amd.elementwise_i8_prepare(4, q_in, [st])
        got = (got.view(np.int8).T if got.shape[0] == 4 else np.repeat(got.view(np.int8).T, 4, 1)).astype(np.float64)
        real = E.real_step(np.broadcast_to(v, (256, 4)), st, q_in)
        worst = max(worst, float(np.abs(got - real).max()))
    print("largest deviation of %s: %.4f LSB" % (kind, worst))
    assert worst <= MEASURED_LSB[kind]


# ---- the refusals -------------------------------------------------------------------------------------------------------------------
Q = (0.05, 3)
GOOD = {"add": ("add", np.int8(5), (0.04, 1), (0.07, -2), 0), "prelu": ("prelu", np.int8(7), (0.01, 0), (0.05, 1)),
        "clamp": ("clamp", (0.05, 0), 1), "requantize": ("requantize", (0.03, 4))}


def _refused(desc, *words, entry="check", table=None):
    lib = amd.lib()
    if entry == "check":
        code = lib.lce_hip_elementwise_i8_check(C.byref(desc))
    else:
        buf = np.zeros((max(desc.channels, 1), 256), np.uint8) if table is None else table
        code = lib.lce_hip_elementwise_i8_prepare(C.byref(desc), buf.ctypes.data)
    msg = lib.lce_hip_last_error().decode()
    assert code == amd.ERR_INVALID, (code, msg)
    for w in words:
        assert w in msg, (w, msg)


def _desc(steps, q_in=Q, head=None, channels=4):
    return amd._ew_i8_desc("test", channels, q_in, steps, head)


def test_the_good_steps_pass():
    for kind in KINDS:
        d, keep = _desc([GOOD[kind]])
        assert amd.lib().lce_hip_elementwise_i8_check(C.byref(d)) == amd.OK, amd.lib().lce_hip_last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_a_bad_scale_or_zero_point_names_the_step(kind):
    op = kind.upper()
    for field, value, word in (("out_scale", 0.0, "out_scale"), ("out_scale", float("inf"), "out_scale"), ("out_scale", float("nan"), "out_scale"),
                               ("out_zero_point", 128, "out_zero_point"), ("out_zero_point", -129, "out_zero_point")):
        d, keep = _desc([GOOD["clamp"], GOOD[kind]])
        setattr(d.steps[1], field, value)
        _refused(d, "step 2 (%s)" % op, word)
    if kind in ("add", "prelu"):
        for field, value in (("operand_scale", -1.0), ("operand_zero_point", 200)):
            d, keep = _desc([GOOD[kind]])
            setattr(d.steps[0], field, value)
            _refused(d, "step 1 (%s)" % op, field)


def test_the_input_and_the_head_are_checked():
    d, keep = _desc([GOOD["clamp"]])
    d.in_scale = 0.0
    _refused(d, "in_scale")
    d, keep = _desc([GOOD["clamp"]])
    d.in_zero_point = 300
    _refused(d, "in_zero_point")
    d, keep = _desc([GOOD["clamp"]], head=((0.04, 0), (0.07, 0), 0))
    d.addend_zero_point = -200
    _refused(d, "head", "in2_zero_point")
    # the head's output multiplier 2 max(s1, s2) / (2^20 so) must be below 1
    d, keep = _desc([GOOD["clamp"]], head=((0.04, 0), (1e-8, 0), 0))
    _refused(d, "head", "real multiplier", "(0, 1)")
    d, keep = _desc([GOOD["clamp"]], head=((0.04, 0), (0.07, 0), 0))
    d.head_activation = 7
    _refused(d, "head", "activation")
    d, keep = _desc([GOOD["clamp"]])
    d.has_head = 2
    _refused(d, "has_head")


def test_an_add_multiplier_outside_the_unit_interval_is_refused_as_the_residual_add_refuses_it():
    d, keep = _desc([("add", np.int8(1), (0.04, 0), (1e-8, 0), 0)])
    _refused(d, "step 1 (ADD)", "real multiplier", "(0, 1)")
    p = amd.AddInt8Params()
    assert amd.lib().lce_hip_add_int8_prepare(C.byref(amd.AddInt8Desc(Q[0], Q[1], 0.04, 0, 1e-8, 0, 0)), C.byref(p)) == amd.ERR_INVALID


def test_an_activation_on_prelu_or_requantize_is_refused():
    for kind in ("prelu", "requantize"):
        d, keep = _desc([GOOD[kind]])
        d.steps[0].activation = amd.ACT_RELU
        _refused(d, "step 1 (%s)" % kind.upper(), "activation must be NONE")
    d, keep = _desc([GOOD["add"]])
    d.steps[0].activation = 4
    _refused(d, "step 1 (ADD)", "unknown activation")


def test_reserved_fields_step_counts_ops_and_operand_kinds():
    d, keep = _desc([GOOD["add"]])
    d.reserved[1] = 1
    _refused(d, "reserved")
    d, keep = _desc([GOOD["add"], GOOD["prelu"]])
    d.steps[1].reserved[0] = 1
    _refused(d, "step 2 (PRELU)", "reserved")
    for n in (0, 9, -1):
        d, keep = _desc([GOOD["clamp"]])
        d.num_steps = n
        _refused(d, "num_steps must be 1..8")
    # a head alone is the residual ADD's job
    d, keep = _desc([GOOD["clamp"]], head=((0.04, 0), (0.07, 0), 0))
    d.num_steps = 0
    _refused(d, "num_steps", "lce_hip_add_int8")
    d, keep = _desc([GOOD["clamp"]])
    d.steps[0].op = 4
    _refused(d, "step 1", "unknown op")
    d, keep = _desc([GOOD["clamp"]])
    d.steps[0].operand = amd.EW_PER_CHANNEL
    _refused(d, "step 1 (CLAMP)", "operand")
    d, keep = _desc([GOOD["add"]])
    d.steps[0].operand = amd.EW_TENSOR
    _refused(d, "step 1 (ADD)", "operand")
    d, keep = _desc([GOOD["clamp"]])
    d.channels = -1
    _refused(d, "channels")
    assert amd.lib().lce_hip_elementwise_i8_check(None) == amd.ERR_INVALID


def test_an_intermediate_that_could_leave_int32_is_refused():
    # si / so = 2^24: (v - zi) * 2^25 with |v - zi| up to 255 does not fit
    for kind in ("clamp", "requantize", "prelu"):
        st = {"clamp": ("clamp", (2.0 ** -24, 0), 0), "requantize": ("requantize", (2.0 ** -24, 0)),
              "prelu": ("prelu", np.int8(1), (1.0, 0), (2.0 ** -24, 0))}[kind]
        d, keep = _desc([st], q_in=(1.0, 0))
        _refused(d, "step 1 (%s)" % kind.upper(), "could leave int32")
    # 255 * 2^23 fits, 255 * 255 * 2^23 (the negative side of a PRELU whose alpha scale is 1) does not
    d, keep = _desc([("requantize", (2.0 ** -22, 0))], q_in=(1.0, 0))
    assert amd.lib().lce_hip_elementwise_i8_check(C.byref(d)) == amd.OK
    d, keep = _desc([("prelu", np.int8(1), (1.0, 0), (2.0 ** -16, 0))], q_in=(1.0, 0))
    _refused(d, "step 1 (PRELU)", "could leave int32")
    # a real multiplier that float32 cannot hold
    d, keep = _desc([("clamp", (1e-30, 0), 0)], q_in=(1e30, 0))
    _refused(d, "step 1 (CLAMP)", "real multiplier")


def test_prepare_needs_its_pointers_and_check_does_not_read_them():
    d, keep = _desc([GOOD["add"]])
    d.steps[0].values = None
    assert amd.lib().lce_hip_elementwise_i8_check(C.byref(d)) == amd.OK
    _refused(d, "step 1 (ADD)", "null values", entry="prepare")
    d, keep = _desc([GOOD["clamp"]])
    assert amd.lib().lce_hip_elementwise_i8_prepare(C.byref(d), None) == amd.ERR_INVALID
    n = C.c_size_t()
    assert amd.lib().lce_hip_elementwise_i8_table_size(C.byref(d), C.byref(n)) == amd.OK and n.value == 256
    d, keep = _desc([GOOD["clamp"], ("add", np.arange(4, dtype=np.int8), (0.04, 1), (0.07, -2), 0)])
    assert amd.lib().lce_hip_elementwise_i8_table_size(C.byref(d), C.byref(n)) == amd.OK and n.value == 4 * 256


def test_the_python_wrapper_checks_shapes_without_a_device():
    x = np.zeros((2, 3, 8), np.int8)
    t = np.zeros((1, 256), np.uint8)
    steps = [GOOD["clamp"]]
    for bad in (dict(x=x.astype(np.float32)), dict(table=np.zeros((2, 256), np.uint8)), dict(table=t.astype(np.int8)),
                dict(addend=x), dict(head=((0.1, 0), (0.2, 0))), dict(out=False), dict(out=np.zeros((2, 3, 9), np.int8)),
                dict(out_bits=np.zeros((2, 3, 2), np.int32))):
        kw = dict(x=x, table=t, q_in=Q, steps=steps)
        kw.update(bad)
        with pytest.raises(ValueError):
            amd.elementwise_i8(**kw)
    for steps_bad in ([("relu", (0.1, 0), 0)], [("clamp", (0.1, 0))], [("add", np.zeros(3, np.int8), (0.1, 0), (0.1, 0), 0)],
                      [GOOD["clamp"]] * 9, [("prelu", 300, (0.1, 0), (0.1, 0))]):
        with pytest.raises(ValueError):
            amd.elementwise_i8_prepare(8, Q, steps_bad)


# ---- the launch the entry reports ----------------------------------------------------------------------------------------------------
def _launch(channels, rows, steps, forced=-1, align=(0, 0, 0), head=None):
    d, keep = _desc(steps, head=head, channels=channels)
    L = amd.EwI8Launch()
    base = 1 << 20
    code = amd.lib().lce_hip_elementwise_i8_path(C.byref(d), rows, base + align[0], None if head is None else base, base, base + align[1],
                                                 base + 4 * align[2], forced, C.byref(L))
    return code, {n: int(getattr(L, n)) for n, _ in amd.EwI8Launch._fields_}


def test_the_paths_the_entry_takes_and_refuses():
    per = lambda c: [("add", np.zeros(c, np.int8), (0.04, 1), (0.07, -2), 0)]
    code, L = _launch(128, 1000, per(128))
    assert code == amd.OK and (L["path"], L["flat"], L["table_rows"], L["lds_bytes"], L["head_variant"]) == (amd.EW_I8_PATH_LDS, 1, 128, 128 * 260, -1)
    assert L["lds_max_channels"] == 608 and L["waves_per_block"] == 16
    code, L = _launch(608, 1000, per(608))
    assert (L["path"], L["blocks"], L["waves_per_block"]) == (amd.EW_I8_PATH_LDS, 10, 16)
    # below 128 channels and beyond what fits: the global path (profiles/elementwise_i8/chains.txt)
    for c in (32, 64, 96, 127, 640, 1024):
        code, L = _launch(c, 1000, per(c))
        assert (L["path"], L["flat"], L["lds_bytes"], L["waves_per_block"]) == (amd.EW_I8_PATH_GLOBAL, int(c % 32 == 0), 0, 4), c
    code, L = _launch(32, 1000, per(32), forced=amd.EW_I8_PATH_LDS)
    assert L["waves_per_block"] == 4 and L["lds_bytes"] == 32 * 260
    code, L = _launch(128, 1000, per(128), align=(1, 0, 0))
    assert (L["path"], L["flat"], L["lds_max_channels"]) == (amd.EW_I8_PATH_LDS, 0, 630)
    code, L = _launch(630, 1000, per(630))
    assert (L["path"], L["flat"]) == (amd.EW_I8_PATH_LDS, 0)
    code, L = _launch(64, 1000, [GOOD["clamp"]])
    assert (L["path"], L["table_rows"], L["lds_bytes"]) == (amd.EW_I8_PATH_ONE_ROW, 1, 256)
    # forced: the LDS path up to what fits, ONE_ROW for one row only, LDS / GLOBAL for a row per channel only
    assert _launch(608, 10, per(608), forced=amd.EW_I8_PATH_LDS)[0] == amd.OK
    assert _launch(640, 10, per(640), forced=amd.EW_I8_PATH_LDS)[0] == amd.ERR_INVALID
    assert "608" in amd.lib().lce_hip_last_error().decode()
    assert _launch(630, 10, per(630), forced=amd.EW_I8_PATH_LDS)[0] == amd.OK
    assert _launch(631, 10, per(631), forced=amd.EW_I8_PATH_LDS)[0] == amd.ERR_INVALID
    assert _launch(64, 10, per(64), forced=amd.EW_I8_PATH_ONE_ROW)[0] == amd.ERR_INVALID
    assert _launch(64, 10, [GOOD["clamp"]], forced=amd.EW_I8_PATH_GLOBAL)[0] == amd.ERR_INVALID
    assert _launch(64, 10, per(64), forced=3)[0] == amd.ERR_INVALID
    # a table that is not 4-byte aligned
    d, keep = _desc(per(64), channels=64)
    L = amd.EwI8Launch()
    assert amd.lib().lce_hip_elementwise_i8_path(C.byref(d), 10, 1 << 20, None, (1 << 20) + 2, 1 << 20, None, -1, C.byref(L)) == amd.ERR_INVALID
    # a head reports the variant the residual ADD has proven for its parameters
    code, L = _launch(64, 1000, per(64), head=((0.05, 1), (0.05, 2), 0))
    want = amd.add_int8_params(Q, (0.05, 1), (0.05, 2))["variant"]
    assert code == amd.OK and L["head_variant"] == want


def test_zero_rows_or_channels_is_a_no_op_and_null_pointers_are_refused_before_any_device_call():
    d, keep = _desc([GOOD["clamp"]], channels=8)
    lib = amd.lib()
    assert lib.lce_hip_elementwise_i8(C.byref(d), None, None, None, 0, None, None, None) == amd.OK
    d0, keep0 = _desc([GOOD["clamp"]], channels=0)
    assert lib.lce_hip_elementwise_i8(C.byref(d0), None, None, None, 5, None, None, None) == amd.OK
    assert lib.lce_hip_elementwise_i8(C.byref(d), 1 << 20, None, 1 << 20, 5, None, None, None) == amd.ERR_INVALID
    assert "both outputs" in lib.lce_hip_last_error().decode()
    assert lib.lce_hip_elementwise_i8(C.byref(d), None, None, 1 << 20, 5, 1 << 20, None, None) == amd.ERR_INVALID
    assert lib.lce_hip_elementwise_i8(C.byref(d), 1 << 20, 1 << 20, 1 << 20, 5, 1 << 20, None, None) == amd.ERR_INVALID
    assert "addend" in lib.lce_hip_last_error().decode()
    assert lib.lce_hip_elementwise_i8_forced(C.byref(d), -1, 1 << 20, None, 1 << 20, 5, 1 << 20, None, None) == amd.ERR_INVALID
