"""Standalone activations, RESHAPE and the per-image gate without a GPU: the accuracy of the stated LOGISTIC against float64; the
real bodies of csrc/lce_kernels_eltwise.h on the CPU (tests/hostsim_eltwise) against tests/activation_ref.py byte for byte; the
reader's six builtin codes; the three predicates of lce_tflite_model_open_passes, one refusal per file; the partition with and
without the new names; the Python keywords; and the refusals of lce_hip_elementwise_ex, which need no device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import activation_models as AM
import activation_ref as AR
import hostsim_eltwise_lib as HS
import oracle_lib as O
import partition_ref as PR
from section_models import _sections_of
from test_head_sections_host import open_passes, release
from tflite_writer import ModelBuilder, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

# The largest error of the stated LOGISTIC against float64 1 / (1 + exp(-x)), in ulps of the float32 result: measured 2.40 on
# 1.8e8 samples, plus 1 ulp for the points no sample met.
LOGISTIC_MAX_ULP = 2.40 + 1.0
FLT_MAX = np.float32(3.4028234663852886e38)
NONE, RELU, RELU_N1_TO_1, RELU6 = range(4)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---- LOGISTIC: the statement -----------------------------------------------------------------------------------------------------
def logistic_ulps(x, y):
    """|y - sigmoid(x)| in ulps of the float32 nearest sigmoid(x) (the subnormal spacing below the smallest normal)."""
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        ref = np.where(x64 >= 0, 1 / (1 + np.exp(-x64)), np.exp(x64) / (1 + np.exp(x64)))
    r32 = np.abs(ref.astype(np.float32))
    ulp = np.where(r32 < 2.0 ** -126, 2.0 ** -149, np.spacing(np.maximum(r32, np.float32(2.0 ** -126))).astype(np.float64))
    return np.abs(y.astype(np.float64) - ref) / ulp


def logistic_samples(n, seed):
    g = np.random.default_rng(seed)
    return [a.astype(np.float32) for a in (g.uniform(-110, 110, n), g.standard_normal(n) * 3, g.standard_normal(n) * 1e-3, g.uniform(-12, 0, n))]


def test_the_stated_logistic_is_within_its_measured_error_of_float64():
    """The NumPy restatement on 1.2 M samples and the kernel's own function (the host simulation's) on 16 M."""
    worst = 0.0
    for x in logistic_samples(300_000, 1):
        worst = max(worst, logistic_ulps(x, AR.logistic(x)).max())
    for x in logistic_samples(4_000_000, 2):
        worst = max(worst, logistic_ulps(x, HS.sim_logistic(x)).max())
    print("largest LOGISTIC error: %.3f ulp" % worst)
    assert worst <= LOGISTIC_MAX_ULP


def test_the_kernels_logistic_is_the_restatement_byte_for_byte():
    x = np.concatenate(logistic_samples(250_000, 3))
    assert same(HS.sim_logistic(x), AR.logistic(x))


def test_logistic_at_its_edges():
    below, above = np.nextafter(np.float32(-104), np.float32(-200)), np.nextafter(np.float32(-104), np.float32(0))
    nan = np.array([0x7FC01234, 0xFFC00001], np.uint32).view(np.float32)
    x = np.array([0.0, -0.0, 104, -104, below, above, 88.7, -88.7, np.inf, -np.inf, 1e-40, -1e-40, FLT_MAX, -FLT_MAX, -100], np.float32)
    for f in (AR.logistic, HS.sim_logistic):
        y = f(x)
        assert y[0] == 0.5 and y[1] == 0.5 and y[2] == 1 and y[6] == 1 and y[8] == 1 and y[12] == 1
        assert y[3] == 0 and y[5] == 0                                          # (exp(-104) is below half the smallest subnormal)
        assert 0 < y[14] < 2.0 ** -126                                          # exp(-100) is a subnormal: nothing is flushed
        for k in (4, 9, 13):
            assert y[k] == 0 and not np.signbit(y[k])                           # x < -104 and -inf give +0
        assert y[10] == 0.5 and y[11] == 0.5 and 0 < y[7] < 1e-38
        assert np.array_equal(f(nan).view(np.uint32), nan.view(np.uint32))      # a NaN passes unchanged
    assert same(AR.logistic(x), HS.sim_logistic(x))


def test_prelu_and_clamp_on_special_values():
    sub = np.float32(1e-40)
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, sub, -sub, FLT_MAX, -FLT_MAX, 1.5, -1.5, 7.0], np.float32)
    for alpha in (-2.0, 0.0, 3.0, 0.25):
        y = AR.prelu(x, np.float32(alpha))
        assert np.signbit(y[1]) and y[1] == 0 and not np.signbit(y[0]) and np.isnan(y[2]) and y[3] == np.inf
        assert same(y[[5, 7, 9, 11]], x[[5, 7, 9, 11]])
        with np.errstate(over="ignore", invalid="ignore"):
            assert same(y[[4, 6, 8, 10]], (x[[4, 6, 8, 10]] * np.float32(alpha)).astype(np.float32))
    y = AR.clamp(x, RELU)
    assert np.signbit(y[1]) and y[1] == 0 and np.isnan(y[2]) and y[3] == FLT_MAX and y[4] == 0 and y[6] == 0 and y[5] == sub
    y = AR.clamp(x, RELU6)
    assert y[11] == 6 and y[7] == 6 and y[9] == 1.5 and y[10] == 0
    y = AR.clamp(x, RELU_N1_TO_1)
    assert y[9] == 1 and y[10] == -1 and y[6] == -sub and np.isnan(y[2])


# ---- the kernel bodies on the CPU ------------------------------------------------------------------------------------------------
def operands(shape, seed, special=True):
    g = np.random.default_rng(seed)
    C = shape[-1]
    x = (g.standard_normal(shape) * 3).astype(np.float32)
    if special:
        flat = x.reshape(-1)
        for k, v in enumerate((0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, FLT_MAX, -FLT_MAX, -104.0, 88.7)):
            flat[g.integers(0, flat.size, max(1, flat.size // 97))] = np.float32(v)
    return dict(x=x, gate=g.uniform(-1, 2, (shape[0],) + (1,) * (len(shape) - 2) + (C,)).astype(np.float32),
                alpha=g.choice([-1.5, 0.0, 0.25, 2.0], C).astype(np.float32), shift=g.standard_normal(C).astype(np.float32),
                res=g.standard_normal(shape).astype(np.float32), m=g.uniform(0.5, 1.5, C).astype(np.float32))


def programs(o):
    return {
        "add_gate": [("add", o["gate"], NONE)],
        "mul_gate_relu": [("mul", o["gate"], RELU)],
        "clamp_relu": [("clamp", None, RELU)],
        "clamp_n1": [("clamp", None, RELU_N1_TO_1)],
        "clamp_relu6": [("clamp", None, RELU6)],
        "prelu_channel": [("prelu", o["alpha"], NONE)],
        "prelu_scalar": [("prelu", -0.75, NONE)],
        "logistic": [("logistic", None, NONE)],
        "rprelu": [("add", o["shift"], NONE), ("prelu", o["alpha"], NONE), ("add", o["m"], NONE)],
        "old_kinds": [("mul", o["m"], NONE), ("add", o["shift"], NONE), ("add", o["res"], RELU), ("mul", 0.5, NONE)],
        "eight": [("mul", o["m"], NONE), ("add", o["shift"], NONE), ("add", o["res"], NONE), ("prelu", o["alpha"], NONE),
                  ("mul", o["gate"], NONE), ("logistic", None, NONE), ("add", -0.5, NONE), ("clamp", None, RELU_N1_TO_1)],
    }


# (shape, grid cap, offset in floats): the flat path with 1, 2 and 3 words per row, an image smaller than a wave's iteration (96
# floats) and larger than one, totals that end in a partial block of 32 words, grids so small that every wave iterates; the row
# path at ragged channel counts, and at 32 channels through pointers 4 bytes off
FLAT = [((37, 1, 3, 32), 1, 0), ((3, 7, 7, 64), 2, 0), ((5, 3, 5, 96), 1, 0), ((2, 9, 9, 96), 3, 0), ((70, 1, 1, 32), 1, 0), ((1, 33, 37, 64), 2048, 0)]
ROWS = [((3, 5, 5, 1), 1, 0), ((4, 3, 3, 31), 2, 0), ((4, 3, 3, 33), 2, 0), ((3, 2, 4, 70), 1, 0), ((2, 5, 3, 129), 2, 0), ((5, 3, 3, 32), 1, 1)]


@pytest.mark.parametrize("shape,cap,offset", FLAT + ROWS)
def test_the_kernel_bodies_match_the_restatement(shape, cap, offset):
    o = operands(shape, sum(shape) + cap)
    for name, steps in programs(o).items():
        want = AR.chain(o["x"], steps)
        out, bits, flat = HS.sim_chain(o["x"], steps, cap=cap, offset=offset)
        assert flat == ((shape, cap, offset) in FLAT), name
        assert same(out, want), (name, shape)
        assert np.array_equal(bits, O.bitpack(want)), (name, shape)                  # (padding bits of a ragged row: 0)
    steps = programs(o)["eight"]
    want = AR.chain(o["x"], steps)
    only_bits = HS.sim_chain(o["x"], steps, want_out=False, cap=cap, offset=offset)
    assert only_bits[0] is None and np.array_equal(only_bits[1], O.bitpack(want))
    only_float = HS.sim_chain(o["x"], steps, want_bits=False, cap=cap, offset=offset)
    assert only_float[1] is None and same(only_float[0], want)
    in_place = HS.sim_chain(o["x"], steps, cap=cap, offset=offset, in_place=True)
    assert same(in_place[0], want) and np.array_equal(in_place[1], O.bitpack(want))


@pytest.mark.parametrize("shape,cap,offset", [FLAT[1], FLAT[2], ROWS[2], ROWS[5]])
def test_the_old_step_kinds_give_the_old_instances_bytes(shape, cap, offset):
    """ADD / MUL with a scalar, per-channel or tensor operand: the instance lce_hip_elementwise_ex launches against the one
    lce_hip_elementwise launches."""
    o = operands(shape, 5)
    steps = programs(o)["old_kinds"]
    new, old = HS.sim_chain(o["x"], steps, cap=cap, offset=offset, ex=1), HS.sim_chain(o["x"], steps, cap=cap, offset=offset, ex=0)
    assert same(new[0], old[0]) and np.array_equal(new[1], old[1]) and same(new[0], AR.chain(o["x"], steps))


def test_the_extended_kernels_use_no_scratch_and_no_lds():
    """The unit of lce_hip_elementwise_ex emits exactly the two extended instances, without scratch memory, LDS or spills; the unit
    of lce_hip_elementwise still emits its own two (tests/test_elementwise_sections_host.py)."""
    import hipcc_lib as H
    kernels, resources, _, mnemonics = H.compile_unit("lce_tu_eltwise_ex.hip")
    assert len(kernels) == 2 and all("eltwise" in k and "Li1E" in k for k in kernels), kernels
    for key in H.RESOURCE_KEYS:
        assert resources[key] == ["0", "0"], (key, resources[key])
    # one rounding per op outside the stated exp: plain adds and multiplies are there, and the division is the full one
    assert {"v_add_f32_e32", "v_mul_f32_e32", "v_div_scale_f32", "v_div_fixup_f32"} <= mnemonics


# ---- the entry's refusals: before any device call ----------------------------------------------------------------------------------
def _step(op, operand=0, values=None, scalar=0.0, activation=0, reserved=(0, 0)):
    return amd.EwStepEx(op, operand, values, scalar, activation, (C.c_int32 * 2)(*reserved))


def test_the_entry_refuses_before_any_device_call():
    """(No device here: a call that passed its checks would fail with another code, LCE_HIP_ERR_RUNTIME / no device.)"""
    lib = amd.lib()
    a, g = 0x1000, 0x2000                                      # (never dereferenced: every call below is refused)
    def call(steps, rows=6, channels=32, rpi=3, x=a, out=a, bits=None, n=None):
        arr = (amd.EwStepEx * max(1, len(steps)))(*steps)
        return lib.lce_hip_elementwise_ex(x, rows, channels, rpi, arr if steps else None, len(steps) if n is None else n, out, bits, None)
    ok = _step(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, g)
    cases = {
        "num_steps": call([ok], n=0), "num_steps ": call([ok] * 8, n=9), "null steps": lib.lce_hip_elementwise_ex(a, 6, 32, 3, None, 1, a, None, None),
        "unknown op": call([_step(5)]), "unknown op ": call([_step(-1)]), "unknown operand": call([_step(amd.EW_ADD, 4, g)]),
        "unknown activation": call([_step(amd.EW_CLAMP, activation=4)]), "reserved": call([_step(amd.EW_CLAMP, reserved=(0, 1))]),
        "PRELU's alpha": call([_step(amd.EW_PRELU, amd.EW_TENSOR, g)]), "PRELU's alpha ": call([_step(amd.EW_PRELU, amd.EW_PER_IMAGE_CHANNEL, g)]),
        "no activation": call([_step(amd.EW_LOGISTIC, activation=1)]), "no activation ": call([_step(amd.EW_PRELU, scalar=0.5, activation=3)]),
        "does not divide": call([ok], rows=7, rpi=3), "needs rows_per_image": call([ok], rpi=0),
        "null operand": call([_step(amd.EW_MUL, amd.EW_PER_IMAGE_CHANNEL, None)]), "null operand ": call([_step(amd.EW_PRELU, amd.EW_PER_CHANNEL, None)]),
        "both outputs": call([ok], out=None), "null input": call([ok], x=None),
        "4-byte aligned": call([ok], x=a + 2), "4-byte aligned ": call([_step(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, g + 1)]),
        "4-byte aligned  ": call([ok], bits=a + 6),
    }
    for what, rc in cases.items():
        assert rc == amd.ERR_INVALID, what
    assert call([_step(amd.EW_PRELU, amd.EW_TENSOR, g)]) == amd.ERR_INVALID and b"PRELU" in lib.lce_hip_last_error()
    assert call([ok], rows=7, rpi=3) == amd.ERR_INVALID and b"does not divide" in lib.lce_hip_last_error()
    # zero rows or channels is a no-op, checked after the steps and before the pointers
    assert call([ok], rows=0, x=None, out=None) == amd.OK and call([ok], channels=0, x=None, out=None) == amd.OK
    assert call([_step(9)], rows=0) == amd.ERR_INVALID
    assert lib.lce_hip_elementwise_grid_cap() == 2048
    assert lib.lce_hip_abi_version() == 3
    for name in ("lce_hip_elementwise_ex", "lce_hip_elementwise_grid_cap", "lce_hip_memcpy_d2d"):
        assert name in amd.ABI_SYMBOLS and hasattr(lib, name)


def test_the_python_wrapper_checks_shapes_without_a_device():
    x = np.zeros((2, 3, 3, 8), np.float32)
    assert amd._ew_ex_check(x, [("mul", np.zeros((2, 1, 1, 8), np.float32), 0), ("prelu", np.zeros(8, np.float32), 0), ("add", x, 1),
                                ("logistic", None, 0), ("clamp", None, 3), ("add", 1.0, 0)], None, True) == [3, 1, 2, 0, 0, 0]
    for steps in ([("prelu", x, 0)], [("logistic", None, 1)], [("clamp", 1.0, 0)], [("mul", np.zeros((2, 8), np.float32), 0)], [("tanh", None, 0)],
                  [("add", None, 0)], []):
        with pytest.raises(ValueError):
            amd._ew_ex_check(x, steps, None, None)


# ---- the reader and the partition ------------------------------------------------------------------------------------------------
def test_the_six_builtin_codes_round_trip():
    b = ModelBuilder()
    t = [b.tensor([1, 2, 2, 4], np.float32, "t%d" % k) for k in range(7)]
    alpha = b.tensor([4], np.float32, "alpha", np.ones(4, np.float32))
    shape = b.tensor([4], np.int32, "shape", np.array([1, 2, 2, 4], np.int32))
    codes = [AM.LOGISTIC, AM.RELU_OP, AM.RELU_N1_TO_1_OP, AM.RELU6_OP, AM.RESHAPE, AM.PRELU]
    for k, code in enumerate(codes):
        b.builtin_op(code, [t[k]] + ([alpha] if code == AM.PRELU else [shape] if code == AM.RESHAPE else []), [t[k + 1]])
    b.inputs, b.outputs = [t[0]], [t[6]]
    model = mr.LceModel(b.finish())
    assert [o.builtin_code for o in model.operators] == [14, 19, 20, 21, 22, 54] == codes
    assert [len(o.inputs) for o in model.operators] == [1, 1, 1, 1, 2, 2] and model.sections == []
    # with `stem` the chain of standalone operators is one section, whatever stands at its head
    model = mr.LceModel(b.finish(), stem_sections=True, **AM.NEW_KEYWORDS)
    assert [(s.ops, s.inputs, s.outputs) for s in model.sections] == [(list(range(6)), [t[0]], [t[6]])]


def test_open_passes_knows_the_three_names_and_still_refuses_the_rest():
    data = AM.gated_model()[0]
    lib = mr.tflite_lib()
    for passes in (b"activation", b"reshape", b"gate", b"gate,activation,reshape", ",".join(AM.OLD_NAMES + AM.NEW_NAMES).encode()):
        h, err, _ = open_passes(data, passes)
        assert h, err
        lib.lce_tflite_model_close(h)
    for passes, offender in ((b"activations", b"'activations'"), (b"gate,gates", b"'gates'"), (b"reshape,head,reshape", b"'reshape'"),
                             (b"activation,activation", b"'activation'"), (b"gate,", b"''"), (b"Gate", b"'Gate'"), (b"gate,elementwise,gate", b"'gate'")):
        h, msg, _ = open_passes(data, passes)
        assert not h and offender in msg and (b"unknown" in msg or b"twice" in msg), (passes, msg)


@pytest.mark.parametrize("fixture", ["reactnet", "gated", "flatten"])
def test_without_the_new_names_the_networks_partition_as_before(fixture):
    """Every old name given: the sections are what tests/partition_ref.py derives with the new operators as the host's."""
    data, x, out, info = dict(reactnet=AM.reactnet_model, gated=AM.gated_model, flatten=AM.flatten_head_model)[fixture]()
    model = mr.LceModel(data, **AM.OLD_KEYWORDS)
    ops, constants, outputs = AM.graph_of(model)
    want = PR.partition(ops, info["kinds"], constants, outputs, stem=True)
    assert [(s.ops, s.inputs, s.outputs) for s in model.sections] == want and len(want) >= 1
    assert not mr.Interpreter(model).lce_only
    h, err, keep = open_passes(data, ",".join(AM.OLD_NAMES).encode(), at_page_end=True)
    assert h and _sections_of(h) == want, err
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    # and no other entry reaches the new operators: with nothing named the sections hold LCE operators only
    for s in mr.LceModel(data).sections:
        assert all(info["kinds"][i] in PR.LCE_OPS for i in s.ops)


@pytest.mark.parametrize("fixture", ["reactnet", "gated", "flatten"])
def test_with_the_new_names_each_network_is_one_section(fixture):
    data, x, out, info = dict(reactnet=AM.reactnet_model, gated=AM.gated_model, flatten=AM.flatten_head_model)[fixture]()
    names = dict(reactnet=dict(elementwise_sections=True, activation_sections=True),
                 gated=dict(head_sections=True, elementwise_sections=True, **AM.NEW_KEYWORDS),
                 flatten=dict(head_sections=True, reshape_sections=True))[fixture]
    model = mr.LceModel(data, **names)
    outs = out if isinstance(out, list) else [out]
    assert [(s.ops, s.inputs, s.outputs) for s in model.sections] == [(list(range(len(model.operators))), [x], sorted(outs))]
    assert mr.Interpreter(model).lce_only
    # the walker's shapes at another batch (no device: shape inference only)
    for t in outs:
        dims, nbytes = model.section_tensor_shape(0, t, 5)
        file_shape = model.tensors[t].shape
        carried = file_shape if len(file_shape) == 4 else (file_shape[0], 1, 1, file_shape[1])
        assert dims == (5,) + tuple(carried[1:]) and nbytes == 5 * 4 * int(np.prod(carried[1:]))
    # one name short, the network is no longer one section
    for missing in names:
        fewer = mr.LceModel(data, **{k: v for k, v in names.items() if k != missing})
        assert not mr.Interpreter(fewer).lce_only, missing


@pytest.mark.parametrize("case", AM.REFUSALS)
def test_each_predicate_refuses(case):
    data, k = AM.single_op_model(case)
    h, err, keep = open_passes(data, ",".join(AM.OLD_NAMES + AM.NEW_NAMES).encode(), at_page_end=True)
    assert h, err
    assert all(k not in ops for ops, _, _ in _sections_of(h)), case
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)


@pytest.mark.parametrize("case", AM.CONTROLS)
def test_each_predicate_takes_the_well_formed_twin(case):
    data, k = AM.single_op_model(case)
    name = dict(prelu="activation", logistic="activation", reshape="reshape", gate="gate")[case]
    h, err, keep = open_passes(data, name.encode(), at_page_end=True)
    assert h and [k in ops for ops, _, _ in _sections_of(h)] == [True], (case, err)
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    others = [n for n in AM.OLD_NAMES + AM.NEW_NAMES if n != name]
    h, err, _ = open_passes(data, ",".join(others).encode())
    assert h and all(k not in ops for ops, _, _ in _sections_of(h)), case          # and nothing but its own name takes it
    mr.tflite_lib().lce_tflite_model_close(h)


def test_alpha_shapes():
    """[C], [1,1,C], [1,1,1,C], [1] and [] qualify; [1,C], [H,W,C] and a constant of the wrong size do not."""
    for shape, ok in (([32], True), ([1, 1, 32], True), ([1, 1, 1, 32], True), ([1], True), ([], True), ([1, 32], False), ([4, 4, 32], False),
                      ([16], False), ([1, 4, 1, 32], False)):
        b = ModelBuilder()
        x, y = b.tensor([1, 4, 4, 32], np.float32, "x"), b.tensor([1, 4, 4, 32], np.float32, "y")
        alpha = b.tensor(shape or [1], np.float32, "alpha", np.full(shape or [1], 0.25, np.float32))
        if not shape:                                                # (the writer takes no 0-d array: a scalar's shape vector is empty)
            b.tensors[alpha].fields[0] = _Vector("i", [])
        b.builtin_op(AM.PRELU, [x, alpha], [y])
        b.inputs, b.outputs = [x], [y]
        model = mr.LceModel(b.finish(), stem_sections=True, activation_sections=True)
        assert (len(model.sections) == 1) == ok, shape


# ---- what the parent commit cannot do ----------------------------------------------------------------------------------------------
def test_the_keywords_exist_and_a_reactnet_file_is_no_longer_the_hosts():
    data = AM.reactnet_model()[0]
    for keyword in AM.NEW_KEYWORDS:
        model = mr.LceModel(data, **{keyword: True})                 # (a TypeError before the keywords existed)
        assert getattr(model, keyword) and mr._PASS_NAMES[keyword] in AM.NEW_NAMES
        assert not any(getattr(mr.LceModel(data), k) for k in AM.NEW_KEYWORDS)
    it = mr.Interpreter(data, batch_size=3, elementwise_sections=True, activation_sections=True)
    assert it.lce_only and len(it.sections) == 1
    it._require_lce_only()                                           # predict()'s gate: NotImplementedError naming PRELU before
    with pytest.raises(NotImplementedError):
        mr.Interpreter(data, batch_size=3, elementwise_sections=True)._require_lce_only()
