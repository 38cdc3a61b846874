"""The classifier head's kernels without a GPU: the real bodies of csrc/lce_kernels_head.h on the CPU (tests/hostsim_head: the
lanes of a block as fibers, v_mfma_f32_16x16x4_f32 emulated as the k-ordered fmaf chain the kernel takes it for) against
tests/head_ref.py, byte for byte; the known answers; the accuracy of the stated exp against float64; the bound of the restated
softmax against a float64 softmax; and the C ABI's refusals, which need no device.  What a
simulation cannot decide -- that the instruction IS such a chain -- is the GPU suite's (tests/test_gpu_head.py)."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import conv1x1_ref as CR
import head_ref as HR
import hostsim_lib
from section_models import float_fixture

amd = importlib.import_module("compute-engine_amd")
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_head")
OUT_MARK = np.float32(777)
ACTS = (HR.NONE, HR.RELU, HR.RELU_N1_TO_1, HR.RELU6)
FLT_MAX = np.float32(3.4028234663852886e38)
FLT_MIN = np.float32(2.0 ** -126)          # the smallest normal
EXP_MAX_ULP = 1.0                          # measured: 0.93 ulp, rounded up to a whole ulp
FC_BATCHES, FC_K, FC_N = (1, 3, 33), (1, 6, 32, 70, 132), (1, 31, 33, 70)
SM_ROWS, SM_COLS, SM_BETAS = (1, 5), (1, 2, 63, 64, 65, 129, 1000, 1001), (1.0, 0.5)
_lib = None


def lib():
    """tests/hostsim_head/liblce_hostsim_head.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        _lib = hostsim_lib.load(DIR, "liblce_hostsim_head.so")
        _lib.lce_hostsim_fully_connected.argtypes = [C.c_void_p] * 5 + [C.c_int32]
        _lib.lce_hostsim_softmax.argtypes = [C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_int32]
        _lib.lce_hostsim_softmax.restype = None
        _lib.lce_hostsim_head_exp.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        _lib.lce_hostsim_head_exp.restype = None
    return _lib


def placed(a, offset):
    """A copy of `a` whose first byte lies `offset` floats behind a 16-byte boundary."""
    return hostsim_lib.placed(a, 4 * offset)


def sim_fc(x, w, bias, act, cap=3, offset=0):
    """(out, took the 16-byte path)"""
    x, w = placed(np.asarray(x, np.float32), offset), placed(np.asarray(w, np.float32), offset)
    d = (C.c_int32 * 4)(x.shape[0], x.shape[1], w.shape[0], act)
    out = np.full((x.shape[0], w.shape[0]), OUT_MARK, np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    vec = lib().lce_hostsim_fully_connected(d, x.ctypes.data, w.ctypes.data, None if b is None else b.ctypes.data, out.ctypes.data, cap)
    return out, bool(vec)


def sim_softmax(x, beta, cap=3, in_place=False):
    x = np.ascontiguousarray(x, np.float32).copy()
    out = x if in_place else np.full(x.shape, OUT_MARK, np.float32)
    lib().lce_hostsim_softmax(x.shape[0], x.shape[1], beta, x.ctypes.data, out.ctypes.data, cap)
    return out


def sim_exp(a):
    a = np.ascontiguousarray(a, np.float32)
    e = np.empty_like(a)
    lib().lce_hostsim_head_exp(a.ctypes.data, e.ctypes.data, a.size)
    return e


def agree(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def fc_operands(batch, k, n, seed=0, special=False):
    g = np.random.default_rng(1000 * batch + 10 * k + n + seed)
    x = float_fixture((batch, k), 7 * batch + k + seed, special)
    w = (g.standard_normal((n, k)) * g.choice([1e-2, 1.0, 30.0], (n, k))).astype(np.float32)
    if special:
        w[::5] *= np.float32(1e-36)
    return x, w, g.standard_normal(n).astype(np.float32)


def softmax_rows(rows, cols, seed=0):
    """Finite rows of mixed spread: logits of a classifier, a row that holds the clamp's +-FLT_MAX (so a = -inf), spreads beyond 104
    (entries that underflow to +0) and just inside it (entries that land in the subnormals)."""
    g = np.random.default_rng(100 * rows + cols + seed)
    x = (g.standard_normal((rows, cols)) * g.choice([0.1, 3.0, 40.0], (rows, 1))).astype(np.float32)
    x[0, ::7] -= np.float32(95.0)
    x[0, ::11] -= np.float32(120.0)
    if rows > 1:
        x[1, ::3] = -FLT_MAX
        x[1, cols // 2] = FLT_MAX if cols > 2 else x[1, cols // 2]
        x[2, :] = np.float32(-0.0)
        x[2, ::2] = np.float32(0.0)
    return x


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_a_negative_zero_accumulator_survives_the_k_tail():
    """fmaf(1e-30f, -1e-30f, +0) = -0.0 (the product underflows to -0): the tail's padding (x = -0.0, w = +0.0) adds -0.0 to it."""
    assert np.signbit(CR.fma32(np.float32(1e-30), np.float32(-1e-30), np.float32(0.0))) and CR.fma32(np.float32(1e-30), np.float32(-1e-30), np.float32(0.0)) == 0
    for k in (1, 5, 6, 16, 17, 19):                                  # the product last, only padding behind it: every tail length
        x = np.zeros((2, k), np.float32)
        w = np.zeros((3, k), np.float32)
        x[:, k - 1], w[:, k - 1] = np.float32(1e-30), np.float32(-1e-30)
        for offset in (0, 1):
            out, _ = sim_fc(x, w, None, HR.NONE, offset=offset)
            assert np.array_equal(out.view(np.uint32), np.full((2, 3), 0x80000000, np.uint32)), (k, offset)
        assert np.array_equal(HR.fully_connected(x, w).view(np.uint32), np.full((2, 3), 0x80000000, np.uint32))


@pytest.mark.parametrize("n", [1, 2, 64, 128, 1024])
def test_a_row_of_equal_values_gives_one_nth_exactly(n):
    for value in (0.0, -3.5, 1e30):
        x = np.full((2, n), value, np.float32)
        want = np.full((2, n), np.float32(1.0) / np.float32(n), np.float32)
        assert np.array_equal(sim_softmax(x, 1.0), want) and np.array_equal(HR.softmax(x), want)


def test_one_entry_far_above_the_rest_takes_everything():
    x = np.zeros((1, 70), np.float32)
    x[0, 13] = 200.0
    want = np.zeros((1, 70), np.float32)
    want[0, 13] = 1.0
    for got in (sim_softmax(x, 1.0), HR.softmax(x), sim_softmax(x, 0.75)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))       # +0.0, not -0.0


# ---- the kernel bodies against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FC_K)
def test_the_fully_connected_body_gives_the_reference_bytes(k):
    n_checks = vecs = 0
    for batch in FC_BATCHES:
        x, w, bias = fc_operands(batch, k, max(FC_N))
        t = CR.chain(x, w)                                           # once at the widest N, sliced below
        for n in FC_N:
            for act in ACTS:
                for with_bias in (True, False):
                    offset = (n_checks // 2) % 2
                    b = bias[:n] if with_bias else None
                    with np.errstate(invalid="ignore", over="ignore"):
                        want = CR.clamp(t[:, :n] + b[None, :] if with_bias else t[:, :n], act)
                    out, vec = sim_fc(x, w[:n], b, act, offset=offset)
                    assert vec == (k % 4 == 0 and offset == 0)
                    vecs += vec
                    assert agree(out, want), (batch, k, n, act, with_bias, offset)
                    n_checks += 1
    assert n_checks == 3 * 4 * 4 * 2 and (vecs > 0) == (k % 4 == 0)


@pytest.mark.parametrize("k", [6, 32, 70])
def test_the_fully_connected_body_on_special_values(k):
    for batch, n in ((3, 33), (33, 31)):
        x, w, bias = fc_operands(batch, k, n, seed=5, special=True)
        assert batch < 33 or ((~np.isfinite(x)).any() and (np.abs(x[x != 0]) < FLT_MIN).any())     # NaN or inf, and subnormals
        for offset in (0, 1):
            out, _ = sim_fc(x, w, bias, HR.NONE, offset=offset)
            assert agree(out, HR.fully_connected(x, w, bias, HR.NONE)), (batch, k, n, offset)


@pytest.mark.parametrize("k", [63, 64, 65, 128, 196])
def test_the_fully_connected_body_at_the_edges_of_a_chunk(k):
    """A chunk of K is 64 channels: one short of it, exactly one, one more, exactly two, three and a 16-byte tail."""
    x, w, bias = fc_operands(3, k, 33, seed=2)
    for offset in (0, 1):
        out, vec = sim_fc(x, w, bias, HR.RELU_N1_TO_1, offset=offset)
        assert vec == (k % 4 == 0 and offset == 0) and agree(out, HR.fully_connected(x, w, bias, HR.RELU_N1_TO_1)), (k, offset)


def test_more_tiles_than_one_pass_of_a_capped_grid():
    """One block of four waves against 3 x 5 = 15 tiles, the last row and column tiles ragged."""
    x, w, bias = fc_operands(33, 70, 70)
    out, _ = sim_fc(x, w, bias, HR.RELU, cap=1)
    assert agree(out, HR.fully_connected(x, w, bias, HR.RELU))


@pytest.mark.parametrize("cols", SM_COLS)
def test_the_softmax_body_gives_the_reference_bytes(cols):
    for rows in SM_ROWS:
        x = softmax_rows(rows, cols)
        for beta in SM_BETAS:
            want = HR.softmax(x, beta)
            assert np.isfinite(want).all() and (want >= 0).all()
            assert np.array_equal(sim_softmax(x, beta).view(np.uint32), want.view(np.uint32)), (rows, cols, beta)
            assert np.array_equal(sim_softmax(x, beta, cap=1, in_place=True).view(np.uint32), want.view(np.uint32)), (rows, cols, beta)
    if cols >= 63:
        assert (HR.softmax(softmax_rows(1, cols)) == 0).any()        # the spread beyond 104 underflowed to +0


def test_rows_with_nan_or_infinity_do_not_fault():
    x = softmax_rows(5, 65)
    x[0, 3], x[3, 0], x[4, 7] = np.nan, np.inf, -np.inf
    got = sim_softmax(x, 1.0)
    assert got.shape == x.shape
    assert np.array_equal(got[1:3].view(np.uint32), HR.softmax(x[1:3]).view(np.uint32))     # the finite rows keep their bytes


# ---- the accuracy of the stated exp ----------------------------------------------------------------------------------------------
def exp_arguments():
    """Every float32 within 64 steps of a power of two in [-128, -2^-149] (clipped to [-104, 0]), the neighbourhoods of the
    thresholds (-104, the first subnormal result, the end of the normal range) and of the multiples of ln 2 / 2, where n
    changes; then 10^7 others, uniform in [-104, 0] and log-uniform towards 0."""
    steps = np.arange(-64, 65, dtype=np.int64)
    centres = [np.float32(-(2.0 ** k)) for k in range(-149, 8)] + [np.float32(v) for v in (-104.0, -103.2789, -87.33654, -87.0)]
    centres += [np.float32(-0.5 * math.log(2.0) * j) for j in range(1, 301)]
    near = (np.array(centres, np.float32).view(np.uint32).astype(np.int64)[:, None] + steps[None, :]).astype(np.uint32).view(np.float32).ravel()
    near = near[np.isfinite(near) & (near >= -104) & (near <= 0)]
    g = np.random.default_rng(2024)
    uniform = (-g.uniform(0.0, 104.0, 8_000_000)).astype(np.float32)
    log_uniform = (-np.exp(g.uniform(math.log(1e-30), math.log(104.0), 2_000_000))).astype(np.float32)
    return np.concatenate([near, uniform, log_uniform, np.float32([0.0, -0.0])])


def ulp_error(e, a):
    """|e - exp(a)| in float32 ulps of exp(a) (2^-149 below the normal range)."""
    exact = np.exp(a.astype(np.float64))
    ulp = np.where(exact < 2.0 ** -126, 2.0 ** -149, np.spacing(np.maximum(exact, 2.0 ** -126).astype(np.float32)).astype(np.float64))
    return np.abs(e.astype(np.float64) - exact) / ulp


def test_the_stated_exp_is_within_one_ulp_of_exp():
    a = exp_arguments()
    assert a.size >= 10_000_000 and a.min() == -104 and a.max() == 0
    e = sim_exp(a)                                                   # the kernel's own function, compiled for the CPU
    err = ulp_error(e, a)
    worst = int(err.argmax())
    print("exp: max error %.4f ulp at a = %r (normal range %.4f, subnormal results %.4f)"
          % (err[worst], float(a[worst]), err[e >= FLT_MIN].max(), err[e < FLT_MIN].max()))
    assert err.max() <= EXP_MAX_ULP, (err[worst], a[worst])
    # the restatement is the same function: every argument near a power of two or a threshold, and a slice of the others
    part = np.concatenate([a[:40000], a[-500_000:]])
    assert np.array_equal(HR.exp32(part).view(np.uint32), sim_exp(part).view(np.uint32))
    # outside [-104, 0]
    odd = np.float32([-104.00001, -1e30, -np.inf, np.nan, 1e-3, 5.0])
    assert np.array_equal(sim_exp(odd).view(np.uint32), np.float32([0, 0, 0, 0, 1, 1]).view(np.uint32))
    assert np.array_equal(HR.exp32(odd).view(np.uint32), np.float32([0, 0, 0, 0, 1, 1]).view(np.uint32))


def softmax_tolerance(x, beta):
    """Per element, with u = 2^-24 (half an ulp, relative), p the float64 softmax, a = (x - max) * beta and
    D = ceil(cols / 64) + 6 the depth of the sum:

      a_i is computed in two rounded operations, so it is off by at most 2 u |a_i|, which moves exp(a_i) by that much relatively;
      the stated exp adds EXP_MAX_ULP ulp, at most 2 u EXP_MAX_ULP relatively:       e_i is within 2 u (E + |a_i|) of exp(a_i);
      s is a sum of non-negative terms through D rounded adds: D u relatively, on top of the terms' own error, whose weighted mean
      is sum_j p_j 2 u (E + |a_j|);
      the division rounds once: u.

    So |out_i - p_i| <= p_i u (2 (E + |a_i|) + D + 2 sum_j p_j (E + |a_j|) + 1), taken times 1.01 for the second-order terms (the
    first-order sum is below 2^-16), plus the smallest normal for entries whose e_i or quotient left the normal range (there the
    errors are absolute: at most an ulp of 2^-149 each, and an entry beyond -104 counts as +0 while exp of it is below 2^-150)."""
    x64 = x.astype(np.float64)
    a = (x64 - x64.max(axis=1, keepdims=True)) * float(beta)
    p = np.exp(a)
    p /= p.sum(axis=1, keepdims=True)
    u, depth = 2.0 ** -24, -(-x.shape[1] // 64) + 6
    own = 2.0 * (EXP_MAX_ULP + np.abs(a))
    rel = own + depth + (p * own).sum(axis=1, keepdims=True) + 1.0
    return p, 1.01 * u * rel * p + float(FLT_MIN)


@pytest.mark.parametrize("cols", [1, 10, 65, 1000, 1001])
def test_the_restated_softmax_is_within_its_derived_bound_of_a_float64_softmax(cols):
    worst = 0.0
    for rows in (5, 64):
        for beta in SM_BETAS:
            x = softmax_rows(rows, cols, seed=3)
            p, tol = softmax_tolerance(x, beta)
            got = HR.softmax(x, beta).astype(np.float64)
            worst = max(worst, float((np.abs(got - p) / tol).max()))
            assert (np.abs(got - p) <= tol).all(), (rows, beta, float((np.abs(got - p) / tol).max()))
            assert (np.abs(got.sum(axis=1) - 1.0) <= tol.sum(axis=1)).all()
    print("softmax: the largest error is %.3f of the bound at %d columns" % (worst, cols))


# ---- the C ABI: refusals need no device -------------------------------------------------------------------------------------------
def test_the_abi():
    assert amd.lib().lce_hip_abi_version() == 3
    for name in ("lce_hip_fully_connected_f32", "lce_hip_fully_connected_f32_check", "lce_hip_softmax_f32", "lce_hip_softmax_f32_check"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    assert C.sizeof(amd.FcDesc) == 16 and [n for n, _ in amd.FcDesc._fields_] == ["batch", "inputs", "outputs", "activation"]


def _last_error():
    return amd.lib().lce_hip_last_error().decode()


def test_the_checks_refuse_before_any_device_call():
    l = amd.lib()
    fc = lambda *d: l.lce_hip_fully_connected_f32_check(C.byref(amd.FcDesc(*d)))
    assert fc(256, 512, 1000, amd.ACT_RELU6) == amd.OK and fc(1, 1, 1, 0) == amd.OK
    for d in ((0, 4, 4, 0), (4, 0, 4, 0), (4, 4, -1, 0)):
        assert fc(*d) == amd.ERR_INVALID and "extents" in _last_error()
    assert fc(4, 4, 4, 4) == amd.ERR_INVALID and "activation" in _last_error()
    assert fc(2 ** 31 - 1, 4, 2 ** 31 - 1, 0) == amd.ERR_UNSUPPORTED and "tiles" in _last_error()
    assert l.lce_hip_fully_connected_f32_check(None) == amd.ERR_INVALID
    sm = l.lce_hip_softmax_f32_check
    assert sm(256, 1000, 1.0) == amd.OK and sm(1, 1, 1e-3) == amd.OK
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert sm(4, 4, beta) == amd.ERR_INVALID and "beta" in _last_error()
    assert sm(0, 4, 1.0) == amd.ERR_INVALID and sm(4, 0, 1.0) == amd.ERR_INVALID
    assert sm(1, 2 ** 31, 1.0) == amd.ERR_UNSUPPORTED and sm(2 ** 40, 2 ** 30, 1.0) == amd.ERR_UNSUPPORTED
    # the run entries refuse a bad pointer or descriptor before they ask for a device
    a = np.zeros(64, np.float32)
    p = a.ctypes.data
    run = l.lce_hip_fully_connected_f32
    d = C.byref(amd.FcDesc(2, 4, 4, 0))
    assert run(None, p, p, None, p, None) == amd.ERR_INVALID
    assert run(d, None, p, None, p, None) == amd.ERR_INVALID and "input" in _last_error()
    assert run(d, p, None, None, p, None) == amd.ERR_INVALID and "weights" in _last_error()
    assert run(d, p, p + 64, None, None, None) == amd.ERR_INVALID and "output" in _last_error()
    assert run(d, p, p + 64, None, p + 16, None) == amd.ERR_INVALID and "overlaps the input" in _last_error()
    assert run(d, p, p + 64, None, p + 96, None) == amd.ERR_INVALID and "overlaps the filter" in _last_error()
    assert run(d, p, p + 64, p + 128, p + 136, None) == amd.ERR_INVALID and "overlaps the bias" in _last_error()
    assert run(d, p + 2, p + 64, None, p + 192, None) == amd.ERR_INVALID and "aligned" in _last_error()
    run = l.lce_hip_softmax_f32
    assert run(2, 4, 1.0, None, p, None) == amd.ERR_INVALID and run(2, 4, 1.0, p, None, None) == amd.ERR_INVALID
    assert run(2, 4, 0.0, p, p, None) == amd.ERR_INVALID and "beta" in _last_error()
    assert run(2, 4, 1.0, p, p + 16, None) == amd.ERR_INVALID and "partly overlaps" in _last_error()
    assert run(2, 4, 1.0, p + 1, p + 129, None) == amd.ERR_INVALID and "aligned" in _last_error()


def test_the_python_wrappers_check_shapes_without_a_device():
    x, w = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    for bad in (dict(x=x[0]), dict(w=w[:, :7]), dict(x=x.astype(np.float64)), dict(bias=np.zeros(4, np.float32)), dict(activation=4),
                dict(out=np.zeros((3, 4), np.float32))):
        kw = dict(x=x, w=w, bias=None, activation=amd.ACT_NONE, out=None)
        kw.update(bad)
        with pytest.raises(ValueError, match="fully_connected"):
            amd._fully_connected_check(**kw)
    assert amd._fully_connected_check(x, w, np.zeros(5, np.float32), amd.ACT_RELU, None)[1] == (3, 5)
    for bad in (dict(beta=0.0), dict(beta=float("nan")), dict(x=x.astype(np.int32)), dict(out=np.zeros((3, 7), np.float32))):
        kw = dict(x=x, beta=1.0, out=None)
        kw.update(bad)
        with pytest.raises(ValueError, match="softmax"):
            amd._softmax_check(**kw)
    assert amd._softmax_check(np.zeros((2, 3, 8), np.float32), 0.5, None) == (6, 8)
