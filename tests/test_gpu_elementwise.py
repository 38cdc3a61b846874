"""lce_hip_elementwise and the elementwise sections on the MI355X: the kernel bit for bit against a NumPy restatement of
TFLite's op-by-op float semantics (one rounding per op, CalculateActivationRange, std::min / std::max), its bits against the
oracle's LceQuantize, and a QuickNet body run as ONE section against the same file run section by section with the ADD / MUL
done in NumPy in between."""
import ctypes
import importlib

import numpy as np
import pytest

import oracle_lib as O
from section_models import BODY, body_model

torch = pytest.importorskip("torch")
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMAX = np.float32(np.finfo(np.float32).max)
RANGE = {amd.ACT_NONE: (-FMAX, FMAX), amd.ACT_RELU: (np.float32(0), FMAX), amd.ACT_RELU_N1_TO_1: (np.float32(-1), np.float32(1)),
         amd.ACT_RELU6: (np.float32(0), np.float32(6))}


def ref_op(v, op, operand, act):
    """TFLite's reference Add / Mul on float, then ActivationFunctionWithMinMax: min(max(v, lo), hi), std::max(a, b) = a < b ? b : a."""
    v = (v * operand if op in (amd.EW_MUL, "mul") else v + operand).astype(np.float32)
    lo, hi = RANGE[act]
    v = np.where(v < lo, lo, v)
    return np.where(hi < v, hi, v).astype(np.float32)


def ref(x, steps):
    v = x.astype(np.float32)
    for op, operand, act in steps:
        v = ref_op(v, op, np.float32(operand) if np.isscalar(operand) else operand, act)
    return v


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def inputs(rows, C, seed):
    """x with -0.0, subnormals and values where fma(x, m, b) != fl(fl(x*m) + b); per-channel m, b; a residual with +-inf."""
    g = np.random.default_rng(seed)
    base = g.uniform(0.5, 2.0, C).astype(np.float32) * np.where(g.random(C) < 0.5, -1, 1).astype(np.float32)
    m = g.uniform(0.5, 2.0, C).astype(np.float32)
    b = (-(base * m)).astype(np.float32)                    # cancels the product: its rounding error decides the sum
    x = (base * (1 + g.uniform(-2 ** -10, 2 ** -10, (rows, C)))).astype(np.float32)
    flat = x.reshape(-1)
    k = flat.size
    flat[g.integers(0, k, k // 50 + 1)] = -0.0
    flat[g.integers(0, k, k // 50 + 1)] = np.float32(1e-40) * g.choice([-1, 1])
    res = g.standard_normal((rows, C)).astype(np.float32)
    rf = res.reshape(-1)
    rf[g.integers(0, k, k // 100 + 1)] = np.inf
    rf[g.integers(0, k, k // 100 + 1)] = -np.inf
    return x, m, b, res


def run(x, steps, **kw):
    xd = torch.from_numpy(x).to(DEV)
    dsteps = [(op, o if np.isscalar(o) else torch.from_numpy(np.ascontiguousarray(o)).to(DEV), a) for op, o, a in steps]
    out, bits = amd.elementwise(xd, dsteps, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def programs(m, b, res):
    return {
        "residual": [("add", res, amd.ACT_NONE)],
        "bn_residual_relu": [("mul", m, amd.ACT_NONE), ("add", b, amd.ACT_NONE), ("add", res, amd.ACT_RELU)],
        "eight": [("mul", m, amd.ACT_NONE), ("add", b, amd.ACT_RELU6), ("add", 0.25, amd.ACT_NONE), ("mul", -3.0, amd.ACT_RELU_N1_TO_1),
                  ("add", res, amd.ACT_NONE), ("mul", m, amd.ACT_RELU), ("add", -1e-39, amd.ACT_NONE), ("mul", 0.5, amd.ACT_NONE)],
    }


@pytest.mark.parametrize("C", [1, 3, 31, 32, 33, 64, 96, 100, 256, 512])
def test_kernel_matches_the_semantics_bit_for_bit(C):
    rows = 37
    x, m, b, res = inputs(rows, C, C)
    for name, steps in programs(m, b, res).items():
        want = ref(x, steps)
        got, bits = run(x, steps, out_bits=True)
        assert same(got, want), (C, name)
        assert np.array_equal(bits, O.bitpack(want)), (C, name)
        only_bits = run(x, steps, out=False, out_bits=True)
        assert only_bits[0] is None and np.array_equal(only_bits[1], bits), (C, name)
        only_float = run(x, steps)
        assert only_float[1] is None and same(only_float[0], want), (C, name)


@pytest.mark.parametrize("rows", [1, 7, 256 * 56 * 56])
def test_rows_at_64_channels(rows):
    x, m, b, res = inputs(rows, 64, rows)
    steps = programs(m, b, res)["bn_residual_relu"]
    want = ref(x, steps)
    got, bits = run(x, steps, out_bits=True)
    assert same(got, want)
    assert np.array_equal(bits, O.bitpack(want))


def test_the_edge_semantics():
    """RELU(-0.0) = -0.0, +-inf -> +-FLT_MAX with no activation, subnormals kept, fma != mul + add on most elements, and
    the sign bit of -0.0 is 0."""
    C = 64
    x, m, b, res = inputs(64, C, 5)
    fused = (x.astype(np.float64) * m + b).astype(np.float32)
    two = ((x * m).astype(np.float32) + b).astype(np.float32)
    assert np.mean(fused != two) > 0.5                                   # the inputs do tell an fma apart
    got, _ = run(x, [("mul", m, amd.ACT_NONE), ("add", b, amd.ACT_NONE)])
    assert same(got, two)
    z = np.full((2, C), -0.0, np.float32)
    got, bits = run(z, [("add", -0.0, amd.ACT_RELU)], out_bits=True)
    assert same(got, z) and not bits.any()
    inf = np.array([[np.inf, -np.inf] * (C // 2)], np.float32)
    got, _ = run(inf, [("add", 0.0, amd.ACT_NONE)])
    assert same(got, np.array([[FMAX, -FMAX] * (C // 2)], np.float32))
    sub = np.full((1, C), 1e-40, np.float32)
    got, _ = run(sub, [("mul", 1.0, amd.ACT_NONE)])
    assert same(got, sub)


def test_in_place_misaligned_and_empty():
    C = 64
    x, m, b, res = inputs(50, C, 9)
    steps = programs(m, b, res)["bn_residual_relu"]
    want = ref(x, steps)
    xd = torch.from_numpy(x).to(DEV)
    amd.elementwise(xd, [(op, o if np.isscalar(o) else torch.from_numpy(o).to(DEV), a) for op, o, a in steps], out=xd)
    assert same(xd.cpu().numpy(), want)
    rd = torch.from_numpy(res).to(DEV)
    md, bd = torch.from_numpy(m).to(DEV), torch.from_numpy(b).to(DEV)
    amd.elementwise(torch.from_numpy(x).to(DEV), [("mul", md, 0), ("add", bd, 0), ("add", rd, amd.ACT_RELU)], out=rd)
    assert same(rd.cpu().numpy(), want)
    # pointers 4 bytes past a 16-byte boundary: the row path
    big = torch.zeros(50 * C + 1, dtype=torch.float32, device=DEV)
    xs = big[1:].view(50, C)
    xs.copy_(torch.from_numpy(x))
    bits = torch.zeros((50, 2), dtype=torch.int32, device=DEV)
    out = torch.zeros(50 * C + 1, dtype=torch.float32, device=DEV)[1:].view(50, C)
    amd.elementwise(xs, [("mul", md, 0), ("add", bd, 0), ("add", rd.new_tensor(res), amd.ACT_RELU)], out=out, out_bits=bits)
    assert same(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), O.bitpack(want))
    e = torch.zeros((0, C), dtype=torch.float32, device=DEV)
    o, bb = amd.elementwise(e, [("add", 1.0, 0)], out_bits=True)
    assert o.shape == (0, C) and bb.shape == (0, 2)
    with pytest.raises(amd.LceHipError, match="num_steps"):
        amd.check(amd.lib().lce_hip_elementwise(None, 1, 1, None, 0, None, None, None))
    with pytest.raises(amd.LceHipError, match="both outputs"):
        amd.check(amd.lib().lce_hip_elementwise(ctypes.c_void_p(xs.data_ptr()), 50, C, (amd.EwStep * 1)(amd.EwStep(0, 0, None, 1.0, 0)), 1,
                                                None, None, None))


# ---- sections ---------------------------------------------------------------------------------------------------------
def default_mode(data, info, x):
    """The same file in default mode: one (LceQuantize, LceBconv2d) section per layer, the ADD / MUL in NumPy between."""
    it = mr.Interpreter(data, batch_size=x.shape[0])
    r = x
    for k, li in enumerate(info):
        (y,) = it.run_section(k, [r])
        v = ref_op(y, "mul", li["bn_m"], amd.ACT_NONE)
        if li["residual"]:
            v = ref_op(v, "add", li["bn_a"].reshape(1, 1, 1, -1), amd.ACT_NONE)
            v = ref_op(v, "add", r, li["act"])
        else:
            v = ref_op(v, "add", li["bn_a"].reshape(1, 1, 1, -1), li["act"])
        r = v
    return r


@pytest.mark.parametrize("batch", [1, 7, 256])
def test_the_body_runs_as_one_section(batch):
    data, xt, out, info, outs = body_model()
    x = np.random.default_rng(batch).standard_normal((batch, 56, 56, 64)).astype(np.float32)
    it = mr.Interpreter(data, batch_size=batch, elementwise_sections=True)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert it.model.elementwise_stats() == (len(BODY), 2 * len(BODY) + sum(li["residual"] for li in info), len(BODY) - 1)
    assert it.model.run_stats()[1] == 0
    want = default_mode(data, info, x)
    assert same(got, want)
    if batch == 7:
        assert same(it.predict(x), want)


def test_one_layer_against_the_oracle():
    data, xt, out, info, outs = body_model(BODY[:1])
    x = np.random.default_rng(3).standard_normal((2, 56, 56, 64)).astype(np.float32)
    (got,) = mr.Interpreter(data, batch_size=2, elementwise_sections=True).run_section(0, [x])
    li = info[0]
    y = O.bconv2d(li["spec"].with_batch(2), O.DST_F32, O.bitpack(x), li["w"], li["m"], li["b"])
    want = ref(y, [("mul", li["bn_m"], 0), ("add", li["bn_a"], 0), ("add", x, li["act"])])
    assert same(got, want)


def test_hip_graph_replay_gives_the_same_bytes():
    data, xt, out, info, outs = body_model()
    model = mr.LceModel(data, elementwise_sections=True)
    batch = 7
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((batch, 56, 56, 64)).astype(np.float32)).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    eager = torch.empty(dims, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model.run_section(0, batch, [x.data_ptr()], [eager.data_ptr()], s.cuda_stream)
        s.synchronize()
        model.use_hip_graphs(True)
        y = torch.empty_like(eager)
        for _ in range(3):
            y.zero_()
            model.run_section(0, batch, [x.data_ptr()], [y.data_ptr()], s.cuda_stream)
        s.synchronize()
    assert model.graph_stats()[0] == 1
    assert model.elementwise_stats()[0] == len(BODY)
    assert same(y.cpu().numpy(), eager.cpu().numpy())
    model.use_hip_graphs(False)
