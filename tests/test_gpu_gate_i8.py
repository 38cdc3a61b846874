"""lce_hip_mul_int8 and lce_hip_logistic_int8 on the MI355X, byte for byte with no tolerance against the NumPy restatement of the
header's arithmetic (tests/gate_i8_ref.py): a cut of the CPU simulation's grid, both operand kinds, with and without the residual
ADD, every combination of outputs, in place, an unaligned tensor, a tensor of 2^24 + 2 rows, a HIP-graph capture with one replay,
and a RealToBinary-style int8 body through the model reader as ONE section."""
import importlib

import numpy as np
import pytest

import gate_i8_models as M
import gate_i8_ref as G
import int8_add_ref as ar
from test_gate_i8_hostsim import _case

torch = pytest.importorskip("torch")
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(args, kw, **more):
    x, operand, q1, q2, qo = args
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    rpi = kw["rows_per_image"]
    more.setdefault("out_bits", True)
    out, bits, launch = amd.mul_int8(dev(x), dev(operand), q1, q2, qo, act=kw["act"], per_image=bool(rpi), rows_per_image=rpi,
                                     addend=dev(kw["addend"]), add=kw["add"], report_launch=True, **more)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy(), launch


@pytest.mark.parametrize("channels", [1, 33, 64, 80, 256])
@pytest.mark.parametrize("rpi", [1, 49])
def test_the_shapes_of_the_simulation(channels, rpi):
    for per_image in (False, True):
        for has_add in (False, True):
            args, kw, want, want_bits = _case(channels * 100 + rpi, 3, rpi, channels, per_image, has_add, act=has_add * 3, add_act=1 - has_add)
            out, bits, L = run(args, kw)
            assert L["flat"] == int(channels % 16 == 0) and (L["add_variant"] >= 0) == has_add and L["mul_variant"] == 1
            assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (per_image, has_add)


@pytest.mark.parametrize("channels", [33, 64])
def test_the_literal_mul_variant(channels):
    """A real multiplier of 3.125 (e = 2) is outside the fast variant's precondition (tests/test_gate_i8_hostsim.py)."""
    g = np.random.default_rng(channels)
    q1, q2, qo = (0.5, 3), (0.5, -4), (0.08, 5)
    x = g.integers(-3, 11, (147, channels)).astype(np.int8)
    gate = g.integers(-10, 4, (3, channels)).astype(np.int8)
    addend = g.integers(-128, 128, (147, channels)).astype(np.int8)
    add = ((0.4, 1), (0.9, -2), 0)
    kw = dict(act=0, rows_per_image=49, addend=addend, add=add)
    out, bits, L = run((x, gate, q1, q2, qo), kw)
    want = G.mul_add_q(x, gate, addend, q1, q2, qo, 0, add[0], add[1], 0, 49)
    assert L["mul_variant"] == 0 and np.array_equal(out, want) and np.array_equal(bits, ar.bitpack(want, -2))


@pytest.mark.parametrize("channels", [33, 64, 80])
def test_either_output_alone_and_in_place(channels):
    args, kw, want, want_bits = _case(7 + channels, 3, 49, channels, True, True)
    out, bits, _ = run(args, kw, out_bits=None)
    assert bits is None and np.array_equal(out, want)
    out, bits, _ = run(args, kw, out=False)
    assert out is None and np.array_equal(bits, want_bits)
    x, operand, q1, q2, qo = args
    for where in ("x", "addend"):
        xd, gd, ad = (torch.from_numpy(a).to(DEV) for a in (x, operand, kw["addend"]))
        target = xd if where == "x" else ad
        out, bits = amd.mul_int8(xd, gd, q1, q2, qo, per_image=True, rows_per_image=49, addend=ad, add=kw["add"], out=target, out_bits=True)
        torch.cuda.synchronize()
        assert out is target and np.array_equal(target.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), want_bits)


@pytest.mark.parametrize("channels", [64, 80])
def test_an_unaligned_tensor_takes_the_row_layout(channels):
    args, kw, want, want_bits = _case(3 + channels, 3, 49, channels, True, True)
    x, operand, q1, q2, qo = args
    n = x.size
    pad = lambda a: torch.from_numpy(np.concatenate([np.zeros(5, np.int8), a.reshape(-1)])).to(DEV)[5:5 + n].view(x.shape)
    xd, ad, od = pad(x), pad(kw["addend"]), pad(np.zeros_like(x))
    assert xd.data_ptr() % 16 == 5
    out, bits, L = amd.mul_int8(xd, torch.from_numpy(operand).to(DEV), q1, q2, qo, per_image=True, rows_per_image=49, addend=ad,
                                add=kw["add"], out=od, out_bits=True, report_launch=True)
    torch.cuda.synchronize()
    assert L["flat"] == 0 and np.array_equal(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), want_bits)


def test_a_tensor_of_more_than_two_to_the_24_rows():
    """2^24 + 2 rows of 16 channels (268 million elements, 256 MiB per tensor): a tensor past 2^31 elements would need 2 GiB per
    buffer and minutes of NumPy, so this is the 'just above 2^24 rows' case -- row and chunk indices beyond 24 bits, which a float
    or 24-bit multiply would lose, at 3 rows per image so that 5.6 million gate rows are indexed.  The reference goes through a
    65 536-entry table of gate_i8_ref's results over all pairs, not element by element."""
    rows, C, rpi = (1 << 24) + 2, 16, 3
    (q1, q2, qo), = G.mul_draws(1, 5)
    q_ad, q_sum = (float(np.float32(qo[0] * 1.3)), 7), (float(np.float32(qo[0] * 2.0)), -3)
    g = torch.Generator(device=DEV).manual_seed(1)
    xd = torch.randint(-128, 128, (rows, C), dtype=torch.int8, device=DEV, generator=g)
    gd = torch.randint(-128, 128, (rows // rpi, C), dtype=torch.int8, device=DEV, generator=g)
    out, bits = amd.mul_int8(xd, gd, q1, q2, qo, per_image=True, rows_per_image=rpi, out_bits=True)
    torch.cuda.synchronize()
    a, b = ar.all_pairs()
    table = torch.from_numpy(G.mul_q(a, b, q1, q2, qo)).to(DEV).reshape(-1)
    idx = (xd.to(torch.int64) + 128) * 256 + (gd.repeat_interleave(rpi, dim=0).to(torch.int64) + 128)
    want = table[idx]
    assert torch.equal(out, want)
    tail = want[-4096:].cpu().numpy()
    assert np.array_equal(bits[-4096:].cpu().numpy(), ar.bitpack(tail, qo[1]))
    del idx, want
    # the ADD on the same tensor, in place on the addend; the last rows against the restatement
    ad = torch.randint(-128, 128, (rows, C), dtype=torch.int8, device=DEV, generator=g)
    ad_tail = ad[-4096:].cpu().numpy()
    amd.mul_int8(xd, gd, q1, q2, qo, per_image=True, rows_per_image=rpi, addend=ad, add=(q_ad, q_sum), out=ad)
    torch.cuda.synchronize()
    first = rows - 4096
    x_tail = xd[-4096:].cpu().numpy()
    g_tail = gd[first // rpi:].cpu().numpy().repeat(rpi, axis=0)[first % rpi:first % rpi + 4096]
    assert np.array_equal(ad[-4096:].cpu().numpy(), G.mul_add_q(x_tail, g_tail, ad_tail, q1, q2, qo, 0, q_ad, q_sum))


@pytest.mark.parametrize("shape", [(3, 64), (5, 7, 7, 33), (1, 1)])
def test_logistic(shape):
    q_in = (0.03, -7)
    x = np.random.default_rng(shape[-1]).integers(-128, 128, shape).astype(np.int8)
    out, bits = amd.logistic_int8(x, q_in, out_bits=True)
    assert np.array_equal(out, G.logistic_q(x, q_in)) and not bits.any()
    xd = torch.from_numpy(x).to(DEV)
    out, bits = amd.logistic_int8(xd, q_in, out=xd, table=torch.from_numpy(amd.logistic_int8_table(q_in)).to(DEV))
    torch.cuda.synchronize()
    assert out is xd and bits is None and np.array_equal(xd.cpu().numpy(), G.logistic_q(x, q_in))


def test_hip_graph_capture_and_one_replay():
    args, kw, want, want_bits = _case(99, 3, 49, 64, True, True)
    x, operand, q1, q2, qo = args
    xd, gd, ad = (torch.from_numpy(a).to(DEV) for a in (x, operand, kw["addend"]))
    out, bits = torch.zeros_like(xd), torch.zeros((147, 2), dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    call = lambda: amd.mul_int8(xd, gd, q1, q2, qo, per_image=True, rows_per_image=49, addend=ad, add=kw["add"], out=out, out_bits=bits,
                                stream=s.cuda_stream)
    with torch.cuda.stream(s):
        call()                                                       # eager first
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            call()
    x2 = np.random.default_rng(1).integers(-128, 128, x.shape).astype(np.int8)
    xd.copy_(torch.from_numpy(x2))
    out.zero_(), bits.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = G.mul_add_q(x2, operand, kw["addend"], q1, q2, qo, 0, kw["add"][0], kw["add"][1], kw["add"][2], 49)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), ar.bitpack(want, kw["add"][1][1]))


# ---- sections -------------------------------------------------------------------------------------------------------------------------
NAMES = tuple(M.NAMES.split(","))
_MODEL = {}


def _model():
    """The fixture and its NumPy forward at batch 1 and 3, computed once."""
    if not _MODEL:
        data, xt, out, info = M.realtobinary_i8_model()
        xs = {n: np.random.default_rng(n).integers(-128, 128, (n, 8, 8, 64), dtype=np.int8) for n in (1, 3)}
        _MODEL.update(data=data, out=out, info=info, xs=xs, want={n: M.realtobinary_i8_forward(x, info)[0] for n, x in xs.items()})
    return _MODEL


@pytest.mark.parametrize("batch", [1, 3])
def test_the_realtobinary_body_runs_as_one_section_and_each_gate_as_one_launch(batch):
    m = _model()
    x, want = m["xs"][batch], m["want"][batch]
    it = mr.Interpreter(m["data"], batch_size=batch, passes=NAMES)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert np.array_equal(got, want)
    # one launch per block, MUL and ADD in it; the first block's sum feeds the second block's LceQuantize; the ADDs are not int8_add's
    assert it.model.gate_i8_stats() == (2, 4, 1) and it.model.int8_add_stats() == (0, 0)
    assert np.array_equal(it.predict(x), want)
    # without int8_add: the MUL is a launch of its own (one operator), the ADD the host's -- the same bytes
    cut = mr.Interpreter(m["data"], batch_size=batch, passes=("head_i8", "reshape", "gate_i8"))
    assert len(cut.sections) == 2
    v = x
    for k, bi in enumerate(m["info"]["blocks"]):
        (product,) = cut.run_section(k, [v])
        assert cut.model.gate_i8_stats() == (1, 1, 0)
        v = ar.add_q(product, v, (bi["q_m"][0], bi["q_m"][1], bi["q_in"][0], bi["q_in"][1], bi["q_o"][0], bi["q_o"][1]), bi["add_act"])
    assert np.array_equal(v, want)


def test_hip_graphs_eager_record_replay():
    m = _model()
    x, want = m["xs"][3], m["want"][3]
    it = mr.Interpreter(m["data"], batch_size=3, passes=NAMES)
    xd = torch.from_numpy(x).to(DEV)
    y = torch.zeros(want.shape, dtype=torch.int8, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    it.model.use_hip_graphs(True)
    with torch.cuda.stream(s):
        for _ in range(3):
            y.zero_()
            it.model.run_section(0, 3, [xd.data_ptr()], [y.data_ptr()], s.cuda_stream)
            s.synchronize()
            assert np.array_equal(y.cpu().numpy(), want)
    assert it.model.graph_stats()[0] == 1 and it.model.gate_i8_stats() == (2, 4, 1)
    it.model.use_hip_graphs(False)


@pytest.mark.parametrize("case", M.CONTROLS)
def test_each_well_formed_operator_in_its_section(case):
    data, k, inputs, ref = M.single_op_model(case)
    g = np.random.default_rng(3)
    x = g.standard_normal((6, 4, 4, 32)).astype(np.float32)
    plain = mr.Interpreter(data, batch_size=6)
    (y,) = plain.run_section(0, [x])
    extra = [g.integers(-128, 128, (6,) + tuple(plain.model.tensors[t].shape[1:])).astype(np.int8) for t in inputs[1:]]
    want = ref(*extra, y)
    it = mr.Interpreter(data, batch_size=6, passes=("gate_i8", "head_i8"))
    assert [s.ops for s in it.sections] == [list(range(k + 1))]
    (got,) = it.run_section(0, [x] + extra)
    assert np.array_equal(got, want), case
    assert it.model.gate_i8_stats() == ((1, 1, 0) if case.startswith("mul") else (0, 0, 0))
