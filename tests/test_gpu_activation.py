"""lce_hip_elementwise_ex and the activation / reshape / gate sections on the MI355X: the entry byte for byte against
tests/activation_ref.py (both paths, every step kind, the per-image operand on images smaller and larger than a wave's iteration,
a launch at the grid cap), its refusals, and three networks -- a ReActNet-style pair of blocks, a RealToBinary-style gated block,
a head that flattens -- as ONE section each against the composition of the oracle and the restated references."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import activation_models as AM
import activation_ref as AR
import oracle_lib as O
from test_activation_host import FLAT, FLT_MAX, NONE, RELU, ROWS, operands, programs, same

torch = pytest.importorskip("torch")
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(x, steps, **kw):
    out, bits = amd.elementwise_ex(x, steps, **kw)
    return out, bits


# ---- the entry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, _, _ in FLAT + ROWS[:5]] + [(3, 2, 2, 64), (2, 3, 3, 160)])
def test_every_step_kind_on_both_paths(shape):
    o = operands(shape, sum(shape))
    for name, steps in programs(o).items():
        want = AR.chain(o["x"], steps)
        got, bits = run(o["x"], steps, out_bits=True)
        assert same(got, want), (name, shape)
        assert np.array_equal(bits, O.bitpack(want)), (name, shape)              # (ragged channels: the padding bits are 0)
    steps = programs(o)["eight"]
    want = AR.chain(o["x"], steps)
    only_bits = run(o["x"], steps, out=False, out_bits=True)
    assert only_bits[0] is None and np.array_equal(only_bits[1], O.bitpack(want))
    only_float = run(o["x"], steps)
    assert only_float[1] is None and same(only_float[0], want)
    # in place, with both outputs and with the float output alone
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dsteps = [(op, t(v) if isinstance(v, np.ndarray) else v, a) for op, v, a in steps]
    for with_bits in (True, False):
        xd = t(o["x"])
        _, bits = amd.elementwise_ex(xd, dsteps, out=xd, out_bits=True if with_bits else None)
        assert same(xd.cpu().numpy(), want)
        assert bits is None or np.array_equal(bits.cpu().numpy(), O.bitpack(want))


def test_the_row_path_at_32_channels_through_pointers_4_bytes_off():
    shape = (5, 3, 3, 32)
    o = operands(shape, 77)
    steps = programs(o)["eight"]
    want = AR.chain(o["x"], steps)
    def off(a):                                                      # 4 bytes behind a 16-byte boundary
        big = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
        v = big[1:].view(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert v.data_ptr() % 16 == 4
        return v
    dsteps = [(op, off(v) if isinstance(v, np.ndarray) else v, a) for op, v, a in steps]
    out = torch.zeros(o["x"].size + 1, dtype=torch.float32, device=DEV)[1:].view(shape)
    _, bits = amd.elementwise_ex(off(o["x"]), dsteps, out=out, out_bits=True)
    assert same(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), O.bitpack(want))


def test_a_launch_at_the_grid_cap_iterates():
    """More 1024-float blocks than the launcher's grid has waves, so some waves take a second iteration: the channel word and the
    image index advance by the grid stride there."""
    cap = amd.lib().lce_hip_elementwise_grid_cap()
    H, C = 31, 96                                                    # three words per row: the stride is no multiple of a row
    per_image = H * H * C
    batch = cap * 4 * 1024 // per_image + 3
    assert batch * per_image > cap * 4 * 1024 + 1024 and (batch * per_image // 32) % 32 != 0      # ... and a partial last block
    o = operands((batch, H, H, C), 11, special=False)
    steps = [("add", o["shift"], NONE), ("mul", o["gate"], NONE), ("prelu", o["alpha"], NONE), ("add", o["m"], RELU)]
    want = AR.chain(o["x"], steps)
    got, bits = run(o["x"], steps, out_bits=True)
    assert same(got, want) and np.array_equal(bits, O.bitpack(want))


def test_special_values():
    sub = np.float32(1e-40)
    v = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, sub, -sub, FLT_MAX, -FLT_MAX, 1.5, -1.5, 7.0, 104, -104, 88.7, -88.7,
                  np.nextafter(np.float32(-104), np.float32(-200)), np.nextafter(np.float32(-104), np.float32(0)), -100, 1e-3], np.float32)
    for C_ in (32, 20):                                              # the flat and the row path
        x = np.resize(v, (3, 2, 2, C_)).astype(np.float32)
        for alpha in (-2.0, 0.0, 3.0):
            for steps in ([("prelu", alpha, NONE)], [("prelu", np.full(C_, alpha, np.float32), NONE)]):
                assert same(run(x, steps)[0], AR.chain(x, steps))
        for act in (1, 2, 3):
            assert same(run(x, [("clamp", None, act)])[0], AR.clamp(x, act))
        got = run(x, [("logistic", None, NONE)])[0]
        assert same(got, AR.logistic(x))
        assert np.array_equal(got.view(np.uint32)[np.isnan(x)], x.view(np.uint32)[np.isnan(x)])     # a NaN passes unchanged
    relu_of_negative_zero = run(np.full((1, 1, 1, 32), -0.0, np.float32), [("clamp", None, RELU)], out_bits=True)
    assert np.signbit(relu_of_negative_zero[0]).all() and not relu_of_negative_zero[1].any()


def test_the_refusals_launch_nothing():
    x = torch.ones((6, 32), dtype=torch.float32, device=DEV)
    out = torch.full((6, 32), 5.0, dtype=torch.float32, device=DEV)
    g = torch.ones((2, 32), dtype=torch.float32, device=DEV)
    def call(step, rows=6, rpi=3, xp=None, op=None):
        arr = (amd.EwStepEx * 1)(step)
        return amd.lib().lce_hip_elementwise_ex(C.c_void_p(xp or x.data_ptr()), rows, 32, rpi, arr, 1, C.c_void_p(op or out.data_ptr()), None, None)
    S = lambda *a: amd.EwStepEx(*a)
    assert call(S(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, g.data_ptr(), 0.0, 0)) == amd.OK        # (the well-formed call runs)
    torch.cuda.synchronize()
    assert (out == 2).all()
    out.fill_(5.0)
    for rc in (call(S(7, 0, None, 0.0, 0)), call(S(amd.EW_ADD, 9, g.data_ptr(), 0.0, 0)), call(S(amd.EW_CLAMP, 0, None, 0.0, 5)),
               call(S(amd.EW_PRELU, amd.EW_TENSOR, x.data_ptr(), 0.0, 0)), call(S(amd.EW_LOGISTIC, 0, None, 0.0, 1)),
               call(S(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, g.data_ptr(), 0.0, 0), rpi=4),
               call(S(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, g.data_ptr(), 0.0, 0), rpi=0),
               call(S(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, None, 0.0, 0)),
               call(S(amd.EW_ADD, amd.EW_PER_IMAGE_CHANNEL, g.data_ptr() + 2, 0.0, 0)),
               call(S(amd.EW_CLAMP, 0, None, 0.0, 1), xp=x.data_ptr() + 1)):
        assert rc == amd.ERR_INVALID
    torch.cuda.synchronize()
    assert (out == 5).all()
    e = torch.zeros((0, 32), dtype=torch.float32, device=DEV)
    o, b = amd.elementwise_ex(e, [("logistic", None, NONE)], out_bits=True)
    assert o.shape == (0, 32) and b.shape == (0, 1)


# ---- sections -----------------------------------------------------------------------------------------------------------------------
FIXTURES = dict(
    reactnet=(AM.reactnet_model, AM.reactnet_forward, dict(elementwise_sections=True, activation_sections=True)),
    gated=(AM.gated_model, AM.gated_forward, dict(head_sections=True, elementwise_sections=True, **AM.NEW_KEYWORDS)),
    flatten=(AM.flatten_head_model, lambda x, info: AM.flatten_head_forward(x, info)[0], dict(head_sections=True, reshape_sections=True)))


@functools.lru_cache(maxsize=None)
def fixture(name, batch):
    """(file, info, keywords, input, expected output): built and restated once per (network, batch)."""
    build, forward, keywords = FIXTURES[name]
    data, x_t, out_t, info = build()
    x = np.random.default_rng(batch + len(name)).standard_normal((batch,) + info["shape"]).astype(np.float32)
    want = forward(x, info)
    want.setflags(write=False)
    return data, info, keywords, x, want


@pytest.mark.parametrize("batch", [3, 33])
def test_a_reactnet_pair_of_blocks_is_one_section_and_each_tail_one_launch(batch):
    data, info, keywords, x, want = fixture("reactnet", batch)
    it = mr.Interpreter(data, batch_size=batch, **keywords)
    assert len(it.sections) == 1 and it.lce_only
    assert same(it.predict(x), want)
    (got,) = it.run_section(0, [x])
    assert same(got, want)
    # two tails of six operators, one launch each; the first writes the second block's sign bits, the second has no reader of bits
    assert it.model.activation_stats() == (2, 12, 1)
    assert it.model.elementwise_stats() == (0, 0, 0) and it.model.gate_stats() == (0, 0) and it.model.run_stats()[1] == 0


@pytest.mark.parametrize("batch", [3, 33])
def test_a_gated_block_is_one_section(batch):
    data, info, keywords, x, want = fixture("gated", batch)
    it = mr.Interpreter(data, batch_size=batch, **keywords)
    assert len(it.sections) == 1 and it.lce_only
    assert same(it.predict(x), want)
    (got,) = it.run_section(0, [x])
    assert same(got, want)
    assert it.model.head_stats() == (1, 2, 0)
    assert it.model.activation_stats() == (2, 3, 0)                  # the LOGISTIC alone; the gate MUL and the shortcut ADD together
    assert it.model.gate_stats() == (1, 0) and it.model.reshape_stats() == (1, 0) and it.model.elementwise_stats() == (0, 0, 0)


@pytest.mark.parametrize("batch", [3, 33])
def test_a_flatten_head_is_one_section(batch):
    data, info, keywords, x, want = fixture("flatten", batch)
    it = mr.Interpreter(data, batch_size=batch, **keywords)
    assert len(it.sections) == 1 and it.lce_only
    got = it.predict(x)
    assert got.shape == (batch, 10) and same(got, want)
    assert it.model.reshape_stats() == (1, 0) and it.model.head_stats() == (0, 1, 1)
    # the flattened tensor delivered as well: the view becomes ONE copy into the caller's buffer
    data2, _, outs, info2 = AM.flatten_head_model(deliver_flat=True)
    it2 = mr.Interpreter(data2, batch_size=batch, **keywords)
    by_tensor = dict(zip(it2.sections[0].outputs, it2.run_section(0, [x])))
    assert same(by_tensor[outs[0]], want) and same(by_tensor[outs[1]], AM.flatten_head_forward(x, info2)[1])
    assert it2.model.reshape_stats() == (0, 1)


@pytest.mark.parametrize("name", ["reactnet", "gated"])
def test_hip_graph_replay_gives_the_same_bytes(name):
    batch = 3
    data, info, keywords, x, want = fixture(name, batch)
    model = mr.LceModel(data, **keywords)
    xd = torch.from_numpy(x).to(DEV)
    out_t = model.sections[0].outputs[0]
    dims, _ = model.section_tensor_shape(0, out_t, batch)
    eager = torch.empty(dims, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model.run_section(0, batch, [xd.data_ptr()], [eager.data_ptr()], s.cuda_stream)
        s.synchronize()
        stats = model.activation_stats()
        model.use_hip_graphs(True)
        y = torch.empty_like(eager)
        for _ in range(3):
            y.zero_()
            model.run_section(0, batch, [xd.data_ptr()], [y.data_ptr()], s.cuda_stream)
        s.synchronize()
    assert model.graph_stats()[0] == 1 and model.activation_stats() == stats
    assert same(eager.cpu().numpy(), want) and same(y.cpu().numpy(), eager.cpu().numpy())
    model.use_hip_graphs(False)
