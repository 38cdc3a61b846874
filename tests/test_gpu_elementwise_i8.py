"""lce_hip_elementwise_i8 on the MI355X, byte for byte with no tolerance against the NumPy restatement of the header's arithmetic
(tests/elementwise_i8_ref.py): the shapes of the CPU simulation, every path forced and the default, a head over ALL 65 536 input
pairs in every channel, the largest table the LDS path takes and the first the global path must, a launch whose waves stride, and
a HIP-graph capture with one replay."""
import importlib

import numpy as np
import pytest

import elementwise_i8_ref as E
from test_elementwise_i8_hostsim import SHAPES, _case

torch = pytest.importorskip("torch")
amd = importlib.import_module("compute-engine_amd")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS, GLOBAL, ONE_ROW = amd.EW_I8_PATH_LDS, amd.EW_I8_PATH_GLOBAL, amd.EW_I8_PATH_ONE_ROW


def run(x, q_in, steps, addend=None, head=None, path=None, **kw):
    table = amd.elementwise_i8_prepare(x.shape[-1], q_in, steps, head=head)
    xd = torch.from_numpy(x).to(DEV)
    ad = None if addend is None else torch.from_numpy(addend).to(DEV)
    kw.setdefault("out_bits", True)
    out, bits, launch = amd.elementwise_i8(xd, torch.from_numpy(table).to(DEV), q_in, steps, addend=ad, head=head, path=path,
                                           report_launch=True, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy(), launch


def by_table(x, q_in, steps):
    """The chain without a head through the NumPy restatement's OWN table (elementwise_i8_ref.table: ``chain`` on all 256 values of
    every channel) -- for tensors too large to push through int64 arithmetic element by element in a few seconds."""
    t = E.table(x.shape[-1], q_in, steps).view(np.int8)
    row = (np.arange(x.shape[-1], dtype=np.int32) * 256) if t.shape[0] > 1 else np.zeros(x.shape[-1], np.int32)
    out = np.take(t.reshape(-1), row[None, :] + (x.view(np.uint8) ^ 0x80))
    last = steps[-1]
    return out, E.ar.bitpack(out, (last[3] if last[0] in ("add", "prelu") else last[1])[1])


@pytest.mark.parametrize("rows,channels", SHAPES)
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("path", [None, LDS, GLOBAL, ONE_ROW])
def test_the_shapes_of_the_simulation_on_every_path(rows, channels, head, path):
    x, addend, q_in, h, steps, want = _case(rows * 1000 + channels, rows, channels, head, per_channel=path != ONE_ROW)
    out, bits, L = run(x, q_in, steps, addend, h, path)
    assert L["path"] == ((ONE_ROW if channels == 1 else GLOBAL) if path is None else path) and L["flat"] == (channels % 32 == 0)
    assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])
    # either output alone, and in place on the input
    out, bits, _ = run(x, q_in, steps, addend, h, path, out=False)
    assert out is None and np.array_equal(bits, want[1])
    xd = torch.from_numpy(x).to(DEV)
    ad = None if addend is None else torch.from_numpy(addend).to(DEV)
    table = torch.from_numpy(amd.elementwise_i8_prepare(channels, q_in, steps, head=h)).to(DEV)
    amd.elementwise_i8(xd, table, q_in, steps, addend=ad, head=h, out=xd, path=path)
    assert np.array_equal(xd.cpu().numpy(), want[0])


@pytest.mark.parametrize("channels", [2, 32])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_head_over_all_pairs_in_every_channel(channels, seed):
    """x1 = (r + c) & 255, x2 = ((r >> 8) + 3 c) & 255 over 65 536 rows: every channel meets every (x1, x2) pair, and the draws
    meet every variant of the head's arithmetic the host proves."""
    g = np.random.default_rng(seed)
    q_in, head, steps = E.reactnet_tail(g, channels)
    if seed == 0:
        head = ((q_in[0], 3), (float(np.float32(q_in[0] * 1.5)), -5), 0)     # equal input scales: the shift form
        q, steps = head[1], []
        for kind in ("add", "prelu", "add"):
            steps.append(E.draw_step(g, kind, q, channels, True))
            q = steps[-1][3]
    r, c = np.arange(65536, dtype=np.int64)[:, None], np.arange(channels, dtype=np.int64)[None, :]
    x1 = ((r + c) & 255).astype(np.uint8).view(np.int8)
    x2 = (((r >> 8) + 3 * c) & 255).astype(np.uint8).view(np.int8)
    pairs = {(int(a), int(b)) for a, b in zip(x1[:, channels - 1], x2[:, channels - 1])}
    assert len(pairs) == 65536
    want = E.chain(x1, q_in, steps, x2, head)
    seen = set()
    for path in (None, LDS, GLOBAL):
        out, bits, L = run(x1, q_in, steps, x2, head, path)
        seen.add(L["head_variant"])
        assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1]), (path, L)
    assert seen == {amd.add_int8_params(q_in, head[0], head[1], head[2])["variant"]}
    if seed == 0:
        assert seen == {amd.ADD_INT8_SHIFT}


def _wide(channels, rows, seed):
    g = np.random.default_rng(seed)
    x = g.integers(-128, 128, (rows, channels)).astype(np.int8)
    q_in = (E._scale(g), E._zp(g))
    first = E.draw_step(g, "prelu", q_in, channels, True)
    first = ("prelu", g.integers(-128, 128, channels).astype(np.int8)) + first[2:]
    steps = [first, E.draw_step(g, "add", first[3], channels, True)]
    return x, q_in, steps


def test_the_largest_table_the_lds_path_takes_and_the_global_path_beyond():
    x, q_in, steps = _wide(32, 4, 0)
    top = run(x, q_in, steps)[2]["lds_max_channels"]
    assert top == 608
    for channels, path, want_path in ((top, LDS, LDS), (top, None, LDS), (top, GLOBAL, GLOBAL), (top + 32, None, GLOBAL), (1024, None, GLOBAL),
                                      (630, None, LDS), (631, None, GLOBAL), (128, None, LDS), (96, None, GLOBAL)):
        x, q_in, steps = _wide(channels, 70, channels)
        want = by_table(x, q_in, steps)
        assert np.array_equal(E.chain(x[:3], q_in, steps)[0], want[0][:3])
        out, bits, L = run(x, q_in, steps, path=path)
        assert L["path"] == want_path and L["flat"] == (channels % 32 == 0)
        assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1]), channels
    x, q_in, steps = _wide(top + 32, 4, 1)
    with pytest.raises(amd.LceHipError):
        run(x, q_in, steps, path=LDS)


@pytest.mark.parametrize("channels,path", [(608, LDS), (64, GLOBAL), (64, ONE_ROW)])
def test_more_iterations_than_the_launch_has_waves(channels, path):
    """Sized from the geometry the entry reports: the flat layout takes 4096 elements per wave and iteration."""
    x, q_in, steps = _wide(channels, 8, 2)
    if path == ONE_ROW:
        steps = [("prelu", np.int8(-77)) + steps[0][2:], ("clamp", steps[0][3], 1)]
    table = torch.from_numpy(amd.elementwise_i8_prepare(channels, q_in, steps)).to(DEV)
    probe = torch.empty(((1 << 26) // channels, channels), dtype=torch.int8, device=DEV)      # enough work to reach the grid's cap
    L = amd.elementwise_i8(probe, table, q_in, steps, path=path, report_launch=True)[2]
    waves = L["blocks"] * L["waves_per_block"]
    rows = -(-(waves * 4096 * 5 // 4) // channels)
    x = np.random.default_rng(7).integers(-128, 128, (rows, channels)).astype(np.int8)
    out, bits, L2 = run(x, q_in, steps, path=path)
    assert L2["flat"] == 1 and L2["blocks"] * L2["waves_per_block"] == waves and -(-x.size // 4096) > waves
    want = by_table(x, q_in, steps)
    assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])


def test_hip_graph_capture_and_one_replay():
    x, addend, q_in, h, steps, want = _case(99, 260, 64, True)
    table = torch.from_numpy(amd.elementwise_i8_prepare(64, q_in, steps, head=h)).to(DEV)
    xd, ad = torch.from_numpy(x).to(DEV), torch.from_numpy(addend).to(DEV)
    out, bits = torch.zeros_like(xd), torch.zeros((260, 2), dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    kw = dict(addend=ad, head=h, out=out, out_bits=bits)
    with torch.cuda.stream(s):
        amd.elementwise_i8(xd, table, q_in, steps, stream=s.cuda_stream, **kw)                    # eager first
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            amd.elementwise_i8(xd, table, q_in, steps, stream=s.cuda_stream, **kw)
    x2 = np.random.default_rng(1).integers(-128, 128, x.shape).astype(np.int8)
    xd.copy_(torch.from_numpy(x2))
    out.zero_(), bits.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = E.chain(x2, q_in, steps, addend, h)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(bits.cpu().numpy(), want[1])


# ---- sections -------------------------------------------------------------------------------------------------------------------------
import elementwise_i8_models as M                                                                     # noqa: E402

mr = importlib.import_module("compute-engine_amd.model_runner")
NEW = ("elementwise_i8",)


def by_default_partition(data, info, x):
    """The same file at the default partition: its sections on the GPU, each builtin operator in NumPy (elementwise_i8_models.host_op).
    Returns tensor index -> array for everything that was computed."""
    it = mr.Interpreter(data, batch_size=x.shape[0])
    vals = {it.model.inputs[0]: x}
    ran, progress = set(), True
    while progress:
        progress = False
        for k, sec in enumerate(it.sections):
            if k not in ran and all(t in vals for t in sec.inputs):
                vals.update(zip(sec.outputs, it.run_section(k, [vals[t] for t in sec.inputs])))
                ran.add(k)
                progress = True
        for op, kind, ins, out, params in info["host"]:
            if out not in vals and all(t in vals for t in ins):
                vals[out] = M.host_op(kind, [vals[t] for t in ins], params)
                progress = True
    assert len(ran) == len(it.sections)
    return vals


def rand_i8(shape, seed):
    return np.random.default_rng(seed).integers(-128, 128, shape, dtype=np.int8)


@pytest.mark.parametrize("batch,act", [(3, 0), (16, 1)])
def test_the_reactnet_body_runs_as_one_section_and_each_tail_as_one_launch(batch, act):
    data, xt, out, info = M.reactnet_i8_model(act=act)
    x = rand_i8((batch, 8, 8, 64), batch)
    want = by_default_partition(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, int8_add_sections=True, passes=NEW)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert np.array_equal(got, want[out])
    # one launch per tail, the residual ADD as its head (4 operators each); the first tail's result feeds an LceQuantize
    assert it.model.elementwise_i8_stats() == (2, 8, 1) and it.model.int8_add_stats() == (0, 0)
    assert np.array_equal(it.predict(x), want[out])
    # without int8_add the residual ADD is the host's and the partition is the default one: the same bytes, no launch of the pass
    alone = mr.Interpreter(data, batch_size=batch, passes=NEW)
    assert [s.ops for s in alone.sections] == [s.ops for s in mr.Interpreter(data).sections]


def test_the_requantize_join_runs_as_one_section():
    data, xt, out, info = M.requantize_concat_model()
    x = rand_i8((5, 8, 8, 64), 1)
    want = by_default_partition(data, info, x)
    it = mr.Interpreter(data, batch_size=5, concat_sections=True, passes=NEW)
    assert len(it.sections) == 1
    (got,) = it.run_section(0, [x])
    assert np.array_equal(got, want[out])
    assert it.model.elementwise_i8_stats() == (1, 1, 0) and it.model.concat_stats() == (1, 1)
    assert np.array_equal(it.predict(x), want[out])


def test_the_standalone_relu6_runs_inside_the_section_with_its_bits_folded():
    data, xt, out, info = M.relu6_model()
    x = rand_i8((4, 8, 8, 64), 2)
    want = by_default_partition(data, info, x)
    it = mr.Interpreter(data, batch_size=4, passes=NEW)
    (got,) = it.run_section(0, [x])
    assert np.array_equal(got, want[out]) and it.model.elementwise_i8_stats() == (1, 1, 1)
    # HIP graphs: eager, record + launch, replay
    xd = torch.from_numpy(x).to(DEV)
    y = torch.zeros(got.shape, dtype=torch.int8, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    it.model.use_hip_graphs(True)
    with torch.cuda.stream(s):
        for _ in range(3):
            y.zero_()
            it.model.run_section(0, 4, [xd.data_ptr()], [y.data_ptr()], s.cuda_stream)
        s.synchronize()
    assert it.model.graph_stats()[0] == 1 and it.model.elementwise_i8_stats() == (1, 1, 1)
    assert np.array_equal(y.cpu().numpy(), want[out])
    it.model.use_hip_graphs(False)


@pytest.mark.parametrize("case", M.CONTROLS)
def test_each_well_formed_operator_in_its_section(case):
    data, k, ref = M.single_op_model(case)
    x = np.random.default_rng(3).standard_normal((6, 4, 4, 32)).astype(np.float32)
    plain = mr.Interpreter(data, batch_size=6)
    (y,) = plain.run_section(0, [x])
    want = M.host_op(ref[0], [y], ref[1])
    it = mr.Interpreter(data, batch_size=6, passes=NEW)
    assert [s.ops for s in it.sections] == [[0, 1, k]]
    (got,) = it.run_section(0, [x])
    assert np.array_equal(got, want), case
    assert it.model.elementwise_i8_stats() == (1, 1, 0)
