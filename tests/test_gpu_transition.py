"""lce_hip_pool_depthwise_f32 / lce_hip_pool_depthwise_i8 on the MI355X, byte for byte and without tolerance: the cases of
tests/transition_cases.py (the host simulation's) through the real entries on both paths against the composition of the two NumPy
references (tests/transition_ref.py) and against lce_hip_pool2d followed by lce_hip_depthwise_conv2d_f32 / _i8 on the device; the three
output combinations with marks around them; more work than one pass of the grid; one launch captured in a HIP graph and replayed;
the refusals that need device pointers; and the float and int8 transition fixtures and the int8 network as ONE section with
passes=("transition",) against the fixtures' own forward and the same file opened without the name -- the float pair as one launch,
eagerly and as a HIP graph, the int8 pair as the two launches the reader leaves it."""
import importlib

import numpy as np
import pytest

import depthwise_i8_models as DM
import depthwise_i8_ref as DI
import transition_cases as TC
import transition_ref as R
from section_models import quicknet_transition_model
from test_depthwise_sections_host import ALL_FLAGS

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = ("transition",)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def marked(shape, dtype, mark):
    """A tensor of `shape` filled with `mark`, 16-byte aligned, with 64 marker bytes on each side.  Returns (the view, the buffer)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = torch.from_numpy(np.frombuffer(np.full(1, mark, dtype).tobytes() * ((n + 128) // np.dtype(dtype).itemsize), np.uint8).copy()).to(DEV)
    t = raw[64:64 + n].view(torch.float32 if dtype == np.float32 else torch.int8).view(shape)
    assert t.data_ptr() % 16 == 0
    return t, raw


def _finish(out, raw, bits, took, mark_bytes):
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    n = out.numel() * out.element_size()
    assert raw[:64].tobytes() == mark_bytes * (64 // len(mark_bytes)) and raw[64 + n:].tobytes() == mark_bytes * (64 // len(mark_bytes))
    return out.cpu().numpy(), bits.cpu().numpy(), bool(took)


def _pool_kw(pool):
    return dict(pool_stride=pool["stride"], pool_padding=pool["padding"], pool_activation=pool.get("activation", amd.ACT_NONE))


def run_f32(x, pool, w, bias, stride, padding, m, act, want_out=True, want_bits=True, path=None):
    """amd.pool_depthwise into marked buffers: (out, bits, took the 16-byte path) as NumPy arrays; an output that was not asked for
    comes back as its marks, and the 64 bytes on each side of the value output must still be marks."""
    shape = R.pool_depthwise(np.zeros((1,) + x.shape[1:], np.float32), pool, w, None, stride, padding, m).shape[1:]
    out, raw = marked((x.shape[0],) + shape, np.float32, TC.OUT_MARK_F32)
    bits = torch.full((x.shape[0],) + shape[:2] + ((shape[2] + 31) // 32,), int(TC.BITS_MARK), dtype=torch.int32, device=DEV)
    _, _, took = amd.pool_depthwise(dev(x), pool["filter"], dev(w), dev(bias), stride=stride, padding=padding, depth_multiplier=m, activation=act,
                                    out=out if want_out else False, out_bits=bits if want_bits else False, path=path, report_path=True,
                                    **_pool_kw(pool))
    return _finish(out, raw, bits, took, np.float32(TC.OUT_MARK_F32).tobytes())


def run_i8(x, pool, w, bias, sw, q_out, stride, padding, m, act, want_out=True, want_bits=True, path=None):
    q_in = (pool["scale"], pool["zero_point"])
    table, _, _ = amd.depthwise_conv2d_i8_prepare(w, bias, sw, q_in, q_out, m, act)
    assert np.array_equal(table, DI.table(w, bias, sw, q_in[0], q_out[0]))
    shape = R.pooled(np.zeros((1,) + x.shape[1:], np.int8), pool).shape
    oh, ow = (DI.out_and_pad(shape[1 + k], w.shape[1 + k], stride[k], padding)[0] for k in (0, 1))
    shape = (x.shape[0], oh, ow, w.shape[3])
    out, raw = marked(shape, np.int8, TC.OUT_MARK_I8)
    bits = torch.full(shape[:3] + ((shape[3] + 31) // 32,), int(TC.BITS_MARK), dtype=torch.int32, device=DEV)
    _, _, took = amd.pool_depthwise_i8(dev(x), pool["filter"], dev(w), dev(table), q_in, q_out, stride=stride, padding=padding, depth_multiplier=m,
                                       activation=act, out=out if want_out else False, out_bits=bits if want_bits else False, path=path,
                                       report_path=True, **_pool_kw(pool))
    return _finish(out, raw, bits, took, np.int8(TC.OUT_MARK_I8).tobytes())


def _paths(c, chunk):
    """The entry's own choice, the row path, and -- where the operands qualify with both outputs -- the 16-byte path forced."""
    return (None, 0, 1) if TC.expect_vec(c, chunk, True) else (None, 0)


def _with_forced(run):
    """`run` reporting a forced 16-byte path as the cases' checks expect a path to be reported: only the entry's own choice counts."""
    def wrapped(*a, path=None, **kw):
        out, bits, vec = run(*a, path=path, **kw)
        assert path != 1 or vec
        return out, bits, vec and path is None
    return wrapped


# ---- the entries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.F32))
def test_the_float_cases_on_both_paths_against_the_composition(name):
    c = TC.F32[name]
    TC.check_f32(_with_forced(run_f32), c, paths=_paths(c, 4))


@pytest.mark.parametrize("name", sorted(TC.I8))
def test_the_int8_cases_on_both_paths_against_the_composition(name):
    c = TC.I8[name]
    TC.check_i8(_with_forced(run_i8), c, paths=_paths(c, 16))


@pytest.mark.parametrize("name", sorted(TC.F32))
def test_the_float_cases_against_the_two_launches(name):
    c = TC.F32[name]
    x, w, bias = (dev(a) for a in TC.operands_f32(c))
    pool = c["pool"]
    pooled, _ = amd.pool2d(x, amd.POOL_MAX, pool["filter"], pool["stride"], pool["padding"], pool["activation"])
    kw = dict(stride=c["stride"], padding=c["padding"], depth_multiplier=c["m"], activation=c["act"], out_bits=True)
    want, want_bits = amd.depthwise_conv2d(pooled, w, bias, **kw)
    for path in _paths(c, 4):
        got, bits = amd.pool_depthwise(x, pool["filter"], w, bias, path=path, **kw, **_pool_kw(pool))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(bits, want_bits), (name, path)


@pytest.mark.parametrize("name", sorted(TC.I8))
def test_the_int8_cases_against_the_two_launches(name):
    c = TC.I8[name]
    x, pool, w, bias, sw, q_out = TC.operands_i8(c)
    q_in = (pool["scale"], pool["zero_point"])
    table = dev(amd.depthwise_conv2d_i8_prepare(w, bias, sw, q_in, q_out, c["m"], c["act"])[0])
    x, w = dev(x), dev(w)
    pooled, _ = amd.pool2d(x, amd.POOL_MAX, pool["filter"], pool["stride"], pool["padding"], pool["activation"], scale=q_in[0], zero_point=q_in[1])
    kw = dict(stride=c["stride"], padding=c["padding"], depth_multiplier=c["m"], activation=c["act"], out_bits=True)
    want, want_bits = amd.depthwise_conv2d_i8(pooled, w, table, q_in, q_out, **kw)
    for path in _paths(c, 16):
        got, bits = amd.pool_depthwise_i8(x, pool["filter"], w, table, q_in, q_out, path=path, **kw, **_pool_kw(pool))
        assert torch.equal(got, want) and torch.equal(bits, want_bits), (name, path)


@pytest.mark.parametrize("path", (None, 0))
def test_more_work_than_one_pass_of_the_grid(path):
    """6 x 40 x 40 output pixels of 224 channels against a grid of 2048 blocks of four waves: 537 600 float chunks are 8400 wave tasks
    and the row paths have 38 400 segments, so their grid-stride loops run, with a stride that is no multiple of a pixel's 56
    chunks.  (The int8 16-byte path has 2100 wave tasks here: its loop is the same walk, which the host simulation strides.)"""
    c = TC.quicknet((6, 80, 79, 224), act=R.RELU, seed=70)
    x, w, bias = TC.operands_f32(c)
    want = TC.want_f32(c, x, w, bias)
    out, bits = amd.pool_depthwise(x, (2, 2), w, bias, stride=2, activation=c["act"], out_bits=True, path=path)
    assert np.array_equal(out.view(np.int32), want.view(np.int32)) and np.array_equal(bits, R.bitpack_f32(want))
    x, pool, w, bias, sw, q_out = TC.operands_i8(c)
    want = TC.want_i8(c, x, pool, w, bias, sw, q_out)
    q_in = (pool["scale"], pool["zero_point"])
    table = amd.depthwise_conv2d_i8_prepare(w, bias, sw, q_in, q_out, 1, c["act"])[0]
    out, bits = amd.pool_depthwise_i8(x, (2, 2), w, table, q_in, q_out, stride=2, activation=c["act"], out_bits=True, path=path)
    assert np.array_equal(out, want) and np.array_equal(bits, DI.bitpack(want, q_out[1]))


def test_a_capture_and_replay_of_the_launch():
    """The launch allocates and copies nothing: captured once into a HIP graph on the caller's stream, replayed on new contents of
    the same buffers, against the composition."""
    c = TC.quicknet((2, 9, 8, 64), seed=80)
    x, w, bias = TC.operands_f32(c)
    xd, wd, bd = dev(x), dev(w), dev(bias)
    out = torch.zeros((2, 5, 4, 64), dtype=torch.float32, device=DEV)
    bits = torch.zeros((2, 5, 4, 2), dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        amd.pool_depthwise(xd, (2, 2), wd, bd, stride=2, out=out, out_bits=bits, stream=s.cuda_stream)          # eager first
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            amd.pool_depthwise(xd, (2, 2), wd, bd, stride=2, out=out, out_bits=bits, stream=s.cuda_stream)
    for seed in (1, 2):
        x2 = (np.random.default_rng(seed).standard_normal(x.shape) * 4).astype(np.float32)
        xd.copy_(torch.from_numpy(x2))
        out.zero_(), bits.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = TC.want_f32(c, x2, w, bias)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)) and np.array_equal(bits.cpu().numpy(), R.bitpack_f32(want))


def test_refusals_on_the_device():
    flat = torch.zeros(2 * 2 * 8 * 8 * 64, dtype=torch.float32, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:2 * 8 * 8 * 64 - 64 + 2 * 4 * 4 * 64].view(2, 4, 4, 64)
    w = torch.zeros(1, 3, 3, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.pool_depthwise(x, (2, 2), w, stride=2, out=out)
    with pytest.raises(amd.LceHipError, match="the two outputs overlap"):
        both = torch.zeros(2 * 4 * 4 * 64, dtype=torch.float32, device=DEV)
        amd.pool_depthwise(x, (2, 2), w, stride=2, out=both.view(2, 4, 4, 64), out_bits=both[:64].view(torch.int32).view(2, 4, 4, 2))
    with pytest.raises(amd.LceHipError, match="the 16-byte path needs"):
        amd.pool_depthwise(x, (3, 3), w, pool_stride=2, stride=2, path=1)                 # the pool's geometry
    x8 = torch.zeros(1, 4, 4, 32, dtype=torch.int8, device=DEV)
    w8 = torch.zeros(1, 3, 3, 32, dtype=torch.int8, device=DEV)
    table = torch.zeros(3, 32, dtype=torch.int32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the table"):
        amd.pool_depthwise_i8(x8, (2, 2), w8, table, (0.5, 0), (0.5, 0), stride=2, out=table.view(torch.int8).view(-1)[:128].view(1, 2, 2, 32))
    torch.cuda.synchronize()
    assert (flat == 0).all() and (table == 0).all()                                       # nothing was written


# ---- sections -------------------------------------------------------------------------------------------------------------------------
def _stats(model):
    return dict(transition=model.transition_stats(), pool=model.pool_stats(), depthwise=model.depthwise_stats(),
                depthwise_i8=model.depthwise_i8_stats())


@pytest.mark.parametrize("batch", [1, 3])
def test_the_float_transition_as_one_section(batch):
    from test_gpu_depthwise import run_cut, same
    data, xt, out, info = quicknet_transition_model()
    x = np.random.default_rng(batch).standard_normal((batch, info["size"], info["size"], info["channels"])).astype(np.float32)
    cut = run_cut(data, info, x)                                       # the fixture's own forward: NumPy does every builtin operator
    two = mr.Interpreter(data, batch_size=batch, **ALL_FLAGS)
    one = mr.Interpreter(data, batch_size=batch, passes=NEW, **ALL_FLAGS)
    assert [s.ops for s in one.sections] == [s.ops for s in two.sections] and len(one.sections) == 1
    (want,), (got,) = two.run_section(0, [x]), one.run_section(0, [x])
    assert same(got, want) and same(got, cut[out])
    assert _stats(two.model) == dict(transition=(0, 0, 0), pool=(1, 0), depthwise=(1, 0), depthwise_i8=(0, 0))
    assert _stats(one.model) == dict(transition=(1, 2, 0), pool=(0, 0), depthwise=(0, 0), depthwise_i8=(0, 0))
    assert one.model.conv1x1_stats() == two.model.conv1x1_stats() == (1, 1)
    assert same(one.predict(x), want)


@pytest.mark.parametrize("name", ["transition_per_channel", "transition_per_tensor", "network_per_channel", "network_per_tensor"])
def test_the_int8_fixtures_as_one_section(name):
    """The reader leaves an int8 pair as two launches (lce_hip_pool_depthwise_i8 measured slower than they are,
    profiles/transition/layers.txt): with the name the bytes are the fixture's own forward's and the counters are unmoved."""
    batch = 3
    data, xt, out, info = DM.FIXTURES[name]()
    x = DM.fixture_input(info, batch, 1)
    two = mr.Interpreter(data, batch_size=batch, **DM.EVERY_FLAG)
    one = mr.Interpreter(data, batch_size=batch, passes=NEW, **DM.EVERY_FLAG)
    assert [s.ops for s in one.sections] == [s.ops for s in two.sections] and len(one.sections) == 1
    (base,), (got,) = two.run_section(0, [x]), one.run_section(0, [x])
    want = info["oracle"](x)
    assert got.dtype == info["out_dtype"] and np.array_equal(got.reshape(want.shape).view(np.uint8), want.view(np.uint8))
    assert np.array_equal(got.view(np.uint8), base.view(np.uint8)) and np.unique(got).size > 3
    n_dw = info["stats"]["depthwise_i8"][0]
    assert _stats(two.model) == _stats(one.model) == dict(transition=(0, 0, 0), pool=(1, 0), depthwise=(0, 0), depthwise_i8=(n_dw, 0))
    assert one.model.conv_i8_stats() == info["stats"]["conv_i8"] and one.model.int8_add_stats() == info["stats"]["int8_add"]
    assert np.array_equal(one.predict(x).reshape(want.shape).view(np.uint8), want.view(np.uint8))


def test_the_folded_quantize_and_the_walkers_refusals_on_the_device():
    """The small model of tests/transition_models.py: the blur feeds only an LceQuantize, which folds into the fused launch (one launch,
    two operators, one LceQuantize); with an AVERAGE pool, a second reader of the pooled tensor or the pooled tensor delivered, two
    launches remain.  Every variant gives the bytes of the same file opened without the name."""
    import transition_models as TM
    for variant, fused in ((None, True), ("average", False), ("second_reader", False), ("deliver_pooled", False)):
        data, xt, outs, info = TM.pool_blur_model(**({variant: True} if variant else {}))
        x = np.random.default_rng(3).standard_normal((2, info["size"], info["size"], info["channels"])).astype(np.float32)
        two = mr.Interpreter(data, batch_size=2, **TM.FLAGS)
        one = mr.Interpreter(data, batch_size=2, passes=NEW, **TM.FLAGS)
        assert [s.ops for s in one.sections] == [s.ops for s in two.sections] and len(one.sections) == 1
        want, got = two.run_section(0, [x]), one.run_section(0, [x])
        assert len(got) == len(outs) and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want)), variant
        assert (_stats(two.model)["transition"], two.model.pool_stats(), two.model.depthwise_stats()) == ((0, 0, 0), (1, 0), (1, 1))
        assert _stats(one.model)["transition"] == ((1, 2, 1) if fused else (0, 0, 0)), variant
        assert (one.model.pool_stats(), one.model.depthwise_stats()) == (((0, 0), (0, 0)) if fused else ((1, 0), (1, 1))), variant


def test_hip_graph_replay_of_a_section_gives_the_same_bytes():
    data, xt, out, info = quicknet_transition_model()
    model = mr.LceModel(data, passes=NEW, **ALL_FLAGS)
    batch = 5
    xh = np.random.default_rng(11).standard_normal((batch, info["size"], info["size"], info["channels"])).astype(np.float32)
    x = torch.from_numpy(xh).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    y = torch.zeros(dims, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(s):
        model.use_hip_graphs(True)
        for _ in range(3):                                            # eager, then recorded, then replayed
            y.zero_()
            model.run_section(0, batch, [x.data_ptr()], [y.data_ptr()], s.cuda_stream)
            s.synchronize()
            runs.append((y.clone(), model.transition_stats(), model.pool_stats(), model.graph_stats()))
    assert [r[3] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1:3] for r in runs] == [((1, 2, 0), (0, 0))] * 3
    model.use_hip_graphs(False)
    (want,) = mr.Interpreter(data, batch_size=batch, **ALL_FLAGS).run_section(0, [xh])
    for r in runs:
        assert np.array_equal(r[0].cpu().numpy().view(np.uint8), np.ascontiguousarray(want).reshape(dims).view(np.uint8))
