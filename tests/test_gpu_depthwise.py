"""lce_hip_depthwise_conv2d_f32 and the depthwise sections on the MI355X, exact and without tolerance: the kernels against the
NumPy reference (tests/depthwise_ref.py: the fmaf chain over the in-bounds taps in raster order) over the grid of images, batches,
channel counts, filters, strides, paddings, bias, activations, multipliers and output combinations, the bits against the oracle's
LceQuantize of the reference, the known answers worked by hand, more chunks than one pass of the capped grid, a 4-byte-offset
view, one convolution whose input exceeds 2^32 bytes, and the fixtures of tests/test_depthwise_sections_host.py run as ONE section
against the same file under the default partition with NumPy doing every builtin operator.  NaN positions are compared as
positions, every other byte as a byte."""
import importlib

import numpy as np
import pytest

import depthwise_ref as R
import oracle_lib as O
from section_models import DEPTHWISE_CONV_2D, float_fixture
from test_depthwise_sections_host import ACTS, ALL_FLAGS, FIXTURES, KNOWN, OLD_FLAGS, grid_operands, known_case

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GRID_IMAGES = [(1, 1), (5, 7), (8, 8)]
GRID_BATCHES = (1, 3)
GRID_CHANNELS = (1, 3, 4, 31, 32, 33, 64, 100)
GRID_FILTERS = ((1, 1), (2, 2), (3, 3), (5, 3))
GRID_STRIDES = ((1, 1), (2, 2), (2, 1), (3, 4))
GRID_PADDINGS = (R.SAME, R.VALID)


def agree(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(x, w, bias=None, **kw):
    out, bits = amd.depthwise_conv2d(dev(x) if isinstance(x, np.ndarray) else x, dev(w) if isinstance(w, np.ndarray) else w,
                                     dev(bias) if isinstance(bias, np.ndarray) else bias, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def check(xd, wd, bd, kw, want):
    """The three output combinations of one convolution against the reference `want` and the oracle's bits of it."""
    want_bits = O.bitpack(want)
    got, none = run(xd, wd, bd, **kw)
    assert none is None and agree(got, want), kw
    both = run(xd, wd, bd, out_bits=True, **kw)
    assert agree(both[0], want) and np.array_equal(both[1], want_bits), kw
    only = run(xd, wd, bd, out=False, out_bits=True, **kw)
    assert only[0] is None and np.array_equal(only[1], want_bits), kw


def sweep(cin, m):
    """Every image, batch, filter, stride and padding of the grid at `cin` input channels and multiplier `m`, with and without
    special values; the chain is computed once per geometry, bias and clamp on top of it.  Returns the number of checks."""
    n = 0
    cout = cin * m
    for special in (False, True):
        for filt in GRID_FILTERS:
            w, bias = grid_operands(filt, cout, special)
            wd, bd = dev(w), dev(bias)
            for image in GRID_IMAGES:
                for batch in GRID_BATCHES:
                    x = float_fixture((batch, *image, cin), image[0] * 1000 + batch * 100 + cin, special)
                    xd = dev(x)
                    for stride in (GRID_STRIDES if not special else GRID_STRIDES[::3]):
                        for padding in GRID_PADDINGS:
                            if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
                                continue                                         # an empty output
                            t = R.chain(x, w, stride, padding, m)
                            for b, bb in ((bd, bias), (None, None)) if not special else ((bd, bias),):
                                for act in (ACTS if not special else (ACTS[0], ACTS[3])):
                                    kw = dict(stride=stride, padding=padding, depth_multiplier=m, activation=act)
                                    check(xd, wd, b, kw, R.finish(t, bb, act))
                                    n += 1
    return n


# geometries per special kind: SAME always, VALID where the image holds the filter ((1,1) holds 1x1 only; (5,7) and (8,8) all)
GEOMETRIES = 2 * (3 * 4 + 1 + 2 * 4)


@pytest.mark.parametrize("channels", GRID_CHANNELS)
def test_the_grid(channels):
    assert sweep(channels, 1) == GEOMETRIES * (4 * 2 * 4 + 2 * 1 * 2)


@pytest.mark.parametrize("channels,multiplier", [(3, 2), (3, 3), (32, 2), (32, 3)])
def test_the_grid_with_a_depth_multiplier(channels, multiplier):
    assert sweep(channels, multiplier) == GEOMETRIES * (4 * 2 * 4 + 2 * 1 * 2)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name):
    x, w, bias, kw, want = known_case(name)
    for outs in (dict(out_bits=True), dict(out=False, out_bits=True)):
        got, bits = run(x, w, bias, **outs, **kw)
        assert got is None or (got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))), (name, got)
        assert np.array_equal(bits, O.bitpack(want))
    if name == "minus_zero":
        assert want.view(np.uint32).tolist() == [[[[0x80000000]]]] and bits.reshape(-1).tolist() == [0]


# one reference for the two tests below: 257 x 257 output pixels of 32 channels are 528392 16-byte chunks -- the capped grid
# covers 2048 blocks x 4 waves x 64 = 524288 per pass -- and the last wave has 8 of its 64 lanes in use; on the row path they
# are 66049 wave tasks against 8192 waves
BIG = {}


def big():
    if not BIG:
        shape = (1, 258, 258, 32)
        assert 257 * 257 * 8 > 2048 * 4 * 64 and (257 * 257 * 8) % 64 == 8
        x = float_fixture(shape, 5)
        w, bias = grid_operands((2, 2), 32)
        BIG.update(x=x, w=w, bias=bias, want=R.depthwise(x, w, bias, (1, 1), R.VALID, 1, R.RELU))
        BIG["want"].setflags(write=False)
    return BIG


def test_more_chunks_than_one_pass_of_the_grid_and_a_ragged_last_wave():
    c = big()
    for outs in (dict(out_bits=True), dict()):               # with bits, and the tensor alone
        got, bits = run(c["x"], c["w"], c["bias"], stride=1, padding=amd.PADDING_VALID, activation=amd.ACT_RELU, **outs)
        assert agree(got, c["want"]) and (bits is None or np.array_equal(bits, O.bitpack(c["want"])))


def shifted(a):
    t = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def test_four_byte_offsets_take_the_row_path_and_agree_with_the_aligned_run():
    c = big()
    kw = dict(stride=1, padding=amd.PADDING_VALID, activation=amd.ACT_RELU, out_bits=True)
    aligned = run(c["x"], c["w"], c["bias"], **kw)
    got = run(shifted(c["x"]), dev(c["w"]), dev(c["bias"]), **kw)
    assert agree(got[0], c["want"]) and agree(got[0], aligned[0]) and np.array_equal(got[1], aligned[1])
    # each operand alone, and the output, on a smaller tensor with special values
    shape = (3, 7, 7, 64)
    x = float_fixture(shape, 8, special=True)
    w, bias = grid_operands((3, 3), 64, special=True)
    want = R.depthwise(x, w, bias, (2, 2), R.SAME)
    out = torch.zeros(want.size + 1, dtype=torch.float32, device=DEV)[1:].view(want.shape)
    for xd, wd, bd, o in ((shifted(x), dev(w), dev(bias), True), (dev(x), shifted(w), dev(bias), True),
                          (dev(x), dev(w), shifted(bias), True), (dev(x), dev(w), dev(bias), out), (dev(x), dev(w), dev(bias), True)):
        got, bits = run(xd, wd, bd, stride=2, out=o, out_bits=True)
        assert agree(got, want) and np.array_equal(bits, O.bitpack(want))


def test_refusals_on_the_device():
    flat = torch.zeros(2 * 2 * 8 * 8 * 64, dtype=torch.float32, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:-64].view(2, 8, 8, 64)   # begins inside the input
    w = torch.zeros(1, 3, 3, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.depthwise_conv2d(x, w, out=out)
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.depthwise_conv2d(x, w, out=False, out_bits=w.view(torch.int32).view(-1)[:256].view(2, 8, 8, 2))


def test_an_input_of_more_than_two_to_the_32_bytes():
    """4100 x 4100 pixels of 64 channels are 4.3 GB; 3x3 / 2 SAME pads nothing in front and one row and column behind.  The first
    output rows, and the last ones -- which read across the byte offset 2^32 of the input (its row 4092) and to its end -- against
    the reference on slices: the offsets are 64-bit.  Run once."""
    side, c = 4100, 64
    assert side * side * c * 4 > 2 ** 32 and 2 ** 32 // (side * c * 4) == 4092
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((1, side, side, c), dtype=torch.float32, device=DEV, generator=g)
    w, bias = grid_operands((3, 3), c)
    out, bits = amd.depthwise_conv2d(x, dev(w), dev(bias), stride=2, padding=amd.PADDING_SAME, activation=amd.ACT_RELU_N1_TO_1, out_bits=True)
    torch.cuda.synchronize()
    assert out.shape == (1, side // 2, side // 2, c) and bits.shape == (1, side // 2, side // 2, 2)
    # an even number of leading input rows under SAME is padded like the whole image, except that its last output row misses
    # the row behind it: that row is dropped
    head = R.depthwise(x[:, :8].cpu().numpy(), w, bias, (2, 2), R.SAME, 1, R.RELU_N1_TO_1)[:, :3]
    assert agree(out[:, :3].cpu().numpy(), head) and np.array_equal(bits[:, :3].cpu().numpy(), O.bitpack(head))
    # the trailing input rows from an even row on are padded exactly like the whole image
    first = side // 2 - 8                                    # output rows 2042 .. 2049 read input rows 4084 .. 4099
    tail = R.depthwise(x[:, 2 * first:].cpu().numpy(), w, bias, (2, 2), R.SAME, 1, R.RELU_N1_TO_1)
    assert tail.shape[1] == 8 and 2 * first < 4092 < side
    assert agree(out[:, first:].cpu().numpy(), tail) and np.array_equal(bits[:, first:].cpu().numpy(), O.bitpack(tail))


# ---- sections -----------------------------------------------------------------------------------------------------------------
def run_cut(data, info, x):
    """The file under the DEFAULT partition, section by section on the GPU, every builtin operator in NumPy (info["host"]).
    Returns tensor index -> array for every tensor that crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0])
    model = it.model
    section_of = {op: k for k, sec in enumerate(it.sections) for op in sec.ops}
    live, ran = {model.inputs[0]: x}, set()
    for i, op in enumerate(model.operators):
        if i in section_of:
            k = section_of[i]
            if k not in ran:
                ran.add(k)
                live.update(zip(it.sections[k].outputs, it.run_section(k, [live[t] for t in it.sections[k].inputs])))
        else:
            live[op.outputs[0]] = info["host"][i](*[live[t] for t in op.inputs if t >= 0 and not model.tensors[t].constant])
    assert len(ran) == len(it.sections) == 2
    return live


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                                        b.view(np.int32) if b.dtype == np.float32 else b)


# (depthwise, conv1x1, pool) of one run of each fixture as ONE section.  quicknet: the blur's result goes on to the 1x1
# convolution in float, and that one takes the LceQuantize behind it.  fold: the blur feeds only the LceQuantize, which is folded
# into it.
STATS = dict(quicknet=((1, 0), (1, 1), (1, 0)), fold=((1, 1), (0, 0), (0, 0)))


def stats(model):
    return model.depthwise_stats(), model.conv1x1_stats(), model.pool_stats()


@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_each_fixture_runs_as_one_section(name, batch):
    data, xt, out, info = FIXTURES[name]()
    x = np.random.default_rng(batch).standard_normal((batch, info["size"], info["size"], info["channels"])).astype(np.float32)
    cut = run_cut(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, **ALL_FLAGS)
    assert len(it.sections) == 1 and it.lce_only
    assert it.model.operators[info["depthwise"]].builtin_code == DEPTHWISE_CONV_2D
    (got,) = it.run_section(0, [x])
    print(name, batch, stats(it.model), it.model.elementwise_stats(), it.model.run_stats()[1])
    assert same(got, cut[out])
    d = cut[info["tensors"]["d"]]                            # the blurred tensor crossed the host in the cut run
    assert d.shape == (batch, info["size"] // 2, info["size"] // 2, info["channels"])
    if name == "fold":
        assert (d < 0).any() and (d > 0).any()               # both bit values occur
    assert stats(it.model) == STATS[name]
    assert it.model.concat_stats() == (0, 0) and it.model.int8_add_stats() == (0, 0)
    if batch == 3:
        assert same(it.predict(x), cut[out])
        # without the new flag the same bytes come out of two sections and the host's blur
        two = mr.Interpreter(data, batch_size=batch, **OLD_FLAGS)
        assert len(two.sections) == 2 and two.model.depthwise_stats() == (0, 0)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_hip_graph_replay_gives_the_same_bytes(name):
    data, xt, out, info = FIXTURES[name]()
    model = mr.LceModel(data, **ALL_FLAGS)
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
            runs.append((y.clone(), stats(model), model.graph_stats()))
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1] for r in runs] == [STATS[name]] * 3
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))
    assert same(runs[2][0].cpu().numpy(), run_cut(data, info, xh)[out])
    model.use_hip_graphs(False)
