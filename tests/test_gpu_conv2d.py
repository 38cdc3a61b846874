"""lce_hip_conv2d_f32 and the conv2d / stem sections on the MI355X, exact and without tolerance: the kernels against the NumPy
reference (tests/conv2d_ref.py: the fmaf chain over the in-bounds taps in raster order and the channels of a tap in order) over
the grid of K = fh fw Cin, images, batches, filters, strides, paddings and output channels, with and without bias, the four
activations, the three output combinations and special values; the bits against the oracle's LceQuantize of the reference; the
known answers worked by hand; 1x1 filters against amd.conv1x1; more tiles than one pass of the capped grid on both pixel
enumerations; 4-byte-offset views; one convolution whose input exceeds 2^32 bytes; and the fixtures of
tests/test_conv2d_sections_host.py run as ONE section against the same file under the parent's flags with NumPy doing the stem,
and against the oracle's operators.  NaN positions are compared as positions, every other byte as a byte."""
import importlib

import numpy as np
import pytest

import conv2d_ref as R
import oracle_lib as O
from section_models import ADD, MUL, NONE, float_fixture, float_op
from test_conv2d_sections_host import (ACTS, ALL_FLAGS, FIXTURES, KNOWN, PARENT_FLAGS, grid_operands, known_case,
                                       quicknet_stem_model, _graph)

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (filter, Cin): K = 1 (below one 8-step group), 27 and 15 (no multiple of 8), 24 and 36 (16-byte loads; 36 ends its second chunk
# inside a tap), 147 and 297 (several chunks, a chunk boundary inside a tap)
GRID_K = (((1, 1), 1), ((3, 3), 3), ((2, 3), 4), ((3, 3), 4), ((7, 7), 3), ((3, 3), 33), ((1, 5), 3))
GRID_IMAGES = ((1, 1), (5, 7), (9, 8))
GRID_BATCHES = (1, 3)
GRID_STRIDES = ((1, 1), (2, 2), (2, 1), (4, 3))
GRID_PADDINGS = (R.SAME, R.VALID)
GRID_COUT = (1, 33, 160)


def agree(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(x, w, bias=None, **kw):
    out, bits = amd.conv2d(dev(x) if isinstance(x, np.ndarray) else x, dev(w) if isinstance(w, np.ndarray) else w,
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


def geometries(filt):
    for image in GRID_IMAGES:
        for batch in GRID_BATCHES:
            for stride in GRID_STRIDES:
                for padding in GRID_PADDINGS:
                    if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
                        continue                             # an empty output
                    yield image, batch, stride, padding


@pytest.mark.parametrize("filt,cin", GRID_K)
def test_the_grid(filt, cin):
    """Every image, batch, stride and padding at one (filter, Cin): the chain is computed once at the widest Cout and sliced;
    bias and activation rotate over the checks, so that every pairing occurs at every Cout."""
    w, bias = grid_operands(filt, cin, max(GRID_COUT))
    n = 0
    for image, batch, stride, padding in geometries(filt):
        x = float_fixture((batch, *image, cin), image[0] * 1000 + batch * 100 + cin)
        xd = dev(x)
        t = R.chain(x, w, stride, padding)
        for cout in GRID_COUT:
            act, with_bias = ACTS[n % 4], (n // 4) % 2 == 0
            b = bias[:cout] if with_bias else None
            check(xd, dev(w[:cout]), dev(b), dict(stride=stride, padding=padding, activation=act), R.finish(t[..., :cout], b, act))
            n += 1
    # SAME always, VALID where the image holds the filter
    valid = sum(i[0] >= filt[0] and i[1] >= filt[1] for i in GRID_IMAGES)
    assert n == (3 + valid) * 2 * 4 * 3


@pytest.mark.parametrize("special", [False, True])
def test_bias_activations_and_outputs(special):
    """With and without bias, the four activations, the three output combinations -- on 35-pixel images (one 128-pixel tile spans
    the three images' interiors; the rest of their pixels are border) and on an image smaller than the 7x7 filter (every pixel
    clipped) --, plain and with +-0, subnormals, +-inf, NaN and huge values in input and filter."""
    seen = set()
    for filt, cin, image, stride in (((3, 3), 3, (5, 7), (1, 1)), ((7, 7), 3, (5, 7), (2, 1)), ((2, 3), 4, (9, 8), (2, 2)), ((7, 7), 3, (1, 1), (1, 1))):
        w, bias = grid_operands(filt, cin, 33, special)
        x = float_fixture((3, *image, cin), 77 + cin, special)
        xd, wd, bd = dev(x), dev(w), dev(bias)
        t = R.chain(x, w, stride, R.SAME)
        seen |= {"nan"} if np.isnan(t).any() else set()
        seen |= {"inf"} if np.isinf(t).any() else set()
        seen |= {"subnormal"} if ((t != 0) & (np.abs(t) < np.float32(1.1754944e-38))).any() else set()
        for b, bb in ((bd, bias), (None, None)):
            for act in ACTS:
                check(xd, wd, b, dict(stride=stride, padding=R.SAME, activation=act), R.finish(t, bb, act))
    assert seen == ({"nan", "inf", "subnormal"} if special else set()), seen


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name):
    x, w, bias, kw, want = known_case(name)
    for outs in (dict(out_bits=True), dict(out=False, out_bits=True), dict()):
        got, bits = run(x, w, bias, **outs, **kw)
        assert got is None or (got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))), (name, got)
        assert bits is None or np.array_equal(bits, O.bitpack(want))


def test_a_1x1_filter_gives_the_bytes_of_conv1x1():
    for cin, cout, stride in ((33, 40, 2), (64, 160, 1), (3, 1, (2, 1))):
        x = float_fixture((3, 5, 7, cin), 9, special=True)
        w, bias = grid_operands((1, 1), cin, cout, special=True)
        for padding in GRID_PADDINGS:
            a = run(x, w, bias, stride=stride, padding=padding, activation=amd.ACT_RELU_N1_TO_1, out_bits=True)
            o, bits = amd.conv1x1(dev(x), dev(w), dev(bias), stride=stride, activation=amd.ACT_RELU_N1_TO_1, out_bits=True)
            assert agree(a[0], o.cpu().numpy()) and np.array_equal(a[1], bits.cpu().numpy())


# one reference per enumeration for the tests below.  interior: 517 x 513 under 3x3 SAME has 515 x 511 = 263165 interior pixels:
# 2056 tiles of 128 against the grid's cap of 2048, the last tile with 125 of its 128 rows.  border: a 1 x 201 filter on 100 x 100
# clips every window: 10000 wave tasks against 8192 waves
BIG = {}


def big(kind):
    if kind not in BIG:
        if kind == "interior":
            shape, filt = (1, 517, 513, 1), (3, 3)
            assert 515 * 511 > 2048 * 128 and (515 * 511) % 128 == 125
        else:
            shape, filt = (1, 100, 100, 1), (1, 201)
            assert 100 * 100 > 2048 * 4
        x = float_fixture(shape, 5)
        w, bias = grid_operands(filt, 1, 33)
        want = R.conv2d(x, w, bias, (1, 1), R.SAME, R.RELU)
        want.setflags(write=False)
        BIG[kind] = dict(x=x, w=w, bias=bias, want=want)
    return BIG[kind]


@pytest.mark.parametrize("kind", ["interior", "border"])
def test_more_tiles_than_one_pass_of_the_grid_and_a_ragged_last_tile(kind):
    c = big(kind)
    for outs in (dict(out_bits=True), dict()):               # with bits, and the tensor alone
        got, bits = run(c["x"], c["w"], c["bias"], stride=1, padding=amd.PADDING_SAME, activation=amd.ACT_RELU, **outs)
        assert agree(got, c["want"]) and (bits is None or np.array_equal(bits, O.bitpack(c["want"])))


def shifted(a):
    t = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def test_four_byte_offsets_take_the_dword_path_and_agree_with_the_aligned_run():
    """Cin = 4 takes 16-byte loads when input and filter allow it: each operand alone, and the output, at a 4-byte offset."""
    x = float_fixture((3, 7, 7, 4), 8, special=True)
    w, bias = grid_operands((3, 3), 4, 33, special=True)
    want = R.conv2d(x, w, bias, (2, 2), R.SAME)
    aligned = run(x, w, bias, stride=2, out_bits=True)
    assert agree(aligned[0], want)
    out = torch.zeros(want.size + 1, dtype=torch.float32, device=DEV)[1:].view(want.shape)
    for xd, wd, bd, o in ((shifted(x), dev(w), dev(bias), True), (dev(x), shifted(w), dev(bias), True), (dev(x), dev(w), shifted(bias), True),
                          (dev(x), dev(w), dev(bias), out), (shifted(x), shifted(w), shifted(bias), out)):
        got, bits = run(xd, wd, bd, stride=2, out=o, out_bits=True)
        assert agree(got, want) and np.array_equal(bits, O.bitpack(want)) and np.array_equal(bits, aligned[1])


def test_refusals_on_the_device():
    flat = torch.zeros(2 * 2 * 8 * 8 * 64, dtype=torch.float32, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:-64].view(2, 8, 8, 64)   # begins inside the input
    w = torch.zeros(64, 3, 3, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.conv2d(x, w, out=out)
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.conv2d(x, w, out=False, out_bits=w.view(torch.int32).view(-1)[:256].view(2, 8, 8, 2))
    bias = torch.zeros(64, dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the bias"):
        amd.conv2d(x[:1, :1, :1], w, bias, out=bias.view(1, 1, 1, 64))


def test_an_input_of_more_than_two_to_the_32_bytes():
    """40000 x 40000 pixels of one channel are 6.4 GB.  3x3 at stride 5714 SAME gives 8 x 8 outputs (7 x 5714 + 3 - 40000 = 1:
    nothing in front, one row and column of padding behind): 7 x 7 interior windows, of which row 6 starts at byte 5.5e9, and 15
    clipped ones at the far edges.  The reference runs on the 23 touched rows and columns, which at stride 3 have the same
    geometry.  Run once."""
    side, s = 40000, 5714
    assert side * side * 4 > 2 ** 32 and 6 * s * side * 4 > 2 ** 32 and 7 * s + 2 == side
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((1, side, side, 1), dtype=torch.float32, device=DEV, generator=g)
    w, bias = grid_operands((3, 3), 1, 5)
    out, bits = amd.conv2d(x, dev(w), dev(bias), stride=s, padding=amd.PADDING_SAME, activation=amd.ACT_RELU_N1_TO_1, out_bits=True)
    torch.cuda.synchronize()
    assert out.shape == (1, 8, 8, 5) and bits.shape == (1, 8, 8, 1)
    touched = torch.tensor([o * s + d for o in range(8) for d in range(3) if o * s + d < side], device=DEV)
    assert touched.numel() == 23
    small = x[:, touched][:, :, touched].cpu().numpy()
    want = R.conv2d(small, w, bias, (3, 3), R.SAME, R.RELU_N1_TO_1)
    assert want.shape == (1, 8, 8, 5) and agree(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), O.bitpack(want))


# ---- sections -----------------------------------------------------------------------------------------------------------------
def run_cut(data, info, x):
    """The file under the PARENT's flags, section by section on the GPU, every operator outside them in NumPy (info["host"]).
    Returns tensor index -> array for every tensor that crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0], **PARENT_FLAGS)
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
    assert [s.ops for s in it.sections] == info["parent_sections"] and len(ran) == len(it.sections)
    return live


def oracle_run(name, info, x):
    """The whole fixture on the CPU: the NumPy references for the float operators, the oracle's LceQuantize and LceBconv2d."""
    conv = lambda cv, v: O.bconv2d(cv["spec"].with_batch(x.shape[0]), O.DST_F32, O.bitpack(v), cv["w"], cv["m"], cv["b"])
    h = info["host"]
    if name == "float3x3":
        (k,) = info["conv2d"]
        return O.bitpack(h[k](conv(info["convs"][0], x)))
    v = x
    for k in info["stem"]:
        v = h[k](v)
    y = conv(info["convs"][0], v)
    if name == "bireal":
        bd = info["body"]
        y = float_op(float_op(float_op(y, MUL, bd["m"], NONE), ADD, bd["a"], NONE), ADD, v, NONE)
    return y


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                                        b.view(np.int32) if b.dtype == np.float32 else b)


def stats(model):
    return dict(conv2d=model.conv2d_stats(), conv1x1=model.conv1x1_stats(), depthwise=model.depthwise_stats(), pool=model.pool_stats())


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_each_fixture_runs_as_one_section(name, batch):
    data, xt, out, info = FIXTURES[name]()
    x = np.random.default_rng(batch).standard_normal((batch,) + info["shape"]).astype(np.float32)
    cut = run_cut(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, **ALL_FLAGS)
    assert len(it.sections) == 1 and it.lce_only and it.sections[0].inputs == [xt]
    (got,) = it.run_section(0, [x])
    print(name, batch, stats(it.model), it.model.elementwise_stats(), it.model.run_stats()[1])
    assert same(got, cut[out]) and same(got, oracle_run(name, info, x))
    assert stats(it.model) == info["stats"]
    assert it.model.concat_stats() == (0, 0) and it.model.int8_add_stats() == (0, 0)
    if batch == 3:
        assert same(it.predict(x), cut[out])


def test_predict_runs_the_quicknet_stem_and_the_pool_stem():
    for first in ("conv", "pool"):
        data, xt, out, info = quicknet_stem_model(first=first)
        x = np.random.default_rng(4).standard_normal((2,) + info["shape"]).astype(np.float32)
        flags = ALL_FLAGS if first == "conv" else dict(stem_sections=True, **PARENT_FLAGS)
        it = mr.Interpreter(data, batch_size=2, **flags)
        (sectioned,) = it.run_section(0, [x])
        assert same(it.predict(x), sectioned) and same(sectioned, oracle_run("quicknet", info, x)) and stats(it.model) == info["stats"]
        with pytest.raises(NotImplementedError):
            mr.Interpreter(data, batch_size=2, **PARENT_FLAGS).predict(x)


def test_a_1x1_filter_runs_on_either_entry_with_the_same_bytes():
    data, k = _graph("filter_1x1")
    x = np.random.default_rng(6).standard_normal((3, 8, 8, 64)).astype(np.float32)
    outs = []
    for kw, want in ((dict(conv1x1_sections=True, conv2d_sections=True), ((0, 0), (1, 1))), (dict(conv2d_sections=True), ((1, 1), (0, 0))),
                     (dict(conv1x1_sections=True), ((0, 0), (1, 1)))):
        it = mr.Interpreter(data, batch_size=3, **kw)
        outs.append(it.run_section(0, [x])[0])
        assert (it.model.conv2d_stats(), it.model.conv1x1_stats()) == want, kw
    assert same(outs[0], outs[1]) and same(outs[0], outs[2])


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_hip_graph_replay_gives_the_same_bytes(name):
    data, xt, out, info = FIXTURES[name]()
    model = mr.LceModel(data, **ALL_FLAGS)
    batch = 5
    xh = np.random.default_rng(11).standard_normal((batch,) + info["shape"]).astype(np.float32)
    x = torch.from_numpy(xh).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    dt = torch.int32 if name == "float3x3" else torch.float32
    y = torch.zeros(dims, dtype=dt, device=DEV)
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
    assert [r[1] for r in runs] == [info["stats"]] * 3
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))
    assert same(runs[2][0].cpu().numpy(), oracle_run(name, info, xh))
    model.use_hip_graphs(False)
