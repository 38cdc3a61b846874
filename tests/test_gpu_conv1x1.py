"""lce_hip_conv1x1_f32 and the conv1x1 sections on the MI355X, exact and without tolerance: the kernel against the NumPy
reference (tests/conv1x1_ref.py: the fmaf chain over the input channels in order) over the grid of images, batches, channel
counts, strides, bias, activations and output combinations, the bits against the oracle's LceQuantize of the reference, the known
answers worked by hand, one convolution whose input exceeds 2^32 bytes, and the fixtures of
tests/test_conv1x1_sections_host.py run as ONE section against the same file run section by section with the host doing the
pools, MUL / ADD and the convolution, and against the oracle's operators.  NaN positions are compared as positions."""
import importlib

import numpy as np
import pytest

import conv1x1_ref as R
import oracle_lib as O
import pool_ref as PR
from section_models import CONV_2D, float_fixture
from test_conv1x1_sections_host import (ACTS, ALL_FLAGS, FIXTURES, GRID_BATCHES, GRID_CIN, GRID_COUT, GRID_IMAGES, GRID_STRIDES,
                                        KNOWN, grid_operands, known_case)

torch = pytest.importorskip("torch")
from test_gpu_elementwise import ref_op  # noqa: E402  (TFLite's float MUL / ADD, one rounding each)

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def agree(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(x, w, bias=None, **kw):
    out, bits = amd.conv1x1(dev(x) if isinstance(x, np.ndarray) else x, dev(w) if isinstance(w, np.ndarray) else w,
                            dev(bias) if isinstance(bias, np.ndarray) else bias, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def check(xd, wd, bd, stride, act, want):
    """The three output combinations of one convolution against the reference `want` and the oracle's bits of it."""
    want_bits = O.bitpack(want)
    kw = dict(stride=stride, activation=act)
    got, none = run(xd, wd, bd, **kw)
    assert none is None and agree(got, want)
    both = run(xd, wd, bd, out_bits=True, **kw)
    assert agree(both[0], want) and np.array_equal(both[1], want_bits)
    only = run(xd, wd, bd, out=False, out_bits=True, **kw)
    assert only[0] is None and np.array_equal(only[1], want_bits)


# ---- the kernel grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", GRID_CIN)
def test_the_grid(cin):
    """The chain of the widest filter is computed once per tensor: output channel o depends on w[o] alone, and a stride only
    selects pixels."""
    n = 0
    cmax = max(GRID_COUT)
    for special in (False, True):
        w, bias = grid_operands(cin, cmax, special)
        for image in GRID_IMAGES:
            for batch in GRID_BATCHES:
                x = float_fixture((batch, *image, cin), image[0] * 1000 + batch * 100 + cin, special)
                chain = R.chain(x.reshape(-1, cin), w).reshape(batch, *image, cmax)
                xd = dev(x)
                for cout in GRID_COUT:
                    wd, bd = dev(w[:cout]), dev(bias[:cout])
                    for stride in (GRID_STRIDES if not special else GRID_STRIDES[::2]):
                        t = np.ascontiguousarray(chain[:, ::stride[0], ::stride[1], :cout])
                        for b in (bd, None):
                            with np.errstate(invalid="ignore", over="ignore"):
                                tb = t if b is None else (t + bias[None, None, None, :cout]).astype(np.float32)
                            for act in (ACTS if not special else (ACTS[0], ACTS[3])):
                                check(xd, wd, b, stride, act, R.clamp(tb, act))
                                n += 1
    assert n == 3 * 2 * 7 * 2 * (3 * 4 + 2 * 2)


@pytest.mark.parametrize("name", [k[0] for k in KNOWN])
def test_the_known_answers(name):
    x, w, bias, want, bit = known_case(name)
    for kw in (dict(out_bits=True), dict(out=False, out_bits=True)):
        got, bits = run(x, w, bias, **kw)
        assert got is None or (got.shape == (1, 1, 1, 1) and int(got.view(np.uint32)[0, 0, 0, 0]) == want), (name, got)
        assert bits.reshape(-1).tolist() == [bit]
    if name.startswith("minus_zero") and bias is None:
        assert want == 0x80000000 and bit == 0 and x.shape[3] in (1, 3, 33)


def test_more_tiles_than_one_pass_of_the_grid_and_a_ragged_last_tile():
    """515 x 513 pixels = 2064 tiles of 128 and 3 pixels more (the capped grid covers 2048 tiles per pass); two channel slices, the
    second one ragged."""
    shape = (1, 515, 513, 4)
    assert shape[1] * shape[2] > 2048 * 128 and (shape[1] * shape[2]) % 128 == 3
    x = float_fixture(shape, 5)
    w, bias = grid_operands(4, 161)
    want = R.conv1x1(x, w, bias, 1, R.RELU)
    got, bits = run(x, w, bias, activation=amd.ACT_RELU, out_bits=True)
    assert agree(got, want) and np.array_equal(bits, O.bitpack(want))
    want = R.conv1x1(x, w, None, (2, 1), R.NONE)
    got, bits = run(x, w, None, stride=(2, 1), out_bits=True)
    assert agree(got, want) and np.array_equal(bits, O.bitpack(want))


def test_four_byte_offsets_take_the_unaligned_path():
    shape, cout = (3, 7, 7, 64), 96
    x = float_fixture(shape, 8, special=True)
    w, bias = grid_operands(64, cout, special=True)
    want = R.conv1x1(x, w, bias, 2)

    def shifted(a):
        t = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)[1:].view(a.shape)
        t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    out = torch.zeros(want.size + 1, dtype=torch.float32, device=DEV)[1:].view(want.shape)
    for xd, wd, o in ((shifted(x), dev(w), None), (dev(x), shifted(w), None), (shifted(x), shifted(w), out), (dev(x), dev(w), out)):
        got, bits = run(xd, wd, shifted(bias), stride=2, out=o, out_bits=True)
        assert agree(got, want) and np.array_equal(bits, O.bitpack(want))


def test_refusals_on_the_device():
    flat = torch.zeros(2 * 8 * 8 * 64 + 2 * 8 * 8 * 32, dtype=torch.float32, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:-64].view(2, 8, 8, 32)   # begins inside the input
    w = torch.zeros(32, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.conv1x1(x, w, out=out)
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.conv1x1(x, w, out=False, out_bits=w.view(torch.int32).view(-1)[:128].view(2, 8, 8, 1))


def test_an_input_of_more_than_two_to_the_32_bytes():
    """2^22 pixels x 288 channels -> 32: the input is 4.8 GB.  The first rows, the last rows and the rows around the byte offset
    2^32 against the reference: the offsets are 64-bit.  Run once."""
    side, cin, cout = 2048, 288, 32
    rows = side * side
    assert rows * cin * 4 > 2 ** 32
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((1, side, side, cin), dtype=torch.float32, device=DEV, generator=g)
    w, bias = grid_operands(cin, cout)
    out, bits = amd.conv1x1(x, dev(w), dev(bias), activation=amd.ACT_RELU_N1_TO_1, out_bits=True)
    torch.cuda.synchronize()
    assert out.shape == (1, side, side, cout) and bits.shape == (1, side, side, 1)
    mid = 2 ** 32 // (cin * 4)
    flat_x, flat_o, flat_b = x.view(rows, cin), out.view(rows, cout), bits.view(rows, 1)
    for lo, hi in ((0, 1024), (mid - 768, mid + 768), (rows - 1024, rows)):
        want = R.conv1x1(flat_x[lo:hi].cpu().numpy().reshape(1, 1, hi - lo, cin), w, bias, 1, R.RELU_N1_TO_1).reshape(hi - lo, cout)
        assert agree(flat_o[lo:hi].cpu().numpy(), want), (lo, hi)
        assert np.array_equal(flat_b[lo:hi].cpu().numpy(), O.bitpack(want)), (lo, hi)


# ---- sections -----------------------------------------------------------------------------------------------------------------
def conv(cv, bits, batch):
    return O.bconv2d(cv["spec"].with_batch(batch), O.DST_F32, bits, cv["w"], cv["m"], cv["b"])


def bn(info, v, act):
    return ref_op(ref_op(v, "mul", info["bn_m"], amd.ACT_NONE), "add", info["bn_a"], act)


def reference(name, info, x):
    """The fixture composed from the oracle's LceQuantize / LceBconv2d, the one-rounding MUL / ADD, the pool reference and the
    convolution reference.  Returns tensor index -> array for the tensors a cut run hands over, and the graph output."""
    batch, t = x.shape[0], info["tensors"]
    if name == "bireal":
        r = conv(info["convs"][0], O.bitpack(x), batch)
        aa = bn(info, conv(info["convs"][1], O.bitpack(r), batch), amd.ACT_NONE)
        p = PR.pool2d(r, PR.AVERAGE, (2, 2), (2, 2), PR.VALID)
        s = R.conv1x1(p, info["w"], info["wb"])
        rr = ref_op(aa, "add", s, amd.ACT_NONE)
        return {t["r"]: r, t["aa"]: aa, t["p"]: p, t["s"]: s, t["rr"]: rr}, conv(info["convs"][2], O.bitpack(rr), batch)
    aa = bn(info, conv(info["convs"][0], O.bitpack(x), batch), amd.ACT_RELU)
    p = PR.pool2d(aa, PR.MAX, (2, 2), (2, 2), PR.VALID)
    tt = R.conv1x1(p, info["w"], None)
    return {t["p"]: p, t["t"]: tt}, conv(info["convs"][1], O.bitpack(tt), batch)


def host_ops(model, info):
    """What the host does for the fixture's builtin operators under the default partition: operator index -> function."""
    ops = {}
    for k in info["pools"]:
        o = model.operators[k]
        ops[k] = lambda v, o=o: PR.pool2d(v, PR.MAX if o.builtin_code == 17 else PR.AVERAGE, (o.filter_height, o.filter_width),
                                          (o.stride_h, o.stride_w), o.padding, o.activation)
    o = model.operators[info["conv1x1"]]
    assert o.builtin_code == CONV_2D and (o.dilation_w, o.dilation_h) == (1, 1)
    ops[info["conv1x1"]] = lambda v, o=o: R.conv1x1(v, info["w"], info["wb"], (o.stride_h, o.stride_w), o.activation)
    ops[info["mul"]] = lambda v: ref_op(v, "mul", info["bn_m"], amd.ACT_NONE)
    ops[info["add"]] = lambda v: ref_op(v, "add", info["bn_a"], model.operators[info["add"]].activation)
    if "join" in info:
        ops[info["join"]] = lambda a, b: ref_op(a, "add", b, amd.ACT_NONE)
    return ops


def run_cut(data, info, x):
    """The file under the DEFAULT partition, section by section on the GPU, every builtin operator in NumPy.  Returns tensor
    index -> array for every tensor that crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0])
    model = it.model
    host = host_ops(model, info)
    section_of = {op: k for k, sec in enumerate(it.sections) for op in sec.ops}
    live, ran = {model.inputs[0]: x}, set()
    for i, op in enumerate(model.operators):
        if i in section_of:
            k = section_of[i]
            if k not in ran:
                ran.add(k)
                live.update(zip(it.sections[k].outputs, it.run_section(k, [live[t] for t in it.sections[k].inputs])))
        else:
            live[op.outputs[0]] = host[i](*[live[t] for t in op.inputs if t >= 0 and not model.tensors[t].constant])
    assert len(ran) == len(it.sections) > 1
    return live


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                                        b.view(np.int32) if b.dtype == np.float32 else b)


# (conv1x1, pool, elementwise, LceQuantize folded into LceBconv2d) of one run of each fixture as ONE section.  bireal: the
# convolution's result goes on to the ADD in float; MUL -> ADD is one chain, the joining ADD a second one that takes the
# LceQuantize behind it; the first LceBconv2d writes the bits of the main branch's LceQuantize itself.  dense: the convolution
# feeds only the LceQuantize, which is folded into it.
STATS = dict(bireal=((1, 0), (1, 0), (2, 3, 1), 1), dense=((1, 1), (1, 0), (1, 2, 0), 0))


def stats(model):
    return model.conv1x1_stats(), model.pool_stats(), model.elementwise_stats(), model.run_stats()[1]


@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_each_fixture_runs_as_one_section(name, batch):
    x = np.random.default_rng(batch).standard_normal((batch, 8, 8, 64)).astype(np.float32)
    data, xt, out, info = FIXTURES[name]()
    cut = run_cut(data, info, x)
    handed, want = reference(name, info, x)
    it = mr.Interpreter(data, batch_size=batch, **ALL_FLAGS)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    print(name, batch, stats(it.model))
    assert same(got, want) and same(got, cut[out])
    for t, v in handed.items():                              # what the cut run handed over
        if t in cut:
            assert same(cut[t], v), t
    assert info["tensors"]["p"] in cut and info["tensors"]["s" if name == "bireal" else "t"] in cut
    assert stats(it.model) == STATS[name]
    assert it.model.concat_stats() == (0, 0) and it.model.int8_add_stats() == (0, 0)
    if batch == 3:
        assert same(it.predict(x), want)
        # without the conv1x1 flag the same bytes come out of two sections and the host's convolution
        two = mr.Interpreter(data, batch_size=batch, elementwise_sections=True, pool_sections=True)
        assert len(two.sections) == 2 and two.model.conv1x1_stats() == (0, 0)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_hip_graph_replay_gives_the_same_bytes(name):
    data, xt, out, info = FIXTURES[name]()
    model = mr.LceModel(data, **ALL_FLAGS)
    batch = 5
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((batch, 8, 8, 64)).astype(np.float32)).to(DEV)
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
    assert same(runs[2][0].cpu().numpy(), reference(name, info, x.cpu().numpy())[1])
    model.use_hip_graphs(False)
