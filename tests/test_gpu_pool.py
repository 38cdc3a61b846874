"""lce_hip_pool2d and the pool sections on the MI355X, exact and without tolerance: the kernels against the NumPy reference
(tests/pool_ref.py) over the grid of windows, images, channel counts, activations, zero points and output combinations, the bits
against the oracle's LceQuantize of the reference, the known answers worked by hand, one pool of more than 2^32 bytes compared
on the device, and the fixtures of tests/test_pool_sections_host.py run as ONE section against the same file run section by
section with the host doing the pools, and against the oracle's operators.  NaN positions are compared as positions, and for
MAX +0.0 and -0.0 compare equal (which of the two a window of both gives is unspecified)."""
import importlib

import numpy as np
import pytest

import oracle_lib as O
import pool_ref as R
from section_models import alexnet_body_model
from test_pool_sections_host import (ACTS, BATCHES, F32_CHANNELS, GRID_IMAGES, GRID_WINDOWS, I8_CHANNELS, INT8_KNOWN, INT8_Q,
                                     POOL_Q, WINDOW_OF, fixture_seed, float_fixture, int8_body_model, int8_fixture,
                                     int8_known_case, window_of)

torch = pytest.importorskip("torch")
from test_gpu_elementwise import ref_op  # noqa: E402  (TFLite's float MUL / ADD, one rounding each)

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZERO_POINTS = (-128, -3, 0, 127)


def agree(got, want, op):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    if op == R.MAX:
        return bool(np.all((got == want) | nan))
    return np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def run(x, *args, **kw):
    out, bits = amd.pool2d(torch.from_numpy(x).to(DEV) if isinstance(x, np.ndarray) else x, *args, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def check(xd, want, op, filt, stride, padding, act, zero_point=0, **q):
    """The three output combinations of one pool against the reference `want` and the oracle's bits of it."""
    want_bits = O.bitpack(want, zero_point)
    args = (op, filt, stride, padding, act)
    got, none = run(xd, *args, zero_point=zero_point, **q)
    assert none is None and agree(got, want, op)
    both = run(xd, *args, out_bits=True, zero_point=zero_point, **q)
    assert agree(both[0], want, op) and np.array_equal(both[1], want_bits)
    only = run(xd, *args, out=False, out_bits=True, zero_point=zero_point, **q)
    assert only[0] is None and np.array_equal(only[1], want_bits)


# ---- the kernel grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", GRID_WINDOWS, ids=str)
def test_float_pools_over_the_grid(w):
    n = 0
    for image in GRID_IMAGES:
        filt, stride, padding = window_of(w, image)
        for batch in BATCHES:
            for c in sum(F32_CHANNELS.values(), ()):
                seed = fixture_seed(image, batch, c)
                kinds = [(R.MAX, "max"), (R.AVERAGE, "average")] + ([(R.AVERAGE, "average_inf")] if c in (33, 64) else [])
                for op, kind in kinds:
                    x = float_fixture((batch, *image, c), seed, kind)
                    xd = torch.from_numpy(x).to(DEV)
                    for act in ACTS:
                        check(xd, R.pool2d(x, op, filt, stride, padding, act), op, filt, stride, padding, act)
                        n += 1
    assert n == 3 * 2 * 9 * 2 * 4 + 3 * 2 * 2 * 4


@pytest.mark.parametrize("w", GRID_WINDOWS, ids=str)
def test_int8_pools_over_the_grid(w):
    for image in GRID_IMAGES:
        filt, stride, padding = window_of(w, image)
        for batch in BATCHES:
            for c in sum(I8_CHANNELS.values(), ()):
                x = int8_fixture((batch, *image, c), fixture_seed(image, batch, c))
                xd = torch.from_numpy(x).to(DEV)
                for op in (R.MAX, R.AVERAGE):
                    for act in ACTS:
                        for zp in ZERO_POINTS:
                            want = R.pool2d(x, op, filt, stride, padding, act, INT8_Q[0], zp)
                            check(xd, want, op, filt, stride, padding, act, zero_point=zp, scale=INT8_Q[0])


def test_the_known_answers():
    x = np.array([2.0 ** 24, 1.0, 1.0], np.float32).reshape(1, 1, 3, 1)
    got, _ = run(x, amd.POOL_AVERAGE, (2, 3), 1, amd.PADDING_SAME)
    assert got.reshape(-1).tolist() == [8388608.0, 5592405.5, 1.0]
    x = np.array([np.nan, -np.inf, -np.inf, np.nan], np.float32).reshape(1, 2, 2, 1)
    got, bits = run(x, amd.POOL_MAX, 2, 2, amd.PADDING_VALID, out_bits=True)
    assert got.reshape(-1).tolist() == [float(-R.FLT_MAX)] and bits.reshape(-1).tolist() == [1]
    for n in sorted(WINDOW_OF):
        x, filt, want = int8_known_case(n)
        got, _ = run(x, amd.POOL_AVERAGE, filt, 1, amd.PADDING_VALID, scale=1.0, zero_point=0)
        assert np.array_equal(got, want), n
    assert len(INT8_KNOWN) == 18
    # subnormals are neither flushed on the way in nor on the way out: the average of two equal subnormals is that subnormal
    tiny = np.full((1, 1, 2, 4), 1e-45, np.float32)
    got, _ = run(tiny, amd.POOL_AVERAGE, (1, 2), 1, amd.PADDING_VALID)
    assert np.array_equal(got.view(np.int32).reshape(-1), np.ones(4, np.int32))
    # the largest filter the entry accepts, as a global pool of 65536 taps (sums up to 128 x 2^16)
    g = np.random.default_rng(3)
    big = g.integers(-128, 128, (1, 256, 256, 16)).astype(np.int8)
    big[..., 0], big[..., 1] = -128, 127
    a, n = big.astype(np.int64).sum(axis=(1, 2)), 65536
    num = np.where(a > 0, a + n // 2, a - n // 2)
    want = {R.MAX: big.max(axis=(1, 2)), R.AVERAGE: (np.sign(num) * (np.abs(num) // n)).astype(np.int8)}
    assert want[R.AVERAGE][0, :2].tolist() == [-128, 127]
    for op in (R.MAX, R.AVERAGE):
        got, _ = run(big, op, 256, 1, amd.PADDING_VALID, scale=1.0, zero_point=0)
        assert np.array_equal(got.reshape(1, 16), want[op])


@pytest.mark.parametrize("c", [96, 33])
@pytest.mark.parametrize("kind", ["f32", "i8"])
def test_more_chunks_than_one_pass_of_the_capped_grid(kind, c):
    """64 x 27 x 27 output pixels: 1.1 M 16-byte chunks of 96 floats (the capped grid covers 0.5 M per pass), 46 656 wave tasks
    on the row path (8192 per pass): the grid-stride advance runs on both."""
    shape = (64, 27, 27, c)
    x = float_fixture(shape, 5, "average") if kind == "f32" else int8_fixture(shape, 5)
    xd = torch.from_numpy(x).to(DEV)
    q = {} if kind == "f32" else dict(scale=INT8_Q[0], zero_point=INT8_Q[1])
    for op in (R.MAX, R.AVERAGE):
        want = R.pool2d(x, op, (3, 3), (1, 1), R.SAME, R.RELU, *(() if kind == "f32" else INT8_Q))
        got, bits = run(xd, op, 3, 1, amd.PADDING_SAME, amd.ACT_RELU, out_bits=True, **q)
        assert agree(got, want, op) and np.array_equal(bits, O.bitpack(want, q.get("zero_point", 0)))


def test_a_four_byte_offset_slice_takes_the_unaligned_path():
    shape = (3, 7, 7, 64)
    x = float_fixture(shape, 8, "max")
    base = torch.zeros(x.size + 1, dtype=torch.float32, device=DEV)
    shifted = base[1:].view(shape)
    shifted.copy_(torch.from_numpy(x))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for op in (R.MAX, R.AVERAGE):
        xx = x if op == R.MAX else float_fixture(shape, 8, "average")
        shifted.copy_(torch.from_numpy(xx))
        want = R.pool2d(xx, op, (3, 3), (2, 2), R.SAME)
        got, bits = run(shifted, op, 3, 2, amd.PADDING_SAME, out_bits=True)
        assert agree(got, want, op) and np.array_equal(bits, O.bitpack(want))
        out = torch.zeros(want.size + 1, dtype=torch.float32, device=DEV)[1:].view(want.shape)      # an unaligned output
        got, bits = run(torch.from_numpy(xx).to(DEV), op, 3, 2, amd.PADDING_SAME, out=out, out_bits=True)
        assert agree(got, want, op) and np.array_equal(bits, O.bitpack(want))
    xi = int8_fixture(shape, 9)
    b = torch.zeros(xi.size + 4, dtype=torch.int8, device=DEV)[4:].view(shape)
    b.copy_(torch.from_numpy(xi))
    want = R.pool2d(xi, R.AVERAGE, (2, 2), (2, 2), R.SAME, R.NONE, *INT8_Q)
    got, bits = run(b, amd.POOL_AVERAGE, 2, 2, amd.PADDING_SAME, out_bits=True, scale=INT8_Q[0], zero_point=INT8_Q[1])
    assert np.array_equal(got, want) and np.array_equal(bits, O.bitpack(want, INT8_Q[1]))


def test_refusals_on_the_device():
    flat = torch.zeros(2 * 8 * 8 * 64 + 2 * 4 * 4 * 64, dtype=torch.float32, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:-64].view(2, 4, 4, 64)   # begins inside the input
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.pool2d(x, amd.POOL_MAX, 2, 2, amd.PADDING_VALID, out=out)


def test_more_than_two_to_the_32_bytes():
    """One int8 MAX pool 2x2 / 2 of a 5.4 GB tensor, compared on the device with the maximum of its four strided views: the
    offsets are 64-bit.  Run once; nothing of that size goes to the host."""
    shape = (5, 32768, 2048, 16)
    assert np.prod(shape) > 2 ** 32
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(-128, 128, shape, dtype=torch.int8, device=DEV, generator=g)
    out, _ = amd.pool2d(x, amd.POOL_MAX, 2, 2, amd.PADDING_VALID, scale=1.0, zero_point=0)
    torch.cuda.synchronize()
    want = torch.maximum(torch.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2]), torch.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2]))
    assert out.shape == want.shape and torch.equal(out, want)


# ---- sections -----------------------------------------------------------------------------------------------------------------
def conv(cv, bits, batch, dst=O.DST_F32, **q):
    return O.bconv2d(cv["spec"].with_batch(batch), dst, bits, cv["w"], cv["m"], cv["b"], **q)


def float_reference(info, x):
    """The float fixture composed from the oracle's LceQuantize / LceBconv2d, the one-rounding batch norm and the pool
    reference.  Returns the tensors in order: y0, p0, aa, y1, p1, y2."""
    batch = x.shape[0]
    y0 = conv(info["convs"][0], O.bitpack(x), batch)
    p0 = R.pool2d(y0, R.MAX, (3, 3), (2, 2), R.VALID)
    aa = ref_op(ref_op(p0, "mul", info["bn_m"], amd.ACT_NONE), "add", info["bn_a"], amd.ACT_NONE)
    y1 = conv(info["convs"][1], O.bitpack(aa), batch)
    p1 = R.pool2d(y1, R.AVERAGE, (2, 2), (2, 2), R.SAME, R.RELU6)
    return y0, p0, aa, y1, p1, conv(info["convs"][2], O.bitpack(p1), batch)


def int8_reference(info, x):
    batch = x.shape[0]
    q = dict(out_scale=POOL_Q[0], out_zero_point=POOL_Q[1])
    y0 = conv(info["convs"][0], O.bitpack(x, 4), batch, O.DST_I8, **q)
    p0 = R.pool2d(y0, R.MAX, (3, 3), (2, 2), R.VALID, R.NONE, *POOL_Q)
    y1 = conv(info["convs"][1], O.bitpack(p0, POOL_Q[1]), batch, O.DST_I8, **q)
    return y0, p0, y1, R.pool2d(y1, R.AVERAGE, (2, 2), (2, 2), R.SAME, R.RELU, *POOL_Q)


def host_ops(model, info):
    """What the host does for the fixture's builtin operators under the default partition: operator index -> function."""
    ops = {}
    for k in info["pools"]:
        o = model.operators[k]
        t = model.tensors[o.inputs[0]]
        q = () if t.scale is None else (t.scale, t.zero_point)
        ops[k] = lambda v, o=o, q=q: R.pool2d(v, R.MAX if o.builtin_code == 17 else R.AVERAGE, (o.filter_height, o.filter_width),
                                              (o.stride_h, o.stride_w), o.padding, o.activation, *q)
    if "mul" in info:
        ops[info["mul"]] = lambda v: ref_op(v, "mul", info["bn_m"], amd.ACT_NONE)
        ops[info["add"]] = lambda v: ref_op(v, "add", info["bn_a"], amd.ACT_NONE)
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
            live[op.outputs[0]] = host[i](*[live[t] for t in op.inputs if not model.tensors[t].constant])
    assert len(ran) == len(it.sections) > 1
    return live


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                                        b.view(np.int32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("batch", [1, 3, 64])
def test_the_alexnet_body_runs_as_one_section(batch):
    x = np.random.default_rng(batch).standard_normal((batch, 15, 15, 64)).astype(np.float32)
    data, xt, out, info = alexnet_body_model()
    cut = run_cut(data, info, x)
    y0, p0, aa, y1, p1, y2 = float_reference(info, x)
    assert np.any(p1 == 6.0) and np.any(p1 == 0.0)                     # (the second pool's RELU6 clamps at both ends)
    it = mr.Interpreter(data, batch_size=batch, elementwise_sections=True, pool_sections=True)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert same(got, y2) and same(got, cut[out])
    # what the cut run handed over: the convolution outputs and the pooled tensors
    for t, want in zip((info["convs"][0]["y"], info["pooled"][0], info["convs"][1]["y"], info["pooled"][1]), (y0, p0, y1, p1)):
        assert same(cut[t], want)
    # two pools; the second one's LceQuantize is folded into it, the first one's into the batch-norm chain behind it
    assert it.model.pool_stats() == (2, 1)
    assert it.model.elementwise_stats() == (1, 2, 1)
    assert it.model.run_stats()[1] == 0 and it.model.concat_stats() == (0, 0) and it.model.int8_add_stats() == (0, 0)
    if batch == 3:
        assert same(it.predict(x), y2)
        only = mr.Interpreter(data, batch_size=batch, pool_sections=True)     # the pool flag alone: cut at the MUL / ADD
        assert len(only.sections) == 2
        first = dict(zip(only.sections[0].outputs, only.run_section(0, [x])))
        assert same(first[info["pooled"][0]], p0) and only.model.pool_stats() == (1, 0)
        (last,) = only.run_section(1, [aa])
        assert same(last, y2) and only.model.pool_stats() == (1, 1)


@pytest.mark.parametrize("batch", [1, 3, 64])
def test_the_int8_body_runs_as_one_section(batch):
    x = np.random.default_rng(batch).integers(-128, 128, (batch, 15, 15, 64), dtype=np.int64).astype(np.int8)
    data, xt, out, info = int8_body_model()
    cut = run_cut(data, info, x)
    y0, p0, y1, p1 = int8_reference(info, x)
    it = mr.Interpreter(data, batch_size=batch, pool_sections=True)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert same(got, p1) and same(cut[out], p1)
    for t, want in zip((info["convs"][0]["y"], info["pooled"][0], info["convs"][1]["y"]), (y0, p0, y1)):
        assert same(cut[t], want)
    # the first pool feeds only an LceQuantize (bits alone are written), the second is delivered
    assert it.model.pool_stats() == (2, 1)
    assert it.model.elementwise_stats() == (0, 0, 0) and it.model.run_stats()[1] == 0
    if batch == 3:
        assert same(it.predict(x), p1)


def test_hip_graph_replay_gives_the_same_bytes():
    data, xt, out, info = alexnet_body_model()
    model = mr.LceModel(data, elementwise_sections=True, pool_sections=True)
    batch = 5
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((batch, 15, 15, 64)).astype(np.float32)).to(DEV)
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
            runs.append((y.clone(), model.pool_stats(), model.elementwise_stats(), model.graph_stats()))
    assert [r[3] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1] for r in runs] == [(2, 1)] * 3 and [r[2] for r in runs] == [(1, 2, 1)] * 3
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))
    assert same(runs[2][0].cpu().numpy(), float_reference(info, x.cpu().numpy())[-1])
    model.use_hip_graphs(False)
