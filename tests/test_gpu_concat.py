"""lce_hip_concat and the concat sections on the MI355X, bit for bit and without tolerance: the kernel against np.concatenate
(float compared as int32 views: the join is a copy), its bits against the oracle's LceQuantize, one join of more than 2^32
bytes compared on the device against its own inputs, and the dense fixtures of tests/test_concat_sections_host.py run as ONE
section against the same file run section by section with the host doing the joins, and against the oracle's operators."""
import importlib

import numpy as np
import pytest

import oracle_lib as O
from section_models import DENSE_STAGES, dense_block_model, joins_of
from test_concat_sections_host import INT8_GROWTHS, INT8_Q, dense_reference, int8_dense_model, int8_dense_reference

torch = pytest.importorskip("torch")
from test_gpu_elementwise import ref_op  # noqa: E402  (TFLite's float MUL / ADD, one rounding each)

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ALIGNED = [(64, 64), (128, 64), (256, 64, 64), (32,) * 8]
RAGGED = [(1, 31), (33, 64, 7), (63, 1), (5, 3)]
INT8_ONLY = [(16, 16), (48, 17)]
ROWS = [1, 37, 3136, 256 * 28 * 28]
SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x00000001,
                    0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7FABCDEF, 0xFFABCDEF], np.uint32).view(np.int32)


def patterns(rows, c, seed):
    """Random 32-bit patterns: every float class occurs, and +-0, +-inf, quiet / signalling NaNs with payloads and the
    smallest / largest subnormals of both signs are planted."""
    g = np.random.default_rng(seed)
    a = g.integers(-2 ** 31, 2 ** 31, (rows, c), dtype=np.int64).astype(np.int32)
    flat = a.reshape(-1)
    k = max(1, flat.size // 7)
    flat[g.integers(0, flat.size, k)] = SPECIAL[g.integers(0, SPECIAL.size, k)]
    return a


def make(kind, rows, channels, seed):
    if kind == "f32":
        return [patterns(rows, c, seed + 31 * k).view(np.float32) for k, c in enumerate(channels)]
    if kind == "i32":
        return [patterns(rows, c, seed + 31 * k) for k, c in enumerate(channels)]
    g = np.random.default_rng(seed)
    return [g.integers(-128, 128, (rows, c), dtype=np.int64).astype(np.int8) for c in channels]


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def run(tensors, **kw):
    out, bits = amd.concat(tensors, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def check(xs, zero_points=(0,)):
    """The joined bytes, the bits at every zero point, and the three output combinations."""
    want = np.concatenate(xs, axis=-1)
    assert same(raw(want), np.concatenate([raw(x) for x in xs], axis=-1))       # (NumPy's own join is a copy too)
    dev = [torch.from_numpy(x).to(DEV) for x in xs]
    got, none = run(dev)
    assert none is None and same(got, want)
    if xs[0].dtype == np.int32:
        return
    for zp in zero_points:
        want_bits = O.bitpack(want, zp)
        both = run(dev, out_bits=True, zero_point=zp)
        assert same(both[0], want) and np.array_equal(both[1], want_bits), zp
        only = run(dev, out=False, out_bits=True, zero_point=zp)
        assert only[0] is None and np.array_equal(only[1], want_bits), zp


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("channels", ALIGNED + RAGGED, ids=lambda c: "x".join(map(str, c)))
def test_float_join_is_np_concatenate_bit_for_bit(channels, rows):
    check(make("f32", rows, channels, rows + len(channels)))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("channels", ALIGNED + RAGGED + INT8_ONLY, ids=lambda c: "x".join(map(str, c)))
def test_int8_join_and_its_bits_at_four_zero_points(channels, rows):
    check(make("i8", rows, channels, rows + len(channels)), zero_points=(-128, 0, 5, 127))


@pytest.mark.parametrize("rows", ROWS[:3])
@pytest.mark.parametrize("channels", [(2, 2), (4, 8, 4), (1, 3), (5, 2, 1), (8,) * 8], ids=lambda c: "x".join(map(str, c)))
def test_bitpacked_join(channels, rows):
    check(make("i32", rows, channels, rows))
    with pytest.raises(ValueError, match="no bit output"):
        amd.concat([torch.zeros((2, 4), dtype=torch.int32, device=DEV)] * 2, out_bits=True)


@pytest.mark.parametrize("kind,c", [("f32", 64), ("f32", 7), ("i8", 64), ("i8", 5)])
def test_the_same_tensor_twice(kind, c):
    (x,) = make(kind, 333, (c,), 4)
    (y,) = make(kind, 333, (2 * c,), 5)
    check([x, x], zero_points=(3,) if kind == "i8" else (0,))
    check([x, y, x], zero_points=(3,) if kind == "i8" else (0,))


def test_a_four_byte_offset_slice_takes_the_unaligned_path():
    rows, c = 100, 64
    x0, x1 = make("f32", rows, (c, c), 8)
    base = torch.zeros(rows * c + 1, dtype=torch.float32, device=DEV)
    shifted = base[1:].view(rows, c)
    shifted.copy_(torch.from_numpy(x0))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    want = np.concatenate([x0, x1], axis=-1)
    got, bits = run([shifted, torch.from_numpy(x1).to(DEV)], out_bits=True)
    assert same(got, want) and np.array_equal(bits, O.bitpack(want))
    out = torch.zeros(rows * 2 * c + 1, dtype=torch.float32, device=DEV)[1:].view(rows, 2 * c)   # an unaligned output
    got, bits = run([torch.from_numpy(x0).to(DEV), torch.from_numpy(x1).to(DEV)], out=out, out_bits=True)
    assert same(got, want) and np.array_equal(bits, O.bitpack(want))
    (b0,) = make("i8", rows, (c,), 9)
    b = torch.zeros(rows * c + 4, dtype=torch.int8, device=DEV)[4:].view(rows, c)
    b.copy_(torch.from_numpy(b0))
    got, bits = run([b, b], out_bits=True, zero_point=-7)
    want = np.concatenate([b0, b0], axis=-1)
    assert same(got, want) and np.array_equal(bits, O.bitpack(want, -7))


def test_refusals_and_empty_on_the_device():
    x = torch.zeros((8, 64), dtype=torch.float32, device=DEV)
    flat = torch.zeros(8 * 64 + 8 * 192, dtype=torch.float32, device=DEV)
    x1, out = flat[:8 * 128].view(8, 128), flat[8 * 64:].view(8, 192)                # the output begins inside input 1
    with pytest.raises(amd.LceHipError, match="overlaps input 1"):
        amd.concat([x, x1], out=out)
    e = torch.zeros((0, 64), dtype=torch.float32, device=DEV)
    o, b = amd.concat([e, e], out_bits=True)
    assert o.shape == (0, 128) and b.shape == (0, 4)


def test_more_than_two_to_the_32_elements():
    """One int8 join whose output has more than 2^32 elements (4.3 GB read, 4.3 GB written), compared on the device against
    its own inputs.

    Run once; nothing of that size goes to the host."""
    rows, c = 2 ** 25 + 1000, 64
    assert rows * 2 * c > 2 ** 32
    g = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randint(-128, 128, (rows, c), dtype=torch.int8, device=DEV, generator=g) for _ in range(2)]
    out = torch.zeros((rows, 2 * c), dtype=torch.int8, device=DEV)
    amd.concat(xs, out=out)
    torch.cuda.synchronize()
    for k, x in enumerate(xs):
        assert torch.equal(out[:, k * c:(k + 1) * c], x), k
    # the bits of the last rows (beyond 2^32 bytes into the output), against the oracle
    _, bits = amd.concat(xs, out=False, out_bits=True, zero_point=5)
    tail = np.concatenate([x[-64:].cpu().numpy() for x in xs], axis=-1)
    assert np.array_equal(bits[-64:].cpu().numpy(), O.bitpack(tail, 5))
    head = np.concatenate([x[:64].cpu().numpy() for x in xs], axis=-1)
    assert np.array_equal(bits[:64].cpu().numpy(), O.bitpack(head, 5))


# ---- sections -----------------------------------------------------------------------------------------------------------------
def host_ops(steps):
    """What the host does for the fixture's builtin operators: operator index -> function of its non-constant inputs."""
    ops = {}
    for s in steps:
        if s["kind"] != "dense":
            continue
        ops[s["join"]] = lambda *xs: np.concatenate(xs, axis=-1)
        if "mul" in s:
            ops[s["mul"]] = lambda v, m=s["bn_m"]: ref_op(v, "mul", m, amd.ACT_NONE)
            ops[s["add"]] = lambda v, a=s["bn_a"]: ref_op(v, "add", a.reshape(1, 1, 1, -1), amd.ACT_NONE)
    return ops


def run_cut(data, steps, x, **flags):
    """The file at the partition `flags` give, section by section on the GPU, every operator outside the sections in NumPy.
    Returns tensor index -> array for every tensor that crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0], **flags)
    model, host = it.model, host_ops(steps)
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


def prefixes(stages):
    """The fixture cut after 1, 2, ... dense layers (the full one last)."""
    flat = [(s, k) for s, g in enumerate(stages) for k in range(len(g))]
    for n in range(1, len(flat) + 1):
        s, k = flat[n - 1]
        yield tuple(stages[:s]) + (tuple(stages[s][:k + 1]),)


@pytest.mark.parametrize("batch", [1, 3, 64])
def test_the_dense_block_runs_as_one_section(batch):
    x = np.random.default_rng(batch).standard_normal((batch, 16, 16, 64)).astype(np.float32)
    data, xt, out, steps = dense_block_model()
    cut = run_cut(data, steps, x, elementwise_sections=True)
    composed = dense_reference(steps, x)
    dense = [(k, s) for k, s in enumerate(steps) if s["kind"] == "dense"]
    assert len(list(prefixes(DENSE_STAGES))) == len(dense)
    # every tensor the cut run hands over is a joined tensor or a slice of one: each prefix of the block, run as ONE section,
    # must deliver its last joined tensor byte for byte
    for n, stages in enumerate(prefixes(DENSE_STAGES), 1):
        data_n, _, out_n, steps_n = dense_block_model(stages=stages)
        it = mr.Interpreter(data_n, batch_size=batch, elementwise_sections=True, concat_sections=True)
        assert len(it.sections) == 1 and it.lce_only
        (got,) = it.run_section(0, [x])
        joins = joins_of(steps_n)
        assert len(joins) == n
        at_step, s = dense[n - 1]
        assert same(got, cut[s["out"]]), n
        assert same(got, composed[at_step]), n
        at = got.shape[-1]
        for cv in reversed(s["convs"]):                              # the convolution outputs the cut run delivered
            g = cv["spec"].channels_out
            assert same(np.ascontiguousarray(got[..., at - g:at]), cut[cv["y"]]), n
            at -= g
        # one launch per join; only a join that an LceQuantize reads directly (the one in front of the stride-2 layer) folds it
        folded = sum(1 for k, t in enumerate(steps_n) if t["kind"] == "dense" and k + 1 < len(steps_n) and steps_n[k + 1]["kind"] == "conv")
        assert it.model.concat_stats() == (n, folded), n
        assert it.model.elementwise_stats()[0] == n
    assert folded == 1
    if batch == 3:
        assert same(it.predict(x), composed[-1])


@pytest.mark.parametrize("batch", [3, 64])
def test_the_int8_dense_block_runs_as_one_section(batch):
    x = np.random.default_rng(batch).integers(-128, 128, (batch, 16, 16, 64), dtype=np.int64).astype(np.int8)
    data, xt, out, steps = int8_dense_model()
    cut = run_cut(data, steps, x, int8_add_sections=True)
    composed = int8_dense_reference(steps, x)
    assert same(cut[out], composed[-1])
    for n in range(1, len(INT8_GROWTHS) + 1):
        data_n, _, out_n, steps_n = int8_dense_model(growths=INT8_GROWTHS[:n])
        it = mr.Interpreter(data_n, batch_size=batch, int8_add_sections=True, concat_sections=True)
        assert len(it.sections) == 1 and it.lce_only
        (got,) = it.run_section(0, [x])
        # every join is read by an LceQuantize; the last one by nothing else
        assert it.model.concat_stats() == (n, n), n
        assert it.model.int8_add_stats() == (0, 0) and it.model.elementwise_stats() == (0, 0, 0)
        if n == len(INT8_GROWTHS):
            assert same(got, cut[out]) and same(got, composed[-1])
            assert same(it.predict(x), composed[-1])
        else:                                                         # (a shorter block ends in another last convolution)
            assert same(got, int8_dense_reference(steps_n, x)[-1]), n
            assert same(run_cut(data_n, steps_n, x)[out_n], got), n


def test_hip_graph_replay_gives_the_same_bytes():
    data, xt, out, steps = dense_block_model()
    model = mr.LceModel(data, elementwise_sections=True, concat_sections=True)
    batch, n = 5, len(joins_of(steps))
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((batch, 16, 16, 64)).astype(np.float32)).to(DEV)
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
            runs.append((y.clone(), model.concat_stats(), model.graph_stats()))
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1] for r in runs] == [(n, 1)] * 3
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))
    want = dense_reference(steps, x.cpu().numpy())[-1]
    assert same(runs[2][0].cpu().numpy(), want)
    model.use_hip_graphs(False)
