"""lce_hip_depthwise_conv2d_i8 on the MI355X, byte for byte and without tolerance against the NumPy restatement
(tests/depthwise_i8_ref.py): the known answers worked by hand; the grid over filters, images, strides, paddings, channels and depth
multipliers with rotating bias, activation, output combination, input zero point, scale kind and placement, each case through the
path the entry picks (asserted) and, where that is the 16-byte path, through the row path as well (tests/depthwise_i8_cases.py); an
asymmetric case in which a transposed index cannot hide; the three output combinations with marker bytes around them; the
refusals that need device pointers; one launch captured in a HIP graph and replayed on the caller's stream; an input of just over
2^32 bytes; and the fixtures of tests/depthwise_i8_models.py run as ONE section through Interpreter against the same file cut
under every earlier name with NumPy doing the operators between, and against the oracle."""
import importlib

import numpy as np
import pytest

import depthwise_i8_models as DM
import depthwise_i8_ref as R
from depthwise_i8_cases import BITS_MARK, GRID, KNOWN, OUT_MARK, operands, run_grid

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def placed(a, offset, fill=None):
    """`a` (or, with `fill`, a tensor of a's shape filled with it) on the device, its first byte `offset` bytes behind a 16-byte
    boundary, with 64 marker bytes on each side.  Returns (the view, the whole buffer)."""
    a = np.ascontiguousarray(a)
    raw = torch.full((a.nbytes + 144,), int(OUT_MARK), dtype=torch.int8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    t = raw[64 + offset:64 + offset + a.nbytes].view(a.shape)
    if fill is None:
        t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == offset and t.is_contiguous()
    return t, raw


def run(x, w, bias, sw, q_in, q_out, stride, padding, m, act, want_out=True, want_bits=True, offset=0, path=None):
    """amd.depthwise_conv2d_i8 with the table amd.depthwise_conv2d_i8_prepare makes, into marked buffers: (out, bits, took the
    16-byte path) as NumPy arrays; an output that was not asked for comes back as its marks, and the 64 bytes around the int8
    output must still be marks."""
    w = np.asarray(w).reshape((1,) + np.asarray(w).shape[-3:])
    table, _, _ = amd.depthwise_conv2d_i8_prepare(w, bias, sw, q_in, q_out, m, act)
    assert np.array_equal(table, R.table(w, bias, sw, q_in[0], q_out[0]))
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    oh, ow = R.out_and_pad(x.shape[1], w.shape[1], st[0], padding)[0], R.out_and_pad(x.shape[2], w.shape[2], st[1], padding)[0]
    cout = w.shape[3]
    xd, wd = placed(x, offset)[0], placed(w, offset)[0]
    out, raw = placed(np.empty((x.shape[0], oh, ow, cout), np.int8), offset, fill=OUT_MARK)
    bits = torch.full((x.shape[0], oh, ow, (cout + 31) // 32), BITS_MARK, dtype=torch.int32, device=DEV)
    _, _, took = amd.depthwise_conv2d_i8(xd, wd, dev(table), q_in, q_out, stride=st, padding=padding, depth_multiplier=m, activation=act,
                                         out=out if want_out else False, out_bits=bits if want_bits else False, path=path, report_path=True)
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    assert (raw[:64 + offset] == OUT_MARK).all() and (raw[64 + offset + out.numel():] == OUT_MARK).all()
    return out.cpu().numpy(), bits.cpu().numpy(), bool(took)


# ---- the entry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name):
    k = KNOWN[name]
    for path in (None, 0):
        out, bits, _ = run(k["x"], k["w"], k["bias"], k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], k["m"], k["act"], path=path)
        assert np.array_equal(out, k["want"]) and np.array_equal(bits, R.bitpack(k["want"], k["q_out"][1])), (path, out, k["want"])


def test_the_known_corner_on_sixteen_byte_chunks():
    """The hand-worked corner pixel (4 taps inside, 5 skipped) repeated over 32 channels, so that the 16-byte path runs it too."""
    k = KNOWN["corner_same_pad"]
    x, w, want = (np.repeat(k[n], 32, axis=3) for n in ("x", "w", "want"))
    for path in (None, 1, 0):
        out, bits, vec = run(x, w, None, k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], 1, k["act"], path=path)
        assert vec == (path != 0)
        assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, k["q_out"][1]))


@pytest.mark.parametrize("filt,cin,m", GRID)
def test_the_grid(filt, cin, m):
    n, vecs = run_grid(run, filt, cin, m)
    assert n >= 9 and (vecs > 0) == (m == 1 and cin % 16 == 0)


@pytest.mark.parametrize("cin,m", [(32, 1), (7, 3)])
def test_an_asymmetric_case_in_which_a_transposed_index_cannot_hide(cin, m):
    """H != W, stride_h != stride_w, a filter that is neither square nor symmetric, three images, more chunks than one wave."""
    x, w, bias, sw, q_in, q_out = operands((3, 11, 6, cin), (2, 5), m, 77, zi=-9, stride=(3, 2), padding=R.SAME)
    want = R.depthwise_i8(x, w, bias, sw, q_in, q_out, (3, 2), R.SAME, m)
    assert want.shape == (3, 4, 3, cin * m) and np.unique(want).size > 100
    assert not np.array_equal(R.depthwise_i8(x, w[:, ::-1], bias, sw, q_in, q_out, (3, 2), R.SAME, m), want)        # (the filter is not symmetric)
    assert not np.array_equal(R.depthwise_i8(x, w[:, :, ::-1], bias, sw, q_in, q_out, (3, 2), R.SAME, m), want)
    for path in (None, 0):
        out, bits, vec = run(x, w, bias, sw, q_in, q_out, (3, 2), R.SAME, m, R.NONE, path=path)
        assert vec == (path is None and m == 1)
        assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, q_out[1]))


@pytest.mark.parametrize("cin,m,offset", [(64, 1, 0), (64, 1, 1), (33, 1, 0), (32, 2, 0)])
def test_out_only_bits_only_and_both_write_nothing_else(cin, m, offset):
    x, w, bias, sw, q_in, q_out = operands((2, 9, 8, cin), (3, 3), m, 13, zi=5, act=R.RELU6, stride=(2, 2))
    want = R.depthwise_i8(x, w, bias, sw, q_in, q_out, (2, 2), R.SAME, m, R.RELU6)
    for want_out, want_bits in ((True, False), (False, True), (True, True)):
        out, bits, vec = run(x, w, bias, sw, q_in, q_out, 2, R.SAME, m, R.RELU6, want_out=want_out, want_bits=want_bits, offset=offset)
        assert vec == (m == 1 and cin % 16 == 0 and offset == 0)
        assert np.array_equal(out, want) if want_out else (out == OUT_MARK).all()
        assert np.array_equal(bits, R.bitpack(want, q_out[1])) if want_bits else (bits == BITS_MARK).all()


def test_more_work_than_one_pass_of_the_grid():
    """2048 blocks of 4 waves are one pass: 2 x 150 x 150 output pixels of 16 chunks are 11250 wave tasks of the 16-byte path for its
    8192 waves, and 180000 segments of the row path."""
    x, w, bias, sw, q_in, q_out = operands((2, 300, 299, 256), (3, 3), 1, 5, zi=11, act=R.RELU, stride=(2, 2))
    want = R.depthwise_i8(x, w, bias, sw, q_in, q_out, (2, 2), R.SAME, 1, R.RELU)
    assert want.shape == (2, 150, 150, 256) and want.size // 16 // 64 > 2048 * 4
    for path in (None, 0):
        out, bits, vec = run(x, w, bias, sw, q_in, q_out, 2, R.SAME, 1, R.RELU, path=path)
        assert vec == (path is None) and np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, q_out[1]))


def test_an_input_of_just_over_two_to_the_32_bytes():
    """11587 x 11587 pixels of 32 int8 channels are 4 296 274 208 bytes, 1 306 912 more than 2^32.  3x3 at stride 1655 SAME gives 8 x 8
    outputs (7 x 1655 + 3 - 11587 = 1: nothing in front, one row and column of padding behind); the windows of output row 7 start
    at byte 4.295e9 > 2^32.  The input is filled on the device; the reference runs on the 23 touched rows and columns, which at
    stride 3 have the same geometry, and the last output rows are what is compared on the host.  Both paths, run once each."""
    side, s, c = 11587, 1655, 32
    assert side * side * c > 2 ** 32 and 7 * s * side * c > 2 ** 32 and 7 * s + 2 == side
    assert (7 * (s - 1) + 2) ** 2 * c < 2 ** 32                     # (the next smaller image of this geometry does not cross 2^32)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(-128, 128, (1, side, side, c), dtype=torch.int8, device=DEV, generator=g)
    _, w, bias, sw, q_in, q_out = operands((1, 23, 23, c), (3, 3), 1, 3, zi=-77, stride=(3, 3))
    table, _, _ = amd.depthwise_conv2d_i8_prepare(w, bias, sw, q_in, q_out, 1, amd.ACT_NONE)
    touched = torch.tensor([o * s + d for o in range(8) for d in range(3) if o * s + d < side], device=DEV)
    assert touched.numel() == 23
    small = x[:, touched][:, :, touched].cpu().numpy()
    want = R.depthwise_i8(small, w, bias, sw, q_in, q_out, (3, 3), R.SAME)
    assert want.shape == (1, 8, 8, c) and np.unique(want[:, 6:]).size > 50
    for path in (None, 0):
        out, bits, took = amd.depthwise_conv2d_i8(x, dev(w), dev(table), q_in, q_out, stride=s, padding=amd.PADDING_SAME, out_bits=True,
                                                  path=path, report_path=True)
        torch.cuda.synchronize()
        assert took == (1 if path is None else 0) and out.shape == (1, 8, 8, c) and bits.shape == (1, 8, 8, 1)
        assert np.array_equal(out.cpu().numpy()[:, 6:], want[:, 6:]) and np.array_equal(bits.cpu().numpy()[:, 6:], R.bitpack(want, q_out[1])[:, 6:])


def test_a_capture_and_replay_of_the_launch():
    """The launch allocates and copies nothing: captured once into a HIP graph on the caller's stream, replayed on new contents
    of the same buffers, against the eager bytes."""
    for cin, m in ((64, 1), (20, 2)):
        x, w, bias, sw, q_in, q_out = operands((2, 9, 8, cin), (3, 3), m, 21, zi=4, stride=(2, 2))
        table = dev(amd.depthwise_conv2d_i8_prepare(w, bias, sw, q_in, q_out, m, amd.ACT_NONE)[0])
        xd, wd = dev(x), dev(w)
        shape = (2, 5, 4, cin * m)
        out = torch.zeros(shape, dtype=torch.int8, device=DEV)
        bits = torch.zeros(shape[:3] + ((shape[3] + 31) // 32,), dtype=torch.int32, device=DEV)
        kw = dict(stride=2, depth_multiplier=m, out=out, out_bits=bits)
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            amd.depthwise_conv2d_i8(xd, wd, table, q_in, q_out, stream=s.cuda_stream, **kw)          # eager first
            s.synchronize()
            with torch.cuda.graph(graph, stream=s):
                amd.depthwise_conv2d_i8(xd, wd, table, q_in, q_out, stream=s.cuda_stream, **kw)
        for seed in (1, 2):
            x2 = np.random.default_rng(seed).integers(-128, 128, x.shape, dtype=np.int64).astype(np.int8)
            xd.copy_(torch.from_numpy(x2))
            eager = amd.depthwise_conv2d_i8(xd, wd, table, q_in, q_out, stride=2, depth_multiplier=m, out_bits=True)
            out.zero_(), bits.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want = R.depthwise_i8(x2, w, bias, sw, q_in, q_out, (2, 2), R.SAME, m)
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), R.bitpack(want, q_out[1]))
            assert torch.equal(out, eager[0]) and torch.equal(bits, eager[1])


def test_refusals_on_the_device():
    import ctypes as C
    flat = torch.zeros(2 * 2 * 8 * 8 * 64, dtype=torch.int8, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:-64].view(2, 8, 8, 64)   # begins inside the input
    w = torch.zeros(1, 3, 3, 64, dtype=torch.int8, device=DEV)
    table = torch.zeros(3, 64, dtype=torch.int32, device=DEV)
    q = ((0.5, 0), (0.5, 0))
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.depthwise_conv2d_i8(x, w, table, *q, out=out)
    small = torch.zeros(1, 2, 2, 64, dtype=torch.int8, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.depthwise_conv2d_i8(small, w, table, *q, out=False, out_bits=w.view(-1)[:32].view(torch.int32).view(1, 2, 2, 2))
    with pytest.raises(amd.LceHipError, match="overlaps the table"):
        amd.depthwise_conv2d_i8(small[:, :1, :1].contiguous(), w, table, *q, out=table.view(torch.int8).view(-1)[:64].view(1, 1, 1, 64))
    with pytest.raises(amd.LceHipError, match="the two outputs overlap"):
        both = torch.zeros(256, dtype=torch.int8, device=DEV)
        amd.depthwise_conv2d_i8(small, w, table, *q, out=both.view(1, 2, 2, 64), out_bits=both[224:].view(torch.int32).view(1, 2, 2, 2))
    # alignment: the bits and the table need 4 bytes (the library checks the device addresses it is given; nothing is launched)
    raw = torch.zeros(4096, dtype=torch.int8, device=DEV)
    d = amd.DepthwiseI8Desc(1, 2, 2, 64, 1, 3, 3, 1, 1, amd.PADDING_SAME, amd.ACT_NONE, 0.5, 0, 0.5, 0)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    rc = amd.lib().lce_hip_depthwise_conv2d_i8(C.byref(d), p(small), p(w), p(table), None, p(raw, 2), None)
    assert rc == amd.ERR_INVALID and "out_bits_dev must be 4-byte aligned" in amd.lib().lce_hip_last_error().decode()
    rc = amd.lib().lce_hip_depthwise_conv2d_i8(C.byref(d), p(small), p(w), p(raw, 1025), p(raw, 2048), None, None)
    assert rc == amd.ERR_INVALID and "table_dev must be 4-byte aligned" in amd.lib().lce_hip_last_error().decode()
    with pytest.raises(amd.LceHipError, match="the 16-byte path needs"):
        amd.depthwise_conv2d_i8(torch.zeros(1, 2, 2, 33, dtype=torch.int8, device=DEV), torch.zeros(1, 1, 1, 33, dtype=torch.int8, device=DEV),
                                torch.zeros(3, 33, dtype=torch.int32, device=DEV), *q, path=1)
    torch.cuda.synchronize()
    assert (flat == 0).all() and (raw == 0).all() and (w == 0).all() and (table == 0).all()      # nothing was written


# ---- sections -----------------------------------------------------------------------------------------------------------------
def run_cut(data, info, x):
    """The file under every EARLIER name, section by section on the GPU, every operator outside the sections in NumPy
    (info["host"]: the depthwise convolution is tests/depthwise_i8_ref.py's).  Returns tensor index -> array for every tensor that
    crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0], **DM.EARLIER)
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
    assert model.depthwise_i8_stats() == (0, 0)
    return live


def stats(model):
    return dict(depthwise_i8=model.depthwise_i8_stats(), conv_i8=model.conv_i8_stats(), int8_add=model.int8_add_stats(), pool=model.pool_stats())


@pytest.mark.parametrize("name", sorted(DM.FIXTURES))
def test_each_fixture_runs_as_one_section(name):
    batch = 3
    data, xt, out, info = DM.FIXTURES[name]()
    x = DM.fixture_input(info, batch, 1)
    cut = run_cut(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, **DM.EVERY_FLAG)
    assert len(it.sections) == 1 and it.lce_only and it.sections[0].inputs == [xt]
    (got,) = it.run_section(0, [x])
    print(name, stats(it.model), it.model.run_stats()[1])
    want = info["oracle"](x)
    got = got.reshape(want.shape)
    assert got.dtype == info["out_dtype"] and np.array_equal(got.view(np.uint8), np.ascontiguousarray(cut[out]).reshape(want.shape).view(np.uint8))
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert np.unique(got).size > 3 and not np.array_equal(got[0], got[1])
    assert stats(it.model) == info["stats"]
    pred = it.predict(x)
    assert np.array_equal(pred.reshape(want.shape).view(np.uint8), want.view(np.uint8))
    if name.startswith("network"):
        assert pred.dtype == np.float32 and pred.shape == (batch, info["head"]["classes"])
        assert it.model.head_i8_stats() == (1, 1, 1) and it.model.quantize_stats() == (1, 1)
        with pytest.raises(RuntimeError):
            mr.Interpreter(data, batch_size=batch, **DM.EARLIER).predict(x)          # the cut file: predict() refuses it


@pytest.mark.parametrize("name", ["transition_per_channel", "network_per_tensor"])
def test_hip_graph_replay_of_a_section_gives_the_same_bytes(name):
    data, xt, out, info = DM.FIXTURES[name]()
    model = mr.LceModel(data, **DM.EVERY_FLAG)
    batch = 5
    xh = DM.fixture_input(info, batch, 11)
    x = torch.from_numpy(xh).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    y = torch.zeros(dims, dtype=torch.float32 if info["out_dtype"] == np.float32 else torch.int8, device=DEV)
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
    want = info["oracle"](xh)
    for r in runs:
        assert np.array_equal(r[0].cpu().numpy().reshape(want.shape).view(np.uint8), want.view(np.uint8))
    model.use_hip_graphs(False)
