"""lce_hip_conv2d_i8 on the MI355X, byte for byte and without tolerance: the kernel against the NumPy restatement of TFLite's
reference_integer_ops::ConvPerChannel (tests/conv2d_i8_ref.py) on the known answers worked by hand and over the grid of
K = fh fw Cin, images, batches, strides, paddings and output channels with rotating bias, activation, output combination, input
zero point and scale kind (tests/conv2d_i8_cases.py); an asymmetric filter on an identity-like image, which no row <-> column
swap in the operand or the C/D map of the matrix instruction can pass; views at a 1-byte offset; more tiles than one pass of the
capped grid; one input above 2^32 bytes; a capture and replay of the launch; the refusals that need device pointers; and the
fixtures of tests/int8_conv_models.py run as ONE section against the same file under the parent's flags with NumPy doing the
convolution on the host, and against the oracle's operators."""
import importlib

import numpy as np
import pytest

import conv2d_i8_ref as R
import int8_conv_models as M
from conv2d_i8_cases import GRID, KNOWN, operands, run_grid

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shifted(a, offset=1):
    """`a` on the device, its first byte `offset` bytes behind a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    raw = torch.zeros(a.nbytes + 16, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    t = raw[offset:offset + a.nbytes].view(torch.int8).view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == offset and t.is_contiguous()
    return t


def run(x, w, bias, sw, q_in, q_out, stride, padding, act, want_out=True, want_bits=True, offset=0):
    """amd.conv2d_i8 with the table amd.conv2d_i8_prepare makes: (out, bits, None) as NumPy arrays."""
    table, _, _ = amd.conv2d_i8_prepare(w, bias, sw, q_in, q_out, act)
    assert np.array_equal(table, R.table(w, bias, sw, q_in[0], q_in[1], q_out[0]))
    place = (lambda a: shifted(a, offset)) if offset else dev
    out, bits = amd.conv2d_i8(place(x), place(w), dev(table), q_in, q_out, stride=stride, padding=padding, activation=act,
                              out=True if want_out else False, out_bits=want_bits)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy(), None


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name):
    k = KNOWN[name]
    for outs in (dict(), dict(want_out=False), dict(want_bits=False)):
        out, bits, _ = run(k["x"], k["w"], k["bias"], k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], k["act"], **outs)
        assert out is None or (out.dtype == np.int8 and np.array_equal(out, k["want"])), (name, out)
        assert bits is None or np.array_equal(bits, R.bitpack(k["want"], k["q_out"][1])), name


@pytest.mark.parametrize("filt,cin", GRID)
def test_the_grid(filt, cin):
    n, _ = run_grid(run, filt, cin)
    assert n >= 9


def test_an_asymmetric_filter_on_an_identity_like_image_decides_rows_and_columns():
    """A 1x1 convolution of 40 pixels x 32 channels whose pixel p is 1 in channel p % 32 and 0 elsewhere, under multiplier 1 and
    zero points 0: output (p, o) is w[o][p % 32], with w[o][c] = 3 o - 5 c + 1 far from symmetric.  With the rows and columns of an
    operand or of the C/D map swapped, the kernel would write w[p % 32][o] instead."""
    pixels, cin, cout = 40, 32, 33
    x = np.zeros((1, 5, 8, cin), np.int8)
    x.reshape(pixels, cin)[np.arange(pixels), np.arange(pixels) % cin] = 1
    w = (3 * np.arange(cout)[:, None] - 5 * np.arange(cin)[None, :] + 1).astype(np.int8).reshape(cout, 1, 1, cin)
    want = w.reshape(cout, cin).T[np.arange(pixels) % cin].reshape(1, 5, 8, cout)
    assert not np.array_equal(w.reshape(cout, cin)[:32, :32], w.reshape(cout, cin)[:32, :32].T)
    assert np.array_equal(want, R.conv2d_i8(x, w, None, 1.0, (1.0, 0), (1.0, 0), 1, R.VALID))
    for offset in (0, 1):                                           # the 16-byte path and the byte path
        out, bits, _ = run(x, w, None, 1.0, (1.0, 0), (1.0, 0), 1, R.VALID, R.NONE, offset=offset)
        assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, 0))


def test_views_at_a_one_byte_offset_agree_with_the_aligned_run():
    """Cin = 16 takes 16-byte loads when input and filter allow it: each operand alone, and the output, at a 1-byte offset."""
    x, w, bias, sw, q_in, q_out = operands((3, 7, 7, 16), (3, 3), 33, 8, zi=-9)
    want = R.conv2d_i8(x, w, bias, sw, q_in, q_out, (2, 2), R.SAME, R.RELU6)
    table = dev(amd.conv2d_i8_prepare(w, bias, sw, q_in, q_out, amd.ACT_RELU6)[0])
    out = torch.zeros(want.size + 1, dtype=torch.int8, device=DEV)[1:].view(want.shape)
    assert out.data_ptr() % 16 == 1
    for xd, wd, o in ((dev(x), dev(w), True), (shifted(x), dev(w), True), (dev(x), shifted(w), True), (dev(x), dev(w), out),
                      (shifted(x), shifted(w), out)):
        got, bits = amd.conv2d_i8(xd, wd, table, q_in, q_out, stride=2, activation=amd.ACT_RELU6, out=o, out_bits=True)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), R.bitpack(want, q_out[1]))


def test_more_tiles_than_one_pass_of_the_grid_and_a_ragged_last_tile():
    """517 x 513 output pixels are 2073 tiles of 128 against the grid's cap of 2048, the last with 5 of its 128 rows."""
    assert 517 * 513 > 2048 * 128 and (517 * 513) % 128 == 5
    x, w, bias, sw, q_in, q_out = operands((1, 517, 513, 3), (3, 3), 33, 5, zi=11)
    want = R.conv2d_i8(x, w, bias, sw, q_in, q_out, (1, 1), R.SAME, R.RELU)
    out, bits, _ = run(x, w, bias, sw, q_in, q_out, 1, R.SAME, R.RELU)
    assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, q_out[1]))


def test_an_input_of_more_than_two_to_the_32_bytes():
    """69995 x 69995 pixels of one int8 channel are 4.9 GB.  3x3 at stride 9999 SAME gives 8 x 8 outputs (7 x 9999 + 3 - 69995 = 1:
    nothing in front, one row and column of padding behind); the windows of output row 7 start at byte 4.899e9 > 2^32.  The
    reference runs on the 23 touched rows and columns, which at stride 3 have the same geometry.  Run once."""
    side, s = 69995, 9999
    assert side * side > 2 ** 32 and 7 * s * side > 2 ** 32 and 7 * s + 2 == side
    free, _ = torch.cuda.mem_get_info()
    if free < side * side + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % ((side * side + (1 << 30)) / 1e9, free / 1e9))
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(-128, 128, (1, side, side, 1), dtype=torch.int8, device=DEV, generator=g)
    _, w, bias, sw, q_in, q_out = operands((1, 3, 3, 1), (3, 3), 5, 3, zi=-77)
    sw = sw * np.float32(8)                                          # (K = 9: spread the outputs over the int8 range)
    table, _, _ = amd.conv2d_i8_prepare(w, bias, sw, q_in, q_out, amd.ACT_RELU_N1_TO_1)
    out, bits = amd.conv2d_i8(x, dev(w), dev(table), q_in, q_out, stride=s, padding=amd.PADDING_SAME, activation=amd.ACT_RELU_N1_TO_1,
                              out_bits=True)
    torch.cuda.synchronize()
    assert out.shape == (1, 8, 8, 5) and bits.shape == (1, 8, 8, 1)
    touched = torch.tensor([o * s + d for o in range(8) for d in range(3) if o * s + d < side], device=DEV)
    assert touched.numel() == 23
    small = x[:, touched][:, :, touched].cpu().numpy()
    want = R.conv2d_i8(small, w, bias, sw, q_in, q_out, (3, 3), R.SAME, R.RELU_N1_TO_1)
    assert want.shape == (1, 8, 8, 5) and np.array_equal(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), R.bitpack(want, q_out[1]))


def test_a_capture_and_replay_of_the_launch():
    """The launch allocates and copies nothing: captured once into a HIP graph, replayed on new contents of the same buffers."""
    x, w, bias, sw, q_in, q_out = operands((2, 9, 8, 3), (3, 3), 40, 21, zi=4)
    table = dev(amd.conv2d_i8_prepare(w, bias, sw, q_in, q_out, amd.ACT_NONE)[0])
    xd, wd = dev(x), dev(w)
    want0 = R.conv2d_i8(x, w, bias, sw, q_in, q_out, (2, 2), R.SAME)
    out = torch.zeros(want0.shape, dtype=torch.int8, device=DEV)
    bits = torch.zeros(want0.shape[:3] + (2,), dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        amd.conv2d_i8(xd, wd, table, q_in, q_out, stride=2, out=out, out_bits=bits, stream=s.cuda_stream)       # eager first
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            amd.conv2d_i8(xd, wd, table, q_in, q_out, stride=2, out=out, out_bits=bits, stream=s.cuda_stream)
    for seed in (1, 2):
        x2 = np.random.default_rng(seed).integers(-128, 128, x.shape, dtype=np.int64).astype(np.int8)
        xd.copy_(torch.from_numpy(x2))
        out.zero_(), bits.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = R.conv2d_i8(x2, w, bias, sw, q_in, q_out, (2, 2), R.SAME)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), R.bitpack(want, q_out[1]))


def test_refusals_on_the_device():
    flat = torch.zeros(2 * 2 * 8 * 8 * 64, dtype=torch.int8, device=DEV)
    x, out = flat[:2 * 8 * 8 * 64].view(2, 8, 8, 64), flat[2 * 8 * 8 * 64 - 64:-64].view(2, 8, 8, 64)   # begins inside the input
    w = torch.zeros(64, 3, 3, 64, dtype=torch.int8, device=DEV)
    table = torch.zeros(3, 64, dtype=torch.int32, device=DEV)
    q = ((0.5, 0), (0.5, 0))
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.conv2d_i8(x, w, table, *q, out=out)
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.conv2d_i8(x, w, table, *q, out=False, out_bits=w.view(-1)[:1024].view(torch.int32).view(2, 8, 8, 2))
    with pytest.raises(amd.LceHipError, match="overlaps the table"):
        amd.conv2d_i8(x[:1, :1, :1], w, table, *q, out=table.view(torch.int8).view(-1)[:64].view(1, 1, 1, 64))


# ---- sections -----------------------------------------------------------------------------------------------------------------
def run_cut(data, info, x):
    """The file under the PARENT's flags, section by section on the GPU, every operator outside them in NumPy (info["host"]: the
    convolution is tests/conv2d_i8_ref.py's).  Returns tensor index -> array for every tensor that crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0], **info["parent_flags"])
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
    assert model.conv_i8_stats() == (0, 0)
    return live


def stats(model):
    return dict(conv_i8=model.conv_i8_stats(), int8_add=model.int8_add_stats(), pool=model.pool_stats())


def image(info, batch, seed):
    return np.random.default_rng(seed).integers(-128, 128, (batch,) + info["shape"], dtype=np.int64).astype(np.int8)


@pytest.mark.parametrize("batch", [2, 3])
@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_each_fixture_runs_as_one_section(name, batch):
    data, xt, out, info = M.FIXTURES[name]()
    x = image(info, batch, batch)
    cut = run_cut(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, **M.ALL_FLAGS)
    assert len(it.sections) == 1 and it.lce_only and it.sections[0].inputs == [xt]
    (got,) = it.run_section(0, [x])
    print(name, batch, stats(it.model), it.model.run_stats()[1])
    want = info["oracle"](x)
    assert got.dtype == np.int8 and got.shape == want.shape and np.array_equal(got, cut[out]) and np.array_equal(got, want)
    assert stats(it.model) == info["stats"]
    assert np.array_equal(it.predict(x), want)


@pytest.mark.parametrize("name", ["shortcut_per_channel", "stem_per_tensor"])
def test_hip_graph_replay_gives_the_same_bytes(name):
    data, xt, out, info = M.FIXTURES[name]()
    model = mr.LceModel(data, **M.ALL_FLAGS)
    batch = 5
    xh = image(info, batch, 11)
    x = torch.from_numpy(xh).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    y = torch.zeros(dims, dtype=torch.int8, device=DEV)
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
    for r in runs:
        assert np.array_equal(r[0].cpu().numpy(), info["oracle"](xh))
    model.use_hip_graphs(False)
