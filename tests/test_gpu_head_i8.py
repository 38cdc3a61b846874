"""The int8 classifier head and the float / int8 boundary on the MI355X, byte for byte and without tolerance: lce_hip_fully_connected_i8
against the NumPy restatement (tests/head_i8_ref.py) over the grid of batch, K and N with rotating bias, scale kind, input zero point
and activation (tests/head_i8_cases.py); the MAP case -- one-hot rows against an asymmetric weight, which no row <-> column swap in
the operand map or the C/D map of v_mfma_i32_16x16x64_i8 can pass; the accumulator's extremes; views at a 1-byte offset (the byte
path with K % 16 == 0); equality with lce_hip_conv2d_i8 on the one-pixel image; lce_hip_mean_i8, lce_hip_softmax_i8,
lce_hip_quantize_f32_i8 and lce_hip_dequantize_i8_f32 against their restatements; the refusals that need device pointers; a capture
and replay of the head's four launches; and the fixtures of tests/head_i8_models.py run as ONE section through
Interpreter.predict() against the same file cut under the parent's flags with NumPy doing the new operators, and against the
oracle."""
import importlib

import numpy as np
import pytest

import head_i8_cases as K
import head_i8_models as HM
import head_i8_ref as H
import int8_conv_models as M

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


def run(x, w, bias, sw, q_in, q_out, act=H.NONE, offset=0):
    """amd.fully_connected_i8 with the table amd.fully_connected_i8_prepare makes: (out as a NumPy array, None)."""
    table, _, _ = amd.fully_connected_i8_prepare(w, bias, sw, q_in, q_out, act)
    assert np.array_equal(table, H.fc_table(w, bias, sw, q_in[0], q_in[1], q_out[0]))
    place = (lambda a: shifted(a, offset)) if offset else dev
    out = amd.fully_connected_i8(place(x), place(w), dev(table), q_in, q_out, act)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None


# ---- FULLY_CONNECTED ----------------------------------------------------------------------------------------------------------------
def test_the_grid():
    n, vecs = K.run_fc_grid(run)
    assert n == len(K.FC_GRID) and vecs >= 6


def test_the_map_case_decides_the_operand_map_and_the_cd_map():
    """Input row i is one-hot at k = i mod K with a value that depends on i; w[o][k] = 3 o - 5 k folded into int8 is asymmetric.
    Output (i, o) comes from w[o][i mod K] alone: with rows and columns swapped in an operand or in the C/D map -- a transposed
    store -- the kernel would write what belongs at (o, i)."""
    x, w, bias, sw, q_in, q_out = K.map_case()
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out)
    assert np.unique(want).size > 100 and not np.array_equal(want[:33, :33], want[:33, :33].T)
    for offset in (0, 1):                                           # K = 70: the byte path either way; and K = 64 below
        out, _ = run(x, w, bias, sw, q_in, q_out, offset=offset)
        assert np.array_equal(out, want), np.argwhere(out != want)[:5]
    x, w, bias, sw, q_in, q_out = K.map_case(33, 64, 33)            # the 16-byte path
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out)
    assert not np.array_equal(want[:33, :33], want[:33, :33].T)
    out, _ = run(x, w, bias, sw, q_in, q_out)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]


def test_the_accumulators_extremes():
    x, w, bias, sw, q_in, q_out = K.extremes_case()
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out)
    assert len(set(want[0].tolist())) >= 3
    out, _ = run(x, w, bias, sw, q_in, q_out)
    assert np.array_equal(out, want)


def test_views_at_a_one_byte_offset_force_the_byte_path_with_k_a_multiple_of_16():
    x, w, bias, sw, q_in, q_out = K.fc_operands(17, 64, 33, 5)
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out, H.RELU)
    table = dev(amd.fully_connected_i8_prepare(w, bias, sw, q_in, q_out, amd.ACT_RELU)[0])
    out = torch.zeros(want.size + 1, dtype=torch.int8, device=DEV)[1:].view(want.shape)
    assert out.data_ptr() % 16 == 1
    for xd, wd, o in ((dev(x), dev(w), None), (shifted(x), dev(w), None), (dev(x), shifted(w), None), (dev(x), dev(w), out),
                      (shifted(x, 15), shifted(w, 3), out)):
        got = amd.fully_connected_i8(xd, wd, table, q_in, q_out, amd.ACT_RELU, out=o)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("batch,k,n", [(33, 70, 1000), (3, 512, 70), (17, 65, 33)])
def test_the_bytes_of_conv2d_i8_on_the_one_pixel_image(batch, k, n):
    x, w, bias, sw, q_in, q_out = K.fc_operands(batch, k, n, 3, zi=-9)
    table = dev(amd.fully_connected_i8_prepare(w, bias, sw, q_in, q_out, amd.ACT_RELU6)[0])
    fc = amd.fully_connected_i8(dev(x), dev(w), table, q_in, q_out, amd.ACT_RELU6)
    conv, _ = amd.conv2d_i8(dev(x.reshape(batch, 1, 1, k)), dev(w.reshape(n, 1, 1, k)), table, q_in, q_out, activation=amd.ACT_RELU6)
    torch.cuda.synchronize()
    assert torch.equal(fc, conv.view(batch, n)) and len(torch.unique(fc)) > 20
    assert np.array_equal(fc.cpu().numpy(), H.fully_connected_i8(x, w, bias, sw, q_in, q_out, H.RELU6))


# ---- MEAN, SOFTMAX, QUANTIZE / DEQUANTIZE ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(K.MEAN_SETS) + 1))
def test_mean(case):
    h, w, c, q_in, q_out = (K.MEAN_SETS + [(7, 7, 512, (0.05, -4), (0.021, 3))])[case]
    x = K.mean_input(h, w, c, 3, 40 + case)
    got = amd.mean_i8(dev(x), q_in, q_out)
    torch.cuda.synchronize()
    assert got.shape == (3, c) and np.array_equal(got.cpu().numpy(), H.mean_i8(x, q_in, q_out))


@pytest.mark.parametrize("rows", [1, 3, 257])
def test_softmax(rows):
    for cols in (1, 7, 63, 64, 65, 129, 1000):
        q = K.softmax_input(rows, cols, rows + cols)
        for scale, beta in ((0.05, 1.0), (0.2, 0.5)):
            got = amd.softmax_i8(dev(q), scale, beta)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), H.softmax_i8(q, scale, beta)), (rows, cols, scale)
    qd = dev(q)                                                      # in place
    assert amd.softmax_i8(qd, 0.05, out=qd) is qd
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy(), H.softmax_i8(q, 0.05))


def test_quantize_and_dequantize():
    g = np.random.default_rng(9)
    x = (g.standard_normal((3, 17, 17, 3)) * 3).astype(np.float32)
    x.reshape(-1)[:9] = [np.nan, np.inf, -np.inf, 0.025, -0.025, 0.075, 1e30, -1e30, -0.0]
    q = g.integers(-128, 128, (257, 1000), dtype=np.int64).astype(np.int8)
    for scale, zp in ((0.05, -4), (0.0157, -128), (1.0 / 256.0, -128), (1.0, 127)):
        got = amd.quantize_i8(dev(x), (scale, zp))
        back = amd.dequantize_i8(dev(q), (scale, zp))
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), H.quantize(x, scale, zp)) and int(got.view(-1)[0]) == zp
        assert np.array_equal(back.cpu().numpy().view(np.uint32), H.dequantize(q, scale, zp).view(np.uint32))
        every = dev(np.arange(-128, 128).astype(np.int8))
        assert torch.equal(amd.quantize_i8(amd.dequantize_i8(every, (scale, zp)), (scale, zp)), every)
    assert np.array_equal(amd.quantize_i8(x[0, 0, 0], (0.5, 3)), H.quantize(x[0, 0, 0], 0.5, 3))       # NumPy in, NumPy out


def test_refusals_on_the_device_and_no_launch_afterwards():
    flat = torch.full((4096,), 7, dtype=torch.int8, device=DEV)
    x, w = flat[:16 * 64].view(16, 64), torch.zeros(32, 64, dtype=torch.int8, device=DEV)
    table = torch.zeros(3, 32, dtype=torch.int32, device=DEV)
    q = ((0.5, 0), (0.5, 0))
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.fully_connected_i8(x, w, table, *q, out=flat[1000:1000 + 16 * 32].view(16, 32))
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.fully_connected_i8(x, w, table, *q, out=w.view(-1)[:512].view(16, 32))
    with pytest.raises(amd.LceHipError, match="overlaps the table"):
        amd.fully_connected_i8(x[:1], w, table, *q, out=table.view(torch.int8).view(-1)[:32].view(1, 32))
    img = flat[:2 * 3 * 3 * 8].view(2, 3, 3, 8)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.mean_i8(img, *q, out=flat[140:156].view(2, 8))
    with pytest.raises(amd.LceHipError, match="partly overlaps"):
        amd.softmax_i8(flat[:40].view(4, 10), 0.1, out=flat[5:45].view(4, 10))
    with pytest.raises(amd.LceHipError, match="exactly"):
        amd.softmax_i8(flat[:40].view(4, 10), 0.1, q_out=(1.0 / 256.0, 0))
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.quantize_i8(f, (0.5, 0), out=f.view(torch.int8)[8:72])
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.dequantize_i8(f.view(torch.int8)[:64], (0.5, 0), out=f)
    torch.cuda.synchronize()
    assert bool((flat == 7).all()) and bool((f == 0).all()) and bool((w == 0).all())          # nothing was launched


def test_a_capture_and_replay_of_the_four_launches_of_the_head():
    """MEAN -> FULLY_CONNECTED -> SOFTMAX -> DEQUANTIZE allocate and copy nothing: captured once into a HIP graph, replayed twice on
    new contents of the same buffers."""
    x, w, bias, sw, q_p, q_l = K.fc_operands(5, 40, 7, 2)
    q_x = (0.05, -4)
    table = dev(amd.fully_connected_i8_prepare(w, bias, sw, q_p, q_l)[0])
    img = K.mean_input(5, 5, 40, 5, 0)
    xd, wd = dev(img), dev(w)
    pooled = torch.zeros((5, 40), dtype=torch.int8, device=DEV)
    logits, probs = (torch.zeros((5, 7), dtype=torch.int8, device=DEV) for _ in range(2))
    scores = torch.zeros((5, 7), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def head():
        amd.mean_i8(xd, q_x, q_p, out=pooled, stream=s.cuda_stream)
        amd.fully_connected_i8(pooled, wd, table, q_p, q_l, out=logits, stream=s.cuda_stream)
        amd.softmax_i8(logits, q_l[0], out=probs, stream=s.cuda_stream)
        amd.dequantize_i8(probs, H.SOFTMAX_OUT, out=scores, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        head()                                                       # eager first
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            head()
    for seed in (1, 2):
        img2 = K.mean_input(5, 5, 40, 5, seed)
        xd.copy_(torch.from_numpy(img2))
        scores.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = H.dequantize(H.softmax_i8(H.fully_connected_i8(H.mean_i8(img2, q_x, q_p), w, bias, sw, q_p, q_l), q_l[0]), *H.SOFTMAX_OUT)
        assert np.array_equal(scores.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.unique(want).size > 3


# ---- sections -----------------------------------------------------------------------------------------------------------------
def run_cut(data, info, x):
    """The file under the PARENT's flags (every name but head_i8 and quantize), section by section on the GPU, every operator
    outside them in NumPy (info["host"]: the restatements of tests/head_i8_ref.py).  Returns tensor index -> array."""
    it = mr.Interpreter(data, batch_size=x.shape[0], **M.ALL_FLAGS)
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
    assert len(ran) == len(it.sections) and model.head_i8_stats() == (0, 0, 0) and model.quantize_stats() == (0, 0)
    return live


@pytest.mark.parametrize("name", sorted(HM.FIXTURES))
def test_each_fixture_runs_as_one_section_through_predict(name):
    batch = 3
    data, xt, out, info = HM.FIXTURES[name]()
    x = HM.fixture_input(info, batch, 1)
    cut = run_cut(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, **HM.EVERY_FLAG)
    assert len(it.sections) == 1 and it.lce_only and it.sections[0].inputs == [xt]
    got = it.predict(x)
    want = info["oracle"](x)
    stats = (it.model.head_i8_stats(), it.model.quantize_stats(), it.model.conv_i8_stats())
    print(name, stats)
    assert got.dtype == info["out_dtype"] and got.shape == want.shape == (batch, info["head"]["classes"])
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(cut[out]).view(np.uint8)) and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert np.unique(got).size > 3 and not np.array_equal(got[0], got[1])
    network = name.startswith("network")
    assert stats == ((1, 1, 1), (int(network and info["in_dtype"] == np.float32), int(info["out_dtype"] == np.float32)), (int(network), int(network)))
    (again,) = it.run_section(0, [x])
    assert np.array_equal(again.reshape(got.shape).view(np.uint8), got.view(np.uint8))


def test_hip_graph_replay_of_the_whole_network_gives_the_same_bytes():
    data, xt, out, info = HM.network_fixture()
    model = mr.LceModel(data, **HM.EVERY_FLAG)
    batch = 5
    xh = HM.fixture_input(info, batch, 11)
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
            runs.append((y.clone(), model.head_i8_stats(), model.quantize_stats(), model.graph_stats()))
    assert [r[3] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1:3] for r in runs] == [((1, 1, 1), (1, 1))] * 3
    want = info["oracle"](xh)
    for r in runs:
        assert np.array_equal(r[0].cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32))
    model.use_hip_graphs(False)
