"""The binarized Dense layer on the MI355X.  lce_hip_binary_fully_connected against the NumPy restatement
(tests/binary_dense_ref.py) byte for byte -- this decides what the host simulation cannot, the operand and accumulator layout of
the FP4 matrix instruction --, against lce_hip_unpack + lce_hip_fully_connected_f32 byte for byte where the scales are powers of
two, against float64 within a derived bound where they are not, and the fixture networks of tests/binary_dense_models.py through
run_section, predict and HIP-graph replay against their NumPy forward passes."""
import importlib

import numpy as np
import pytest

import binary_dense_models as BM
import binary_dense_ref as R
import head_ref as HR

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BATCHES, KS, NS = (1, 33, 65), (31, 64, 65, 288, 9216), (1, 33, 100)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def operands(m, k, n, seed, scales="mixed"):
    g = np.random.default_rng(seed)
    a_neg = g.integers(0, 2, (m, k)).astype(bool)
    a_neg[0] = False                                                 # against an all-equal weight row: |t| = K
    w, s, bias = BM.dense_weights(g, k, n, scales)
    w[0] = np.abs(w[0])
    return R.pack_signs(a_neg), w, s, bias


# ---- the entry against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_the_entry_gives_the_restated_bytes(k):
    checks = 0
    for m in BATCHES:
        a, w, s, bias = operands(m, k, max(NS), 100 * m + k)
        ad = dev(a)
        for n in NS:
            wb, sc = amd.bfc_prepare(w[:n])
            assert np.array_equal(sc.view(np.int32), s[:n].view(np.int32))
            wbd, scd, bd = dev(wb), dev(sc), dev(bias[:n])
            for act, with_bias in ((amd.ACT_NONE, True), (amd.ACT_RELU, False), (amd.ACT_RELU_N1_TO_1, True), (amd.ACT_RELU6, True)):
                b = bias[:n] if with_bias else None
                want_v, want_bits = R.binary_fully_connected(a, wb, sc, b, k, act)
                v, bits = amd.binary_fully_connected(ad, k, wbd, scd, bd if with_bias else None, activation=act, out=True, out_bits=True)
                assert same(host(v), want_v) and np.array_equal(host(bits), want_bits), (m, k, n, act)
                if act == amd.ACT_RELU_N1_TO_1:                      # each output alone
                    v1, none = amd.binary_fully_connected(ad, k, wbd, scd, bd, activation=act)
                    none2, bits1 = amd.binary_fully_connected(ad, k, wbd, scd, bd, activation=act, out=False, out_bits=True)
                    assert none is None and none2 is None and torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(bits1, bits)
                checks += 1
    assert checks == len(BATCHES) * len(NS) * 4


def test_numpy_in_numpy_out_and_the_scalar_load_path():
    a, w, s, bias = operands(33, 512, 40, 7)
    wb, sc = amd.bfc_prepare(w)
    want_v, want_bits = R.binary_fully_connected(a, wb, sc, bias, 512, R.RELU)
    v, bits = amd.binary_fully_connected(a, 512, wb, sc, bias, activation=amd.ACT_RELU, out_bits=True)
    assert same(v, want_v) and np.array_equal(bits, want_bits)
    # operands 4 bytes behind a 16-byte boundary take the 4-byte loads
    buf_a = torch.zeros(a.size + 1, dtype=torch.int32, device=DEV)
    buf_w = torch.zeros(wb.size + 1, dtype=torch.int32, device=DEV)
    ad, wd = buf_a[1:].view(a.shape), buf_w[1:].view(wb.shape)
    ad.copy_(dev(a))
    wd.copy_(dev(wb))
    assert ad.data_ptr() % 16 == 4
    v, bits = amd.binary_fully_connected(ad, 512, wd, dev(sc), dev(bias), activation=amd.ACT_RELU, out_bits=True)
    assert same(host(v), want_v) and np.array_equal(host(bits), want_bits)


def test_more_tiles_than_one_pass_of_the_grid():
    """2080 x 4100 outputs are 65 x 129 = 8385 tiles against the 8192 waves of one pass of the grid."""
    m, k, n = 2080, 8, 4100
    a, w, s, bias = operands(m, k, n, 11)
    wb, sc = amd.bfc_prepare(w)
    v, bits = amd.binary_fully_connected(dev(a), k, dev(wb), dev(sc), dev(bias), out_bits=True)
    want_v, want_bits = R.binary_fully_connected(a, wb, sc, bias, k)
    assert same(host(v), want_v) and np.array_equal(host(bits), want_bits)


# ---- against the float entry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n", [(33, 288, 100), (65, 9216, 33), (1, 65, 33), (65, 512, 1000)])
def test_power_of_two_scales_give_the_bytes_of_the_float_chain(m, k, n):
    """Every product +-1 x +-2^e and every partial sum of the float chain is exact, so lce_hip_unpack +
    lce_hip_fully_connected_f32 on the same bits and the float weights computes the same bytes, whatever the bias."""
    a, w, s, bias = operands(m, k, n, 21 + k, scales="pow2")
    w[1] = np.sign(w[1]) * np.float32(1.0)                          # (a scale of exactly 1)
    wb, sc = amd.bfc_prepare(w)
    ad, wd, bd = dev(a), dev(w), dev(bias)
    for act, b in ((amd.ACT_NONE, bd), (amd.ACT_RELU6, bd), (amd.ACT_NONE, None)):
        new, _ = amd.binary_fully_connected(ad, k, dev(wb), dev(sc), b, activation=act)
        old = amd.fully_connected(amd.unpack(ad, k, torch.float32), wd, b, activation=act)
        assert torch.equal(new.view(torch.int32), old.view(torch.int32)), (m, k, n, act)


@pytest.mark.parametrize("m,k,n", [(33, 288, 100), (65, 9216, 33), (1, 31, 33)])
def test_random_scales_stay_within_two_half_ulps_of_float64(m, k, n):
    """v = fl(fl(t s) + b): |v - (t s + b)| <= ulp(p) / 2 + ulp(v) / 2, p = fl(t s).  Derived, not measured; the float chain is
    not compared here (it rounds K times)."""
    a, w, s, bias = operands(m, k, n, 31 + k)
    wb, sc = amd.bfc_prepare(w)
    v, _ = amd.binary_fully_connected(dev(a), k, dev(wb), dev(sc), dev(bias))
    v = host(v)
    t = R.dot(a, wb, k).astype(np.float64)
    exact = t * sc.astype(np.float64)[None, :] + bias.astype(np.float64)[None, :]
    p = (t * sc.astype(np.float64)[None, :]).astype(np.float32)
    bound = 0.5 * np.spacing(np.abs(p)).astype(np.float64) + 0.5 * np.spacing(np.abs(v)).astype(np.float64)
    err = np.abs(v.astype(np.float64) - exact)
    print("largest error / bound: %.3f" % float((err / bound).max()))
    assert (err <= bound).all()


def test_the_entry_refuses_on_the_device():
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    a, wb = buf[:8].view(4, 2), buf[8:18].view(5, 2)
    sc, out = torch.ones(5, device=DEV), torch.zeros(4, 5, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the input"):
        amd.binary_fully_connected(a, 64, wb, sc, out_bits=buf[4:8].view(4, 1), out=False)
    with pytest.raises(amd.LceHipError, match="overlaps the filter"):
        amd.binary_fully_connected(a, 64, wb, sc, out_bits=buf[16:20].view(4, 1), out=False)
    with pytest.raises(ValueError):
        amd.binary_fully_connected(a, 65, wb, sc)                    # three words per row, not two
    with pytest.raises(ValueError):
        amd.binary_fully_connected(a, 64, wb, sc, out=False)
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and float(out.abs().sum()) == 0.0


# ---- whole networks --------------------------------------------------------------------------------------------------------------
def images(n, shape, seed):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(shape)).astype(np.float32)


def replay(model, section, batch, inputs, stats):
    """The section eagerly, recorded and replayed on a private stream: the outputs of the three runs (equal, checked here)."""
    sec = model.sections[section]
    ins = [dev(x) for x in inputs]
    outs = [torch.zeros(model.section_tensor_shape(section, t, batch)[0], dtype=torch.float32, device=DEV) for t in sec.outputs]
    s = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(s):
        model.use_hip_graphs(True)
        for _ in range(3):
            for y in outs:
                y.zero_()
            model.run_section(section, batch, [x.data_ptr() for x in ins], [y.data_ptr() for y in outs], s.cuda_stream)
            s.synchronize()
            runs.append(([y.clone() for y in outs], stats(), model.graph_stats()))
    model.use_hip_graphs(False)
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert runs[0][1] == runs[1][1] == runs[2][1]
    for r in runs[1:]:
        for y, y0 in zip(r[0], runs[0][0]):
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
    return [y.cpu().numpy().reshape(batch, -1) for y in runs[2][0]], runs[2][1]


@pytest.mark.parametrize("fixture", ("alexnet_tail", "body_tail"))
def test_a_tail_of_binary_dense_layers_runs_from_the_image_to_the_probabilities(fixture):
    data, xt, outs, info = (BM.alexnet_tail_model if fixture == "alexnet_tail" else BM.body_tail_model)()
    n_layers = len(info["layers"])
    it = mr.Interpreter(data, batch_size=4, stem_sections=True, **BM.KEYWORDS_HEAD)
    assert len(it.sections) == 1 and it.lce_only
    x = images(7, info["shape"], 41)
    logits, probs, _ = BM.tail_forward(BM.flat_of(x, info), info)
    assert fixture == "alexnet_tail" or np.unique(logits).size > 20   # (alexnet_tail: a RELU in front of a sign leaves one constant input)
    want_stats = ((n_layers, n_layers, n_layers - 1), (0, 0, 1))
    stats = lambda: (it.model.binary_dense_stats(), it.model.head_stats())
    for batch in (1, 5):
        (got,) = it.run_section(0, [x[:batch]])
        assert got.shape == (batch, 10) and same(got, probs[:batch]), batch
        assert stats() == want_stats
    got = it.predict(x)                                              # a ragged last batch: 4 + 3
    assert got.shape == (7, 10) and same(got, probs)
    assert stats() == want_stats
    (got,), seen = replay(it.model, 0, 3, [x[:3]], stats)
    assert same(got, probs[:3]) and seen == want_stats
    # up to the last Dense layer's output byte for byte, and the stated softmax behind it
    body = mr.Interpreter(data, stem_sections=True, **BM.KEYWORDS)
    (got,) = body.run_section(0, [x])
    assert same(got, logits) and same(HR.softmax(got), probs)
    assert body.model.binary_dense_stats() == want_stats[0] and body.model.head_stats() == (0, 0, 0)
    # the float entries on the dequantized signs agree within rounding (they round once per input)
    ref = mr.Interpreter(data, stem_sections=True, head_sections=True, reshape_sections=True)
    (old,) = ref.run_section(0, [x])
    assert ref.model.head_stats() == (0, n_layers, 1) and old.shape == got.shape


def test_a_skipped_dequantize_costs_no_bytes_of_intermediates():
    data, xt, outs, info = BM.alexnet_tail_model()
    model = mr.LceModel(data, stem_sections=True, **BM.KEYWORDS_HEAD)
    batch = 5
    x = dev(images(batch, info["shape"], 43))
    y = torch.zeros(model.section_tensor_shape(0, outs[0], batch)[0], dtype=torch.float32, device=DEV)
    model.run_section(0, batch, [x.data_ptr()], [y.data_ptr()], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    # the bits in front of each Dense layer and the logits the SOFTMAX reads: no dequantized floats, no hidden Dense values
    words = sum((L["k"] + 31) // 32 for L in info["layers"])
    assert model.run_stats()[2] == batch * 4 * (words + 10)
    assert model.binary_dense_stats() == (3, 3, 2)


def test_a_dequantize_with_a_second_reader_is_still_written():
    data, xt, outs, info = BM.second_reader_model()
    it = mr.Interpreter(data, **BM.KEYWORDS)
    assert len(it.sections) == 1 and it.lce_only                    # (the graph begins at its rank-2 input)
    t = np.tanh(images(5, (info["k"],), 47)).astype(np.float32)
    want_out, want_sign = BM.second_reader_forward(t, info)
    by_tensor = dict(zip(it.sections[0].outputs, range(2)))
    for batch in (1, 5):
        got = it.run_section(0, [t[:batch]])
        assert same(got[by_tensor[outs[0]]], want_out[:batch]) and same(got[by_tensor[info["sign"]]], want_sign[:batch])
        assert it.model.binary_dense_stats() == (1, 0, 0)
    # predict: the delivered dequantize and the Dense output into the pipeline's buffers, a ragged last batch (2 + 2 + 1)
    got = mr.Interpreter(it.model, batch_size=2).predict(t)
    assert [g.shape for g in got] == [want_out.shape, want_sign.shape] and same(got[0], want_out) and same(got[1], want_sign)
    assert it.model.binary_dense_stats() == (1, 0, 0)
    got, seen = replay(it.model, 0, 3, [t[:3]], it.model.binary_dense_stats)
    assert same(got[by_tensor[outs[0]]], want_out[:3]) and same(got[by_tensor[info["sign"]]], want_sign[:3]) and seen == (1, 0, 0)


def test_a_dense_output_that_is_delivered_and_quantized_gives_both():
    data, xt, outs, info = BM.value_and_bits_model()
    it = mr.Interpreter(data, **BM.KEYWORDS)
    assert len(it.sections) == 1 and it.sections[0].outputs == outs and it.lce_only
    t = np.tanh(images(6, (info["layers"][0]["k"],), 53)).astype(np.float32)
    want = BM.value_and_bits_forward(t, info)
    for batch in (1, 6):
        got = it.run_section(0, [t[:batch]])
        assert same(got[0], want[0][:batch]) and same(got[1], want[1][:batch])
        assert it.model.binary_dense_stats() == (2, 2, 1)
    # predict: a launch that writes value AND bits, the value into the pipeline's buffer, a ragged last batch (4 + 2)
    got = mr.Interpreter(it.model, batch_size=4).predict(t)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert it.model.binary_dense_stats() == (2, 2, 1)
    got, seen = replay(it.model, 0, 4, [t[:4]], it.model.binary_dense_stats)
    assert same(got[0], want[0][:4]) and same(got[1], want[1][:4]) and seen == (2, 2, 1)


def test_a_dequantize_read_by_a_binary_layer_and_by_another_operator_of_the_section_is_still_written():
    """One `binary_dense` reader and one `head` FULLY_CONNECTED (mixed magnitudes) read the same dequantized tensor in the same
    section: the LceDequantize runs, the binary layer still reads the bits."""
    data, xt, outs, info = BM.shared_reader_model()
    it = mr.Interpreter(data, batch_size=2, **BM.KEYWORDS_HEAD)
    assert len(it.sections) == 1 and it.lce_only and it.sections[0].outputs == outs
    t = np.tanh(images(5, (info["k"],), 61)).astype(np.float32)
    want = BM.shared_reader_forward(t, info)
    stats = lambda: (it.model.binary_dense_stats(), it.model.head_stats())
    for batch in (1, 5):
        got = it.run_section(0, [t[:batch]])
        assert same(got[0], want[0][:batch]) and same(got[1], want[1][:batch])
        assert stats() == ((1, 0, 0), (0, 1, 0))
    got = it.predict(t)
    assert same(got[0], want[0]) and same(got[1], want[1]) and stats() == ((1, 0, 0), (0, 1, 0))
    got, seen = replay(it.model, 0, 3, [t[:3]], stats)
    assert same(got[0], want[0][:3]) and same(got[1], want[1][:3]) and seen == ((1, 0, 0), (0, 1, 0))
    # the dequantized floats are an intermediate of this section: bits, then floats
    assert it.model.run_stats()[2] >= 5 * 4 * ((info["k"] + 31) // 32 + info["k"])


@pytest.mark.parametrize("case", ("mixed_magnitudes", "rank4_hw"))
def test_a_refused_dense_layer_runs_on_the_float_entry(case):
    data, xt, out, info = BM.refusal_model(case)
    it = mr.Interpreter(data, **BM.KEYWORDS_HEAD)
    shape = tuple(it.model.tensors[it.sections[0].inputs[0]].shape[1:])
    t = np.tanh(images(3, shape, 59)).astype(np.float32)
    (got,) = it.run_section(0, [t])
    sign = np.where(t < 0, np.float32(-1), np.float32(1)).reshape(3, -1)
    assert same(got, HR.fully_connected(sign, info["w"], info["wb"]))
    assert it.model.binary_dense_stats() == (0, 0, 0) and it.model.head_stats() == (0, 1, 0)
