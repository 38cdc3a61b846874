"""lce_hip_add_int8 and the int8-ADD sections on the MI355X, bit for bit with no tolerance: the kernel over ALL 65 536 input
pairs against the NumPy restatement of TFLite's integer arithmetic (tests/int8_add_ref.py), its bits against the oracle's int8
LceQuantize at the output zero point, every kernel variant forced, and an int8 residual body run as ONE section against the
same file run section by section at the default partition with the NumPy ADD in between."""
import importlib

import numpy as np
import pytest

import int8_add_ref as R
import oracle_lib as O
from test_int8_add_host import EQUAL_SCALES, INT8_BODY, NO_CHEAP_FORM, RATIO_2_12, int8_body_model

torch = pytest.importorskip("torch")
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = (R.ACT_NONE, R.ACT_RELU, R.ACT_RELU_N1_TO_1, R.ACT_RELU6)


def qkw(q, act=R.ACT_NONE):
    return dict(q1=q[0:2], q2=q[2:4], q_out=q[4:6], activation=act)


def run(x1, x2, q, act=R.ACT_NONE, **kw):
    a, b = torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV)
    out, bits = amd.add_int8(a, b, **qkw(q, act), **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def check(x1, x2, q, act=R.ACT_NONE, **kw):
    want = R.add_q(x1, x2, q, act)
    got, bits = run(x1, x2, q, act, out_bits=True, **kw)
    assert np.array_equal(got, want), (q, act, kw, int(np.count_nonzero(got != want)))
    assert np.array_equal(bits, O.bitpack(want, q[5])), (q, act, kw)
    return want


def layouts():
    """Every (x1, x2) pair as [256, 256] and [1024, 64] (the flat path) and with a ragged channel count, [1041, 63]: the 65 536
    pairs followed by the first 47 again (the row path).  Each layout holds every pair; none is skipped."""
    x1, x2 = R.all_pairs()
    f1, f2 = x1.reshape(-1), x2.reshape(-1)
    ragged = lambda f: np.concatenate([f, f[:1041 * 63 - 65536]]).reshape(1041, 63)
    return (("256x256", x1, x2), ("1024x64", f1.reshape(1024, 64), f2.reshape(1024, 64)), ("1041x63", ragged(f1), ragged(f2)))


CASES = ([("A act %d" % a, R.SET_A, a) for a in ACTS] +
         [("B", R.SET_B, 0), ("C", R.SET_C, 0), ("C relu6", R.SET_C, 3), ("equal scales", EQUAL_SCALES, 0),
          ("ratio 2^-12", RATIO_2_12, 1)] +
         [("literal %d" % k, q, 0) for k, q in enumerate(NO_CHEAP_FORM)] +
         [("random %d" % k, q, k % 4) for k, q in enumerate(R.random_sets(24, seed=2))])


@pytest.mark.parametrize("name,q,act", CASES, ids=[c[0] for c in CASES])
def test_all_pairs_match_the_restatement(name, q, act):
    for layout, x1, x2 in layouts():
        assert x1.size >= 65536
        want = check(x1, x2, q, act)
        assert np.array_equal(R.bitpack(want, q[5]), O.bitpack(want, q[5]))


def test_set_a_is_not_real_rounding_on_the_gpu():
    x1, x2 = R.all_pairs()
    got, _ = run(x1, x2, R.SET_A)
    assert np.count_nonzero(got != R.real_rounding(x1, x2, R.SET_A)) == 14


ALL_VARIANTS = (amd.ADD_INT8_LITERAL, amd.ADD_INT8_SPLIT, amd.ADD_INT8_SHIFT)


@pytest.mark.parametrize("name,q,variants", [
    ("B", R.SET_B, ALL_VARIANTS),                                    # a set where each of the three applies
    ("ratio 2^-12", RATIO_2_12, ALL_VARIANTS),
    ("A", R.SET_A, (amd.ADD_INT8_LITERAL, amd.ADD_INT8_SPLIT)),
    ("C", R.SET_C, (amd.ADD_INT8_LITERAL, amd.ADD_INT8_SPLIT)),
    ("equal scales", EQUAL_SCALES, (amd.ADD_INT8_LITERAL, amd.ADD_INT8_SHIFT)),
])
def test_every_variant_forced_gives_the_same_bytes(name, q, variants):
    for act in ACTS:
        for layout, x1, x2 in layouts():
            for v in variants:
                check(x1, x2, q, act, variant=v)


def test_the_chooser_falls_back_to_the_literal_variant():
    x1, x2 = R.all_pairs()
    for q in NO_CHEAP_FORM:
        assert amd.add_int8_params(q[0:2], q[2:4], q[4:6])["variant"] == amd.ADD_INT8_LITERAL
        check(x1, x2, q)
        for v in (amd.ADD_INT8_SPLIT, amd.ADD_INT8_SHIFT):
            with pytest.raises(amd.LceHipError, match="not proven"):
                run(x1, x2, q, variant=v)
    assert amd.add_int8_params(R.SET_A[0:2], R.SET_A[2:4], R.SET_A[4:6])["variant"] == amd.ADD_INT8_SPLIT


def rand_i8(shape, seed):
    return np.random.default_rng(seed).integers(-128, 128, shape, dtype=np.int8)


@pytest.mark.parametrize("C", [1, 31, 32, 33, 64, 96, 127, 256])
def test_channel_counts(C):
    x1, x2 = rand_i8((37, C), C), rand_i8((37, C), C + 1000)
    for q, act in ((R.SET_A, R.ACT_RELU), (R.SET_B, R.ACT_NONE)):
        want = check(x1, x2, q, act)
        only_bits = run(x1, x2, q, act, out=False, out_bits=True)
        assert only_bits[0] is None and np.array_equal(only_bits[1], O.bitpack(want, q[5]))
        only_int8 = run(x1, x2, q, act)
        assert only_int8[1] is None and np.array_equal(only_int8[0], want)


@pytest.mark.parametrize("rows", [1, 7, 1000, 256 * 56 * 56])
def test_rows_at_64_channels(rows):
    x1, x2 = rand_i8((rows, 64), rows), rand_i8((rows, 64), rows + 1)
    check(x1, x2, R.SET_A, R.ACT_NONE)
    if rows <= 1000:
        check(x1, x2, R.SET_C, R.ACT_RELU6)


def test_in_place_unaligned_stream_and_empty():
    C = 64
    x1, x2 = rand_i8((50, C), 1), rand_i8((50, C), 2)
    q = R.SET_A
    want = R.add_q(x1, x2, q)
    for alias in (0, 1):                                            # out aliases in1, then in2
        a, b = torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV)
        bits = torch.zeros((50, 2), dtype=torch.int32, device=DEV)
        amd.add_int8(a, b, **qkw(q), out=(a, b)[alias], out_bits=bits)
        assert np.array_equal((a, b)[alias].cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), O.bitpack(want, q[5]))
        assert np.array_equal((b, a)[alias].cpu().numpy(), (x2, x1)[alias])
    # base pointers off a 16-byte boundary: the row path, for a channel count the flat path would take
    for off1, off2, offo in ((1, 0, 0), (0, 3, 0), (0, 0, 5), (1, 2, 3)):
        def at(off, src=None):
            big = torch.zeros(50 * C + 16, dtype=torch.int8, device=DEV)
            v = big[off:off + 50 * C].view(50, C)
            if src is not None:
                v.copy_(torch.from_numpy(src))
            return v
        a, b, o = at(off1, x1), at(off2, x2), at(offo)
        assert a.data_ptr() % 16 == off1 and b.data_ptr() % 16 == off2 and o.data_ptr() % 16 == offo
        _, bits = amd.add_int8(a, b, **qkw(q), out=o, out_bits=True)
        assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(bits.cpu().numpy(), O.bitpack(want, q[5]))
        amd.add_int8(a, b, **qkw(q), out=a)                          # in place on a tensor that may be unaligned
        assert np.array_equal(a.cpu().numpy(), want)
    # a stream of its own
    s = torch.cuda.Stream()
    a, b = torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out, bits = amd.add_int8(a, b, **qkw(q, R.ACT_RELU), out_bits=True, stream=s.cuda_stream)
    s.synchronize()
    want_relu = R.add_q(x1, x2, q, R.ACT_RELU)
    assert np.array_equal(out.cpu().numpy(), want_relu) and np.array_equal(bits.cpu().numpy(), O.bitpack(want_relu, q[5]))
    e = torch.zeros((0, C), dtype=torch.int8, device=DEV)
    o, bb = amd.add_int8(e, e, **qkw(q), out_bits=True)
    assert o.shape == (0, C) and bb.shape == (0, 2)
    # NumPy in, NumPy out
    got, gbits = amd.add_int8(x1, x2, **qkw(q), out_bits=True)
    assert np.array_equal(got, want) and np.array_equal(gbits, O.bitpack(want, q[5]))


# ---- sections ---------------------------------------------------------------------------------------------------------
def default_mode(data, info, x):
    """The same file at the default partition: the sections between the ADDs on the GPU, each ADD in NumPy.  Returns every
    section's outputs (tensor index -> array) and the tensor after every layer."""
    it = mr.Interpreter(data, batch_size=x.shape[0])
    r, after, delivered, k, pending = x, [], {}, 0, None
    for li in info:
        if pending is None:                                          # (a layer without a shortcut does not end a section)
            pending = dict(zip(it.sections[k].outputs, it.run_section(k, [r])))
            delivered.update(pending)
            k += 1
        y = pending[li["y"]]
        if li["shortcut"]:
            r = R.add_q(y, r, li["q"], li["act"])
            pending = None
        else:
            r = y
        after.append(r)
    assert k == len(it.sections)
    return delivered, after


def expected_stats(info):
    """(launches, LceQuantize folded): one launch per shortcut; every sum but a last layer's feeds an LceQuantize."""
    return (sum(li["shortcut"] for li in info), sum(1 for k, li in enumerate(info) if li["shortcut"] and k + 1 < len(info)))


@pytest.mark.parametrize("batch", [3, 64])
def test_the_int8_body_runs_as_one_section(batch):
    data, xt, out, info = int8_body_model()
    x = rand_i8((batch, 56, 56, 64), batch)
    delivered, after = default_mode(data, info, x)
    it = mr.Interpreter(data, batch_size=batch, int8_add_sections=True)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert it.model.int8_add_stats() == expected_stats(info) == (5, 4)
    assert it.model.elementwise_stats() == (0, 0, 0)
    assert np.array_equal(got, after[-1])
    # every output of every default section: the same body cut after each layer delivers that layer's tensor, and the
    # convolution outputs the default sections hand to the host are the ADD's first input in both runs
    for n in range(1, len(info)):
        data_n, _, out_n, info_n = int8_body_model(INT8_BODY[:n])
        itn = mr.Interpreter(data_n, batch_size=batch, int8_add_sections=True)
        assert len(itn.sections) == 1
        (got_n,) = itn.run_section(0, [x])
        assert np.array_equal(got_n, after[n - 1]), n
        assert itn.model.int8_add_stats() == expected_stats(info_n), n
        if not info_n[-1]["shortcut"]:
            assert np.array_equal(got_n, delivered[info[n - 1]["y"]]), n
    assert np.array_equal(it.predict(x), after[-1])


def test_both_flags_together_on_the_int8_body():
    data, xt, out, info = int8_body_model(INT8_BODY[:3])
    model = mr.LceModel(data, int8_add_sections=True, elementwise_sections=True)
    x = rand_i8((3, 56, 56, 64), 5)
    _, after = default_mode(data, info, x)
    (got,) = mr.Interpreter(model, batch_size=3).run_section(0, [x])
    assert np.array_equal(got, after[-1])
    assert model.int8_add_stats() == (2, 2) and model.elementwise_stats() == (0, 0, 0)


def test_hip_graph_replay_gives_the_same_bytes():
    data, xt, out, info = int8_body_model()
    model = mr.LceModel(data, int8_add_sections=True)
    batch = 5
    xh = rand_i8((batch, 56, 56, 64), 11)
    x = torch.from_numpy(xh).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    eager = torch.empty(dims, dtype=torch.int8, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        model.run_section(0, batch, [x.data_ptr()], [eager.data_ptr()], s.cuda_stream)
        s.synchronize()
        model.use_hip_graphs(True)
        y = torch.empty_like(eager)
        for _ in range(3):                                           # eager, record + launch, replay
            y.zero_()
            model.run_section(0, batch, [x.data_ptr()], [y.data_ptr()], s.cuda_stream)
        s.synchronize()
    assert model.graph_stats()[0] == 1
    assert model.int8_add_stats() == expected_stats(info)
    assert np.array_equal(y.cpu().numpy(), eager.cpu().numpy())
    assert np.array_equal(eager.cpu().numpy(), default_mode(data, info, xh)[1][-1])
    model.use_hip_graphs(False)
