"""The binarized Dense layer without a GPU: lce_hip_bfc_prepare and lce_hip_bfc_check (accepted rows, every refusal), the real
kernel body of csrc/lce_kernels_bfc.h on the host simulation against the NumPy restatement (tests/binary_dense_ref.py) byte for
byte, and the model reader: the "binary_dense" name of lce_tflite_model_open_passes, its priority over "head", the sections and
launch-free shape walks of the fixture networks (tests/binary_dense_models.py), and the refusals that fall back to "head"."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import binary_dense_models as BM
import binary_dense_ref as R
import hostsim_binary_dense_lib as S
from test_head_sections_host import open_passes

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

BATCHES = (1, 31, 33, 65)
KS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 288)        # (128: four whole words, the 16-byte load path)
NS = (1, 31, 32, 33, 100)
OUTPUTS = ((True, True), (True, False), (False, True))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- prepare and check ------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_three_entries():
    lib = amd.lib()
    for name in ("lce_hip_bfc_check", "lce_hip_bfc_prepare", "lce_hip_binary_fully_connected"):
        assert hasattr(lib, name) and name in amd.ABI_SYMBOLS
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_binary_dense_stats")
    assert lib.lce_hip_abi_version() == 3


@pytest.mark.parametrize("k", (1, 31, 32, 33, 64, 70, 288))
def test_prepare_gives_the_bits_and_scales(k):
    g = np.random.default_rng(k)
    n = 9
    sign = g.integers(0, 2, (n, k)).astype(bool)
    s = np.concatenate([g.uniform(1e-3, 50, n - 4), [2.0 ** -100, 2.0 ** 100, 1.0, np.float32(1e-20)]]).astype(np.float32)
    w = np.where(sign, -s[:, None], s[:, None]).astype(np.float32)
    bits, scale = amd.bfc_prepare(w)
    assert bits.dtype == np.int32 and bits.shape == (n, (k + 31) // 32) and scale.dtype == np.float32
    assert np.array_equal(bits, R.pack_signs(sign)) and np.array_equal(_bits(scale), _bits(s))
    want = R.prepare(w)
    assert np.array_equal(bits, want[0]) and np.array_equal(_bits(scale), _bits(want[1]))
    # the padding bits of a ragged last word are 0
    if k % 32:
        assert not np.any(bits.view(np.uint32)[:, -1] >> np.uint32(k % 32))
    # all negative: every channel bit set, the padding still 0
    allneg, _ = amd.bfc_prepare(-np.abs(w))
    assert np.array_equal(R.unpack_signs(allneg, k), -np.ones((n, k), np.int64))
    assert np.array_equal(allneg, R.pack_signs(np.ones((n, k), bool)))


def _refused(w):
    assert R.prepare(w) is None
    with pytest.raises(amd.LceHipError) as e:
        amd.bfc_prepare(w)
    assert e.value.code == amd.ERR_UNSUPPORTED, e.value
    return e.value.message


def test_prepare_refuses_what_is_not_plus_minus_s():
    g = np.random.default_rng(5)
    base = np.where(g.integers(0, 2, (6, 70)).astype(bool), np.float32(-0.37), np.float32(0.37)).astype(np.float32)
    amd.bfc_prepare(base)
    one_ulp = (np.nextafter(np.float32(0.37), np.float32(1)), np.nextafter(np.float32(0.37), np.float32(0)))
    for value in one_ulp + (-one_ulp[0], 0.0, -0.0, np.nan, np.inf, -np.inf):
        for at in ((0, 0), (3, 0), (3, 41), (5, 69)):
            w = base.copy()
            w[at] = value
            assert "output %d" % at[0] in _refused(w)
    # a scale outside [2^-100, 2^100], and the subnormals
    for s in (np.float32(2.0 ** -101), np.nextafter(np.float32(2.0 ** -100), np.float32(0)), np.nextafter(np.float32(2.0 ** 100), np.float32(np.inf)),
              np.float32(2.0 ** 101), np.float32(1e-45), np.float32(np.inf), np.float32(np.nan)):
        w = base.copy()
        w[2] = np.where(w[2] < 0, -s, s)
        _refused(w)
    # rows may differ from each other
    w = base.copy()
    w[4] *= np.float32(3)
    amd.bfc_prepare(w)


def test_prepare_and_check_refuse_too_many_inputs():
    lib = amd.lib()
    ok = amd.BfcDesc(1, (1 << 23) - 1, 1, amd.ACT_NONE)
    assert lib.lce_hip_bfc_check(C.byref(ok)) == amd.OK
    d = amd.BfcDesc(1, 1 << 23, 1, amd.ACT_NONE)
    assert lib.lce_hip_bfc_check(C.byref(d)) == amd.ERR_UNSUPPORTED
    w = np.ones((1, 1 << 23), np.float32)
    assert R.prepare(w) is None
    with pytest.raises(amd.LceHipError) as e:
        amd.bfc_prepare(w)
    assert e.value.code == amd.ERR_UNSUPPORTED and "2^23" in e.value.message
    w = np.ones((1, (1 << 23) - 1), np.float32)
    bits, scale = amd.bfc_prepare(w)
    assert not bits.any() and scale[0] == 1


def test_check_and_the_entry_refuse_bad_arguments_before_any_device_call():
    lib = amd.lib()
    assert lib.lce_hip_bfc_check(None) == amd.ERR_INVALID
    for bad in ((0, 4, 4, 0), (4, 0, 4, 0), (4, 4, 0, 0), (-1, 4, 4, 0), (4, 4, 4, 4), (4, 4, 4, -1)):
        d = amd.BfcDesc(*bad)
        assert lib.lce_hip_bfc_check(C.byref(d)) == amd.ERR_INVALID, bad
    d = amd.BfcDesc(1 << 30, 4, 1 << 30, 0)
    assert lib.lce_hip_bfc_check(C.byref(d)) == amd.ERR_UNSUPPORTED
    d = amd.BfcDesc(2, 64, 40, 0)
    w = np.ones((40, 64), np.float32)
    bits, scale = np.zeros((40, 2), np.int32), np.zeros(40, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, vp(w), vp(bits), vp(scale)), (C.byref(d), None, vp(bits), vp(scale)), (C.byref(d), vp(w), None, vp(scale)),
                 (C.byref(d), vp(w), vp(bits), None)):
        assert lib.lce_hip_bfc_prepare(*args) == amd.ERR_INVALID
    # the run entry: pointers are judged as numbers, nothing is dereferenced and no device is asked for
    run = lib.lce_hip_binary_fully_connected
    a, wb, sc, bi, out, ob = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    p = C.c_void_p
    cases = {"null desc": (None, p(a), p(wb), p(sc), p(bi), p(out), p(ob)),
             "null input": (C.byref(d), None, p(wb), p(sc), p(bi), p(out), p(ob)),
             "null filter": (C.byref(d), p(a), None, p(sc), p(bi), p(out), p(ob)),
             "null scale": (C.byref(d), p(a), p(wb), None, p(bi), p(out), p(ob)),
             "both outputs are null": (C.byref(d), p(a), p(wb), p(sc), p(bi), None, None),
             "overlaps the input": (C.byref(d), p(a), p(wb), p(sc), p(bi), p(a + 8), p(ob)),
             "overlaps the filter": (C.byref(d), p(a), p(wb), p(sc), p(bi), p(out), p(wb + 4)),
             "overlaps the scale": (C.byref(d), p(a), p(wb), p(sc), p(bi), p(sc + 4), p(ob)),
             "overlaps the bias": (C.byref(d), p(a), p(wb), p(sc), p(bi), p(out), p(bi)),
             "two outputs overlap": (C.byref(d), p(a), p(wb), p(sc), p(bi), p(out), p(out + 16)),
             "4-byte aligned": (C.byref(d), p(a), p(wb), p(sc + 2), p(bi), p(out), p(ob))}
    for what, args in cases.items():
        assert run(*args, None) == amd.ERR_INVALID, what
        assert what in lib.lce_hip_last_error().decode(), (what, lib.lce_hip_last_error())
    bad = amd.BfcDesc(2, 64, 40, 7)
    assert run(C.byref(bad), p(a), p(wb), p(sc), p(bi), p(out), p(ob), None) == amd.ERR_INVALID


# ---- the kernel body on the host simulation ----------------------------------------------------------------------------------------
def _operands(m, k, n, seed):
    """Activation and weight bits with all-equal rows (|t| = K) among random ones, scales (one a power of two), and biases that
    make v exactly 0 (a bias of -p), keep a zero sum zero (a bias of -0.0), and a NaN."""
    g = np.random.default_rng(seed)
    a_neg, w_neg = g.integers(0, 2, (m, k)).astype(bool), g.integers(0, 2, (n, k)).astype(bool)
    a_neg[0] = False
    w_neg[0] = False                                           # t[0][0] = +K
    if n > 1:
        w_neg[1] = True                                        # t[0][1] = -K
    if m > 1:
        a_neg[1] = True
    if n > 2 and k >= 2:
        w_neg[2] = np.arange(k) % 2 == 1                       # against the all-equal rows: t = 0 (even K) or +-1
    s = g.uniform(0.01, 3, n).astype(np.float32)
    s[0] = np.float32(0.5)
    a, w = R.pack_signs(a_neg), R.pack_signs(w_neg)
    t = R.dot(a, w, k)
    bias = g.standard_normal(n).astype(np.float32)
    bias[0] = -(np.float32(k) * s[0])                          # row 0: p + bias = +0.0 exactly
    if n > 1:
        bias[1] = np.float32(k) * s[1]                         # row 0, column 1: -K s + K s
    if n > 2:
        bias[2] = np.float32(-0.0)
    if n > 3:
        bias[3] = np.float32(np.nan)
    assert abs(t[0, 0]) == k
    return a, w, s, bias, t


@pytest.mark.parametrize("m", BATCHES)
def test_the_simulated_kernel_equals_the_restatement(m):
    seen_zero = seen_nan = seen_vec = seen_rows = 0
    for k, n in itertools.product(KS, NS):
        a, w, s, bias, t = _operands(m, k, n, 1000 * m + 10 * k + n)
        for with_bias, act in itertools.product((True, False), R.ACTIVATIONS):
            b = bias if with_bias else None
            want_v, want_bits = R.binary_fully_connected(a, w, s, b, k, act)
            if with_bias and act == R.NONE:
                assert want_v[0, 0] == 0 and not np.signbit(want_v[0, 0])
                seen_zero += int(np.sum(want_v == 0))
                seen_nan += int(np.isnan(want_v).sum())
            for (value, bits), cap in itertools.product(OUTPUTS, (1, 1 << 20)):
                v, ob, vec = S.sim(a, w, s, b, k, act, value=value, bits=bits, cap=cap)
                seen_vec += vec
                seen_rows += 1
                if value:
                    assert np.array_equal(_bits(v), _bits(want_v)), (m, k, n, with_bias, act, cap)
                if bits:
                    assert np.array_equal(ob, want_bits), (m, k, n, with_bias, act, cap)
    assert seen_zero and seen_vec and seen_rows == len(KS) * len(NS) * 2 * 4 * 3 * 2
    assert seen_nan


def test_the_scalar_load_path_gives_the_same_bytes():
    """Operands 4 bytes behind a 16-byte boundary take the 4-byte loads even where K allows the wide ones."""
    for m, k, n in ((33, 128, 33), (2, 512, 40), (65, 288, 31)):
        a, w, s, bias, _ = _operands(m, k, n, 77 + k)
        want_v, want_bits = R.binary_fully_connected(a, w, s, bias, k, R.RELU6)
        took = []
        for offset in (0, 4):
            v, ob, vec = S.sim(a, w, s, bias, k, R.RELU6, cap=2, offset=offset)
            took.append(vec)
            assert np.array_equal(_bits(v), _bits(want_v)) and np.array_equal(ob, want_bits)
        assert took == [(k + 31) // 32 % 4 == 0, False]


def test_negative_zero_and_nan_give_bit_zero():
    """The bit rule is v < 0: a NaN bias gives NaN values and 0 bits, a sum of zero times a scale is +0.0, and a bias of -0.0
    under it leaves +0.0."""
    k, n = 64, 33
    a = R.pack_signs(np.zeros((2, k), bool))
    w_neg = np.zeros((n, k), bool)
    w_neg[:, ::2] = True                                       # every t = 0
    w = R.pack_signs(w_neg)
    s = np.full(n, 0.75, np.float32)
    for bias in (None, np.full(n, -0.0, np.float32)):
        v, ob, _ = S.sim(a, w, s, bias, k)
        assert np.array_equal(_bits(v), np.zeros((2, n), np.int32)) and not ob.any()
    v, ob, _ = S.sim(a, w, s, np.full(n, np.nan, np.float32), k, R.RELU)
    assert np.isnan(v).all() and not ob.any()
    # every value negative: all N bits set, the padding bits of the ragged last word 0
    v, ob, _ = S.sim(a, R.pack_signs(np.ones((n, k), bool)), s, None, k)
    assert (v == -48).all() and np.array_equal(ob.view(np.uint32), np.tile(np.array([0xFFFFFFFF, 1], np.uint32), (2, 1)))


@pytest.mark.parametrize("signs", ("equal", "random"))
def test_a_long_sum_is_exact(signs):
    m, k, n = 2, 9216, 33
    g = np.random.default_rng(9)
    a_neg, w_neg = g.integers(0, 2, (m, k)).astype(bool), g.integers(0, 2, (n, k)).astype(bool)
    if signs == "equal":
        a_neg[:] = False
        a_neg[1] = True
        w_neg[:] = False
        w_neg[1::2] = True
    a, w = R.pack_signs(a_neg), R.pack_signs(w_neg)
    s, bias = g.uniform(0.01, 3, n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    t = R.dot(a, w, k)
    assert signs == "random" or (np.abs(t) == k).all()
    for cap in (1, 1 << 20):
        v, ob, vec = S.sim(a, w, s, bias, k, cap=cap)
        want_v, want_bits = R.binary_fully_connected(a, w, s, bias, k)
        assert vec and np.array_equal(_bits(v), _bits(want_v)) and np.array_equal(ob, want_bits)
    v, _, _ = S.sim(a, w, np.ones(n, np.float32), None, k)
    assert np.array_equal(v.astype(np.int64), t)


def test_one_very_long_row_is_exact():
    k = 70001
    g = np.random.default_rng(10)
    a_neg = g.integers(0, 2, (1, k)).astype(bool)
    for w_neg, want in ((a_neg, k), (~a_neg, -k), (g.integers(0, 2, (1, k)).astype(bool), None)):
        a, w = R.pack_signs(a_neg), R.pack_signs(w_neg)
        v, ob, _ = S.sim(a, w, np.ones(1, np.float32), None, k)
        t = int(R.dot(a, w, k)[0, 0])
        assert want is None or t == want
        assert v[0, 0] == t and ob[0, 0] == int(t < 0)


# ---- the reader and the partition --------------------------------------------------------------------------------------------------
FIXTURES = dict(alexnet_tail=BM.alexnet_tail_model, body_tail=BM.body_tail_model, second_reader=BM.second_reader_model,
                value_and_bits=BM.value_and_bits_model, shared_reader=BM.shared_reader_model)


def _kinds(data, **keywords):
    """Per operator: the index of the section that holds it, or None."""
    m = mr.LceModel(data, **keywords)
    where = {}
    for k, s in enumerate(m.sections):
        for i in s.ops:
            where[i] = k
    return m, [where.get(i) for i in range(len(m.operators))]


def test_open_passes_knows_the_name_and_still_refuses_the_others():
    data = BM.alexnet_tail_model()[0]
    lib = mr.tflite_lib()
    h, msg, _ = open_passes(data, b"binary_dense")
    assert h, msg
    lib.lce_tflite_model_close(h)
    for passes, offender in ((b"binary_dense,binary_dense", b"'binary_dense' is named twice"), (b"head,binary_dense,head", b"'head' is named twice"),
                             (b"binary-dense", b"unknown name 'binary-dense'"), (b"binary_dense,", b"unknown name ''"),
                             (b"binary_dense,dense", b"unknown name 'dense'"), (b"Binary_dense", b"unknown name 'Binary_dense'")):
        h, msg, _ = open_passes(data, passes)
        assert not h and offender in msg, (passes, msg)
    assert mr._PASS_NAMES["binary_dense_sections"] == "binary_dense" and "binary_dense_sections" in mr._NAMED_ONLY


@pytest.mark.parametrize("fixture", sorted(FIXTURES))
def test_without_the_name_nothing_changes(fixture):
    """`head` alone takes every Dense layer as a float FULLY_CONNECTED, as before; the name alone moves only the binary ones."""
    data = FIXTURES[fixture]()[0]
    parts = lambda m: [(s.ops, s.inputs, s.outputs) for s in m.sections]
    assert parts(mr.LceModel(data)) == parts(mr.LceModel(data, elementwise_sections=True))
    m_head = mr.LceModel(data, head_sections=True, reshape_sections=True, stem_sections=True)
    m_both = mr.LceModel(data, binary_dense_sections=True, head_sections=True, reshape_sections=True, stem_sections=True)
    assert parts(m_head) == parts(m_both)                      # the same operators join; only who runs them differs


@pytest.mark.parametrize("fixture", ("alexnet_tail", "body_tail"))
@pytest.mark.parametrize("head", (False, True))
def test_a_full_tail_is_one_section(fixture, head):
    data, x, outs, info = FIXTURES[fixture]()
    keywords = dict(BM.KEYWORDS_HEAD if head else BM.KEYWORDS, stem_sections=True)
    m, where = _kinds(data, **keywords)
    n_ops = len(m.operators)
    # without `head` the SOFTMAX is the host's; everything else is one section
    assert len(m.sections) == 1
    assert where == [0] * (n_ops - 1) + [0 if head else None]
    assert m.sections[0].inputs == [x]
    assert m.sections[0].outputs == (outs if head else [info["logits"]])
    # launch-free shape walk: every tensor the section delivers, rank 2 carried as [b, 1, 1, C]
    for batch in (1, 5):
        for t in m.sections[0].outputs:
            dims, nbytes = m.section_tensor_shape(0, t, batch)
            assert tuple(dims) == (batch, 1, 1, 10) and nbytes == batch * 10 * 4
        # a skipped dequantize still has a shape, and so have the bits a Dense layer leaves
        for L in info["layers"]:
            assert tuple(m.section_tensor_shape(0, L["sign"], batch)[0]) == (batch, 1, 1, L["k"])
            assert tuple(m.section_tensor_shape(0, L["bits"], batch)[0]) == (batch, 1, 1, (L["k"] + 31) // 32)
            assert tuple(m.section_tensor_shape(0, L["out"], batch)[0]) == (batch, 1, 1, L["n"])
    ip = mr.Interpreter(m, batch_size=4)
    assert ip.lce_only == head


def test_a_refused_layer_is_left_to_head_and_to_nobody_without_it():
    """The row's place in front of `head`'s shows where a layer is refused: with both names the refused Dense layer joins a
    section (as `head`'s), with `binary_dense` alone nobody takes it.  Which of the two rows runs a layer BOTH accept is not
    visible without a launch: the GPU suite asserts it through binary_dense_stats() and head_stats()."""
    data, x, out, info = BM.refusal_model("mixed_magnitudes")
    m, where = _kinds(data, **BM.KEYWORDS_HEAD)
    assert where[info["fc"]] == 0 and len(m.sections) == 1
    m2, where2 = _kinds(data, **BM.KEYWORDS)
    assert where2[info["fc"]] is None                         # nobody else takes it


def test_two_readers_of_one_dequantize_in_one_section():
    """A `binary_dense` layer and a `head` FULLY_CONNECTED (mixed magnitudes) read the same dequantized tensor: one section with
    both names; with `binary_dense` alone the refused layer is the host's and the section delivers the floats to it."""
    data, x, outs, info = BM.shared_reader_model()
    m, where = _kinds(data, **BM.KEYWORDS_HEAD)
    assert where == [0, 0, 0, 0] and m.sections[0].inputs == [x] and m.sections[0].outputs == outs
    for t, c in ((info["sign"], info["k"]), (outs[0], info["n"]), (outs[1], info["n2"])):
        assert tuple(m.section_tensor_shape(0, t, 3)[0]) == (3, 1, 1, c)
    m, where = _kinds(data, **BM.KEYWORDS)
    assert where == [0, 0, 0, None] and m.sections[0].outputs == [info["sign"], outs[0]]


@pytest.mark.parametrize("case", BM.REFUSALS)
def test_what_the_predicate_refuses_falls_back_to_head(case):
    data, x, out, info = BM.refusal_model(case)
    _, alone = _kinds(data, **BM.KEYWORDS)
    assert alone[info["fc"]] is None, case                    # `binary_dense` does not take it ...
    m, both = _kinds(data, **BM.KEYWORDS_HEAD)
    _, head = _kinds(data, head_sections=True, reshape_sections=True)
    assert both == head                                        # ... and the partition is `head`'s own
    assert (both[info["fc"]] is not None) == info["head"], case
    if info["head"]:
        k = both[info["fc"]]
        dims, _ = m.section_tensor_shape(k, out, 3)
        assert tuple(dims) == (3, 1, 1, 10)


def test_a_dequantize_with_a_second_reader_and_a_delivered_value_keep_their_tensors():
    data, x, outs, info = BM.second_reader_model()
    m = mr.LceModel(data, **BM.KEYWORDS)
    assert [(s.ops, s.inputs, s.outputs) for s in m.sections] == [([info["quantize"], info["dequantize"], info["fc"]], [info["t"]], [info["sign"], outs[0]])]
    assert tuple(m.section_tensor_shape(0, info["sign"], 7)[0]) == (7, 1, 1, info["k"])
    assert tuple(m.section_tensor_shape(0, outs[0], 7)[0]) == (7, 1, 1, info["n"])
    data, x, outs, info = BM.value_and_bits_model()
    m = mr.LceModel(data, **BM.KEYWORDS)
    assert len(m.sections) == 1 and m.sections[0].outputs == outs and m.sections[0].inputs == [info["t"]]
    for t, L in zip(outs, info["layers"]):
        assert tuple(m.section_tensor_shape(0, t, 2)[0]) == (2, 1, 1, L["n"])


def test_a_rank_2_lcedequantize_walks():
    """LceQuantize -> LceDequantize on rank-2 tensors (the sign behind a flatten), carried as [b, 1, 1, C]: the walk registers both
    shapes, with the name alone."""
    data, x, outs, info = BM.second_reader_model()
    m = mr.LceModel(data, binary_dense_sections=True)
    assert m.sections[0].ops[:2] == [info["quantize"], info["dequantize"]]
    assert tuple(m.section_tensor_shape(0, info["bits"], 3)[0]) == (3, 1, 1, 3)
    dims, nbytes = m.section_tensor_shape(0, info["sign"], 3)
    assert tuple(dims) == (3, 1, 1, 70) and nbytes == 3 * 70 * 4
