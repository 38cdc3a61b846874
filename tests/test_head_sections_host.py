"""The classifier head in the model reader, without a GPU: lce_tflite_model_open_passes (every subset of the eight earlier names
partitions as the options struct does, the refusals, "head" on files without a head), the three option readers, the candidate
rules one violation per file (each file placed so that it ENDS at an unreadable page: a read past an options table faults), the
Python constructor's route, and the sections and shapes of a QuickNet-shaped network."""
import ctypes as C
import importlib
import itertools
import mmap

import numpy as np
import pytest

import head_models as HM
import section_models as SM
import test_concat_sections_host as T_CONCAT
import test_conv1x1_sections_host as T_CONV1X1
import test_conv2d_sections_host as T_CONV2D
import test_depthwise_sections_host as T_DEPTHWISE
import test_int8_add_host as T_INT8
import test_pool_sections_host as T_POOL
from section_models import RELU, _conv, _sections_of
from tflite_writer import ModelBuilder

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

KEYWORDS = [keyword for keyword, _, _, _ in mr._SECTION_KEYWORDS]
NAMES = [mr._PASS_NAMES[k] for k in KEYWORDS]
# the fixtures of the earlier *_sections_host tests: none of them has a head
NO_HEAD = dict(small=SM.small_model, mixed=SM.mixed_model, body=lambda: SM.body_model(SM.BODY[:2]), dense=SM.dense_block_model,
               alexnet=SM.alexnet_body_model, bireal=SM.bireal_block_model, quicknet_transition=SM.quicknet_transition_model,
               int8_dense=T_CONCAT.int8_dense_model, int8_pool_body=T_POOL.int8_body_model, int8_add_body=T_INT8.int8_body_model,
               **{"conv1x1_" + k: v for k, v in T_CONV1X1.FIXTURES.items()}, **{"depthwise_" + k: v for k, v in T_DEPTHWISE.FIXTURES.items()},
               **{"conv2d_" + k: v for k, v in T_CONV2D.FIXTURES.items()})


def open_passes(data, passes, at_page_end=False):
    """lce_tflite_model_open_passes; `at_page_end`: on a copy of the file that ENDS at a page that cannot be read.  Returns
    (handle or None, message, what keeps the copy alive)."""
    lib = mr.tflite_lib()
    err = C.create_string_buffer(256)
    keep = data
    if at_page_end:
        page = mmap.PAGESIZE
        pages = -(-len(data) // page)
        m = mmap.mmap(-1, (pages + 1) * page)
        view = (C.c_char * ((pages + 1) * page)).from_buffer(m)
        base = C.addressof(view)
        libc = C.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        at = base + pages * page - len(data)
        C.memmove(at, data, len(data))
        assert libc.mprotect(base + pages * page, page, 0) == 0, C.get_errno()
        keep = (m, view, libc, base + pages * page, page)
        h = lib.lce_tflite_model_open_passes(C.cast(at, C.c_char_p), len(data), passes, err, 256)
    else:
        h = lib.lce_tflite_model_open_passes(data, len(data), passes, err, 256)
    return h, err.value, keep


def release(keep):
    if isinstance(keep, tuple):
        _, _, libc, guard, page = keep                               # (the mapping goes with its last reference)
        assert libc.mprotect(guard, page, mmap.PROT_READ | mmap.PROT_WRITE) == 0


def _parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


# ---- open_passes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["quicknet_head", "conv2d_quicknet", "dense"])
def test_every_subset_of_the_eight_names_partitions_as_the_keywords_do(fixture):
    data = HM.quicknet_head_model()[0] if fixture == "quicknet_head" else NO_HEAD[fixture]()[0]
    lib = mr.tflite_lib()
    seen = set()
    for mask in range(256):
        chosen = [k for k in range(8) if mask >> k & 1]
        want = _parts(mr.LceModel(data, **{KEYWORDS[k]: True for k in chosen}))
        for order in (chosen, chosen[::-1]):
            h, err, _ = open_passes(data, ",".join(NAMES[k] for k in order).encode())
            assert h, (mask, err)
            assert _sections_of(h) == want, mask
            lib.lce_tflite_model_close(h)
        seen.add(str(want))
    assert len(seen) > 2                                             # (the names do something on this file)
    h, _, _ = open_passes(data, b"")
    assert _sections_of(h) == _parts(mr.LceModel(data))              # "" is lce_tflite_model_open
    lib.lce_tflite_model_close(h)


def test_open_passes_refuses_what_it_does_not_know():
    data = HM.quicknet_head_model()[0]
    lib = mr.tflite_lib()
    err = C.create_string_buffer(256)
    assert not lib.lce_tflite_model_open_passes(data, len(data), None, err, 256) and b"null passes" in err.value
    assert not lib.lce_tflite_model_open_passes(data, len(data), None, None, 0)
    for passes, offender in ((b"heads", b"'heads'"), (b"pool,tail", b"'tail'"), (b"pool,,stem", b"''"), (b"pool,", b"''"), (b",", b"''"),
                             (b"pool, stem", b"' stem'"), (b"HEAD", b"'HEAD'"), (b"head,pool,head", b"'head'"), (b"stem,stem", b"'stem'"),
                             (b"elementwise,int8_add,concat,pool,conv1x1,depthwise,conv2d,stem,head,conv2d", b"'conv2d'")):
        h, msg, _ = open_passes(data, passes)
        assert not h and offender in msg, (passes, msg)
    h, msg, _ = open_passes(b"not a model", b"head")
    assert not h and msg
    assert not lib.lce_tflite_model_open_passes(None, 0, b"head", err, 256) and b"null buffer" in err.value


def test_no_other_entry_reaches_the_head():
    """Every flag of the options struct, and every keyword but head_sections, leaves the head with the host."""
    data, x, out, info = HM.quicknet_head_model()
    hi = info["head"]
    model = mr.LceModel(data, int8_add_sections=True, concat_sections=True, **HM.ALL_FLAGS)
    assert _parts(model) == [(list(range(hi["mean"])), [x], [info["body_out"]])] and not mr.Interpreter(model).lce_only
    h, _ = SM._open(data, np.array([56, 7, 31] + [0] * 11, np.uint32).tobytes())
    assert _sections_of(h) == _parts(model)
    mr.tflite_lib().lce_tflite_model_close(h)
    for ext in (32, 64, 128):                                        # (and the struct has no bit for it)
        h, err = SM._open(data, np.array([56, 7, ext] + [0] * 11, np.uint32).tobytes())
        assert not h and b"flags" in err


@pytest.mark.parametrize("name", sorted(NO_HEAD))
def test_head_changes_nothing_on_a_file_without_a_head(name):
    data = NO_HEAD[name]()[0]
    for flags in ({}, dict(elementwise_sections=True), dict(int8_add_sections=True, concat_sections=True, **HM.ALL_FLAGS)):
        without, with_head = mr.LceModel(data, **flags), mr.LceModel(data, head_sections=True, **flags)
        assert _parts(with_head) == _parts(without)
        assert mr.Interpreter(with_head).lce_only == mr.Interpreter(without).lce_only
        assert with_head.head_stats() == (0, 0, 0)


# ---- the option readers ------------------------------------------------------------------------------------------------------------
def _options(model, k):
    lib = mr.tflite_lib()
    keep, present, fc, beta = C.c_int32(-1), C.c_int32(-1), (C.c_int32 * 3)(), C.c_float(-1)
    assert lib.lce_tflite_model_operator_reducer(model._h, k, C.byref(keep)) == amd.OK
    assert lib.lce_tflite_model_operator_fully_connected(model._h, k, fc, C.byref(present)) == amd.OK
    got = dict(keep_dims=keep.value, fc=tuple(fc) if present.value else None)
    assert lib.lce_tflite_model_operator_softmax(model._h, k, C.byref(beta), C.byref(present)) == amd.OK
    got["beta"] = beta.value if present.value else None
    return got


def test_the_option_readers():
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, 4, 4, 8], "x")
    axis = b.tensor([2], np.int32, "axis", np.array([1, 2], np.int32))
    w = f32([3, 8], "w", np.ones((3, 8), np.float32))
    t = [f32([1, 8], "t%d" % i) for i in range(3)] + [f32([1, 3], "u%d" % i) for i in range(6)]
    ops = [HM.mean_op(b, [x, axis], [t[0]], keep_dims=True), HM.mean_op(b, [x, axis], [t[1]], keep_dims=False),
           HM.mean_op(b, [x, axis], [t[2]], options=False),
           HM.fc_op(b, [t[0], w], [t[3]], activation=3, weights_format=1, keep_num_dims=True), HM.fc_op(b, [t[0], w], [t[4]]),
           HM.fc_op(b, [t[0], w], [t[5]], options=False),
           HM.softmax_op(b, [t[3]], [t[6]], beta=0.25), HM.softmax_op(b, [t[3]], [t[7]], beta=float("nan")),
           HM.softmax_op(b, [t[3]], [t[8]], options=False)]
    b.inputs, b.outputs = [x], t[6:]
    data = b.finish()
    h, err, keep = open_passes(data, b"head", at_page_end=True)
    assert h, err
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    model = mr.LceModel(data)
    got = [_options(model, k) for k in ops]
    assert [g["keep_dims"] for g in got] == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert [g["fc"] for g in got] == [None, None, None, (3, 1, 1), (0, 0, 0), None, None, None, None]
    assert [g["beta"] for g in got[:6]] == [None] * 6 and got[6]["beta"] == 0.25 and np.isnan(got[7]["beta"]) and got[8]["beta"] is None
    lib = mr.tflite_lib()
    v = C.c_int32()
    for bad in (-1, len(ops)):
        assert lib.lce_tflite_model_operator_reducer(model._h, bad, C.byref(v)) == amd.ERR_INVALID
        assert lib.lce_tflite_model_operator_fully_connected(model._h, bad, (C.c_int32 * 3)(), C.byref(v)) == amd.ERR_INVALID
        assert lib.lce_tflite_model_operator_softmax(model._h, bad, C.byref(C.c_float()), C.byref(v)) == amd.ERR_INVALID
    assert lib.lce_tflite_model_operator_reducer(model._h, 0, None) == amd.ERR_INVALID


# ---- the candidates: one rule violated per file -----------------------------------------------------------------------------------------
VIOLATIONS = ("mean_axis_3", "mean_axis_without_data", "mean_axis_1_only", "mean_output_shape", "fc_weight_one_column_more",
              "fc_weights_format_1", "fc_no_options", "fc_int8_weights", "fc_weight_without_data", "fc_keep_num_dims_rank_4", "fc_tanh",
              "softmax_beta_0", "softmax_beta_nan", "softmax_no_options", "softmax_other_shape")


def violation_model(case):
    """x -> LceQuantize -> LceBconv2d -> y [1, 4, 4, 32] -> MEAN -> FULLY_CONNECTED (32 -> 6) -> SOFTMAX, with one condition of
    one candidate rule broken.  Returns (file, the index of the operator that must stay with the host, the three head operators)."""
    H, Cc, N = 4, 32, 6
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    x = f32([1, H, H, Cc], "x")
    q = b.tensor([1, H, H, 1], np.int32, "q")
    b.custom_op("LceQuantize", [x], [q], b"")
    y, _ = _conv(b, q, H, Cc, Cc, 3)
    g = np.random.default_rng(1)
    axis_values = {"mean_axis_3": [3], "mean_axis_1_only": [1]}.get(case, [1, -2])
    axis = b.tensor([len(axis_values)], np.int32, "axis", None if case == "mean_axis_without_data" else np.array(axis_values, np.int32))
    pooled_shape = {"mean_axis_3": [1, H, H], "mean_axis_1_only": [1, H, Cc], "mean_output_shape": [1, Cc + 1]}.get(case, [1, Cc])
    if case == "fc_keep_num_dims_rank_4":
        pooled_shape = [1, 1, 1, Cc]
    pooled = f32(pooled_shape, "pooled")
    k_mean = HM.mean_op(b, [y, axis], [pooled], keep_dims=case == "fc_keep_num_dims_rank_4")
    k_in = Cc + 1 if case == "fc_weight_one_column_more" else Cc
    wv = (g.standard_normal((N, k_in)) * 0.3).astype(np.float32)
    if case == "fc_int8_weights":
        w = b.tensor([N, k_in], np.int8, "w", np.ones((N, k_in), np.int8), scale=0.5, zero_point=0)
    else:
        w = f32([N, k_in], "w", None if case == "fc_weight_without_data" else wv)
    logits = f32([1, N], "logits")
    k_fc = HM.fc_op(b, [pooled, w, f32([N], "wb", np.zeros(N, np.float32))], [logits], activation=4 if case == "fc_tanh" else RELU,
                    weights_format=1 if case == "fc_weights_format_1" else 0, keep_num_dims=case == "fc_keep_num_dims_rank_4",
                    options=case != "fc_no_options")
    probs = f32([1, N + 1] if case == "softmax_other_shape" else [1, N], "probs")
    beta = {"softmax_beta_0": 0.0, "softmax_beta_nan": float("nan")}.get(case, 1.0)
    k_sm = HM.softmax_op(b, [logits], [probs], beta, options=case != "softmax_no_options")
    b.inputs, b.outputs = [x], [probs]
    stays = k_mean if case.startswith("mean") else k_fc if case.startswith("fc") else k_sm
    return b.finish(), stays, (k_mean, k_fc, k_sm)


@pytest.mark.parametrize("case", VIOLATIONS)
def test_a_violated_rule_leaves_the_operator_with_the_host(case):
    data, stays, head_ops = violation_model(case)
    h, err, keep = open_passes(data, b"elementwise,pool,conv1x1,depthwise,conv2d,stem,head", at_page_end=True)
    assert h, err
    sections = _sections_of(h)
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    taken = set(itertools.chain.from_iterable(ops for ops, _, _ in sections))
    assert stays not in taken and {0, 1} <= taken, (case, sections)
    model = mr.LceModel(data, head_sections=True, **HM.ALL_FLAGS)
    assert _parts(model) == sections and not mr.Interpreter(model).lce_only
    # the two other head operators still join when their own rules hold: as the body's section, or behind the host's operator
    # as a section of their own (rank-2 tensors and all) -- and the walk of every section gives every delivered tensor a shape
    others = [k for k in head_ops if k != stays]
    if case in ("fc_weights_format_1", "fc_no_options", "fc_tanh", "softmax_beta_0", "softmax_no_options"):
        assert set(others) <= taken, (case, sections)
    for k, (ops, ins, outs) in enumerate(sections):
        for t in ins + outs:
            dims, nbytes = model.section_tensor_shape(k, t, 3)
            assert dims[0] == 3 and nbytes > 0
            if len(model.tensors[t].shape) == 2:
                assert tuple(dims) == (3, 1, 1, model.tensors[t].shape[1])


def test_the_unbroken_file_is_one_section():
    data, _, head_ops = violation_model("none")
    model = mr.LceModel(data, head_sections=True)
    assert [s.ops for s in model.sections] == [[0, 1, 2, 3, 4]] and mr.Interpreter(model).lce_only


# ---- the Python constructor ---------------------------------------------------------------------------------------------------------------
def test_the_constructor_goes_through_open_passes_only_with_head_sections(monkeypatch):
    data = HM.quicknet_head_model()[0]
    lib = mr.tflite_lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("lce_tflite_model_open"):
                def spy(*a):
                    calls.append((name, a[2] if isinstance(a[2], (bytes, int)) else C.cast(a[2], C.POINTER(C.c_uint32))[0]))
                    return getattr(lib, name)(*a)
                return spy
            return getattr(lib, name)
    monkeypatch.setattr(mr, "tflite_lib", lambda: Spy())
    mr.LceModel(data)
    mr.LceModel(data, elementwise_sections=True)
    mr.LceModel(data, concat_sections=True)
    mr.LceModel(data, **HM.ALL_FLAGS)
    mr.LceModel(data, head_sections=False, stem_sections=True)
    mr.LceModel(data, head_sections=True)
    mr.LceModel(data, head_sections=True, stem_sections=True, elementwise_sections=True)
    mr.Interpreter(data, **HM.EVERY_FLAG)
    assert calls == [("lce_tflite_model_open_ex", 0), ("lce_tflite_model_open_ex", 1), ("lce_tflite_model_open_opts", 8),
                     ("lce_tflite_model_open_opts", 56), ("lce_tflite_model_open_opts", 56), ("lce_tflite_model_open_passes", b"head"),
                     ("lce_tflite_model_open_passes", b"elementwise,stem,head"),
                     ("lce_tflite_model_open_passes", b"elementwise,pool,conv1x1,depthwise,conv2d,stem,head")]


# ---- sections and shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_dims", [False, True])
def test_a_quicknet_shaped_network_is_one_section_from_the_image_to_the_probabilities(keep_dims):
    data, x, out, info = HM.quicknet_head_model(keep_dims=keep_dims)
    hi = info["head"]
    model = mr.LceModel(data, **HM.EVERY_FLAG)
    n_ops = len(model.operators)
    assert [model.operators[k].builtin_code for k in (hi["mean"], hi["fc"], hi["softmax"])] == [HM.MEAN, HM.FULLY_CONNECTED, HM.SOFTMAX]
    assert _parts(model) == [(list(range(n_ops)), [x], [out])] and model.inputs == [x] and model.outputs == [out]
    it = mr.Interpreter(data, **HM.EVERY_FLAG)
    assert it.lce_only and mr.Interpreter(model).lce_only and it.output_shapes == [(1, info["classes"])]
    for batch in (1, 5):
        assert model.section_tensor_shape(0, hi["tensors"]["pooled"], batch) == ((batch, 1, 1, 64), batch * 64 * 4)
        assert model.section_tensor_shape(0, hi["tensors"]["logits"], batch) == ((batch, 1, 1, 10), batch * 40)
        assert model.section_tensor_shape(0, out, batch) == ((batch, 1, 1, 10), batch * 40)
        assert model.section_tensor_shape(0, x, batch)[0] == (batch, 8, 8, 3)
    assert model.head_stats() == (0, 0, 0)
    mr.tflite_lib().lce_tflite_model_head_stats(model._h, None, None, None)      # any pointer may be NULL
    mr.tflite_lib().lce_tflite_model_head_stats(None, None, None, None)
    # without the stem flags the stem is the host's and body and head are the section; head alone: the head joins the last layer's
    part = mr.LceModel(data, head_sections=True, elementwise_sections=True)
    assert [s.ops for s in part.sections] == [list(range(1, n_ops))] and not mr.Interpreter(part).lce_only


def test_a_head_behind_an_operator_of_the_host_is_a_section_of_its_own():
    data, x, out, info = HM.head_only_model()
    hi = info["head"]
    model = mr.LceModel(data, **HM.EVERY_FLAG)
    assert _parts(model) == [([hi["mean"], hi["fc"], hi["softmax"]], [info["t"]], [out])]
    assert not mr.Interpreter(model).lce_only
    assert model.section_tensor_shape(0, info["t"], 2)[0] == (2, 5, 5, 40) and model.section_tensor_shape(0, out, 2)[0] == (2, 1, 1, 7)
    assert [s.ops for s in mr.LceModel(data, **HM.ALL_FLAGS).sections] == []


# ---- the tables of model_runner.py against the library -------------------------------------------------------------------------------
def test_every_row_of_the_python_tables_is_one_the_library_knows():
    """_PASSES (keyword, name) and _PASS_STATS (export, counters) from the outside: the library accepts each name alone, the keyword
    sets its own attribute and no other, an unknown keyword is a TypeError, and every *_stats method reports as many zeros as the
    table says on a model that has not run."""
    data = SM.small_model()[0]
    lib = mr.tflite_lib()
    keywords = [row[0] for row in mr._PASSES]
    assert len(mr._PASSES) == 18 and len(set(keywords)) == 18 and len({row[1] for row in mr._PASSES}) == 18
    assert keywords == [k for k, _, _, _ in mr._SECTION_KEYWORDS] + list(mr._NAMED_ONLY) == list(mr._PASS_NAMES)
    for keyword, name, word, bit, form in mr._PASSES:
        assert (word is None) == (bit is None) == (form is None) == (keyword in mr._NAMED_ONLY), keyword
        assert keyword == name + "_sections" and mr._PASS_NAMES[keyword] == name
        h, err, _ = open_passes(data, name.encode())
        assert h, (name, err)
        lib.lce_tflite_model_close(h)
        model = mr.LceModel(data, **{keyword: True})
        assert [k for k in keywords if getattr(model, k)] == [keyword]
        assert all(getattr(model, k) is False for k in keywords if k != keyword) and getattr(model, keyword) is True
        assert mr.Interpreter(data, **{keyword: True}).model.__dict__[keyword] is True
    for constructor in (mr.LceModel, mr.Interpreter):
        for unknown in ("tail_sections", "head", "elementwise_section"):
            with pytest.raises(TypeError, match=unknown):
                constructor(data, **{unknown: True})
            with pytest.raises(TypeError, match=unknown):
                constructor(data, head_sections=True, **{unknown: False})
    with pytest.raises(TypeError, match="tail_sections"):
        mr.Interpreter(mr.LceModel(data), tail_sections=True)            # (checked even where a ready model makes it moot)
    assert len(mr._PASS_STATS) == 17
    model = mr.LceModel(data)
    for name, counters in mr._PASS_STATS.items():
        assert hasattr(lib, "lce_tflite_model_%s_stats" % name), name
        assert getattr(model, name + "_stats")() == (0,) * counters, name
        assert getattr(mr.LceModel, name + "_stats").__doc__, name
