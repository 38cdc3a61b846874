"""The `slice` pass of lce_tflite_model_open_passes without a GPU: the reader's StridedSliceOptions, the predicate and every
refusal, the window resolution against Python's own slicing, the partition with and without the name, the walker's shapes, the
names, the keyword, the stats and the exported symbols."""
import ctypes as C
import importlib

import numpy as np
import pytest

import slice_models as SM
from section_models import _sections_of
from test_head_sections_host import NO_HEAD, open_passes, release
from tflite_writer import ModelBuilder, _Vector

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

EVERY_OLD_NAME = [name for _, name, _, _, _ in mr._PASSES if name != "slice"]


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
def test_the_meliusnet_fixture_is_what_the_checks_need():
    data, net, out = SM.meliusnet_model()
    model = mr.LceModel(data)
    codes = [model.operators[k].builtin_code for k in net.ops_of("slice")]
    assert codes == [SM.STRIDED_SLICE] * 4 and len(net.ops_of("improve_add")) == 2 and len(net.ops_of("dense_join")) == 2
    joined = [net.run[k][1] for k in net.ops_of("dense_join", "improve_join")]
    assert [model.tensors[t].shape[3] for t in joined] == [128, 128, 192, 192] and model.tensors[net.x0].shape == (1, 8, 8, 64)
    x = np.random.default_rng(0).standard_normal((2, 8, 8, 64)).astype(np.float32)
    live = net.forward(x)
    assert live[out].shape == (2, 8, 8, 192) and np.isfinite(live[out]).all()
    # the improvement block changes the last 64 channels and nothing else
    for k in net.ops_of("improve_join"):
        ins, y, _ = net.run[k]
        src = net.run[net.ops_of("slice")[0]][0][0] if k == net.ops_of("improve_join")[0] else net.run[net.ops_of("slice")[2]][0][0]
        c = live[src].shape[-1]
        assert np.array_equal(live[y][..., :c - 64], live[src][..., :c - 64]) and not np.array_equal(live[y][..., c - 64:], live[src][..., c - 64:])


def test_window_resolution_is_pythons_slicing():
    """Every (begin, end, masks) over an axis of 6 channels: the slice qualifies exactly when Python's x[begin:end] is not empty,
    and its output is as wide.  (Where the window begins is what the GPU tests' bytes pin.)"""
    C_, seen = 6, set()
    for begin in range(-8, 9):
        for end in range(-8, 9):
            for bm, em in ((0, 0), (8, 0), (0, 8), (8, 8)):
                at, count = SM.resolve(C_, begin, end, bm != 0, em != 0)
                b = ModelBuilder()
                x = b.tensor([1, 2, 2, C_], np.float32, "x")
                y = b.tensor([1, 2, 2, max(count, 1)], np.float32, "y")
                i32 = lambda name, v: b.tensor([4], np.int32, name, np.array(v, np.int32))
                k = SM.strided_slice_op(b, [x, i32("b", [0, 0, 0, begin]), i32("e", [1, 2, 2, end]), i32("s", [1, 1, 1, 1])], [y], bm, em)
                bits = b.tensor([1, 2, 2, 1], np.int32, "bits")
                b.custom_op("LceQuantize", [y], [bits], b"")
                b.inputs, b.outputs = [x], [bits]
                model = mr.LceModel(b.finish(), stem_sections=True, slice_sections=True)
                assert [s.ops for s in model.sections] == ([[k, k + 1]] if count else [[k + 1]]), (begin, end, bm, em)
                if count:
                    assert model.section_tensor_shape(0, y, 3)[0] == (3, 2, 2, count)
                seen.add(count)
    assert seen == set(range(C_ + 1))
    assert SM.resolve(96, -32, 0, False, True) == (64, 32) and SM.resolve(96, -500, 500) == (0, 96) and SM.resolve(96, 64, 64) == (0, 0)


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
def test_the_two_builtin_codes_round_trip():
    for case, code, n in (("masked", 45, 4), ("slice", 65, 3)):
        data, k, _ = SM.single_op_model(case)
        op = mr.LceModel(data).operators[k]
        assert op.builtin_code == code and len(op.inputs) == n and len(op.outputs) == 1


# ---- the predicate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SM.REFUSALS)
def test_each_refusal_stays_with_the_host(case):
    data, k, _ = SM.single_op_model(case)
    h, err, keep = open_passes(data, ",".join(EVERY_OLD_NAME + ["slice"]).encode(), at_page_end=True)
    assert h, err
    secs = _sections_of(h)
    assert all(k not in ops for ops, _, _ in secs) and [ops for ops, _, _ in secs] == [[k + 1]], case
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)


@pytest.mark.parametrize("case", SM.CONTROLS)
def test_each_well_formed_twin_joins(case):
    data, k, (begin, count) = SM.single_op_model(case)
    h, err, keep = open_passes(data, b"stem,slice", at_page_end=True)
    assert h and [ops for ops, _, _ in _sections_of(h)] == [[k, k + 1]], (case, err)
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    model = mr.LceModel(data, stem_sections=True, slice_sections=True)
    y = model.operators[k].outputs[0]
    assert model.section_tensor_shape(0, y, 5)[0] == (5, 4, 4, count)
    # nothing but its own name takes it, and without `stem` a slice of the graph's input is the host's
    h, err, _ = open_passes(data, ",".join(EVERY_OLD_NAME).encode())
    assert h and [ops for ops, _, _ in _sections_of(h)] == [[k + 1]], case
    mr.tflite_lib().lce_tflite_model_close(h)
    assert [s.ops for s in mr.LceModel(data, slice_sections=True).sections] == [[k + 1]]


# ---- the partition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int8])
def test_the_meliusnet_body_is_one_section_only_with_the_name(dtype):
    data, net, out = SM.meliusnet_model(dtype)
    names = SM.FLOAT_NAMES if dtype == np.float32 else SM.INT8_NAMES
    model = mr.LceModel(data, **names)
    assert parts(model) == [(list(range(len(model.operators))), [net.x0], [out])]
    assert mr.Interpreter(model).lce_only
    # without the name every slice cuts the body, and what hangs on a slice (the ADD, the CONCATENATION) goes with it
    without = mr.LceModel(data, **{k: v for k, v in names.items() if k != "slice_sections"})
    host = set(net.ops_of("slice", "improve_add", "improve_join"))
    # (float: the batch norm that reads an improvement block's CONCATENATION becomes ready in the host's epoch too, and the graph
    # ends in such a CONCATENATION; int8: the LceQuantize that reads it opens the next section, and a last binary layer a third)
    assert len(without.sections) == (2 if dtype == np.float32 else 3) and not mr.Interpreter(without).lce_only
    inside = {i for s in without.sections for i in s.ops}
    assert not (inside & host) and inside | host | set(net.ops_of("bn")) >= set(range(len(model.operators)))
    # one name short, the body is no longer one section
    for missing in names:
        assert not mr.Interpreter(mr.LceModel(data, **{k: v for k, v in names.items() if k != missing})).lce_only, missing
    # the same through the C entry
    h, err, keep = open_passes(data, ",".join(mr._PASS_NAMES[k] for k in names).encode(), at_page_end=True)
    assert h and _sections_of(h) == parts(model), err
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)


@pytest.mark.parametrize("case", SM.VARIANTS)
def test_each_variant_is_one_section(case):
    data, net, outs = SM.variant_model(case)
    model = mr.LceModel(data, **SM.FLOAT_NAMES)
    assert parts(model) == [(list(range(len(model.operators))), [net.x0], sorted(outs))]


@pytest.mark.parametrize("fixture", sorted(NO_HEAD))
def test_no_other_fixtures_partition_moves_when_slice_is_named(fixture):
    data = NO_HEAD[fixture]()[0]
    for names in ([], EVERY_OLD_NAME, ["elementwise", "concat"], ["stem"]):
        h, err, _ = open_passes(data, ",".join(names).encode())
        g, err2, _ = open_passes(data, ",".join(names + ["slice"]).encode())
        assert h and g, (err, err2)
        assert _sections_of(h) == _sections_of(g), (fixture, names)
        for x in (h, g):
            mr.tflite_lib().lce_tflite_model_close(x)


# ---- the walker's shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
def test_inferred_shapes_over_windows_sums_and_joins(batch):
    data, net, out = SM.meliusnet_model()
    model = mr.LceModel(data, **SM.FLOAT_NAMES)
    for k in net.ops_of("slice", "improve_add", "improve_join", "dense_join"):
        t = net.run[k][1]
        shape = model.tensors[t].shape
        assert model.section_tensor_shape(0, t, batch) == ((batch,) + tuple(shape[1:]), batch * 4 * int(np.prod(shape[1:]))), k
    data, net, out = SM.meliusnet_model(np.int8)
    model = mr.LceModel(data, **SM.INT8_NAMES)
    for k in net.ops_of("slice", "improve_add", "improve_join"):
        t = net.run[k][1]
        shape = model.tensors[t].shape
        assert model.section_tensor_shape(0, t, batch) == ((batch,) + tuple(shape[1:]), batch * int(np.prod(shape[1:]))), k


def test_a_file_whose_slice_input_disagrees_with_the_inferred_shape_is_refused():
    """The LceBconv2d output a slice reads is declared 8 channels wider than its filter makes it: the partition takes the file at
    its word, the walk must not (the window [72, 136) would be read past the buffer)."""
    net = SM.Net()
    y = net.binary(net.x0, 128)
    net.b.tensors[y].fields[0] = _Vector("i", [1, 8, 8, 136])
    net.channels[y] = 136
    s = net.slice(y, 72, 64, "plain")
    data = net.finish([net.binary(s)])
    model = mr.LceModel(data, **SM.FLOAT_NAMES)
    assert len(model.sections) == 1
    with pytest.raises(amd.LceHipError, match="slice input's shape"):
        model.section_tensor_shape(0, s, 2)


# ---- names, keyword, stats, symbols -------------------------------------------------------------------------------------------------
def test_open_passes_knows_the_name_and_still_refuses_the_rest():
    data = SM.meliusnet_model()[0]
    lib = mr.tflite_lib()
    for passes in (b"slice", b"slice,concat,elementwise", ",".join(EVERY_OLD_NAME + ["slice"]).encode()):
        h, err, _ = open_passes(data, passes)
        assert h, err
        lib.lce_tflite_model_close(h)
    for passes, offender in ((b"slices", b"'slices'"), (b"slice,slice", b"'slice'"), (b"slice,concat,slice", b"'slice'"), (b"slice,", b"''"),
                             (b"Slice", b"'Slice'"), (b"strided_slice", b"'strided_slice'")):
        h, msg, _ = open_passes(data, passes)
        assert not h and offender in msg and (b"unknown" in msg or b"twice" in msg), (passes, msg)
    # no bit and no struct size reaches it: every bit of both words set, the slices still cut the body
    opts = mr._OpenOptions56(56, 7, 31)
    err = C.create_string_buffer(256)
    h = lib.lce_tflite_model_open_opts(data, len(data), C.byref(opts), err, 256)
    assert h and len(_sections_of(h)) == 2, err.value
    lib.lce_tflite_model_close(h)


def test_the_keyword_exists_and_the_pinned_tables_keep_their_contents():
    data, net, out = SM.meliusnet_model()
    model = mr.LceModel(data, slice_sections=True)                      # (a TypeError before the keyword existed)
    assert model.slice_sections and not mr.LceModel(data).slice_sections
    assert mr.Interpreter(data, batch_size=2, **SM.FLOAT_NAMES).lce_only
    with pytest.raises(TypeError):
        mr.LceModel(data, slices_sections=True)
    assert mr._PASS_NAMES["slice_sections"] == "slice" and list(mr._PASS_NAMES)[-1] == "slice_sections"
    assert mr._PASS_STATS["slice"] == 3


def test_stats_are_zero_before_any_run():
    model = mr.LceModel(SM.meliusnet_model()[0], **SM.FLOAT_NAMES)
    assert model.slice_stats() == (0, 0, 0) and model.concat_stats() == (0, 0)


def test_the_symbols_are_exported():
    for s in ("lce_hip_join_windows", "lce_hip_join_windows_check"):
        assert s in amd.ABI_SYMBOLS and hasattr(amd.lib(), s)
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_slice_stats")


def _window(data=1 << 20, pitch=192, begin=0, count=64, addend=0, reserved=(0, 0)):
    w = amd.Window()
    w.data_dev, w.pitch, w.begin, w.count, w.addend_dev = data, pitch, begin, count, addend or None
    w.reserved[0], w.reserved[1] = reserved
    return w


def _c_call(windows, type=amd.F32, n=None, rows=4, zero_point=0, out=1 << 24, bits=1 << 25):
    arr = (amd.Window * max(len(windows), 1))(*windows)
    code = amd.lib().lce_hip_join_windows(type, arr if windows is not None else None, len(windows) if n is None else n, rows, zero_point,
                                          out, bits, None)
    return code, amd.lib().lce_hip_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(windows=[_window()], n=0), "num_windows"), (dict(windows=[_window()] * 8, n=9), "num_windows"),
    (dict(windows=[_window()], type=amd.BITPACKED), "float32 or int8"),
    (dict(windows=[_window(begin=129)]), "no window"), (dict(windows=[_window(begin=-1)]), "no window"), (dict(windows=[_window(count=0)]), "no window"),
    (dict(windows=[_window(pitch=2 ** 31 - 1, count=2 ** 30)] * 2), "2^31"),
    (dict(windows=[_window(addend=1 << 22)], type=amd.I8), "addend"), (dict(windows=[_window(addend=(1 << 22) + 2)]), "4-byte"),
    (dict(windows=[_window()], type=amd.I8, zero_point=128), "zero point"), (dict(windows=[_window()], zero_point=1), "zero point"),
    (dict(windows=[_window(reserved=(0, 1))]), "reserved"), (dict(windows=[_window(data=0)]), "null"),
    (dict(windows=[_window()], out=0, bits=0), "both outputs"),
    (dict(windows=[_window()], out=(1 << 20) + 4 * 4 * 192 - 4), "overlaps the source"),        # the last byte of the source's [rows, pitch]
    (dict(windows=[_window(addend=1 << 22)], bits=(1 << 22) + 8), "overlaps the addend"),
    (dict(windows=[_window()], bits=(1 << 24) + 64), "two outputs overlap"),
])
def test_the_c_entry_refuses_before_any_device_call(kw, msg):
    code, text = _c_call(**kw)
    assert code == amd.ERR_INVALID and msg in text, text


def test_zero_rows_is_a_no_op_checked_first():
    assert _c_call([_window(data=0, count=0)], rows=0, out=0, bits=0, n=0)[0] == amd.OK


def test_the_python_wrapper_checks_shapes_without_a_device():
    x, w = np.zeros((2, 3, 128), np.float32), np.zeros((2, 3, 64), np.float32)
    for windows, kw, msg in (([], {}, "1..8 windows"), ([(x, 0, 64)] * 9, {}, "1..8 windows"), ([(x, 64, 65)], {}, "no window"),
                             ([(x, -1, 4)], {}, "no window"), ([(x, 0, 0)], {}, "no window"), ([(x, 0, 32, w)], {}, "addend"),
                             ([(x.astype(np.int8), 0, 64, w)], {}, "addend"), ([(x, 0, 64), (w[:1], 0, 64)], {}, "tensor 1"),
                             ([(x.astype(np.int32), 0, 64)], {}, "float32 or int8"), ([(x, 0, 64)], dict(zero_point=1), "zero point"),
                             ([(x, 0, 64)], dict(out=np.zeros((2, 3, 65), np.float32)), "out must be"), ([(x, 0)], {}, "a window is")):
        with pytest.raises(ValueError, match=msg):
            amd.join_windows(windows, **kw)
    with pytest.raises(ValueError, match="no window"):
        amd.channel_slice(x, 100, 64)
