"""The int8 elementwise chain in the model reader, without a GPU ("elementwise_i8" of lce_tflite_model_open_passes): the partition
of an int8 ReActNet-style body, a requantize -> CONCATENATION join and a standalone RELU6 with and without the name, one file per
rule of the predicate, every earlier fixture unmoved by the name, the shapes the walker infers, and the ``passes=`` keyword of the
Python constructors.  The GPU side is tests/test_gpu_elementwise_i8.py."""
import importlib

import numpy as np
import pytest

import elementwise_i8_models as M
from section_models import _sections_of
from test_head_sections_host import NO_HEAD, open_passes, release

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

EVERY_OLD_NAME = [name for _, name, _, _, _ in mr._PASSES]
NEW = ("elementwise_i8",)


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


def test_the_name_is_newer_than_the_python_table_and_the_symbol_is_exported():
    """Fails without the feature: the library does not know the name and does not export the counters."""
    assert "elementwise_i8" not in EVERY_OLD_NAME and len(mr._PASSES) == 18 and len(mr._PASS_STATS) == 17
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_elementwise_i8_stats")
    h, err, _ = open_passes(M.relu6_model()[0], b"elementwise_i8")
    assert h, err
    mr.tflite_lib().lce_tflite_model_close(h)


# ---- the partition ------------------------------------------------------------------------------------------------------------------
def test_the_reactnet_body_with_and_without_the_name():
    data, x, out, info = M.reactnet_i8_model()
    n = len(mr.LceModel(data).operators)
    assert n == 12
    # today: every builtin operator cuts -- one section per block (LceQuantize, LceBconv2d), with or without int8_add's ADD
    plain = mr.LceModel(data)
    assert [s.ops for s in plain.sections] == [[0, 1], [6, 7]]
    assert parts(mr.LceModel(data, int8_add_sections=True)) == [([0, 1, 2], [x], [info["tails"][0]["tensors"][0]]),
                                                               ([6, 7, 8], [info["tails"][0]["tensors"][3]], [info["tails"][1]["tensors"][0]])]
    # the name alone: the residual ADD is the host's, and the tail behind it becomes ready in the host's epoch -- nothing moves
    alone = mr.LceModel(data, passes=NEW)
    assert [s.ops for s in alone.sections] == [[0, 1], [6, 7]]
    # both: ONE section from x to the last tensor
    both = mr.LceModel(data, int8_add_sections=True, passes=NEW)
    assert parts(both) == [(list(range(n)), [x], [out])]
    assert mr.Interpreter(both).lce_only and mr.Interpreter(data, int8_add_sections=True, passes=NEW).lce_only
    assert not mr.Interpreter(data, passes=NEW).lce_only


def test_the_requantize_join_with_and_without_the_name():
    data, x, out, info = M.requantize_concat_model()
    n = len(mr.LceModel(data).operators)
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1, 2], [5, 6]]
    # concat alone: the requantize keeps the join with the host (its input is the host's)
    assert [s.ops for s in mr.LceModel(data, concat_sections=True).sections] == [[0, 1, 2], [5, 6]]
    # the name alone: the requantize joins the first section, the CONCATENATION still cuts
    assert [s.ops for s in mr.LceModel(data, passes=NEW).sections] == [[0, 1, 2, 3], [5, 6]]
    both = mr.LceModel(data, concat_sections=True, passes=NEW)
    assert parts(both) == [(list(range(n)), [x], [out])]


def test_the_standalone_relu6_with_and_without_the_name():
    data, x, out, info = M.relu6_model()
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [3, 4]]
    every_old = dict.fromkeys([k for k, _, _, _, _ in mr._PASSES], True)
    assert [s.ops for s in mr.LceModel(data, **every_old).sections] == [[0, 1], [3, 4]]
    assert parts(mr.LceModel(data, passes=NEW)) == [([0, 1, 2, 3, 4], [x], [out])]


# ---- the predicate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.REFUSALS)
def test_each_broken_rule_stays_with_the_host(case):
    data, k, _ = M.single_op_model(case)
    # (every old name too, to show that nothing takes it -- but for the residual ADD's, which takes the ADD of two tensors, and for
    # "quantize", which takes the float -> int8 QUANTIZE)
    skip = {"add_two_tensors_no_int8_add": "int8_add", "quantize_from_float": "quantize"}.get(case)
    h, err, keep = open_passes(data, ",".join([n for n in EVERY_OLD_NAME if n != skip] + ["elementwise_i8"]).encode(), at_page_end=True)
    assert h, err
    assert all(k not in ops for ops, _, _ in _sections_of(h)), case
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)


@pytest.mark.parametrize("case", M.CONTROLS)
def test_each_well_formed_operator_joins(case):
    data, k, ref = M.single_op_model(case)
    h, err, keep = open_passes(data, b"elementwise_i8", at_page_end=True)
    assert h and [ops for ops, _, _ in _sections_of(h)] == [[0, 1, k]], (case, err)
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    # nothing but its own name takes it
    h, err, _ = open_passes(data, ",".join(EVERY_OLD_NAME).encode())
    assert h and [ops for ops, _, _ in _sections_of(h)] == [[0, 1]], case
    mr.tflite_lib().lce_tflite_model_close(h)
    model = mr.LceModel(data, passes=NEW)
    y = model.operators[k].outputs[0]
    assert model.section_tensor_shape(0, y, 5)[0] == (5, 4, 4, 32)


@pytest.mark.parametrize("fixture", sorted(NO_HEAD))
def test_no_other_fixtures_partition_moves_when_the_name_is_added(fixture):
    data = NO_HEAD[fixture]()[0]
    for names in ([], EVERY_OLD_NAME, ["elementwise", "concat"], ["int8_add"], ["stem"]):
        h, err, _ = open_passes(data, ",".join(names).encode())
        g, err2, _ = open_passes(data, ",".join(names + ["elementwise_i8"]).encode())
        assert h and g, (err, err2)
        assert _sections_of(h) == _sections_of(g), (fixture, names)
        for x in (h, g):
            mr.tflite_lib().lce_tflite_model_close(x)


def test_a_float_reactnet_is_unmoved():
    import activation_models as AM
    data = AM.reactnet_model()[0]
    for names in ([], list(AM.OLD_NAMES) + list(AM.NEW_NAMES)):
        h, _, _ = open_passes(data, ",".join(names).encode())
        g, _, _ = open_passes(data, ",".join(names + ["elementwise_i8"]).encode())
        assert h and g and _sections_of(h) == _sections_of(g)
        for x in (h, g):
            mr.tflite_lib().lce_tflite_model_close(x)


# ---- the walker's shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
def test_inferred_shapes_over_the_chain_the_head_and_the_folded_quantize(batch):
    data, x, out, info = M.reactnet_i8_model()
    model = mr.LceModel(data, int8_add_sections=True, passes=NEW)
    for tail in info["tails"]:
        for t in tail["tensors"]:
            assert model.section_tensor_shape(0, t, batch) == ((batch, 8, 8, 64), batch * 8 * 8 * 64)
    q2 = model.operators[info["tails"][1]["quantize"]].outputs[0]
    assert model.section_tensor_shape(0, q2, batch) == ((batch, 8, 8, 2), batch * 8 * 8 * 2 * 4)
    data, x, out, info = M.requantize_concat_model()
    model = mr.LceModel(data, concat_sections=True, passes=NEW)
    assert model.section_tensor_shape(0, model.operators[info["requantize"]].outputs[0], batch)[0] == (batch, 8, 8, 32)
    assert model.section_tensor_shape(0, model.operators[info["concat"]].outputs[0], batch)[0] == (batch, 8, 8, 96)


# ---- the keyword --------------------------------------------------------------------------------------------------------------------
def test_the_passes_keyword():
    data = M.relu6_model()[0]
    model = mr.LceModel(data, passes=["elementwise_i8"])
    assert model.passes == ("elementwise_i8",) and model.elementwise_i8_stats() == (0, 0, 0)
    assert mr.LceModel(data).passes == () and mr.LceModel(data).elementwise_i8_stats() == (0, 0, 0)
    # appended to the names of the keywords given; any name in it forces the route through lce_tflite_model_open_passes
    seen = []
    real = mr.tflite_lib().lce_tflite_model_open_passes
    class Spy:
        def __getattr__(self, name):
            return getattr(mr._tfl, name)
    lib = mr.tflite_lib()
    orig = mr.tflite_lib
    try:
        class Wrapped:
            def __getattr__(self, name):
                if name == "lce_tflite_model_open_passes":
                    def call(data, size, names, err, n):
                        seen.append(names)
                        return real(data, size, names, err, n)
                    return call
                return getattr(lib, name)
        mr.tflite_lib = lambda: Wrapped()
        m2 = mr.LceModel(data, int8_add_sections=True, concat_sections=True, passes=("elementwise_i8",))
        m3 = mr.LceModel(data, passes=("elementwise",))
    finally:
        mr.tflite_lib = orig
    assert seen == [b"int8_add,concat,elementwise_i8", b"elementwise"]
    assert m2.int8_add_sections and m2.concat_sections and not m2.pool_sections and m3.passes == ("elementwise",)
    # the library's refusal becomes the ValueError
    for bad, word in ((("elementwise_i9",), "elementwise_i9"), (("elementwise_i8", "elementwise_i8"), "twice"), (("elementwise_i8", ""), "unknown")):
        with pytest.raises(ValueError, match=word):
            mr.LceModel(data, passes=bad)
    with pytest.raises(ValueError, match="twice"):
        mr.LceModel(data, int8_add_sections=True, passes=("int8_add",))
    with pytest.raises(TypeError):
        mr.LceModel(data, passes="elementwise_i8")
    with pytest.raises(TypeError):
        mr.LceModel(data, elementwise_i8_sections=True)
    it = mr.Interpreter(data, passes=("elementwise_i8",))
    assert it.model.passes == ("elementwise_i8",) and it.lce_only
    assert mr.Interpreter(model, passes=("nonsense",)).model is model
