"""The int8 squeeze-and-excite gate in the model reader, without a GPU ("gate_i8" of lce_tflite_model_open_passes): the partition of
a RealToBinary-style int8 body with and without the name, one file per rule of the two predicates, every earlier fixture unmoved
by the name, the shapes the walker infers (the MUL and its residual ADD as one launch, the folded LceQuantize, the LOGISTIC on a
rank-2 tensor), and the ``passes=`` route of the Python constructors.  The GPU side is tests/test_gpu_gate_i8.py."""
import importlib

import pytest

import elementwise_i8_models as EM
import gate_i8_models as M
from section_models import _sections_of
from test_head_sections_host import NO_HEAD, open_passes, release

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

EVERY_OLD_NAME = [name for _, name, _, _, _ in mr._PASSES] + ["elementwise_i8"]
NEW = ("gate_i8",)
OTHERS = dict(head_i8_sections=True, reshape_sections=True, int8_add_sections=True)


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


def test_the_name_is_newer_than_the_python_table_and_the_symbols_are_exported():
    """Fails without the feature: the library does not know the name and exports neither the entries nor the counters."""
    assert "gate_i8" not in EVERY_OLD_NAME and len(mr._PASSES) == 18
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_gate_i8_stats")
    for name in ("lce_hip_mul_int8", "lce_hip_mul_int8_prepare", "lce_hip_mul_int8_path", "lce_hip_logistic_int8", "lce_hip_logistic_int8_prepare"):
        assert name in amd.ABI_SYMBOLS and hasattr(amd.lib(), name)
    h, err, _ = open_passes(M.single_op_model("mul_gate_slot1")[0], b"gate_i8")
    assert h, err
    mr.tflite_lib().lce_tflite_model_close(h)


# ---- the partition ------------------------------------------------------------------------------------------------------------------
def test_the_realtobinary_body_with_and_without_the_name():
    data, x, out, info = M.realtobinary_i8_model()
    b0, b1 = info["blocks"]
    n = len(mr.LceModel(data).operators)
    assert n == 18
    # today: every earlier name together still leaves LOGISTIC and MUL with the host -- more than one section, and the large
    # tensor y leaves the device in every block
    every_old = dict.fromkeys([k for k, _, _, _, _ in mr._PASSES], True)
    for old in (mr.LceModel(data, **every_old), mr.LceModel(data, passes=("elementwise_i8",), **every_old), mr.LceModel(data, **OTHERS)):
        assert len(old.sections) > 1
        assert all(b["logistic"] not in s.ops and b["mul"] not in s.ops for s in old.sections for b in (b0, b1))
        assert b0["tensors"]["y"] in old.sections[0].outputs
    assert [s.ops for s in mr.LceModel(data, **OTHERS).sections] == [[0, 1, 2, 3, 4], [9, 10, 11, 12, 13]]
    assert [s.ops for s in mr.LceModel(data).sections] == [[0, 1], [9, 10]]
    # the name alone: MEAN and FULLY_CONNECTED are the host's, so LOGISTIC and MUL become ready in the host's epoch -- nothing moves
    assert [s.ops for s in mr.LceModel(data, passes=NEW).sections] == [[0, 1], [9, 10]]
    # with the three names that carry the rest of the block: ONE section from x to the last sum
    both = mr.LceModel(data, passes=NEW, **OTHERS)
    assert parts(both) == [(list(range(n)), [x], [out])]
    assert parts(mr.LceModel(data, passes=tuple(M.NAMES.split(",")))) == parts(both)
    assert mr.Interpreter(both).lce_only and not mr.Interpreter(data, **OTHERS).lce_only
    # without int8_add the ADD is the host's and cuts every block behind its MUL
    cut = mr.LceModel(data, passes=NEW, head_i8_sections=True, reshape_sections=True)
    assert [s.ops for s in cut.sections] == [[0, 1, 2, 3, 4, 5, 6, 7], [9, 10, 11, 12, 13, 14, 15, 16]]


@pytest.mark.parametrize("batch", [1, 5])
def test_the_walkers_shapes_the_fused_add_and_the_folded_quantize(batch):
    """The walk without a run.  A product that the absorbed ADD alone reads is never written: the MUL and the ADD are ONE launch, and
    the walk holds no tensor of the product's name -- lce_tflite_model_section_tensor_shape refuses it -- in both blocks (in the
    second the gate stands in the MUL's slot 0 and the product in the ADD's slot 1).  The sum is the fold's value, the next
    block's LceQuantize its bits, the LOGISTIC runs on [b, C] carried as [b,1,1,C]."""
    data, x, out, info = M.realtobinary_i8_model()
    model = mr.LceModel(data, passes=NEW, **OTHERS)
    assert model.operators[info["blocks"][0]["mul"]].inputs[1] == info["blocks"][0]["tensors"]["gate"]
    assert model.operators[info["blocks"][1]["mul"]].inputs[0] == info["blocks"][1]["tensors"]["gate"]
    assert model.operators[info["blocks"][1]["add"]].inputs[1] == info["blocks"][1]["tensors"]["product"]
    for bi in info["blocks"]:
        t = bi["tensors"]
        assert model.section_tensor_shape(0, t["sigmoid"], batch) == ((batch, 1, 1, 64), batch * 64)
        assert model.section_tensor_shape(0, t["gate"], batch) == ((batch, 1, 1, 64), batch * 64)
        for name in ("y", "sum"):
            assert model.section_tensor_shape(0, t[name], batch) == ((batch, 8, 8, 64), batch * 8 * 8 * 64)
        with pytest.raises(amd.LceHipError, match="does not touch"):
            model.section_tensor_shape(0, t["product"], batch)
        assert model.operators[bi["logistic"]].inputs == [t["h2"]] and len(model.tensors[t["h2"]].shape) == 2
    q2 = model.operators[info["blocks"][1]["quantize"]].outputs[0]
    assert model.section_tensor_shape(0, q2, batch) == ((batch, 8, 8, 2), batch * 8 * 8 * 2 * 4)
    assert model.gate_i8_stats() == (0, 0, 0) and mr.LceModel(data).gate_i8_stats() == (0, 0, 0)


def test_the_add_stays_int8_adds_where_the_product_is_a_tensor_of_its_own():
    """The controls of the walker's decision, each still ONE section in which the product IS a tensor of the walk (the MUL is a
    launch of its own and the ADD the int8 ADD pass's): a product with a second reader, and a product the section delivers
    because int8_add is not named."""
    data, x, out, info = M.realtobinary_i8_model(side_reader=True)
    model = mr.LceModel(data, passes=NEW, **OTHERS)
    assert len(model.sections) == 1 and len(model.sections[0].outputs) == 3
    for bi in info["blocks"]:
        assert sorted(j for j, op in enumerate(model.operators) if bi["tensors"]["product"] in op.inputs) == [bi["add"], bi["side"]]
        for name in ("y", "product", "sum"):
            assert model.section_tensor_shape(0, bi["tensors"][name], 3) == ((3, 8, 8, 64), 3 * 8 * 8 * 64)
    data, x, out, info = M.realtobinary_i8_model()
    cut = mr.LceModel(data, passes=NEW, head_i8_sections=True, reshape_sections=True)
    for k, bi in enumerate(info["blocks"]):
        assert cut.sections[k].outputs == [bi["tensors"]["product"]]
        assert cut.section_tensor_shape(k, bi["tensors"]["product"], 3) == ((3, 8, 8, 64), 3 * 8 * 8 * 64)


# ---- the predicates -----------------------------------------------------------------------------------------------------------------
def test_each_broken_rule_stays_with_the_host():
    for case in M.REFUSALS:
        data, k, _, _ = M.single_op_model(case)
        h, err, keep = open_passes(data, ",".join(EVERY_OLD_NAME + ["gate_i8"]).encode(), at_page_end=True)
        assert h, (case, err)
        assert all(k not in ops for ops, _, _ in _sections_of(h)), case
        mr.tflite_lib().lce_tflite_model_close(h)
        release(keep)


@pytest.mark.parametrize("case", M.CONTROLS)
def test_each_well_formed_operator_joins(case):
    data, k, _, _ = M.single_op_model(case)
    names = b"head_i8,gate_i8" if case == "logistic_rank2" else b"gate_i8"
    h, err, keep = open_passes(data, names, at_page_end=True)
    assert h and [ops for ops, _, _ in _sections_of(h)] == [list(range(k + 1))], (case, err)
    mr.tflite_lib().lce_tflite_model_close(h)
    release(keep)
    # nothing but its own name takes it
    h, err, _ = open_passes(data, ",".join(EVERY_OLD_NAME).encode())
    assert h and all(k not in ops for ops, _, _ in _sections_of(h)), case
    mr.tflite_lib().lce_tflite_model_close(h)
    model = mr.LceModel(data, passes=NEW + (("head_i8",) if case == "logistic_rank2" else ()))
    y = model.operators[k].outputs[0]
    assert model.section_tensor_shape(0, y, 5)[0] == ((5, 1, 1, 32) if case == "logistic_rank2" else (5, 4, 4, 32))


def test_the_constant_mul_and_the_logistic_of_the_older_fixtures_keep_their_verdicts():
    """elementwise_i8_models' `mul_int8` (a constant operand) stays with the host under both names; its `logistic_int8` -- an
    output at (1/256, -128) -- is refused by elementwise_i8 alone and taken by gate_i8."""
    for case, taken in (("mul_int8", False), ("logistic_int8", True)):
        data, k, _ = EM.single_op_model(case)
        for names, want in ((b"elementwise_i8", False), (b"elementwise_i8,gate_i8", taken)):
            h, err, _ = open_passes(data, names)
            assert h and any(k in ops for ops, _, _ in _sections_of(h)) == want, (case, names)
            mr.tflite_lib().lce_tflite_model_close(h)


def test_no_other_fixtures_partition_moves_when_the_name_is_added():
    for fixture in sorted(NO_HEAD):
        data = NO_HEAD[fixture]()[0]
        for names in ([], EVERY_OLD_NAME, ["elementwise", "concat"], ["int8_add"], ["stem"]):
            h, err, _ = open_passes(data, ",".join(names).encode())
            g, err2, _ = open_passes(data, ",".join(names + ["gate_i8"]).encode())
            assert h and g, (fixture, err, err2)
            assert _sections_of(h) == _sections_of(g), (fixture, names)
            for x in (h, g):
                mr.tflite_lib().lce_tflite_model_close(x)


def test_the_float_gated_block_the_int8_reactnet_and_the_int8_heads_are_unmoved():
    import activation_models as AM
    import head_i8_models as HM8
    files = [AM.gated_model()[0], AM.reactnet_model()[0], EM.reactnet_i8_model()[0], EM.requantize_concat_model()[0], EM.relu6_model()[0]]
    files += [make()[0] for make in HM8.FIXTURES.values()]
    for data in files:
        for names in ([], EVERY_OLD_NAME):
            h, _, _ = open_passes(data, ",".join(names).encode())
            g, _, _ = open_passes(data, ",".join(names + ["gate_i8"]).encode())
            assert h and g and _sections_of(h) == _sections_of(g)
            for x in (h, g):
                mr.tflite_lib().lce_tflite_model_close(x)


# ---- the keyword --------------------------------------------------------------------------------------------------------------------
def test_the_passes_route():
    data = M.realtobinary_i8_model()[0]
    model = mr.LceModel(data, passes=["gate_i8"])
    assert model.passes == ("gate_i8",) and model.gate_i8_stats() == (0, 0, 0)
    for bad, word in ((("gate_i9",), "gate_i9"), (("gate_i8", "gate_i8"), "twice")):
        with pytest.raises(ValueError, match=word):
            mr.LceModel(data, passes=bad)
    with pytest.raises(TypeError):
        mr.LceModel(data, gate_i8_sections=True)
    it = mr.Interpreter(data, passes=tuple(M.NAMES.split(",")))
    assert it.model.passes == tuple(M.NAMES.split(",")) and it.lce_only
