"""The "transition" name of lce_tflite_model_open_passes in the model reader, without a GPU: the partition does not move; without
the name the walk is what it was; with it the pooled tensor of a float transition (section_models.quicknet_transition_model) is no
tensor of the walk, while every other tensor keeps its shape and the LceQuantize behind a blur that only it reads still folds; and
the walker declines (the pooled tensor stays a tensor of the walk: two launches) when the pooled tensor has a second reader, when
the section delivers it, when the pool is AVERAGE, and for the int8 fixtures (depthwise_i8_models' transition and network), whose
fused entry measured slower than the two launches.  The
counters are of the last RUN and stay zero here; tests/test_gpu_transition.py checks them on the device (one launch and two
operators per transition, the pool's and the depthwise convolution's own counters lower by one each)."""
import importlib

import pytest

import depthwise_i8_models as DM
import transition_models as TM
from section_models import _sections_of, quicknet_transition_model
from test_depthwise_sections_host import ALL_FLAGS
from test_head_sections_host import NO_HEAD, open_passes

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")

NEW = ("transition",)
EVERY_OLD_NAME = [name for _, name, _, _, _ in mr._PASSES] + ["elementwise_i8", "gate_i8"]


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


def shapes(model, batch):
    """tensor -> (dims, bytes) for every tensor the walk of section 0 holds."""
    held = {}
    for t in range(len(model.tensors)):
        try:
            held[t] = model.section_tensor_shape(0, t, batch)
        except amd.LceHipError as e:
            assert "does not touch" in str(e)
    return held


def test_opening_with_the_name_succeeds_and_the_counters_are_exported():
    """Fails without the feature: the library does not know the name."""
    assert "transition" not in EVERY_OLD_NAME and len(mr._PASSES) == 18
    assert hasattr(mr.tflite_lib(), "lce_tflite_model_transition_stats")
    h, err, _ = open_passes(quicknet_transition_model()[0], b"transition")
    assert h, err
    mr.tflite_lib().lce_tflite_model_close(h)
    model = mr.LceModel(quicknet_transition_model()[0], passes=["transition"])
    assert model.passes == NEW and model.transition_stats() == (0, 0, 0)
    for bad, word in ((("transitions",), "transitions"), (("transition", "transition"), "twice")):
        with pytest.raises(ValueError, match=word):
            mr.LceModel(quicknet_transition_model()[0], passes=bad)


@pytest.mark.parametrize("batch", [1, 4])
def test_the_float_transition_with_and_without_the_name(batch):
    data, x, out, info = quicknet_transition_model()
    pool = info["depthwise"] - 1
    old, new = mr.LceModel(data, **ALL_FLAGS), mr.LceModel(data, passes=NEW, **ALL_FLAGS)
    assert new.operators[pool].outputs == [info["tensors"]["p"]] and new.operators[info["depthwise"]].inputs[0] == info["tensors"]["p"]
    assert parts(old) == parts(new) and len(new.sections) == 1
    # the name alone enables nothing: the default partition
    assert parts(mr.LceModel(data, passes=NEW)) == parts(mr.LceModel(data))
    a, b = shapes(old, batch), shapes(new, batch)
    p = info["tensors"]["p"]
    H, Cc = info["size"], info["channels"]
    assert a[p] == ((batch, H, H, Cc), batch * H * H * Cc * 4)
    assert p not in b and {t: s for t, s in a.items() if t != p} == b
    with pytest.raises(amd.LceHipError, match="does not touch"):
        new.section_tensor_shape(0, p, batch)
    assert b[info["tensors"]["d"]] == ((batch, H // 2, H // 2, Cc), batch * (H // 2) ** 2 * Cc * 4)
    assert old.transition_stats() == new.transition_stats() == (0, 0, 0) and new.pool_stats() == (0, 0)


@pytest.mark.parametrize("name", ["transition_per_channel", "transition_per_tensor", "network_per_channel"])
def test_the_int8_fixtures_keep_their_two_launches(name):
    """lce_hip_pool_depthwise_i8 measured slower than the two launches (profiles/transition/layers.txt), so the reader leaves an int8
    pair alone: with the name the partition and the walk -- the pooled tensor included -- are what they are without it."""
    data, x, out, info = DM.FIXTURES[name]()
    old, new = mr.LceModel(data, **DM.EVERY_FLAG), mr.LceModel(data, passes=NEW, **DM.EVERY_FLAG)
    assert parts(old) == parts(new) and len(new.sections) == 1
    assert parts(mr.LceModel(data, passes=NEW, **DM.EARLIER)) == parts(mr.LceModel(data, **DM.EARLIER))
    pools = [j for j, op in enumerate(new.operators) if op.builtin_code == 17]
    assert len(pools) == 1 and new.operators[pools[0] + 1].builtin_code == 4
    p = new.operators[pools[0]].outputs[0]
    assert new.operators[pools[0] + 1].inputs[0] == p
    a, b = shapes(old, 3), shapes(new, 3)
    assert a == b and p in b and b[p][0][0] == 3 and b[p][1] == b[p][0][0] * b[p][0][1] * b[p][0][2] * b[p][0][3]


def test_the_quantize_behind_a_blur_that_only_it_reads_still_folds():
    data, x, outs, info = TM.pool_blur_model()
    old, new = mr.LceModel(data, **TM.FLAGS), mr.LceModel(data, passes=NEW, **TM.FLAGS)
    assert parts(old) == parts(new) and [s.ops for s in new.sections] == [list(range(6))]
    a, b = shapes(old, 2), shapes(new, 2)
    t = info["tensors"]
    assert t["p"] in a and t["p"] not in b and {k: s for k, s in a.items() if k != t["p"]} == b
    assert b[t["bits"]] == ((2, 4, 4, 2), 2 * 4 * 4 * 2 * 4) and b[t["d"]] == ((2, 4, 4, 64), 2 * 4 * 4 * 64 * 4)


@pytest.mark.parametrize("variant", ["average", "second_reader", "deliver_pooled"])
def test_the_walker_declines_and_two_launches_remain(variant):
    data, x, outs, info = TM.pool_blur_model(**{variant: True})
    old, new = mr.LceModel(data, **TM.FLAGS), mr.LceModel(data, passes=NEW, **TM.FLAGS)
    assert parts(old) == parts(new)
    assert any(info["pool"] in s.ops and info["depthwise"] in s.ops for s in new.sections)
    a, b = shapes(old, 2), shapes(new, 2)
    assert a == b and b[info["tensors"]["p"]] == ((2, 8, 8, 64), 2 * 8 * 8 * 64 * 4)          # the pooled tensor IS a tensor of the walk


def test_no_fixtures_partition_moves_when_the_name_is_added():
    for fixture in sorted(NO_HEAD):
        data = NO_HEAD[fixture]()[0]
        for names in ([], EVERY_OLD_NAME, ["pool", "depthwise"], ["stem"]):
            h, err, _ = open_passes(data, ",".join(names).encode())
            g, err2, _ = open_passes(data, ",".join(names + ["transition"]).encode())
            assert h and g, (fixture, err, err2)
            assert _sections_of(h) == _sections_of(g), (fixture, names)
            for m in (h, g):
                mr.tflite_lib().lce_tflite_model_close(m)
