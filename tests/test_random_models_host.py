"""Random mixed float / int8 networks (tests/random_models.py) against the code that composes the fused passes, on the CPU: the
partition of each seed's file with every keyword, with each keyword dropped and with the seed's own subset dropped, against the
independent restatement of tests/partition_ref.py; the section walk without launches (lce_tflite_model_section_tensor_shape: every
walker's shape inference and every fold's registered bit shape) against the shapes of the NumPy forward pass; the generator's own
wiring; and the floors on what the kept seeds cover."""
import collections
import importlib

import numpy as np
import pytest

import partition_ref as P
import random_models as RM

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


@pytest.mark.parametrize("seed", RM.SEEDS)
def test_with_every_keyword_the_file_is_one_section(seed):
    info = RM.build(seed)
    model = mr.LceModel(info["data"], **RM.EVERY_FLAG)
    # the library reads the file as the generator wrote it
    assert [(op.inputs, op.outputs) for op in model.operators] == info["ops"]
    assert {t for t, T in enumerate(model.tensors) if T.constant} == info["constants"]
    assert model.inputs == [info["input"]] and model.outputs == info["outputs"]
    n = len(info["ops"])
    assert None not in info["names"]
    assert parts(model) == [(list(range(n)), [info["input"]], sorted(info["outputs"]))] == RM.reference_partition(info, RM.EVERY_FLAG)
    it = mr.Interpreter(info["data"], **RM.EVERY_FLAG)
    assert it.lce_only and len(it.sections) == 1


@pytest.mark.parametrize("seed", RM.SEEDS)
def test_the_walk_infers_the_shape_of_every_tensor(seed):
    info = RM.build(seed)
    model = mr.LceModel(info["data"], **RM.EVERY_FLAG)
    vals = info["forward"](info["x"])
    assert set(vals) == set(range(len(model.tensors))) - info["constants"]
    for batch in (1, 5):
        for t, v in vals.items():
            want = (batch,) + ((1, 1, v.shape[1]) if v.ndim == 2 else v.shape[1:])          # (rank 2 is carried as [b, 1, 1, C])
            dims, nbytes = model.section_tensor_shape(0, t, batch)
            assert dims == want and nbytes == int(np.prod(want)) * v.dtype.itemsize, (t, dims, want)
    # (a value that folded away -- its only reader is the LceQuantize its producer's launch absorbed -- is among them: every walker
    # registers its result's shape before the fold decides whether the value is written, so only a tensor the walk never
    # touches is refused)
    with pytest.raises(amd.LceHipError, match="does not touch"):
        model.section_tensor_shape(0, min(info["constants"] | {len(model.tensors)}), 1)


def dropped_sets(seed):
    names = sorted(RM.EVERY_FLAG)
    return [{k: True for k in names if k != name} for name in names] + [RM.cut_flags(seed)]


@pytest.mark.parametrize("seed", RM.SEEDS)
def test_the_partition_with_keywords_dropped_is_the_restated_one(seed):
    info = RM.build(seed)
    cut = 0
    for flags in dropped_sets(seed):
        want = RM.reference_partition(info, flags)
        model = mr.LceModel(info["data"], **flags)
        assert parts(model) == want, (sorted(set(RM.EVERY_FLAG) - set(flags)), parts(model), want)
        cut += want != RM.reference_partition(info, RM.EVERY_FLAG)
        # every section's walk still infers its tensors' shapes
        vals = info["forward"](info["x"][:2])
        for k, (_, ins, outs) in enumerate(want):
            for t in ins + outs:
                v = vals[t]
                assert model.section_tensor_shape(k, t, 2)[0] == (2,) + ((1, 1, v.shape[1]) if v.ndim == 2 else v.shape[1:])
    assert cut >= 1                                                   # (dropping a keyword did move a boundary)


@pytest.mark.parametrize("seed", RM.SEEDS)
def test_the_forward_pass_agrees_with_itself_section_by_section(seed):
    """The seed's own cut, run as the GPU test runs it: the operators outside the sections one by one, every section from its
    inputs alone to its outputs alone.  Guards the generator's wiring and the section lists."""
    info = RM.build(seed)
    x = info["x"][:3]
    vals = info["forward"](x)
    sections = RM.reference_partition(info, RM.cut_flags(seed))
    variable = lambda i: [t for t in info["ops"][i][0] if t >= 0 and t not in info["constants"]]
    ran = set()

    def run_section(k, arrays):
        members, ins, outs = sections[k]
        ran.add(k)
        inner = dict(zip(ins, arrays))
        for j in members:
            inner[info["ops"][j][1][0]] = info["host"][j](*[inner[t] for t in variable(j)])
        return [inner[t] for t in outs]
    live = RM.run_cut(info, sections, x, run_section)
    assert set(info["outputs"]) <= set(live) and len(ran) == len(sections)
    for t, v in live.items():
        assert v.dtype == vals[t].dtype and np.array_equal(v.view(np.uint8), vals[t].view(np.uint8)), t


def test_the_kept_seeds_are_what_the_conditions_keep_and_cover_every_feature_and_pass():
    kept = tuple(s for s in range(RM.CANDIDATES) if not RM.violations(RM.build(s)))
    assert kept == RM.SEEDS
    assert 4 * (RM.CANDIDATES - len(kept)) <= RM.CANDIDATES
    features, passes = collections.Counter(), collections.Counter()
    for s in RM.SEEDS:
        info = RM.build(s)
        features.update(k for k, v in info["features"].items() if v)
        passes.update(set(info["names"]))
    print("features", dict(sorted(features.items())), "passes", {k: passes[k] for k in P.PASSES + P.LCE_OPS})
    assert all(features[k] >= 5 for k in RM.FEATURES), features
    assert all(features[k] >= 5 for k in RM.JOIN_FEATURES), features   # joins of 4 and of exactly 8 inputs, a repeated input, ragged channels
    assert all(passes[k] >= 5 for k in P.PASSES), passes
    # the shapes stay small
    for s in RM.SEEDS:
        info = RM.build(s)
        assert 6 <= len(info["ops"]) <= 20 and info["x"].shape[0] == info["batch"] + 2 <= 10
        assert all(5 <= d <= 12 for d in info["x"].shape[1:3])
