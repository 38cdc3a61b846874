"""Generation 2 of the random mixed networks (tests/random_models2.py: all 25 rows of the pass table and the "transition" fusion)
against the code that composes the fused passes, on the CPU, as tests/test_random_models_host.py does it for generation 1: the
partition of each seed's file with every keyword and name, with each of them dropped and with the seed's own subset dropped,
against tests/partition_ref2.py; the section walk without launches against the shapes of the NumPy forward pass; the generator's
own wiring; the floors on what the kept seeds cover; and generation 1 itself against the digests recorded before generation 2
existed."""
import collections
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import partition_ref2 as P2
import random_models as RM
import random_models2 as R2

amd = importlib.import_module("compute-engine_amd")
# (LCE_FUZZ_SEED / LCE_FUZZ_EXAMPLES append freshly drawn seeds here as they do in tests/test_gpu_random_models2.py)
SEEDS = list(R2.SEEDS) + R2.fuzz_seeds()
mr = importlib.import_module("compute-engine_amd.model_runner")


def open_model(info, flags):
    passes, keywords = R2.model_args(flags)
    return mr.LceModel(info["data"], passes=passes, **keywords)


def parts(model):
    return [(s.ops, s.inputs, s.outputs) for s in model.sections]


def carried(v, batch):
    return (batch,) + ((1, 1, v.shape[1]) if v.ndim == 2 else v.shape[1:])          # (rank 2 is carried as [b, 1, 1, C])


def test_generation_1_is_bit_identical():
    """random_models.build(s) gives the files and inputs it gave before generation 2 was written, for all 56 candidates (the six
    dropped ones decide SEEDS), and SEEDS is the list it was."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "random_models_gen1_digests.json")) as f:
        golden = json.load(f)
    assert RM.CANDIDATES == golden["candidates"] == 56 and list(RM.SEEDS) == golden["seeds"] and len(RM.SEEDS) == 50
    for s in range(RM.CANDIDATES):
        info = RM.build(s)
        assert hashlib.sha256(bytes(info["data"]) + info["x"].tobytes()).hexdigest() == golden["sha256"][str(s)], s


@pytest.mark.parametrize("seed", SEEDS)
def test_with_every_keyword_and_name_the_file_is_one_section(seed):
    info = R2.build(seed)
    model = open_model(info, R2.EVERY_FLAG)
    # the library reads the file as the generator wrote it
    assert [(op.inputs, op.outputs) for op in model.operators] == info["ops"]
    assert {t for t, T in enumerate(model.tensors) if T.constant} == info["constants"]
    assert model.inputs == [info["input"]] and model.outputs == info["outputs"]
    n = len(info["ops"])
    assert None not in info["names"]
    assert parts(model) == [(list(range(n)), [info["input"]], sorted(info["outputs"]))] == R2.reference_partition(info, R2.EVERY_FLAG)
    passes, keywords = R2.model_args(R2.EVERY_FLAG)
    it = mr.Interpreter(info["data"], passes=passes, **keywords)
    assert it.lce_only and len(it.sections) == 1


@pytest.mark.parametrize("seed", SEEDS)
def test_the_walk_infers_the_shape_of_every_tensor(seed):
    info = R2.build(seed)
    model = open_model(info, R2.EVERY_FLAG)
    vals = info["forward"](info["x"])
    assert set(vals) == set(range(len(model.tensors))) - info["constants"]
    elided = info["walk"]["elided"]
    for batch in (1, 5):
        for t, v in vals.items():
            if t in elided:
                # a pooled tensor inside a fused transition and a product under a rider ADD exist in registers only: the walk
                # holds no tensor of that name, which is how a walk without launches shows that the two operators share a launch
                with pytest.raises(amd.LceHipError, match="does not touch"):
                    model.section_tensor_shape(0, t, batch)
                continue
            want = carried(v, batch)
            dims, nbytes = model.section_tensor_shape(0, t, batch)
            assert dims == want and nbytes == int(np.prod(want)) * v.dtype.itemsize, (t, dims, want)
    with pytest.raises(amd.LceHipError, match="does not touch"):
        model.section_tensor_shape(0, min(info["constants"] | {len(model.tensors)}), 1)


def dropped_sets(seed):
    names = sorted(R2.EVERY_FLAG)
    return [{k: True for k in names if k != name} for name in names] + [R2.cut_flags(seed)]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_partition_with_names_dropped_is_the_restated_one(seed):
    info = R2.build(seed)
    cut = 0
    vals = info["forward"](info["x"][:2])
    for flags in dropped_sets(seed):
        want = R2.reference_partition(info, flags)
        model = open_model(info, flags)
        assert parts(model) == want, (sorted(set(R2.EVERY_FLAG) - set(flags)), parts(model), want)
        cut += want != R2.reference_partition(info, R2.EVERY_FLAG)
        # every section's walk still infers its tensors' shapes
        for k, (_, ins, outs) in enumerate(want):
            for t in ins + outs:
                assert model.section_tensor_shape(k, t, 2)[0] == carried(vals[t], 2)
    assert cut >= 1                                                   # (dropping a name did move a boundary)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_forward_pass_agrees_with_itself_section_by_section(seed):
    info = R2.build(seed)
    x = info["x"][:3]
    vals = info["forward"](x)
    sections = R2.reference_partition(info, R2.cut_flags(seed))
    variable = lambda i: [t for t in info["ops"][i][0] if t >= 0 and t not in info["constants"]]
    ran = set()

    def run_section(k, arrays):
        members, ins, outs = sections[k]
        ran.add(k)
        inner = dict(zip(ins, arrays))
        for j in members:
            inner[info["ops"][j][1][0]] = info["host"][j](*[inner[t] for t in variable(j)])
        return [inner[t] for t in outs]
    live = R2.run_cut(info, sections, x, run_section)
    assert set(info["outputs"]) <= set(live) and len(ran) == len(sections)
    for t, v in live.items():
        assert v.dtype == vals[t].dtype and np.array_equal(v.view(np.uint8), vals[t].view(np.uint8)), t


def test_the_kept_seeds_are_what_the_conditions_keep_and_cover_every_feature_pass_and_pair():
    kept = tuple(s for s in range(R2.CANDIDATES) if not R2.violations(R2.build(s)))
    assert kept == R2.SEEDS
    assert 4 * (R2.CANDIDATES - len(kept)) <= R2.CANDIDATES
    features, passes, pairs = collections.Counter(), collections.Counter(), collections.Counter()
    for s in R2.SEEDS:
        info = R2.build(s)
        features.update(k for k, v in info["features"].items() if v)
        passes.update(set(info["names"]))
        pairs.update(info["pairs"])
    print("features", dict(sorted(features.items())), "passes", {k: passes[k] for k in P2.PASSES + P2.P.LCE_OPS})
    print("pairs", {"%s>%s" % k: v for k, v in sorted(pairs.items())})
    assert all(features[k] >= 5 for k in R2.FEATURES), features
    assert all(features[k] >= 5 for k in R2.JOIN_FEATURES), features
    assert all(passes[k] >= 5 for k in P2.PASSES), passes
    assert all(features[k] >= 2 for k in R2.VARIANTS), features      # (l_cap: a chain with activations on both sides of the cap's cut)
    assert all(features[k] >= 1 for k in R2.CLAMPS), features        # int8 RELU, RELU_N1_TO_1 and RELU6 steps
    assert len(pairs) >= 10, pairs
    # the shapes stay small; 6 to 24 operators (generation 1: 20 -- a gate block alone is six)
    for s in R2.SEEDS:
        info = R2.build(s)
        assert 6 <= len(info["ops"]) <= R2.MAX_OPS == 24 and info["x"].shape[0] == info["batch"] + 2 <= 10
        assert all(5 <= d <= 12 for d in info["x"].shape[1:3])
