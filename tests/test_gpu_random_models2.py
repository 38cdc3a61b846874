"""Generation 2 of the random mixed networks (tests/random_models2.py) through all 25 rows of the pass table and the "transition"
fusion on the MI355X, byte for byte and without tolerance against the composed NumPy restatements, as
tests/test_gpu_random_models.py does it for generation 1: each kept seed as ONE section through predict() and run_section(), with
all the launch counters -- generation 1's and the eight newer tuples -- against tests/partition_ref2.py; every third seed cut into
sections by the seed's own subset of the keywords and passes= names, with NumPy doing the operators between and every tensor that
crosses the host compared; and four seeds recorded into a HIP graph and replayed on new input contents.

A longer hunt on a GPU machine: LCE_FUZZ_SEED=1 LCE_FUZZ_EXAMPLES=500 python -m pytest <this file> appends freshly drawn seeds,
kept under the same conditions and the same drop cap."""
import collections
import importlib

import numpy as np
import pytest

import partition_ref2 as P2
import random_models2 as R2

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = list(R2.SEEDS) + R2.fuzz_seeds()
CUT_SEEDS = SEEDS[::3]
# a fused transition, an int8 gate with a rider, a slice that took over a join, a binary Dense layer (a test below checks that they
# hold them: written out, so that collecting this file builds no model)
GRAPH_SEEDS = [0, 24, 3, 2]
_launched, _folded, _special, _models = collections.Counter(), collections.Counter(), collections.Counter(), [0]
# the passes that can write bits, but for the int8 LOGISTIC: its output is never below its zero point of -128, so the LceQuantize
# behind it would write zeros only and the conditions on a draw drop such a seed (tests/test_gpu_gate_i8.py covers that fold)
FOLDERS = tuple(p for p in P2.FOLDING if p != "logistic_i8")


def interpreter(info, flags, batch):
    passes, keywords = R2.model_args(flags)
    return mr.Interpreter(info["data"], batch_size=batch, passes=passes, **keywords)


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    a, b = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert np.array_equal(a, b), (what, int(np.sum(a != b)), got.size)


def count(walk):
    for name in P2.PASSES:
        _launched[name] += walk["passes"][name]
        _folded[name] += walk["folded"][name]
    _launched["reshape"] += walk["views"] + walk["copies"]
    _launched["pool"] += walk["transition"][0]                        # (a fused pair launched its pool and its blur)
    _launched["depthwise"] += walk["transition"][0]
    _folded["LceBconv2d"] += walk["conv_quantize"]
    _folded["transition"] += walk["transition"][2]
    for k, v in (("head", walk["heads"]), ("rider", walk["riders"]), ("take_over", walk["joins"]), ("skipped", walk["dequantize_skipped"]),
                 ("transition", walk["transition"][0])):
        _special[k] += v


@pytest.mark.parametrize("seed", SEEDS)
def test_one_section_equals_the_forward_pass(seed):
    info = R2.build(seed)
    x = info["x"]
    assert x.shape[0] == info["batch"] + 2                            # a ragged last batch
    if info["types"][info["input"]] == "i8":
        assert x.min() == -128 and x.max() == 127
    else:
        assert np.signbit(x[x == 0]).any() and np.isnan(x).any() == info["nan_ok"]
    want = info["forward"](x)
    it = interpreter(info, R2.EVERY_FLAG, info["batch"])
    assert it.lce_only and len(it.sections) == 1
    got = it.predict(x)
    got = list(got) if isinstance(got, (list, tuple)) else [got]
    assert len(got) == len(info["outputs"])
    for t, g in zip(info["outputs"], got):
        assert_same(g, want[t], ("predict", seed, t, info["names"]))
    expected = R2.expected_stats(info)
    assert R2.model_stats(it.model) == expected
    got = it.run_section(0, [x])
    assert it.sections[0].outputs == sorted(info["outputs"])
    for t, g in zip(it.sections[0].outputs, got):
        assert_same(g, want[t], ("run_section", seed, t))
    assert R2.model_stats(it.model) == expected
    count(info["walk"])
    _models[0] += 1


@pytest.mark.parametrize("seed", CUT_SEEDS)
def test_the_file_cut_by_dropped_names_equals_the_forward_pass_at_every_boundary(seed):
    info = R2.build(seed)
    flags = R2.cut_flags(seed)
    x = info["x"]
    want = info["forward"](x)
    sections = R2.reference_partition(info, flags)
    it = interpreter(info, flags, x.shape[0])
    assert [(s.ops, s.inputs, s.outputs) for s in it.sections] == sections
    ran = []

    def run_section(k, arrays):
        outs = it.run_section(k, arrays)
        assert R2.model_stats(it.model) == R2.expected_stats(info, flags, k), (seed, k)
        ran.append(k)
        return outs
    live = R2.run_cut(info, sections, x, run_section)
    assert sorted(ran) == list(range(len(sections))) and set(info["outputs"]) <= set(live)
    for t, v in sorted(live.items()):
        assert_same(v, want[t], ("cut", seed, t, sorted(set(R2.EVERY_FLAG) - set(flags))))


@pytest.mark.parametrize("seed", GRAPH_SEEDS)
def test_hip_graph_replay_of_a_random_section_gives_the_same_bytes(seed):
    info = R2.build(seed)
    passes, keywords = R2.model_args(R2.EVERY_FLAG)
    model = mr.LceModel(info["data"], passes=passes, **keywords)
    outs = model.sections[0].outputs
    xs = [info["x"], np.ascontiguousarray(info["x"][::-1])]
    batch = xs[0].shape[0]
    x = torch.from_numpy(xs[0]).to(DEV)
    dt = dict(f32=torch.float32, i8=torch.int8, bits=torch.int32)
    ys = [torch.zeros(model.section_tensor_shape(0, t, batch)[0], dtype=dt[info["types"][t]], device=DEV) for t in outs]
    s = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(s):
        model.use_hip_graphs(True)
        for k in range(3):                                            # eager, then recorded, then replayed on new contents
            x.copy_(torch.from_numpy(xs[k // 2]))
            for y in ys:
                y.zero_()
            s.synchronize()
            model.run_section(0, batch, [x.data_ptr()], [y.data_ptr() for y in ys], s.cuda_stream)
            s.synchronize()
            runs.append(([y.cpu().numpy() for y in ys], R2.model_stats(model), model.graph_stats()))
    model.use_hip_graphs(False)
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1] for r in runs] == [R2.expected_stats(info)] * 3
    for k, r in enumerate(runs):
        want = info["forward"](xs[k // 2])
        for t, g in zip(outs, r[0]):
            assert_same(g.reshape(want[t].shape), want[t], ("graph", seed, k, t))
    assert not np.array_equal(runs[1][0][0], runs[2][0][0])


def test_the_graph_seeds_hold_a_transition_a_rider_a_taken_over_join_and_a_binary_dense_layer():
    assert len(GRAPH_SEEDS) == 4 and len(set(GRAPH_SEEDS)) == 4 and set(GRAPH_SEEDS) <= set(R2.SEEDS)
    walks = [R2.build(s)["walk"] for s in GRAPH_SEEDS]
    assert walks[0]["transition"][0] >= 1
    assert walks[1]["riders"] >= 1 and "logistic_i8" in R2.build(GRAPH_SEEDS[1])["names"]
    assert walks[2]["joins"] >= 1
    assert walks[3]["passes"]["binary_dense"] >= 1


def test_the_conditions_drop_at_most_one_fuzz_seed_in_four():
    dropped, drawn = R2.fuzz_dropped()
    assert 4 * dropped <= drawn, (dropped, drawn)


def test_random_models_launched_every_pass_and_folded_a_quantize_into_each():
    """(same process, after the seeds) every one of the 25 passes launched (RESHAPE: ran), every pass the generator grows an
    LceQuantize behind, LceBconv2d and the fused transition wrote the bits of one, and a head ADD, a rider ADD, a taken-over
    CONCATENATION, an LceDequantize that was not launched and a fused transition were each counted at least once -- by the
    restated walk, which the seeds' tests found equal to the library's counters."""
    if _models[0] < len(R2.SEEDS):
        pytest.skip("the seeds did not all run in this process")
    assert all(_launched[name] >= 1 for name in P2.PASSES), _launched
    assert all(_folded[name] >= 1 for name in FOLDERS + ("LceBconv2d", "transition")), _folded
    assert all(_special[k] >= 1 for k in ("head", "rider", "take_over", "skipped", "transition")), _special
