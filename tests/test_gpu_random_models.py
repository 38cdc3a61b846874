"""Random mixed float / int8 networks (tests/random_models.py) through every fused pass of the section runner on the MI355X, byte
for byte and without tolerance against the composed NumPy restatements: each kept seed as ONE section through predict() (true
batches with a ragged last one) and run_section(), with the launch counters against tests/partition_ref.py; a fixed third of the
seeds cut into sections by the seed's own subset of the keywords, with NumPy doing the operators between and every tensor that
crosses the host compared; and four seeds recorded into a HIP graph and replayed on new input contents.

A longer hunt on a GPU machine: LCE_FUZZ_SEED=1 LCE_FUZZ_EXAMPLES=500 python -m pytest <this file> appends freshly drawn seeds (either
variable alone starts a hunt, as in tests/test_gpu_model_random.py), kept under the same conditions and the same drop cap."""
import collections
import importlib

import numpy as np
import pytest

import partition_ref as P
import random_models as RM

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = list(RM.SEEDS) + RM.fuzz_seeds()
CUT_SEEDS = SEEDS[::3]
_with = lambda name: [s for s in RM.SEEDS if name in RM.build(s)["names"]][:2]
GRAPH_SEEDS = _with("softmax") + _with("softmax_i8")
_launched, _folded, _models = collections.Counter(), collections.Counter(), [0]


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    same = np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    assert same, (what, int(np.sum(np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8))), got.size)


def count(stats):
    for name in P.FOLDING:
        _launched[name] += stats[name][0]
        _folded[name] += stats[name][-1]
    for group, names in (("head", P.HEADS[:3]), ("head_i8", P.HEADS[3:]), ("quantize", ("quantize", "dequantize"))):
        for name, n in zip(names, stats[group]):
            _launched[name] += n
    _folded["LceBconv2d"] += stats["fused_quantize"]


@pytest.mark.parametrize("seed", SEEDS)
def test_one_section_equals_the_forward_pass(seed):
    info = RM.build(seed)
    x = info["x"]
    assert x.shape[0] == info["batch"] + 2                            # a ragged last batch
    if info["types"][info["input"]] == "i8":
        assert x.min() == -128 and x.max() == 127
    else:
        assert np.signbit(x[x == 0]).any() and np.isnan(x).any() == info["nan_ok"]
    want = info["forward"](x)
    it = mr.Interpreter(info["data"], batch_size=info["batch"], **RM.EVERY_FLAG)
    assert it.lce_only and len(it.sections) == 1
    got = it.predict(x)
    got = list(got) if isinstance(got, (list, tuple)) else [got]
    assert len(got) == len(info["outputs"])
    for t, g in zip(info["outputs"], got):
        assert_same(g, want[t], ("predict", seed, t, info["names"]))
    expected = RM.expected_stats(info)
    assert RM.model_stats(it.model) == expected
    got = it.run_section(0, [x])
    assert it.sections[0].outputs == sorted(info["outputs"])
    for t, g in zip(it.sections[0].outputs, got):
        assert_same(g, want[t], ("run_section", seed, t))
    assert RM.model_stats(it.model) == expected
    count(expected)
    _models[0] += 1


@pytest.mark.parametrize("seed", CUT_SEEDS)
def test_the_file_cut_by_dropped_keywords_equals_the_forward_pass_at_every_boundary(seed):
    info = RM.build(seed)
    flags = RM.cut_flags(seed)
    x = info["x"]
    want = info["forward"](x)
    sections = RM.reference_partition(info, flags)
    it = mr.Interpreter(info["data"], batch_size=x.shape[0], **flags)
    assert [(s.ops, s.inputs, s.outputs) for s in it.sections] == sections
    ran = []

    def run_section(k, arrays):
        outs = it.run_section(k, arrays)
        assert RM.model_stats(it.model) == RM.expected_stats(info, flags, k), (seed, k)
        ran.append(k)
        return outs
    live = RM.run_cut(info, sections, x, run_section)
    assert sorted(ran) == list(range(len(sections))) and set(info["outputs"]) <= set(live)
    for t, v in sorted(live.items()):
        assert_same(v, want[t], ("cut", seed, t, sorted(set(RM.EVERY_FLAG) - set(flags))))


@pytest.mark.parametrize("seed", GRAPH_SEEDS)
def test_hip_graph_replay_of_a_random_section_gives_the_same_bytes(seed):
    info = RM.build(seed)
    model = mr.LceModel(info["data"], **RM.EVERY_FLAG)
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
            runs.append(([y.cpu().numpy() for y in ys], RM.model_stats(model), model.graph_stats()))
    model.use_hip_graphs(False)
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1] for r in runs] == [RM.expected_stats(info)] * 3
    for k, r in enumerate(runs):
        want = info["forward"](xs[k // 2])
        for t, g in zip(outs, r[0]):
            assert_same(g.reshape(want[t].shape), want[t], ("graph", seed, k, t))
    assert not np.array_equal(runs[1][0][0], runs[2][0][0])


def test_the_graph_seeds_hold_a_float_and_an_int8_head():
    assert len(GRAPH_SEEDS) == 4 and len(set(GRAPH_SEEDS)) == 4


def test_the_conditions_drop_at_most_one_fuzz_seed_in_four():
    dropped, drawn = RM.fuzz_dropped()
    assert 4 * dropped <= drawn, (dropped, drawn)


def test_random_models_launched_every_pass_and_folded_a_quantize_into_each():
    """(same process, after the seeds) every one of the seventeen passes launched, and every pass with a bit output, and
    LceBconv2d, wrote the bits of an LceQuantize at least once."""
    if _models[0] < len(RM.SEEDS):
        pytest.skip("the seeds did not all run in this process")
    assert all(_launched[name] >= 1 for name in P.PASSES), _launched
    assert all(_folded[name] >= 1 for name in P.FOLDING + ("LceBconv2d",)), _folded
