"""The `slice` pass on the MI355X, byte for byte: the MeliusNet-style fixtures of tests/slice_models.py run as ONE section -- every
improvement block one lce_hip_join_windows launch -- against their NumPy forward pass and against the same file cut at the slices
with NumPy doing them; the variants that must NOT fold (a delivered slice, two readers, a fused RELU, an addend from the chain);
predict() with a ragged last batch; and HIP-graph replay."""
import importlib

import numpy as np
import pytest

import slice_models as SM

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(a, b):
    raw = lambda v: np.ascontiguousarray(v).view(np.int32) if v.dtype == np.float32 else v
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def image(net, batch, seed):
    g = np.random.default_rng(seed)
    if net.i8:
        return g.integers(-128, 128, (batch, net.H, net.H, 64), dtype=np.int64).astype(np.int8)
    return g.standard_normal((batch, net.H, net.H, 64)).astype(np.float32)


def run_cut(data, net, x, **names):
    """The file at the partition `names` give, section by section on the GPU, every operator outside the sections by its NumPy
    restatement.  Returns tensor -> array for every tensor that crossed the host."""
    it = mr.Interpreter(data, batch_size=x.shape[0], **names)
    section_of = {op: k for k, sec in enumerate(it.sections) for op in sec.ops}
    live, ran = {net.x0: x}, set()
    for i in range(len(it.model.operators)):
        if i in section_of:
            k = section_of[i]
            if k not in ran:
                ran.add(k)
                live.update(zip(it.sections[k].outputs, it.run_section(k, [live[t] for t in it.sections[k].inputs])))
        else:
            ins, out, fn = net.run[i]
            live[out] = fn(*[live[t] for t in ins])
    assert len(ran) == len(it.sections) > 1
    return live


@pytest.mark.parametrize("batch", [1, 3, 64])
def test_the_float_body_runs_as_one_section_with_one_launch_per_improvement_block(batch):
    data, net, out = SM.meliusnet_model()
    x = image(net, batch, batch)
    want = net.forward(x)[out]
    it = mr.Interpreter(data, batch_size=batch, **SM.FLOAT_NAMES)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert same(got, want)
    # two improvement blocks: two launches, both took over a CONCATENATION, nothing folds (a batch norm reads every join);
    # lce_hip_concat ran the two dense blocks' joins only; every batch norm is one chain of two operators
    assert it.model.slice_stats() == (2, 0, 2)
    assert it.model.concat_stats() == (2, 0)
    assert it.model.elementwise_stats() == (4, 8, 4)
    cut = run_cut(data, net, x, elementwise_sections=True, concat_sections=True)
    assert same(cut[out], got)
    if batch == 3:
        assert same(it.predict(x), want)


@pytest.mark.parametrize("batch", [3, 64])
def test_the_int8_body(batch):
    data, net, out = SM.meliusnet_model(np.int8)
    x = image(net, batch, batch + 7)
    want = net.forward(x)[out]
    it = mr.Interpreter(data, batch_size=batch, **SM.INT8_NAMES)
    assert len(it.sections) == 1 and it.lce_only
    (got,) = it.run_section(0, [x])
    assert same(got, want) and np.unique(want).size > 20
    # per improvement block the `b` slice runs standalone into the int8 ADD and the `f` slice folds into the join; every join is
    # read by an LceQuantize, the last one by nothing else
    assert it.model.slice_stats() == (4, 2, 2)
    assert it.model.concat_stats() == (2, 2) and it.model.int8_add_stats() == (2, 0)
    cut = run_cut(data, net, x, int8_add_sections=True, concat_sections=True)
    assert same(cut[out], got)


@pytest.mark.parametrize("case", SM.VARIANTS)
def test_each_variant_gives_the_right_bytes_and_launches(case):
    data, net, outs = SM.variant_model(case)
    x = image(net, 3, len(case))
    live = net.forward(x)
    it = mr.Interpreter(data, batch_size=3, **SM.FLOAT_NAMES)
    assert len(it.sections) == 1 and it.sections[0].outputs == sorted(outs)
    got = it.run_section(0, [x])
    for t, y in zip(it.sections[0].outputs, got):
        assert same(y, live[t]), (case, t)
    slices, concats, chains = SM.VARIANT_STATS[case]
    assert it.model.slice_stats() == slices and it.model.concat_stats()[0] == concats and it.model.elementwise_stats()[0] == chains


def test_predict_with_a_ragged_last_batch():
    data, net, out = SM.meliusnet_model()
    x = image(net, 11, 5)
    it = mr.Interpreter(data, batch_size=4, **SM.FLOAT_NAMES)
    assert same(it.predict(x), net.forward(x)[out])


def test_hip_graph_replay_gives_the_same_bytes_and_allocates_nothing():
    data, net, out = SM.meliusnet_model()
    model = mr.LceModel(data, **SM.FLOAT_NAMES)
    batch = 5
    x = torch.from_numpy(image(net, batch, 11)).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    y = torch.zeros(dims, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(s):
        model.use_hip_graphs(True)
        for _ in range(3):                                            # eager, then recorded, then replayed
            y.zero_()
            model.run_section(0, batch, [x.data_ptr()], [y.data_ptr()], s.cuda_stream)
            s.synchronize()
            runs.append((y.clone(), model.slice_stats(), model.graph_stats(), model.run_stats()[2]))
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]            # (a recording fails if anything is allocated inside it)
    assert [r[1] for r in runs] == [(2, 0, 2)] * 3
    assert runs[0][3] == runs[1][3] == runs[2][3]                     # the scratch buffers of the eager run serve all three
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))
    assert same(runs[2][0].cpu().numpy(), net.forward(x.cpu().numpy())[out])
    model.use_hip_graphs(False)
