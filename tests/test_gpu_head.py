"""The classifier head on the MI355X, exact and without tolerance: lce_hip_fully_connected_f32 and lce_hip_softmax_f32 against
tests/head_ref.py on the grids of tests/test_head_host.py (both load paths, special values, in place), the fully connected
kernel against lce_hip_conv1x1_f32 on the same operands (one shape with ragged last tiles, one with more tiles than one pass of
the grid), the refusals of both entries, and QuickNet-shaped networks run as ONE section from the image to the probabilities --
run_section, predict through its pipeline, keep_dims, a head that is a section of its own, HIP-graph replay -- against the
restated chain.  NaN positions are compared as positions, every other byte as a byte."""
import importlib

import numpy as np
import pytest

import conv1x1_ref as CR
import head_models as HM
import head_ref as HR
from test_head_host import ACTS, FC_BATCHES, FC_K, FC_N, SM_BETAS, SM_COLS, SM_ROWS, agree, fc_operands, softmax_rows, softmax_tolerance

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, offset=0):
    """`a` on the device; `offset`: its first byte that many floats behind an allocation's (256-byte aligned) start."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=torch.float32, device=DEV)
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want):
    return got.dtype == want.dtype and agree(got, want)


# ---- the two entries against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FC_K)
def test_fully_connected_gives_the_reference_bytes(k):
    n_checks = 0
    for batch in FC_BATCHES:
        x, w, bias = fc_operands(batch, k, max(FC_N))
        t = CR.chain(x, w)
        for offset in (0, 1):                                        # 16-byte loads (when k % 4 == 0) and dword loads
            xd, wd, bd = dev(x, offset), dev(w, offset), dev(bias)
            for n in FC_N:
                for act in ACTS:
                    for with_bias in (True, False):
                        with np.errstate(invalid="ignore", over="ignore"):
                            want = CR.clamp(t[:, :n] + bias[None, :n] if with_bias else t[:, :n], act)
                        got = amd.fully_connected(xd, wd[:n], bd[:n] if with_bias else None, activation=act)
                        assert same(host(got), want), (batch, k, n, act, with_bias, offset)
                        n_checks += 1
    assert n_checks == 3 * 2 * 4 * 4 * 2


@pytest.mark.parametrize("k", [6, 32, 70])
def test_fully_connected_on_special_values(k):
    for batch, n in ((3, 33), (33, 31)):
        x, w, bias = fc_operands(batch, k, n, seed=5, special=True)
        want = HR.fully_connected(x, w, bias, HR.NONE)
        for offset in (0, 1):
            assert same(host(amd.fully_connected(dev(x, offset), dev(w, offset), dev(bias))), want), (batch, k, n, offset)
    x, w, bias = fc_operands(3, k, 33)
    assert same(amd.fully_connected(x, w, bias, activation=amd.ACT_RELU6), HR.fully_connected(x, w, bias, HR.RELU6))   # NumPy in, NumPy out


@pytest.mark.parametrize("batch,k,n", [(33, 70, 1000), (3, 512, 70), (17, 65, 33), (1040, 3, 2032)])
def test_fully_connected_is_conv1x1_on_a_one_pixel_image(batch, k, n):
    """(33, 70, 1000): 3 x 63 tiles, the last row and column tiles ragged, a K tail; (1040, 3, 2032): 65 x 127 = 8255 tiles
    against the 8192 waves of one pass of the grid."""
    x, w, bias = fc_operands(batch, k, n, seed=9)
    xd, wd, bd = dev(x), dev(w), dev(bias)
    for act, b in ((amd.ACT_NONE, bd), (amd.ACT_RELU6, None)):
        conv, _ = amd.conv1x1(xd.view(batch, 1, 1, k), wd, b, activation=act)
        got = amd.fully_connected(xd, wd, b, activation=act)
        assert torch.equal(got.view(torch.int32), conv.view(batch, n).view(torch.int32)), (batch, k, n, act)
    if batch * n * k < 3_000_000:
        assert same(host(got), HR.fully_connected(x, w, None, HR.RELU6))
    out = torch.full((batch, n), 7.0, device=DEV)
    assert amd.fully_connected(xd, wd, bd, out=out) is out
    conv, _ = amd.conv1x1(xd.view(batch, 1, 1, k), wd, bd)
    assert torch.equal(out.view(torch.int32), conv.view(batch, n).view(torch.int32))


@pytest.mark.parametrize("cols", SM_COLS)
def test_softmax_gives_the_reference_bytes(cols):
    for rows in SM_ROWS:
        x = softmax_rows(rows, cols)
        for beta in SM_BETAS:
            want = HR.softmax(x, beta)
            for offset in (0, 1):
                xd = dev(x, offset)
                got = amd.softmax(xd, beta)
                assert same(host(got), want), (rows, cols, beta, offset)
                assert torch.equal(xd, dev(x))                       # the input is untouched
                assert amd.softmax(xd, beta, out=xd) is xd and same(host(xd), want), (rows, cols, beta, offset, "in place")
    x = softmax_rows(5, cols).reshape(5, 1, 1, cols)
    assert same(amd.softmax(x, 0.5), HR.softmax(x, 0.5))             # NumPy in, NumPy out; any leading shape


def test_softmax_of_many_rows_and_of_rows_with_nan():
    """9000 rows: more than one pass of the grid's 8192 waves.  Rows with NaN or infinity do not fault and leave the others alone."""
    x = (np.random.default_rng(3).standard_normal((9000, 10)) * 4).astype(np.float32)
    assert same(host(amd.softmax(dev(x))), HR.softmax(x))
    x[5, 3], x[77, 0], x[8999, 9] = np.nan, np.inf, -np.inf
    got = host(amd.softmax(dev(x)))
    finite = np.isfinite(x).all(axis=1)
    assert same(got[finite], HR.softmax(x[finite]))


# ---- the refusals, on the device -------------------------------------------------------------------------------------------------------
def test_the_entries_refuse_on_the_device():
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    x, w = buf[:64].view(4, 16), buf[64:144].view(5, 16)
    for out, what in ((buf[32:52].view(4, 5), "input"), (buf[140:160].view(4, 5), "filter")):
        with pytest.raises(amd.LceHipError, match="overlaps the " + what):
            amd.fully_connected(x, w, out=out)
    with pytest.raises(amd.LceHipError, match="overlaps the bias"):
        amd.fully_connected(x, w, buf[200:205], out=buf[202:222].view(4, 5))
    with pytest.raises(amd.LceHipError, match="partly overlaps"):
        amd.softmax(x, out=buf[16:80].view(4, 16))
    l = amd.lib()
    d = amd.FcDesc(4, 16, 5, 7)
    assert l.lce_hip_fully_connected_f32(d, x.data_ptr(), w.data_ptr(), None, buf[1000:].data_ptr(), None) == amd.ERR_INVALID
    assert l.lce_hip_softmax_f32(4, 16, float("nan"), x.data_ptr(), buf[1000:].data_ptr(), None) == amd.ERR_INVALID
    assert l.lce_hip_softmax_f32(4, 16, 1.0, x.data_ptr() + 2, buf[1000:].data_ptr(), None) == amd.ERR_INVALID
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                             # nothing was launched


# ---- a whole network ---------------------------------------------------------------------------------------------------------------------
def images(n, shape, seed):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(shape)).astype(np.float32)


def sums_to_one(p, logits, beta):
    """Each row of probabilities sums to 1 within the sum of the per-element bounds tests/test_head_host.py derives."""
    _, tol = softmax_tolerance(logits, beta)
    return bool((np.abs(p.astype(np.float64).sum(axis=1) - 1.0) <= tol.sum(axis=1)).all())


@pytest.mark.parametrize("keep_dims", [False, True])
def test_a_quicknet_shaped_network_runs_from_the_image_to_the_probabilities(keep_dims):
    data, xt, out, info = HM.quicknet_head_model(keep_dims=keep_dims)
    hi = info["head"]
    it = mr.Interpreter(data, batch_size=2, **HM.EVERY_FLAG)
    assert len(it.sections) == 1 and it.lce_only
    x = images(5, info["shape"], 17)
    body = HM.body_forward(x, info)
    logits = HR.fully_connected(HR.mean_hw(body), hi["w"], hi["wb"], hi["activation"])
    want = HR.softmax(logits, hi["beta"])
    for batch in (1, 3):
        (got,) = it.run_section(0, [x[:batch]])
        assert got.shape == (batch, 10) and same(got, want[:batch]), batch
        assert it.model.head_stats() == (1, 1, 1)
        assert it.model.conv2d_stats()[0] == 1 and it.model.elementwise_stats()[0] == 2
    got = it.predict(x)                                              # three passes of the pipeline, the last one short
    assert got.shape == (5, 10) and same(got, want)
    assert it.model.head_stats() == (1, 1, 1)
    assert sums_to_one(got, logits, hi["beta"]) and (got >= 0).all()
    # the same file with the head left to the host: the section delivers the map the head reads
    body_only = mr.Interpreter(data, **HM.ALL_FLAGS)
    (delivered,) = body_only.run_section(0, [x])
    assert same(delivered, body) and same(HM.head_forward(delivered, hi), got)


def test_a_head_that_is_a_section_of_its_own():
    data, xt, out, info = HM.head_only_model()
    hi = info["head"]
    it = mr.Interpreter(data, **HM.EVERY_FLAG)
    assert [s.ops for s in it.sections] == [[hi["mean"], hi["fc"], hi["softmax"]]] and not it.lce_only
    t = np.tanh(images(4, info["shape"], 23)).astype(np.float32)     # the host's operator
    for batch in (1, 4):
        (got,) = it.run_section(0, [t[:batch]])
        assert got.shape == (batch, 7) and same(got, HM.head_forward(t[:batch], hi))
        assert it.model.head_stats() == (1, 1, 1)
    with pytest.raises(NotImplementedError):
        it.predict(t)


def test_hip_graph_replay_gives_the_same_bytes():
    data, xt, out, info = HM.quicknet_head_model()
    model = mr.LceModel(data, **HM.EVERY_FLAG)
    batch = 3
    xh = images(batch, info["shape"], 29)
    x = torch.from_numpy(xh).to(DEV)
    dims, _ = model.section_tensor_shape(0, out, batch)
    assert dims == (batch, 1, 1, 10)
    y = torch.zeros(dims, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(s):
        model.use_hip_graphs(True)
        for _ in range(3):                                           # eager, then recorded, then replayed
            y.zero_()
            model.run_section(0, batch, [x.data_ptr()], [y.data_ptr()], s.cuda_stream)
            s.synchronize()
            runs.append((y.clone(), model.head_stats(), model.graph_stats()))
    assert [r[2] for r in runs] == [(0, 0), (1, 1), (1, 2)]
    assert [r[1] for r in runs] == [(1, 1, 1)] * 3
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))
    assert same(runs[2][0].cpu().numpy().reshape(batch, 10), HM.quicknet_forward(xh, info))
    model.use_hip_graphs(False)
