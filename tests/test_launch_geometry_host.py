"""The streaming kernels' launch geometry at 512 .. 2048 images per GPU, on the CPU (tests/launch_geometry.py):

* LONG_RUN_CASES, the literal table the GPU tests run, IS the host planner's answer: regenerating it reproduces it, and every entry
  gives a block the work of the big launch it stands for;
* what the table covers is stated: every (layer, output type, 512 / 1024 / 2048) cell's own choice is in it or is a block-GEMM
  kernel, and the long-run features the kernels can go wrong on each occur;
* every entry, and every seeded draw of forced geometry options that the planner accepts, runs in the host simulation (the real
  kernel bodies, thread by thread) to the oracle's bytes, both outputs, nothing written outside them."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hostsim_lib as H
import launch_geometry as L
import oracle_lib as O


# ------------------------------------------------------------------------------------ the table is the planner's answer

def _small_plan(case):
    return L.plan_fields(L.case_spec(case), L.DST_OF[case[6]], case[7])


def _big_plan(case):
    batch, h, w, cin, cout, stride, dst, options, kernel, big_batch, big_opts = case
    return L.plan_fields(L.layer_spec(big_batch, h, w, cin, cout, stride), L.DST_OF[dst], big_opts + ";compute_units=%d" % L.BIG_CUS)


def test_the_table_is_what_scale_down_returns():
    """A planner change that moves the geometry at 512 .. 2048 images fails here and says which entries to regenerate
    (python -c "import launch_geometry as L; [print('    %r,' % (c,)) for c in L.generate_long_run_cases()]" from tests/)."""
    fresh = L.generate_long_run_cases()
    gone = [L.case_id(c) for c in L.LONG_RUN_CASES if c not in fresh]
    new = [c for c in fresh if c not in L.LONG_RUN_CASES]
    assert not gone and not new, "LONG_RUN_CASES is stale.\n  no longer generated: %s\n  missing: %s" % (gone, new)
    assert fresh == L.LONG_RUN_CASES, "the same entries in another order"
    assert len(set(map(L.case_id, L.LONG_RUN_CASES))) == len(L.LONG_RUN_CASES)


@pytest.mark.parametrize("index", range(len(L.LONG_RUN_CASES)), ids=lambda i: L.case_id(L.LONG_RUN_CASES[i]))
def test_an_entry_gives_a_block_the_work_of_the_big_launch(index):
    case = L.LONG_RUN_CASES[index]
    small, big = _small_plan(case), _big_plan(case)
    assert small["err"] == "" and big["err"] == ""
    assert small["kernel"] == case[8]
    assert L.per_block(small) == L.per_block(big) and L.per_block(small) is not None
    assert L.blocks_in_x(small) >= 2
    assert big["num_cus"] == L.BIG_CUS and big["chunk"] == case[9]


# ------------------------------------------------------------------------------------ coverage is stated

def test_every_cell_is_covered_or_a_block_gemm():
    """For the 7 layers x 3 output types x (512, 1024, 2048): the planner's own choice (engine=auto, 256 CUs) is a streaming kernel whose
    per-block work some entry has, or a block-GEMM kernel (listed with -rA)."""
    have = [L.per_block(_small_plan(c)) for c in L.LONG_RUN_CASES]
    gemm = []
    for layer in L.LAYERS:
        for dst in L.DST_NAMES:
            for big_batch in L.BIG_BATCHES:
                f = L.big_plan((layer, dst, big_batch, "auto", ""))
                assert f["err"] == "", (layer, dst, big_batch, f["err"])
                pb = L.per_block(f)
                if pb is None:
                    assert f["kernel"].startswith("bconv2d_mfma"), (layer, dst, big_batch, f["kernel"])
                    gemm.append("%dx%dx%d->%d s%d %s @%d: %s" % (layer[0], layer[0], layer[1], layer[2], layer[3], dst, big_batch, f["kernel"]))
                else:
                    assert pb in have, (layer, dst, big_batch, f["kernel"])
    print("block-GEMM cells (%d of %d):" % (len(gemm), len(L.LAYERS) * 9))
    for line in gemm:
        print("  " + line)
    assert len(gemm) < len(L.LAYERS) * 9


def test_the_long_run_features_each_occur():
    plans = [(c, _small_plan(c)) for c in L.LONG_RUN_CASES]
    stream = [(c, f) for c, f in plans if L.family(f) == "stream"]
    wstream = [(c, f) for c, f in plans if L.family(f) == "wstream"]
    whole_image = lambda c, f: f["st_rs"] == f["out_h"] and not f["st_flat"]
    features = {
        "interleaved runs of >= 28 segments per block": [c for c, f in stream if f["st_gstr"] > 1 and f["st_spb"] >= 28],
        "8 whole images per block": [c for c, f in stream if whole_image(c, f) and f["st_spb"] == 8],
        "a flat run (7x7) with an uneven last run": [c for c, f in stream if f["st_flat"] and c[1] == 7 and not L.full_runs(f)],
        "two blocks per CU with >= 4 segments per block": [c for c, f in stream if f["st_occ"] == 2 and f["st_spb"] >= 4 and c[6] == "bp" and c[3] == 64],
        "wstream with two images resident": [c for c, f in wstream if f["ws_ipb"] == 2],
        "wstream whose last group has one image": [c for c, f in wstream if f["ws_ipb"] == 2 and c[0] % 2 == 1],
        "stride 2": [c for c in L.LONG_RUN_CASES if c[5] == 2],
    }
    for chunks in (64, 128, 256, 512):
        features["the %d-channel instance" % chunks] = [c for c in L.LONG_RUN_CASES if "3x3x%d," % chunks in c[8]]
    for family in ("bconv2d_stream<", "bconv2d_wstream<"):
        for dst in ("f32", "i8", "bitpacked"):
            features[family + dst] = [c for c in L.LONG_RUN_CASES if c[8].startswith(family + dst)]
    features["an uneven last run of consecutive segments"] = [c for c, f in stream if f["st_gstr"] == 1 and not f["st_flat"] and not L.full_runs(f)]
    missing = [name for name, cases in features.items() if not cases]
    assert not missing, missing


# ------------------------------------------------------------------------------------ every entry in the host simulation

GUARD = 64


def _guarded(shape, dtype):
    """(buffer, view): `view` is an array of `shape` 64 bytes into a buffer poisoned with 0x5A, 64 more bytes behind it."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = np.full(n + 2 * GUARD, 0x5A, np.uint8)
    return buf, buf[GUARD:GUARD + n].view(dtype).reshape(shape)


def _simulate(spec, dst, options, ops, kernel=None, max_batch=0):
    """The host simulation of the plan against the oracle: the output on all images, the second output (float / int8 plans), the guard
    bytes around both."""
    odst = L.DST_OF[dst]
    out_buf, out = _guarded(spec.output_shape(odst), {"f32": np.float32, "i8": np.int8, "bp": np.int32}[dst])
    bits_buf, bits = _guarded(spec.output_shape(O.DST_BITPACKED), np.int32) if dst != "bp" else (None, None)
    opts = L.option_dict(options)
    got, name = H.bconv2d(spec, odst, ops.x, ops.w, ops.mul, ops.bias, thresholds=ops.thr, out_scale=ops.scale, out_zero_point=ops.zp,
                          engine=opts["engine"], options=opts, sign_words=bits, out=out, max_batch=max_batch)
    assert got is out
    if kernel is not None:
        assert name == kernel
    assert np.array_equal(out.view(np.uint8), ops.want.view(np.uint8)), (name, "first differing image %d" % _first_bad_image(out, ops.want))
    assert (out_buf[:GUARD] == 0x5A).all() and (out_buf[-GUARD:] == 0x5A).all(), (name, "wrote outside the output")
    if bits is not None:
        assert np.array_equal(bits, ops.want_bits), (name, "second output")
        assert (bits_buf[:GUARD] == 0x5A).all() and (bits_buf[-GUARD:] == 0x5A).all(), (name, "wrote outside the second output")
    return name


def _first_bad_image(got, want):
    bad = np.nonzero((got.view(np.uint8).reshape(got.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1)).any(axis=1))[0]
    return int(bad[0]) if bad.size else -1


class _Ahead:
    """Runs job(i) for the parametrized test i and, on worker threads, the jobs of the next few tests meanwhile: most of these launches
    have two blocks, which keep two cores busy (the simulation runs the blocks of a launch in parallel, hostsim.cpp), so a few at a time
    fill the machine.  A job's assertion error is raised in its own test."""

    def __init__(self, job, count, window=8):
        self.job, self.count, self.window, self.futures, self.pool = job, count, window, {}, None

    def result(self, index):
        if self.pool is None:
            self.pool = ThreadPoolExecutor(max_workers=max(1, min(4, (os.cpu_count() or 2) // 2)))
        for i in range(index, min(self.count, index + self.window)):
            if i not in self.futures:
                self.futures[i] = self.pool.submit(self.job, i)
        return self.futures.pop(index).result()


def _entry_job(index):
    case = L.LONG_RUN_CASES[index]
    _simulate(L.case_spec(case), case[6], case[7], L.case_operands(index), kernel=case[8])


_entries = _Ahead(_entry_job, len(L.LONG_RUN_CASES))


@pytest.mark.parametrize("index", range(len(L.LONG_RUN_CASES)), ids=lambda i: L.case_id(L.LONG_RUN_CASES[i]))
def test_an_entry_in_the_host_simulation_equals_the_oracle(index):
    _entries.result(index)


# ------------------------------------------------------------------------------------ a launch smaller than the one planned for

# (batch, planned launch, layer, output type, options, kernel): the simulation plans for `planned` images and runs the batch in launches
# of that size; the last one is smaller and takes make_stream_args' / make_ws_args' branches for it (on the GPU: a slice of run_host,
# tests/test_gpu_launch_geometry.py) -- interleaved runs keep the planned stride, flat runs the planned run length (5 images: a run of 4
# and a run of 1), the weight-streaming kernel gets fewer groups (3 images: the last group has one), two blocks per CU fewer runs
SMALLER_LAUNCHES = [
    (7, 5, (28, 128, 128, 1), "f32", "engine=stream;stream_rows=4;stream_interleave=1;compute_units=2", "bconv2d_stream<f32,3x3x128,rows4,il>"),
    (13, 8, (7, 512, 512, 1), "f32", "engine=stream;stream_rows=7;stream_interleave=0;stream_flat=1;compute_units=8", "bconv2d_stream<f32,3x3x512,rows7>"),
    (7, 4, (7, 512, 512, 1), "i8", "engine=wstream;wstream_images=2;compute_units=2", "bconv2d_wstream<i8,3x3x512,images2,blocks4>"),
    (9, 6, (56, 64, 64, 1), "bp", "engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=2;compute_units=2", "bconv2d_stream<bitpacked,3x3x64,rows56,x2>"),
]


@pytest.mark.parametrize("case", SMALLER_LAUNCHES, ids=lambda c: c[5])
def test_a_launch_smaller_than_planned_in_the_host_simulation(case):
    batch, planned, (hw, cin, cout, stride), dst, options, kernel = case
    spec = L.layer_spec(batch, hw, hw, cin, cout, stride)
    plan = L.plan_fields(spec, L.DST_OF[dst], options, max_batch=planned)
    assert plan["err"] == "" and plan["kernel"] == kernel and plan["chunk"] == planned
    if dst == "f32" and cin == 512:
        assert plan["st_flat"] == 1 and plan["st_spb"] == 4 and (batch - planned) % 4
    _simulate(spec, dst, options, L.operands(spec, dst, 8000 + batch), kernel=kernel, max_batch=planned)


def _owned_segments(g, block):
    """lce_kernels_stream.h, "this block's run of segments": g0, g0 + GSTR, ... below S, at most SPB of them."""
    g0 = block * g["G0M"]
    count = min(g["SPB"], max(0, -(-(g["S"] - g0) // g["GSTR"])))
    return [g0 + k * g["GSTR"] for k in range(count)]


@pytest.mark.parametrize("index", range(len(L.LONG_RUN_CASES)), ids=lambda i: L.case_id(L.LONG_RUN_CASES[i]))
def test_every_launch_up_to_the_planned_one_gives_each_segment_to_one_block(index):
    """An entry's plan launched on 1 .. batch images (run_host's slices, a batch's last chunk): every segment belongs to exactly one
    block and no block is empty -- interleaved runs keep the planned stride on min(S, stride) blocks, flat runs keep the planned run
    length --; the weight-streaming kernel's groups hold every image, the last one at least one."""
    case = L.LONG_RUN_CASES[index]
    spec = L.case_spec(case)
    fields, by_batch = L.launches(spec, L.DST_OF[case[6]], case[7], range(1, spec.batch + 1))
    for batch, g in by_batch.items():
        if g["family"] == "wstream":
            assert g["ipb"] == fields["ws_ipb"] and g["parts"] == fields["ws_parts"] and g["grid_x"] == g["groups"] * g["parts"]
            assert (g["groups"] - 1) * g["ipb"] < batch <= g["groups"] * g["ipb"], (batch, g)
            continue
        assert g["S"] == batch * fields["st_spi"]
        owned = [_owned_segments(g, b) for b in range(g["grid_x"])]
        assert all(owned), (batch, g, "a block without a segment")
        assert sorted(s for run in owned for s in run) == list(range(g["S"])), (batch, g)
        if g["flat"]:
            assert g["SPB"] == fields["st_spb"]         # (the pixel blocks are cut for runs of exactly this length)
        if fields["st_gstr"] > 1:
            assert g["GSTR"] == fields["st_gstr"]       # (the tables' output offsets carry the planned stride)


# ------------------------------------------------------------------------------------ seeded draws of forced geometry

def test_the_forced_geometry_draws_are_mostly_kept():
    """The draws are the same list everywhere (a PCG64 stream, as tests/random_models.py); the ones the host planner refuses are dropped:
    at most 30 % of them, and at least 100 are kept.  FORCED_DROPPED, which the GPU test reads, is the planner's verdict."""
    candidates = L.forced_geometry_candidates()
    kept, dropped = L.forced_geometry_cases()
    print("forced geometry draws: %d kept, %d dropped of %d" % (len(kept), len(dropped), len(candidates)))
    assert len(dropped) <= 0.30 * len(candidates) and len(kept) >= 100
    assert tuple(i for i, c in enumerate(candidates) if c in dropped) == L.FORCED_DROPPED
    assert L.forced_kept() == kept
    assert L.forced_geometry_candidates() == candidates
    # every value of every option is among the kept ones
    seen = {}
    for c in kept:
        for k, v in L.option_dict(c.options).items():
            seen.setdefault(k, set()).add(v)
    assert seen["engine"] == {"stream", "wstream"} and seen["compute_units"] == set("12357")
    assert seen["stream_interleave"] == {"0", "1", "auto"} and seen["stream_blocks_per_cu"] == {"auto", "2"}
    assert seen["stream_pixel_phases"] == {"0", "2", "4"} and seen["stream_flat"] == {"0", "1"}
    assert seen["wstream_images"] == set("0123") and seen["wstream_blocks"] == set("0124")
    assert {c.dst for c in kept} == set(L.DST_NAMES) and {c.spec.stride_h for c in kept} == {1, 2}
    assert {(c.spec.padding, c.spec.pad_values) for c in kept} == set(L.PADDINGS.values())
    assert {(c.spec.in_h, c.spec.in_w) for c in kept} == {(7, 7), (8, 12), (14, 14), (9, 30), (28, 28)}
    assert {c.spec.channels_in for c in kept} == {64, 128, 192, 256, 320, 512}
    assert {c.spec.channels_out for c in kept} == {32, 64, 96, 128, 256, 320}


_KEPT = L.forced_kept()


def _draw_job(index):
    case = _KEPT[index]
    _simulate(case.spec, case.dst, case.options, L.operands(case.spec, case.dst, case.seed))


_draws = _Ahead(_draw_job, len(_KEPT))


@pytest.mark.parametrize("index", range(len(_KEPT)), ids=lambda i: "%03d_%s" % (i, L.forced_id(_KEPT[i])))
def test_a_forced_geometry_draw_in_the_host_simulation_equals_the_oracle(index):
    case = _KEPT[index]
    plan = L.plan_fields(case.spec, L.DST_OF[case.dst], case.options)
    assert plan["err"] == "" and L.family(plan) == L.option_dict(case.options)["engine"]
    _draws.result(index)
