"""The batch-sharded path on real devices.

The path shards over the batch with no data-path collective: rank r owns a contiguous NHWC slab, weights are
replicated, and the process group carries only barriers, the timing reduction and (when a consumer wants the whole
batch) an all-gather of the outputs.  What can be falsified:

  * every rank's HIP shard, reassembled by all_gather_batch, is BIT-IDENTICAL to the single-GPU full-batch run and to
    the CPU oracle -- over RCCL with one rank per GPU where the box has several (the driver's 8-GPU node), and on ANY
    box with two ranks that share GPU 0 and gather over gloo (everything but the xGMI transport);
  * one process can drive one plan per device (lce_hip_set_device), and a plan refuses
    to run on a device it is not bound to;
  * bench.py's line: the contract fields, weak scaling (--gpus N) and BASELINE config 4 as stated
    (--gpus 8 --global-batch 2048, strong scaling), `rccl_world_size == N`.
"""
import importlib
import json
import os
import socket
import time
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NGPU = torch.cuda.device_count()
LAYER = dict(in_h=14, in_w=14, channels_in=256, filter_h=3, filter_w=3, channels_out=256)   # QuickNet's 14x14 section


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, world, port, backend, global_batch, dst_name, q):
    """One rank: its slab on its GPU through the C ABI, the gather, and (rank 0) the comparisons."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    import oracle_lib as O
    import synth
    amd = importlib.import_module("compute-engine_amd")
    shard = importlib.import_module("compute-engine_amd.batch_shard")
    dev_index = rank if backend == "nccl" else 0           # gloo leg: every rank shares GPU 0
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    assert dist.get_world_size() == world
    dst, odst = {"f32": (amd.F32, O.DST_F32), "i8": (amd.I8, O.DST_I8), "bp": (amd.BITPACKED, O.DST_BITPACKED)}[dst_name]
    full = O.ConvSpec(batch=global_batch, padding=O.PADDING_SAME, pad_values=1, **LAYER)
    x, w, mul, bias = synth.conv_inputs(full, 4242)                              # the same operands on every rank
    thr = O.thresholds_converter(full, mul, bias)

    def run(images):
        n = images.shape[0]
        plan = amd.Bconv2dPlan(amd.ConvParams(n, 14, 14, 256, 3, 3, 256, padding=amd.PADDING_SAME, pad_values=1, dst_type=dst,
                                              out_scale=0.125, out_zero_point=3))
        plan.set_weights(w, mul, bias, thr)
        out = plan.run(torch.from_numpy(np.ascontiguousarray(images)).to(dev))
        torch.cuda.synchronize(dev)
        assert plan.device() == dev_index
        return out, plan.kernel_name()

    start, count = shard.shard_range(global_batch, world, rank)
    local, name = run(x[start:start + count])
    gathered = shard.all_gather_batch(local if backend == "nccl" else local.cpu(), global_batch, dist).cpu().numpy()
    ok_full = ok_oracle = True
    if rank == 0:
        whole, _ = run(x)                                                        # the single-GPU full-batch run
        ok_full = bool(np.array_equal(whole.cpu().numpy().view(np.uint8), gathered.view(np.uint8)))
        subset = sorted({0, 1, global_batch // 2, global_batch - 1})
        want = O.bconv2d(O.ConvSpec(batch=len(subset), padding=O.PADDING_SAME, pad_values=1, **LAYER), odst, x[subset], w, mul, bias,
                         thresholds=thr, out_scale=0.125, out_zero_point=3, threads=8)
        ok_oracle = bool(np.array_equal(gathered[subset].view(np.uint8), want.view(np.uint8)))
    dist.barrier()
    q.put((rank, ok_full, ok_oracle, name, dist.get_world_size()))
    dist.destroy_process_group()


def _run_sharded(world, backend, global_batch, dst_name):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, backend, global_batch, dst_name, q)) for r in range(world)]
    for p in procs:
        p.start()
    results, deadline = [], time.monotonic() + 600
    while len(results) < world:                       # (a worker that died is reported at once, not after the timeout)
        try:
            results.append(q.get(timeout=2))
        except Exception:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead, f"a rank exited with {dead}"
            assert time.monotonic() < deadline, "ranks did not report within 600 s"
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(r[0] for r in results) == list(range(world))
    assert all(r[1] and r[2] for r in results), results
    assert all(r[4] == world for r in results)
    return results


@pytest.mark.skipif(NGPU < 2, reason="needs at least two GPUs (one rank per GPU over RCCL)")
@pytest.mark.parametrize("dst", ["f32", "bp"])
def test_sharded_hip_run_equals_the_single_gpu_run_over_rccl(dst):
    world = min(NGPU, 8)
    results = _run_sharded(world, "nccl", 64 * world + 3, dst)                   # ragged shards: the first 3 ranks take one more
    assert all(r[3].startswith("bconv2d_") for r in results)


@pytest.mark.parametrize("dst,global_batch", [("f32", 37), ("i8", 32), ("bp", 5)])
def test_sharded_hip_run_equals_the_single_gpu_run_two_ranks_on_one_gpu(dst, global_batch):
    """The same check where there is ONE GPU: two ranks share it and gather over gloo -- the slabs, the HIP runs, the
    reassembly and both comparisons are the real ones, only the transport is not xGMI."""
    _run_sharded(2, "gloo", global_batch, dst)


def test_one_process_drives_one_plan_per_device():
    """SURVEY.md section 7 step 8's other layout: ONE process, one plan / stream / slab per device (lce_hip_set_device)."""
    import oracle_lib as O
    import synth
    amd = importlib.import_module("compute-engine_amd")
    shard = importlib.import_module("compute-engine_amd.batch_shard")
    n = max(1, NGPU)
    global_batch = 24 * n + 1
    full = O.ConvSpec(batch=global_batch, padding=O.PADDING_SAME, pad_values=1, **LAYER)
    x, w, mul, bias = synth.conv_inputs(full, 99)
    plans, outs = [], []
    for d in range(n):                                                            # launch everything, then wait
        amd.check(amd.lib().lce_hip_set_device(d))
        start, count = shard.shard_range(global_batch, n, d)
        plan = amd.Bconv2dPlan(amd.ConvParams(count, 14, 14, 256, 3, 3, 256, padding=amd.PADDING_SAME, pad_values=1, dst_type=amd.F32))
        plan.set_weights(w, mul, bias, None)
        xd = torch.from_numpy(np.ascontiguousarray(x[start:start + count])).to(f"cuda:{d}")
        outs.append(plan.run(xd))
        plans.append(plan)
    for d in range(n):
        torch.cuda.synchronize(d)
        assert plans[d].device() == d
    amd.check(amd.lib().lce_hip_set_device(0))
    got = np.concatenate([o.cpu().numpy() for o in outs], axis=0)
    subset = [0, global_batch // 2, global_batch - 1]
    want = O.bconv2d(O.ConvSpec(batch=3, padding=O.PADDING_SAME, pad_values=1, **LAYER), O.DST_F32, x[subset], w, mul, bias, threads=8)
    assert np.array_equal(got[subset].view(np.int32), want.view(np.int32))
    whole = amd.Bconv2dPlan(amd.ConvParams(global_batch, 14, 14, 256, 3, 3, 256, padding=amd.PADDING_SAME, pad_values=1, dst_type=amd.F32))
    whole.set_weights(w, mul, bias, None)
    ref = whole.run(torch.from_numpy(x).to("cuda:0")).cpu().numpy()
    assert np.array_equal(ref.view(np.int32), got.view(np.int32))
    if n >= 2:
        # a plan is bound to the device it first ran on: with another device current it must refuse, not read foreign memory
        amd.check(amd.lib().lce_hip_set_device(1))
        xd0 = torch.from_numpy(np.ascontiguousarray(x[:plans[0].params.batch])).to("cuda:0")
        with pytest.raises(amd.LceHipError, match="bound to HIP device 0"):
            plans[0].run_ptr(xd0.data_ptr(), outs[0].data_ptr(), 0)
        amd.check(amd.lib().lce_hip_set_device(0))


def _bench(*flags, timeout=900, no_extra=True, plain=False):
    """bench.py's one line; plain=True: without the --no-extra / --no-cpu-baseline opt-outs (which act with --full only)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    opt_outs = [] if plain else [*(["--no-extra"] if no_extra else []), "--no-cpu-baseline"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", *opt_outs, *flags],
                         env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_bench_single_gpu_line_has_the_contract_fields():
    r = _bench()
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in r, key
    assert r["n_gpus"] == 1 and r["steps"] == 5 and r["roofline"]["bound"] == "hbm" and 0 < r["roofline"]["frac"] < 1
    assert r["scaling"] == "weak" and r["rccl_world_size"] == 1 and r["config"]["global_batch"] == 256
    assert r["kernel"].startswith(("bconv2d_stream<f32", "bconv2d_mfma_direct<f32")) and r["dtype"].startswith("fp4-e2m1")
    assert abs(r["value"] - 9 * 256 * 256 * 56 * 56 * 256 / (r["ms_per_step"] * 1e-3)) < 1e-6 * r["value"]


def test_bench_global_batch_is_strong_scaling():
    r = _bench("--global-batch", "64")
    assert r["scaling"] == "strong" and r["config"]["global_batch"] == 64 and r["config"]["per_gpu_batch"] == 64
    assert abs(r["value"] - 9 * 256 * 256 * 56 * 56 * 64 / (r["ms_per_step"] * 1e-3)) < 1e-6 * r["value"]


def _layer_on_the_oracle(batch):
    """The float output of bench.py's layer on its own seeded operands (tools/synthetic_layers.py, seed 0), from the CPU oracle."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle_lib as O
    import synthetic_layers as SL
    layer = SL.Layer(batch=batch, in_h=56, in_w=56, channels_in=256, filter_h=3, filter_w=3, channels_out=256,
                     padding=SL.PADDING_SAME, pad_values=1)
    w, mul, bias, _ = SL.weights(layer, 0)
    spec = O.ConvSpec(batch=batch, in_h=56, in_w=56, channels_in=256, filter_h=3, filter_w=3, channels_out=256,
                      padding=O.PADDING_SAME, pad_values=1)
    return O.bconv2d(spec, O.DST_F32, SL.activations(layer, 0), w, mul, bias, threads=8)


def test_bench_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """A plain run times exactly --steps steps and measures nothing beyond its headline (no `extra`, `cpu_baseline`: --full
    has them); --dump-outputs writes the last timed step's float output, whole when it fits 32 MB, else the 32768 pixels a
    generator seeded with 0 draws (all 256 channels) -- bit for bit the oracle's on the same seeded operands, so two builds'
    files compare element for element."""
    r = _bench("--steps", "7", "--warmup", "1", "--dump-outputs", str(tmp_path / "b256"), plain=True)
    assert r["steps"] == 7 and "extra" not in r and "cpu_baseline" not in r and r["roofline"]["bound"] == "hbm"
    got = np.load(tmp_path / "b256" / "output.npy")
    assert got.dtype == np.float32 and got.shape == (32768, 256) and got.nbytes <= 64 << 20
    idx = np.sort(np.random.default_rng(0).choice(256 * 56 * 56, 32768, replace=False))
    want = _layer_on_the_oracle(256).reshape(-1, 256)[idx]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    r = _bench("--global-batch", "8", "--dump-outputs", str(tmp_path / "b8"), plain=True)
    assert r["steps"] == 5 and r["outputs_dumped"]["holds"] == "the whole output"
    got = np.load(tmp_path / "b8" / "output.npy")
    assert got.dtype == np.float32 and got.shape == (8, 56, 56, 256)
    assert np.array_equal(got.view(np.int32), _layer_on_the_oracle(8).view(np.int32))


@pytest.mark.skipif(NGPU < 2, reason="needs at least two GPUs")
def test_bench_on_every_gpu_of_the_node_over_rccl():
    n = NGPU
    r = _bench("--gpus", str(n))
    assert r["n_gpus"] == n and r["rccl_world_size"] == n and len(r["per_rank_ms_per_step"]) == n
    assert r["config"]["global_batch"] == 256 * n and r["scaling"] == "weak"
    assert abs(r["value"] - n * r["per_gpu_value"]) < 1e-6 * r["value"]          # whole-job value = sum over ranks
    chk = r["multi_gpu_self_check"]                                              # the line proves what it came from
    assert chk["distinct_devices"] == n and chk["sharded_equals_single_gpu_on_every_rank"] and chk["rccl_version"]
    assert sorted(d["rank"] for d in chk["devices"]) == list(range(n)) and len({d["uuid"] for d in chk["devices"]}) == n
    # BASELINE config 4 as stated: 2048 images over the node (on fewer than 8 GPUs: the same per-GPU share)
    r = _bench("--gpus", str(n), "--global-batch", str(256 * n))
    assert r["scaling"] == "strong" and r["config"]["global_batch"] == 256 * n and r["rccl_world_size"] == n


def test_bench_collectives_against_the_real_rccl_with_one_rank():
    """Every collective call of bench.py's N > 1 path -- RCCL process group bound to the device, all_gather_object, the
    self-check's all_gather_batch of device tensors, max / gather over ranks, barriers with device_ids, the sharded config-4 chain --
    executed against the real RCCL on a box with ONE GPU: torch.distributed.run with one rank and LCE_BENCH_RCCL_WITH_ONE_RANK=1.
    (What a one-GPU box cannot show is the transport between devices; test_bench_on_every_gpu_of_the_node_over_rccl does.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["LCE_BENCH_RCCL_WITH_ONE_RANK"] = "1"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
                          "--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--full"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = lines[0]
    assert r["n_gpus"] == 1 and r["rccl_world_size"] == 1 and r["collective_backend"] == "nccl (RCCL)"
    chk = r["multi_gpu_self_check"]
    assert chk["sharded_equals_single_gpu_on_every_rank"] and chk["rccl_version"] and chk["distinct_devices"] == 1
    c4 = r["config4_quicknet_large_sharded"]
    assert c4["global_batch"] == 256 and len(c4["per_rank_chain_ms"]) == 1 and 0.3 < c4["chain_ms"] < 5


@pytest.mark.parametrize("dst", ["f32", "bp"])
def test_sharded_hip_run_over_rccl_with_one_rank(dst):
    """The sharded run's collective leg (all_gather_batch on device tensors) against the real RCCL, world size 1."""
    results = _run_sharded(1, "nccl", 19, dst)
    assert len(results) == 1


def test_bench_multi_rank_path_with_two_ranks_sharing_one_gpu():
    """The N > 1 code path of bench.py -- self-launch through torch.distributed.run, shard ranges, barriers, max / gather over
    ranks, the config-4 chain every rank runs -- on a box with ONE GPU: --share-gpu puts both ranks on cuda:0 and lets them meet
    over gloo (a test aid, not a measurement; the RCCL variant is the test above)."""
    r = _bench("--gpus", "2", "--share-gpu", "--full", no_extra=False, timeout=900)
    assert r["n_gpus"] == 2 and r["rccl_world_size"] == 2 and len(r["per_rank_ms_per_step"]) == 2
    assert r["collective_backend"].startswith("gloo") and r["config"]["global_batch"] == 512 and r["scaling"] == "weak"
    assert abs(r["value"] - 9 * 256 * 256 * 56 * 56 * 512 / (r["ms_per_step"] * 1e-3)) < 1e-6 * r["value"]
    c4 = r["config4_quicknet_large_sharded"]
    assert c4["global_batch"] == 512 and len(c4["per_rank_chain_ms"]) == 2 and c4["chain_ms"] >= max(c4["per_rank_chain_ms"]) - 1e-9
    assert abs(c4["images_per_s"] - 512 / (c4["chain_ms"] * 1e-3)) < 1e-6 * c4["images_per_s"]
    assert "extra" not in r and "cpu_baseline" not in r      # N = 1 only
    chk = r["multi_gpu_self_check"]       # the sharded run was reassembled and compared on both ranks before anything was timed
    assert chk["sharded_equals_single_gpu_on_every_rank"] and chk["distinct_devices"] == 1 and len(chk["devices"]) == 2
    assert {d["rank"] for d in chk["devices"]} == {0, 1} and len({d["pid"] for d in chk["devices"]}) == 2


def test_eight_gpu_preflight_config4_as_stated_with_two_ranks_on_one_gpu():
    """Round 6 (review item 5): the first real 8-GPU run will be the driver's, so the exact shape of that run -- BASELINE config 4,
    `--global-batch 2048` (strong scaling: the ranks split a fixed batch), the self-check, the sharded QuickNetLarge chain, the line's
    fields -- runs here end to end with two ranks that share GPU 0 over gloo (`--share-gpu`; 1024 images per rank).  What this cannot
    show is the xGMI transport; everything else of `python -m torch.distributed.run ... bench.py --gpus N --global-batch 2048` is the
    code that runs there."""
    r = _bench("--gpus", "2", "--share-gpu", "--global-batch", "2048", "--steps", "3", "--full", no_extra=False, timeout=1200)
    assert r["n_gpus"] == 2 and r["rccl_world_size"] == 2 and r["steps"] == 3 and r["scaling"] == "strong"
    assert r["config"]["global_batch"] == 2048 and r["config"]["per_gpu_batch"] == 1024
    assert abs(r["value"] - 9 * 256 * 256 * 56 * 56 * 2048 / (r["ms_per_step"] * 1e-3)) < 1e-6 * r["value"]
    assert len(r["per_rank_value"]) == 2 and all(v > 0 for v in r["per_rank_value"])
    assert r["value"] <= sum(r["per_rank_value"]) * (1 + 1e-9)          # the whole job runs at the slowest rank's pace
    chk = r["multi_gpu_self_check"]
    assert chk["sharded_equals_single_gpu_on_every_rank"] and len(chk["devices"]) == 2
    c4 = r["config4_quicknet_large_sharded"]
    assert c4["global_batch"] == 2048 and len(c4["per_rank_chain_ms"]) == 2 and len(c4["per_rank_images_per_s"]) == 2
    assert abs(c4["images_per_s"] - 2048 / (c4["chain_ms"] * 1e-3)) < 1e-6 * c4["images_per_s"]
    assert "efficiency" not in json.dumps(r)          # (the driver computes scaling efficiency from the per-N lines; this file never does)
