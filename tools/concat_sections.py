#!/usr/bin/env python
"""GPU timing of the channel join between binary layers (lce_hip_concat) and of the dense block of
tests/test_concat_sections_host.py at batch 256:
  1. the kernel alone at 256 x {28x28x(128+64), 28x28x(320+64), 14x14x(256+64+64)}, float, with the joined tensor only and
     with the bits as well: device-event time per launch and algorithmic bytes (read sum C + write sum C, + 1/8 B per element
     for the bits) / time as a fraction of 8 TB/s.  The operand sets rotate through more than twice the 256 MB Infinity
     Cache, so every launch reads HBM.  The yardstick is torch.cat(dim=3, out=) on the same tensors in the same process,
     interleaved A-B-A-B for --rounds rounds; the margin is the spread torch.cat shows against itself over the rounds.
  2. the block (H = 28 -> 14, 128 channels in, the fixture's growths): (a) ONE section (elementwise + concat sections),
     eager, (b) the same as a HIP-graph replay, (c) the way without the opt-in: the elementwise-sections partition through
     Interpreter.run_section with NumPy on the host for every operator outside the sections (device-to-host copy,
     np.concatenate and the batch norm it cuts off, host-to-device copy), (d) everything but the joins: the sections of that
     partition back to back on pre-made device tensors plus the batch-norm chains the host ran in (c) as lce_hip_elementwise
     launches; and the joins of (a) alone, each at its own shape with rotating operands.
usage: concat_sections.py [--iters N] [--rounds R] [--quick]     (--quick: a few iterations, for a run under rocprofv3 --kernel-trace)"""
import argparse
import importlib
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
from test_concat_sections_host import DENSE_STAGES, dense_block_model, joins_of          # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
SHAPES = ((28, (128, 64)), (28, (320, 64)), (14, (256, 64, 64)))


def timed(fn, iters, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def operand_sets(batch, h, channels, gen):
    """Enough (inputs, joined, bits) sets that a pass over all of them moves more than twice the Infinity Cache."""
    rows, total = batch * h * h, sum(channels)
    per_set = rows * total * 8
    sets = max(2, math.ceil(2 * CACHE / per_set) + 1)
    xs = [[torch.randn((batch, h, h, c), device=DEV, generator=gen) for c in channels] for _ in range(sets)]
    outs = [torch.empty((batch, h, h, total), device=DEV) for _ in range(sets)]
    bits = [torch.empty((batch, h, h, (total + 31) // 32), dtype=torch.int32, device=DEV) for _ in range(sets)]
    return sets, xs, outs, bits


def concat_into(xs, out, bits=None, stream=None):
    """lce_hip_concat into existing tensors (amd.concat allocates its bits)."""
    import ctypes as C
    ptrs = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
    ch = (C.c_int32 * len(xs))(*[t.shape[-1] for t in xs])
    rows = xs[0].numel() // xs[0].shape[-1]
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    amd.check(amd.lib().lce_hip_concat(amd.F32, ptrs, ch, len(xs), rows, 0, C.c_void_p(None if out is None else out.data_ptr()),
                                       C.c_void_p(None if bits is None else bits.data_ptr()), C.c_void_p(st)))


def kernel_rows(iters, rounds, batch=256):
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(7)
    for h, channels in SHAPES:
        sets, xs, outs, bits = operand_sets(batch, h, channels, gen)
        n = batch * h * h * sum(channels)
        ours, cat, with_bits = [], [], []
        for _ in range(rounds):                                   # A-B-A-B; the bits variant rides along as a third leg
            ours.append(timed(lambda i: concat_into(xs[i % sets], outs[i % sets]), iters))
            cat.append(timed(lambda i: torch.cat(xs[i % sets], dim=3, out=outs[i % sets]), iters))
            with_bits.append(timed(lambda i: concat_into(xs[i % sets], outs[i % sets], bits[i % sets]), iters))
        # the launches are byte-equal to the yardstick
        concat_into(xs[0], outs[0], bits[0])
        ref = torch.cat(xs[0], dim=3)
        equal = bool(torch.equal(outs[0].view(torch.int32), ref.view(torch.int32)))
        name = "256x%dx%dx(%s)" % (h, h, "+".join(map(str, channels)))
        spread = max(cat) - min(cat)
        for label, t, b in (("lce_hip_concat, joined only ", ours, 8 * n), ("torch.cat(dim=3, out=)       ", cat, 8 * n),
                            ("lce_hip_concat, joined + bits", with_bits, 8 * n + n / 8)):
            med = statistics.median(t)
            lines.append("kernel  %-22s %s median %8.1f us  (min %.1f, max %.1f over %d rounds)  %6.3f TB/s  %.3f of 8 TB/s"
                         % (name, label, med, min(t), max(t), rounds, b / med / 1e6, b / med / 1e6 / 8))
        d = statistics.median(ours) - statistics.median(cat)
        lines.append("kernel  %-22s lce_hip_concat - torch.cat = %+.1f us; torch.cat's own spread %.1f us: %s; bytes equal: %s; %d operand sets of %.0f MB"
                     % (name, d, spread, "inside the spread or faster" if d <= spread else "SLOWER by more than the spread", equal, sets, 8 * n / 2 ** 20))
        del xs, outs, bits, ref
        torch.cuda.empty_cache()
    return lines


def host_cut_run(it, steps, x):
    """(c): the sections of `it` through Interpreter.run_section (NumPy in, NumPy out), every other operator in NumPy."""
    model = it.model
    host = {}
    for s in steps:
        if s["kind"] == "dense":
            host[s["join"]] = lambda *xs: np.concatenate(xs, axis=-1)
            host[s["mul"]] = lambda v, m=s["bn_m"]: v * m
            host[s["add"]] = lambda v, a=s["bn_a"]: v + a
    section_of = {op: k for k, sec in enumerate(it.sections) for op in sec.ops}
    live, ran = {model.inputs[0]: x}, set()
    for i, op in enumerate(model.operators):
        if i in section_of:
            k = section_of[i]
            if k not in ran:
                ran.add(k)
                live.update(zip(it.sections[k].outputs, it.run_section(k, [live[t] for t in it.sections[k].inputs])))
        else:
            live[op.outputs[0]] = host[i](*[live[t] for t in op.inputs if not model.tensors[t].constant])
    return live[model.outputs[0]]


def block_rows(iters, batch=256, H=28, C0=128):
    data, xt, out_t, steps = dense_block_model(H=H, C0=C0, transition=2 * C0)
    gen = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randn((batch, H, H, C0), device=DEV, generator=gen) for _ in range(2)]
    s = torch.cuda.Stream()
    dt = {mr.INT8: torch.int8, mr.INT32: torch.int32, mr.FLOAT32: torch.float32}
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        fused = mr.LceModel(data, elementwise_sections=True, concat_sections=True)
        assert len(fused.sections) == 1
        dims, _ = fused.section_tensor_shape(0, out_t, batch)
        y = torch.empty(dims, dtype=torch.float32, device=DEV)
        # one input buffer per recorded graph (the pointers are part of its key), so eager and replay read the same tensors
        t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
        stats = fused.concat_stats()
        eager_out = y.clone()
        fused.use_hip_graphs(True)
        t_b = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters, warmup=6)
        graphs = fused.graph_stats()
        fused.run_section(0, batch, [xs[(iters - 1) % 2].data_ptr()], [y.data_ptr()], stream)
        s.synchronize()
        same = bool(torch.equal(y.view(torch.int32), eager_out.view(torch.int32)))
        fused.use_hip_graphs(False)
        # the joins of (a) alone, each at its own shape
        t_joins, gbytes = 0.0, 0.0
        for st in (st for st in steps if st["kind"] == "dense"):
            op = fused.operators[st["join"]]
            shapes = [fused.section_tensor_shape(0, t, batch)[0] for t in op.inputs]
            sets, jx, jo, jb = operand_sets(batch, shapes[0][1], [sh[3] for sh in shapes], gen)
            folds = any(fused.operators[r].custom_code == "LceQuantize" for r in range(len(fused.operators))
                        if st["out"] in fused.operators[r].inputs)
            t_joins += timed(lambda i: concat_into(jx[i % sets], jo[i % sets], jb[i % sets] if folds else None, stream), max(8, iters))
            gbytes += 8 * jo[0].numel() / 1e9
            del jx, jo, jb
            torch.cuda.empty_cache()
        # (d) everything but the joins: the elementwise partition's sections on pre-made inputs, and the batch norms that
        # partition leaves to the host as launches of their own (bits out only, as inside (a))
        cut = mr.LceModel(data, elementwise_sections=True)
        calls = []
        for k, sec in enumerate(cut.sections):
            ins = [torch.randn(cut.section_tensor_shape(k, t, batch)[0], device=DEV, generator=gen) for t in sec.inputs]
            outs = [torch.empty(cut.section_tensor_shape(k, t, batch)[0], dtype=dt[cut.tensors[t].type], device=DEV) for t in sec.outputs]
            calls.append((k, ins, outs))
        covered = {op for sec in cut.sections for op in sec.ops}
        chains = []
        for st in (st for st in steps if st["kind"] == "dense" and st["mul"] not in covered):
            shape = fused.section_tensor_shape(0, st["x"], batch)[0]
            chains.append((torch.randn(shape, device=DEV, generator=gen),
                           [("mul", torch.from_numpy(st["bn_m"]).to(DEV), amd.ACT_NONE), ("add", torch.from_numpy(st["bn_a"]).to(DEV), amd.ACT_NONE)],
                           torch.empty(tuple(shape[:3]) + ((shape[3] + 31) // 32,), dtype=torch.int32, device=DEV)))

        def rest(i):
            for k, ins, outs in calls:
                cut.run_section(k, batch, [a.data_ptr() for a in ins], [o.data_ptr() for o in outs], stream)
            for v, chain, bits in chains:
                amd.elementwise(v, chain, out=False, out_bits=bits, stream=stream)
        t_d = timed(rest, iters)
        # (its sections behind the first begin with an LceQuantize launch of their own; in (a) a batch norm or a join writes those bits)
        quantize_in_d = sum(1 for sec in cut.sections[1:] if cut.operators[sec.ops[0]].custom_code == "LceQuantize")
    # (c) through the host, host clock around whole runs (each ends in device-to-host copies, which synchronise)
    it = mr.Interpreter(cut, batch_size=batch)
    x_host = xs[0].cpu().numpy()
    got = host_cut_run(it, steps, x_host)
    hosts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_cut_run(it, steps, x_host)
        hosts.append((time.perf_counter() - t0) * 1e6)
    t_c = statistics.median(hosts)
    fused.run_section(0, batch, [xs[0].data_ptr()], [y.data_ptr()], 0)
    torch.cuda.synchronize()
    close = bool(np.array_equal(got.view(np.int32), y.cpu().numpy().view(np.int32)))
    n_joins = len(joins_of(steps))
    return ["block   batch %d, %dx%d -> %dx%d, %d channels in, growths %s, %d joins (%.2f GB read + written by them)"
            % (batch, H, H, H // 2, H // 2, C0, DENSE_STAGES, n_joins, gbytes),
            "block   (a) one section (elementwise + concat sections), eager   %10.1f us" % t_a,
            "block   (b) one section, HIP-graph replay                        %10.1f us   (graphs recorded / replays: %s; bytes equal to eager: %s)" % (t_b, graphs, same),
            "block   (c) elementwise sections only, joins and cut-off batch norms in NumPy through the host %10.1f us   (median of 3, host clock; "
            "%d sections; bytes equal to (a): %s; a / c = %.4f)" % (t_c, len(cut.sections), close, t_a / t_c),
            "block   (d) everything but the joins (that partition's sections + %d batch-norm launches), back to back %10.1f us   "
            "(holds %d LceQuantize launches that (a) folds into a batch norm: a high estimate of the rest; a - d = %.1f us)"
            % (len(chains), t_d, quantize_in_d, t_a - t_d),
            "block   the %d joins alone, each at its shape with rotating operands %10.1f us = %.1f %% of (a)   (lce_hip_concat launches / LceQuantize folded in (a): %s)"
            % (n_joins, t_joins, 100 * t_joins / t_a, stats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    iters = 4 if a.quick else a.iters
    rounds = 1 if a.quick else max(5, a.rounds)
    print("device:", torch.cuda.get_device_name(DEV))
    for line in kernel_rows(iters, rounds):
        print(line, flush=True)
    if not a.kernel_only:
        for line in block_rows(max(4, iters // 2)):
            print(line, flush=True)


if __name__ == "__main__":
    main()
