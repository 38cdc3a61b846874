#!/usr/bin/env python
"""GPU timing of the int8 CONV_2D (lce_hip_conv2d_i8) and of the fixtures of tests/int8_conv_models.py:
  1. the kernel alone at batch 256 on three layers of an int8-converted network -- the 3x3 / 2 stem on 224x224x3 -> 64, the
     7x7 / 2 stem on 224x224x3 -> 64, the 1x1 shortcut on 28x28x64 -> 128 -- with bias and RELU, the int8 tensor only:
     microseconds per launch from HIP events around back-to-back launches and the same from a captured graph, after a 40 ms
     spin-up, the operand sets rotating through more than the 256 MB cache, three repeats (the median and the spread are
     printed).  Against the layer's byte bound (input bytes at the 8 TB/s read rate + output bytes at the 5.5 TB/s the chip
     writes) and against the float entry at the same shape in the same process (lce_hip_conv2d_f32 for the
     stems, lce_hip_conv1x1_f32 for the shortcut), which moves four times the bytes.
  2. each fixture as ONE section (every flag) against the parent's partition: its sections on the GPU and the tensors that
     cross to the host operator copied to the host and back (the host's own arithmetic is NOT counted: a floor for the cut).
usage: conv2d_i8_sections.py [--launches N] [--batch B] [--quick]"""
import argparse
import ctypes as C
import importlib
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
import int8_conv_models as M                                                                                 # noqa: E402
import pool_ref as PR                                                                                        # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
READ, WRITE = 8.0e12, 5.5e12
SPINUP_MS = 40.0
# (name, input extent, Cin, filter, stride, Cout)
LAYERS = (("stem 3x3/2 224x224x3 -> 64", 224, 3, 3, 2, 64), ("stem 7x7/2 224x224x3 -> 64", 224, 3, 7, 2, 64),
          ("shortcut 1x1 28x28x64 -> 128", 28, 64, 1, 1, 128))


def spin_up(fn, ms=SPINUP_MS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    while True:
        for i in range(8):
            fn(i)
        b.record()
        b.synchronize()
        if a.elapsed_time(b) >= ms:
            return


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches        # us per launch


def measure(fn, launches, sets, stream):
    """(median, spread) of three repeats of events around `launches` launches, and the same for a graph of `sets` launches."""
    spin_up(fn)
    eager = [timed(fn, launches) for _ in range(3)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for i in range(sets):
            fn(i)
    spin_up(lambda i: g.replay(), 10.0)
    reps = max(1, launches // sets)
    graph = [timed(lambda i: g.replay(), reps) / sets for _ in range(3)]
    return (statistics.median(eager), max(eager) - min(eager)), (statistics.median(graph), max(graph) - min(graph))


def ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def kernel_rows(launches, batch):
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(7)
    s = torch.cuda.Stream()
    for name, size, cin, filt, stride, cout in LAYERS:
        oh = PR.out_and_pad(size, filt, stride, amd.PADDING_SAME)[0]
        n_in, n_out = batch * size * size * cin, batch * oh * oh * cout
        bound_i8 = (n_in / READ + n_out / WRITE) * 1e6
        bound_f32 = 4 * bound_i8
        sets = max(2, math.ceil(CACHE / (n_in + n_out)) + 1)
        sets_f = max(2, math.ceil(CACHE / (4 * (n_in + n_out))) + 1)
        q_in, q_out = (0.02, -128 if cin == 3 else -4), (0.05, -9)
        w, bias, sw = M.conv_constants(cout, (filt, filt), cin, 3, q_in, q_out, True)
        table, _, _ = amd.conv2d_i8_prepare(w, bias, sw, q_in, q_out, amd.ACT_RELU)
        wd, td = torch.from_numpy(w).to(DEV), torch.from_numpy(table).to(DEV)
        xs = [torch.randint(-128, 128, (batch, size, size, cin), dtype=torch.int8, device=DEV, generator=gen) for _ in range(sets)]
        outs = [torch.empty((batch, oh, oh, cout), dtype=torch.int8, device=DEV) for _ in range(sets)]
        desc = amd.Conv2dI8Desc(batch, size, size, cin, cout, filt, filt, stride, stride, amd.PADDING_SAME, amd.ACT_RELU, q_in[0], q_in[1],
                                q_out[0], q_out[1])
        with torch.cuda.stream(s):
            st = C.c_void_p(s.cuda_stream)
            i8 = lambda i: amd.check(amd.lib().lce_hip_conv2d_i8(C.byref(desc), ptr(xs[i % sets]), ptr(wd), ptr(td), ptr(outs[i % sets]), None, st))
            (e_i8, se_i8), (g_i8, sg_i8) = measure(i8, launches, sets, s)
        del xs, outs
        torch.cuda.empty_cache()
        xf = [torch.randn((batch, size, size, cin), device=DEV, generator=gen) for _ in range(sets_f)]
        of = [torch.empty((batch, oh, oh, cout), device=DEV) for _ in range(sets_f)]
        wf = torch.randn((cout, filt, filt, cin), device=DEV, generator=gen) * 0.2
        bf = torch.randn((cout,), device=DEV, generator=gen)
        with torch.cuda.stream(s):
            if filt == 1:
                fd = amd.Conv1x1Desc(batch, size, size, cin, cout, stride, stride, amd.ACT_RELU)
                f32 = lambda i: amd.check(amd.lib().lce_hip_conv1x1_f32(C.byref(fd), ptr(xf[i % sets_f]), ptr(wf), ptr(bf), ptr(of[i % sets_f]), None, st))
            else:
                fd = amd.Conv2dDesc(batch, size, size, cin, cout, filt, filt, stride, stride, amd.PADDING_SAME, amd.ACT_RELU)
                f32 = lambda i: amd.check(amd.lib().lce_hip_conv2d_f32(C.byref(fd), ptr(xf[i % sets_f]), ptr(wf), ptr(bf), ptr(of[i % sets_f]), None, st))
            (e_f, se_f), (g_f, sg_f) = measure(f32, launches, sets_f, s)
        del xf, of
        torch.cuda.empty_cache()
        lines += ["kernel  %-30s batch %d: int8  events %8.1f us (spread %.1f)  graph %8.1f us (spread %.1f)  byte bound %6.1f us = %.2f of the graph time  (%d operand sets)"
                  % (name, batch, e_i8, se_i8, g_i8, sg_i8, bound_i8, bound_i8 / g_i8, sets),
                  "kernel  %-30s batch %d: float events %8.1f us (spread %.1f)  graph %8.1f us (spread %.1f)  byte bound %6.1f us = %.2f of the graph time  (%d operand sets)"
                  % (name, batch, e_f, se_f, g_f, sg_f, bound_f32, bound_f32 / g_f, sets_f),
                  "kernel  %-30s int8 / float = %.2f (graph), %.2f (events): %s" % (name, g_i8 / g_f, e_i8 / e_f, "FASTER" if g_i8 < g_f else "SLOWER than the float entry")]
    return lines


def section_rows(launches, batch):
    lines = []
    for name in sorted(M.FIXTURES):
        data, xt, out_t, info = M.FIXTURES[name]()
        gen = torch.Generator(device=DEV).manual_seed(1)
        xs = [torch.randint(-128, 128, (batch,) + info["shape"], dtype=torch.int8, device=DEV, generator=gen) for _ in range(2)]
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            stream = s.cuda_stream
            fused = mr.LceModel(data, **M.ALL_FLAGS)
            assert len(fused.sections) == 1 and fused.sections[0].inputs == [xt]
            dims, _ = fused.section_tensor_shape(0, out_t, batch)
            y = torch.empty(dims, dtype=torch.int8, device=DEV)
            one = lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream)
            spin_up(one)
            t_a = statistics.median(timed(one, launches) for _ in range(3))
            stats = fused.conv_i8_stats()
            fused.use_hip_graphs(True)
            spin_up(one)
            t_b = statistics.median(timed(one, launches) for _ in range(3))
            fused.use_hip_graphs(False)
            # the parent's partition: its sections, and every tensor that crosses to a host operator goes to the host and back
            cut = mr.LceModel(data, **info["parent_flags"])
            assert [sec.ops for sec in cut.sections] == info["parent_sections"]
            bufs = []
            for k, sec in enumerate(cut.sections):
                ins = [torch.empty(cut.section_tensor_shape(k, t, batch)[0], dtype=torch.int8, device=DEV) for t in sec.inputs]
                outs = [torch.empty(cut.section_tensor_shape(k, t, batch)[0], dtype={mr.INT8: torch.int8, mr.INT32: torch.int32}[cut.tensors[t].type],
                                    device=DEV) for t in sec.outputs]
                bufs.append((k, ins, outs, [torch.empty(o.shape, dtype=o.dtype).pin_memory() for o in outs]))

            def cut_run(i):
                for k, ins, outs, pins in bufs:
                    cut.run_section(k, batch, [t.data_ptr() for t in ins], [t.data_ptr() for t in outs], stream)
                    for o, p in zip(outs, pins):
                        p.copy_(o, non_blocking=True)
                        o.copy_(p, non_blocking=True)
            spin_up(cut_run)
            t_c = statistics.median(timed(cut_run, launches) for _ in range(3))
        lines += ["section %-22s batch %d: (a) one section, eager %8.1f us  (b) HIP-graph replay %8.1f us  (conv_i8 launches / LceQuantize folded: %s)"
                  % (name, batch, t_a, t_b, stats),
                  "section %-22s batch %d: (c) the parent's %d section(s) + the crossing tensors to the host and back, no host arithmetic %8.1f us  (a / c = %.2f)"
                  % (name, batch, len(cut.sections), t_c, t_a / t_c)]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    launches = 6 if a.quick else a.launches
    print("device:", torch.cuda.get_device_name(DEV))
    for line in kernel_rows(launches, a.batch):
        print(line, flush=True)
    for line in section_rows(launches, a.batch):
        print(line, flush=True)


if __name__ == "__main__":
    main()
