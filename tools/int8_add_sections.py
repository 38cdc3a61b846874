#!/usr/bin/env python
"""GPU timing of the int8 residual ADD between binary layers (lce_hip_add_int8) and of the int8 residual body of
tests/test_int8_add_host.py at batch 256:
  1. the kernel alone at 256 x {56x56x64, 28x28x128}, int8 sum and bits out, every variant that is proven for the parameter
     set (set A: literal, split; set B: literal, split, shift): device-event time per launch and algorithmic bytes (read both
     inputs, write the sum, write the bits: 3.125 B per element) / time as a fraction of 8 TB/s.  In the same call, on the same
     shapes, the FLOOR taken from the tree: lce_hip_elementwise with one tensor ADD step, float and bits out (12.125 B per
     element).  The operand sets rotate through more than twice the 256 MB Infinity Cache, so every launch reads HBM.
  2. the body: (a) one section with LCE_TFLITE_SECTIONS_INT8_ADD, eager, (b) the same as a HIP-graph replay, (c) the default
     partition's sections alone, back to back, WITHOUT any ADD and without the host round trips -- a lower bound for any host.
usage: int8_add_sections.py [--iters N] [--quick]        (--quick: a few iterations, for a run under rocprofv3 --kernel-trace)"""
import argparse
import importlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
import int8_add_ref as R                                          # noqa: E402
from test_int8_add_host import INT8_BODY, int8_body_model          # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
VARIANT = {amd.ADD_INT8_LITERAL: "literal", amd.ADD_INT8_SPLIT: "split", amd.ADD_INT8_SHIFT: "shift"}


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


def kernel_rows(iters):
    out = []
    for h, c in ((56, 64), (28, 128)):
        shape = (256, h, h, c)
        n = math.prod(shape)
        sets = max(2, math.ceil(2 * CACHE / (3 * n)) + 1)
        g = torch.Generator(device=DEV).manual_seed(c)
        rnd = lambda: torch.randint(-128, 128, shape, device=DEV, generator=g, dtype=torch.int8)
        x1, x2 = [rnd() for _ in range(sets)], [rnd() for _ in range(sets)]
        os_ = [torch.empty(shape, dtype=torch.int8, device=DEV) for _ in range(sets)]
        bs = [torch.empty(shape[:-1] + (c // 32,), dtype=torch.int32, device=DEV) for _ in range(sets)]
        bytes_ = n * 3 + n / 8
        for name, q, variants in (("A", R.SET_A, (0, 1)), ("B", R.SET_B, (0, 1, 2))):
            kw = dict(q1=q[0:2], q2=q[2:4], q_out=q[4:6])
            chosen = amd.add_int8_params(**kw)["variant"]
            for v in variants:
                us = timed(lambda i: amd.add_int8(x1[i % sets], x2[i % sets], out=os_[i % sets], out_bits=bs[i % sets], variant=v, **kw), iters)
                out.append("kernel  256x%dx%dx%-4d int8 ADD set %s %-8s%s %8.1f us  %6.3f TB/s  %.3f of 8 TB/s  (%d operand sets, %.0f MB each)"
                           % (h, h, c, name, VARIANT[v], " (chosen)" if v == chosen else "         ", us, bytes_ / us / 1e6,
                              bytes_ / us / 1e6 / 8, sets, 3 * n / 2 ** 20))
        del x1, x2, os_
        torch.cuda.empty_cache()
        # the floor from the tree: the float kernel with one tensor ADD step, float and bits out
        fsets = max(2, math.ceil(2 * CACHE / (12 * n)) + 1)
        fx = [torch.randn(shape, device=DEV, generator=g) for _ in range(fsets)]
        fr = [torch.randn(shape, device=DEV, generator=g) for _ in range(fsets)]
        fo = [torch.empty(shape, device=DEV) for _ in range(fsets)]
        steps = [[("add", fr[k], amd.ACT_NONE)] for k in range(fsets)]
        us = timed(lambda i: amd.elementwise(fx[i % fsets], steps[i % fsets], out=fo[i % fsets], out_bits=bs[i % len(bs)]), iters)
        fbytes = n * 12 + n / 8
        out.append("floor   256x%dx%dx%-4d float ADD + bits (lce_hip_elementwise)  %8.1f us  %6.3f TB/s  %.3f of 8 TB/s  (%d operand sets)"
                   % (h, h, c, us, fbytes / us / 1e6, fbytes / us / 1e6 / 8, fsets))
        del fx, fr, fo, bs, steps
        torch.cuda.empty_cache()
    return out


def body_rows(iters, batch=256):
    data, xt, out_t, info = int8_body_model()
    g = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randint(-128, 128, (batch, 56, 56, 64), device=DEV, generator=g, dtype=torch.int8) for _ in range(2)]
    s = torch.cuda.Stream()
    rows = []
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        fused = mr.LceModel(data, int8_add_sections=True)
        dims, _ = fused.section_tensor_shape(0, out_t, batch)
        y = torch.empty(dims, dtype=torch.int8, device=DEV)
        # one input buffer per recorded graph (the pointers are part of its key), so eager and replay read the same tensors
        t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
        stats = fused.int8_add_stats()
        eager_out = y.clone()
        fused.use_hip_graphs(True)
        t_b = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters, warmup=6)
        graphs = fused.graph_stats()
        fused.run_section(0, batch, [xs[(iters - 1) % 2].data_ptr()], [y.data_ptr()], stream)
        s.synchronize()
        same = bool(torch.equal(y, eager_out))
        fused.use_hip_graphs(False)
        # (c) the default partition's sections alone: every section on pre-made inputs of its own, no ADD, no host work between
        plain = mr.LceModel(data)
        dt = {mr.INT8: torch.int8, mr.INT32: torch.int32, mr.FLOAT32: torch.float32}
        calls = []
        for k, sec in enumerate(plain.sections):
            ins = [torch.randint(-128, 128, plain.section_tensor_shape(k, t, batch)[0], device=DEV, generator=g, dtype=torch.int8)
                   for t in sec.inputs]
            outs = [torch.empty(plain.section_tensor_shape(k, t, batch)[0], dtype=dt[plain.tensors[t].type], device=DEV) for t in sec.outputs]
            calls.append((k, ins, outs))
        t_c = timed(lambda i: [plain.run_section(k, batch, [a.data_ptr() for a in ins], [o.data_ptr() for o in outs], stream)
                               for k, ins, outs in calls], iters)
    rows += ["body    batch %d, %d layers (%s)" % (batch, len(INT8_BODY), ", ".join("%dx%dx%d->%d%s%s" % (h, h, c, co, " s2" if st == 2 else "", "" if sc else " no shortcut")
                                                                        for h, c, co, st, sc in INT8_BODY)),
             "body    (a) one section (int8 ADD sections), eager          %9.1f us" % t_a,
             "body    (b) one section, HIP-graph replay                   %9.1f us   (graphs recorded / replays: %s; bytes equal to eager: %s)" % (t_b, graphs, same),
             "body    (c) the default partition's %d sections alone, no ADD %9.1f us   (lower bound for any host; a - c = %.1f us, b - c = %.1f us)"
             % (len(plain.sections), t_c, t_a - t_c, t_b - t_c),
             "body    lce_hip_add_int8 launches / LceQuantize folded in (a): %s" % (stats,)]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    iters = 6 if a.quick else a.iters
    print("device:", torch.cuda.get_device_name(DEV))
    for line in kernel_rows(iters) + body_rows(max(4, iters // 2)):
        print(line, flush=True)


if __name__ == "__main__":
    main()
