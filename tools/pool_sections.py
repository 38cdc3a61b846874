#!/usr/bin/env python
"""GPU timing of the 2-D pooling between binary layers (lce_hip_pool2d) and of the AlexNet-style body of
tests/test_pool_sections_host.py at batch 256:
  1. the kernel alone at float 256x56x56x64 and 256x28x28x192 (MAX 3x3 / 2 VALID), float 256x28x28x256 (MAX and AVERAGE 2x2 / 2)
     and int8 256x28x28x256 (AVERAGE 2x2 / 2), each with the pooled tensor only and with the bits as well: device-event time per
     launch and algorithmic bytes (input + output, + 1/8 B per output element for the bits, each once) / time as a fraction of
     8 TB/s.  The operand sets rotate through more than twice the 256 MB Infinity Cache, so every launch reads HBM.  The
     yardstick for float is torch.nn.functional.max_pool2d / avg_pool2d on the same memory viewed as channels-last NCHW tensors,
     in the same process, interleaved A-B-A-B for --rounds rounds; the margin is the spread torch shows against itself over the
     rounds.  torch has no int8 pooling: the int8 rows stand alone.
  2. the body (15x15 -> 7x7 -> 4x4 at 64 channels is the test's; here H = 57 -> 28 -> 14, 256 channels): (a) ONE section
     (elementwise + pool sections), eager, (b) the same as a HIP-graph replay, (c) the default partition through
     Interpreter.run_section with the NumPy test reference on the host for every operator outside the sections: a check that the
     bytes agree and the cost of THIS project's host path, not of a TensorFlow Lite host -- no measure of the feature's gain.
The plain-against-non-temporal comparison of the window loads is tools/probes/pool_loads.hip.
usage: pool_sections.py [--iters N] [--rounds R] [--quick]     (--quick: a few iterations, for a run under rocprofv3 --kernel-trace)"""
import argparse
import ctypes as C
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
import pool_ref as R                                                                      # noqa: E402
from test_pool_sections_host import alexnet_body_model                                    # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
# (dtype, H, C, op, filter, stride)
SHAPES = (("f32", 56, 64, amd.POOL_MAX, 3, 2), ("f32", 28, 192, amd.POOL_MAX, 3, 2), ("f32", 28, 256, amd.POOL_MAX, 2, 2),
          ("f32", 28, 256, amd.POOL_AVERAGE, 2, 2), ("i8", 28, 256, amd.POOL_AVERAGE, 2, 2))


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


def pool_into(desc, x, out, bits=None, stream=None):
    """lce_hip_pool2d into existing tensors (amd.pool2d allocates its outputs)."""
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    amd.check(amd.lib().lce_hip_pool2d(C.byref(desc), C.c_void_p(x.data_ptr()), C.c_void_p(None if out is None else out.data_ptr()),
                                       C.c_void_p(None if bits is None else bits.data_ptr()), C.c_void_p(st)))


def kernel_rows(iters, rounds, batch=256):
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(7)
    for kind, h, c, op, f, s in SHAPES:
        oh = (h - f) // s + 1
        esz = 4 if kind == "f32" else 1
        n_in, n_out = batch * h * h * c, batch * oh * oh * c
        sets = max(2, math.ceil(2 * CACHE / ((n_in + n_out) * esz)) + 1)
        if kind == "f32":
            xs = [torch.randn((batch, h, h, c), device=DEV, generator=gen) for _ in range(sets)]
        else:
            xs = [torch.randint(-128, 128, (batch, h, h, c), dtype=torch.int8, device=DEV, generator=gen) for _ in range(sets)]
        outs = [torch.empty((batch, oh, oh, c), dtype=xs[0].dtype, device=DEV) for _ in range(sets)]
        bits = [torch.empty((batch, oh, oh, (c + 31) // 32), dtype=torch.int32, device=DEV) for _ in range(sets)]
        desc = amd.Pool2dDesc(op, amd.F32 if kind == "f32" else amd.I8, batch, h, h, c, f, f, s, s, amd.PADDING_VALID, amd.ACT_NONE, 0.05, -3)
        ours, theirs, with_bits = [], [], []
        torch_pool = torch.nn.functional.max_pool2d if op == amd.POOL_MAX else torch.nn.functional.avg_pool2d
        nchw = [x.permute(0, 3, 1, 2) for x in xs]                    # the same memory, channels-last
        for _ in range(rounds):                                       # A-B-A-B; the bits variant rides along as a third leg
            ours.append(timed(lambda i: pool_into(desc, xs[i % sets], outs[i % sets]), iters))
            if kind == "f32":
                theirs.append(timed(lambda i: torch_pool(nchw[i % sets], f, s), iters))
            with_bits.append(timed(lambda i: pool_into(desc, xs[i % sets], outs[i % sets], bits[i % sets]), iters))
        name = "%s 256x%dx%dx%d %s %dx%d/%d" % (kind, h, h, c, "MAX" if op == amd.POOL_MAX else "AVERAGE", f, f, s)
        rows = [("lce_hip_pool2d, pooled only ", ours, (n_in + n_out) * esz), ("lce_hip_pool2d, pooled + bits", with_bits, (n_in + n_out) * esz + n_out / 8)]
        if theirs:
            rows.insert(1, ("torch %-22s" % torch_pool.__name__, theirs, (n_in + n_out) * esz))
        for label, t, b in rows:
            med = statistics.median(t)
            lines.append("kernel  %-34s %s median %8.1f us  (min %.1f, max %.1f over %d rounds)  %6.3f TB/s  %.3f of 8 TB/s"
                         % (name, label, med, min(t), max(t), rounds, b / med / 1e6, b / med / 1e6 / 8))
        if theirs:
            pool_into(desc, xs[0], outs[0])
            ref = torch_pool(nchw[0], f, s).permute(0, 2, 3, 1)
            equal = bool(torch.equal(outs[0], ref)) if op == amd.POOL_MAX else "max |diff| %.3g" % float((outs[0] - ref).abs().max())
            d, spread = statistics.median(ours) - statistics.median(theirs), max(theirs) - min(theirs)
            lines.append("kernel  %-34s lce_hip_pool2d - torch = %+.1f us; torch's own spread %.1f us: %s; against torch: %s; %d operand sets"
                         % (name, d, spread, "inside the spread or faster" if d <= spread else "SLOWER by more than the spread", equal, sets))
        del xs, outs, bits, nchw
        torch.cuda.empty_cache()
    return lines


def host_cut_run(it, info, x):
    """(c): the sections of `it` through Interpreter.run_section (NumPy in, NumPy out), every other operator in NumPy."""
    model = it.model
    host = {info["mul"]: lambda v: v * info["bn_m"], info["add"]: lambda v: v + info["bn_a"]}
    for k in info["pools"]:
        o = model.operators[k]
        host[k] = lambda v, o=o: R.pool2d(v, R.MAX if o.builtin_code == 17 else R.AVERAGE, (o.filter_height, o.filter_width),
                                          (o.stride_h, o.stride_w), o.padding, o.activation)
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


def body_rows(iters, batch=256, H=57, Cc=256):
    data, xt, out_t, info = alexnet_body_model(H=H, C=Cc)
    gen = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randn((batch, H, H, Cc), device=DEV, generator=gen) for _ in range(2)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        fused = mr.LceModel(data, elementwise_sections=True, pool_sections=True)
        assert len(fused.sections) == 1
        dims, _ = fused.section_tensor_shape(0, out_t, batch)
        y = torch.empty(dims, dtype=torch.float32, device=DEV)
        t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
        stats = fused.pool_stats()
        eager_out = y.clone()
        fused.use_hip_graphs(True)
        t_b = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters, warmup=6)
        graphs = fused.graph_stats()
        fused.run_section(0, batch, [xs[(iters - 1) % 2].data_ptr()], [y.data_ptr()], stream)
        s.synchronize()
        same = bool(torch.equal(y.view(torch.int32), eager_out.view(torch.int32)))
        fused.use_hip_graphs(False)
    it = mr.Interpreter(data, batch_size=batch)
    x_host = xs[0].cpu().numpy()
    got = host_cut_run(it, info, x_host)
    hosts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_cut_run(it, info, x_host)
        hosts.append((time.perf_counter() - t0) * 1e6)
    t_c = statistics.median(hosts)
    fused.run_section(0, batch, [xs[0].data_ptr()], [y.data_ptr()], 0)
    torch.cuda.synchronize()
    close = bool(np.array_equal(got.view(np.int32), y.cpu().numpy().view(np.int32)))
    sizes = info["sizes"]
    return ["body    batch %d, %dx%d -> %dx%d -> %dx%d, %d channels, MAX 3x3 / 2 VALID and AVERAGE 2x2 / 2 SAME"
            % (batch, sizes[0], sizes[0], sizes[1], sizes[1], sizes[2], sizes[2], Cc),
            "body    (a) one section (elementwise + pool sections), eager   %10.1f us   (lce_hip_pool2d launches / LceQuantize folded: %s)" % (t_a, stats),
            "body    (b) one section, HIP-graph replay                      %10.1f us   (graphs recorded / replays: %s; bytes equal to eager: %s)" % (t_b, graphs, same),
            "body    (c) default partition, pools and batch norm by the NumPy test reference on the host (not a TFLite host) %10.1f us   (median of 3, host clock; %d sections; "
            "bytes equal to (a): %s; a / c = %.4f)" % (t_c, len(it.sections), close, t_a / t_c)]


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
        for line in body_rows(max(4, iters // 2)):
            print(line, flush=True)


if __name__ == "__main__":
    main()
