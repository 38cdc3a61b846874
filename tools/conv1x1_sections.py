#!/usr/bin/env python
"""GPU timing of the float 1x1 CONV_2D between binary layers (lce_hip_conv1x1_f32) and of the two fixtures of
tests/test_conv1x1_sections_host.py:
  1. the kernel alone at batch 256: 28x28 64 -> 128, 14x14 128 -> 256, 7x7 256 -> 512 (downsampling shortcuts) and 28x28
     320 -> 160 (a dense transition), with the float output only and with the bits as well.  One HIP graph holds one launch per
     operand set, and the sets rotate through more than twice the 256 MB Infinity Cache, so every launch reads HBM; the graph
     is replayed and timed with device events.  Beside each time: the bound max(bytes / 8 TB/s, 2 M N K / 155 TF) (bytes: input +
     filter + output, each once), and torch.nn.functional.conv2d on the same memory viewed as channels-last NCHW tensors, in
     the same process, interleaved A-B-A-B for --rounds rounds.  torch may reorder the sum; this kernel may not (the bytes are
     an fmaf chain in channel order), so the outputs are compared by their largest difference, not for equality.
  2. each fixture (Bi-RealNet-style downsampling block, dense transition) at 56x56, batch 256: ONE section (element-wise +
     pool + conv1x1 sections) eager and as a HIP-graph replay; and at --cut-batch images the same file cut by default, through
     Interpreter.run_section with the NumPy test references on the host for every operator outside the sections, with the
     host's share of that time: a check that the bytes agree and the cost of THIS project's host path, not of a TensorFlow
     Lite host.
  --shift-input: part 1 alone, at 28x28 64 -> 128 alone, with every input one float past a 16-byte boundary, which takes the
  entry to its dword load path (torch is not run on such memory).
usage: conv1x1_sections.py [--iters N] [--rounds R] [--quick] [--kernel-only] [--shift-input]
       (--quick: for a run under rocprofv3 --kernel-trace)"""
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
import conv1x1_ref as R                                                                   # noqa: E402
import pool_ref as PR                                                                     # noqa: E402
from test_conv1x1_sections_host import ALL_FLAGS, FIXTURES                                # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
HBM, MATRIX_F32 = 8e12, 155e12
SHAPES = ((28, 64, 128), (14, 128, 256), (7, 256, 512), (28, 320, 160))       # (H = W, Cin, Cout)


def conv_into(desc, x, w, bias, out, bits, stream):
    amd.check(amd.lib().lce_hip_conv1x1_f32(C.byref(desc), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                                            C.c_void_p(None if bias is None else bias.data_ptr()),
                                            C.c_void_p(None if out is None else out.data_ptr()),
                                            C.c_void_p(None if bits is None else bits.data_ptr()), C.c_void_p(stream)))


def graph_time(fn, sets, iters):
    """us per call of fn(i, stream): one graph of `sets` calls (i = 0 .. sets-1), replayed `iters` times between two events."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(sets):                                          # warm up every operand set eagerly
            fn(i, s.cuda_stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(sets):
                fn(i, torch.cuda.current_stream().cuda_stream)
        g.replay()
        s.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(iters):
            g.replay()
        b.record(s)
        b.synchronize()
    return a.elapsed_time(b) * 1e3 / (iters * sets)


def kernel_rows(iters, rounds, batch=256, shift=False):
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(7)
    for h, cin, cout in SHAPES[:1] if shift else SHAPES:
        m = batch * h * h
        nbytes = (m * cin + cout * cin + m * cout) * 4
        bound_mem, bound_mat = nbytes / HBM * 1e6, 2.0 * m * cout * cin / MATRIX_F32 * 1e6
        sets = max(2, math.ceil(2 * CACHE / nbytes) + 1)
        if shift:                                                        # (allocations are 16-byte aligned: one float behind)
            xs = [torch.randn((m * cin + 1,), device=DEV, generator=gen)[1:].view(batch, h, h, cin) for _ in range(sets)]
            assert all(x.data_ptr() % 16 == 4 for x in xs)
        else:
            xs = [torch.randn((batch, h, h, cin), device=DEV, generator=gen) for _ in range(sets)]
        w = torch.randn((cout, cin), device=DEV, generator=gen) * 0.1
        bias = torch.randn((cout,), device=DEV, generator=gen)
        outs = [torch.empty((batch, h, h, cout), device=DEV) for _ in range(sets)]
        bits = [torch.empty((batch, h, h, (cout + 31) // 32), dtype=torch.int32, device=DEV) for _ in range(sets)]
        desc = amd.Conv1x1Desc(batch, h, h, cin, cout, 1, 1, amd.ACT_NONE)
        nchw = [x.permute(0, 3, 1, 2) for x in xs]                       # the same memory, channels-last
        w4 = w.view(cout, cin, 1, 1).contiguous(memory_format=torch.channels_last)
        ours, with_bits, theirs = [], [], []
        holder = [None] * sets

        def torch_conv(i, stream):
            holder[i] = torch.nn.functional.conv2d(nchw[i], w4, bias)
        how = "HIP graph"
        for _ in range(rounds):                                          # A-B-A-B; the bits variant rides along as a third leg
            ours.append(graph_time(lambda i, st: conv_into(desc, xs[i], w, bias, outs[i], None, st), sets, iters))
            if shift:
                with_bits.append(graph_time(lambda i, st: conv_into(desc, xs[i], w, bias, outs[i], bits[i], st), sets, iters))
                continue
            try:
                theirs.append(graph_time(torch_conv, sets, iters))
            except Exception as e:                                       # (a library that cannot be captured: eager, device events)
                how = "eager (%s)" % type(e).__name__
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for i in range(sets):
                    torch_conv(i, None)
                a.record()
                for k in range(iters * sets):
                    torch_conv(k % sets, None)
                b.record()
                b.synchronize()
                theirs.append(a.elapsed_time(b) * 1e3 / (iters * sets))
            with_bits.append(graph_time(lambda i, st: conv_into(desc, xs[i], w, bias, outs[i], bits[i], st), sets, iters))
        name = "256x%dx%d %d->%d" % (h, h, cin, cout)
        bound = max(bound_mem, bound_mat)
        for label, t in (("lce_hip_conv1x1_f32, float only  ", ours), ("lce_hip_conv1x1_f32, float + bits", with_bits),
                         ("torch conv2d fp32, %-15s" % how, theirs))[:2 if shift else 3]:
            med = statistics.median(t)
            lines.append("kernel  %-22s %s median %8.1f us  (min %.1f, max %.1f over %d rounds)  %5.1f TF  %5.2f TB/s  bound / time %.3f"
                         % (name, label, med, min(t), max(t), rounds, 2.0 * m * cout * cin / med / 1e6, nbytes / med / 1e6, bound / med))
        if shift:
            lines.append("kernel  %-22s the input one float past a 16-byte boundary (the dword load path); %d operand sets" % (name, sets))
            continue
        conv_into(desc, xs[0], w, bias, outs[0], None, torch.cuda.current_stream(DEV).cuda_stream)
        ref = torch.nn.functional.conv2d(nchw[0], w4, bias).permute(0, 2, 3, 1)
        ratio = statistics.median(ours) / statistics.median(theirs)
        lines.append("kernel  %-22s bound max(%.1f us of bytes at 8 TB/s, %.1f us of 2MNK at 155 TF) = %.1f us; ours / torch = %.2f%s; "
                     "max |ours - torch| = %.3g; %d operand sets"
                     % (name, bound_mem, bound_mat, bound, ratio, " (MORE THAN TWICE torch)" if ratio > 2 else "",
                        float((outs[0] - ref).abs().max()), sets))
        del xs, outs, bits, nchw, holder
        torch.cuda.empty_cache()
    return lines


def host_cut_run(it, info, x):
    """The sections of `it` through Interpreter.run_section (NumPy in, NumPy out), every other operator by the NumPy test
    references.  Returns (graph output, seconds spent in the host's operators)."""
    model = it.model
    act = lambda k: model.operators[k].activation
    clamp = lambda v, a: R.clamp(v.astype(np.float32), a)
    host = {info["mul"]: lambda v: clamp(v * info["bn_m"], act(info["mul"])), info["add"]: lambda v: clamp(v + info["bn_a"], act(info["add"]))}
    if "join" in info:
        host[info["join"]] = lambda a, b: (a + b).astype(np.float32)
    for k in info["pools"]:
        o = model.operators[k]
        host[k] = lambda v, o=o: PR.pool2d(v, PR.MAX if o.builtin_code == 17 else PR.AVERAGE, (o.filter_height, o.filter_width),
                                           (o.stride_h, o.stride_w), o.padding, o.activation)
    o = model.operators[info["conv1x1"]]
    host[info["conv1x1"]] = lambda v: R.conv1x1(v, info["w"], info["wb"], (o.stride_h, o.stride_w), o.activation)
    section_of = {op: k for k, sec in enumerate(it.sections) for op in sec.ops}
    live, ran, spent = {model.inputs[0]: x}, set(), 0.0
    for i, op in enumerate(model.operators):
        if i in section_of:
            k = section_of[i]
            if k not in ran:
                ran.add(k)
                live.update(zip(it.sections[k].outputs, it.run_section(k, [live[t] for t in it.sections[k].inputs])))
        else:
            t0 = time.perf_counter()
            live[op.outputs[0]] = host[i](*[live[t] for t in op.inputs if t >= 0 and not model.tensors[t].constant])
            spent += time.perf_counter() - t0
    return live[model.outputs[0]], spent


def fixture_rows(name, iters, batch=256, cut_batch=8, H=56, Cc=64):
    data, xt, out_t, info = FIXTURES[name](H=H, C=Cc)
    gen = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randn((batch, H, H, Cc), device=DEV, generator=gen) for _ in range(2)]
    s = torch.cuda.Stream()

    def timed(fn, n, warmup=3):
        for i in range(warmup):
            fn(i)
        s.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for i in range(n):
            fn(i)
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        fused = mr.LceModel(data, **ALL_FLAGS)
        assert len(fused.sections) == 1
        dims, _ = fused.section_tensor_shape(0, out_t, batch)
        y = torch.empty(dims, dtype=torch.float32, device=DEV)
        t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
        stats = fused.conv1x1_stats()
        fused.use_hip_graphs(True)
        t_b = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters, warmup=6)
        graphs = fused.graph_stats()
        fused.use_hip_graphs(False)
    it = mr.Interpreter(data, batch_size=cut_batch)
    one = mr.Interpreter(data, batch_size=cut_batch, **ALL_FLAGS)
    x_host = xs[0][:cut_batch].cpu().numpy()
    got, _ = host_cut_run(it, info, x_host)
    t0 = time.perf_counter()
    _, spent = host_cut_run(it, info, x_host)
    t_c = time.perf_counter() - t0
    (want,) = one.run_section(0, [x_host])
    t0 = time.perf_counter()
    one.run_section(0, [x_host])
    t_d = time.perf_counter() - t0
    equal = bool(np.array_equal(got.view(np.int32), want.view(np.int32)))
    return ["%-7s batch %d, %dx%d -> %dx%d, %d channels in" % (name, batch, H, H, H // 2, H // 2, Cc),
            "%-7s (a) one section (element-wise + pool + conv1x1 sections), eager  %10.1f us   (lce_hip_conv1x1_f32 launches / LceQuantize folded: %s)"
            % (name, t_a, stats),
            "%-7s (b) one section, HIP-graph replay                              %10.1f us   (graphs recorded / replays: %s)" % (name, t_b, graphs),
            "%-7s (c) batch %d through NumPy arrays: cut by default, %d sections, host operators by the NumPy test references (not a TFLite "
            "host) %.1f ms of which the host's operators %.1f ms; one section %.1f ms; bytes equal: %s"
            % (name, cut_batch, len(it.sections), t_c * 1e3, spent * 1e3, t_d * 1e3, equal)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--shift-input", action="store_true")
    a = ap.parse_args()
    iters = 2 if a.quick else a.iters
    rounds = 1 if a.quick else max(3, a.rounds)
    print("device:", torch.cuda.get_device_name(DEV))
    for line in kernel_rows(iters, rounds, shift=a.shift_input):
        print(line, flush=True)
    if not a.kernel_only and not a.shift_input:
        for name in sorted(FIXTURES):
            for line in fixture_rows(name, max(4, iters // 2)):
                print(line, flush=True)


if __name__ == "__main__":
    main()
