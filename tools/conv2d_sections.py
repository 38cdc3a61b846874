#!/usr/bin/env python
"""GPU timing of the float KxK CONV_2D (lce_hip_conv2d_f32) and of the stem fixtures of tests/test_conv2d_sections_host.py at
batch 256:
  1. the kernel alone at the three stems -- 224x224x3 -> 3x3 / 2 SAME -> 32 (QuickNet), 224x224x3 -> 7x7 / 2 SAME -> 64
     (Bi-RealNet, BinaryResNetE, BinaryDenseNet), 227x227x3 -> 11x11 / 4 VALID -> 64 (BinaryAlexNet) -- with bias and RELU, the
     float tensor only: device-event time per call (both launches of it), against its byte bound (the output written once at
     8 TB/s; the input is 3 channels and the filter a few KB) and against torch.nn.functional.conv2d in fp32 on the same memory
     viewed as channels-last NCHW (TFLite's SAME pads unevenly, which conv2d's symmetric padding cannot say: torch is given
     F.pad's output, prepared OUTSIDE the timed region, which favours torch).  The operand sets rotate through more than twice
     the 256 MB Infinity Cache.  Interleaved A-B-A-B for --rounds rounds; the margin is torch's own spread over the rounds.
  2. each stem fixture with a 224 input (227 for BinaryAlexNet): (a) ONE section (every flag), eager, (b) the same as a HIP-graph
     replay, (c) as the parent commit runs it: the stem by torch on the device, the body as its sections -- no host copy, so (c)
     is a floor for a host that keeps its tensors on the device.
usage: conv2d_sections.py [--iters N] [--rounds R] [--quick] [--batch B]"""
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
import pool_ref as PR                                                                                        # noqa: E402
from test_conv2d_sections_host import ALL_FLAGS, PARENT_FLAGS, alexnet_stem_model, bireal_stem_model, quicknet_stem_model  # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
# (name, input extent, filter, stride, padding, Cout)
STEMS = (("quicknet 3x3/2 SAME -> 32", 224, 3, 2, amd.PADDING_SAME, 32), ("bireal 7x7/2 SAME -> 64", 224, 7, 2, amd.PADDING_SAME, 64),
         ("alexnet 11x11/4 VALID -> 64", 227, 11, 4, amd.PADDING_VALID, 64))
F = torch.nn.functional
ACT = {0: lambda v: v, 1: torch.relu, 2: lambda v: v.clamp(-1, 1), 3: lambda v: v.clamp(0, 6)}


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


def ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def pads(size, filt, stride, padding):
    """(before, behind) of TFLite's padding rule."""
    out, before = PR.out_and_pad(size, filt, stride, padding)
    return before, max(0, (out - 1) * stride + filt - size) - before


def kernel_rows(iters, rounds, batch):
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(7)
    for name, size, filt, stride, padding, cout in STEMS:
        oh = PR.out_and_pad(size, filt, stride, padding)[0]
        n_in, n_out = batch * size * size * 3, batch * oh * oh * cout
        sets = max(2, math.ceil(2 * CACHE / ((n_in + n_out) * 4)) + 1)
        xs = [torch.randn((batch, size, size, 3), device=DEV, generator=gen) for _ in range(sets)]
        outs = [torch.empty((batch, oh, oh, cout), device=DEV) for _ in range(sets)]
        w = torch.randn((cout, filt, filt, 3), device=DEV, generator=gen) * 0.2
        bias = torch.randn((cout,), device=DEV, generator=gen)
        desc = amd.Conv2dDesc(batch, size, size, 3, cout, filt, filt, stride, stride, padding, amd.ACT_RELU)
        st = torch.cuda.current_stream(DEV).cuda_stream
        ours_fn = lambda i: amd.check(amd.lib().lce_hip_conv2d_f32(C.byref(desc), ptr(xs[i % sets]), ptr(w), ptr(bias), ptr(outs[i % sets]),
                                                                 None, C.c_void_p(st)))
        before, behind = pads(size, filt, stride, padding)
        nchw = [F.pad(x.permute(0, 3, 1, 2), (before, behind, before, behind)).contiguous(memory_format=torch.channels_last) for x in xs]
        wt = w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        theirs_fn = lambda i: torch.relu_(F.conv2d(nchw[i % sets], wt, bias, stride=stride))
        ours, theirs = [], []
        for _ in range(rounds):
            ours.append(timed(ours_fn, iters))
            theirs.append(timed(theirs_fn, iters))
        ours_fn(0)
        diff = float((outs[0] - theirs_fn(0).permute(0, 2, 3, 1)).abs().max())
        label = "f32 %dx%dx%dx3 %s" % (batch, size, size, name)
        bound = n_out * 4 / 8e6
        flop = 2.0 * n_out * filt * filt * 3
        for who, t in (("lce_hip_conv2d_f32       ", ours), ("torch conv2d channels-last", theirs)):
            med = statistics.median(t)
            lines.append("kernel  %-52s %s median %9.1f us  (min %.1f, max %.1f over %d rounds)  %.2f x the byte bound of %.1f us; %.1f TFLOP/s"
                         % (label, who, med, min(t), max(t), rounds, med / bound, bound, flop / med / 1e6))
        d, spread = statistics.median(ours) - statistics.median(theirs), max(theirs) - min(theirs)
        lines.append("kernel  %-52s conv2d - torch = %+.1f us; torch's own spread %.1f us: %s; max |conv2d - torch| = %.3g; %d operand sets"
                     % (label, d, spread, "inside the spread or faster" if d <= spread else "SLOWER by more than the spread", diff, sets))
        del xs, outs, nchw
        torch.cuda.empty_cache()
    return lines


def torch_stem(stem_ops, size):
    """The stem operators as torch calls on an NHWC device tensor (what a host that keeps its tensors on the device would run)."""
    steps = []
    for op in stem_ops:
        if op[0] == "conv":
            _, w, b, stride, padding, act = op
            wt = torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))).to(DEV)
            bt = torch.from_numpy(b).to(DEV)
            pb = pads(size, w.shape[1], stride, padding)
            steps.append(lambda v, wt=wt, bt=bt, pb=pb, stride=stride, act=act:
                         ACT[act](F.conv2d(F.pad(v.permute(0, 3, 1, 2), pb + pb), wt, bt, stride=stride)).permute(0, 2, 3, 1))
            size = PR.out_and_pad(size, w.shape[1], stride, padding)[0]
        elif op[0] == "depthwise":
            _, k, stride, padding = op
            kt = torch.from_numpy(np.ascontiguousarray(k[0].transpose(2, 0, 1)[:, None])).to(DEV)
            pb = pads(size, k.shape[1], stride, padding)
            steps.append(lambda v, kt=kt, pb=pb, stride=stride:
                         F.conv2d(F.pad(v.permute(0, 3, 1, 2), pb + pb), kt, None, stride=stride, groups=kt.shape[0]).permute(0, 2, 3, 1))
            size = PR.out_and_pad(size, k.shape[1], stride, padding)[0]
        elif op[0] == "pool":
            _, filt, stride, padding = op
            pb = pads(size, filt, stride, padding)
            steps.append(lambda v, pb=pb, filt=filt, stride=stride:
                         F.max_pool2d(F.pad(v.permute(0, 3, 1, 2), pb + pb, value=float("-inf")), filt, stride).permute(0, 2, 3, 1))
            size = PR.out_and_pad(size, filt, stride, padding)[0]
        else:
            c = torch.from_numpy(op[1]).to(DEV)
            steps.append((lambda v, c=c: v * c) if op[0] == "mul" else (lambda v, c=c: v + c))

    def run(v):
        for s in steps:
            v = s(v)
        return v.contiguous()
    return run


def section_rows(iters, batch):
    lines = []
    for name, make, size in (("quicknet", quicknet_stem_model, 224), ("bireal", bireal_stem_model, 224), ("alexnet", alexnet_stem_model, 227)):
        data, xt, out_t, info = make(size=size)
        gen = torch.Generator(device=DEV).manual_seed(1)
        xs = [torch.randn((batch,) + info["shape"], device=DEV, generator=gen) for _ in range(2)]
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            stream = s.cuda_stream
            fused = mr.LceModel(data, **ALL_FLAGS)
            assert len(fused.sections) == 1 and fused.sections[0].inputs == [xt]
            dims, _ = fused.section_tensor_shape(0, out_t, batch)
            y = torch.empty(dims, dtype=torch.float32, device=DEV)
            t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
            stats = fused.conv2d_stats()
            fused.run_section(0, batch, [xs[0].data_ptr()], [y.data_ptr()], stream)
            s.synchronize()
            eager_out = y.clone()
            fused.use_hip_graphs(True)
            t_b = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters, warmup=6)
            graphs = fused.graph_stats()
            fused.run_section(0, batch, [xs[0].data_ptr()], [y.data_ptr()], stream)
            s.synchronize()
            same = bool(torch.equal(y.view(torch.int32), eager_out.view(torch.int32)))
            fused.use_hip_graphs(False)
            # (c) the parent's partition: the stem with torch on the device, then the body's section
            cut = mr.LceModel(data, **PARENT_FLAGS)
            assert [sec.ops for sec in cut.sections] == info["parent_sections"] and len(cut.sections) == 1
            sec = cut.sections[0]
            stem = torch_stem(info["stem_ops"], size)
            y2 = torch.empty(dims, dtype=torch.float32, device=DEV)
            assert sec.outputs == [out_t] and len(sec.inputs) == 1

            def cut_run(i):
                v = stem(xs[i % 2])
                cut.run_section(0, batch, [v.data_ptr()], [y2.data_ptr()], stream)
            t_c = timed(cut_run, iters)
            cut_run(0)
            s.synchronize()
            differ = float((y2 != eager_out).float().mean())
        lines += ["section %-8s batch %d, %s input: %d operators, stem %s" % (name, batch, "x".join(map(str, info["shape"])), len(fused.operators),
                                                                            [o[0] for o in info["stem_ops"]]),
                  "section %-8s (a) one section (every flag), eager         %10.1f us   (conv2d calls / LceQuantize folded: %s)" % (name, t_a, stats),
                  "section %-8s (b) one section, HIP-graph replay           %10.1f us   (graphs recorded / replays: %s; bytes equal to eager: %s)"
                  % (name, t_b, graphs, same),
                  "section %-8s (c) torch stem on the device + body section %10.1f us   (a / c = %.3f; %.4f of the outputs differ: torch's convolutions "
                  "round differently and the binary layer amplifies a flipped sign)" % (name, t_c, t_a / t_c, differ)]
        del xs
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    iters = 3 if a.quick else a.iters
    rounds = 1 if a.quick else max(3, a.rounds)
    print("device:", torch.cuda.get_device_name(DEV))
    for line in kernel_rows(iters, rounds, a.batch):
        print(line, flush=True)
    if not a.kernel_only:
        for line in section_rows(max(3, iters // 2), a.batch):
            print(line, flush=True)


if __name__ == "__main__":
    main()
