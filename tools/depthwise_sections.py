#!/usr/bin/env python
"""GPU timing of the float DEPTHWISE_CONV_2D between binary layers (lce_hip_depthwise_conv2d_f32) and of the QuickNet transition
of tests/test_depthwise_sections_host.py at batch 256:
  1. the kernel alone at QuickNet's three transitions, 256x56x56x64, 256x28x28x128 and 256x14x14x256, each 3x3 / 2 SAME with the
     blur weights, with the blurred tensor only and with the bits as well: device-event time per launch and algorithmic bytes
     (input + output, + 1/8 B per output element for the bits, each once) / time as a fraction of 8 TB/s.  The operand sets rotate
     through more than twice the 256 MB Infinity Cache, so every launch reads HBM.  Two yardsticks in the same process,
     interleaved A-B-C-A-B-C for --rounds rounds: lce_hip_pool2d MAX 3x3 / 2 SAME at the same shape (the same input and output
     traffic, no weights, no multiplies) and torch.nn.functional.conv2d(groups=C) on the same memory viewed as channels-last
     NCHW tensors (TFLite's SAME on an even extent pads one row and column BEHIND, which conv2d's symmetric padding cannot say:
     torch is given F.pad's output, prepared OUTSIDE the timed region, which favours torch).  The margin is the spread each
     yardstick shows against itself over the rounds.
  2. the transition (tests' fixture at H = 56, C = 64: LceQuantize, LceBconv2d, MUL, ADD, ADD, MAX_POOL_2D, the blur, CONV_2D 1x1,
     LceQuantize, LceBconv2d, MUL, ADD): (a) ONE section (all four flags), eager, (b) the same as a HIP-graph replay, (c) the same
     file without the depthwise flag: two sections, with torch doing the blur and the 1x1 convolution between them on the device
     (both are the host's then) -- no host copy, so (c) is a floor for what a host that keeps its tensors on the device costs.
The plain-against-non-temporal and cached-against-LDS comparisons are tools/probes/depthwise_loads.hip.
usage: depthwise_sections.py [--iters N] [--rounds R] [--quick]     (--quick: a few iterations, for a run under rocprofv3 --kernel-trace)"""
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
import depthwise_ref as R                                                                 # noqa: E402
from test_depthwise_sections_host import ALL_FLAGS, OLD_FLAGS, quicknet_transition_model  # noqa: E402

DEV = torch.device("cuda:0")
CACHE = 256 << 20
SHAPES = ((56, 64), (28, 128), (14, 256))
F = torch.nn.functional


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


def depthwise_into(desc, x, w, out, bits=None):
    st = torch.cuda.current_stream(DEV).cuda_stream
    amd.check(amd.lib().lce_hip_depthwise_conv2d_f32(C.byref(desc), ptr(x), ptr(w), None, ptr(out), ptr(bits), C.c_void_p(st)))


def pool_into(desc, x, out):
    st = torch.cuda.current_stream(DEV).cuda_stream
    amd.check(amd.lib().lce_hip_pool2d(C.byref(desc), ptr(x), ptr(out), None, C.c_void_p(st)))


def kernel_rows(iters, rounds, batch=256):
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(7)
    for h, c in SHAPES:
        oh = (h + 1) // 2
        n_in, n_out = batch * h * h * c, batch * oh * oh * c
        sets = max(2, math.ceil(2 * CACHE / ((n_in + n_out) * 4)) + 1)
        xs = [torch.randn((batch, h, h, c), device=DEV, generator=gen) for _ in range(sets)]
        outs = [torch.empty((batch, oh, oh, c), device=DEV) for _ in range(sets)]
        bits = [torch.empty((batch, oh, oh, (c + 31) // 32), dtype=torch.int32, device=DEV) for _ in range(sets)]
        blur = np.ascontiguousarray(np.broadcast_to(R.BLUR[None, :, :, None], (1, 3, 3, c)))
        w = torch.from_numpy(blur).to(DEV)
        wt = torch.from_numpy(np.ascontiguousarray(blur[0].transpose(2, 0, 1)[:, None])).to(DEV)      # [C, 1, 3, 3]
        desc = amd.DepthwiseDesc(batch, h, h, c, 1, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE)
        pdesc = amd.Pool2dDesc(amd.POOL_MAX, amd.F32, batch, h, h, c, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE, 1.0, 0)
        # torch: the same memory as channels-last NCHW; TFLite's SAME on an even extent pads one row and column BEHIND, which
        # conv2d's symmetric padding cannot say, so the padded copies are made here, outside the timed region
        nchw = [F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)).contiguous(memory_format=torch.channels_last) for x in xs]
        ours, pool, theirs, with_bits = [], [], [], []
        for _ in range(rounds):
            ours.append(timed(lambda i: depthwise_into(desc, xs[i % sets], w, outs[i % sets]), iters))
            pool.append(timed(lambda i: pool_into(pdesc, xs[i % sets], outs[i % sets]), iters))
            theirs.append(timed(lambda i: F.conv2d(nchw[i % sets], wt, None, stride=2, groups=c), iters))
            with_bits.append(timed(lambda i: depthwise_into(desc, xs[i % sets], w, outs[i % sets], bits[i % sets]), iters))
        name = "f32 256x%dx%dx%d 3x3/2 SAME" % (h, h, c)
        by = (n_in + n_out) * 4
        rows = [("lce_hip_depthwise_conv2d_f32, tensor only  ", ours, by), ("lce_hip_pool2d MAX (yardstick)             ", pool, by),
                ("torch conv2d(groups=C), channels-last      ", theirs, by), ("lce_hip_depthwise_conv2d_f32, tensor + bits", with_bits, by + n_out / 8)]
        for label, t, b in rows:
            med = statistics.median(t)
            lines.append("kernel  %-28s %s median %8.1f us  (min %.1f, max %.1f over %d rounds)  %6.3f TB/s  %.3f of 8 TB/s; bound %.1f us"
                         % (name, label, med, min(t), max(t), rounds, b / med / 1e6, b / med / 1e6 / 8, b / 8e6))
        depthwise_into(desc, xs[0], w, outs[0])
        ref = F.conv2d(nchw[0], wt, None, stride=2, groups=c).permute(0, 2, 3, 1)
        diff = float((outs[0] - ref).abs().max())
        for label, t in (("lce_hip_pool2d", pool), ("torch", theirs)):
            d, spread = statistics.median(ours) - statistics.median(t), max(t) - min(t)
            lines.append("kernel  %-28s depthwise - %s = %+.1f us; %s's own spread %.1f us: %s" % (name, label, d, label, spread,
                         "inside the spread or faster" if d <= spread else "SLOWER by more than the spread"))
        lines.append("kernel  %-28s max |depthwise - torch| = %.3g; %d operand sets" % (name, diff, sets))
        del xs, outs, bits, nchw
        torch.cuda.empty_cache()
    return lines


def section_rows(iters, batch=256, H=56, Cc=64):
    data, xt, out_t, info = quicknet_transition_model(H=H, C=Cc)
    gen = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randn((batch, H, H, Cc), device=DEV, generator=gen) for _ in range(2)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        fused = mr.LceModel(data, **ALL_FLAGS)
        assert len(fused.sections) == 1
        dims, _ = fused.section_tensor_shape(0, out_t, batch)
        y = torch.empty(dims, dtype=torch.float32, device=DEV)
        t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
        stats = fused.depthwise_stats()
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
        # (c) without the depthwise flag: [0..5], the blur and the 1x1 convolution with torch on the device, [8..11]
        cut = mr.LceModel(data, **OLD_FLAGS)
        assert len(cut.sections) == 2
        p_t, t_t = info["tensors"]["p"], info["tensors"]["t"]
        assert cut.sections[0].inputs == [xt] and cut.sections[0].outputs == [p_t]
        assert cut.sections[1].inputs == [t_t] and cut.sections[1].outputs == [out_t]
        p = torch.empty(cut.section_tensor_shape(0, p_t, batch)[0], dtype=torch.float32, device=DEV)
        blur = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(R.BLUR[None, None], (Cc, 1, 3, 3)))).to(DEV)
        w1 = torch.from_numpy(np.ascontiguousarray(info["w"].transpose(0, 3, 1, 2))).to(DEV)          # [2C, 1, 1, C] -> [2C, C, 1, 1]
        b1 = torch.from_numpy(info["wb"]).to(DEV)
        y2 = torch.empty(dims, dtype=torch.float32, device=DEV)

        def cut_run(i):
            cut.run_section(0, batch, [xs[i % 2].data_ptr()], [p.data_ptr()], stream)
            d = F.conv2d(F.pad(p.permute(0, 3, 1, 2), (0, 1, 0, 1)), blur, None, stride=2, groups=Cc)
            t = F.conv2d(d, w1, b1).permute(0, 2, 3, 1).contiguous()
            cut.run_section(1, batch, [t.data_ptr()], [y2.data_ptr()], stream)
        t_c = timed(cut_run, iters)
        cut_run(0)
        s.synchronize()
        close = float((y2 - eager_out).abs().max())
    return ["section batch %d, %dx%dx%d -> %dx%dx%d: LceQuantize, LceBconv2d, MUL, ADD, ADD, MAX_POOL_2D 2x2/1, blur 3x3/2, CONV_2D 1x1, LceQuantize, LceBconv2d, MUL, ADD"
            % (batch, H, H, Cc, H // 2, H // 2, 2 * Cc),
            "section (a) one section (all flags), eager                      %10.1f us   (depthwise launches / LceQuantize folded: %s)" % (t_a, stats),
            "section (b) one section, HIP-graph replay                       %10.1f us   (graphs recorded / replays: %s; bytes equal to eager: %s)" % (t_b, graphs, same),
            "section (c) two sections, torch blur + 1x1 on the device between %9.1f us   (max |c - a| = %.3g: torch's convolutions round differently; a / c = %.3f)"
            % (t_c, close, t_a / t_c)]


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
        for line in section_rows(max(4, iters // 2)):
            print(line, flush=True)


if __name__ == "__main__":
    main()
