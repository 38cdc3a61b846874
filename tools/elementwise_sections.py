#!/usr/bin/env python
"""GPU timing of the float elementwise tail between binary layers (lce_hip_elementwise) and of the QuickNet body of
tests/test_elementwise_sections_host.py run three ways at batch 256:
  1. the kernel alone at 256 x {56x56x64, 28x28x128, 14x14x256}, "residual + bits" and "BN + residual + bits": device-event
     time per launch, algorithmic bytes (read x, read the residual, write the float result, write the bits: 12.125 B per
     element; the per-channel constants are noise) / time, as a fraction of 8 TB/s.  The input sets rotate through more than
     twice the 256 MB Infinity Cache, so every launch reads HBM.
  2. the body: (a) one section with LCE_TFLITE_SECTIONS_ELEMENTWISE, (b) default-mode sections with the same MUL / ADD / ADD /
     clamp done by torch on the device in between, (c) the convolutions alone (their plans on pre-made inputs).  The
     elementwise share of the chain is (a - c) / a.
usage: elementwise_sections.py [--iters N] [--quick]        (--quick: a few iterations, for a run under rocprofv3)"""
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
from test_elementwise_sections_host import BODY, body_model   # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12
CACHE = 256 << 20


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
    for h, c in ((56, 64), (28, 128), (14, 256)):
        shape = (256, h, h, c)
        n = math.prod(shape)
        set_bytes = n * 12
        sets = max(2, math.ceil(2 * CACHE / set_bytes) + 1)
        g = torch.Generator(device=DEV).manual_seed(c)
        xs = [torch.randn(shape, device=DEV, generator=g) for _ in range(sets)]
        rs = [torch.randn(shape, device=DEV, generator=g) for _ in range(sets)]
        os_ = [torch.empty(shape, device=DEV) for _ in range(sets)]
        bs = [torch.empty(shape[:-1] + (c // 32,), dtype=torch.int32, device=DEV) for _ in range(sets)]
        m, b = torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)
        progs = {"residual + bits": lambda k: [("add", rs[k], amd.ACT_NONE)],
                 "BN + residual + bits": lambda k: [("mul", m, 0), ("add", b, 0), ("add", rs[k], amd.ACT_RELU)]}
        for name, prog in progs.items():
            steps = [prog(k) for k in range(sets)]
            us = timed(lambda i: amd.elementwise(xs[i % sets], steps[i % sets], out=os_[i % sets], out_bits=bs[i % sets]), iters)
            bytes_ = n * 12 + n / 8
            out.append("kernel  256x%dx%dx%-4d %-22s %8.1f us  %6.3f TB/s  %.3f of 8 TB/s  (%d input sets, %.0f MB each)"
                       % (h, h, c, name, us, bytes_ / us / 1e6, bytes_ / us / 1e6 / 8, sets, set_bytes / 2 ** 20))
        del xs, rs, os_, bs
        torch.cuda.empty_cache()
    return out


def body_rows(iters, batch=256):
    data, xt, out_t, info, outs = body_model()
    g = torch.Generator(device=DEV).manual_seed(1)
    xs = [torch.randn((batch, 56, 56, 64), device=DEV, generator=g) for _ in range(2)]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    # (a) one section
    fused = mr.LceModel(data, elementwise_sections=True)
    dims, _ = fused.section_tensor_shape(0, out_t, batch)
    y = torch.empty(dims, device=DEV)
    t_a = timed(lambda i: fused.run_section(0, batch, [xs[i % 2].data_ptr()], [y.data_ptr()], stream), iters)
    # (b) default mode, torch between the sections
    plain = mr.LceModel(data)
    ys = [torch.empty(plain.section_tensor_shape(k, plain.sections[k].outputs[0], batch)[0], device=DEV) for k in range(len(info))]
    consts = [(torch.from_numpy(li["bn_m"]).to(DEV), torch.from_numpy(li["bn_a"]).to(DEV)) for li in info]
    lo_hi = {0: (-3.4028234663852886e38, 3.4028234663852886e38), 1: (0.0, 3.4028234663852886e38)}

    def torch_between(i):
        r = xs[i % 2]
        for k, li in enumerate(info):
            plain.run_section(k, batch, [r.data_ptr()], [ys[k].data_ptr()], stream)
            v = ys[k] * consts[k][0]
            v = v + consts[k][1]
            if li["residual"]:
                v = v + r
            lo, hi = lo_hi[li["act"]]
            r = torch.clamp(v, lo, hi)
        return r
    t_b = timed(torch_between, iters)
    # (c) the convolutions alone, on bits made once
    plans, bits_in, conv_out = [], [], []
    for k, li in enumerate(info):
        sec = plain.sections[k]
        plans.append(plain.bconv2d_plan(sec.ops[1], batch))
        bits_in.append(torch.zeros(plain.section_tensor_shape(k, plain.operators[sec.ops[1]].inputs[0], batch)[0], dtype=torch.int32, device=DEV))
        conv_out.append(torch.empty(ys[k].shape, device=DEV))
    t_c = timed(lambda i: [p.run_ptr(bi.data_ptr(), co.data_ptr(), stream) for p, bi, co in zip(plans, bits_in, conv_out)], iters)
    rows = ["body    batch %d, %d layers (%s)" % (batch, len(BODY), ", ".join("%dx%dx%d->%d%s" % (h, h, c, co, " s2" if s == 2 else "")
                                                                        for h, c, co, s, _ in BODY)),
            "body    (a) one section (elementwise sections)    %9.1f us" % t_a,
            "body    (b) default sections + torch in between   %9.1f us   (a is %.2fx faster)" % (t_b, t_b / t_a),
            "body    (c) the convolutions alone                %9.1f us" % t_c,
            "body    elementwise share of (a): (a - c) / a = %.1f %%   (%.1f us)" % (100 * (t_a - t_c) / t_a, t_a - t_c),
            "body    elementwise launches / ops / LceQuantize folded in (a): %s" % (fused.elementwise_stats(),)]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    iters = 5 if a.quick else a.iters
    print("device:", torch.cuda.get_device_name(DEV))
    for line in kernel_rows(iters) + body_rows(max(3, iters // 5)):
        print(line, flush=True)


if __name__ == "__main__":
    main()
