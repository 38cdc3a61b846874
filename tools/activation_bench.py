#!/usr/bin/env python3
"""Do the new step kinds of the elementwise chain cost anything?  The RPReLU tail of a ReActNet block (ADD, PRELU, ADD with the
float output and the sign bits) and the gate MUL of a squeeze-and-excite block through lce_hip_elementwise_ex, against chains that
move the same bytes through lce_hip_elementwise -- ADD, MUL, ADD with per-channel constants and both outputs; one per-channel MUL
with the float output -- from ANOTHER build of the library (--baseline-lib: liblce_hip.so built from the parent commit), in ONE
process, interleaved, several times over, so that the spread between repeats is on the page next to the differences.

    python tools/activation_bench.py --baseline-lib /path/to/parent/liblce_hip.so [--launches 50] [--repeats 5] > profiles/activation/chains.txt

Each figure is microseconds per launch from HIP events around `--launches` back-to-back launches, after the 40 ms clock spin-up
bench.py uses.  The outputs of every variant are checked first: the new chains against tests/activation_ref.py on a slice, the
baseline's chain against this build's lce_hip_elementwise byte for byte."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
amd = importlib.import_module("compute-engine_amd")

SHAPES = ((256, 56, 56, 64), (256, 28, 28, 128))
SPINUP_MS = 40.0


def spin_up(torch, fn, ms=SPINUP_MS):
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()


def event_us(torch, fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None, help="liblce_hip.so of the build to compare with (the parent commit's)")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import activation_ref as AR
    dev = torch.device("cuda:0")
    lib = amd.lib()
    base = None
    if args.baseline_lib:
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        base.lce_hip_elementwise.argtypes = lib.lce_hip_elementwise.argtypes
        assert not hasattr(base, "lce_hip_elementwise_ex"), "--baseline-lib already has the extended entry: not the parent's build"
    print("# us per launch; %d launches per figure, %d interleaved repeats; baseline: %s" % (args.launches, args.repeats, args.baseline_lib))
    for shape in SHAPES:
        b, h, w, c = shape
        g = np.random.default_rng(c)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        x = t(g.standard_normal(shape))
        s1, s2, alpha, m = (t(g.standard_normal(c)) for _ in range(4))
        gate = t(g.uniform(0, 1, (b, 1, 1, c)))
        out = torch.empty_like(x)
        bits = torch.empty((b, h, w, (c + 31) // 32), dtype=torch.int32, device=dev)
        rows = b * h * w
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda a: C.c_void_p(a.data_ptr())
        EX, OLD = amd.EwStepEx, amd.EwStep
        rprelu = (EX * 3)(EX(amd.EW_ADD, amd.EW_PER_CHANNEL, s1.data_ptr(), 0.0, 0), EX(amd.EW_PRELU, amd.EW_PER_CHANNEL, alpha.data_ptr(), 0.0, 0),
                          EX(amd.EW_ADD, amd.EW_PER_CHANNEL, s2.data_ptr(), 0.0, 0))
        gate_mul = (EX * 1)(EX(amd.EW_MUL, amd.EW_PER_IMAGE_CHANNEL, gate.data_ptr(), 0.0, 0))
        ama = (OLD * 3)(OLD(amd.EW_ADD, amd.EW_PER_CHANNEL, s1.data_ptr(), 0.0, 0), OLD(amd.EW_MUL, amd.EW_PER_CHANNEL, m.data_ptr(), 0.0, 0),
                        OLD(amd.EW_ADD, amd.EW_PER_CHANNEL, s2.data_ptr(), 0.0, 0))
        mul = (OLD * 1)(OLD(amd.EW_MUL, amd.EW_PER_CHANNEL, m.data_ptr(), 0.0, 0))
        variants = [
            ("rprelu+bits  ex (this build)", lambda: amd.check(lib.lce_hip_elementwise_ex(p(x), rows, c, h * w, rprelu, 3, p(out), p(bits), stream))),
            ("add,mul,add+bits (this build)", lambda: amd.check(lib.lce_hip_elementwise(p(x), rows, c, ama, 3, p(out), p(bits), stream))),
            ("gate mul     ex (this build)", lambda: amd.check(lib.lce_hip_elementwise_ex(p(x), rows, c, h * w, gate_mul, 1, p(out), None, stream))),
            ("channel mul     (this build)", lambda: amd.check(lib.lce_hip_elementwise(p(x), rows, c, mul, 1, p(out), None, stream))),
        ]
        if base is not None:
            variants.insert(2, ("add,mul,add+bits (baseline)", lambda: amd.check(base.lce_hip_elementwise(p(x), rows, c, ama, 3, p(out), p(bits), stream))))
            variants.append(("channel mul     (baseline)", lambda: amd.check(base.lce_hip_elementwise(p(x), rows, c, mul, 1, p(out), None, stream))))
        # the bytes first: the new chains on the first and the last image against the restatement, the baseline against this build
        xs = x.cpu().numpy()
        variants[0][1]()
        torch.cuda.synchronize()
        for n in (0, b - 1):
            want = AR.chain(xs[n:n + 1], [("add", s1.cpu().numpy(), 0), ("prelu", alpha.cpu().numpy(), 0), ("add", s2.cpu().numpy(), 0)])
            assert np.array_equal(out[n:n + 1].cpu().numpy().view(np.int32), want.view(np.int32)), "rprelu mismatch"
        [v for v in variants if v[0].startswith("gate")][0][1]()
        torch.cuda.synchronize()
        for n in (0, b - 1):
            want = AR.chain(xs[n:n + 1], [("mul", gate[n:n + 1].cpu().numpy(), 0)])
            assert np.array_equal(out[n:n + 1].cpu().numpy().view(np.int32), want.view(np.int32)), "gate mismatch"
        if base is not None:
            variants[1][1]()
            torch.cuda.synchronize()
            mine, mine_bits = out.clone(), bits.clone()
            variants[2][1]()
            torch.cuda.synchronize()
            assert torch.equal(mine.view(torch.int32), out.view(torch.int32)) and torch.equal(mine_bits, bits), "baseline mismatch"
        figures = {name: [] for name, _ in variants}
        spin_up(torch, variants[0][1])
        for _ in range(args.repeats):
            for name, fn in variants:
                fn()
                torch.cuda.synchronize()
                figures[name].append(event_us(torch, fn, args.launches))
        mbytes = rows * c * 4 / 1e6
        print("\n%dx%dx%dx%d  (%.0f MB read, %.0f MB written per launch; bits %.1f MB)" % (b, h, w, c, mbytes, mbytes, mbytes / 32))
        for name, _ in variants:
            v = figures[name]
            print("  %-32s median %7.1f   min %7.1f   max %7.1f   %s" % (name, float(np.median(v)), min(v), max(v), " ".join("%.1f" % f for f in v)))


if __name__ == "__main__":
    main()
