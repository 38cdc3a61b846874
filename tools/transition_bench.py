#!/usr/bin/env python3
"""Is a QuickNet transition's pool + blur faster as one launch?  Two ways from the transition's input to the blurred map, float32 and
int8, in ONE process and the same build:

    fused : lce_hip_pool_depthwise_f32 / _i8                               (reads the input, writes the blurred map)
    two   : lce_hip_pool2d, then lce_hip_depthwise_conv2d_f32 / _i8         (the pooled map, as large as the input, goes to memory and back)

at the three transitions of QuickNet at batch 256 (56x56x64, 28x28x128, 14x14x256; pool 2x2 / 1 SAME, blur 3x3 / 2 SAME, the value
output alone: the 1x1 convolution reads it).

    python tools/transition_bench.py > profiles/transition/layers.txt

Each figure is microseconds per call from HIP events around replays of a captured HIP graph that holds one call per operand set.
Consecutive calls use DIFFERENT operand sets (input, pooled map, output) in rotation; the header of each table gives the bytes of
all sets together, which must exceed the 256 MiB last-level cache for the figures to be HBM figures.  The two ways alternate,
A-B-A-B, over `--rounds` rounds; a leg's spread is max - min over its rounds.  The bytes of the two ways are compared first."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("compute-engine_amd")

SHAPES = ((256, 56, 56, 64), (256, 28, 28, 128), (256, 14, 14, 256))
Q_IN, Q_OUT = (0.06, -20), (0.06, -18)
BLUR = (np.outer([1, 2, 1], [1, 2, 1]) / 16.0).astype(np.float32)


def event_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def graph_of(torch, calls):
    """A captured graph of the given launches (callables), warmed up."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in calls:
            f()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in calls:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(torch, g, per_graph, window_ms):
    """us per call: replays for at least `window_ms` after a warm-up of a quarter of that."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < window_ms / 4:
        g.replay()
        torch.cuda.synchronize()
    one = event_us(torch, g.replay, 1)
    calls = max(3, int(window_ms * 1e3 / max(one, 1.0)))
    return event_us(torch, g.replay, min(calls, 2000)) / per_graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-mb", type=float, default=640.0, help="least bytes of operand sets in rotation")
    ap.add_argument("--window-ms", type=float, default=30.0)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lib = amd.lib()
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("# us per call from HIP-graph replays (one call per operand set and graph, >= %.0f ms per figure); %d rounds, fused and two "
          "alternating" % (args.window_ms, args.rounds))
    print("# fused = lce_hip_pool_depthwise_*; two = lce_hip_pool2d then lce_hip_depthwise_conv2d_* (both entries as in the parent commit)")
    print("# bytes: the algorithmic traffic -- fused: input + output; two: input + 2 x pooled map + output -- and GB/s = bytes / time")
    summary = []
    for kind, esz in (("f32", 4), ("i8", 1)):
        for shape in SHAPES:
            b, h, w, c = shape
            oh, ow = (h + 1) // 2, (w + 1) // 2
            in_bytes, out_bytes = b * h * w * c * esz, b * oh * ow * c * esz
            n_sets = max(2, int(np.ceil(args.rotate_mb * 1e6 / (2 * in_bytes + out_bytes))))
            g = torch.Generator(device=dev).manual_seed(0)
            if kind == "f32":
                new = lambda s: torch.randn(s, dtype=torch.float32, device=dev, generator=g)
                empty = lambda s: torch.empty(s, dtype=torch.float32, device=dev)
                filt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(BLUR[None, :, :, None], (1, 3, 3, c)))).to(dev)
                third = None
                pool = amd.Pool2dDesc(amd.POOL_MAX, amd.F32, b, h, w, c, 2, 2, 1, 1, amd.PADDING_SAME, amd.ACT_NONE, 1.0, 0)
                dw = amd.DepthwiseDesc(b, h, w, c, 1, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE)
                fused_entry, dw_entry = lib.lce_hip_pool_depthwise_f32, lib.lce_hip_depthwise_conv2d_f32
            else:
                new = lambda s: torch.randint(-128, 128, s, dtype=torch.int8, device=dev, generator=g)
                empty = lambda s: torch.empty(s, dtype=torch.int8, device=dev)
                blur_q = np.rint(BLUR / np.float32(0.25 / 127.0)).astype(np.int8)
                filt_h = np.ascontiguousarray(np.broadcast_to(blur_q[None, :, :, None], (1, 3, 3, c)))
                table = amd.depthwise_conv2d_i8_prepare(filt_h, None, 0.25 / 127.0, Q_IN, Q_OUT)[0]
                filt, third = torch.from_numpy(filt_h).to(dev), torch.from_numpy(table).to(dev)
                pool = amd.Pool2dDesc(amd.POOL_MAX, amd.I8, b, h, w, c, 2, 2, 1, 1, amd.PADDING_SAME, amd.ACT_NONE, Q_IN[0], Q_IN[1])
                dw = amd.DepthwiseI8Desc(b, h, w, c, 1, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE, Q_IN[0], Q_IN[1], Q_OUT[0], Q_OUT[1])
                fused_entry, dw_entry = lib.lce_hip_pool_depthwise_i8, lib.lce_hip_depthwise_conv2d_i8
            sets = [dict(x=new(shape), pooled=empty(shape), out=empty((b, oh, ow, c)), out2=empty((b, oh, ow, c))) for _ in range(n_sets)]

            def fused(s, out="out"):
                amd.check(fused_entry(C.byref(pool), C.byref(dw), ptr(s["x"]), ptr(filt), ptr(third), ptr(s[out]), None, stream()))

            def two(s, out="out"):
                amd.check(lib.lce_hip_pool2d(C.byref(pool), ptr(s["x"]), ptr(s["pooled"]), None, stream()))
                amd.check(dw_entry(C.byref(dw), ptr(s["pooled"]), ptr(filt), ptr(third), ptr(s[out]), None, stream()))
            for s in sets:
                fused(s)
                two(s, "out2")
            torch.cuda.synchronize()
            for s in sets:
                assert torch.equal(s["out"].view(torch.int8), s["out2"].view(torch.int8)), "fused and two launches differ in bytes"
            graphs = [graph_of(torch, [lambda s=s, f=f: f(s) for s in sets]) for f in (fused, two)]
            name = "%s %dx%dx%dx%d" % ((kind,) + shape)
            print("# %s: %d operand sets, %.0f MB in rotation (last-level cache: 268 MB)" % (name, n_sets, n_sets * (2 * in_bytes + 2 * out_bytes) / 1e6))
            print("# %-24s %-6s %10s %10s   fused/two" % ("dtype shape", "round", "fused", "two"))
            table = []
            for r in range(args.rounds):
                figures = [timed(torch, gr, n_sets, args.window_ms) for gr in graphs]
                table.append(figures)
                print("  %-24s %-6d %10.2f %10.2f   %.3f" % (name, r, figures[0], figures[1], figures[0] / figures[1]))
            summary.append((name, in_bytes + out_bytes, 3 * in_bytes + out_bytes, table))
            del graphs, sets
            torch.cuda.empty_cache()
    print("# summary: medians over the rounds; spread = max - min of a leg over its rounds; faster = the two-launch median minus the fused "
          "median exceeds the larger of the two spreads")
    print("# %-24s %10s %10s %8s %8s %10s %10s %10s %10s  %s"
          % ("dtype shape", "fused", "two", "spr_f", "spr_t", "fused/two", "MB_fused", "GB/s_f", "GB/s_two", "faster"))
    for name, bytes_f, bytes_t, table in summary:
        f, t = [row[0] for row in table], [row[1] for row in table]
        mf, mt, sf, st = float(np.median(f)), float(np.median(t)), max(f) - min(f), max(t) - min(t)
        print("  %-24s %10.2f %10.2f %8.2f %8.2f %10.3f %10.1f %10.0f %10.0f  %s"
              % (name, mf, mt, sf, st, mf / mt, bytes_f / 1e6, bytes_f / mf / 1e3, bytes_t / mt / 1e3, "yes" if mt - mf > max(sf, st) else "NO"))


if __name__ == "__main__":
    main()
