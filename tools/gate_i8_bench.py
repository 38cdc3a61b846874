#!/usr/bin/env python3
"""What does the gate of an int8 squeeze-and-excite block cost?  Three ways to get from the block's int8 output y, its per-image
gate and the shortcut x to the next layer's input, in ONE process, alternating, `--repeats` times over:

    fused : lce_hip_mul_int8 with has_add                      (reads y and x, writes the result: 3 bytes per element + bits)
    split : lce_hip_mul_int8, then lce_hip_add_int8            (the product goes to memory and back: 5 bytes per element + bits)
    add   : lce_hip_add_int8 alone                             (the floor: what the block cost before it had a gate)

each with the bit output only (`_bits`: the next layer's LceQuantize folded, nothing else reads the sum) and with the int8 sum
beside the bits (`_both`: a later shortcut reads it).

    python tools/gate_i8_bench.py [--repeats 3] > profiles/gate_i8/layers.txt

Each figure is microseconds per call from HIP events around replays of a captured HIP graph that holds `--per-graph` calls.
Consecutive calls of a graph use DIFFERENT operand sets (y, x, product, result, bits; the gate is per set too), `--sets` of them in
rotation; the table's header gives the bytes of all sets together, which must exceed the 256 MiB last-level cache for the figures
to be HBM figures.  The bytes of the three ways are checked against each other first (fused == split)."""
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

SHAPES = ((256, 56, 56, 64), (256, 28, 28, 128))
HBM_BYTES_PER_S = 6.29e12
Q_Y, Q_GATE, Q_PRODUCT, Q_X, Q_SUM = (0.05, -3), (1.0 / 256.0, -128), (0.04, 2), (0.06, 5), (0.08, -1)
COLUMNS = ("fused_bits", "fused_both", "split_bits", "split_both", "add_bits", "add_both")


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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets", type=int, default=6, help="operand sets in rotation")
    ap.add_argument("--per-graph", type=int, default=12, help="calls per captured graph (a multiple of --sets)")
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    assert args.per_graph % args.sets == 0
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lib = amd.lib()
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fused_d = amd._mul_int8_desc("bench", Q_Y, Q_GATE, Q_PRODUCT, amd.ACT_NONE, True, (Q_X, Q_SUM, amd.ACT_NONE))
    mul_d = amd._mul_int8_desc("bench", Q_Y, Q_GATE, Q_PRODUCT, amd.ACT_NONE, True, None)
    add_d = amd._add_int8_desc(Q_PRODUCT, Q_X, Q_SUM, amd.ACT_NONE)
    variant = amd.add_int8_params(Q_PRODUCT, Q_X, Q_SUM)["variant"]
    print("# us per call from HIP-graph replays (%d calls per graph, %d operand sets in rotation, >= %.0f ms per figure); %d repeats, "
          "alternating" % (args.per_graph, args.sets, args.window_ms, args.repeats))
    print("# fused = lce_hip_mul_int8 with has_add; split = lce_hip_mul_int8 then lce_hip_add_int8; add = lce_hip_add_int8 alone")
    print("# _bits: bit output only; _both: int8 result and bits.  Per-image gate [b, C] at (1/256, -128); the ADD runs variant %d "
          "(0 literal, 1 split, 2 shift) in all three" % variant)
    summary = []
    for shape in SHAPES:
        b, h, w, c = shape
        rows, rpi = b * h * w, h * w
        g = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *s: torch.randint(-128, 128, s, dtype=torch.int8, device=dev, generator=g)
        sets = [dict(y=rnd(rows, c), gate=rnd(b, c), x=rnd(rows, c), product=torch.empty((rows, c), dtype=torch.int8, device=dev),
                     out=torch.empty((rows, c), dtype=torch.int8, device=dev), out2=torch.empty((rows, c), dtype=torch.int8, device=dev),
                     bits=torch.empty((rows, (c + 31) // 32), dtype=torch.int32, device=dev),
                     bits2=torch.empty((rows, (c + 31) // 32), dtype=torch.int32, device=dev)) for _ in range(args.sets)]
        touched = args.sets * (4 * rows * c + rows * ((c + 31) // 32) * 4)

        def fused(s, both, out="out", bits="bits"):
            amd.check(lib.lce_hip_mul_int8(C.byref(fused_d), ptr(s["y"]), ptr(s["gate"]), ptr(s["x"]), rows, c, rpi,
                                           ptr(s[out]) if both else None, ptr(s[bits]), stream()))

        def split(s, both, out="out", bits="bits"):
            amd.check(lib.lce_hip_mul_int8(C.byref(mul_d), ptr(s["y"]), ptr(s["gate"]), None, rows, c, rpi, ptr(s["product"]), None, stream()))
            amd.check(lib.lce_hip_add_int8(C.byref(add_d), ptr(s["product"]), ptr(s["x"]), rows, c, ptr(s[out]) if both else None,
                                           ptr(s[bits]), stream()))

        def add(s, both):
            amd.check(lib.lce_hip_add_int8(C.byref(add_d), ptr(s["product"]), ptr(s["x"]), rows, c, ptr(s["out"]) if both else None,
                                           ptr(s["bits"]), stream()))
        for s in sets:
            fused(s, True)
            split(s, True, "out2", "bits2")
        torch.cuda.synchronize()
        for s in sets:
            assert torch.equal(s["out"], s["out2"]) and torch.equal(s["bits"], s["bits2"]), "fused and split differ in bytes"
        order = [sets[j % args.sets] for j in range(args.per_graph)]
        kinds = [(fused, False), (fused, True), (split, False), (split, True), (add, False), (add, True)]
        graphs = [graph_of(torch, [lambda s=s, f=f, both=both: f(s, both) for s in order]) for f, both in kinds]
        name = "%dx%dx%dx%d" % shape
        print("# %s: %.0f MB of operands in rotation (last-level cache: 268 MB)" % (name, touched / 1e6))
        print("# %-16s %-6s " % ("shape", "repeat") + " ".join("%10s" % n for n in COLUMNS) + "   fused/split (both)")
        table = []
        for r in range(args.repeats):
            figures = [timed(torch, gr, args.per_graph, args.window_ms) for gr in graphs]
            table.append(figures)
            print("  %-16s %-6d " % (name, r) + " ".join("%10.2f" % v for v in figures) + "   %.3f" % (figures[1] / figures[3]))
        summary.append((name, rows * c, rows * ((c + 31) // 32) * 4, table))
        del graphs, sets
        torch.cuda.empty_cache()
    print("# summary: medians over the repeats.  hbm_us: the algorithmic bytes of the _both column (fused and add: 3 bytes per element + "
          "bits, split: 5 + bits; the gate is negligible) at 6.29 TB/s, the measured HBM copy rate")
    print("# below = the fused figure of EVERY repeat is under the split figure of every repeat, for _bits and for _both")
    print("# %-16s " % "shape" + " ".join("%10s" % n for n in COLUMNS) + " %11s %11s %9s %9s  %s"
          % ("fused/split", "fused/add", "hbm_fused", "hbm_split", "below"))
    for name, elems, bit_bytes, table in summary:
        med = [float(np.median([row[k] for row in table])) for k in range(6)]
        below = all(max(row[a] for row in table) < min(row[b] for row in table) for a, b in ((0, 2), (1, 3)))
        print("  %-16s " % name + " ".join("%10.2f" % v for v in med) + " %11.3f %11.3f %9.2f %9.2f  %s"
              % (med[1] / med[3], med[1] / med[5], (3 * elems + bit_bytes) / HBM_BYTES_PER_S * 1e6,
                 (5 * elems + bit_bytes) / HBM_BYTES_PER_S * 1e6, "yes" if below else "NO"))


if __name__ == "__main__":
    main()
