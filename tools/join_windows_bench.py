#!/usr/bin/env python3
"""What does MeliusNet's improvement block -- y = CONCATENATION(x[..., :C-64], x[..., C-64:] + w) -- cost as ONE
lce_hip_join_windows launch, against the same block composed from four launches, and against lce_hip_concat writing the same
output bytes from dense inputs?  In ONE process, alternating, `--repeats` times over, so that the spread between repeats is on the
page next to the differences.

    python tools/join_windows_bench.py [--repeats 5] > profiles/slice/join_windows.txt

  (a) fused     one lce_hip_join_windows launch: windows (x, 0, C-64) and (x, C-64, 64, addend w)
  (b) composed  two one-window lce_hip_join_windows launches (the slices), lce_hip_elementwise (the ADD), lce_hip_concat
  (c) concat    lce_hip_concat of a dense [rows, C-64] and a dense [rows, 64] tensor: the yardstick.  It writes the same output
                bytes and reads as many source bytes as (a) reads of x, but no addend.  It launches the same kernels
                (lce_kernels_join.h) on whole-tensor windows.

Each figure is microseconds per block from HIP events around replays of a captured HIP graph that holds `--per-graph` blocks.
Consecutive blocks of a graph use DIFFERENT operand sets (x, w, y and every intermediate), `--sets` of them in rotation; the sets
together are several times the 256 MiB last-level cache, so every launch reads from and writes to HBM.  A spin-up of replays
precedes every figure.  Algorithmic bytes: (a), (b): x and w read once, y written once = rows x (2 C + 64) x 4; (c): rows x 2 C x 4.
(b)'s launches move more than that (the slices write and the ADD and the CONCATENATION re-read what (a) keeps in registers): its
bytes/s are per ALGORITHMIC byte, for comparison.  The three give the same bytes, checked here first at every shape."""
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

SHAPES = ((256 * 28 * 28, 128), (256 * 28 * 28, 256), (256 * 14 * 14, 320))      # (rows, C)
G = 64


def event_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def graph_of(torch, launches):
    """A captured graph of the given launches (callables), warmed up."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in launches:
            f()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in launches:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(torch, g, per_graph, window_ms):
    """us per block: replays for at least `window_ms` after a spin-up of half of that."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < window_ms / 2:
        g.replay()
        torch.cuda.synchronize()
    one = event_us(torch, g.replay, 1)
    calls = max(3, int(window_ms * 1e3 / max(one, 1.0)))
    return event_us(torch, g.replay, min(calls, 500)) / per_graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4, help="operand sets in rotation")
    ap.add_argument("--per-graph", type=int, default=8, help="blocks per captured graph (a multiple of --sets)")
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--shapes", default="", help="rows:C,rows:C,... (default: the three of the table)")
    args = ap.parse_args()
    assert args.per_graph % args.sets == 0
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lib = amd.lib()
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")] if args.shapes else SHAPES
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def window(t, begin, count, addend=None):
        w = amd.Window()
        w.data_dev, w.pitch, w.begin, w.count = t.data_ptr(), t.shape[1], begin, count
        w.addend_dev = None if addend is None else addend.data_ptr()
        return w

    print("# us per improvement block from HIP-graph replays (%d blocks per graph, %d operand sets in rotation, >= %.0f ms per figure "
          "after a spin-up); %d repeats, alternating" % (args.per_graph, args.sets, args.window_ms, args.repeats))
    print("# fused = one lce_hip_join_windows; composed = 2 x one-window lce_hip_join_windows + lce_hip_elementwise + lce_hip_concat;")
    print("# concat = lce_hip_concat of dense [rows, C-64] and [rows, 64] (the yardstick: the same output bytes, no addend; the same kernels on whole-tensor windows)")
    print("# %-18s %-6s %10s %10s %10s" % ("rows x C", "repeat", "fused", "composed", "concat"))
    summary = []
    for rows, c in shapes:
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        sets = []
        for k in range(args.sets):
            g = torch.Generator(device=dev).manual_seed(k)
            s = dict(x=torch.randn((rows, c), device=dev, generator=g), w=torch.randn((rows, G), device=dev, generator=g),
                     y_a=f32(rows, c), y_b=f32(rows, c), y_c=f32(rows, c), f=f32(rows, c - G), t=f32(rows, G), s=f32(rows, G))
            s["fd"] = s["x"][:, :c - G].contiguous()                    # (c)'s dense inputs: the bytes (a) makes on the way
            s["sd"] = (s["x"][:, c - G:] + s["w"]).contiguous()
            s["wa"] = (amd.Window * 2)(window(s["x"], 0, c - G), window(s["x"], c - G, G, s["w"]))
            s["wf"] = (amd.Window * 1)(window(s["x"], 0, c - G))
            s["wt"] = (amd.Window * 1)(window(s["x"], c - G, G))
            step = (amd.EwStep * 1)()
            step[0].op, step[0].operand, step[0].values, step[0].activation = amd.EW_ADD, amd.EW_TENSOR, s["w"].data_ptr(), amd.ACT_NONE
            s["step"] = step
            s["cat_b"] = ((C.c_void_p * 2)(s["f"].data_ptr(), s["s"].data_ptr()), (C.c_int32 * 2)(c - G, G))
            s["cat_c"] = ((C.c_void_p * 2)(s["fd"].data_ptr(), s["sd"].data_ptr()), (C.c_int32 * 2)(c - G, G))
            sets.append(s)

        def fused(s):
            amd.check(lib.lce_hip_join_windows(amd.F32, s["wa"], 2, rows, 0, ptr(s["y_a"]), None, stream()))

        def composed(s):
            amd.check(lib.lce_hip_join_windows(amd.F32, s["wf"], 1, rows, 0, ptr(s["f"]), None, stream()))
            amd.check(lib.lce_hip_join_windows(amd.F32, s["wt"], 1, rows, 0, ptr(s["t"]), None, stream()))
            amd.check(lib.lce_hip_elementwise(ptr(s["t"]), rows, G, s["step"], 1, ptr(s["s"]), None, stream()))
            amd.check(lib.lce_hip_concat(amd.F32, s["cat_b"][0], s["cat_b"][1], 2, rows, 0, ptr(s["y_b"]), None, stream()))

        def concat(s):
            amd.check(lib.lce_hip_concat(amd.F32, s["cat_c"][0], s["cat_c"][1], 2, rows, 0, ptr(s["y_c"]), None, stream()))
        for s in sets:
            fused(s), composed(s), concat(s)
        torch.cuda.synchronize()
        for s in sets:
            assert torch.equal(s["y_a"].view(torch.int32), s["y_b"].view(torch.int32)), "fused and composed differ in bytes"
            assert torch.equal(s["y_a"].view(torch.int32), s["y_c"].view(torch.int32)), "fused and the yardstick differ in bytes"
        order = [sets[j % args.sets] for j in range(args.per_graph)]
        graphs = [graph_of(torch, [lambda s=s, f=f: f(s) for s in order]) for f in (fused, composed, concat)]
        rows_us = []
        for r in range(args.repeats):
            figures = [timed(torch, g, args.per_graph, args.window_ms) for g in graphs]
            rows_us.append(figures)
            print("  %-18s %-6d %10.2f %10.2f %10.2f" % ("%d x %d" % (rows, c), r, *figures))
        summary.append((rows, c, rows_us))
        del graphs, sets
        torch.cuda.empty_cache()
    print("# summary: medians over the repeats; spread = max - min of a column over the repeats; TB/s per ALGORITHMIC byte")
    print("#   (fused, composed: rows x (2 C + 64) x 4 bytes; concat: rows x 2 C x 4 bytes).  verdict: fused is within the run-to-run")
    print("#   spread of the yardstick when (concat TB/s - fused TB/s) / concat TB/s <= the larger relative spread of the two columns")
    print("# %-18s %9s %9s %9s %8s %8s %8s %9s %9s %9s  %s" % ("rows x C", "fused_us", "comp_us", "concat_us", "spr_f", "spr_comp", "spr_c",
                                                               "fused_TBs", "comp_TBs", "conc_TBs", "fused vs concat per byte"))
    for rows, c, rows_us in summary:
        med = [float(np.median([r[k] for r in rows_us])) for k in range(3)]
        spr = [max(r[k] for r in rows_us) - min(r[k] for r in rows_us) for k in range(3)]
        nbytes = [rows * (2 * c + G) * 4, rows * (2 * c + G) * 4, rows * 2 * c * 4]
        tbs = [nbytes[k] / med[k] * 1e-6 for k in range(3)]
        deficit = (tbs[2] - tbs[0]) / tbs[2]
        allowed = max(spr[0] / med[0], spr[2] / med[2])
        verdict = "within the spread" if deficit <= allowed else "SLOWER by %.1f%% (spread %.1f%%)" % (deficit * 100, allowed * 100)
        if deficit < 0:
            verdict = "faster by %.1f%%" % (-deficit * 100)
        print("  %-18s %9.2f %9.2f %9.2f %8.2f %8.2f %8.2f %9.3f %9.3f %9.3f  %s"
              % ("%d x %d" % (rows, c), *med, *spr, *tbs, verdict))


if __name__ == "__main__":
    main()
