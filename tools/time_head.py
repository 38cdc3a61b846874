#!/usr/bin/env python3
"""Does the fully connected kernel of the classifier head earn its place?  lce_hip_fully_connected_f32 against
lce_hip_conv1x1_f32 called on a [batch, 1, 1, K] image -- the same bytes (checked here first) -- in ONE process, one after the
other, three times over, so that the spread between repeats is on the page next to the difference between the two.

    python tools/time_head.py [--launches 200] [--repeats 3] > profiles/head/fc_vs_conv1x1.txt

Each figure is microseconds per launch from HIP events around `--launches` back-to-back launches, after the 40 ms clock spin-up
bench.py uses; `graph` is the same from a captured HIP graph of 20 launches (a ~10 us kernel launched from Python is otherwise
timed at the host's launch rate).  Also timed, for the DESIGN.md paragraph: lce_hip_softmax_f32 on the head's logits."""
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

SHAPES = ((256, 512, 1000), (256, 1024, 1000), (1, 512, 1000), (1, 1024, 1000))     # (batch, K, N)
SPINUP_MS = 40.0


def spin_up(torch, fn, ms=SPINUP_MS):
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        for _ in range(16):
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


def graph_us(torch, fn, launches, per_graph=20):
    """From a captured graph of `per_graph` launches; None when the capture fails."""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(per_graph):
                fn()
        g.replay()
        torch.cuda.synchronize()
        spin_up(torch, g.replay, 10.0)
        return event_us(torch, g.replay, max(5, launches // per_graph)) / per_graph
    except Exception as e:                                           # noqa: BLE001 -- the eager figure still stands
        torch.cuda.synchronize()
        print("# graph capture failed: %r" % (e,))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="launches per timed run (>= 20)")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lib = amd.lib()
    g = np.random.default_rng(0)
    print("# us per launch; eager = events around %d launches, graph = the same from a captured graph of 20" % args.launches)
    print("# %-22s %-9s %s" % ("shape (batch x K -> N)", "repeat", "fc_eager  conv1x1_eager  fc_graph  conv1x1_graph"))
    verdict = []
    for batch, k, n in SHAPES:
        x = torch.from_numpy(g.standard_normal((batch, k)).astype(np.float32)).to(dev)
        w = torch.from_numpy((g.standard_normal((n, k)) * 0.05).astype(np.float32)).to(dev)
        b = torch.from_numpy(g.standard_normal(n).astype(np.float32)).to(dev)
        y_fc, y_cv = torch.empty((batch, n), device=dev), torch.empty((batch, n), device=dev)
        fc_desc = amd.FcDesc(batch, k, n, amd.ACT_NONE)
        cv_desc = amd.Conv1x1Desc(batch, 1, 1, k, n, 1, 1, amd.ACT_NONE)
        ptr = lambda t: C.c_void_p(t.data_ptr())

        def fc():
            amd.check(lib.lce_hip_fully_connected_f32(C.byref(fc_desc), ptr(x), ptr(w), ptr(b), ptr(y_fc),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))

        def conv():
            amd.check(lib.lce_hip_conv1x1_f32(C.byref(cv_desc), ptr(x), ptr(w), ptr(b), ptr(y_cv), None,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        fc()
        conv()
        torch.cuda.synchronize()
        assert torch.equal(y_fc.view(torch.int32), y_cv.view(torch.int32)), "the two paths differ in bytes"
        rows = []
        for r in range(args.repeats):
            figures = []
            for fn in (fc, conv):
                spin_up(torch, fn)
                figures.append(event_us(torch, fn, args.launches))
            for fn in (fc, conv):
                figures.append(graph_us(torch, fn, args.launches))
            rows.append(figures)
            print("  %-22s %-9d %s" % ("%d x %d -> %d" % (batch, k, n), r, "  ".join("%8s" % ("-" if v is None else "%.2f" % v) for v in figures)))
        col = 2 if all(row[2] is not None and row[3] is not None for row in rows) else 0
        fcs, cvs = [row[col] for row in rows], [row[col + 1] for row in rows]
        spread = max(max(fcs) - min(fcs), max(cvs) - min(cvs))
        gain = min(cvs) - max(fcs)
        verdict.append((batch, k, n, "graph" if col else "eager", np.median(fcs), np.median(cvs), spread, gain))
    print("# verdict (%s figures): median fc, median conv1x1, largest spread between repeats, worst-case gain = min conv1x1 - max fc" % verdict[0][3])
    for batch, k, n, _, mf, mc, spread, gain in verdict:
        print("#   %d x %d -> %d: fc %.2f us, conv1x1 %.2f us (x%.2f), spread %.2f us, gain %.2f us: %s"
              % (batch, k, n, mf, mc, mc / mf, spread, gain, "fc wins by more than the spread" if gain > spread else "NO clear win"))
    # the softmax of the head's logits, for the record
    for rows_, cols in ((256, 1000), (1, 1000)):
        z = torch.from_numpy(g.standard_normal((rows_, cols)).astype(np.float32)).to(dev)
        out = torch.empty_like(z)

        def sm():
            amd.check(lib.lce_hip_softmax_f32(rows_, cols, 1.0, ptr(z), ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        spin_up(torch, sm)
        print("# softmax %d x %d: eager %.2f us, graph %s us" % (rows_, cols, event_us(torch, sm, args.launches),
                                                              "%.2f" % (graph_us(torch, sm, args.launches) or float("nan"))))


if __name__ == "__main__":
    main()
