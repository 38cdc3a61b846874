#!/usr/bin/env python3
"""What does a binarized Dense layer cost on the FP4 matrix cores, against what the library did for the same layer before?
lce_hip_binary_fully_connected on the bits (value output, and bits-only output: a hidden layer) against lce_hip_unpack +
lce_hip_fully_connected_f32 on the float weights, in ONE process, alternating, `--repeats` times over, so that the spread
between repeats is on the page next to the difference.

    python tools/binary_dense_bench.py [--repeats 3] [--baseline-lib <parent build>/liblce_hip.so] > profiles/binary_dense/layers.txt

The old path's two entries are taken from `--baseline-lib` when given (another build of the library, loaded beside this one as
tools/activation_bench.py does); by default from THIS build, whose lce_hip_unpack and lce_hip_fully_connected_f32 kernels
(lce_kernels.h, lce_kernels_head.h) are the parent commit's, unchanged.  The table's header says which.

Each figure is microseconds per layer from HIP events around replays of a captured HIP graph that holds `--per-graph` layers
(a 10 us kernel launched from Python is otherwise timed at the host's launch rate).  Consecutive layers of a graph use DIFFERENT
operand sets (activations, weights, outputs), `--sets` of them in rotation, so that no launch finds its own operands in L2.  The
bit weights of all sets together (19 MB for 9216 -> 4096) still fit the 256 MiB last-level cache, as one layer's would between the
batches of a network; the float weights (151 MB per set) do not.  So the new entry is timed with its weights cached on the die and
the old one from HBM, while the bytes roofline is taken at the HBM rate: the table's header repeats this.  Power-of-two scales:
the two paths give the same bytes, checked here first at every shape.

Also printed per row: the algorithmic bytes of the new entry (bit operands, scales, bias, the output), its multiply-accumulates,
and the least time the hardware could take -- bytes at 6.29 TB/s (the measured HBM copy rate) against MACs at 4.2e15 MAC/s (the
measured FP4 rate of tools/probes/mfma_fp4_peak.hip) -- and which of the two binds."""
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

SHAPES = ((9216, 4096), (4096, 4096), (4096, 1000), (512, 1000))      # (K, N)
BATCHES = (1, 16, 256, 2048)
HBM_BYTES_PER_S = 6.29e12
FP4_MAC_PER_S = 4.2e15


def event_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def graph_of(torch, layers):
    """A captured graph of the given launches (callables), warmed up."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in layers:
            f()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in layers:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(torch, g, per_graph, window_ms):
    """us per layer: replays for at least `window_ms` after a warm-up of a quarter of that."""
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
    ap.add_argument("--sets", type=int, default=4, help="operand sets in rotation")
    ap.add_argument("--per-graph", type=int, default=8, help="layers per captured graph (a multiple of --sets)")
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--shapes", default="", help="K:N,K:N,... (default: the four layers of the table)")
    ap.add_argument("--batches", default="", help="comma separated (default: 1,16,256,2048)")
    ap.add_argument("--baseline-lib", default="", help="another build's liblce_hip.so for the old path (default: this build)")
    args = ap.parse_args()
    assert args.per_graph % args.sets == 0
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lib = amd.lib()
    old_lib = lib
    if args.baseline_lib:
        old_lib = C.CDLL(os.path.abspath(args.baseline_lib))
        old_lib.lce_hip_unpack.argtypes = lib.lce_hip_unpack.argtypes
        old_lib.lce_hip_fully_connected_f32.argtypes = lib.lce_hip_fully_connected_f32.argtypes
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")] if args.shapes else SHAPES
    batches = [int(v) for v in args.batches.split(",")] if args.batches else BATCHES
    rng = np.random.default_rng(0)
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("# us per layer from HIP-graph replays (%d layers per graph, %d operand sets in rotation, >= %.0f ms per figure); "
          "%d repeats, alternating" % (args.per_graph, args.sets, args.window_ms, args.repeats))
    print("# new = lce_hip_binary_fully_connected (value: float output; bits: bit output only); old = lce_hip_unpack + lce_hip_fully_connected_f32")
    print("# old path from: %s" % (os.path.basename(os.path.dirname(os.path.abspath(args.baseline_lib))) + "/liblce_hip.so (--baseline-lib)" if args.baseline_lib
                                   else "this build (its unpack and float fully-connected kernels are the parent commit's, unchanged)"))
    print("# the rotated bit weights (at most 4 x 4.7 MB) stay in the 256 MiB last-level cache, the rotated float weights (up to 4 x 151 MB) do not:")
    print("#   new is timed with its weights cached on the die, old from HBM; the bytes roofline below is taken at the HBM rate all the same")
    print("# %-22s %-6s %10s %10s %10s   %s" % ("layer (batch x K -> N)", "repeat", "new_value", "new_bits", "old", "old / new_value"))
    summary = []
    for k, n in shapes:
        kw = (k + 31) // 32
        sets = []
        for _ in range(args.sets):
            sign = rng.integers(0, 2, (n, k)).astype(bool)
            scale = np.exp2(rng.integers(-6, 0, n)).astype(np.float32)
            w = np.where(sign, -scale[:, None], scale[:, None]).astype(np.float32)
            wb, sc = amd.bfc_prepare(w)
            sets.append(dict(w=torch.from_numpy(w).to(dev), wb=torch.from_numpy(wb).to(dev), sc=torch.from_numpy(sc).to(dev),
                             bias=torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)))
            del w, sign
        for batch in batches:
            for s in sets:
                s["a"] = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (batch, kw), dtype=np.int64).astype(np.int32)).to(dev)
                s["x"] = torch.empty((batch, k), dtype=torch.float32, device=dev)
                s["y_new"] = torch.empty((batch, n), dtype=torch.float32, device=dev)
                s["y_old"] = torch.empty((batch, n), dtype=torch.float32, device=dev)
                s["bits"] = torch.empty((batch, (n + 31) // 32), dtype=torch.int32, device=dev)
            bdesc = amd.BfcDesc(batch, k, n, amd.ACT_NONE)
            fdesc = amd.FcDesc(batch, k, n, amd.ACT_NONE)

            def new_value(s):
                amd.check(lib.lce_hip_binary_fully_connected(C.byref(bdesc), ptr(s["a"]), ptr(s["wb"]), ptr(s["sc"]), ptr(s["bias"]),
                                                             ptr(s["y_new"]), None, stream()))

            def new_bits(s):
                amd.check(lib.lce_hip_binary_fully_connected(C.byref(bdesc), ptr(s["a"]), ptr(s["wb"]), ptr(s["sc"]), ptr(s["bias"]),
                                                             None, ptr(s["bits"]), stream()))

            def old(s):
                amd.check(old_lib.lce_hip_unpack(amd.F32, ptr(s["a"]), batch, k, C.c_float(1.0), 0, ptr(s["x"]), stream()))
                amd.check(old_lib.lce_hip_fully_connected_f32(C.byref(fdesc), ptr(s["x"]), ptr(s["w"]), ptr(s["bias"]), ptr(s["y_old"]), stream()))
            for s in sets:
                new_value(s)
                new_bits(s)
                old(s)
            torch.cuda.synchronize()
            for s in sets:
                assert torch.equal(s["y_new"].view(torch.int32), s["y_old"].view(torch.int32)), "the two paths differ in bytes"
                assert torch.equal(s["bits"], amd.bitpack(s["y_old"])), "the bit output differs from LceQuantize of the float path"
            order = [sets[j % args.sets] for j in range(args.per_graph)]
            graphs = [graph_of(torch, [lambda s=s, f=f: f(s) for s in order]) for f in (new_value, new_bits, old)]
            rows = []
            for r in range(args.repeats):
                figures = [timed(torch, g, args.per_graph, args.window_ms) for g in graphs]
                rows.append(figures)
                print("  %-22s %-6d %10.2f %10.2f %10.2f   x%.2f" % ("%d x %d -> %d" % (batch, k, n), r, *figures, figures[2] / figures[0]))
            med = [float(np.median([row[c] for row in rows])) for c in range(3)]
            spread = max(max(row[c] for row in rows) - min(row[c] for row in rows) for c in range(3))
            gain = min(row[2] for row in rows) - max(row[0] for row in rows)
            summary.append((batch, k, n, med, spread, gain))
            del graphs
    print("# summary: medians; spread = the largest max - min of a column over the repeats; faster = min old - max new_value > spread")
    print("# algorithmic bytes of the new entry (value output): bit operands + scale + bias + float output; roofline = the larger of")
    print("#   bytes / 6.29 TB/s (HBM, measured copy rate) and MACs / 4.2e15 MAC/s (FP4 matrix cores, measured); the new entry's bit")
    print("#   weights were cached on the die in this run, so a `bytes` row's bound is the one a cold layer would have, not this run's")
    print("# %-22s %9s %9s %9s %8s %8s  %-7s %11s %9s %9s  %s" % ("layer", "new_value", "new_bits", "old", "old/new", "spread", "faster", "bytes", "hbm_us", "mfma_us", "binds"))
    for batch, k, n, med, spread, gain in summary:
        kw = (k + 31) // 32
        nbytes = 4 * (batch * kw + n * kw + 2 * n + batch * n)
        macs = batch * n * k
        hbm_us, mfma_us = nbytes / HBM_BYTES_PER_S * 1e6, macs / FP4_MAC_PER_S * 1e6
        print("  %-22s %9.2f %9.2f %9.2f %8.2f %8.2f  %-7s %11d %9.3f %9.3f  %s"
              % ("%d x %d -> %d" % (batch, k, n), med[0], med[1], med[2], med[2] / med[0], spread, "yes" if gain > spread else "NO",
                 nbytes, hbm_us, mfma_us, "bytes" if hbm_us >= mfma_us else "MFMA"))


if __name__ == "__main__":
    main()
