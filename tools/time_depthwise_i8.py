#!/usr/bin/env python3
"""Does the 16-byte path of the int8 depthwise convolution earn its place, and where does the kernel stand?  At batch 256,
3x3 / 2 SAME, on QuickNet's three transitions and a stem-sized map, in ONE process, the candidates alternating, three times over, so
that the spread between repeats is on the page next to the differences:

    lce_hip_depthwise_conv2d_i8 on its 16-byte path and forced onto its row path (the same bytes, checked here first);
    lce_hip_pool2d int8 MAX at the same shape (the same bytes moved, a kernel that was there before);
    lce_hip_depthwise_conv2d_f32 at the same shape (four times the bytes);
    the byte bound: input + output bytes at the 8.0 TB/s of the data sheet and at the 6.29 TB/s a copy reaches.

    python tools/time_depthwise_i8.py [--launches 100] [--repeats 3] > profiles/depthwise_i8/depthwise_i8.txt

The method is tools/time_head.py's: each figure is microseconds per launch from HIP events around `--launches` back-to-back
launches, after a 40 ms clock spin-up.  The keep / drop rule for the 16-byte path: it stays only if at every shape its slowest
repeat beats the row path's fastest by more than the largest spread between repeats.  Last, the whole int8 network fixture of
tests/depthwise_i8_models.py (c) at batch 256: ONE section against the same file cut at its depthwise operators with NumPy running
what lies between (wall clock, the median of the repeats)."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
amd = importlib.import_module("compute-engine_amd")
mr = importlib.import_module("compute-engine_amd.model_runner")
from time_head import event_us, spin_up  # noqa: E402

BATCH = 256
SHAPES = ((56, 64), (28, 128), (14, 256), (112, 32))               # (height = width, channels)
NAMES = ("i8_vec", "i8_rows", "pool_i8_max", "f32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100, help="launches per timed run")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--no-network", action="store_true", help="skip the fixture (c) comparison")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lib = amd.lib()
    g = np.random.default_rng(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cur = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q_in, q_out = (0.06, -20), (0.06, -18)
    print("# batch %d, 3x3 / 2 SAME; us per launch from events around %d launches; byte bound: (input + output bytes) / 8.0 TB/s and / 6.29 TB/s"
          % (args.batch, args.launches))
    print("# %-16s %-6s %s" % ("shape", "repeat", "  ".join("%11s" % n for n in NAMES)))
    verdict = []
    for hw, c in SHAPES:
        b = args.batch
        oh = (hw + 1) // 2
        x = torch.randint(-128, 128, (b, hw, hw, c), dtype=torch.int8, device=dev)
        blur = np.ascontiguousarray(np.broadcast_to(np.array([[32, 64, 32], [64, 127, 64], [32, 64, 32]], np.int8)[None, :, :, None], (1, 3, 3, c)))
        table_h, _, _ = amd.depthwise_conv2d_i8_prepare(blur, None, 0.25 / 127, q_in, q_out)
        w, table = torch.from_numpy(blur).to(dev), torch.from_numpy(table_h).to(dev)
        y_vec = torch.empty((b, oh, oh, c), dtype=torch.int8, device=dev)
        y_rows, y_pool = torch.empty_like(y_vec), torch.empty_like(y_vec)
        xf = x.to(torch.float32)
        wf = torch.from_numpy(blur.astype(np.float32) / 511.0).to(dev)
        y_f = torch.empty((b, oh, oh, c), dtype=torch.float32, device=dev)
        d8 = amd.DepthwiseI8Desc(b, hw, hw, c, 1, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE, q_in[0], q_in[1], q_out[0], q_out[1])
        df = amd.DepthwiseDesc(b, hw, hw, c, 1, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE)
        dp = amd.Pool2dDesc(amd.POOL_MAX, amd.I8, b, hw, hw, c, 3, 3, 2, 2, amd.PADDING_SAME, amd.ACT_NONE, q_in[0], q_in[1])
        fns = (lambda: amd.check(lib.lce_hip_depthwise_conv2d_i8_forced(C.byref(d8), 1, ptr(x), ptr(w), ptr(table), ptr(y_vec), None, cur())),
               lambda: amd.check(lib.lce_hip_depthwise_conv2d_i8_forced(C.byref(d8), 0, ptr(x), ptr(w), ptr(table), ptr(y_rows), None, cur())),
               lambda: amd.check(lib.lce_hip_pool2d(C.byref(dp), ptr(x), ptr(y_pool), None, cur())),
               lambda: amd.check(lib.lce_hip_depthwise_conv2d_f32(C.byref(df), ptr(xf), ptr(wf), None, ptr(y_f), None, cur())))
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        assert torch.equal(y_vec, y_rows), "the two paths differ in bytes"
        assert len(torch.unique(y_vec)) > 100, "a degenerate output"
        took = C.c_int32(-1)
        amd.check(lib.lce_hip_depthwise_conv2d_i8_path(C.byref(d8), ptr(x), ptr(w), ptr(table), ptr(y_vec), None, C.byref(took)))
        assert took.value == 1, "the entry's own choice at this shape is the 16-byte path"
        rows = []
        for r in range(args.repeats):
            figures = []
            for fn in fns:                                           # alternating: each candidate once per repeat
                spin_up(torch, fn)
                figures.append(event_us(torch, fn, args.launches))
            rows.append(figures)
            print("  %-16s %-6d %s" % ("%dx%dx%d" % (hw, hw, c), r, "  ".join("%11.2f" % v for v in figures)))
        moved = b * (hw * hw + oh * oh) * c
        cols = list(zip(*rows))
        spread = max(max(col) - min(col) for col in cols[:2])
        verdict.append((hw, c, [float(np.median(col)) for col in cols], spread, min(cols[1]) - max(cols[0]), moved))
        del x, xf, y_vec, y_rows, y_pool, y_f
    print("# verdict: medians; spread = the largest max - min between repeats of the two int8 paths; gain = min rows - max vec")
    keep = True
    for hw, c, med, spread, gain, moved in verdict:
        keep = keep and gain > spread
        print("#   %dx%dx%d: vec %.2f us, rows %.2f us (x%.2f), pool int8 MAX %.2f us, f32 %.2f us (x%.2f of vec), spread %.2f us, gain %.2f us: %s; "
              "%.1f MB moved: bound %.2f us at 8.0 TB/s, %.2f us at 6.29 TB/s (vec reaches %.0f%% of the latter)"
              % (hw, hw, c, med[0], med[1], med[1] / med[0], med[2], med[3], med[3] / med[0], spread, gain,
                 "vec wins by more than the spread" if gain > spread else "NO clear win", moved / 1e6, moved / 8.0e6, moved / 6.29e6,
                 100.0 * (moved / 6.29e6) / med[0]))
    print("# the 16-byte path %s" % ("is kept: it wins at every shape by more than the spread" if keep else "does NOT clearly win at every shape"))
    if args.no_network:
        return
    # fixture (c): one section against the cut partition with the host operators between
    import depthwise_i8_models as DM
    data, xt, out, info = DM.network_fixture()
    xs = DM.fixture_input(info, args.batch, 3)
    one = mr.Interpreter(data, batch_size=args.batch, **DM.EVERY_FLAG)
    cut = mr.Interpreter(data, batch_size=args.batch, **DM.EARLIER)
    assert len(one.sections) == 1 and [s.ops for s in cut.sections] == info["parent_sections"]

    def run_one():
        return one.run_section(0, [xs])[0]

    def run_cut():
        model = cut.model
        section_of = {op: k for k, sec in enumerate(cut.sections) for op in sec.ops}
        live, ran = {model.inputs[0]: xs}, set()
        for i, op in enumerate(model.operators):
            if i in section_of:
                k = section_of[i]
                if k not in ran:
                    ran.add(k)
                    live.update(zip(cut.sections[k].outputs, cut.run_section(k, [live[t] for t in cut.sections[k].inputs])))
            else:
                live[op.outputs[0]] = info["host"][i](*[live[t] for t in op.inputs if t >= 0 and not model.tensors[t].constant])
        return live[out]
    a, bb = run_one(), run_cut()
    assert np.array_equal(np.asarray(a).reshape(-1).view(np.uint8), np.asarray(bb).reshape(-1).view(np.uint8)), "one section and the cut file differ"
    times = {"one section": [], "cut at the depthwise operators": []}
    for r in range(args.repeats):
        for name, fn in (("one section", run_one), ("cut at the depthwise operators", run_cut)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
    print("# fixture (c), the int8 network of tests/depthwise_i8_models.py, batch %d, host wall clock with the copies of run_section (ms):" % args.batch)
    for name, v in times.items():
        print("#   %-32s median %.2f ms (%s)" % (name, float(np.median(v)), ", ".join("%.2f" % t for t in v)))
    print("#   launches of the one section: depthwise_i8 %s, conv_i8 %s; the cut file runs its 6 host operators in NumPy"
          % (one.model.depthwise_i8_stats(), one.model.conv_i8_stats()))


if __name__ == "__main__":
    main()
