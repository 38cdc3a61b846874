#!/usr/bin/env python3
"""Does the int8 fully connected kernel of the classifier head earn its place?  lce_hip_fully_connected_i8 against
lce_hip_conv2d_i8 called on a [batch, 1, 1, K] image with a 1x1 filter -- the same bytes (checked here first) -- in ONE process,
one after the other, three times over, so that the spread between repeats is on the page next to the difference between the two.

    python tools/time_head_i8.py [--launches 200] [--repeats 3] > profiles/head_i8/fc_i8_vs_conv2d_i8.txt

The method is tools/time_head.py's: each figure is microseconds per launch from HIP events around `--launches` back-to-back
launches, after a 40 ms clock spin-up; `graph` is the same from a captured HIP graph of 20 launches.  Also timed, for the
DESIGN.md paragraph: lce_hip_mean_i8 on a 7x7x512 map, lce_hip_softmax_i8 on the head's logits, and the two boundary entries."""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
amd = importlib.import_module("compute-engine_amd")
from time_head import event_us, graph_us, spin_up  # noqa: E402

SHAPES = ((256, 512, 1000), (256, 1024, 1000), (1, 512, 1000), (1, 1024, 1000))     # (batch, K, N)
REQUIRED = SHAPES[:2]                                                               # the shapes the kernel must win at


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
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cur = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q_in, q_out = (0.05, -4), (0.04, 3)
    print("# us per launch; eager = events around %d launches, graph = the same from a captured graph of 20" % args.launches)
    print("# %-22s %-9s %s" % ("shape (batch x K -> N)", "repeat", "fc_eager  conv2d_i8_eager  fc_graph  conv2d_i8_graph"))
    verdict = []
    for batch, k, n in SHAPES:
        xh = g.integers(-128, 128, (batch, k), dtype=np.int64).astype(np.int8)
        wh = g.integers(-128, 128, (n, k), dtype=np.int64).astype(np.int8)
        bh = g.integers(-50000, 50000, n, dtype=np.int64).astype(np.int32)
        sw = (g.uniform(0.5, 2.0, n) * 60.0 / (74.0 * 74.0 * np.sqrt(k)) * q_out[0] / q_in[0]).astype(np.float32)
        table_h, _, _ = amd.fully_connected_i8_prepare(wh, bh, sw, q_in, q_out)
        table_c, _, _ = amd.conv2d_i8_prepare(wh.reshape(n, 1, 1, k), bh, sw, q_in, q_out)
        assert np.array_equal(table_h, table_c), "the two prepares differ"
        x, w, t = (torch.from_numpy(a).to(dev) for a in (xh, wh, table_h))
        y_fc = torch.empty((batch, n), dtype=torch.int8, device=dev)
        y_cv = torch.empty((batch, n), dtype=torch.int8, device=dev)
        fc_desc = amd.FcI8Desc(batch, k, n, amd.ACT_NONE, q_in[0], q_in[1], q_out[0], q_out[1])
        cv_desc = amd.Conv2dI8Desc(batch, 1, 1, k, n, 1, 1, 1, 1, amd.PADDING_VALID, amd.ACT_NONE, q_in[0], q_in[1], q_out[0], q_out[1])

        def fc():
            amd.check(lib.lce_hip_fully_connected_i8(C.byref(fc_desc), ptr(x), ptr(w), ptr(t), ptr(y_fc), cur()))

        def conv():
            amd.check(lib.lce_hip_conv2d_i8(C.byref(cv_desc), ptr(x), ptr(w), ptr(t), ptr(y_cv), None, cur()))
        fc()
        conv()
        torch.cuda.synchronize()
        assert torch.equal(y_fc, y_cv), "the two paths differ in bytes"
        assert len(torch.unique(y_fc)) > 100, "a degenerate output"
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
    print("# verdict (%s figures): median fc, median conv2d_i8, largest spread between repeats, worst-case gain = min conv2d_i8 - max fc" % verdict[0][3])
    for batch, k, n, _, mf, mc, spread, gain in verdict:
        print("#   %d x %d -> %d: fc %.2f us, conv2d_i8 %.2f us (x%.2f), spread %.2f us, gain %.2f us: %s%s"
              % (batch, k, n, mf, mc, mc / mf, spread, gain, "fc wins by more than the spread" if gain > spread else "NO clear win",
                 " (a required shape)" if (batch, k, n) in REQUIRED else ""))
    # the other entries of the head, for the record
    def timed(name, fn):
        spin_up(torch, fn)
        print("# %s: eager %.2f us, graph %s us" % (name, event_us(torch, fn, args.launches), "%.2f" % (graph_us(torch, fn, args.launches) or float("nan"))))
    for b in (256, 1):
        m_in = torch.from_numpy(g.integers(-128, 128, (b, 7, 7, 512), dtype=np.int64).astype(np.int8)).to(dev)
        m_out = torch.empty((b, 512), dtype=torch.int8, device=dev)
        md = amd.MeanI8Desc(b, 7, 7, 512, 0.05, -4, 0.021, 3)
        timed("mean_i8 %d x 7 x 7 x 512" % b, lambda: amd.check(lib.lce_hip_mean_i8(C.byref(md), ptr(m_in), ptr(m_out), cur())))
        z = torch.from_numpy(g.integers(-128, 128, (b, 1000), dtype=np.int64).astype(np.int8)).to(dev)
        p = torch.empty_like(z)
        timed("softmax_i8 %d x 1000" % b, lambda: amd.check(lib.lce_hip_softmax_i8(b, 1000, 0.05, 1.0, 1.0 / 256.0, -128, ptr(z), ptr(p), cur())))
        f = torch.empty((b, 1000), dtype=torch.float32, device=dev)
        timed("dequantize %d x 1000" % b, lambda: amd.check(lib.lce_hip_dequantize_i8_f32(b * 1000, 1.0 / 256.0, -128, ptr(p), ptr(f), cur())))
    img = torch.from_numpy(g.uniform(0, 5, (256, 224, 224, 3)).astype(np.float32)).to(dev)
    img_q = torch.empty(img.shape, dtype=torch.int8, device=dev)
    timed("quantize 256 x 224 x 224 x 3", lambda: amd.check(lib.lce_hip_quantize_f32_i8(img.numel(), 0.02, -128, ptr(img), ptr(img_q), cur())))


if __name__ == "__main__":
    main()
