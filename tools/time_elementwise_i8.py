#!/usr/bin/env python3
"""Where should the table of the int8 elementwise chain live, and what does the tail cost on top of the residual ADD?  The chain
of an int8 ReActNet block -- head ADD, ADD per-channel shift, PRELU, ADD per-channel shift, int8 out and bits -- at batch 256 on
56x56x64, 28x28x128, 14x14x256 and 7x7x512, in ONE process:

    lce_hip_elementwise_i8 forced onto the LDS path and onto the global path, and as the entry chooses (the same bytes, checked
      here first);
    the same chain with scalar operands on the one-row path (another table, so other bytes: a figure of its own, no competitor);
    lce_hip_add_int8 alone on the same tensors with the head's parameters -- it moves the same bytes, so it is the yardstick for
      what the tail costs.  (Its kernels, lce_tu_eltwise_i8.hip, are the ones that were there before the chain existed.)

    python tools/time_elementwise_i8.py [--repeats 5] > profiles/elementwise_i8/chains.txt

Method: every candidate is recorded ONCE into a HIP graph of K launches, launch k on operand set k (input, addend, output, bits);
K is chosen so that the sets together exceed twice the 256 MiB Infinity Cache, so no launch finds its operands there.  A figure is
microseconds per launch from events around enough replays of the graph for some 400 launches, after a warm-up replay.  The
candidates ALTERNATE inside each repeat, and the spread between repeats (max - min) stands next to the medians.  The condition:
at each shape the default path is the fastest forced path, or within the spread of it."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
amd = importlib.import_module("compute-engine_amd")
import elementwise_i8_ref as E  # noqa: E402

BATCH = 256
SHAPES = ((56, 64), (28, 128), (14, 256), (7, 512))                # (height = width, channels)
INFINITY_CACHE = 256 << 20
PATHS = {"lds": amd.EW_I8_PATH_LDS, "global": amd.EW_I8_PATH_GLOBAL, "default": None}
NAMES = ("lds", "global", "default", "one_row*", "add_int8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=400, help="launches per timed figure, about")
    ap.add_argument("--batch", type=int, default=BATCH)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    print("# batch %d; head ADD + ADD shift + PRELU + ADD shift, int8 out and bits; us per launch, graph replays over K operand sets "
          "(> 2 x 256 MiB together), %d repeats, candidates alternating" % (args.batch, args.repeats))
    print("# one_row*: the same chain with scalar operands (R = 1); add_int8: the bare residual ADD on the same tensors")
    print("# %-12s %-3s %-6s %s" % ("shape", "K", "repeat", "  ".join("%9s" % n for n in NAMES)))
    verdicts = []
    for hw, c in SHAPES:
        g = np.random.default_rng(hw)
        # a block's tail at the scales such a network has; activations drawn round the zero point (sigma 30), not uniform: what the
        # table is asked for decides the LDS bank conflicts
        q_in, head = (0.05, -3), ((0.06, 4), (0.08, -2), amd.ACT_NONE)
        steps = [("add", g.integers(-128, 128, c).astype(np.int8), (0.02, 0), (0.08, 1), amd.ACT_NONE),
                 ("prelu", g.integers(-128, 128, c).astype(np.int8), (0.008, 0), (0.06, -5)),
                 ("add", g.integers(-128, 128, c).astype(np.int8), (0.02, 0), (0.06, 3), amd.ACT_NONE)]
        scalar_steps = [st[:1] + (np.int8(st[1][0]),) + st[2:] for st in steps]
        rows = args.batch * hw * hw
        set_bytes = rows * c * 3 + rows * ((c + 31) // 32) * 4
        K = 2 * INFINITY_CACHE // set_bytes + 2
        draw = lambda: torch.randn((rows, c), device=dev).mul_(30.0).round_().clamp_(-128, 127).to(torch.int8)
        sets = [(draw(), draw(), torch.empty((rows, c), dtype=torch.int8, device=dev),
                 torch.empty((rows, (c + 31) // 32), dtype=torch.int32, device=dev)) for _ in range(K)]
        table = torch.from_numpy(amd.elementwise_i8_prepare(c, q_in, steps, head=head)).to(dev)
        table1 = torch.from_numpy(amd.elementwise_i8_prepare(c, q_in, scalar_steps, head=head)).to(dev)

        def chain(path, st=steps, tb=table):
            return lambda x, a, o, b: amd.elementwise_i8(x, tb, q_in, st, addend=a, head=head, out=o, out_bits=b, path=path)
        fns = [chain(PATHS["lds"]), chain(PATHS["global"]), chain(None), chain(amd.EW_I8_PATH_ONE_ROW, scalar_steps, table1),
               lambda x, a, o, b: amd.add_int8(x, a, q_in, head[0], head[1], head[2], out=o, out_bits=b)]
        # the same bytes from the three places of the table, and the NumPy chain's on a slice
        x, a, o, b = sets[0]
        results = []
        for fn in fns[:3]:
            o.zero_(), b.zero_()
            fn(x, a, o, b)
            torch.cuda.synchronize()
            results.append((o.clone(), b.clone()))
        assert all(torch.equal(results[0][0], r[0]) and torch.equal(results[0][1], r[1]) for r in results[1:]), "the paths differ in bytes"
        want = E.chain(x[:4096].cpu().numpy(), q_in, steps, a[:4096].cpu().numpy(), head)
        assert np.array_equal(results[0][0][:4096].cpu().numpy(), want[0]) and np.array_equal(results[0][1][:4096].cpu().numpy(), want[1])
        assert len(torch.unique(results[0][0])) > 50, "a degenerate output"
        launch = amd.elementwise_i8(x, table, q_in, steps, addend=a, head=head, out=o, out_bits=b, report_launch=True)[2]
        # one graph per candidate: K launches, one per operand set
        s = torch.cuda.Stream()
        graphs = []
        with torch.cuda.stream(s):
            for fn in fns:
                for t in sets:                                       # eager first: code objects loaded, attributes set
                    fn(*t)
                s.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=s):
                    for t in sets:
                        fn(*t)
                graphs.append(gr)
        replays = max(2, -(-args.launches // K))

        def figure(gr):
            with torch.cuda.stream(s):
                gr.replay()                                          # warm-up: clocks and code
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(replays):
                    gr.replay()
                e1.record(s)
                s.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (replays * K)
        table_rows = []
        for r in range(args.repeats):
            figures = [figure(gr) for gr in graphs]                  # alternating: each candidate once per repeat
            table_rows.append(figures)
            print("  %-12s %-3d %-6d %s" % ("%dx%dx%d" % (hw, hw, c), K, r, "  ".join("%9.2f" % v for v in figures)))
        cols = list(zip(*table_rows))
        med = [float(np.median(col)) for col in cols]
        spread = max(max(col) - min(col) for col in cols[:3])
        verdicts.append((hw, c, med, spread, launch, set_bytes))
        del sets, graphs, results
        torch.cuda.empty_cache()
    print("# verdict: medians; spread = the largest max - min between repeats among lds / global / default")
    ok = True
    for hw, c, med, spread, launch, set_bytes in verdicts:
        best = min(med[0], med[1])
        good = med[2] <= best + spread
        ok = ok and good
        print("#   %dx%dx%d: lds %.2f us, global %.2f us, default %.2f us (path %d, %d blocks x %d waves, %d B of LDS), spread %.2f us: %s; "
              "one_row* %.2f us; add_int8 %.2f us: the chain takes x%.2f of the bare ADD; %.1f MB moved: %.2f us at 6.29 TB/s"
              % (hw, hw, c, med[0], med[1], med[2], launch["path"], launch["blocks"], launch["waves_per_block"], launch["lds_bytes"], spread,
                 "the default is the fastest forced path or within the spread of it" if good else "the default is NOT the fastest path",
                 med[3], med[4], med[2] / med[4], set_bytes / 1e6, set_bytes / 6.29e6))
    print("# the selection rule %s" % ("holds at every shape" if ok else "does NOT hold at every shape"))


if __name__ == "__main__":
    main()
