#!/usr/bin/env python
"""The planner's whole answer as text, HOST-only: for a fixed grid of (descriptor, weight seed, sequence of option strings) one plan
is built, every option string is applied as lce_hip_bconv2d_plan_set_option applies it (what it makes stale is dropped), select_kernel
runs after each step, and the step is printed as one line -- error string, kernel name, est_us (%a), every scalar field of HostPlan,
length and hash of every table, a hash of the selected engine's launch constants (tests/hostsim/hostsim.cpp, hostsim_plan_step).

A change that must not move a plan (a refactor of csrc/lce_plan*.cpp) is checked by running this from both trees and comparing:
    python tools/plan_dump.py | sha256sum
    LCE_PLAN_DEBUG=2 python tools/plan_dump.py --auto 2>&1 >/dev/null | sha256sum      (the auto rows' [lce plan] lines)
usage: plan_dump.py [--auto] [--count]       --auto: the auto-rule rows only; --count: print the number of lines only"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as H  # noqa: E402
import launch_geometry as L  # noqa: E402  (the ctypes plumbing of hostsim_plan_new / _step / _free, shared with the tests)

F32, I8, BP = 0, 1, 2
SAME, VALID = 0, 1
DST_NAME = {F32: "f32", I8: "i8", BP: "bp"}
# tests/test_planner_choice.py: (hw, cin, cout, stride)
LAYERS = [(56, 64, 64, 1), (28, 128, 128, 1), (14, 256, 256, 1), (7, 512, 512, 1), (56, 256, 256, 1),
          (56, 64, 128, 2), (28, 128, 256, 2), (14, 256, 512, 2), (7, 512, 512, 2)]


def desc(batch, h, w, cin, k, cout, dst, stride=1, groups=1, dilation=1, padding=SAME, pad_values=1, activation=0, semantics=1,
         out_scale=0.125, out_zero_point=3):
    return H.Desc(batch, h, w, cin, k, k, cout, groups, stride, stride, dilation, dilation, padding, pad_values, activation, dst,
                  semantics, float(out_scale), int(out_zero_point))


def describe(d):
    return "b%d %dx%dx%d k%d -> %d s%d g%d d%d pad%d/%d act%d sem%d %s" % (
        d.batch, d.in_height, d.in_width, d.channels_in, d.filter_height, d.channels_out, d.stride_height, d.groups, d.dilation_height,
        d.padding, d.pad_values, d.activation, d.semantics, DST_NAME[d.dst_type])


weights = L.seeded_weights


def grid(auto_only):
    """[(tag, descriptor, weight seed or None, [(option string, max_batch), ...])]"""
    cases = []

    def one(tag, d, seed, *steps):
        cases.append((tag, d, seed, [s if isinstance(s, tuple) else (s, 0) for s in steps]))

    # the auto rule on the rows of tests/test_planner_choice.py, without weights (as that test makes its plans) and with
    for hw, cin, cout, s in LAYERS:
        for b in (1, 16, 64, 256):
            for dst in (F32, I8, BP):
                one("auto", desc(b, hw, hw, cin, 3, cout, dst, stride=s), None, "")
                one("auto+w", desc(b, hw, hw, cin, 3, cout, dst, stride=s), 1, "")
    if auto_only:
        return cases
    forced = ["engine=valu", "engine=mfma", "engine=direct", "engine=pointwise", "engine=stream", "engine=wstream", "kernel=tiled",
              "kernel=general", "tile=1x16", "tile=2x32", "engine=mfma;tile=128x128", "engine=direct;tile=256x64", "engine=mfma;tile=256x256",
              "engine=valu;kernel=tiled;tile=4x16", "engine=direct;tile2d=on", "engine=direct;tile2d=off"]
    for hw, cin, cout, s in LAYERS:
        for b in (1, 64):
            for dst in (F32, I8, BP):
                for f in forced:
                    one("forced", desc(b, hw, hw, cin, 3, cout, dst, stride=s), 2, f)
                for cu in (4, 256):
                    one("cus", desc(b, hw, hw, cin, 3, cout, dst, stride=s), 2, "compute_units=%d" % cu)
                    one("cus", desc(b, hw, hw, cin, 3, cout, dst, stride=s), 2, "engine=stream;compute_units=%d" % cu)
    stream_opts = ["stream_rows=7", "stream_rows=5", "stream_rows=2", "stream_interleave=0", "stream_interleave=1", "stream_interleave=auto",
                   "stream_blocks_per_cu=1", "stream_blocks_per_cu=2", "stream_rows=7;stream_interleave=1", "stream_rows=14;stream_interleave=1",
                   "stream_interleave=1;stream_blocks_per_cu=2", "stream_flat=0", "stream_pixel_phases=2", "stream_pixel_phases=4",
                   "stream_rows=7;stream_blocks_per_cu=2;compute_units=4", "stream_interleave=1;compute_units=4"]
    for hw, cin, cout, s in [(56, 64, 64, 1), (28, 128, 128, 1), (14, 256, 256, 1), (7, 512, 512, 1), (56, 64, 128, 2), (28, 64, 96, 1)]:
        for b in (1, 6, 64):
            for dst in (F32, I8, BP):
                for o in stream_opts:
                    one("stream", desc(b, hw, hw, cin, 3, cout, dst, stride=s), 3, "engine=stream;" + o)
                    one("stream/auto", desc(b, hw, hw, cin, 3, cout, dst, stride=s), 3, o)
    for b in (1, 4):
        for dst in (F32, I8, BP):
            for o in ("", "stream_strip=32", "stream_strip=64", "stream_strip=0", "stream_strip=-1", "stream_strip=48", "stream_strip=96"):
                one("strip", desc(b, 224, 224, 256, 3, 64, dst), 3, "engine=stream;" + o)
                one("strip", desc(b, 12, 64, 256, 3, 64, dst), 3, "engine=stream;" + o)
                one("strip", desc(b, 224, 224, 128, 3, 64, dst), 3, "engine=stream;" + o)
            one("strip/auto", desc(b, 224, 224, 256, 3, 64, dst), 3, "")
    for o in ("wstream_blocks=2", "wstream_images=1", "wstream_images=3;wstream_blocks=1", "wstream_images=100"):
        for dst in (F32, I8, BP):
            one("wstream", desc(8, 14, 14, 256, 3, 256, dst), 3, "engine=wstream;" + o)
    # 1x1 layers
    for cin in (64, 192, 512, 96, 320):
        for s in (1, 2):
            for b in (1, 64, 256):
                for dst in (F32, I8, BP):
                    for o in ("", "engine=pointwise", "engine=mfma", "engine=valu", "pointwise_channels=32", "pointwise_channels=128",
                              "engine=pointwise;pointwise_channels=64"):
                        one("1x1", desc(b, 28, 28, cin, 1, 128, dst, stride=s), 4, o)
    one("1x1", desc(256, 56, 56, 256, 1, 256, F32), 4, "")
    one("1x1", desc(64, 28, 28, 128, 1, 48, F32), 4, "")
    # grouped, dilated, what the matrix cores refuse, deep, odd ends
    others = [desc(16, 28, 28, 128, 3, 128, F32, groups=2), desc(16, 28, 28, 256, 3, 256, I8, groups=2), desc(16, 28, 28, 128, 3, 128, BP, groups=4),
              desc(16, 28, 28, 128, 3, 64, F32, groups=2), desc(64, 28, 28, 128, 3, 128, F32, dilation=2), desc(64, 28, 28, 128, 3, 128, BP, dilation=2),
              desc(64, 14, 14, 1024, 3, 256, F32), desc(4, 7, 7, 1024, 3, 1024, I8), desc(64, 14, 14, 640, 3, 128, BP), desc(1, 7, 7, 2048, 1, 512, F32),
              desc(64, 28, 28, 32, 3, 64, F32), desc(64, 28, 28, 100, 3, 100, F32), desc(64, 28, 28, 130, 3, 96, I8), desc(8, 28, 28, 64, 5, 64, F32),
              desc(64, 28, 28, 128, 3, 128, F32, padding=VALID), desc(64, 28, 28, 128, 3, 128, F32, pad_values=0),
              desc(64, 28, 28, 128, 3, 128, F32, pad_values=0, semantics=0), desc(64, 28, 28, 128, 3, 128, I8, activation=1),
              desc(64, 28, 28, 128, 3, 128, F32, activation=3), desc(2, 28, 28, 64, 3, 30, F32), desc(2, 28, 28, 64, 3, 40, I8),
              desc(1, 112, 112, 64, 3, 64, F32), desc(16, 16, 96, 64, 3, 64, F32), desc(256, 7, 7, 512, 3, 128, F32), desc(5, 7, 7, 512, 3, 128, BP),
              desc(0, 14, 14, 256, 3, 256, F32), desc(64, 28, 28, 128, 3, 128, I8, out_zero_point=-128)]
    for d in others:
        for o in ("", "engine=valu", "engine=mfma", "engine=direct", "engine=stream", "engine=wstream", "engine=pointwise", "kernel=tiled",
                  "kernel=general", "tile=2x16", "engine=mfma;tile=128x256", "compute_units=4"):
            one("other", d, 5, o)
    # re-selection on ONE plan: the repack conditions and what a selection leaves behind
    L28 = lambda dst, b=64: desc(b, 28, 28, 128, 3, 128, dst)
    L14 = lambda dst, b=64: desc(b, 14, 14, 256, 3, 256, dst)
    L56 = lambda dst, b=64: desc(b, 56, 56, 64, 3, 64, dst)
    L7 = lambda dst, b=64: desc(b, 7, 7, 512, 3, 512, dst)
    tour = ["", "engine=mfma", "engine=stream", "engine=wstream", "engine=auto"]
    for dst in (F32, I8, BP):
        for mk in (L28, L14, L56, L7):
            one("reselect tour", mk(dst), 6, *tour)
        one("reselect engines", L14(dst), 6, "engine=wstream", "engine=stream", "engine=direct", "engine=valu", "engine=mfma", "engine=pointwise",
            "engine=auto", "kernel=general", "kernel=tiled", "kernel=auto")
        one("reselect cus", L28(dst), 6, "", "compute_units=4", "compute_units=64", "engine=stream", "compute_units=304", "engine=auto")
        one("reselect batch", L14(dst, 256), 6, ("", 1), ("", 16), ("", 0), ("", 3), ("engine=stream", 5), ("engine=wstream", 2), ("engine=auto", 64))
        one("reselect stream options", L56(dst), 6, "engine=stream", "stream_rows=7", "stream_interleave=1", "stream_blocks_per_cu=2",
            "stream_rows=5", "stream_rows=0", "stream_blocks_per_cu=auto", "stream_interleave=auto", "engine=auto")
        one("reselect tiles", L28(dst), 6, "engine=valu", "tile=2x32", "tile=1x16", "tile=auto", "engine=mfma;tile=128x128", "tile=256x64", "tile=auto",
            "engine=auto")
        one("reselect refusals", L28(dst), 6, "", "engine=pointwise", "engine=wstream", "stream_rows=5;engine=stream", "engine=auto", "stream_rows=0",
            "engine=bogus", "tile=3x3", "")
        one("reselect 1x1", desc(64, 28, 28, 192, 1, 128, dst), 6, "", "engine=mfma", "engine=pointwise", "pointwise_channels=32", "engine=auto",
            ("", 1), "engine=valu", "engine=auto")
        one("reselect no weights", L14(dst), None, *tour)
    one("reselect int8 rounding", L14(I8), 6, "", "int8_rounding=exact", "int8_rounding=auto", "engine=stream", "int8_rounding=exact", "engine=wstream",
        "int8_rounding=auto", "engine=mfma", "engine=auto")
    one("reselect int8 rounding", L28(I8), 7, "engine=stream", "int8_rounding=exact", "engine=auto", "int8_rounding=auto")
    one("reselect int8 ties", L14(I8), -8, *tour)
    one("reselect int8 ties", L28(I8), -8, "", "engine=stream", "int8_rounding=exact", "engine=mfma", "int8_rounding=auto", "engine=auto")
    one("reselect int8 1x1", desc(64, 28, 28, 128, 1, 128, I8), 7, "", "int8_rounding=exact", "engine=mfma", "int8_rounding=auto", "engine=auto")
    one("reselect strips", desc(2, 224, 224, 256, 3, 64, F32), 6, "engine=stream", "stream_strip=32", "stream_strip=0", "stream_strip=-1", "engine=auto")
    one("reselect grouped", desc(16, 28, 28, 128, 3, 128, F32, groups=2), 6, "", "engine=mfma", "engine=direct", "engine=valu", "engine=stream", "engine=auto")
    return cases


def main():
    lines = 0
    for tag, d, seed, steps in grid("--auto" in sys.argv):
        for i, ((opts, max_batch), out) in enumerate(zip(steps, L.plan_lines(d, seed, steps))):
            lines += 1
            if out is None:
                print("%s | %s | seed %s | refused: %s" % (tag, describe(d), seed, L.planner_lib().hostsim_last_error().decode()))
                break
            if "--count" not in sys.argv:
                print("%s | %s | seed %s | step %d '%s' max_batch %d | %s" % (tag, describe(d), seed, i, opts, max_batch, out))
    if "--count" in sys.argv:
        print(lines)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
