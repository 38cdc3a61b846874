"""Launch geometry of the two streaming kernels (bconv2d_stream, bconv2d_wstream) at 512 .. 2048 images per GPU, scaled down.

What changes above 256 images on 256 CUs is a block's run, not the arithmetic: plan_stream_geometry sizes it as
ceil(batch * segments_per_image / CUs), and the plan option `compute_units` overrides the CU count.  So a launch of 2048 images on
256 CUs and one of 16 images on 2 CUs give a block the same work -- the same segments per block, ring, production schedule, pixel
blocks -- and the small one runs in milliseconds.

  plan_fields   the host planner's whole answer (tests/hostsim/hostsim.cpp, hostsim_plan_step) as {field: value}
  per_block     the fields of it that describe ONE block's work
  scale_down    the smallest (batch, compute_units) whose per_block equals a big launch's, and its uneven-run sibling
  LONG_RUN_CASES            what scale_down returns for the QuickNet layers at 512 / 1024 / 2048 images, as a literal table: the GPU
                            tests need neither the host simulation nor a compiler (tests/test_launch_geometry_host.py regenerates it)
  forced_geometry_cases     seeded draws of forced geometry options, the same list on every machine

tools/plan_dump.py prints its lines through plan_lines / seeded_weights of this file."""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple, Optional

import numpy as np

import hostsim_lib as H
import oracle_lib as O
import synth

DST_OF = {"f32": O.DST_F32, "i8": O.DST_I8, "bp": O.DST_BITPACKED}
DST_NAMES = ("f32", "i8", "bp")

# (h = w, cin, cout, stride): QuickNet's 3x3 layers and the stride-2 layers of the same maps (tests/test_planner_choice.py)
LAYERS = [(56, 64, 64, 1), (28, 128, 128, 1), (14, 256, 256, 1), (7, 512, 512, 1), (56, 64, 128, 2), (28, 128, 256, 2), (14, 256, 512, 2)]
BIG_BATCHES = (512, 1024, 2048)
ENGINES = ("auto", "stream", "wstream")
BIG_CUS = 256
# Two launches that no (layer, output type, 512 / 1024 / 2048, engine) cell reaches on this planner, added to the table so that the
# kernels' longest runs of these kinds are in it: (layer, output type, big batch, engine, further options of the big plan)
#  * flat runs (pixel blocks cut across whole 7x7 images) are the planner's choice up to 256 images per GPU only -- 4 images per
#    block; the ring of an 8-image flat run does not fit LDS, so from 512 on engine=stream takes one-row segments;
#  * two resident blocks per CU (bitpacked output, 64-channel bank) come with whole-image segments at 512 (1 per block) and 1024
#    (2 per block) and not at 2048 (two rings of 4 images do not fit): 4 segments per block need the 14-row segments that the
#    estimate prices 1 % behind (32.5 us against 32.1 us at 512 images).
EXTRA_CELLS = [((7, 512, 512, 1), "f32", 256, "stream", ""),
               ((56, 64, 64, 1), "bp", 512, "stream", "stream_rows=14;stream_interleave=1;stream_blocks_per_cu=2")]

_planner = None


def planner_lib() -> C.CDLL:
    """tests/hostsim/liblce_hostsim.so with the prototypes of hostsim_plan_new / _step / _free set."""
    global _planner
    if _planner is None:
        lib = H.lib()
        lib.hostsim_plan_new.restype = C.c_void_p
        lib.hostsim_plan_step.restype = C.c_char_p
        lib.hostsim_plan_step.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lib.hostsim_plan_free.argtypes = [C.c_void_p]
        lib.hostsim_plan_launch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
        _planner = lib
    return _planner


def seeded_weights(d: H.Desc, seed: int):
    """Seeded operands of the layer: filter words, multiplier, bias, thresholds.  seed < 0: the ties-everywhere int8 parameters
    (multiplier 0.25, integer biases) that no neighbouring pair rescues."""
    g = np.random.Generator(np.random.PCG64(abs(seed)))
    n, taps, cwg = d.channels_out, d.filter_height * d.filter_width, (d.channels_in // d.groups + 31) // 32
    filt = g.integers(-2 ** 31, 2 ** 31, size=(n, taps, cwg), dtype=np.int64).astype(np.int32)
    k = taps * (d.channels_in // d.groups)
    if seed < 0:
        mul = np.full(n, 0.25, np.float32)
        bias = g.integers(-4, 5, size=n).astype(np.float32)
    else:
        mul = g.uniform(0.5, 1.5, n).astype(np.float32) / np.float32(np.sqrt(k))
        bias = g.standard_normal(n).astype(np.float32)
    thr = g.integers(0, k + 1, size=n, dtype=np.int64).astype(np.int32)
    return [np.ascontiguousarray(a) for a in (filt, mul, bias, thr)]


def plan_lines(d: H.Desc, weights_seed, steps):
    """One host plan of descriptor `d` (weights_seed None: a plan without weights), re-selected once per (option string, max_batch)
    of `steps`: yields hostsim_plan_step's line of every step.  A descriptor the planner refuses yields one None."""
    lib = planner_lib()
    w = [None] * 4 if weights_seed is None else seeded_weights(d, weights_seed)
    plan = lib.hostsim_plan_new(C.byref(d), *[None if a is None else a.ctypes.data_as(C.c_void_p) for a in w])
    if not plan:
        yield None
        return
    try:
        for opts, max_batch in steps:
            yield lib.hostsim_plan_step(plan, opts.encode(), max_batch).decode()
    finally:
        lib.hostsim_plan_free(plan)


_HEAD = re.compile(r'err="(.*)" kernel="([^"]*)" (.*)$')


def parse_line(line: str) -> dict:
    """err and kernel as strings, est_us as a float, tables ("count:hash") and args (hex) as strings, every other field an int."""
    m = _HEAD.match(line)
    assert m, line
    fields = {"err": m.group(1), "kernel": m.group(2)}
    for item in m.group(3).split(" "):
        k, v = item.split("=", 1)
        if k == "est_us":
            fields[k] = float.fromhex(v)
        elif ":" in v or k == "args":
            fields[k] = v
        else:
            fields[k] = int(v)
    return fields


def option_string(options) -> str:
    if isinstance(options, str):
        return options
    return H.option_string(options or {}).decode()


def option_dict(options) -> dict:
    if isinstance(options, dict):
        return dict(options)
    return dict(item.split("=", 1) for item in options.split(";") if item)


def plan_fields(spec: O.ConvSpec, dst: int, options, max_batch: int = 0, weights_seed=None) -> dict:
    """The host planner's answer for `spec` with output type `dst` under `options` ("key=value;..." or a dict), as a C-ABI plan
    without further options would be made (stream_interleave and the like on auto).  A refusal comes back in fields["err"]."""
    (line,) = plan_lines(H.make_desc(spec, dst, 0.125, 3), weights_seed, [(option_string(options), max_batch)])
    if line is None:
        return {"err": planner_lib().hostsim_last_error().decode(), "kernel": ""}
    return parse_line(line)


def launches(spec: O.ConvSpec, dst: int, options, batches):
    """The plan of `spec` under `options` launched on fewer images than planned: {batch: launch constants} as make_stream_args /
    make_ws_args build them (hostsim_plan_launch): grid x and, for the weight-stationary kernel, S, SPB, GSTR, G0M, flat; for the
    weight-streaming kernel groups, parts and images per group."""
    lib = planner_lib()
    d = H.make_desc(spec, dst, 0.125, 3)
    plan = lib.hostsim_plan_new(C.byref(d), None, None, None, None)
    assert plan, lib.hostsim_last_error().decode()
    try:
        fields = parse_line(lib.hostsim_plan_step(plan, option_string(options).encode(), 0).decode())
        assert fields["err"] == "", fields["err"]
        out = {}
        for batch in batches:
            raw = (C.c_int32 * 8)()
            assert lib.hostsim_plan_launch(plan, batch, raw) == 0
            v = list(raw)
            out[batch] = ({"family": "stream", "grid_x": v[1], "S": v[2], "SPB": v[3], "GSTR": v[4], "G0M": v[5], "flat": v[6]} if v[0] == 1 else
                          {"family": "wstream", "grid_x": v[1], "groups": v[2], "parts": v[3], "ipb": v[7]})
        return fields, out
    finally:
        lib.hostsim_plan_free(plan)


STREAM_FIELDS = ("st_rs", "st_spb", "st_rows", "st_pitch", "st_ring_bytes", "st_nq", "st_flat", "st_pph_log", "st_ny", "st_occ", "st_nstrip",
                 "st_wso", "st_srs", "st_pbs", "st_qg", "st_ipr")
WSTREAM_FIELDS = ("ws_ipb", "ws_parts", "ws_nb", "ws_ny", "ws_hp", "ws_wp", "ws_pitch", "ws_img_pitch", "ws_lds_images", "ws_occupancy")


def family(fields: dict) -> Optional[str]:
    """"stream" / "wstream" for the two streaming kernels, None for every other kernel and for a refusal."""
    if fields.get("err") or not fields.get("use_mfma"):
        return None
    return "wstream" if fields["use_wstream"] else "stream" if fields["use_stream"] else None


def per_block(fields: dict) -> Optional[dict]:
    """What one block of the launch does: everything of the plan but the number of blocks and where their runs start."""
    fam = family(fields)
    if fam == "stream":
        sub = {k: fields[k] for k in ("kernel",) + STREAM_FIELDS}
        sub["interleaved"] = fields["st_gstr"] > 1
        return sub
    if fam == "wstream":
        return {k: fields[k] for k in ("kernel",) + WSTREAM_FIELDS}
    return None


def full_runs(fields: dict) -> bool:
    """Every block of a launch of fields["chunk"] images has a whole run: no short last run, no image group with fewer images."""
    if family(fields) == "stream":
        return fields["chunk"] * fields["st_spi"] == fields["st_gx"] * fields["st_spb"]
    return fields["chunk"] % fields["ws_ipb"] == 0


def blocks_in_x(fields: dict) -> int:
    """The grid's x extent of a launch of fields["chunk"] images (make_stream_args / make_ws_args of a full launch)."""
    if family(fields) == "stream":
        return fields["st_gx"]
    return -(-fields["chunk"] // fields["ws_ipb"]) * fields["ws_parts"]


def layer_spec(batch, h, w, cin, cout, stride, padding=O.PADDING_SAME, pad_values=1) -> O.ConvSpec:
    return O.ConvSpec(batch, h, w, cin, 3, 3, cout, 1, stride, stride, 1, 1, padding, pad_values)


def forced_options(big: dict) -> dict:
    """The plan options that pin a small launch to the big plan's own choices (everything but compute_units)."""
    if family(big) == "stream":
        return {"engine": "stream", "stream_rows": big["st_rs"], "stream_interleave": int(big["st_gstr"] > 1),
                "stream_blocks_per_cu": big["st_occ"], "stream_flat": big["st_flat"]}
    return {"engine": "wstream", "wstream_images": big["ws_ipb"], "wstream_blocks": big["ws_blocks_pref"] or 4}


class ScaledDown(NamedTuple):
    batch: int
    options: str                    # "key=value;..." with compute_units last
    sibling: Optional[int]          # a batch one image smaller on the same compute_units (an uneven last run), or None
    per_block: dict


def big_options(engine: str, extra: str = "") -> str:
    return "engine=%s" % engine + (";" + extra if extra else "")


def scale_down(spec_big: O.ConvSpec, dst: int, engine: str, extra: str = "") -> Optional[ScaledDown]:
    """The launch with the fewest output pixels (batch 2 .. 64, compute_units 2 .. 16, at least 2 blocks in x) that gives a block
    the work the planner gives it for `spec_big` on 256 CUs under engine=`engine` (and the `extra` options): segment rows, interleave,
    blocks per CU, stream_flat, wstream_images / wstream_blocks are forced to the big plan's values, and per_block must come out
    equal; where the big launch's runs are all whole, so are the small one's.  `sibling` is the launch of one image fewer on the same
    compute_units where that keeps per_block: its last run is short (its last image group smaller).
    None where the big plan is not one of the two streaming kernels, or no such launch exists."""
    big = plan_fields(spec_big, dst, big_options(engine, extra) + ";compute_units=%d" % BIG_CUS)
    want = per_block(big)
    if want is None:
        return None
    forced = forced_options(big)

    def small(batch, cus):
        return plan_fields(spec_big.with_batch(batch), dst, {**forced, "compute_units": cus})

    for batch in range(2, 65):              # fewest pixels first: the first hit is the answer
        for cus in range(2, 17):
            f = small(batch, cus)
            if per_block(f) != want or blocks_in_x(f) < 2 or (full_runs(big) and not full_runs(f)):
                continue
            sib = small(batch - 1, cus) if batch > 2 else None
            ok = sib is not None and per_block(sib) == want and blocks_in_x(sib) >= 2 and not full_runs(sib)
            return ScaledDown(batch, option_string({**forced, "compute_units": cus}), batch - 1 if ok else None, want)
    return None


def cells():
    """[(layer, dst name, big batch, engine, extra options)]: the 7 x 3 x 3 cells under each of the three engines, then EXTRA_CELLS."""
    return [(layer, dst, big_batch, engine, "") for layer in LAYERS for dst in DST_NAMES for big_batch in BIG_BATCHES
            for engine in ENGINES] + list(EXTRA_CELLS)


def big_plan(cell) -> dict:
    (hw, cin, cout, stride), dst, big_batch, engine, extra = cell
    return plan_fields(layer_spec(big_batch, hw, hw, cin, cout, stride), DST_OF[dst],
                       big_options(engine, extra) + ";compute_units=%d" % BIG_CUS)


def _key(layer, dst, pb):
    return (layer, dst) + tuple(sorted(pb.items()))


def generate_long_run_cases():
    """LONG_RUN_CASES from the planner: scale_down over cells(), one entry per distinct (layer, output type, per_block) -- the first
    cell that reaches it stands for it --, then the uneven-run siblings."""
    cases, seen, siblings = [], set(), []
    for cell in cells():
        (hw, cin, cout, stride), dst, big_batch, engine, extra = cell
        pb = per_block(big_plan(cell))
        if pb is None or _key(cell[0], dst, pb) in seen:
            continue
        seen.add(_key(cell[0], dst, pb))
        sd = scale_down(layer_spec(big_batch, hw, hw, cin, cout, stride), DST_OF[dst], engine, extra)
        if sd is None:
            continue
        tail = (dst, sd.options, pb["kernel"], big_batch, big_options(engine, extra))
        cases.append((sd.batch, hw, hw, cin, cout, stride) + tail)
        if sd.sibling is not None:
            siblings.append((sd.sibling, hw, hw, cin, cout, stride) + tail)
    return cases + siblings


def case_id(case) -> str:
    batch, h, w, cin, cout, stride, dst, options, kernel, big_batch, big_opts = case
    return "%dx%dx%d-%d_s%d_%s_b%d_cu%s_for_%d_%s" % (h, w, cin, cout, stride, dst, batch, option_dict(options)["compute_units"], big_batch,
                                                      option_dict(big_opts)["engine"])


def case_spec(case) -> O.ConvSpec:
    batch, h, w, cin, cout, stride = case[:6]
    return layer_spec(batch, h, w, cin, cout, stride)


# (batch, h, w, cin, cout, stride, output type, plan options, kernel name, the big batch and the options on 256 CUs it stands for)
LONG_RUN_CASES = [
    (4, 56, 56, 64, 64, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=1;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x64,rows14,il>', 512, 'engine=stream'),
    (8, 56, 56, 64, 64, 1, 'f32', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x64,rows56>', 1024, 'engine=stream'),
    (16, 56, 56, 64, 64, 1, 'f32', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x64,rows56>', 2048, 'engine=stream'),
    (4, 56, 56, 64, 64, 1, 'i8', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x64,rows56>', 512, 'engine=auto'),
    (8, 56, 56, 64, 64, 1, 'i8', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x64,rows56>', 1024, 'engine=auto'),
    (16, 56, 56, 64, 64, 1, 'i8', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x64,rows56>', 2048, 'engine=auto'),
    (2, 56, 56, 64, 64, 1, 'bp', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=2;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x64,rows56,x2>', 512, 'engine=auto'),
    (6, 56, 56, 64, 64, 1, 'bp', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=2;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x64,rows56,x2>', 1024, 'engine=auto'),
    (16, 56, 56, 64, 64, 1, 'bp', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x64,rows56>', 2048, 'engine=auto'),
    (4, 28, 28, 128, 128, 1, 'f32', 'engine=stream;stream_rows=4;stream_interleave=1;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows4,il>', 512, 'engine=auto'),
    (2, 28, 28, 128, 128, 1, 'f32', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<f32,3x3x128,images1,blocks4>', 512, 'engine=wstream'),
    (8, 28, 28, 128, 128, 1, 'f32', 'engine=stream;stream_rows=4;stream_interleave=1;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows4,il>', 1024, 'engine=auto'),
    (16, 28, 28, 128, 128, 1, 'f32', 'engine=stream;stream_rows=4;stream_interleave=1;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows4,il>', 2048, 'engine=auto'),
    (4, 28, 28, 128, 128, 1, 'i8', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows28>', 512, 'engine=auto'),
    (2, 28, 28, 128, 128, 1, 'i8', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<i8,3x3x128,images1,blocks4>', 512, 'engine=wstream'),
    (8, 28, 28, 128, 128, 1, 'i8', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows28>', 1024, 'engine=auto'),
    (16, 28, 28, 128, 128, 1, 'i8', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows28>', 2048, 'engine=auto'),
    (4, 28, 28, 128, 128, 1, 'bp', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows28>', 512, 'engine=auto'),
    (2, 28, 28, 128, 128, 1, 'bp', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<bitpacked,3x3x128,images1,blocks4>', 512, 'engine=wstream'),
    (8, 28, 28, 128, 128, 1, 'bp', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows28>', 1024, 'engine=auto'),
    (16, 28, 28, 128, 128, 1, 'bp', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows28>', 2048, 'engine=auto'),
    (4, 14, 14, 256, 256, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x256,rows14>', 512, 'engine=auto'),
    (2, 14, 14, 256, 256, 1, 'f32', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<f32,3x3x256,images1,blocks4>', 512, 'engine=wstream'),
    (8, 14, 14, 256, 256, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x256,rows14>', 1024, 'engine=auto'),
    (16, 14, 14, 256, 256, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x256,rows14>', 2048, 'engine=auto'),
    (4, 14, 14, 256, 256, 1, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x256,rows14>', 512, 'engine=auto'),
    (2, 14, 14, 256, 256, 1, 'i8', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<i8,3x3x256,images1,blocks4>', 512, 'engine=wstream'),
    (8, 14, 14, 256, 256, 1, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x256,rows14>', 1024, 'engine=auto'),
    (16, 14, 14, 256, 256, 1, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x256,rows14>', 2048, 'engine=stream'),
    (4, 14, 14, 256, 256, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x256,rows14>', 512, 'engine=auto'),
    (2, 14, 14, 256, 256, 1, 'bp', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<bitpacked,3x3x256,images1,blocks4>', 512, 'engine=wstream'),
    (8, 14, 14, 256, 256, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x256,rows14>', 1024, 'engine=auto'),
    (16, 14, 14, 256, 256, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x256,rows14>', 2048, 'engine=auto'),
    (4, 7, 7, 512, 512, 1, 'f32', 'engine=wstream;wstream_images=2;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<f32,3x3x512,images2,blocks4>', 512, 'engine=auto'),
    (16, 7, 7, 512, 512, 1, 'f32', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<f32,3x3x512,rows1>', 512, 'engine=stream'),
    (32, 7, 7, 512, 512, 1, 'f32', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<f32,3x3x512,rows1>', 1024, 'engine=stream'),
    (64, 7, 7, 512, 512, 1, 'f32', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<f32,3x3x512,rows1>', 2048, 'engine=stream'),
    (4, 7, 7, 512, 512, 1, 'i8', 'engine=wstream;wstream_images=2;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<i8,3x3x512,images2,blocks4>', 512, 'engine=auto'),
    (16, 7, 7, 512, 512, 1, 'i8', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<i8,3x3x512,rows1>', 512, 'engine=stream'),
    (32, 7, 7, 512, 512, 1, 'i8', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<i8,3x3x512,rows1>', 1024, 'engine=stream'),
    (64, 7, 7, 512, 512, 1, 'i8', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<i8,3x3x512,rows1>', 2048, 'engine=stream'),
    (4, 7, 7, 512, 512, 1, 'bp', 'engine=wstream;wstream_images=2;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<bitpacked,3x3x512,images2,blocks4>', 512, 'engine=auto'),
    (16, 7, 7, 512, 512, 1, 'bp', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<bitpacked,3x3x512,rows1>', 512, 'engine=stream'),
    (32, 7, 7, 512, 512, 1, 'bp', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<bitpacked,3x3x512,rows1>', 1024, 'engine=stream'),
    (64, 7, 7, 512, 512, 1, 'bp', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=8', 'bconv2d_stream<bitpacked,3x3x512,rows1>', 2048, 'engine=stream'),
    (4, 28, 28, 128, 256, 2, 'f32', 'engine=stream;stream_rows=2;stream_interleave=1;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows2,il>', 512, 'engine=auto'),
    (2, 28, 28, 128, 256, 2, 'f32', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<f32,3x3x128,images1,blocks4>', 512, 'engine=wstream'),
    (8, 28, 28, 128, 256, 2, 'f32', 'engine=stream;stream_rows=2;stream_interleave=1;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows2,il>', 1024, 'engine=auto'),
    (16, 28, 28, 128, 256, 2, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows14>', 2048, 'engine=stream'),
    (4, 28, 28, 128, 256, 2, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows14>', 512, 'engine=auto'),
    (2, 28, 28, 128, 256, 2, 'i8', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<i8,3x3x128,images1,blocks4>', 512, 'engine=wstream'),
    (8, 28, 28, 128, 256, 2, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows14>', 1024, 'engine=auto'),
    (16, 28, 28, 128, 256, 2, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows14>', 2048, 'engine=auto'),
    (4, 28, 28, 128, 256, 2, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows14>', 512, 'engine=auto'),
    (2, 28, 28, 128, 256, 2, 'bp', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<bitpacked,3x3x128,images1,blocks4>', 512, 'engine=wstream'),
    (8, 28, 28, 128, 256, 2, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows14>', 1024, 'engine=auto'),
    (16, 28, 28, 128, 256, 2, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows14>', 2048, 'engine=auto'),
    (8, 14, 14, 256, 512, 2, 'f32', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<f32,3x3x256,rows1>', 512, 'engine=stream'),
    (2, 14, 14, 256, 512, 2, 'f32', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<f32,3x3x256,images1,blocks2>', 512, 'engine=wstream'),
    (16, 14, 14, 256, 512, 2, 'f32', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<f32,3x3x256,rows1>', 1024, 'engine=stream'),
    (32, 14, 14, 256, 512, 2, 'f32', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<f32,3x3x256,rows1>', 2048, 'engine=stream'),
    (2, 14, 14, 256, 512, 2, 'i8', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<i8,3x3x256,images1,blocks2>', 512, 'engine=auto'),
    (8, 14, 14, 256, 512, 2, 'i8', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<i8,3x3x256,rows1>', 512, 'engine=stream'),
    (16, 14, 14, 256, 512, 2, 'i8', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<i8,3x3x256,rows1>', 1024, 'engine=stream'),
    (32, 14, 14, 256, 512, 2, 'i8', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<i8,3x3x256,rows1>', 2048, 'engine=stream'),
    (8, 14, 14, 256, 512, 2, 'bp', 'engine=stream;stream_rows=7;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<bitpacked,3x3x256,rows7>', 512, 'engine=auto'),
    (2, 14, 14, 256, 512, 2, 'bp', 'engine=wstream;wstream_images=1;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<bitpacked,3x3x256,images1,blocks2>', 512, 'engine=wstream'),
    (16, 14, 14, 256, 512, 2, 'bp', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<bitpacked,3x3x256,rows1>', 1024, 'engine=stream'),
    (32, 14, 14, 256, 512, 2, 'bp', 'engine=stream;stream_rows=1;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<bitpacked,3x3x256,rows1>', 2048, 'engine=stream'),
    (8, 7, 7, 512, 512, 1, 'f32', 'engine=stream;stream_rows=7;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=1;compute_units=8', 'bconv2d_stream<f32,3x3x512,rows7>', 256, 'engine=stream'),
    (4, 56, 56, 64, 64, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=1;stream_blocks_per_cu=2;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x64,rows14,il,x2>', 512, 'engine=stream;stream_rows=14;stream_interleave=1;stream_blocks_per_cu=2'),
    (7, 56, 56, 64, 64, 1, 'f32', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x64,rows56>', 1024, 'engine=stream'),
    (15, 56, 56, 64, 64, 1, 'f32', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x64,rows56>', 2048, 'engine=stream'),
    (3, 56, 56, 64, 64, 1, 'i8', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x64,rows56>', 512, 'engine=auto'),
    (7, 56, 56, 64, 64, 1, 'i8', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x64,rows56>', 1024, 'engine=auto'),
    (15, 56, 56, 64, 64, 1, 'i8', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x64,rows56>', 2048, 'engine=auto'),
    (5, 56, 56, 64, 64, 1, 'bp', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=2;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x64,rows56,x2>', 1024, 'engine=auto'),
    (15, 56, 56, 64, 64, 1, 'bp', 'engine=stream;stream_rows=56;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x64,rows56>', 2048, 'engine=auto'),
    (3, 28, 28, 128, 128, 1, 'i8', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows28>', 512, 'engine=auto'),
    (7, 28, 28, 128, 128, 1, 'i8', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows28>', 1024, 'engine=auto'),
    (15, 28, 28, 128, 128, 1, 'i8', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows28>', 2048, 'engine=auto'),
    (3, 28, 28, 128, 128, 1, 'bp', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows28>', 512, 'engine=auto'),
    (7, 28, 28, 128, 128, 1, 'bp', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows28>', 1024, 'engine=auto'),
    (15, 28, 28, 128, 128, 1, 'bp', 'engine=stream;stream_rows=28;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows28>', 2048, 'engine=auto'),
    (3, 14, 14, 256, 256, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x256,rows14>', 512, 'engine=auto'),
    (7, 14, 14, 256, 256, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x256,rows14>', 1024, 'engine=auto'),
    (15, 14, 14, 256, 256, 1, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x256,rows14>', 2048, 'engine=auto'),
    (3, 14, 14, 256, 256, 1, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x256,rows14>', 512, 'engine=auto'),
    (7, 14, 14, 256, 256, 1, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x256,rows14>', 1024, 'engine=auto'),
    (15, 14, 14, 256, 256, 1, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x256,rows14>', 2048, 'engine=stream'),
    (3, 14, 14, 256, 256, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x256,rows14>', 512, 'engine=auto'),
    (7, 14, 14, 256, 256, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x256,rows14>', 1024, 'engine=auto'),
    (15, 14, 14, 256, 256, 1, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x256,rows14>', 2048, 'engine=auto'),
    (3, 7, 7, 512, 512, 1, 'f32', 'engine=wstream;wstream_images=2;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<f32,3x3x512,images2,blocks4>', 512, 'engine=auto'),
    (3, 7, 7, 512, 512, 1, 'i8', 'engine=wstream;wstream_images=2;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<i8,3x3x512,images2,blocks4>', 512, 'engine=auto'),
    (3, 7, 7, 512, 512, 1, 'bp', 'engine=wstream;wstream_images=2;wstream_blocks=4;compute_units=2', 'bconv2d_wstream<bitpacked,3x3x512,images2,blocks4>', 512, 'engine=auto'),
    (15, 28, 28, 128, 256, 2, 'f32', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<f32,3x3x128,rows14>', 2048, 'engine=stream'),
    (3, 28, 28, 128, 256, 2, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows14>', 512, 'engine=auto'),
    (7, 28, 28, 128, 256, 2, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows14>', 1024, 'engine=auto'),
    (15, 28, 28, 128, 256, 2, 'i8', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<i8,3x3x128,rows14>', 2048, 'engine=auto'),
    (3, 28, 28, 128, 256, 2, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows14>', 512, 'engine=auto'),
    (7, 28, 28, 128, 256, 2, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows14>', 1024, 'engine=auto'),
    (15, 28, 28, 128, 256, 2, 'bp', 'engine=stream;stream_rows=14;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=2', 'bconv2d_stream<bitpacked,3x3x128,rows14>', 2048, 'engine=auto'),
    (7, 14, 14, 256, 512, 2, 'bp', 'engine=stream;stream_rows=7;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=0;compute_units=4', 'bconv2d_stream<bitpacked,3x3x256,rows7>', 512, 'engine=auto'),
    (7, 7, 7, 512, 512, 1, 'f32', 'engine=stream;stream_rows=7;stream_interleave=0;stream_blocks_per_cu=1;stream_flat=1;compute_units=8', 'bconv2d_stream<f32,3x3x512,rows7>', 256, 'engine=stream'),
]


# ------------------------------------------------------------------------------------ operands and the oracle's answer

class Operands(NamedTuple):
    x: np.ndarray
    w: np.ndarray
    mul: Optional[np.ndarray]
    bias: Optional[np.ndarray]
    thr: Optional[np.ndarray]
    scale: float
    zp: int
    want: np.ndarray                    # the oracle's output, all images
    want_bits: Optional[np.ndarray]     # its LceQuantize (float / int8 output), None for bitpacked output


def operands(spec: O.ConvSpec, dst: str, seed: int, zero_point: Optional[int] = None, threads: int = 8) -> Operands:
    """Seeded operands as tests/test_hostsim_kernels.py's _run_all_dst_mfma makes them (a fifth of the multipliers negative; thresholds
    with INT32_MAX / INT32_MIN / -1 entries; int8 parameters from synth.int8_quant_params unless `zero_point` is given) and the
    oracle's output."""
    x, w, mul, bias = synth.conv_inputs(spec, seed, negative_mul_fraction=0.2)
    scale, zp = 1.0, 0
    if dst == "i8":
        scale, zp = synth.int8_quant_params(seed)
        scale, zp = float(scale), zp if zero_point is None else zero_point
    if dst == "bp":
        thr = O.thresholds_converter(spec, mul, bias)
        thr[::5] = np.iinfo(np.int32).max
        thr[1::7] = np.iinfo(np.int32).min
        thr[2::11] = -1
        return Operands(x, w, None, None, thr, scale, zp, O.bconv2d(spec, O.DST_BITPACKED, x, w, thresholds=thr, threads=threads), None)
    want = O.bconv2d(spec, DST_OF[dst], x, w, mul, bias, out_scale=scale, out_zero_point=zp, threads=threads)
    return Operands(x, w, mul, bias, None, scale, zp, want, O.bitpack(want, zp))


def case_operands(index: int) -> Operands:
    """The operands of LONG_RUN_CASES[index]; every third int8 entry's zero point is an end of int8's range (-128: no value is below it,
    127), by entry index."""
    case = LONG_RUN_CASES[index]
    extreme = (-128, 127)[(index // 3) % 2] if index % 3 == 0 else None
    return operands(case_spec(case), case[6], 7000 + index, extreme)


# ------------------------------------------------------------------------------------ seeded draws of forced geometry

PADDINGS = {"ONE": (O.PADDING_SAME, 1), "VALID": (O.PADDING_VALID, 0), "SAME0": (O.PADDING_SAME, 0)}
FORCED_SEED, FORCED_CANDIDATES = 9, 160


class ForcedCase(NamedTuple):
    spec: O.ConvSpec
    dst: str
    options: str
    seed: int


def _draw_forced(g) -> ForcedCase:
    pick = lambda seq: seq[int(g.integers(len(seq)))]
    # (weights: a long run of a wide map with a deep filter bank needs a ring that does not fit LDS, and a refused draw tests nothing)
    h, w = pick([(7, 7), (7, 7), (8, 12), (8, 12), (14, 14), (14, 14), (9, 30), (28, 28)])
    cin, cout = pick([64, 64, 128, 128, 192, 256, 320, 512]), pick([32, 64, 96, 128, 256, 320])
    batch, stride = int(g.integers(2, 25)), pick([1, 2])
    padding, pad_values = PADDINGS[pick(["ONE", "VALID", "SAME0"])]
    dst = pick(DST_NAMES)
    # SAME-zero padding: the reference semantics (exact zero padding; what the streaming kernels run), which take an even channel count
    spec = O.ConvSpec(batch, h, w, cin, 3, 3, cout, 1, stride, stride, 1, 1, padding, pad_values, O.ACT_NONE, O.SEM_REFERENCE)
    engine = pick(["stream", "stream", "wstream"])
    # (the weight-streaming kernel keeps whole expanded images in LDS and has no 64-channel instance: such draws go to the other kernel)
    images = pick([0, 1, 2, 3])
    image_bytes = ((spec.out_h - 1) * stride + 3) * ((spec.out_w - 1) * stride + 3) * ((cin + 63) // 64 * 32 + 16)
    if engine == "wstream" and (cin <= 64 or max(1, images) * image_bytes > 144 * 1024):
        engine = "stream"
    options = {"engine": engine, "compute_units": pick([1, 2, 3, 5, 7])}
    if engine == "stream":
        divisors = [r for r in range(1, spec.out_h + 1) if spec.out_h % r == 0]
        options["stream_rows"] = pick([0] + divisors)
        options["stream_interleave"] = pick(["0", "1", "auto"])
        # (two blocks per CU: one instance is compiled for it -- every second draw there, one in sixteen elsewhere, where it is refused)
        options["stream_blocks_per_cu"] = pick(["auto", "2"] if dst == "bp" and cin == 64 else ["auto"] * 15 + ["2"])
        options["stream_pixel_phases"] = pick([0, 0, 2, 4])
        options["stream_flat"] = pick([0, 1])
    else:
        options["wstream_images"] = images
        options["wstream_blocks"] = pick([0, 1, 2, 4])
    return ForcedCase(spec, dst, option_string(options), int(g.integers(0, 10_000)))


def forced_geometry_candidates(seed: int = FORCED_SEED, n: int = FORCED_CANDIDATES):
    """`n` candidates from a PCG64 stream: the same list on every machine."""
    g = np.random.Generator(np.random.PCG64(seed))
    return [_draw_forced(g) for _ in range(n)]


def forced_geometry_cases(seed: int = FORCED_SEED, n: int = FORCED_CANDIDATES):
    """(kept, dropped) of forced_geometry_candidates: the ones the host planner refuses (an option the layer's instance is not compiled
    for, a ring that does not fit, an image too large to be resident) are dropped."""
    kept, dropped = [], []
    for case in forced_geometry_candidates(seed, n):
        (dropped if plan_fields(case.spec, DST_OF[case.dst], case.options)["err"] else kept).append(case)
    return kept, dropped


# The candidates (by index) that the host planner refuses, as a literal: the GPU test takes the kept ones from here, without the host
# simulation (tests/test_launch_geometry_host.py checks the list against the planner).
FORCED_DROPPED = (1, 4, 6, 14, 18, 20, 21, 23, 24, 32, 35, 45, 47, 48, 49, 50, 54, 64, 73, 74, 87, 89, 90, 92, 94, 95, 99, 100, 103, 112, 115, 117, 118, 123, 124, 126, 127, 131, 141, 143, 149, 150, 151, 158)


def forced_kept():
    return [c for i, c in enumerate(forced_geometry_candidates()) if i not in FORCED_DROPPED]


def forced_id(case: ForcedCase) -> str:
    s = case.spec
    pad = {(O.PADDING_SAME, 1): "one", (O.PADDING_VALID, 0): "valid", (O.PADDING_SAME, 0): "same0"}[(s.padding, s.pad_values)]
    return "b%d_%dx%dx%d-%d_s%d_%s_%s_%s" % (s.batch, s.in_h, s.in_w, s.channels_in, s.channels_out, s.stride_h, pad, case.dst,
                                               case.options.replace(";", ",").replace("=", ""))
