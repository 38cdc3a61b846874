"""The streaming kernels' long per-block runs on the GPU, through the C ABI against the oracle (tests/launch_geometry.py).

At 512 .. 2048 images per GPU a block of bconv2d_stream walks 14 .. 56 segments or 2 .. 8 whole images, its ring wrapping many times,
and bconv2d_wstream keeps two images resident; at up to 256 images -- all the other GPU tests -- a run is at most one image long.
Only the GPU has the counted waits, the LDS-DMA ordering and the ring's read / write separation for real.  LONG_RUN_CASES gives a
block the same work on 2 .. 8 `compute_units` and a few images:

* every entry equals the oracle on all images, with the second output, nothing written outside either;
* the same operands with the device's own CU count (short runs) give the same bytes;
* seeded draws of forced geometry options (segment rows, interleave, pixel phases, flat runs, two blocks per CU, resident images);
* run_host, whose slices are launches smaller than the one planned for (make_stream_args / make_ws_args)."""
import os

import numpy as np
import pytest
import torch

import launch_geometry as L
import oracle_lib as O
from lce_amd import amd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NTHREADS = min(16, os.cpu_count() or 8)
GUARD = 64
ADST = {"f32": amd.F32, "i8": amd.I8, "bp": amd.BITPACKED}
TDTYPE = {"f32": torch.float32, "i8": torch.int8, "bp": torch.int32}


def _plan(spec, dst, ops, options):
    plan = amd.Bconv2dPlan(amd.ConvParams(spec.batch, spec.in_h, spec.in_w, spec.channels_in, spec.filter_h, spec.filter_w, spec.channels_out,
                                          spec.groups, spec.stride_h, spec.stride_w, spec.dilation_h, spec.dilation_w, spec.padding,
                                          spec.pad_values, spec.activation, ADST[dst], spec.semantics, out_scale=ops.scale,
                                          out_zero_point=ops.zp))
    plan.set_weights(ops.w, ops.mul, ops.bias, ops.thr)
    for key, value in L.option_dict(options).items():
        plan.set_option(key, str(value))
    return plan


def _guarded(shape, dtype):
    """(buffer, view): `view` is a tensor of `shape` 64 bytes into a buffer poisoned with 0x5A, 64 more bytes behind it."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype).reshape(shape)


def _guards_untouched(buf):
    edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((edge == 0x5A).all())


def _bytes(t):
    return t.contiguous().cpu().numpy().view(np.uint8)


def _first_bad_image(got, want):
    bad = np.nonzero((got.reshape(want.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1)).any(axis=1))[0]
    return "first differing image %d of %d" % (int(bad[0]), want.shape[0]) if bad.size else "equal"


def _check_against_the_oracle(spec, dst, ops, options, kernel=None):
    """run into a guarded, poisoned buffer; float / int8 plans again as run_dual into poisoned bits."""
    plan = _plan(spec, dst, ops, options)
    xd = torch.from_numpy(ops.x).to(DEV)
    buf, out = _guarded(plan.output_shape, TDTYPE[dst])
    plan.run(xd, out)
    torch.cuda.synchronize()
    name = plan.kernel_name()
    if kernel is not None:
        assert name == kernel
    got = _bytes(out)
    assert np.array_equal(got, ops.want.view(np.uint8)), (name, _first_bad_image(got, ops.want))
    assert _guards_untouched(buf), (name, "wrote outside the output")
    if dst == "bp":
        return name
    buf2, out2 = _guarded(plan.output_shape, TDTYPE[dst])
    bits_buf, bits = _guarded(ops.want_bits.shape, torch.int32)
    plan.run_dual(xd, out2, bits)
    torch.cuda.synchronize()
    assert torch.equal(out2, out), (name, "run_dual's output differs from run's")
    # (the oracle's bitpack leaves the padding bits of a ragged last word 0)
    assert np.array_equal(bits.cpu().numpy(), ops.want_bits), (name, "second output")
    assert _guards_untouched(buf2) and _guards_untouched(bits_buf), (name, "run_dual wrote outside its outputs")
    return name


_IDS = [L.case_id(c) for c in L.LONG_RUN_CASES]


@pytest.mark.parametrize("index", range(len(L.LONG_RUN_CASES)), ids=lambda i: _IDS[i])
def test_long_runs_equal_the_oracle(index):
    case = L.LONG_RUN_CASES[index]
    _check_against_the_oracle(L.case_spec(case), case[6], L.case_operands(index), case[7], kernel=case[8])


@pytest.mark.parametrize("index", range(len(L.LONG_RUN_CASES)), ids=lambda i: _IDS[i])
def test_long_runs_equal_short_runs(index):
    """The same operands and options with `compute_units` left to the device: a block's run is a fraction of an image, the bytes are the
    same (the kernel name may differ in what follows from the run length)."""
    case = L.LONG_RUN_CASES[index]
    spec, dst = L.case_spec(case), case[6]
    ops = L.case_operands(index)
    xd = torch.from_numpy(ops.x).to(DEV)
    long_plan = _plan(spec, dst, ops, case[7])
    short_options = {k: v for k, v in L.option_dict(case[7]).items() if k == "engine"}
    short_plan = _plan(spec, dst, ops, short_options)
    long_out, short_out = long_plan.run(xd), short_plan.run(xd)
    torch.cuda.synchronize()
    names = (long_plan.kernel_name(), short_plan.kernel_name())
    assert names[0] == case[8] and names[1].split("<")[0] == names[0].split("<")[0], names
    assert torch.equal(long_out, short_out), names


def test_forced_geometry_draws():
    """The draws that the host planner accepts (tests/test_launch_geometry_host.py keeps L.FORCED_DROPPED equal to its verdict): a
    refusal here is a failure."""
    kept = L.forced_kept()
    assert len(kept) >= 100
    families = set()
    for case in kept:
        ops = L.operands(case.spec, case.dst, case.seed, threads=NTHREADS)
        try:
            name = _check_against_the_oracle(case.spec, case.dst, ops, case.options)
        except amd.LceHipError as e:
            raise AssertionError("the GPU refused %s: %s" % (L.forced_id(case), e))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (L.forced_id(case), e))
        assert name.startswith("bconv2d_%s<" % L.option_dict(case.options)["engine"]), (L.forced_id(case), name)
        families.add(name.split(",")[0])
    assert len(families) == 6, sorted(families)        # both kernels with each output type


# (name, spec, output type, options, kernel): plans whose run_host slices are launches SMALLER than the one planned for.  The batch
# is the smallest that lce_hip_bconv2d_run_host (csrc/lce_hip_api.hip) cuts into 3 slices: slices = min(8, input + output bytes / 8 MiB).
#  * the flat run's ring holds at most 4 images (tests/launch_geometry.py, EXTRA_CELLS), so 244 images need 61 blocks: no small
#    compute_units there; two blocks per CU hold at most 2 whole images each, so 502 images need 251;
#  * slices of 82 / 81 images are no multiples of the flat run of 4; slices of 297 images leave the last group of images2 with one.
RUN_HOST_CASES = [
    ("stream_rows4_il", L.layer_spec(61, 28, 28, 128, 128, 1), "f32", "engine=stream;stream_rows=4;stream_interleave=1;compute_units=4",
     "bconv2d_stream<f32,3x3x128,rows4,il>"),
    ("stream_flat", L.layer_spec(244, 7, 7, 512, 512, 1), "f32", "engine=stream;stream_rows=7;stream_flat=1;compute_units=256",
     "bconv2d_stream<f32,3x3x512,rows7>"),
    ("wstream_images2", L.layer_spec(892, 7, 7, 512, 512, 1), "i8", "engine=wstream;wstream_images=2;compute_units=2",
     "bconv2d_wstream<i8,3x3x512,images2,blocks4>"),
    ("stream_x2", L.layer_spec(502, 56, 56, 64, 64, 1), "bp", "engine=stream;stream_blocks_per_cu=2;compute_units=128",
     "bconv2d_stream<bitpacked,3x3x64,rows56,x2>"),
    ("pointwise", O.ConvSpec(446, 14, 14, 256, 1, 1, 256), "i8", "engine=pointwise;compute_units=4", "bconv2d_pointwise<i8,K4x64,N2x32>"),
]


@pytest.mark.parametrize("name,spec,dst,options,kernel", RUN_HOST_CASES, ids=[c[0] for c in RUN_HOST_CASES])
def test_run_host_slices_launch_less_than_planned(name, spec, dst, options, kernel):
    ops = L.operands(spec, dst, 9100 + spec.batch, threads=NTHREADS)
    # lce_hip_bconv2d_run_host: slices = min(8, max(1, batch * (input + output bytes of an image) / 8 MiB)), at most one per image;
    # slice k has batch / slices images, the first batch % slices one more
    traffic = ops.x.nbytes + ops.want.nbytes
    slices = min(8, max(1, traffic // (8 << 20)), spec.batch)
    assert slices == 3 and (traffic - traffic // spec.batch) // (8 << 20) < 3, "the smallest batch that is cut into 3 slices"
    sizes = [spec.batch // slices + (1 if k < spec.batch % slices else 0) for k in range(slices)]
    if name == "stream_flat":
        assert all(s % 4 for s in sizes), sizes         # no slice is a multiple of the planned run of 4 images
    if name == "wstream_images2":
        assert any(s % 2 for s in sizes), sizes         # an odd slice: its last group has one image
    plan = _plan(spec, dst, ops, options)
    assert plan.kernel_name() == kernel
    device = plan.run(torch.from_numpy(ops.x).to(DEV))
    torch.cuda.synchronize()
    host_buf = np.full(ops.want.nbytes + 2 * GUARD, 0x5A, np.uint8)
    host = host_buf[GUARD:GUARD + ops.want.nbytes].view(ops.want.dtype).reshape(ops.want.shape)
    assert plan.run_host(ops.x, host) is host
    assert plan.kernel_name() == kernel
    got = _bytes(device)
    assert np.array_equal(got, ops.want.view(np.uint8)), (kernel, "run", _first_bad_image(got, ops.want))
    assert np.array_equal(host.view(np.uint8), ops.want.view(np.uint8)), (kernel, "run_host", _first_bad_image(host.view(np.uint8), ops.want))
    assert (host_buf[:GUARD] == 0x5A).all() and (host_buf[-GUARD:] == 0x5A).all(), (kernel, "run_host wrote outside the output")
