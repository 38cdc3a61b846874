"""The real kernel bodies of csrc/lce_kernels_conv2d.h on the CPU (tests/hostsim_conv2d: 256 lanes of a block as fibers, the
f32-input matrix instruction emulated as the k-ordered fmaf chain the kernels take it for) against tests/conv2d_ref.py, byte for
byte: the known answers worked by hand, a grid over K = fh fw Cin, images, strides, paddings and output channels with rotating
bias, activation and output combination, both load paths (16-byte and dword, by the operands' alignment), special values, and more
tiles than one pass of a capped grid on both pixel enumerations.  What a simulation cannot decide -- that the instruction IS such
a chain -- is the GPU suite's (tests/test_gpu_conv2d.py)."""
import ctypes as C
import os
from section_models import float_fixture

import numpy as np
import pytest

import conv2d_ref as R
import hostsim_lib
import oracle_lib as O
from test_conv2d_sections_host import ACTS, KNOWN, grid_operands, known_case

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_conv2d")
OUT_MARK, BITS_MARK = np.float32(777), 0x55555555
_lib = None


def lib():
    """tests/hostsim_conv2d/liblce_hostsim_conv2d.so (hostsim_lib.load brings it up to date first)."""
    global _lib
    if _lib is None:
        _lib = hostsim_lib.load(DIR, "liblce_hostsim_conv2d.so")
        _lib.lce_hostsim_conv2d.argtypes = [C.c_void_p] * 6 + [C.c_int32]
    return _lib


def placed(a, offset):
    """A copy of `a` whose first byte lies `offset` floats behind a 16-byte boundary."""
    return hostsim_lib.placed(a, 4 * offset)


def sim(x, w, bias, stride, padding, act, want_out=True, want_bits=True, cap=3, offset=0):
    """(out, bits, took the 16-byte path, ran the border launch); an output that was not asked for keeps its marks."""
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    x, w = placed(x, offset), placed(w, offset)
    oh, ow = R.out_and_pad(x.shape[1], w.shape[1], st[0], padding)[0], R.out_and_pad(x.shape[2], w.shape[2], st[1], padding)[0]
    d = (C.c_int32 * 12)(*x.shape, w.shape[0], w.shape[1], w.shape[2], st[0], st[1], oh, ow, act)
    out = np.full((x.shape[0], oh, ow, w.shape[0]), OUT_MARK, np.float32)
    bits = np.full((x.shape[0], oh, ow, (w.shape[0] + 31) // 32), BITS_MARK, np.int32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    ran = lib().lce_hostsim_conv2d(d, x.ctypes.data, w.ctypes.data, None if b is None else b.ctypes.data,
                                   out.ctypes.data if want_out else None, bits.ctypes.data if want_bits else None, cap)
    return out, bits, bool(ran & 1), bool(ran & 2)


def agree(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name):
    x, w, bias, kw, want = known_case(name)
    out, bits, _, _ = sim(x, w, bias, kw["stride"], kw["padding"], R.NONE)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(bits, O.bitpack(want)), (out, want)


# (filter, Cin): K = 1, 27, 24 and 36 (the 16-byte path; 36 ends a chunk inside a tap), 147 and 297 (several chunks), 15; and
# 1x1 filters, for which the interior launch is the whole call: K = 4 (the 16-byte path, one short chunk), 33 (the dword path,
# ends inside a chunk), 68 (the 16-byte path, two full chunks and a tail)
@pytest.mark.parametrize("filt,cin", [((1, 1), 1), ((3, 3), 3), ((2, 3), 4), ((3, 3), 4), ((7, 7), 3), ((3, 3), 33), ((1, 5), 3),
                                      ((1, 1), 4), ((1, 1), 33), ((1, 1), 68)])
@pytest.mark.parametrize("special", [False, True])
def test_the_kernel_bodies_give_the_reference_bytes(filt, cin, special):
    w, bias = grid_operands(filt, cin, 160 if not special else 33, special)
    n, vecs = 0, 0
    for image, batch in (((1, 1), 1), ((5, 7), 3), ((9, 8), 1)):
        x = float_fixture((batch, *image, cin), image[0] * 1000 + batch * 100 + cin, special)
        for stride in ((1, 1), (2, 1), (4, 3)):
            for padding in (R.SAME, R.VALID):
                if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
                    continue
                t = R.chain(x, w, stride, padding)
                for cout in ((1, 33, 160) if not special else (33,)):
                    act, with_bias, offset = ACTS[n % 4], (n // 4) % 2 == 0, (n // 2) % 2
                    b = bias[:cout] if with_bias else None
                    want = R.finish(t[..., :cout], b, act)
                    outs = (dict(), dict(want_out=False), dict(want_bits=False))[n % 3]
                    out, bits, vec, border = sim(x, w[:cout], b, stride, padding, act, offset=offset, **outs)
                    assert vec == (cin % 4 == 0 and offset == 0)
                    assert not (border and filt == (1, 1)), "a 1x1 filter has no clipped window: one launch"
                    vecs += vec
                    assert agree(out, want) if outs.get("want_out", True) else (out == OUT_MARK).all(), (image, stride, padding, cout, n)
                    assert np.array_equal(bits, O.bitpack(want)) if outs.get("want_bits", True) else (bits == BITS_MARK).all(), (image, stride, padding, cout, n)
                    n += 1
    assert n >= 9 and (vecs > 0) == (cin % 4 == 0)


@pytest.mark.parametrize("kind", ["interior", "border"])
def test_more_tiles_than_one_pass_of_a_capped_grid(kind):
    """Two blocks per launch.  interior: 2 x 38 x 35 interior pixels are 21 tiles, the last with 100 of its 128 rows, and tiles
    span the two images.  border: a 1 x 41 filter on 20 x 20 clips every window: 400 wave tasks against 8 waves."""
    if kind == "interior":
        x, (w, bias) = float_fixture((2, 40, 37, 1), 5), grid_operands((3, 3), 1, 33)
        assert 2 * 38 * 35 == 20 * 128 + 100
    else:
        x, (w, bias) = float_fixture((1, 20, 20, 1), 5), grid_operands((1, 41), 1, 33)
    want = R.conv2d(x, w, bias, (1, 1), R.SAME, R.RELU)
    out, bits, _, _ = sim(x, w, bias, 1, R.SAME, R.RELU, cap=2)
    assert agree(out, want) and np.array_equal(bits, O.bitpack(want))
