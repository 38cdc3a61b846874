"""The real kernel bodies of csrc/lce_kernels_transition.h on the CPU (tests/hostsim_transition: 256 lanes of a block as fibers)
against tests/transition_ref.py -- tests/pool_ref.py's MAX pool composed with tests/depthwise_ref.py / tests/depthwise_i8_ref.py --
byte for byte: QuickNet's geometry on shapes with odd extents, clipped windows and ragged channels, the general geometries of the row
path, both paths (the entry's own choice, asserted, and the row path forced), the three output combinations, more work than one
pass of a capped grid, the special float values, and an input that ends at a page that cannot be read."""
import ctypes as C
import mmap

import numpy as np
import pytest

import depthwise_i8_ref as DI
import depthwise_ref as DF
import transition_cases as TC
import transition_ref as R
from hostsim_transition_lib import sim_f32, sim_i8


@pytest.mark.parametrize("name", sorted(TC.F32))
def test_the_float_kernel_bodies_give_the_compositions_bytes(name):
    c = TC.F32[name]
    vecs = TC.check_f32(sim_f32, c)
    assert (vecs > 0) == TC.expect_vec(c, 4, False)


@pytest.mark.parametrize("name", sorted(TC.I8))
def test_the_int8_kernel_bodies_give_the_compositions_bytes(name):
    c = TC.I8[name]
    vecs = TC.check_i8(sim_i8, c)
    assert (vecs > 0) == TC.expect_vec(c, 16, False)


def test_the_sixteen_byte_paths_are_covered():
    """The grid must reach both 16-byte kernels with and without bits, and the row kernels with a geometry the other path refuses."""
    assert sum(TC.expect_vec(c, 4, True) for c in TC.F32.values()) >= 3 and sum(TC.expect_vec(c, 16, True) for c in TC.I8.values()) >= 2
    assert sum(not TC.vec_geometry(c) for c in TC.F32.values()) >= 6 and sum(not TC.vec_geometry(c) for c in TC.I8.values()) >= 6
    assert any(TC.expect_vec(c, 16, False) and not TC.expect_vec(c, 16, True) for c in TC.I8.values())


def test_unaligned_operands_take_the_row_path():
    c = TC.F32["quicknet_2x7x9x32"]
    x, w, bias = TC.operands_f32(c)
    out, bits, vec = sim_f32(x, c["pool"], w, bias, c["stride"], c["padding"], 1, c["act"], offset=4)
    want = TC.want_f32(c, x, w, bias)
    assert not vec and np.array_equal(out.view(np.int32), want.view(np.int32)) and np.array_equal(bits, R.bitpack_f32(want))
    c = TC.I8["quicknet_2x7x9x32"]
    x, pool, w, bias, sw, q_out = TC.operands_i8(c)
    out, bits, vec = sim_i8(x, pool, w, bias, sw, q_out, c["stride"], c["padding"], 1, c["act"], offset=1)
    want = TC.want_i8(c, x, pool, w, bias, sw, q_out)
    assert not vec and np.array_equal(out, want) and np.array_equal(bits, DI.bitpack(want, q_out[1]))


@pytest.mark.parametrize("path", (None, 0))
def test_more_work_than_one_pass_of_a_capped_grid(path):
    """Two blocks of four waves.  2 x 10 x 9 output pixels of 96 channels: float 24 chunks a pixel = 4320 chunks = 68 wave tasks (the
    last with 32 chunks), int8 6 chunks a pixel = 17 wave tasks, and 360 segments on the row path -- several passes each, tasks
    that span the two images and a grid stride that is no multiple of a pixel's chunks."""
    c = TC.quicknet((2, 20, 17, 96), act=R.RELU, seed=50)
    x, w, bias = TC.operands_f32(c)
    want = TC.want_f32(c, x, w, bias)
    assert want.shape == (2, 10, 9, 96)
    out, bits, vec = sim_f32(x, c["pool"], w, bias, c["stride"], c["padding"], 1, c["act"], path=path, cap=2)
    assert vec == (path is None)
    assert np.array_equal(out.view(np.int32), want.view(np.int32)) and np.array_equal(bits, R.bitpack_f32(want))
    x, pool, w, bias, sw, q_out = TC.operands_i8(c)
    want = TC.want_i8(c, x, pool, w, bias, sw, q_out)
    out, bits, vec = sim_i8(x, pool, w, bias, sw, q_out, c["stride"], c["padding"], 1, c["act"], path=path, cap=2)
    assert vec == (path is None)
    assert np.array_equal(out, want) and np.array_equal(bits, DI.bitpack(want, q_out[1]))


@pytest.mark.parametrize("pool_act", (R.NONE, R.RELU_N1_TO_1))
@pytest.mark.parametrize("path", (None, 0))
def test_signed_zeros_nan_and_infinities_in_the_pool_windows(path, pool_act):
    """Every pool window draws from +0.0, -0.0, NaN, +-inf, +-FLT_MAX and two ordinary values.  m = (m < x) ? x : m from -FLT_MAX in
    raster order keeps the FIRST of +0.0 / -0.0, never takes a NaN, and the clamp turns +inf into the range's end: the pooled
    value is always finite, and the blur (weights that sum to 1) of it is too.  The row-by-row streaming of the 16-byte path must
    keep that order: its bytes are the composition's, under the blur and under a 1x1 filter of weight 1 (the pooled value times one)."""
    g = np.random.default_rng(7)
    palette = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, R.P.FLT_MAX, -R.P.FLT_MAX, 1.5, -2.0], np.float32)
    x = palette[g.integers(0, palette.size, (2, 6, 6, 32))]
    x[0, 0, 0, :], x[0, 0, 1, :], x[0, 1, 0, :], x[0, 1, 1, :] = -0.0, 0.0, -1.0, np.nan       # -0.0 first: it stays
    x[0, 2, 0, :], x[0, 2, 1, :], x[0, 3, 0, :], x[0, 3, 1, :] = -3.0, 0.0, -0.0, 0.0          # +0.0 first, in the row above -0.0
    pool = dict(TC.QUICKNET["pool"], activation=pool_act)
    pooled = R.pooled(x, pool)
    assert np.isfinite(pooled).all()
    assert np.signbit(pooled[0, 0, 0, 0]) and pooled[0, 0, 0, 0] == 0 and not np.signbit(pooled[0, 2, 0, 0]) and pooled[0, 2, 0, 0] == 0
    for w, stride, bias in ((DF.BLUR[:, :, None].repeat(32, 2), (2, 2), None), (np.ones((1, 1, 32), np.float32), (1, 1), np.full(32, -0.0, np.float32))):
        want = R.pool_depthwise(x, pool, w, bias, stride, R.SAME)
        assert np.isfinite(want).all()
        out, bits, vec = sim_f32(x, pool, w, bias, stride, R.SAME, 1, R.NONE, path=path)
        assert vec == (path is None)
        assert np.array_equal(out.view(np.int32), want.view(np.int32)) and np.array_equal(bits, R.bitpack_f32(want))


def _at_page_end(x):
    """A copy of `x` that ENDS where a page that cannot be read begins; the mapping lives as long as the view."""
    page = mmap.PAGESIZE
    pages = (x.nbytes + page - 1) // page
    libc = C.CDLL(None, use_errno=True)
    libc.mmap.restype = C.c_void_p
    libc.mmap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    base = libc.mmap(None, (pages + 1) * page, mmap.PROT_READ | mmap.PROT_WRITE, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)
    assert base not in (None, C.c_void_p(-1).value), C.get_errno()
    assert libc.mprotect(base + pages * page, page, 0) == 0, C.get_errno()
    start = base + pages * page - x.nbytes
    v = np.ctypeslib.as_array((C.c_uint8 * x.nbytes).from_address(start)).view(x.dtype).reshape(x.shape)
    v[...] = x
    return v


@pytest.mark.parametrize("path", (None, 0))
def test_an_input_of_the_exact_size_with_a_guard_page_behind_it(path):
    """The clipped last row and column of the pool and the lanes past the end read nothing behind the input: a read of one byte
    more would end the process."""
    for c in (TC.quicknet((1, 4, 4, 32), seed=60), TC.quicknet((2, 3, 5, 32), seed=61)):
        x, w, bias = TC.operands_f32(c)
        want = TC.want_f32(c, x, w, bias)
        out, bits, vec = sim_f32(x, c["pool"], w, bias, c["stride"], c["padding"], 1, c["act"], path=path, place_x=_at_page_end)
        assert vec == (path is None)
        assert np.array_equal(out.view(np.int32), want.view(np.int32)) and np.array_equal(bits, R.bitpack_f32(want))
