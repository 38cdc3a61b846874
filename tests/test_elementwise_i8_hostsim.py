"""The kernels of lce_hip_elementwise_i8 on the CPU (tests/hostsim_eltwise_i8: the real bodies of
csrc/lce_kernels_eltwise_i8_chain.h between guard bytes) against the NumPy restatement (tests/elementwise_i8_ref.py): every path,
both layouts, with and without a head, pointer offsets, every combination of outputs, in place, and a grid small enough that
waves stride."""
import importlib

import numpy as np
import pytest

import elementwise_i8_ref as E
import hostsim_eltwise_i8_lib as S

amd = importlib.import_module("compute-engine_amd")

# (129, 32) is 258 chunks: a partial 256-chunk iteration of the flat layout
SHAPES = [(257, 1), (300, 31), (129, 32), (256, 33), (260, 64), (257, 96)]
LDS, GLOBAL, ONE_ROW = amd.EW_I8_PATH_LDS, amd.EW_I8_PATH_GLOBAL, amd.EW_I8_PATH_ONE_ROW


def _case(seed, rows, channels, head, per_channel=True):
    g = np.random.default_rng(seed)
    x = g.integers(-128, 128, (rows, channels)).astype(np.int8)
    x[0, :] = -128
    x[-1, :] = 127
    addend = g.integers(-128, 128, (rows, channels)).astype(np.int8) if head else None
    if head:
        q_in, h, steps = E.reactnet_tail(g, channels)
        if not per_channel:
            steps = [E.draw_step(g, "prelu", h[1], channels, False)]
    else:
        h = None
        q_in = (E._scale(g), E._zp(g))
        first = E.draw_step(g, str(g.choice(["add", "prelu"])), q_in, channels, per_channel)
        if per_channel and np.ndim(first[1]) == 0:
            first = first[:1] + (np.full(channels, first[1], np.int8),) + first[2:]
        steps = [first, E.draw_step(g, str(g.choice(["clamp", "requantize"])), first[3], channels, False)]
    want = E.chain(x, q_in, steps, addend, h)
    return x, addend, q_in, h, steps, want


@pytest.mark.parametrize("rows,channels", SHAPES)
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("path", [None, LDS, GLOBAL, ONE_ROW])
def test_every_path_at_every_shape(rows, channels, head, path):
    x, addend, q_in, h, steps, want = _case(rows * 1000 + channels, rows, channels, head, per_channel=path != ONE_ROW)
    out, bits, L = S.sim_chain(x, q_in, steps, addend, h, path=path)
    assert L["path"] == ((ONE_ROW if channels == 1 else GLOBAL) if path is None else path)     # (below 128 channels: the global path)
    assert L["flat"] == (channels % 32 == 0) and L["table_rows"] == (1 if path == ONE_ROW else channels)
    assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("rows,channels", [(129, 32), (256, 33)])
def test_int8_pointers_need_no_alignment(rows, channels, offset):
    """A misaligned tensor sends a C % 32 == 0 launch to the row layout; the bytes are the same."""
    x, addend, q_in, h, steps, want = _case(offset, rows, channels, True)
    for path in (LDS, GLOBAL):
        out, bits, L = S.sim_chain(x, q_in, steps, addend, h, path=path, offset=offset)
        assert L["flat"] == 0
        assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])


def test_a_bit_output_that_is_only_word_aligned_keeps_the_flat_layout():
    x, addend, q_in, h, steps, want = _case(9, 129, 32, False)
    for bits_offset in (1, 2, 3):
        out, bits, L = S.sim_chain(x, q_in, steps, path=LDS, bits_offset=bits_offset)
        assert L["flat"] == 1 and np.array_equal(out, want[0]) and np.array_equal(bits, want[1])


@pytest.mark.parametrize("rows,channels", [(129, 32), (300, 31), (257, 96)])
@pytest.mark.parametrize("path", [LDS, GLOBAL, ONE_ROW])
def test_either_output_alone(rows, channels, path):
    x, addend, q_in, h, steps, want = _case(77 + channels, rows, channels, True, per_channel=path != ONE_ROW)
    out, bits, _ = S.sim_chain(x, q_in, steps, addend, h, path=path, want_bits=False)
    assert bits is None and np.array_equal(out, want[0])
    out, bits, _ = S.sim_chain(x, q_in, steps, addend, h, path=path, want_out=False)
    assert out is None and np.array_equal(bits, want[1])


@pytest.mark.parametrize("rows,channels", [(129, 32), (256, 33), (260, 64)])
@pytest.mark.parametrize("where", ["in", "addend"])
def test_in_place(rows, channels, where):
    x, addend, q_in, h, steps, want = _case(31 + channels, rows, channels, True)
    for path in (LDS, GLOBAL):
        out, bits, _ = S.sim_chain(x, q_in, steps, addend, h, path=path, in_place=where)
        assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])


@pytest.mark.parametrize("rows,channels", [(129, 32), (260, 64), (300, 31), (257, 96)])
@pytest.mark.parametrize("path", [LDS, GLOBAL, ONE_ROW])
def test_a_grid_small_enough_that_waves_stride(rows, channels, path):
    """One or two blocks: every wave takes several iterations, and on the flat layout the chunk's place in its row advances by the
    modular step between them ((260, 64): 4 chunks per row against a stride of 1024 or 2048 chunks; (257, 96): 6 per row)."""
    x = np.random.default_rng(3).integers(-128, 128, (rows * 24, channels)).astype(np.int8)
    g = np.random.default_rng(4)
    q_in, steps = E.draw_chain(g, channels, 2, path != ONE_ROW, kinds=("prelu",))
    if path != ONE_ROW:
        steps[0] = ("prelu", g.integers(-128, 128, channels).astype(np.int8)) + steps[0][2:]
    want = E.chain(x, q_in, steps)
    for cap in (1, 2):
        out, bits, L = S.sim_chain(x, q_in, steps, path=path, cap=cap)
        tasks = (x.size // 16 + 255) // 256 if L["flat"] else x.shape[0] * ((channels + 63) // 64)
        assert tasks > 2 * cap * L["waves_per_block"] and L["blocks_run"] == cap
        assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])


def test_the_wide_block_of_a_large_table():
    """Above 16 KiB of table in LDS a block has 16 waves: C = 96 is 24 960 bytes."""
    x, addend, q_in, h, steps, want = _case(5, 257, 96, True)
    out, bits, L = S.sim_chain(x, q_in, steps, addend, h, path=LDS, cap=1)
    assert L["waves_per_block"] == 16 and L["lds_bytes"] == 96 * 260
    assert np.array_equal(out, want[0]) and np.array_equal(bits, want[1])
