"""The real kernel bodies of csrc/lce_kernels_head_i8.h on the CPU (tests/hostsim_head_i8: 256 lanes of a block as fibers, the int8
matrix instruction emulated as the exact integer dot product under the row / column and C/D maps the kernel assumes) against
tests/head_i8_ref.py, byte for byte, on exact-size buffers: the FULLY_CONNECTED grid over batch, K and N with both load paths (16
bytes and bytes, by K and by the operands' alignment) and the tails, the map case, the accumulator's extremes, a capped grid that
makes the kernel stride; and the MEAN, SOFTMAX and QUANTIZE / DEQUANTIZE kernels.  What a simulation cannot decide -- that the
instruction HAS those maps -- is the GPU suite's (tests/test_gpu_head_i8.py)."""
import numpy as np
import pytest

import head_i8_cases as K
import head_i8_ref as H
from hostsim_head_i8_lib import OUT_MARK, sim_dequantize, sim_fc, sim_mean, sim_quantize, sim_softmax

# (the simulation runs a lane per fiber: N = 1000 at K = 512 is left to the device, the other corners are kept)
SIM_GRID = [c for c in K.FC_GRID if c[1] * c[2] <= 33000] + [(33, 512, 33), (17, 256, 40)]


def test_the_grid_on_both_load_paths_gives_the_reference_bytes():
    n, vecs = K.run_fc_grid(lambda *a: sim_fc(*a), SIM_GRID)
    assert n == len(SIM_GRID) >= 14 and 4 <= vecs < n


def test_one_byte_offsets_force_the_byte_path_with_k_a_multiple_of_16():
    x, w, bias, sw, q_in, q_out = K.fc_operands(17, 64, 33, 5)
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out)
    for offset, vec in ((0, True), (1, False), (15, False)):
        out, took = sim_fc(x, w, bias, sw, q_in, q_out, offset=offset)
        assert took == vec and np.array_equal(out, want), offset


def test_the_map_case():
    x, w, bias, sw, q_in, q_out = K.map_case()
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out)
    assert np.unique(want).size > 100 and not np.array_equal(want[:33, :33], want[:33, :33].T)
    out, _ = sim_fc(x, w, bias, sw, q_in, q_out)
    assert np.array_equal(out, want)


def test_the_accumulators_extremes():
    x, w, bias, sw, q_in, q_out = K.extremes_case()
    want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out)
    assert len(set(want[0].tolist())) >= 3
    out, vec = sim_fc(x, w, bias, sw, q_in, q_out)
    assert vec and np.array_equal(out, want)


def test_more_tiles_than_one_pass_of_a_capped_grid():
    """One block of four waves for 3 x 5 = 15 tiles: every wave strides."""
    x, w, bias, sw, q_in, q_out = K.fc_operands(33, 70, 70, 9)
    out, _ = sim_fc(x, w, bias, sw, q_in, q_out, cap=1)
    assert np.array_equal(out, H.fully_connected_i8(x, w, bias, sw, q_in, q_out))


@pytest.mark.parametrize("case", range(len(K.MEAN_SETS)))
def test_the_mean_kernel(case):
    h, w, c, q_in, q_out = K.MEAN_SETS[case]
    x = K.mean_input(h, w, c, 3, case)
    assert np.array_equal(sim_mean(x, q_in, q_out, cap=2), H.mean_i8(x, q_in, q_out))


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 7), (5, 63), (3, 64), (3, 65), (9, 129), (3, 1000)])
def test_the_softmax_kernel(rows, cols):
    q = K.softmax_input(rows, cols, rows + cols)
    for scale, beta in ((0.05, 1.0), (0.2, 0.5)):
        assert np.array_equal(sim_softmax(q, scale, beta, cap=1), H.softmax_i8(q, scale, beta))


def test_the_boundary_kernels():
    g = np.random.default_rng(4)
    x = (g.standard_normal(1500) * 3).astype(np.float32)
    x[:6] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30]
    q = g.integers(-128, 128, 1500).astype(np.int8)
    for scale, zp in ((0.05, -4), (0.0157, -128), (1.0, 127)):
        got = sim_quantize(x, scale, zp, cap=2)
        assert np.array_equal(got, H.quantize(x, scale, zp)) and got[0] == zp
        assert np.array_equal(sim_dequantize(q, scale, zp, cap=2).view(np.uint32), H.dequantize(q, scale, zp).view(np.uint32))
    assert OUT_MARK == 0x5A
