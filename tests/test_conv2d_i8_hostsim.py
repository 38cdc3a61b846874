"""The real kernel body of csrc/lce_kernels_conv2d_i8.h on the CPU (tests/hostsim_conv2d_i8: 256 lanes of a block as fibers, the
int8 matrix instruction emulated as the exact integer dot product under the row / column and C/D maps the kernel assumes) against
tests/conv2d_i8_ref.py, byte for byte: the known answers worked by hand, the grid over K = fh fw Cin, images, strides, paddings
and output channels with rotating bias, activation, output combination, input zero point and scale kind, both load paths (16
bytes and bytes, by the operands' alignment), and more tiles than one pass of a capped grid.  What a simulation cannot decide --
that the instruction HAS those maps -- is the GPU suite's (tests/test_gpu_conv2d_i8.py)."""
import numpy as np
import pytest

import conv2d_i8_ref as R
from conv2d_i8_cases import GRID, KNOWN, REQUANT_KNOWN, operands, run_grid
from hostsim_conv2d_i8_lib import requantize, sim


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name):
    k = KNOWN[name]
    out, bits, _ = sim(k["x"], k["w"], k["bias"], k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], k["act"])
    assert np.array_equal(out, k["want"]) and np.array_equal(bits, R.bitpack(k["want"], k["q_out"][1])), (out, k["want"])


def test_the_requantization_of_the_epilogue_gives_the_known_answers():
    acc, m, e, want = (np.array(c, np.int64) for c in zip(*REQUANT_KNOWN))
    assert np.array_equal(requantize(acc, m, e), want)


@pytest.mark.parametrize("filt,cin", GRID)
def test_the_kernel_body_gives_the_reference_bytes(filt, cin):
    n, vecs = run_grid(sim, filt, cin)
    assert n >= 9 and (vecs > 0) == (cin % 16 == 0)


def test_more_tiles_than_one_pass_of_a_capped_grid():
    """Two blocks per grid row: 2 x 20 x 19 output pixels are 6 tiles, the last with 120 of its 128 rows, and tiles span the two
    images; 160 channels are two grid rows."""
    x, w, bias, sw, q_in, q_out = operands((2, 40, 37, 3), (3, 3), 160, 5, zi=-7)
    assert 2 * 20 * 19 == 5 * 128 + 120
    want = R.conv2d_i8(x, w, bias, sw, q_in, q_out, (2, 2), R.SAME, R.RELU)
    out, bits, _ = sim(x, w, bias, sw, q_in, q_out, 2, R.SAME, R.RELU, cap=2)
    assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, q_out[1]))
