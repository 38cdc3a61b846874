"""The real kernel bodies of csrc/lce_kernels_depthwise_i8.h on the CPU (tests/hostsim_depthwise_i8: 256 lanes of a block as fibers)
against tests/depthwise_i8_ref.py, byte for byte: the known answers worked by hand and the grid over filters, images, strides,
paddings, channels and depth multipliers with rotating bias, activation, output combination, input zero point, scale kind and
placement -- through the path the entry's rule picks (asserted) and, where that is the 16-byte path, through the row path too --
and more chunks and segments than one pass of a capped grid."""
import numpy as np
import pytest

import depthwise_i8_ref as R
from depthwise_i8_cases import GRID, KNOWN, operands, run_grid
from hostsim_depthwise_i8_lib import sim


@pytest.mark.parametrize("path", (None, 0))
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_known_answers(name, path):
    k = KNOWN[name]
    out, bits, _ = sim(k["x"], k["w"], k["bias"], k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], k["m"], k["act"], path=path)
    assert np.array_equal(out, k["want"]) and np.array_equal(bits, R.bitpack(k["want"], k["q_out"][1])), (out, k["want"])


@pytest.mark.parametrize("path", (None, 0))
def test_the_known_corner_on_sixteen_byte_chunks(path):
    """The hand-worked corner pixel (4 taps inside, 5 skipped) repeated over 32 channels, so that the 16-byte path runs it too."""
    k = KNOWN["corner_same_pad"]
    x, w, want = (np.repeat(k[n], 32, axis=3) for n in ("x", "w", "want"))
    out, bits, vec = sim(x, w, None, k["sw"], k["q_in"], k["q_out"], k["stride"], k["padding"], 1, k["act"], path=path)
    assert vec == (path is None)
    assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, k["q_out"][1]))


@pytest.mark.parametrize("filt,cin,m", GRID)
def test_the_kernel_bodies_give_the_reference_bytes(filt, cin, m):
    n, vecs = run_grid(sim, filt, cin, m)
    assert n >= 9 and (vecs > 0) == (m == 1 and cin % 16 == 0)


@pytest.mark.parametrize("path", (None, 0))
def test_more_work_than_one_pass_of_a_capped_grid(path):
    """Two blocks: 2 x 10 x 9 output pixels of 6 chunks are 1080 chunks = 17 wave tasks of 64 (the last with 56), and 2 x 180
    segments of the row path, for 8 waves; tasks span the two images and the grid stride is no multiple of a pixel's chunks."""
    x, w, bias, sw, q_in, q_out = operands((2, 20, 17, 96), (3, 3), 1, 5, zi=-7, act=R.RELU, stride=(2, 2))
    want = R.depthwise_i8(x, w, bias, sw, q_in, q_out, (2, 2), R.SAME, 1, R.RELU)
    assert want.shape == (2, 10, 9, 96)
    out, bits, vec = sim(x, w, bias, sw, q_in, q_out, 2, R.SAME, 1, R.RELU, path=path, cap=2)
    assert vec == (path is None)
    assert np.array_equal(out, want) and np.array_equal(bits, R.bitpack(want, q_out[1]))
