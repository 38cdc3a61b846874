"""The kernels of lce_hip_mul_int8 on the CPU (tests/hostsim_gate_i8: the real bodies of csrc/lce_kernels_mul_i8.h between guard
bytes, with the launch lce_hip_mul_int8_path reports) against the NumPy restatement (tests/gate_i8_ref.py): both layouts, both
operand kinds, with and without the ADD, every activation, every combination of outputs, in place, pointer offsets, and a grid small
enough that waves stride.  The shapes are the smallest at which a lane's image index can go wrong: rows_per_image 1 and 3 put
several images into one wave, and 48 and 80 channels give a row an odd number of 16-byte chunks."""
import itertools

import numpy as np
import pytest

import gate_i8_ref as G
import hostsim_gate_i8_lib as S
from hostsim_gate_i8_lib import amd
import int8_add_ref as ar

CHANNELS = [1, 31, 32, 33, 48, 64, 80, 100, 256]
RPI = [1, 3, 49]
BATCH = [1, 3]


def _case(seed, batch, rpi, channels, per_image, has_add, act=0, add_act=0):
    g = np.random.default_rng(seed)
    rows = batch * rpi
    q1, q2, qo = G.mul_draws(1, seed)[0]
    x = g.integers(-128, 128, (rows, channels)).astype(np.int8)
    x[0, :] = -128
    x[-1, :] = 127
    operand = g.integers(-128, 128, (batch if per_image else rows, channels)).astype(np.int8)
    addend = add = None
    if has_add:
        addend = g.integers(-128, 128, (rows, channels)).astype(np.int8)
        q_ad = (float(np.float32(qo[0] * g.uniform(0.5, 2.0))), int(g.integers(-128, 128)))
        q_sum = (float(np.float32((qo[0] + q_ad[0]) * g.uniform(0.6, 1.2))), int(g.integers(-60, 60)))
        add = (q_ad, q_sum, add_act)
        want = G.mul_add_q(x, operand, addend, q1, q2, qo, act, q_ad, q_sum, add_act, rpi if per_image else 0)
        zo = q_sum[1]
    else:
        want = G.mul_q(x, operand, q1, q2, qo, act, rpi if per_image else 0)
        zo = qo[1]
    kw = dict(act=act, rows_per_image=rpi if per_image else 0, addend=addend, add=add)
    return (x, operand, q1, q2, qo), kw, want, ar.bitpack(want, zo)


def _flat(channels, offset=0):
    return int(channels % 16 == 0 and offset == 0)


@pytest.mark.parametrize("channels", CHANNELS)
def test_every_shape_both_operand_kinds_with_and_without_the_add(channels):
    for batch, rpi, per_image, has_add in itertools.product(BATCH, RPI, (False, True), (False, True)):
        args, kw, want, want_bits = _case(channels * 100 + rpi * 7 + batch, batch, rpi, channels, per_image, has_add)
        out, bits, L = S.sim_mul(*args, **kw)
        assert L["flat"] == _flat(channels) and (L["add_variant"] >= 0) == has_add and L["mul_variant"] == 1
        assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (batch, rpi, per_image, has_add)


def test_every_add_variant_and_either_input_order():
    """The simulation runs the ADD variant lce_hip_mul_int8_path reports, on the kernel parameters and the input order it reports.
    An addend scale above the product's puts the addend first (product_first 0); equal scales are the SHIFT variant, unequal
    ones SPLIT; the LITERAL kernel is run on the same parameters (it is right for all).  Both layouts, both operand kinds."""
    seen = set()
    for ratio, channels, per_image in itertools.product((0.5, 1.0, 1.7), (33, 64), (False, True)):
        g = np.random.default_rng(int(ratio * 10) + channels)
        q1, q2, qo = G.mul_draws(1, channels)[0]
        x = g.integers(-128, 128, (9, channels)).astype(np.int8)
        operand = g.integers(-128, 128, (3 if per_image else 9, channels)).astype(np.int8)
        addend = g.integers(-128, 128, (9, channels)).astype(np.int8)
        q_ad, q_sum = (float(np.float32(qo[0] * ratio)), 11), (float(np.float32(qo[0] * (1 + ratio) * 0.8)), -7)
        want = G.mul_add_q(x, operand, addend, q1, q2, qo, 0, q_ad, q_sum, 1, 3 if per_image else 0)
        for literal_add in (False, True):
            out, bits, L = S.sim_mul(x, operand, q1, q2, qo, rows_per_image=3 if per_image else 0, addend=addend, add=(q_ad, q_sum, 1),
                                     literal_add=literal_add)
            assert np.array_equal(out, want) and np.array_equal(bits, ar.bitpack(want, -7)), (ratio, channels, per_image, literal_add)
        assert L["add_variant"] == amd.add_int8_params(qo, q_ad, q_sum, 1)["variant"]
        seen.add((L["add_variant"], L["product_first"]))
    assert {v for v, _ in seen} >= {1, 2} and {f for _, f in seen} == {0, 1}, seen


def test_each_activation_on_either_stage():
    for act, channels, per_image in itertools.product((0, 1, 2, 3), (33, 48, 64), (False, True)):
        args, kw, want, want_bits = _case(act + channels, 3, 3, channels, per_image, False, act=act)
        out, bits, _ = S.sim_mul(*args, **kw)
        assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (act, channels, per_image)
        args, kw, want, want_bits = _case(act + channels, 3, 3, channels, per_image, True, act=3 - act, add_act=act)
        out, bits, _ = S.sim_mul(*args, **kw)
        assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (act, channels, per_image)


def test_either_output_alone():
    for channels, has_add in itertools.product((1, 33, 48, 64, 100), (False, True)):
        args, kw, want, want_bits = _case(5 + channels, 3, 3, channels, True, has_add)
        out, bits, _ = S.sim_mul(*args, want_bits=False, **kw)
        assert bits is None and np.array_equal(out, want), (channels, has_add)
        out, bits, _ = S.sim_mul(*args, want_out=False, **kw)
        assert out is None and np.array_equal(bits, want_bits), (channels, has_add)


def test_in_place():
    for channels, where, per_image in itertools.product((31, 48, 64, 256), ("x", "addend"), (False, True)):
        args, kw, want, want_bits = _case(11 + channels, 3, 3, channels, per_image, True)
        out, bits, _ = S.sim_mul(*args, in_place=where, **kw)
        assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (channels, where, per_image)


def test_int8_pointers_need_no_alignment():
    """A misaligned tensor sends a C % 16 == 0 launch to the row layout; the bytes are the same."""
    for offset, channels, has_add in itertools.product((1, 5), (32, 48, 100), (False, True)):
        args, kw, want, want_bits = _case(offset + channels, 3, 3, channels, True, has_add)
        out, bits, L = S.sim_mul(*args, offset=offset, **kw)
        assert L["flat"] == 0, (offset, channels)
        assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (offset, channels, has_add)


def test_a_bit_output_that_is_only_word_aligned_keeps_its_layout():
    for channels, bits_offset in itertools.product((32, 48, 33), (1, 3)):
        args, kw, want, want_bits = _case(channels, 3, 3, channels, True, True)
        out, bits, L = S.sim_mul(*args, bits_offset=bits_offset, **kw)
        assert L["flat"] == _flat(channels) and np.array_equal(out, want) and np.array_equal(bits, want_bits), (channels, bits_offset)


@pytest.mark.parametrize("per_image", [False, True])
def test_a_grid_small_enough_that_waves_stride(per_image):
    """One or two blocks of four waves: every wave takes several iterations (a batch large enough for that)."""
    for channels, rpi in ((64, 49), (80, 49), (256, 3), (48, 1), (100, 49), (31, 3)):
        batch = {49: 24, 3: 400, 1: 2200}[rpi]
        args, kw, want, want_bits = _case(channels + rpi, batch, rpi, channels, per_image, True)
        for cap in (1, 2):
            out, bits, L = S.sim_mul(*args, cap=cap, **kw)
            rows = batch * rpi
            tasks = (rows * (channels // 16) + 255) // 256 if L["flat"] else rows * ((channels + 63) // 64)
            assert tasks > 2 * cap * L["waves_per_block"] and L["blocks_run"] == cap, (channels, rpi, cap)
            assert np.array_equal(out, want) and np.array_equal(bits, want_bits), (channels, rpi, cap)


@pytest.mark.parametrize("channels", [33, 64])
@pytest.mark.parametrize("scale_out,variant", [(0.08, 0), (0.3, 0), (0.6, 1)])
def test_the_literal_variant_where_the_fast_one_does_not_apply(channels, scale_out, variant):
    """A real multiplier of 1/2 and above (e >= 0) is outside the fast variant's precondition: 0.5 * 0.5 / 0.08 = 3.125 (e = 2) and
    0.25 / 0.3 = 0.83 (e = 0) run the literal formula, 0.25 / 0.6 = 0.42 (e = -1) the fast one.  The values keep |(x1 - z1)(x2 - z2)| <= 49, so
    that at 3.125 fewer than half of the products can reach a clamp bound."""
    g = np.random.default_rng(channels)
    q1, q2, qo = (0.5, 3), (0.5, -4), (scale_out, 5)
    x = g.integers(-3, 11, (147, channels)).astype(np.int8)
    gate = g.integers(-10, 4, (3, channels)).astype(np.int8)
    addend = g.integers(-128, 128, (147, channels)).astype(np.int8)
    add = ((0.4, 1), (0.9, -2), 0)
    out, bits, L = S.sim_mul(x, gate, q1, q2, qo, rows_per_image=49, addend=addend, add=add)
    assert L["mul_variant"] == variant
    want = G.mul_add_q(x, gate, addend, q1, q2, qo, 0, add[0], add[1], 0, 49)
    assert np.array_equal(out, want) and np.array_equal(bits, ar.bitpack(want, -2))
    assert np.mean((G.mul_q(x, gate, q1, q2, qo, 0, 49) == 127) | (G.mul_q(x, gate, q1, q2, qo, 0, 49) == -128)) < 0.5
