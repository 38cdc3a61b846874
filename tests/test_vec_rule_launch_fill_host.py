"""The launch fills and path rules the entries of csrc/lce_hip_api.hip share with the host simulations (pool_window_fill,
pool_set_stride, window_vec_rule of lce_kernels_pool.h; <family>_fill, <family>_vec_rule and <family>_grid of the matrix kernels'
headers), on the smallest shapes at which they can go wrong: the simulations fill their launches with the product's own functions,
so a wrong padding, per_pixel, grid step or path rule fails here, on the CPU.  Every output is compared byte for byte with the
references the families' own suites use; the path a simulation took is compared with the entry's `_path` answer on the same
addresses."""
import ctypes as C
import importlib

import numpy as np
import pytest

import binary_dense_ref as BR
import conv2d_i8_cases as CK
import conv2d_i8_ref as CQ
import conv2d_ref as CF
import depthwise_i8_cases as DK
import depthwise_i8_ref as DI
import head_i8_cases as HK
import head_i8_ref as HQ
import head_ref as HR
import hostsim_binary_dense_lib as BS
import hostsim_conv2d_i8_lib as CS
import hostsim_depthwise_i8_lib as DS
import hostsim_head_i8_lib as HS
import transition_cases as TC
import transition_ref as TR
from hostsim_transition_lib import sim_f32, sim_i8
from test_binary_dense_host import _operands as bfc_operands
from test_conv2d_hostsim import sim as conv2d_sim
from test_conv2d_sections_host import grid_operands
from test_head_host import fc_operands, sim_fc
from test_transition_host import dw8_desc, dw_desc, pool_desc

amd = importlib.import_module("compute-engine_amd")

# ---- the padding split: (input, filter, stride) per axis.  SAME with an odd total pad (1: nothing in front), SAME with an even
# total (2: 1 in front), VALID.  Height and width take different rows, so that a swap of the two shows.
ODD_A, ODD_B, EVEN, VALID_A, VALID_B = (5, 2, 2), (4, 3, 2), (5, 3, 1), (5, 3, 2), (4, 2, 1)
PADDINGS = {"odd_odd": (ODD_A, ODD_B, DI.SAME), "odd_even": (ODD_B, EVEN, DI.SAME), "even_odd": (EVEN, ODD_A, DI.SAME),
            "valid": (VALID_A, VALID_B, DI.VALID)}


def test_the_padding_cases_are_the_stated_ones():
    """NumPy's side of the comparison, worked by hand: total pad 1 -> 0 in front, total 2 -> 1, VALID -> 0."""
    assert [DI.out_and_pad(i, f, s, DI.SAME) for i, f, s in (ODD_A, ODD_B, EVEN)] == [(3, 0), (2, 0), (5, 1)]
    assert [DI.out_and_pad(i, f, s, DI.VALID) for i, f, s in (VALID_A, VALID_B)] == [(2, 0), (3, 0)]


@pytest.mark.parametrize("name", sorted(PADDINGS))
@pytest.mark.parametrize("cin", (32, 5))
def test_depthwise_i8_pads_as_numpy_does(name, cin):
    """The simulation returns -1 (the loader asserts) unless pool_window_fill's ph, pw are tests/depthwise_i8_ref.py's."""
    (ih, fh, sh), (iw, fw, sw_), padding = PADDINGS[name]
    x, w, bias, sw, q_in, q_out = DK.operands((2, ih, iw, cin), (fh, fw), 1, 11, zi=3, stride=(sh, sw_), padding=padding)
    want = DI.depthwise_i8(x, w, bias, sw, q_in, q_out, (sh, sw_), padding, 1, DI.NONE)
    for path in (None, 0):
        out, bits, vec = DS.sim(x, w, bias, sw, q_in, q_out, (sh, sw_), padding, 1, DI.NONE, path=path)
        assert vec == (path is None and cin == 32)
        assert np.array_equal(out, want) and np.array_equal(bits, DI.bitpack(want, q_out[1]))


@pytest.mark.parametrize("name", sorted(PADDINGS))
@pytest.mark.parametrize("pool", ("quicknet", "3x3s2same"))
def test_the_transitions_pad_as_numpy_does(name, pool):
    """Both windows: the pool in front (2x2 / 1 SAME: total 1, 0 in front; 3x3 / 2 SAME on 9 x 7: totals 2 and 2) and the depthwise
    window on the pooled map.  The simulations return -1 (the loader asserts) unless all four paddings are tests/pool_ref.py's."""
    (ih, fh, sh), (iw, fw, sw_), padding = PADDINGS[name]
    p = TC.QUICKNET["pool"] if pool == "quicknet" else TC.POOLS[pool]
    shape = (2, ih, iw, 32) if pool == "quicknet" else (2, 2 * ih - 1, 2 * iw - 1, 32)      # (3x3 / 2 SAME pools 2 n - 1 to n)
    c = TC.case(shape, p, (fh, fw), (sh, sw_), padding, seed=70)
    assert TR.pooled(np.zeros(shape, np.float32), c["pool"]).shape[1:3] == (ih, iw)
    TC.check_f32(sim_f32, c)
    TC.check_i8(sim_i8, c)


# ---- a grid step that is no whole number of pixels: cap = 3 blocks of 4 waves of 64 chunks = 768 chunks a step; 5 chunks a pixel
# leave step_chunks = 3; a 1 x 13 x 13 output has 845 chunks, more than one step.  With bits the path needs C % 32 == 0: 96 channels
# (6 or 24 chunks a pixel: a whole number of pixels a step) and 160 (10 or 40 chunks a pixel: step_chunks = 8 with bits).
@pytest.mark.parametrize("cin,want_bits", ((80, False), (96, True), (160, True)))
def test_depthwise_i8_steps_a_grid_that_is_no_whole_number_of_pixels(cin, want_bits):
    x, w, bias, sw, q_in, q_out = DK.operands((1, 13, 13, cin), (3, 3), 1, 21, zi=-5)
    want = DI.depthwise_i8(x, w, bias, sw, q_in, q_out, (1, 1), DI.SAME, 1, DI.NONE)
    assert want.shape == (1, 13, 13, cin) and 169 * (cin // 16) > 768 and 768 % (cin // 16) == {80: 3, 96: 0, 160: 8}[cin]
    out, bits, vec = DS.sim(x, w, bias, sw, q_in, q_out, 1, DI.SAME, 1, DI.NONE, want_bits=want_bits, cap=3)
    assert vec and np.array_equal(out, want)
    assert not want_bits or np.array_equal(bits, DI.bitpack(want, q_out[1]))


@pytest.mark.parametrize("kind,cin,want_bits", (("f32", 20, False), ("i8", 80, False), ("f32", 96, True), ("i8", 96, True), ("f32", 160, True),
                                                ("i8", 160, True)))
def test_the_transitions_step_a_grid_that_is_no_whole_number_of_pixels(kind, cin, want_bits):
    c = TC.case((1, 13, 13, cin), TC.QUICKNET["pool"], (3, 3), (1, 1), TR.SAME, seed=80)
    per_pixel = cin // (4 if kind == "f32" else 16)
    assert 169 * per_pixel > 768 and 768 % per_pixel == {96: 0, 160: 8}.get(cin, 3)
    outputs = (dict(want_out=True, want_bits=want_bits),)
    vecs = (TC.check_f32 if kind == "f32" else TC.check_i8)(sim_f32 if kind == "f32" else sim_i8, c, outputs=outputs, paths=(None,), cap=3)
    assert vecs == 1


# ---- the path rule at its edges: what the simulation took (window_vec_rule, for the transitions && transition_vec_geometry) is the
# entry's `_path` answer on the same descriptor and addresses, and the documented rule.
def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _entry_path(name, descs, seen):
    took = C.c_int32(-1)
    rc = getattr(amd.lib(), name)(*[C.byref(d) for d in descs], *[_ptr(seen[k]) for k in ("x", "w", "third", "out", "bits")], C.byref(took))
    assert rc == amd.OK, amd.lib().lce_hip_last_error().decode()
    return took.value


# (channels, depth multiplier, bits, the offsets of input, filter, table / bias and output, the documented answer)
EDGES = {"aligned": (32, 1, True, (0, 0, 0, 0), 1), "no_bits": (48, 1, False, (0, 0, 0, 0), 1), "bits_on_48": (48, 1, True, (0, 0, 0, 0), 0),
         "multiplier_2": (16, 2, True, (0, 0, 0, 0), 0), "input_off": (32, 1, True, (4, 0, 0, 0), 0), "filter_off": (32, 1, True, (0, 4, 0, 0), 0),
         "third_off": (32, 1, True, (0, 0, 4, 0), 0), "output_off": (32, 1, True, (0, 0, 0, 4), 0)}


@pytest.mark.parametrize("name", sorted(EDGES) + ["one_short"])
def test_the_depthwise_i8_rule_is_the_entrys(name):
    cin, m, want_bits, offsets, rule = EDGES.get(name, (47, 1, False, (0, 0, 0, 0), 0))       # 47: one element short of 3 chunks
    x, w, bias, sw, q_in, q_out = DK.operands((1, 4, 4, cin), (3, 3), m, 31)
    seen = {}
    _, _, vec = DS.sim(x, w, bias, sw, q_in, q_out, 1, DI.SAME, m, DI.NONE, want_bits=want_bits, offsets=offsets, seen=seen)
    d = amd.DepthwiseI8Desc(1, 4, 4, cin, m, 3, 3, 1, 1, amd.PADDING_SAME, amd.ACT_NONE, q_in[0], q_in[1], q_out[0], q_out[1])
    assert int(vec) == rule == _entry_path("lce_hip_depthwise_conv2d_i8_path", (d,), seen)


GEOMETRIES = {"pool_stride_2": (dict(filter=(2, 2), stride=(2, 2), padding=TR.SAME), (3, 3)),
              "pool_3x3": (dict(filter=(3, 3), stride=(1, 1), padding=TR.SAME), (3, 3)), "depthwise_5x5": (TC.QUICKNET["pool"], (5, 5))}


@pytest.mark.parametrize("kind", ("f32", "i8"))
@pytest.mark.parametrize("name", sorted(EDGES) + ["one_short"] + sorted(GEOMETRIES))
def test_the_transitions_rule_is_the_entrys(name, kind):
    chunk = 4 if kind == "f32" else 16
    pool, filt = GEOMETRIES.get(name, (TC.QUICKNET["pool"], (3, 3)))
    cin, m, want_bits, offsets, rule = EDGES.get(name, (3 * chunk - 1, 1, False, (0, 0, 0, 0), 0) if name == "one_short" else (32, 1, True, (0, 0, 0, 0), 0))
    c = TC.case((1, 6, 6, cin), pool, filt, (2, 2), TR.SAME, m=m, seed=90)
    seen = {}
    if kind == "f32":
        x, w, bias = TC.operands_f32(c)
        _, _, vec = sim_f32(x, c["pool"], w, bias, c["stride"], c["padding"], m, c["act"], want_bits=want_bits, offsets=offsets, seen=seen)
        descs = (pool_desc(amd.F32, shape=c["shape"], filt=pool["filter"], stride=pool["stride"]),
                 dw_desc((1,) + TR.pooled(x, c["pool"]).shape[1:3] + (cin,), m, filt))
    else:
        x, p, w, bias, sw, q_out = TC.operands_i8(c)
        _, _, vec = sim_i8(x, p, w, bias, sw, q_out, c["stride"], c["padding"], m, c["act"], want_bits=want_bits, offsets=offsets, seen=seen)
        descs = (pool_desc(amd.I8, shape=c["shape"], filt=pool["filter"], stride=pool["stride"], scale=p["scale"], zp=p["zero_point"]),
                 dw8_desc((1,) + TR.pooled(x, p).shape[1:3] + (cin,), m, filt, q_in=(p["scale"], p["zero_point"]), q_out=q_out))
    assert int(vec) == rule == _entry_path("lce_hip_pool_depthwise_%s_path" % kind, descs, seen)


# ---- the matrix kernels: K (Kw for the binary layer) one below and at a multiple of the load width -- the documented rule, as
# these entries have no `_path` form --, M and N one above a multiple of the tile so that `tiles` rounds up, and cap = 1: a single
# block strides over every tile.
@pytest.mark.parametrize("k,vec", ((63, False), (64, True)))
def test_fully_connected_f32_fill_rule_and_grid(k, vec):
    x, w, bias = fc_operands(17, k, 33)
    out, took = sim_fc(x, w, bias, HR.RELU, cap=1)
    want = HR.fully_connected(x, w, bias, HR.RELU)
    assert took == vec and np.array_equal(out.view(np.int32), want.view(np.int32))
    assert not sim_fc(x, w, bias, HR.RELU, cap=1, offset=1)[1]


@pytest.mark.parametrize("k,vec", ((63, False), (64, True)))
def test_fully_connected_i8_fill_rule_and_grid(k, vec):
    x, w, bias, sw, q_in, q_out = HK.fc_operands(17, k, 33, 3)
    out, took = HS.sim_fc(x, w, bias, sw, q_in, q_out, cap=1)
    assert took == vec and np.array_equal(out, HQ.fully_connected_i8(x, w, bias, sw, q_in, q_out))
    assert not HS.sim_fc(x, w, bias, sw, q_in, q_out, cap=1, offset=4)[1]


@pytest.mark.parametrize("k,vec", ((96, False), (97, True), (128, True)))
def test_binary_fully_connected_fill_rule_and_grid(k, vec):
    """Kw = ceil(K / 32): 96 inputs are 3 words, 97 and 128 are 4."""
    a, w, s, bias, _ = bfc_operands(33, k, 65, 7)
    v, bits, took = BS.sim(a, w, s, bias, k, BR.NONE, cap=1)
    want_v, want_bits = BR.binary_fully_connected(a, w, s, bias, k, BR.NONE)
    assert took == vec and np.array_equal(v.view(np.int32), want_v.view(np.int32)) and np.array_equal(bits, want_bits)
    assert not BS.sim(a, w, s, bias, k, BR.NONE, cap=1, offset=4)[2]


@pytest.mark.parametrize("cin,vec", ((3, False), (4, True)))
def test_conv2d_f32_rule_and_grids(cin, vec):
    """A 1 x 5 x 45 image under 3x3 / 1 SAME: the interior (no tap clipped) is 3 x 43 = 129 pixels, one above a tile of 128, so
    mtiles = 2 and the single interior block of cap = 1 strides to a second tile that holds one pixel; the border's 96 pixels of 3
    segments (129 channels) are 288 wave tasks on one block; grid.y is 2."""
    h, wd, cout = 5, 45, 129
    interior, border_pixels = (h - 2) * (wd - 2), h * wd - (h - 2) * (wd - 2)
    assert interior == 129 and -(-interior // 128) == 2 and border_pixels * -(-cout // 64) == 288 and -(-cout // 128) == 2
    g = np.random.default_rng(cin)
    x = g.standard_normal((1, h, wd, cin)).astype(np.float32)
    w, bias = grid_operands((3, 3), cin, cout)
    out, bits, took, border = conv2d_sim(x, w, bias, 1, CF.SAME, CF.RELU, cap=1)
    want = CF.conv2d(x, w, bias, (1, 1), CF.SAME, CF.RELU)
    assert took == vec and border and np.array_equal(out.view(np.int32), want.view(np.int32))
    assert np.array_equal(bits, TR.bitpack_f32(want))
    assert not conv2d_sim(x, w, bias, 1, CF.SAME, CF.RELU, cap=1, offset=1)[2]


@pytest.mark.parametrize("cin,vec", ((15, False), (16, True)))
def test_conv2d_i8_rule_and_grid(cin, vec):
    """1 x 12 x 11 = 132 pixels, above a tile of 128: mtiles = 2 on the one block of cap = 1; 129 channels make grid.y 2."""
    x, w, bias, sw, q_in, q_out = CK.operands((1, 12, 11, cin), (3, 3), 129, 5, zi=-2)
    out, bits, took = CS.sim(x, w, bias, sw, q_in, q_out, 1, CQ.SAME, CQ.NONE, cap=1)
    want = CQ.conv2d_i8(x, w, bias, sw, q_in, q_out, (1, 1), CQ.SAME, CQ.NONE)
    assert want.shape == (1, 12, 11, 129) and took == vec
    assert np.array_equal(out, want) and np.array_equal(bits, DI.bitpack(want, q_out[1]))
    assert not CS.sim(x, w, bias, sw, q_in, q_out, 1, CQ.SAME, CQ.NONE, cap=1, offset=4)[2]
