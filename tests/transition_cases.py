"""The cases the suites of lce_hip_pool_depthwise_f32 / lce_hip_pool_depthwise_i8 share (tests/test_transition_hostsim.py,
tests/test_gpu_transition.py): QuickNet's geometry (pool 2x2 / 1 SAME, depthwise 3x3 / 2 SAME) on shapes with odd extents, clipped
windows and ragged channels, and a grid of general geometries for the row path; each run through a `run` the suite supplies (the
host simulation of the kernels, or the device) and compared BYTE FOR BYTE with tests/transition_ref.py, the composition of the two
entries' references.  Operands are seeded; the int8 bias and filter scales are calibrated on the reference's exact sums, as
tests/depthwise_i8_cases.py calibrates them -- never on the code under test."""
import numpy as np

import depthwise_i8_ref as DI
import transition_ref as R

OUT_MARK_F32, OUT_MARK_I8, BITS_MARK = np.float32(-12345.5), np.int8(0x5B), np.int32(0x5A5A5A5A)

QUICKNET = dict(pool=dict(filter=(2, 2), stride=(1, 1), padding=R.SAME), filt=(3, 3), stride=(2, 2), padding=R.SAME)
POOLS = {"3x3s2same": dict(filter=(3, 3), stride=(2, 2), padding=R.SAME), "2x2s2valid": dict(filter=(2, 2), stride=(2, 2), padding=R.VALID)}
DEPTHWISE = {"3x3s1": ((3, 3), (1, 1)), "5x5s2": ((5, 5), (2, 2)), "1x1s1": ((1, 1), (1, 1))}


def case(shape, pool, filt, stride, padding, m=1, act=R.NONE, pool_act=R.NONE, bias=True, seed=0):
    return dict(shape=tuple(shape), pool=dict(pool, activation=pool_act), filt=tuple(filt), stride=tuple(stride), padding=padding, m=m, act=act,
                bias=bias, seed=seed)


def quicknet(shape, **kw):
    return case(shape, **QUICKNET, **kw)


# name -> case.  `vec`: the 16-byte path takes it (aligned operands, value output alone or channels % 32 == 0).
F32 = {
    "quicknet_2x7x9x32": quicknet((2, 7, 9, 32), seed=1),                      # odd extents: the blur pads 1 in front, the pool's last row / column clip
    "quicknet_1x8x8x64": quicknet((1, 8, 8, 64), act=R.RELU, bias=False, seed=2),
    "quicknet_3x5x6x33": quicknet((3, 5, 6, 33), seed=3),                      # ragged: rows only
    "quicknet_1x1x1x4": quicknet((1, 1, 1, 4), seed=4),                        # every window clipped
    "quicknet_1x2x3x8": quicknet((1, 2, 3, 8), bias=False, seed=5),
    "quicknet_relu6_pool": quicknet((2, 6, 5, 32), pool_act=R.RELU6, act=R.RELU_N1_TO_1, seed=6),
    "pool1x2_dw2x3_valid": case((2, 6, 7, 36), dict(filter=(1, 2), stride=(1, 1), padding=R.VALID), (2, 3), (1, 2), R.VALID, seed=7),
}
I8 = {
    "quicknet_2x7x9x32": quicknet((2, 7, 9, 32), seed=11),
    "quicknet_1x5x6x48": quicknet((1, 5, 6, 48), act=R.RELU, seed=12),         # 48 channels: the 16-byte path without bits only
    "quicknet_relu6_pool": quicknet((2, 6, 5, 32), pool_act=R.RELU6, act=R.RELU6, bias=False, seed=13),
    "quicknet_1x2x3x17": quicknet((1, 2, 3, 17), seed=14),                     # ragged, every window clipped
}
# the general geometries of the row path: both pools x the three depthwise windows, and a depth multiplier of 2
for _p, _pool in POOLS.items():
    for _d, (_f, _s) in DEPTHWISE.items():
        _k = len(F32)
        F32["%s_%s" % (_p, _d)] = case((2, 9, 8, 5), _pool, _f, _s, R.SAME, m=1 + _k % 2, act=(R.NONE, R.RELU6)[_k % 2], bias=_k % 3 != 0, seed=20 + _k)
        I8["%s_%s" % (_p, _d)] = case((2, 9, 8, 5), _pool, _f, _s, R.SAME, m=1 + (_k + 1) % 2, act=(R.RELU, R.NONE)[_k % 2], bias=_k % 3 != 1, seed=40 + _k)
F32["quicknet_multiplier_2"] = quicknet((1, 6, 6, 16), m=2, seed=30)
I8["quicknet_multiplier_2"] = quicknet((1, 6, 6, 16), m=2, seed=31)


def operands_f32(c):
    """(x, w, bias or None): values around zero wide enough that a RELU6 pool clamps on both sides and both bit values occur."""
    g = np.random.default_rng(c["seed"])
    cout = c["shape"][3] * c["m"]
    x = (g.standard_normal(c["shape"]) * 4.0).astype(np.float32)
    w = g.standard_normal((1,) + c["filt"] + (cout,)).astype(np.float32)
    bias = g.standard_normal(cout).astype(np.float32) if c["bias"] else None
    return x, w, bias


def want_f32(c, x, w, bias):
    return R.pool_depthwise(x, c["pool"], w, bias, c["stride"], c["padding"], c["m"], c["act"])


def operands_i8(c):
    """(x, pool with its quantization, w, bias or None, filter scales, q_out).  The pooled tensor of the REFERENCE calibrates bias and
    scales: a channel's exact sums are centred (one sd up for an activation with a lower bound at the zero point) and an sd is
    mapped to 20 .. 60 output steps."""
    g = np.random.default_rng(c["seed"])
    cout = c["shape"][3] * c["m"]
    zi = int((0, -128, 127, 5, -3)[c["seed"] % 5])
    pool = dict(c["pool"], scale=0.02 if c["pool"]["activation"] == R.NONE else 0.05, zero_point=zi)
    x = g.integers(-128, 128, c["shape"], dtype=np.int64).astype(np.int8)
    w = g.integers(-128, 128, (1,) + c["filt"] + (cout,), dtype=np.int64).astype(np.int8)
    w[w == 0] = 1
    acc = DI.accumulate(R.pooled(x, pool), w, zi, c["stride"], c["padding"], c["m"]).reshape(-1, cout).astype(np.float64)
    mean, sd = acc.mean(0), np.maximum(acc.std(0), 1.0)
    if acc.shape[0] == 1:
        mean, sd = np.full(cout, acc.mean()), np.full(cout, max(acc.std(), 1.0))
    centre = 0.0 if c["act"] in (R.NONE, R.RELU_N1_TO_1) else 1.0
    shift = np.rint(-mean + sd * (centre + g.uniform(-0.5, 0.5, cout)))
    bias = shift.astype(np.int32) if c["bias"] else None
    if bias is None:
        sd = np.maximum(np.sqrt(sd ** 2 + mean ** 2), 1.0)            # (without a bias the sums keep their mean: scale to their RMS)
    so = {R.NONE: 0.05, R.RELU: 0.05, R.RELU6: 0.03, R.RELU_N1_TO_1: 0.01}[c["act"]]
    sw = (g.uniform(0.5, 1.5, cout) * 40.0 / sd * so / pool["scale"]).astype(np.float32)
    return x, pool, w, bias, sw, (so, int(g.integers(-20, 21)))


def want_i8(c, x, pool, w, bias, sw, q_out):
    return R.pool_depthwise_i8(x, pool, w, bias, sw, q_out, c["stride"], c["padding"], c["m"], c["act"])


def vec_geometry(c):
    p = c["pool"]
    return p["stride"] == (1, 1) and max(p["filter"]) <= 2 and max(c["filt"]) <= 3


def expect_vec(c, chunk, want_bits, offset=0):
    """The entries' rule for operands that are 16-byte aligned but for `offset`: `chunk` is 4 (float) or 16 (int8) channels."""
    cout = c["shape"][3] * c["m"]
    return c["m"] == 1 and cout % chunk == 0 and offset == 0 and vec_geometry(c) and (not want_bits or cout % 32 == 0)


OUTPUTS = (dict(want_out=True, want_bits=True), dict(want_out=True, want_bits=False), dict(want_out=False, want_bits=True))


def check_f32(run, c, outputs=OUTPUTS, paths=(None, 0), **kw):
    """Every output combination on every path against the composition; which path ran is asserted.  Returns the launches that took
    the 16-byte path."""
    x, w, bias = operands_f32(c)
    want = want_f32(c, x, w, bias)
    bits_want = R.bitpack_f32(want)
    if want.size >= 64:                                                # no constant passes; without a lower bound at 0 both bit values occur
        assert np.unique(want).size >= 8, c
        assert c["act"] in (R.RELU, R.RELU6) or 0 < int((want < 0).sum()) < want.size, c
    vecs = 0
    for o in outputs:
        for path in paths:
            out, bits, vec = run(x, c["pool"], w, bias, c["stride"], c["padding"], c["m"], c["act"], path=path, **o, **kw)
            assert vec == (path is None and expect_vec(c, 4, o["want_bits"])), (c, o, path)
            vecs += vec
            if o["want_out"]:
                assert out.dtype == np.float32 and out.shape == want.shape and np.array_equal(out.view(np.int32), want.view(np.int32)), (c, o, path)
            else:
                assert out is None or (out == OUT_MARK_F32).all(), (c, o, path)
            if o["want_bits"]:
                assert np.array_equal(bits, bits_want), (c, o, path)
            else:
                assert bits is None or (bits == BITS_MARK).all(), (c, o, path)
    return vecs


def check_i8(run, c, outputs=OUTPUTS, paths=(None, 0), **kw):
    x, pool, w, bias, sw, q_out = operands_i8(c)
    want = want_i8(c, x, pool, w, bias, sw, q_out)
    bits_want = DI.bitpack(want, q_out[1])
    if want.size >= 64:
        assert np.unique(want).size >= 8, (c, np.unique(want).size)
        assert c["act"] in (R.RELU, R.RELU6) or 0 < int((want < q_out[1]).sum()) < want.size, c
    vecs = 0
    for o in outputs:
        for path in paths:
            out, bits, vec = run(x, pool, w, bias, sw, q_out, c["stride"], c["padding"], c["m"], c["act"], path=path, **o, **kw)
            assert vec == (path is None and expect_vec(c, 16, o["want_bits"])), (c, o, path)
            vecs += vec
            if o["want_out"]:
                assert out.dtype == np.int8 and out.shape == want.shape and np.array_equal(out, want), (c, o, path)
            else:
                assert out is None or (out == OUT_MARK_I8).all(), (c, o, path)
            if o["want_bits"]:
                assert np.array_equal(bits, bits_want), (c, o, path)
            else:
                assert bits is None or (bits == BITS_MARK).all(), (c, o, path)
    return vecs
