"""The cases the three suites of lce_hip_depthwise_conv2d_i8 share (tests/test_depthwise_i8_host.py,
tests/test_depthwise_i8_hostsim.py, tests/test_gpu_depthwise_i8.py): the known answers worked by hand, and the grid over filters,
images, strides, paddings, channels and depth multipliers, each run through a `run` the suite supplies (the reference itself, the
host simulation of the kernels, or the device) and compared byte for byte with tests/depthwise_i8_ref.py."""
import numpy as np

import conv2d_i8_cases as CC
import depthwise_i8_ref as R

OUT_MARK, BITS_MARK = CC.OUT_MARK, CC.BITS_MARK
ACTS = (R.NONE, R.RELU, R.RELU_N1_TO_1, R.RELU6)


def _i8(*v):
    return np.array(v, np.int8)


def _known():
    """name -> dict(x, w, bias, sw, q_in, q_out, stride, padding, m, act, want).  Every `want` is worked by hand; the conventions
    are those of tests/conv2d_i8_cases.py: 2^30 as a multiplier is 'times one half', SRDHM(a, 2^30) = a / 2 with a tie going UP
    (3 -> 2, -3 -> -1); RDivPOT(x, n) rounds x / 2^n to nearest, a tie AWAY from zero."""
    K = {}
    # A depthwise convolution on ONE channel is the convolution on one channel, and its filter [1, fh, fw, 1] has the bytes of the
    # convolution's [1, fh, fw, 1]: the answers worked there hold here -- the corner pixel under SAME with zi = 5 (4 taps inside, 5
    # in the padding, which are SKIPPED: read as x = 0 they would add (0 - 5) w), the requantization ties on both sides of zero,
    # e = 0 with a bias, e > 0, e = -31, and the four activations.
    for name, k in CC.KNOWN.items():
        if k["w"].shape[0] == 1 and k["w"].shape[3] == 1:
            K[name] = dict(k, m=1)
    # The same corner on TWO channels with different filters, so that a channel cannot read its neighbour's weights: channel 0 is
    # the case above (76, 66, 46, 36); channel 1 has x = 5 everywhere = zi, so every product is 0 whatever its filter: zo = -3.
    x = np.stack([_i8(10, 20, 30, 40), _i8(5, 5, 5, 5)], -1).reshape(1, 2, 2, 2)
    w = np.stack([_i8(*range(1, 10)), _i8(*range(-9, 0))], -1).reshape(1, 3, 3, 2)
    K["corner_two_channels"] = dict(x=x, w=w, bias=None, sw=0.5, q_in=(0.5, 5), q_out=(2.0, -3), stride=1, padding=R.SAME, m=1, act=R.NONE,
                                    want=np.stack([_i8(76, 66, 46, 36), _i8(-3, -3, -3, -3)], -1).reshape(1, 2, 2, 2))
    # zi = -128 and the extreme weights on four channels of one pixel, multiplier 2^-4 * 2^-4 = 2^-8: m = 2^30, e = -7.
    #   ch 0: (127 + 128) * 127 = 32385 -> SRDHM 16192.5, the tie goes up: 16193 -> / 128 = 126.51 -> 127
    #   ch 1: 255 * -128 = -32640 -> -16320 -> / 128 = -127.5, a tie, away from zero: -128
    #   ch 2: (-128 + 128) * 127 = 0 -> 0
    #   ch 3: 128 * -128 = -16384 -> -8192 -> exactly -64
    K["zi_minus_128"] = dict(x=_i8(127, 127, -128, 0).reshape(1, 1, 1, 4), w=_i8(127, -128, 127, -128).reshape(1, 1, 1, 4), bias=None,
                             sw=0.0625, q_in=(0.0625, -128), q_out=(1.0, 0), stride=1, padding=R.VALID, m=1, act=R.NONE,
                             want=_i8(127, -128, 0, -64).reshape(1, 1, 1, 4))
    # zi = 127, multiplier 2^-5 * 2^-5 = 2^-10: m = 2^30, e = -9, zo = 100.
    #   ch 0: -255 * 127 = -32385 -> SRDHM -16192.5, up: -16192 -> / 512 = -31.625 -> -32 -> 68
    #   ch 1: -255 * -128 = 32640 -> 16320 -> 31.875 -> 32 -> 132 -> clamped to 127
    #   ch 2: 0 * -128 = 0 -> 100
    #   ch 3: -127 * 1 = -127 -> -63.5, up: -63 -> / 512 = -0.12 -> 0 -> 100
    K["zi_127"] = dict(x=_i8(-128, -128, 127, 0).reshape(1, 1, 1, 4), w=_i8(127, -128, -128, 1).reshape(1, 1, 1, 4), bias=None, sw=0.03125,
                       q_in=(0.03125, 127), q_out=(1.0, 100), stride=1, padding=R.VALID, m=1, act=R.NONE,
                       want=_i8(68, 127, 100, 100).reshape(1, 1, 1, 4))
    # The channel mapping, multiplier 1 (m = 2^30, e = 1: (acc << 1) / 2, exact): output o reads input o // m.
    #   m = 2: x = (10, -20), w = (1, 2, 3, 4) -> 10 * 1, 10 * 2, -20 * 3, -20 * 4
    #   m = 3: x = (7, -9), w = (1, -1, 2, 3, -3, 1) -> 7, -7, 14, -27, 27, -9
    K["multiplier_2"] = dict(x=_i8(10, -20).reshape(1, 1, 1, 2), w=_i8(1, 2, 3, 4).reshape(1, 1, 1, 4), bias=None, sw=1.0, q_in=(1.0, 0),
                             q_out=(1.0, 0), stride=1, padding=R.VALID, m=2, act=R.NONE, want=_i8(10, 20, -60, -80).reshape(1, 1, 1, 4))
    K["multiplier_3"] = dict(x=_i8(7, -9).reshape(1, 1, 1, 2), w=_i8(1, -1, 2, 3, -3, 1).reshape(1, 1, 1, 6), bias=None, sw=1.0, q_in=(1.0, 0),
                             q_out=(1.0, 0), stride=1, padding=R.VALID, m=3, act=R.NONE, want=_i8(7, -7, 14, -27, 27, -9).reshape(1, 1, 1, 6))
    return K


KNOWN = _known()

FILTERS = ((1, 1), (3, 3), (2, 3), (5, 1))
IMAGES = (((1, 1), 1), ((5, 7), 3), ((9, 8), 1))
STRIDES = ((1, 1), (2, 2), (4, 3))
CHANNELS = tuple((c, 1) for c in (1, 16, 33, 48, 64, 160)) + tuple((c, m) for c in (5, 32) for m in (2, 3))
GRID = tuple((f, c, m) for f in FILTERS for c, m in CHANNELS)


def operands(shape_x, filt, m, seed, zi=0, per_channel=True, act=R.NONE, stride=(1, 1), padding=R.SAME):
    """Seeded operands of one depthwise convolution: x and w int8 over the full range; the bias and the filter scales are
    CALIBRATED, as a converter calibrates them, on the exact sums of the reference (R.accumulate -- never on the code under test).
    tests/conv2d_i8_cases.py's operands takes the accumulator's spread as 74 x 74 x sqrt(K) from the operands' distributions; that
    holds for a sum over many input channels, but a depthwise channel sums K = fh fw products of ONE filter whose x - zi has the
    mean -0.5 - zi, so here the spread is measured per channel: sd[o] (at least 1), around mean[o].  The bias centres a channel
    (+ sd[o] for an activation with a lower bound at the zero point, so that about a sixth of its values clamp there, not half) and
    adds up to half an sd of noise; the scales map an sd to 20 .. 60 output steps (per tensor: the RMS of the sds), so few values
    reach -128 or 127; the output scale of RELU6 / RELU_N1_TO_1 puts their upper bound 100 steps or more above the zero point."""
    g = np.random.default_rng(seed)
    cout = shape_x[3] * m
    x = g.integers(-128, 128, shape_x, dtype=np.int64).astype(np.int8)
    w = g.integers(-128, 128, (1, filt[0], filt[1], cout), dtype=np.int64).astype(np.int8)
    w[w == 0] = 1                                                    # (a 1x1 filter of weight 0 would make its channel a constant)
    acc = R.accumulate(x, w, zi, stride, padding, m).reshape(-1, cout).astype(np.float64)
    mean, sd = acc.mean(0), np.maximum(acc.std(0), 1.0)
    if acc.shape[0] == 1:                                            # one pixel: the spread is the one across its channels
        mean, sd = np.full(cout, acc.mean()), np.full(cout, max(acc.std(), 1.0))
    centre = 0.0 if act in (R.NONE, R.RELU_N1_TO_1) else 1.0
    bias = np.rint(-mean + sd * (centre + g.uniform(-0.5, 0.5, cout))).astype(np.int32)
    si, so = 0.02, {R.NONE: 0.05, R.RELU: 0.05, R.RELU6: 0.03, R.RELU_N1_TO_1: 0.01}[act]
    mult = g.uniform(0.5, 1.5, cout) * 40.0 / sd if per_channel else g.uniform(0.5, 1.5, 1) * 40.0 / np.sqrt((sd ** 2).mean())
    sw = (mult * so / si).astype(np.float32)
    return x, w, bias, sw, (si, int(zi)), (so, int(g.integers(-20, 21)))


def spread_check(want, q_out, act, where):
    """A kernel that writes a constant must not pass: the REFERENCE's output of a case with at least 64 elements holds at least 16
    distinct values and fewer than half of its bytes sit on a clamp bound."""
    if want.size < 64:
        return
    lo, hi = R.activation_range(act, q_out[0], q_out[1])
    assert np.unique(want).size >= 16, (where, np.unique(want).size)
    assert 2 * int(((want == lo) | (want == hi)).sum()) < want.size, (where, float(((want == lo) | (want == hi)).mean()))


def expect_vec(cout, m, offset, want_out, want_bits):
    """lce_hip_depthwise_conv2d_i8's rule for operands that are 16-byte aligned but for `offset`."""
    return m == 1 and cout % 16 == 0 and offset == 0 and (not want_bits or cout % 32 == 0)


def run_grid(run, filt, cin, m):
    """Every image, stride and padding for one (filter, Cin, multiplier) through `run(x, w, bias, sw, q_in, q_out, stride, padding,
    m, act, want_out=, want_bits=, offset=, path=)` -> (out, bits, took the 16-byte path), against the reference.  Rotates bias
    or none, the activation, the three output combinations, zi, per-channel or per-tensor scales and the placement (offset 1:
    off the 16-byte path).  Asserts which path ran, and runs a case that took the 16-byte path through the row path as well.
    Returns (cases, cases on the 16-byte path)."""
    n, vecs = 0, 0
    cout = cin * m
    for image, batch in IMAGES:
        for stride in STRIDES:
            for padding in (R.SAME, R.VALID):
                if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
                    continue
                k = n + filt[0] + 2 * filt[1] + cin                  # (the rotations start elsewhere for every test of the grid)
                zi = (0, -128, 127, 5, -3)[k % 5]
                act, offset, per_channel = ACTS[k % 4], (k // 2) % 2, (k // 3) % 2 == 0
                # (without a bias a zero-mean sum puts half of a RELU's outputs on its lower bound, which spread_check excludes: the
                # cases without a bias are those of NONE and RELU_N1_TO_1)
                with_bias = act in (R.RELU, R.RELU6) or (k // 4) % 2 == 0
                x, w, bias, sw, q_in, q_out = operands((batch, *image, cin), filt, m, 1000 * image[0] + 100 * batch + 10 * cin + stride[0] + m,
                                                       zi, per_channel, act, stride, padding)
                b = bias if with_bias else None
                want = R.depthwise_i8(x, w, b, sw, q_in, q_out, stride, padding, m, act)
                where = (filt, cin, m, image, batch, stride, padding, n)
                spread_check(want, q_out, act, where)
                outs = (dict(), dict(want_out=False), dict(want_bits=False))[k % 3]
                want_out, want_bits = outs.get("want_out", True), outs.get("want_bits", True)
                for path in (None, 0):
                    out, bits, vec = run(x, w, b, sw, q_in, q_out, stride, padding, m, act, offset=offset, path=path, **outs)
                    if path is None:
                        assert vec == expect_vec(cout, m, offset, want_out, want_bits), where
                        vecs += vec
                    else:
                        assert not vec, where
                    if want_out:
                        assert out.dtype == np.int8 and np.array_equal(out, want), (where, path)
                    else:
                        assert out is None or (out == OUT_MARK).all(), (where, path)
                    if want_bits:
                        assert np.array_equal(bits, R.bitpack(want, q_out[1])), (where, path)
                    else:
                        assert bits is None or (bits == BITS_MARK).all(), (where, path)
                    if not vec:
                        break                                        # (the row path has run)
                n += 1
    return n, vecs
