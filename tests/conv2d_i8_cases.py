"""The cases the three suites of lce_hip_conv2d_i8 share (tests/test_conv2d_i8_host.py, tests/test_conv2d_i8_hostsim.py,
tests/test_gpu_conv2d_i8.py): the known answers worked by hand, and the grid over filters, images, strides, paddings and output
channels, each run through a `run` the suite supplies (the host simulation of the kernel, or the device) and compared byte for
byte with tests/conv2d_i8_ref.py."""
import numpy as np

import conv2d_i8_ref as R

OUT_MARK, BITS_MARK = np.int8(0x5A), 0x55555555
ACTS = (R.NONE, R.RELU, R.RELU_N1_TO_1, R.RELU6)


def _i8(*v):
    return np.array(v, np.int8)


def _known():
    """name -> dict(x, w, bias, sw, q_in, q_out, stride, padding, act, want).  Every `want` is worked by hand below; 2^30 as a
    multiplier is 'times one half', SRDHM(a, 2^30) = trunc((a 2^30 + nudge) / 2^31) with nudge 2^30 for a >= 0 and 1 - 2^30
    below: a / 2 with a tie going UP (3 -> 2, -3 -> -1); RDivPOT(x, n) rounds x / 2^n to nearest, a tie AWAY from zero."""
    K = {}
    # A corner pixel with zi = 5 under SAME padding: the 3x3 window of output (0, 0) of a 2x2 image has 4 taps inside, 5 in the
    # padding, which the reference SKIPS (reading them as x = 0 would add (0 - 5) w).  Multiplier 0.5 * 0.5 / 2 = 2^-3: m = 2^30, e = -2.
    #   (0,0): 5*5 + 15*6 + 25*8 + 35*9 = 630 -> SRDHM 315 -> RDivPOT(315, 2) = 78 rem 3 -> 79 -> + zo = 76
    #   (0,1): 5*4 + 15*5 + 25*7 + 35*8 = 550 -> 275 -> 68 rem 3 -> 69 -> 66
    #   (1,0): 5*2 + 15*3 + 25*5 + 35*6 = 390 -> 195 -> 48 rem 3 -> 49 -> 46
    #   (1,1): 5*1 + 15*2 + 25*4 + 35*5 = 310 -> 155 -> 38 rem 3 -> 39 -> 36
    K["corner_same_pad"] = dict(x=_i8(10, 20, 30, 40).reshape(1, 2, 2, 1), w=_i8(*range(1, 10)).reshape(1, 3, 3, 1), bias=None, sw=0.5,
                                q_in=(0.5, 5), q_out=(2.0, -3), stride=1, padding=R.SAME, act=R.NONE,
                                want=_i8(76, 66, 46, 36).reshape(1, 2, 2, 1))
    # zi = -128, the extreme weights, multiplier 2^-4 * 2^-4 = 2^-8: m = 2^30, e = -7.
    #   ch 0: 255*127 + 255*(-128) + 0*127 + 128*(-128) = -16639 -> SRDHM: -8319.5, the tie goes up: -8319 -> RDivPOT(., 7): -64.99 -> -65
    #   ch 1: -(255 + 255 + 0 + 128) * 128 = -81664 -> -40832 -> exactly -319 -> clamped to -128
    K["zi_minus_128"] = dict(x=_i8(127, 127, -128, 0).reshape(1, 1, 1, 4), w=_i8(127, -128, 127, -128, -128, -128, -128, -128).reshape(2, 1, 1, 4),
                             bias=None, sw=0.0625, q_in=(0.0625, -128), q_out=(1.0, 0), stride=1, padding=R.VALID, act=R.NONE,
                             want=_i8(-65, -128).reshape(1, 1, 1, 2))
    # zi = 127, multiplier 2^-5 * 2^-5 = 2^-10: m = 2^30, e = -9, zo = 100.
    #   ch 0: -255*127 - 255*127 + 0 - 127*1 = -64897 -> SRDHM: -32448.5 -> -32448 -> / 512 = -63.375 -> -63 -> 37
    #   ch 1: 255*128 + 255*128 = 65280 -> 32640 -> 63.75 -> 64 -> 164 -> clamped to 127
    #   ch 2: 65280 + 127*128 = 81536 -> 40768 -> 79.625 -> 80 -> 180 -> 127
    K["zi_127"] = dict(x=_i8(-128, -128, 127, 0).reshape(1, 1, 1, 4),
                       w=_i8(127, 127, -128, 1, -128, -128, 0, 0, -128, -128, -128, -128).reshape(3, 1, 1, 4), bias=None, sw=0.03125,
                       q_in=(0.03125, 127), q_out=(1.0, 100), stride=1, padding=R.VALID, act=R.NONE, want=_i8(37, 127, 127).reshape(1, 1, 1, 3))
    # Requantization ties on each side of zero, multiplier 2^-2: m = 2^30, e = -1 -- two roundings, SRDHM then RDivPOT(., 1).
    #   6 -> 3 -> 1.5: 2      -6 -> -3 -> -1.5: -2 (RDivPOT's threshold for a negative x: the tie goes away from zero)
    #   2 -> 1 -> 0.5: 1      -2 -> -1 -> -0.5: -1
    #   3 -> 1.5: 2 (nudge) -> 1      -3 -> -1.5: -1 (the nudge of a negative product) -> -0.5: -1
    K["ties"] = dict(x=_i8(6, -6, 2, -2, 3, -3).reshape(1, 1, 6, 1), w=_i8(1).reshape(1, 1, 1, 1), bias=None, sw=0.5, q_in=(0.5, 0),
                     q_out=(1.0, 0), stride=1, padding=R.VALID, act=R.NONE, want=_i8(2, -2, 1, -1, 1, -1).reshape(1, 1, 6, 1))
    # e = 0: multiplier 0.5 = 2^30 * 2^(0 - 31): 3 -> 1.5: 2, -3 -> -1.5: -1, 4 -> 2; the bias 1 is added BEFORE: 4, -2, 5 -> 2, -1, 2.5: 3
    K["e_zero"] = dict(x=_i8(3, -3, 4).reshape(1, 1, 3, 1), w=_i8(1).reshape(1, 1, 1, 1), bias=np.array([1], np.int32), sw=1.0, q_in=(0.5, 0),
                       q_out=(1.0, 0), stride=1, padding=R.VALID, act=R.NONE, want=_i8(2, -1, 3).reshape(1, 1, 3, 1))
    # e > 0: multiplier 2 = 2^30 * 2^(2 - 31): (acc << 2) / 2 = 2 acc, exact; -140 is clamped
    K["e_positive"] = dict(x=_i8(3, -3, 50, -70).reshape(1, 1, 4, 1), w=_i8(1).reshape(1, 1, 1, 1), bias=None, sw=1.0, q_in=(2.0, 0),
                           q_out=(1.0, 0), stride=1, padding=R.VALID, act=R.NONE, want=_i8(6, -6, 100, -128).reshape(1, 1, 4, 1))
    # e = -31: multiplier 2^-16 * 2^-16 = 2^-32 = 2^30 * 2^(-31 - 31): +-16129 -> +-8064.5 -> shifted out by 31: 0 on both sides -> zo
    K["e_minus_31"] = dict(x=_i8(127, -127).reshape(1, 1, 2, 1), w=_i8(127).reshape(1, 1, 1, 1), bias=None, sw=2.0 ** -16, q_in=(2.0 ** -16, 0),
                           q_out=(1.0, 7), stride=1, padding=R.VALID, act=R.NONE, want=_i8(7, 7).reshape(1, 1, 2, 1))
    # The four activations at (so, zo) = (0.05, -10) under multiplier 1 (m = 2^30, e = 1): v = x + zo = -110, -35, -10, 5, 117.
    # Q(0) = -10, Q(6) = -10 + 120 = 110, Q(-1) = -30, Q(1) = 10.
    for act, want in ((R.NONE, (-110, -35, -10, 5, 117)), (R.RELU, (-10, -10, -10, 5, 117)), (R.RELU_N1_TO_1, (-30, -30, -10, 5, 10)),
                      (R.RELU6, (-10, -10, -10, 5, 110))):
        K["activation_%d" % act] = dict(x=_i8(-100, -25, 0, 15, 127).reshape(1, 1, 5, 1), w=_i8(1).reshape(1, 1, 1, 1), bias=None, sw=1.0,
                                        q_in=(0.05, 0), q_out=(0.05, -10), stride=1, padding=R.VALID, act=act,
                                        want=_i8(*want).reshape(1, 1, 5, 1))
    return K


KNOWN = _known()

# MultiplyByQuantizedMultiplier alone, (acc, m, e) -> result, by hand: the ties above, and e = -31 at the ends of int32 --
# SRDHM(2^31 - 1, 2^30) = 2^30, whose remainder 2^30 exceeds the threshold 2^30 - 1: 1; SRDHM(-2^31, 2^30) = -2^30, whose
# remainder 2^30 does not exceed the threshold of a negative x, 2^30: -1 + 0; and SRDHM's one saturating pair.
REQUANT_KNOWN = ((3, 1 << 30, 0, 2), (-3, 1 << 30, 0, -1), (6, 1 << 30, -1, 2), (-6, 1 << 30, -1, -2), (-2, 1 << 30, -1, -1),
                 (5, 1 << 30, 2, 10), (-5, 1 << 30, 2, -10), ((1 << 31) - 1, 1 << 30, -31, 1), (-(1 << 31), 1 << 30, -31, -1),
                 (12345, 0, 0, 0), (-(1 << 31), (1 << 31) - 1, 0, -(1 << 31) + 1), ((1 << 31) - 1, (1 << 31) - 1, 0, (1 << 31) - 2))

# (filter, Cin): K = 1, 27, 147, 64 (exactly two instructions), 65 (one byte more), 288 (several chunks, the 16-byte path), 96 (the
# 16-byte path, a filter row of 48), 15 (a chunk ending inside a tap is (3, 3) x 32: 128 = 4 taps exactly -- and (7, 7) x 3: 128 = 42 taps + 2)
GRID = (((1, 1), 1), ((3, 3), 3), ((7, 7), 3), ((1, 1), 64), ((1, 1), 65), ((3, 3), 32), ((2, 3), 16), ((1, 5), 3))
IMAGES = (((1, 1), 1), ((5, 7), 3), ((9, 8), 1))
STRIDES = ((1, 1), (2, 2), (4, 3))


def operands(shape_x, filt, cout, seed, zi=0, per_channel=True):
    """Seeded operands of one convolution: x int8 over the full range, w int8 over the full range, a bias of the
    accumulator's magnitude, filter scales that spread the outputs over the int8 range with some saturation at both ends."""
    g = np.random.default_rng(seed)
    cin = shape_x[3]
    x = g.integers(-128, 128, shape_x, dtype=np.int64).astype(np.int8)
    w = g.integers(-128, 128, (cout, filt[0], filt[1], cin), dtype=np.int64).astype(np.int8)
    K = filt[0] * filt[1] * cin
    spread = 74.0 * 74.0 * np.sqrt(K)
    bias = g.integers(-int(spread), int(spread) + 1, cout, dtype=np.int64).astype(np.int32)
    si, so = 0.02, 0.05
    mult = g.uniform(0.5, 2.0, cout if per_channel else 1) * 60.0 / spread
    sw = (mult * so / si).astype(np.float32)
    return x, w, bias, sw, (si, int(zi)), (so, int(g.integers(-20, 21)))


def run_grid(run, filt, cin):
    """Every image, stride, padding and output channel count for one (filter, Cin) through `run(x, w, bias, sw, q_in, q_out, stride,
    padding, act, want_out, want_bits, offset)` -> (out, bits, vec or None), against the reference.  Rotates bias or none, the
    activation, the three output combinations, zi, per-channel or per-tensor scales and the placement (offset 1: off the
    16-byte path).  Returns (cases, cases on the 16-byte path)."""
    n, vecs = 0, 0
    for image, batch in IMAGES:
        for stride in STRIDES:
            for padding in (R.SAME, R.VALID):
                if padding == R.VALID and (image[0] < filt[0] or image[1] < filt[1]):
                    continue
                zi = (0, -128, 127, 5, -3)[n % 5]
                per_channel = (n // 3) % 2 == 0
                x, w, bias, sw, q_in, q_out = operands((batch, *image, cin), filt, 160, 1000 * image[0] + 100 * batch + 10 * cin + stride[0], zi,
                                                       per_channel)
                acc = R.accumulate(x, w, zi, stride, padding)
                for cout in (1, 33, 160):
                    act, with_bias, offset = ACTS[n % 4], (n // 4) % 2 == 0, (n // 2) % 2
                    b = bias[:cout] if with_bias else None
                    s = sw[:cout] if per_channel else sw
                    want = R.finish(acc[..., :cout], b, s, q_in, q_out, act)
                    outs = (dict(), dict(want_out=False), dict(want_bits=False))[n % 3]
                    out, bits, vec = run(x, w[:cout], b, s, q_in, q_out, stride, padding, act, offset=offset, **outs)
                    where = (filt, cin, image, batch, stride, padding, cout, n)
                    if vec is not None:
                        assert vec == (cin % 16 == 0 and offset == 0), where
                        vecs += vec
                    if outs.get("want_out", True):
                        assert out.dtype == np.int8 and np.array_equal(out, want), where
                    else:
                        assert out is None or (out == OUT_MARK).all(), where
                    if outs.get("want_bits", True):
                        assert np.array_equal(bits, R.bitpack(want, q_out[1])), where
                    else:
                        assert bits is None or (bits == BITS_MARK).all(), where
                    n += 1
    return n, vecs
