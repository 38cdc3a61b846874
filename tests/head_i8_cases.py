"""The cases the suites of the int8 head share (tests/test_head_i8_host.py, tests/test_head_i8_hostsim.py,
tests/test_gpu_head_i8.py): the FULLY_CONNECTED grid, the map case that decides the operand and C/D maps of the matrix
instruction, the accumulator's extremes, and the MEAN / SOFTMAX sets of the feature's specification.  Each FULLY_CONNECTED case
is run through a `run(x, w, bias, sw, q_in, q_out, act)` the suite supplies (the host simulation, or the device) and compared byte
for byte with tests/head_i8_ref.py.  No tests here."""
import numpy as np

import head_i8_ref as H
from int8_conv_models import conv_constants

# (batch, K, N): every value of batch in {1, 15, 16, 17, 33}, K in {1, 15, 16, 17, 63, 64, 65, 70, 512} and N in {1, 15, 16, 17, 33,
# 1000} at least once, and the corners of the three axes
FC_GRID = [(1, 1, 1), (33, 512, 1000), (1, 512, 1), (33, 1, 1), (1, 1, 1000), (33, 512, 1), (33, 1, 1000), (1, 512, 1000),
           (15, 15, 15), (16, 16, 16), (17, 17, 17), (33, 63, 33), (16, 64, 17), (17, 65, 16), (15, 70, 33), (16, 512, 15)]
ZIS = (-128, 0, 127)
ACTS = (H.NONE, H.RELU, H.RELU_N1_TO_1, H.RELU6)
# the MEAN sets: (H, W, C, q_in, q_out); and the SOFTMAX sets: (input scale, beta, cols)
MEAN_SETS = [(7, 7, 40, (0.05, -4), (0.05, -4)), (7, 7, 40, (0.05, -4), (0.021, 3)), (5, 3, 33, (0.02, -128), (0.031, 7)),
             (2, 9, 70, (0.03, 5), (0.03, 5)), (1, 1, 8, (0.05, -4), (0.021, 3))]
SOFTMAX_SETS = [(0.1, 1.0, 10), (0.05, 1.0, 1000), (0.2, 0.5, 67), (0.02, 2.0, 129), (1.0, 1.0, 7), (0.003, 1.0, 64)]


def fc_operands(batch, K, N, seed, zi=-4, per_channel=True, bias=True):
    """Seeded (x, w, bias, sw, q_in, q_out) whose outputs spread over the int8 range."""
    g = np.random.default_rng(1000 * seed + 7 * batch + K + N)
    q_in, q_out = (0.05, zi), (0.04, 3)
    x = g.integers(-128, 128, (batch, K), dtype=np.int64).astype(np.int8)
    w4, b, sw = conv_constants(N, (1, 1), K, seed + K + N, q_in, q_out, per_channel)
    return x, w4.reshape(N, K), (b if bias else None), sw, q_in, q_out


def run_fc_grid(run, cases=FC_GRID):
    """Every case of the grid with rotating bias, scale kind, input zero point and activation, through `run` -> (out, vec).
    Returns (cases run, how many took the 16-byte path)."""
    n = vecs = 0
    for k, (batch, K, N) in enumerate(cases):
        x, w, bias, sw, q_in, q_out = fc_operands(batch, K, N, k, ZIS[k % 3], per_channel=k % 2 == 0, bias=k % 4 != 3)
        act = ACTS[k % 4]
        want = H.fully_connected_i8(x, w, bias, sw, q_in, q_out, act)
        out, vec = run(x, w, bias, sw, q_in, q_out, act)
        assert out.dtype == np.int8 and np.array_equal(out, want), (batch, K, N, np.argwhere(out != want)[:5])
        assert vec is None or vec == (K % 16 == 0), (batch, K, N)
        n += 1
        vecs += bool(K % 16 == 0)
    return n, vecs


def fold_i8(v):
    """An integer array folded into int8 (two's complement wrap)."""
    return ((np.asarray(v, np.int64) + 128) % 256 - 128).astype(np.int8)


def map_case(batch=33, K=70, N=33):
    """The case that decides the maps: input row i is one-hot at k = i (rows beyond K wrap: k = i mod K) with a value that depends
    on i, the weight is ASYMMETRIC, w[o][k] = 3 o - 5 k folded into int8.  Output [i][o] = (v_i - zi) w[o][k_i] + ... requantized:
    a transposed operand or store puts w[k_i][o]-like values where w[o][k_i] belongs.  zi = 0, so the other columns contribute 0."""
    x = np.zeros((batch, K), np.int8)
    rows = np.arange(batch)
    x[rows, rows % K] = fold_i8(17 + 3 * rows)
    w = fold_i8(3 * np.arange(N)[:, None] - 5 * np.arange(K)[None, :])
    q_in, q_out = (0.05, 0), (0.05, 0)
    sw = np.float32(1.0 / 128.0)            # real multiplier 2^-7: products up to 127 * 128 come back as up to 127
    return x, w, None, sw, q_in, q_out


def extremes_case(K=512, N=17, batch=5):
    """x = w = -128 over K = 512 with zi = 127: every product is 255 * 128 (the reference's bound per term), bias at +-2^30."""
    x = np.full((batch, K), -128, np.int8)
    w = np.full((N, K), -128, np.int8)
    w[1::2] = 127
    bias = np.where(np.arange(N) % 3 == 0, 1 << 30, -(1 << 30)).astype(np.int32)
    q_in, q_out = (0.05, 127), (0.05, -5)
    sw = np.float32(2.0 ** -24)
    assert 255 * 128 * K + (1 << 30) <= (1 << 31) - 1
    return x, w, bias, sw, q_in, q_out


def mean_input(h, w, c, batch, seed):
    return np.random.default_rng(seed).integers(-128, 128, (batch, h, w, c), dtype=np.int64).astype(np.int8)


def softmax_input(rows, cols, seed, spread=None):
    """int8 logits: normal around a per-row centre with a per-row spread, so that rows differ in how peaked they are, plus a
    one-hot row (127 against -128: the clamp at 127) when there is room."""
    g = np.random.default_rng(seed)
    sd = g.uniform(2, 60, (rows, 1)) if spread is None else spread
    q = np.clip(np.rint(g.normal(g.uniform(-60, 60, (rows, 1)), sd, (rows, cols))), -128, 127).astype(np.int8)
    if rows > 1:
        q[-1] = -128
        q[-1, cols // 2] = 127
    return q
