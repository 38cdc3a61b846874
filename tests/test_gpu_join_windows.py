"""lce_hip_join_windows on the MI355X, bit for bit and without tolerance: copy windows against NumPy slicing compared as int32
views (NaN payloads, -0.0 and subnormals planted), addend windows against NumPy's float32 sum (where that is a NaN, a NaN),
the bits against the oracle's LceQuantize, on both paths, the three output combinations, 1 to 50176 rows, int8 at four zero
points, and the refusals that need device pointers."""
import importlib

import numpy as np
import pytest

import join_cases as J

torch = pytest.importorskip("torch")

amd = importlib.import_module("compute-engine_amd")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = [1, 37, 3136]


def on_device(windows, offset=0):
    """The windows with every array on the device (one that appears twice is copied once), `offset` BYTES behind a 256-byte
    boundary."""
    placed = {}

    def once(a):
        if a is None:
            return None
        if id(a) not in placed:
            n = a.size + offset // a.itemsize
            t = torch.zeros(n, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)[offset // a.itemsize:].view(a.shape)
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == offset % 16 and t.is_contiguous()
            placed[id(a)] = t
        return placed[id(a)]
    return [(once(t), b, c, once(a)) for t, b, c, a in windows]


def run(windows, **kw):
    out, bits = amd.join_windows(windows, **kw)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if bits is None else bits.cpu().numpy()


def check(windows, zero_points=(0,), offset=0):
    """The joined bytes, the bits at every zero point, and the three output combinations."""
    want, nan = J.reference(windows)
    if nan.any():
        assert nan.mean() < 0.2          # (random patterns: ~0.12 of the sums of an addend window; none of a copy)
    dev = on_device(windows, offset)
    got, none = run(dev)
    assert none is None
    J.assert_joined(got, want, nan)
    for zp in zero_points:
        wb = J.want_bits(want, zp)
        both = run(dev, out_bits=True, zero_point=zp)
        J.assert_joined(both[0], want, nan, zp)
        assert np.array_equal(both[1], wb), zp
        only = run(dev, out=False, out_bits=True, zero_point=zp)
        assert only[0] is None and np.array_equal(only[1], wb), zp


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.VEC_F32) + list(J.ROW_F32))
def test_float_windows_bit_for_bit(name, rows):
    check(J.build("f32", {**J.VEC_F32, **J.ROW_F32}[name], rows, rows + len(name)))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.VEC_I8) + list(J.ROW_I8))
def test_int8_windows_and_their_bits_at_four_zero_points(name, rows):
    check(J.build("i8", {**J.VEC_I8, **J.ROW_I8}[name], rows, rows + len(name)), zero_points=(-128, 0, 5, 127))


def test_the_share_of_nan_sums_comes_from_the_reference_alone():
    w = J.build("f32", J.VEC_F32["192:0+128,128+64a"], 3136, 1)
    _, nan = J.reference(w)
    assert not nan[:, :128].any() and 0.05 < nan[:, 128:].mean() < 0.2


def test_a_second_grid_stride():
    """50176 x 192 floats: the output (38.5 MB) is more than the 32 MiB one sweep of the 2048-block grid covers."""
    rows = 50176
    assert rows * 192 * 4 > 2048 * 4 * 256 * 16
    w = J.build("f32", J.VEC_F32["192:0+128,128+64a"], rows, 3)
    want, nan = J.reference(w)
    got, bits = run(on_device(w), out_bits=True)
    J.assert_joined(got, want, nan)
    assert np.array_equal(bits, J.want_bits(want))


@pytest.mark.parametrize("kind,name", [("f32", "192:0+128,128+64a"), ("i8", "192:0+128,128+64")])
def test_a_base_four_bytes_off_a_16_byte_boundary(kind, name):
    w = J.build(kind, (J.VEC_F32 if kind == "f32" else J.VEC_I8)[name], 100, 8)
    check(w, zero_points=(0,) if kind == "f32" else (-7,), offset=4)


def test_channel_slice_is_the_one_window_call_and_numpy_goes_through():
    (x, b, c, _), = J.build("f32", J.VEC_F32["160:32+96"], 50, 2)
    want = np.ascontiguousarray(x[:, b:b + c])
    got, bits = amd.channel_slice(torch.from_numpy(x).to(DEV), b, c, out_bits=True)
    assert np.array_equal(J.raw(got.cpu().numpy()), J.raw(want)) and np.array_equal(bits.cpu().numpy(), J.want_bits(want))
    got, none = amd.channel_slice(x.reshape(5, 10, 160), b, c)                     # NumPy in, NumPy out, leading axes kept
    assert none is None and np.array_equal(J.raw(got), J.raw(want.reshape(5, 10, c)))
    out = torch.zeros((50, c), dtype=torch.float32, device=DEV)
    assert amd.channel_slice(torch.from_numpy(x).to(DEV), b, c, out=out)[0] is out
    assert np.array_equal(J.raw(out.cpu().numpy()), J.raw(want))


def test_refusals_and_empty_on_the_device():
    flat = torch.zeros(8 * 128 + 8 * 64, dtype=torch.float32, device=DEV)
    x, out = flat[:8 * 128].view(8, 128), flat[8 * 96:8 * 96 + 8 * 64].view(8, 64)
    # the window [64, 128) of the first rows ends before `out` begins, yet x's whole [rows, pitch] range meets it
    with pytest.raises(amd.LceHipError, match="overlaps the source of window 0"):
        amd.join_windows([(x, 64, 64)], out=out)
    w = torch.zeros((8, 64), dtype=torch.float32, device=DEV)
    big = torch.zeros((8, 256), dtype=torch.float32, device=DEV)
    with pytest.raises(amd.LceHipError, match="overlaps the addend of window 1"):
        amd.join_windows([(big, 0, 64), (big, 64, 64, flat[:8 * 64].view(8, 64))], out=flat[:8 * 128].view(8, 128))
    bits = flat[:8 * 4].view(8, 4).view(torch.int32)
    arr = (amd.Window * 1)()
    arr[0].data_dev, arr[0].pitch, arr[0].begin, arr[0].count = big.data_ptr(), 256, 0, 128
    s = torch.cuda.current_stream().cuda_stream
    assert amd.lib().lce_hip_join_windows(amd.F32, arr, 1, 8, 0, flat.data_ptr(), bits.data_ptr(), s) == amd.ERR_INVALID
    assert "two outputs overlap" in amd.lib().lce_hip_last_error().decode()
    assert amd.lib().lce_hip_join_windows(amd.F32, arr, 1, 8, 0, None, None, s) == amd.ERR_INVALID
    arr[0].addend_dev = w.data_ptr() + 2
    assert amd.lib().lce_hip_join_windows_check(amd.F32, arr, 1) == amd.ERR_INVALID
    e = torch.zeros((0, 64), dtype=torch.float32, device=DEV)
    o, b = amd.join_windows([(e, 0, 32), (e, 32, 32)], out_bits=True)
    assert o.shape == (0, 64) and b.shape == (0, 2)
