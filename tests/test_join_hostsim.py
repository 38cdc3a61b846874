"""The join's kernel bodies (csrc/lce_kernels_join.h) on the CPU against NumPy, bit for bit: windows and whole tensors (the dense
join of lce_hip_concat), both paths, every instance, the three output combinations, and grids capped at 1 and 3 blocks so that
every wave takes several grid strides.  No GPU."""
import numpy as np
import pytest

import hostsim_join_lib as H
import join_cases as J

ROWS = [1, 37, 150]          # 150 x 192 floats = 7200 chunks: 8 strides of a 1-block grid, 3 of a 3-block grid


def check(windows, vec, cap, zero_point=0, offset=0):
    want, nan = J.reference(windows)
    wb = J.want_bits(want, zero_point)
    got, bits, took = H.sim(windows, zero_point, True, True, cap, offset)
    assert took == vec
    J.assert_joined(got, want, nan)
    assert np.array_equal(bits, wb)
    got, none, _ = H.sim(windows, zero_point, True, False, cap, offset)
    assert none is None
    J.assert_joined(got, want, nan)
    none, bits, _ = H.sim(windows, zero_point, False, True, cap, offset)
    assert none is None and np.array_equal(bits, wb)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.VEC_F32) + list(J.ROW_F32))
def test_float_windows(name, rows, cap):
    vec = name in J.VEC_F32
    check(J.build("f32", (J.VEC_F32 if vec else J.ROW_F32)[name], rows, rows + cap), vec, cap)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.VEC_I8) + list(J.ROW_I8))
def test_int8_windows_at_four_zero_points(name, rows, cap):
    vec = name in J.VEC_I8
    w = J.build("i8", (J.VEC_I8 if vec else J.ROW_I8)[name], rows, rows + cap)
    for zp in (-128, 0, 5, 127):
        check(w, vec, cap, zp)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.DENSE_VEC_F32) + list(J.DENSE_ROW_F32))
def test_dense_float_joins(name, rows, cap):
    vec = name in J.DENSE_VEC_F32
    check(J.build("f32", (J.DENSE_VEC_F32 if vec else J.DENSE_ROW_F32)[name], rows, rows + cap), vec, cap)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.DENSE_VEC_I8) + list(J.DENSE_ROW_I8))
def test_dense_int8_joins_at_four_zero_points(name, rows, cap):
    vec = name in J.DENSE_VEC_I8
    w = J.build("i8", (J.DENSE_VEC_I8 if vec else J.DENSE_ROW_I8)[name], rows, rows + cap)
    for zp in (-128, 0, 5, 127):
        check(w, vec, cap, zp)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(J.DENSE_WORDS))
def test_bitpacked_words_join_as_four_byte_elements(name, rows, cap):
    """lce_hip_concat's bitpacked kind: int32 patterns through the float instances, value output only, compared as raw bits."""
    case, vec = J.DENSE_WORDS[name]
    w = J.build("f32", case, rows, rows + cap)
    words = [t.view(np.int32) for t, _, _, _ in w]
    got, none, took = H.sim(w, 0, True, False, cap)
    assert none is None and took == vec
    assert np.array_equal(got.view(np.int32), np.concatenate(words, axis=-1))


@pytest.mark.parametrize("kind,name", [("f32", "192:0+128,128+64a"), ("i8", "192:0+128,128+64")])
def test_a_base_four_bytes_off_takes_the_row_path(kind, name):
    w = J.build(kind, (J.VEC_F32 if kind == "f32" else J.VEC_I8)[name], 37, 5)
    check(w, False, 3, 0 if kind == "f32" else -7, offset=4)


def test_a_value_only_launch_needs_no_multiple_of_32():
    w = J.build("f32", J.ROW_F32["68:0+36,36+32a"], 37, 9)
    want, nan = J.reference(w)
    got, _, took = H.sim(w, 0, True, False, 3)
    assert took
    J.assert_joined(got, want, nan)


def test_the_sum_keeps_subnormals_and_a_copy_keeps_minus_zero():
    x = np.zeros((2, 8), np.float32)
    x.view(np.uint32)[0, :] = [0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x80000000, 0x00000001, 0x80000001, 0x7F7FFFFF]
    a = np.zeros((2, 4), np.float32)
    a.view(np.uint32)[0, :] = [0x00000000, 0x00000001, 0x00000001, 0x7F7FFFFF]
    w = [(x, 0, 4, None), (x, 4, 4, a)]
    got, _, took = H.sim(w, 0, True, False, 1)
    assert took
    want = [0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x00000000, 0x00000002, 0x00000000, 0x7F800000]
    assert got.view(np.uint32)[0].tolist() == want
