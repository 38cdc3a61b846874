"""Fixture models with a quantized builtin CONV_2D, shared by tests/test_conv2d_i8_host.py and tests/test_gpu_conv2d_i8.py: a
builder that writes a scale VECTOR and quantized_dimension (tests/tflite_writer.py writes one scale per tensor), the int8
Bi-RealNet-style shortcut block and the int8 stem, each with per-channel or per-tensor filter scales, and their host-side
operators.  No tests here."""
import numpy as np

import conv2d_i8_ref as R
import int8_add_ref as A
import oracle_lib as O
import pool_ref as PR
import synth
from section_models import ADD, AVERAGE_POOL_2D, NONE, RELU, SAME, VALID, bconv_options, conv2d_op, ew_op, pool_op
from tflite_writer import _NP2T, ModelBuilder, _Scalar, _Table, _Vector


class QModelBuilder(ModelBuilder):
    """ModelBuilder whose tensors may carry whole quantization vectors."""

    def qtensor(self, shape, dtype, name, data, scales, zero_points=None, quantized_dimension=None) -> int:
        """A tensor with QuantizationParameters.scale = `scales`, .zero_point = `zero_points` (None: the field is absent) and
        .quantized_dimension (None: absent, the schema's default 0)."""
        t = self.tensor(shape, dtype, name, data)
        fields = {2: _Vector("f", [float(s) for s in scales])}
        if zero_points is not None:
            fields[3] = _Vector("q", [int(z) for z in zero_points])
        if quantized_dimension is not None:
            fields[6] = _Scalar("i", int(quantized_dimension))
        buf = 0 if data is None else len(self.buffers) - 1
        self.tensors[t] = _Table({0: _Vector("i", [int(d) for d in shape]), 1: _Scalar("b", _NP2T[np.dtype(dtype)]),
                                  2: _Scalar("I", buf), 3: name or None, 4: _Table(fields)})
        return t


def filter_tensor(b, w, sw, name="w", zero_points=None, quantized_dimension=0):
    """The constant int8 filter with its scale vector `sw` (1 or Cout scales) and as many zero points, all 0."""
    sw = np.atleast_1d(np.asarray(sw, np.float32))
    zp = [0] * sw.size if zero_points is None else zero_points
    return b.qtensor(w.shape, np.int8, name, w, sw, zp, quantized_dimension)


def conv_constants(cout, filt, cin, seed, q_in, q_out, per_channel):
    """Seeded int8 filter, int32 bias and filter scales whose outputs spread over the int8 range at the given quantization."""
    g = np.random.default_rng(seed)
    w = g.integers(-128, 128, (cout, filt[0], filt[1], cin), dtype=np.int64).astype(np.int8)
    K = filt[0] * filt[1] * cin
    spread = 74.0 * 74.0 * np.sqrt(K)
    bias = g.integers(-int(spread), int(spread) + 1, cout, dtype=np.int64).astype(np.int32)
    mult = g.uniform(0.5, 2.0, cout if per_channel else 1) * 60.0 / spread
    sw = (mult * q_out[0] / q_in[0]).astype(np.float32)
    return w, bias, sw


def _bconv_int8(b, src_bits, H, C, cout, seed, stride, q_out):
    """LceBconv2d 3x3 SAME (one-padding) with an int8 output at q_out; returns (output tensor, its constants)."""
    spec = O.ConvSpec(1, H, H, C, 3, 3, cout, stride_h=stride, stride_w=stride, padding=O.PADDING_SAME, pad_values=1)
    _, w, m, bias = synth.conv_inputs(spec, seed)
    m = (m * np.float32(0.05)).astype(np.float32)
    y = b.tensor([1, spec.out_h, spec.out_h, cout], np.int8, "y%d" % seed, scale=q_out[0], zero_point=q_out[1])
    b.custom_op("LceBconv2d", [src_bits, b.tensor(w.shape, np.int32, "bw%d" % seed, w), b.tensor([cout], np.float32, "bm%d" % seed, m),
                               b.tensor([cout], np.float32, "bb%d" % seed, bias), -1], [y], bconv_options(spec))
    return y, dict(spec=spec, w=w, m=m, b=bias, q=q_out)


def bconv_int8(cv, bits):
    """The oracle's LceBconv2d with int8 output on bitpacked input `bits`."""
    return O.bconv2d(cv["spec"].with_batch(bits.shape[0]), O.DST_I8, bits, cv["w"], cv["m"], cv["b"], out_scale=cv["q"][0],
                     out_zero_point=cv["q"][1])


def shortcut_fixture(per_channel=True, seed=0, H=8, C=64):
    """An int8 Bi-RealNet-style downsampling block on x (int8 [1, H, H, C]):
       0 LceQuantize(x) -> 1 LceBconv2d 3x3 / 2 (C -> 2C, int8) -> y;   2 AVERAGE_POOL_2D 2x2 / 2 (x) -> p;
       3 CONV_2D 1x1 int8 (C -> 2C, + bias) -> s;   4 ADD int8 (y, s), RELU -> the graph output.
    Returns (file, input tensor, output tensor, info)."""
    b = QModelBuilder()
    q_x, q_y, q_s, q_o = (0.05, -4), (0.04, 3), (0.03, -6), (0.06, 5)
    h2, c2 = H // 2, 2 * C
    x = b.tensor([1, H, H, C], np.int8, "x", scale=q_x[0], zero_point=q_x[1])
    q0 = b.tensor([1, H, H, C // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y, cv = _bconv_int8(b, q0, H, C, c2, seed * 10 + 1, 2, q_y)
    p = b.tensor([1, h2, h2, C], np.int8, "p", scale=q_x[0], zero_point=q_x[1])
    pool = pool_op(b, AVERAGE_POOL_2D, [x], [p], (2, 2), (2, 2), VALID)
    w, bias, sw = conv_constants(c2, (1, 1), C, seed + 5, q_x, q_s, per_channel)
    s = b.tensor([1, h2, h2, c2], np.int8, "s", scale=q_s[0], zero_point=q_s[1])
    conv = conv2d_op(b, [p, filter_tensor(b, w, sw), b.tensor([c2], np.int32, "wb", bias)], [s], (1, 1), SAME)
    out = b.tensor([1, h2, h2, c2], np.int8, "out", scale=q_o[0], zero_point=q_o[1])
    add = ew_op(b, ADD, [y, s], [out], RELU)
    b.inputs, b.outputs = [x], [out]
    q_add = (q_y[0], q_y[1], q_s[0], q_s[1], q_o[0], q_o[1])
    host = {pool: lambda v: PR.pool2d(v, PR.AVERAGE, (2, 2), (2, 2), VALID, NONE, q_x[0], q_x[1]),
            conv: lambda v: R.conv2d_i8(v, w, bias, sw, q_x, q_s, (1, 1), SAME),
            add: lambda a, c: A.add_q(a, c, q_add, A.ACT_RELU)}

    def oracle(v):
        return host[add](bconv_int8(cv, O.bitpack(v, q_x[1])), host[conv](host[pool](v)))
    info = dict(shape=(H, H, C), conv=conv, pool=pool, add=add, host=host, oracle=oracle, w=w, bias=bias, sw=sw, q_in=q_x, q_out=q_s,
                ops=5, plain=[[0, 1]], parent_flags=dict(int8_add_sections=True, pool_sections=True, stem_sections=True),
                parent_sections=[[0, 1, 2]], stats=dict(conv_i8=(1, 0), int8_add=(1, 0), pool=(1, 0)))
    return b.finish(), x, out, info


def stem_fixture(per_channel=True, seed=0, H=17, cout=64):
    """An int8 stem on x (int8 [1, 17, 17, 3]): 0 CONV_2D 3x3 / 2 SAME int8 (3 -> 64, + bias, RELU) -> c; 1 LceQuantize(c);
    2 LceBconv2d 3x3 (64 -> 64, int8) -> the graph output.  Returns (file, input tensor, output tensor, info)."""
    b = QModelBuilder()
    q_x, q_c, q_y = (0.02, -128), (0.05, -9), (0.04, 2)
    h2 = (H + 1) // 2
    x = b.tensor([1, H, H, 3], np.int8, "x", scale=q_x[0], zero_point=q_x[1])
    w, bias, sw = conv_constants(cout, (3, 3), 3, seed + 7, q_x, q_c, per_channel)
    c = b.tensor([1, h2, h2, cout], np.int8, "c", scale=q_c[0], zero_point=q_c[1])
    conv = conv2d_op(b, [x, filter_tensor(b, w, sw), b.tensor([cout], np.int32, "wb", bias)], [c], (2, 2), SAME, RELU)
    q0 = b.tensor([1, h2, h2, cout // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [c], [q0], b"")
    y, cv = _bconv_int8(b, q0, h2, cout, cout, seed * 10 + 2, 1, q_y)
    b.inputs, b.outputs = [x], [y]
    host = {conv: lambda v: R.conv2d_i8(v, w, bias, sw, q_x, q_c, (2, 2), SAME, R.RELU)}

    def oracle(v):
        return bconv_int8(cv, O.bitpack(host[conv](v), q_c[1]))
    info = dict(shape=(H, H, 3), conv=conv, host=host, oracle=oracle, w=w, bias=bias, sw=sw, q_in=q_x, q_out=q_c, ops=3, plain=[[1, 2]],
                parent_flags=dict(int8_add_sections=True, pool_sections=True, stem_sections=True), parent_sections=[[1, 2]],
                stats=dict(conv_i8=(1, 1), int8_add=(0, 0), pool=(0, 0)))
    return b.finish(), x, y, info


FIXTURES = {"shortcut_per_channel": lambda: shortcut_fixture(True), "shortcut_per_tensor": lambda: shortcut_fixture(False),
            "stem_per_channel": lambda: stem_fixture(True), "stem_per_tensor": lambda: stem_fixture(False)}
ALL_FLAGS = dict(int8_add_sections=True, pool_sections=True, stem_sections=True, conv2d_i8_sections=True)
