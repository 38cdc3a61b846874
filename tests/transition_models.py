"""A small float model around one pool and one depthwise convolution, for the decisions of the "transition" walker
(tests/test_transition_sections_host.py, tests/test_gpu_transition.py): x (float) -> LceQuantize -> LceBconv2d (3x3, float) y ->
POOL 2x2 / 1 SAME p -> DEPTHWISE_CONV_2D 3x3 / 2 SAME (signed weights and a bias) d -> LceQuantize -> LceBconv2d (float), the graph
output.  The blurred map feeds only the LceQuantize, which therefore folds into the launch that makes it.  Variants: the pool
AVERAGE; a second reader of the pooled tensor (an ADD of a constant whose sum is a graph output); the pooled tensor itself a graph
output.  No tests here."""
import numpy as np

import synth
from section_models import ADD, AVERAGE_POOL_2D, MAX_POOL_2D, NONE, SAME, ModelBuilder, _conv, depthwise_op, ew_op, pool_op

FLAGS = dict(elementwise_sections=True, pool_sections=True, depthwise_sections=True)


def pool_blur_model(H=8, C=64, seed=0, average=False, second_reader=False, deliver_pooled=False):
    """Returns (file, input tensor, output tensors, info): info has the operator indices `pool`, `depthwise`, `quantize` and the
    tensors `p`, `d`, `bits`."""
    b = ModelBuilder()
    f32 = lambda shape, name, data=None: b.tensor(shape, np.float32, name, data)
    g = synth.rng(seed + 901)
    h2 = H // 2
    x = f32([1, H, H, C], "x")
    q0 = b.tensor([1, H, H, C // 32], np.int32, "q0")
    b.custom_op("LceQuantize", [x], [q0], b"")
    y, _ = _conv(b, q0, H, C, C, seed * 10 + 7)
    p = f32([1, H, H, C], "p")
    pool = pool_op(b, AVERAGE_POOL_2D if average else MAX_POOL_2D, [y], [p], (2, 2), (1, 1), SAME)
    k = g.standard_normal((1, 3, 3, C)).astype(np.float32)
    kb = (g.standard_normal(C) * 0.5).astype(np.float32)
    d = f32([1, h2, h2, C], "d")
    dw = depthwise_op(b, [p, f32([1, 3, 3, C], "k", k), f32([C], "kb", kb)], [d], (2, 2), SAME)
    q1 = b.tensor([1, h2, h2, C // 32], np.int32, "q1")
    quantize = b.custom_op("LceQuantize", [d], [q1], b"")
    out, _ = _conv(b, q1, h2, C, C, seed * 10 + 8)
    outputs = [out]
    if second_reader:
        e = f32([1, H, H, C], "e")
        ew_op(b, ADD, [p, f32([C], "shift", g.standard_normal(C).astype(np.float32))], [e], NONE)
        outputs.append(e)
    if deliver_pooled:
        outputs.append(p)
    b.inputs, b.outputs = [x], outputs
    return b.finish(), x, outputs, dict(pool=pool, depthwise=dw, quantize=quantize, tensors=dict(p=p, d=d, bits=q1), size=H, channels=C)
