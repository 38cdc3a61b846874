"""NumPy reference of lce_hip_pool_depthwise_f32 / lce_hip_pool_depthwise_i8 (include/lce_hip.h): nothing but the composition of the
references the two entries already have -- tests/pool_ref.py's MAX pool, then tests/depthwise_ref.py / tests/depthwise_i8_ref.py on
the pooled tensor.  The fused launch must give these bytes."""
import numpy as np

import depthwise_i8_ref as DI
import depthwise_ref as DF
import pool_ref as P

SAME, VALID = P.SAME, P.VALID
NONE, RELU, RELU_N1_TO_1, RELU6 = P.NONE, P.RELU, P.RELU_N1_TO_1, P.RELU6


def _pair(v):
    return (v, v) if isinstance(v, (int, np.integer)) else tuple(v)


def pooled(x, pool):
    """``pool``: dict(filter, stride, padding, activation) of a MAX pool; int8 also scale and zero_point."""
    return P.pool2d(x, P.MAX, _pair(pool["filter"]), _pair(pool["stride"]), pool["padding"], pool.get("activation", NONE),
                    pool.get("scale"), pool.get("zero_point", 0))


def pool_depthwise(x, pool, w, bias=None, stride=(1, 1), padding=SAME, depth_multiplier=1, activation=NONE):
    """float32 [B, H, W, C] -> the depthwise convolution of the pooled tensor, float32."""
    return DF.depthwise(pooled(np.asarray(x, np.float32), pool), w, bias, _pair(stride), padding, depth_multiplier, activation)


def pool_depthwise_i8(x, pool, w, bias, filter_scales, q_out, stride=(1, 1), padding=SAME, depth_multiplier=1, activation=NONE):
    """int8 [B, H, W, C] at the pool's (scale, zero_point), which is the depthwise convolution's input quantization."""
    q_in = (pool["scale"], pool["zero_point"])
    return DI.depthwise_i8(pooled(x, pool), w, bias, filter_scales, q_in, q_out, _pair(stride), padding, depth_multiplier, activation)


def bitpack_f32(v):
    """lce_hip_bitpack of a float32 NHWC tensor: bit = v < 0, LSB first, ceil(C / 32) int32 words per pixel, padding bits 0."""
    v = np.asarray(v)
    c = v.shape[-1]
    words = (c + 31) // 32
    neg = np.zeros(v.shape[:-1] + (words * 32,), np.uint64)
    neg[..., :c] = v < 0
    neg = neg.reshape(v.shape[:-1] + (words, 32))
    return (neg << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)
