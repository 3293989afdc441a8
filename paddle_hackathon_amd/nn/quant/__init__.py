"""``paddle.nn.quant`` (reference: python/paddle/nn/quant/__init__.py): quantization-aware layers,
float functional layers, the fake-quant ops (HIP kernels: csrc/kernels/quant.hip) and weight-only int8
(``weight_quantize`` / ``weight_only_linear``; HIP kernel: csrc/kernels/skinny_w8.hip)."""
from .functional_layers import FloatFunctionalLayer, add, subtract, multiply, divide, reshape, transpose, \
    concat, flatten  # noqa: F401
from .quant_layers import QuantStub, FakeQuantAbsMax, FakeQuantMovingAverageAbsMax, \
    FakeQuantChannelWiseAbsMax, MovingAverageAbsMaxScale, QuantizedConv2D, QuantizedConv2DTranspose, \
    QuantizedLinear, MAOutputScaleLayer, FakeQuantMAOutputScaleLayer  # noqa: F401
from .weight_only import weight_quantize, weight_dequantize, weight_only_linear  # noqa: F401
from . import quant_layers, functional_layers, ops, weight_only  # noqa: F401

__all__ = []
