"""Weight-only int8 quantisation (reference: python/paddle/nn/quant/quantized_linear.py):
``weight_quantize``, ``weight_dequantize`` and ``weight_only_linear``.

The weights are int8, symmetric, one fp32 scale per output channel; activations stay bf16 / fp16. With
at most 16 rows on the GPU the product runs on the int8 weight-streaming kernel
(csrc/kernels/skinny_w8.hip, ``ops.hip.skinny_gemm_w8``): the weights are dequantised exactly in
registers and the scale multiplies the fp32 sum. Anywhere else the weight is dequantised to the
input's dtype and the product runs as ``fused_linear`` does today."""
from __future__ import annotations

import torch

from ...framework.core import Tensor, _wrap, convert_dtype

__all__ = ["weight_quantize", "weight_dequantize", "weight_only_linear"]


def _t(x):
    return x._t if isinstance(x, Tensor) else x


def _int8_only(what, value, want):
    if value != want:
        raise ValueError(f"{what}={value!r}: weight-only quantisation exists for int8 only ({want!r})")


def weight_quantize(x, algo="weight_only_int8"):
    """a float weight ``x`` [K, N] -> (int8 [N, K], fp32 scale [N]): symmetric, per output channel,
    ``scale = absmax / 127`` in fp32 (1 for a channel that is all zero) and
    ``q = clamp(round(x / scale), -127, 127)``. Runs once per weight, as a torch composite."""
    _int8_only("weight_quantize: algo", algo, "weight_only_int8")
    w = _t(x)
    if not isinstance(w, torch.Tensor) or w.dim() != 2 or not w.dtype.is_floating_point:
        raise ValueError(f"weight_quantize: x must be a 2-D float tensor [K, N], got "
                         f"{getattr(w, 'dtype', type(w))} {tuple(getattr(w, 'shape', ()))}")
    w = w.detach().to(torch.float32).t()                               # [N, K]
    absmax = w.abs().amax(1)
    scale = torch.where(absmax > 0, absmax / 127.0, torch.ones_like(absmax))
    q = torch.round(w / scale[:, None]).clamp_(-127, 127).to(torch.int8).contiguous()
    return _wrap(q), _wrap(scale)


def weight_dequantize(x, scale, out_dtype="float16", algo="weight_only_int8"):
    """int8 ``x`` [N, K] with its fp32 ``scale`` [N] -> the weight [K, N] in ``out_dtype``"""
    _int8_only("weight_dequantize: algo", algo, "weight_only_int8")
    from ...incubate.nn.functional import _w8_dequant
    q, s = _t(x), _t(scale)
    if q.dtype != torch.int8 or q.dim() != 2 or s.numel() != q.shape[0]:
        raise ValueError(f"weight_dequantize: x must be int8 [N, K] with a scale of N elements, got {q.dtype} "
                         f"{tuple(q.shape)} and {tuple(s.shape)}")
    return _wrap(_w8_dequant(q, s, convert_dtype(out_dtype)))


def weight_only_linear(x, weight, bias=None, weight_scale=None, weight_dtype="int8"):
    """``x`` [..., K] times the int8 ``weight`` [N, K] of ``weight_quantize`` with its ``weight_scale`` [N],
    plus ``bias`` [N]. On the int8 weight-streaming kernel when x is on the GPU with at most 16 rows,
    nothing needs a gradient, the kernel takes the arguments and ``PHA_DECODE_GEMM`` is not 0; otherwise
    the weight is dequantised to x's dtype and the product runs as ``fused_linear`` does. More than 16
    rows or a CPU input is no fallback; arguments the kernel cannot take at 16 rows or fewer are
    recorded as one (``ops.fallback``)."""
    _int8_only("weight_only_linear: weight_dtype", weight_dtype, "int8")
    from ...incubate.nn import functional as FF
    if weight_scale is None:
        raise ValueError("weight_only_linear: weight_scale (fp32 [N], from weight_quantize) is required")
    a, q, s, b = _t(x), _t(weight), _t(weight_scale), _t(bias)
    if q.dtype != torch.int8 or q.dim() != 2 or q.shape[1] != a.shape[-1] or s.numel() != q.shape[0]:
        raise ValueError(f"weight_only_linear: weight must be int8 [N, K={a.shape[-1]}] with a scale of N elements, "
                         f"got {q.dtype} {tuple(q.shape)} and {tuple(s.shape)}")
    s = s.reshape(-1)
    if a.is_cuda and a.numel() // max(a.shape[-1], 1) <= FF._ops.hip.SKINNY_GEMM_MAX_M:
        out = FF._skinny_linear(a, q, b, "none", None, s)
        if out is not None:
            return _wrap(out)
    return FF.fused_matmul_bias(a, FF._w8_dequant(q, s, a.dtype), b)
