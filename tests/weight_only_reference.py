"""The reference of the weight-only int8 tests: ``dequantised_copy(model)`` is a copy of a GPT with the four matrices
of every layer replaced by dequantize(quantize(w))."""
import copy

import torch

from paddle_hackathon_amd.nn import quant


def dequantised_copy(model):
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for layer in ref.gpt.layers:
            for lin in (layer.self_attn.qkv_proj, layer.self_attn.out_proj, layer.mlp.linear1, layer.mlp.linear2):
                lin.weight._t.copy_(quant.weight_dequantize(*quant.weight_quantize(lin.weight), "float32")._t)
    return ref
