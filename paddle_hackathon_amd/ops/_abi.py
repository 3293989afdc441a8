"""The C ABI of ``libpha_kernels.so``: one table of ctypes signatures, one set of call helpers.

Every ``PHA_API`` function in ``csrc/kernels/*.hip`` has exactly one entry in ``SIGNATURES``;
``_lib._load()`` applies the table to the library right after ``CDLL``, so a call with a wrong
argument type raises ``ctypes.ArgumentError`` instead of handing the kernel a truncated stride or
pointer. ``tests/test_kernel_abi.py`` compares the table with the prototypes in the sources: a
new entry point needs its line here and nothing else.

Codes: ``I`` int, ``LG`` long, ``F`` float, ``U`` unsigned, ``P`` any pointer (tensors, structs,
``int*`` out-parameters, ``hipStream_t``).
"""
from __future__ import annotations

from ctypes import c_float as F, c_int as I, c_long as LG, c_uint as U, c_void_p as P

import torch

# name -> (restype, [argtypes]), grouped by source file
SIGNATURES = {
    # batch_norm.hip
    "pha_bn_num_blocks": (I, [LG, I]),
    "pha_bn_fwd_train": (I, [I, P, P, P, LG, I, P, P, P, P, P, P, P, P, P, F, F, I, P, I, P]),
    "pha_bn_apply": (I, [I, P, P, P, LG, I, P, P, I, P]),
    "pha_bn_bwd": (I, [I, P, P, P, LG, I, P, P, P, P, P, P, P, P, P, I, P, P, I, P]),
    # beam_search.hip
    "pha_beam_search_max_v": (I, []),
    "pha_beam_search_max_k": (I, []),
    "pha_beam_search_step": (I, [I, P, LG, P, P, P, P, P, P, P, P, P, P, I, I, I, LG, I, P]),
    # ce_gelu_embed.hip
    "pha_softmax_ce_fwd": (I, [I, P, P, P, P, LG, I, I, P]),
    "pha_softmax_ce_bwd": (I, [I, P, P, P, P, P, LG, I, I, P]),
    "pha_bias_gelu_fwd": (I, [I, P, P, P, LG, I, I, P]),
    "pha_bias_gelu_bwd": (I, [I, P, P, P, P, LG, I, I, P]),
    "pha_bias_gelu_bwd_rows": (I, [I, P, P, P, P, I, I, I, I, P]),
    "pha_bias_gelu_bwd_db": (I, [I, P, P, P, P, P, I, I, I, I, P]),
    "pha_col_sum_partial": (I, [I, P, P, I, I, I, P]),
    "pha_transpose16_batch": (I, [I, P, P, P, P, P]),
    "pha_transpose16": (I, [P, P, I, I, P]),
    "pha_maxpool2d_nhwc_fwd": (I, [I, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "pha_maxpool2d_nhwc_bwd": (I, [I, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "pha_embedding_bwd": (I, [I, P, P, P, LG, I, LG, LG, P, I, P]),
    "pha_embedding_fwd": (I, [P, P, P, LG, I, LG, P]),
    "pha_seed_bump": (I, [P, P, P]),
    # decode_attn.hip
    "pha_decode_attn_chunk": (I, []),
    "pha_decode_attn": (I, [I, P, P, P, P, LG, LG, F, I, P, P, P, I, I, I, I, P]),
    "pha_decode_attn_rows": (I, [I, P, P, P, P, LG, LG, F, P, P, P, I, I, I, I, P]),
    "pha_decode_attn_beam": (I, [I, P, P, P, P, LG, LG, F, P, P, I, P, P, I, I, I, I, P]),
    # flash_attn.hip
    "pha_flash_attn_fwd_ext": (I, [I, P, P, P, P, P, I, I, I, I, I, I, F, I, P, LG, LG, LG, F, U, P, P]),
    "pha_flash_attn_bwd_ext": (I, [I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, F, I, P, LG, LG, LG, F, U, P, LG,
                                   I, LG, I, P]),
    "pha_flash_attn_fwd": (I, [I, P, P, P, P, P, I, I, I, I, I, I, F, I, P]),
    "pha_flash_attn_bwd_preprocess": (I, [I, P, P, P, I, I, I, I, P]),
    "pha_flash_attn_bwd": (I, [I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, F, I, P]),
    "pha_flash_attn_bwd_packed_od": (I, [I, P, P, P, P, P, P, I, I, I, I, F, I, P]),
    "pha_flash_attn_fwd_packed": (I, [I, P, P, P, I, I, I, I, F, I, P]),
    "pha_flash_attn_bwd_packed": (I, [I, P, P, P, P, P, I, I, I, I, F, I, P]),
    # flash_attn_bwd.hip
    "pha_flash_attn_bwd_fused": (I, [I, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, F, I, P]),
    "pha_flash_attn_bwd_packed_fused": (I, [I, P, P, P, P, P, P, I, I, I, I, F, I, P]),
    # flash_attn_d64.hip
    "pha_fa64_mask_words": (I, [I]),
    "pha_fa64_mask_size": (LG, [I, I, I, I]),
    "pha_fa64_fwd": (I, [I, P, P, P, P, P, I, I, I, I, I, F, I, LG, I, LG, I, LG, I, F, U, P, P, P, P, LG, LG, LG]),
    "pha_fa64_bwd": (I, [I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, F, I, LG, I, LG, I, LG, I, LG, I, LG, I, F, U,
                         P, P, P, P, LG, LG, LG]),
    # gemm256.hip
    "pha_gemm256_nt": (I, [I, P, P, P, P, LG, LG, LG, LG, LG, LG, I, P, I, I, P]),
    "pha_conv256_fwd": (I, [I, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, P, P, P, P, P, P, P,
                            I, P, P]),
    "pha_conv256_fwd_grouped": (I, [I, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, I, LG, I, P, I, I, P, P]),
    "pha_conv256_wgrad_grouped": (I, [I, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, P]),
    "pha_conv256_fwd_f32out": (I, [I, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, P, P]),
    "pha_gemm256_tn": (I, [I, P, P, P, P, LG, LG, LG, LG, LG, I, I, P, I, I, P]),
    "pha_conv256_wgrad": (I, [I, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, P]),
    # gemm4p.hip
    "pha_gemm4p_batched": (I, [I, P, P, P, LG, LG, LG, LG, LG, LG, I, I, I, I, P, I, I, P, I, P, P, I, LG, LG, LG]),
    "pha_gemm4p": (I, [I, P, P, P, LG, LG, LG, LG, LG, LG, I, I, I, I, P, I, I, P, I, P, P]),
    # gemm4w.hip
    "pha_gemm4w": (I, [I, P, P, P, LG, LG, LG, LG, LG, LG, I, I, I, P, P, LG, P, I, P]),
    "pha_colsum_finish": (I, [I, P, P, I, I, P]),
    # gemm8p.hip
    "pha_gemm8p": (I, [I, P, P, P, P, LG, LG, LG, LG, LG, LG, I, I, I, P, I, P, P]),
    # gemm8w.hip
    "pha_gemm8w": (I, [I, P, P, P, LG, LG, LG, LG, LG, LG, I, P, I, P]),
    # gemm_conv.hip
    "pha_gemm": (I, [I, I, I, I, P, LG, P, LG, P, LG, P, LG, LG, LG, I, P, P, P, P]),
    # gpu_ps.hip
    "pha_ps_gpu_find": (I, [P, P, LG, P, P, LG, P, I, I, P, P, I, U, F, P]),
    "pha_ps_gpu_adagrad": (I, [P, P, LG, P, P, I, F, F, F, F, P]),
    # grouped_conv.hip
    "pha_gconv_fwd": (I, [I, P, P, P, P, P, P]),
    "pha_gconv_dgrad": (I, [I, P, P, P, P, P]),
    "pha_gconv_wgrad_ws": (LG, [P, I]),
    "pha_gconv_wgrad_items": (LG, [P]),
    "pha_gconv_wgrad": (I, [I, P, P, P, P, P, I, P]),
    # lamb.hip
    "pha_lamb_sq": (I, [P, LG, P, P, P]),
    "pha_lamb_moment": (I, [P, P, P, P, P, P, P, I, LG, F, F, F, F, F, F, F, P, P]),
    "pha_lamb_apply": (I, [P, P, P, P, P, I, LG, F, P, P]),
    # norm_softmax.hip
    "pha_layer_norm_fwd2": (I, [I, I, P, P, P, P, P, P, P, P, I, I, F, P]),
    "pha_layer_norm_bwd_nblocks": (I, [I, I]),
    "pha_bdrln_fwd2": (I, [I, I, I, P, P, P, P, P, P, P, P, P, I, I, F, U, U, F, P, P]),
    "pha_bdrln_fwd": (I, [I, I, P, P, P, P, P, P, P, P, P, I, I, F, U, U, F, P]),
    "pha_layer_norm_fwd": (I, [I, I, P, P, P, P, P, P, I, I, F, P]),
    "pha_col_sum_rows": (I, [I, P, P, I, I, P]),
    "pha_layer_norm_bwd2": (I, [I, I, P, P, P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "pha_layer_norm_dropout_bwd": (I, [I, I, P, P, P, P, P, P, P, P, P, P, P, I, I, I, U, U, F, P, P]),
    "pha_layer_norm_bwd3": (I, [I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "pha_layer_norm_bwd": (I, [I, I, P, P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "pha_dropout_bias_bwd": (I, [I, I, P, P, P, P, I, I, I, U, U, F, P, P]),
    "pha_softmax_fwd": (I, [I, P, P, I, I, P]),
    "pha_softmax_bwd": (I, [I, P, P, P, I, I, P]),
    # optim.hip
    "pha_chunk_size": (I, []),
    "pha_tensor_meta_size": (I, []),
    "pha_multi_tensor_adam": (I, [I, I, P, P, I, F, F, F, F, F, F, F, I, P, P, P, P, P]),
    "pha_multi_tensor_momentum": (I, [I, I, P, P, I, F, F, F, I, P]),
    "pha_multi_tensor_l2sq": (I, [P, P, I, P, P, P]),
    # quant.hip
    "pha_quant_absmax": (I, [I, P, LG, P, P]),
    "pha_quant_channel_absmax": (I, [I, P, LG, LG, LG, P, P]),
    "pha_quant_dequant": (I, [I, I, P, P, LG, LG, LG, P, I, I, I, P]),
    "pha_quant_moving_avg": (I, [P, P, P, P, F, P]),
    # rnn.hip
    "pha_rnn_fwd": (I, [I, I, I, I, P, P, P, P, P, P, P, P, I, P]),
    "pha_rnn_bwd": (I, [I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, I, P]),
    # sampling.hip
    "pha_sample_logits_max_v": (I, []),
    "pha_sample_logits": (I, [I, P, LG, P, P, P, P, I, I, F, I, F, LG, LG, P]),
    # skinny_gemm.hip
    "pha_skinny_gemm_tile": (I, [I, P, P]),
    "pha_skinny_gemm_plan": (I, [I, I, I, P, P]),
    "pha_skinny_gemm": (I, [I, I, P, LG, P, P, P, P, P, I, I, I, I, I, I, P]),
    # split.hip
    "pha_split3_f32": (I, [P, P, LG, LG, I, P]),
}


def declare(L):
    """set restype / argtypes of every table entry on the loaded library ``L``; a name it does not
    export is an error (the library is always built from this tree's sources)"""
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            raise RuntimeError(f"{L._name} does not export {name} (declared in ops/_abi.py)") from None
        f.restype, f.argtypes = restype, argtypes


DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}   # the kernels' dtype codes


def ptr(t):
    """device address of a tensor, or a null pointer for None"""
    return None if t is None else t.data_ptr()


def stream(t):
    """the current torch HIP stream of the tensor's device (launches order with torch's own work)"""
    return torch.cuda.current_stream(t.device).cuda_stream


def check(rc, name):
    if rc != 0:
        raise RuntimeError(f"{name} failed with hipError {rc}")
