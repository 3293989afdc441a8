"""Fused transformer functionals (reference: python/paddle/incubate/nn/functional/
fused_transformer.py, fused_matmul_bias.py).

The reference fuses these into single CUDA ops; here each maps onto the MI355X kernel set:
products with more than 16 rows (context stage, training) on hipBLASLt (with the bias folded into
the GEMM via ``addmm``); products with at most 16 rows that need no gradient (the decode stage,
small-batch ``fused_linear`` under ``no_grad``) on the weight-streaming kernels of
csrc/kernels/skinny_gemm.hip, which take bias, GELU / ReLU and the residual add in their epilogue
(``PHA_DECODE_GEMM=0`` keeps the library calls); attention on the
MFMA flash-attention HIP kernel when there is no arbitrary additive mask (masked attention
falls back to fused SDPA), LayerNorm / bias-GELU on the HIP kernels. Weight layouts and
return values follow the reference exactly (qkv_weight [3, H, D, E]; cache_kv
[2, B, H, S, D])."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as TF

from ...framework.core import Tensor, _wrap
from ... import ops as _ops

__all__ = ["fused_multi_head_attention", "fused_feedforward", "fused_multi_transformer", "fused_matmul_bias",
           "fused_linear", "fused_bias_dropout_residual_layer_norm"]


def _u(x):
    return None if x is None else (x._t if isinstance(x, Tensor) else x)


def _dropout(x, p, training, mode):
    if p == 0.0:
        return x
    if training:
        if mode in ("upscale_in_train", "upscale-in-train"):
            return TF.dropout(x, p, True)
        return x * (torch.rand_like(x) >= p).to(x.dtype)
    return x if mode in ("upscale_in_train", "upscale-in-train") else x * (1.0 - p)


def _ln(x, w, b, eps):
    if w is None and b is None:
        return TF.layer_norm(x, [x.shape[-1]], None, None, eps)
    w = w if w is not None else torch.ones(x.shape[-1], dtype=x.dtype, device=x.device)
    return _ops.fused.layer_norm(x, [x.shape[-1]], w.to(x.dtype) if w.dtype != x.dtype and w.dtype != torch.float32 else w,
                                 None if b is None else b.to(w.dtype), eps)


def _act(x, bias, activation):
    if activation == "gelu":
        return _ops.fused.bias_gelu(x, bias, False) if bias is not None else _ops.fused.gelu(x, False)
    if activation == "gelu_tanh":
        return _ops.fused.bias_gelu(x, bias, True) if bias is not None else _ops.fused.gelu(x, True)
    h = x + bias if bias is not None else x
    if activation == "relu":
        return torch.relu(h)
    raise ValueError(f"unsupported activation {activation}")


def _skinny_ok(x2, w, w_is_nk, bias=None, residual=None):
    """whether the product x2 [M, K] . w (+ bias, + residual) runs on the weight-streaming kernels
    (ops/hip.skinny_gemm): a GPU tensor on the HIP path, at most 16 rows, nothing that needs a
    gradient, and arguments the kernel takes. PHA_DECODE_GEMM=0 keeps the library call. More than 16
    rows (context stage, training) is no fallback; with at most 16 rows on the GPU, arguments the
    kernel cannot take are recorded as one (a shape class the measurements excluded is not)."""
    if not (isinstance(x2, torch.Tensor) and x2.is_cuda and x2.dim() == 2 and isinstance(w, torch.Tensor)
            and w.dim() == 2):
        return False
    if x2.shape[0] > _ops.hip.SKINNY_GEMM_MAX_M or x2.shape[0] < 1:
        return False
    if os.environ.get("PHA_DECODE_GEMM", "1") == "0" or not _ops.fused._use_hip(x2):
        return False
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x2, w, bias, residual)):
        return False
    if _ops.hip.skinny_gemm_supported(x2, w, w_is_nk, bias, residual):
        return True
    N, K = (w.shape[0], w.shape[1]) if w_is_nk else (w.shape[1], w.shape[0])
    if _ops.hip.skinny_gemm_excluded(N, K, w_is_nk, x2.shape[0]):
        return False
    from ...ops import fallback
    fallback.note("decode_gemm", f"{_ops.hip.skinny_gemm_why_not(x2, w, w_is_nk, bias, residual)} -> library GEMM")
    return False


def _skinny_linear(x, w, bias=None, act="none", residual=None):
    """act(x . w + bias) + residual for x [..., K] of at most 16 rows and w [K, N] on the
    weight-streaming kernels, or None where _skinny_ok keeps the product on today's path"""
    x2 = x.reshape(-1, x.shape[-1])
    r2 = None if residual is None else residual.reshape(-1, residual.shape[-1])
    if r2 is not None and not r2.is_contiguous():
        r2 = r2.contiguous()   # e.g. one token sliced out of a [B, T, E] input: at most 16 rows to copy
    if not _skinny_ok(x2, w, False, bias, r2):
        return None
    return _ops.hip.skinny_gemm(x2, w, False, bias, act, r2).reshape(*x.shape[:-1], w.shape[-1])


def fused_matmul_bias(x, y, bias=None, transpose_x=False, transpose_y=False, name=None):
    a, b = _u(x), _u(y)
    if (not transpose_x and a.is_cuda and a.dim() in (2, 3) and b.dim() == 2 and a.shape[-1] > 0
            and a.numel() // a.shape[-1] <= _ops.hip.SKINNY_GEMM_MAX_M):
        # at most 16 rows: the weight-streaming kernel reads y in either layout, no transposed copy
        a2 = a.reshape(-1, a.shape[-1])
        if _skinny_ok(a2, b, bool(transpose_y), _u(bias)):
            out = _ops.hip.skinny_gemm(a2, b, bool(transpose_y), _u(bias))
            return _wrap(out.reshape(*a.shape[:-1], out.shape[-1]))
    if transpose_x:
        a = a.transpose(-1, -2)
    if transpose_y:
        b = b.transpose(-1, -2)
    if bias is not None and a.dim() == 2:
        return _wrap(torch.addmm(_u(bias), a, b))
    out = torch.matmul(a, b)
    return _wrap(out + _u(bias) if bias is not None else out)


def fused_linear(x, weight, bias=None, transpose_weight=False, name=None):
    return fused_matmul_bias(x, weight, bias, False, transpose_weight)


def _linear(x, w, b):
    if b is not None:
        return torch.addmm(b, x.reshape(-1, x.shape[-1]), w).reshape(*x.shape[:-1], w.shape[-1])
    return x @ w


def fused_bias_dropout_residual_layer_norm(x, residual, bias=None, ln_scale=None, ln_bias=None, dropout_rate=0.5,
                                           ln_epsilon=1e-5, training=True, mode="upscale_in_train", name=None):
    h = _u(x)
    if mode in ("upscale_in_train", "upscale-in-train") or not training or dropout_rate == 0.0:
        # one fused HIP pass each way (ops/fused.py _BiasDropoutResidualLN); eval-mode upscale dropout is identity
        w = _u(ln_scale)
        w = w if w is not None else torch.ones(h.shape[-1], dtype=torch.float32, device=h.device)
        r = _u(residual)
        return _wrap(_ops.fused.bias_dropout_residual_layer_norm(h.contiguous(), r.contiguous().to(h.dtype), _u(bias), w,
                                                                 _u(ln_bias), dropout_rate, training, ln_epsilon))
    if bias is not None:
        h = h + _u(bias)
    h = _dropout(h, dropout_rate, training, mode) + _u(residual)
    return _wrap(_ln(h, _u(ln_scale), _u(ln_bias), ln_epsilon))


def fused_feedforward(x, linear1_weight, linear2_weight, linear1_bias=None, linear2_bias=None, ln1_scale=None,
                      ln1_bias=None, ln2_scale=None, ln2_bias=None, dropout1_rate=0.5, dropout2_rate=0.5,
                      activation="relu", ln1_epsilon=1e-5, ln2_epsilon=1e-5, pre_layer_norm=False, training=True,
                      mode="upscale_in_train", ring_id=-1, add_residual=True, name=None):
    t = _u(x)
    residual = t
    h = _ln(t, _u(ln1_scale), _u(ln1_bias), ln1_epsilon) if pre_layer_norm else t
    h = _act(h @ _u(linear1_weight), _u(linear1_bias), activation)
    h = _dropout(h, dropout1_rate, training, mode)
    h = _linear(h, _u(linear2_weight), _u(linear2_bias))
    if ring_id >= 0:
        from ...parallel import collective as C
        torch.distributed.all_reduce(h)
    if (not pre_layer_norm and add_residual and
            (mode in ("upscale_in_train", "upscale-in-train") or not training or dropout2_rate == 0.0)):
        w = _u(ln2_scale)
        w = w if w is not None else torch.ones(h.shape[-1], dtype=torch.float32, device=h.device)
        return _wrap(_ops.fused.bias_dropout_residual_layer_norm(h.contiguous(), residual.contiguous(), None, w,
                                                                 _u(ln2_bias), dropout2_rate, training, ln2_epsilon))
    h = _dropout(h, dropout2_rate, training, mode)
    if add_residual:
        h = residual + h
    if not pre_layer_norm:
        h = _ln(h, _u(ln2_scale), _u(ln2_bias), ln2_epsilon)
    return _wrap(h)


def _attention(q, k, v, mask, attn_dropout, training, mode, causal=False):
    """q/k/v: [B, H, S, D]. The flash kernels (mask and upscale-in-train dropout in-kernel); the
    downscale-in-infer dropout mode keeps the explicit composite."""
    if mode in ("upscale_in_train", "upscale-in-train") or attn_dropout == 0.0 or not training:
        o = _ops.fused.flash_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), causal=causal,
                                       dropout_p=attn_dropout, training=training, mask=mask)
        return o.transpose(1, 2)
    if mode not in ("upscale_in_train", "upscale-in-train") and attn_dropout > 0:
        s = (q @ k.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
        if mask is not None:
            s = s + mask
        p = _dropout(torch.softmax(s.float(), -1).to(q.dtype), attn_dropout, training, mode)
        return p @ v
    return TF.scaled_dot_product_attention(q, k, v, attn_mask=mask.to(q.dtype) if mask is not None else None,
                                           dropout_p=attn_dropout if training else 0.0, is_causal=causal and mask is None)


def fused_multi_head_attention(x, qkv_weight, linear_weight, pre_layer_norm=False, pre_ln_scale=None,
                               pre_ln_bias=None, ln_scale=None, ln_bias=None, pre_ln_epsilon=1e-05, qkv_bias=None,
                               linear_bias=None, cache_kv=None, attn_mask=None, dropout_rate=0.5,
                               attn_dropout_rate=0.5, ln_epsilon=1e-05, training=True, mode="upscale_in_train",
                               ring_id=-1, add_residual=True, name=None):
    t = _u(x)
    B, S, E = t.shape
    w = _u(qkv_weight)  # [3, H, D, E]
    _, H, D, _ = w.shape
    residual = t
    h = _ln(t, _u(pre_ln_scale), _u(pre_ln_bias), pre_ln_epsilon) if pre_layer_norm else t
    qkv = h.reshape(B * S, E) @ w.reshape(3 * H * D, E).t()
    if qkv_bias is not None:
        qkv = qkv + _u(qkv_bias).reshape(-1)
    qkv = qkv.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)  # [3, B, H, S, D]
    q, k, v = qkv[0], qkv[1], qkv[2]
    cache_out = None
    if cache_kv is not None:
        c = _u(cache_kv)
        k = torch.cat([c[0], k], 2)
        v = torch.cat([c[1], v], 2)
        cache_out = torch.stack([k, v], 0)
    o = _attention(q, k, v, _u(attn_mask), attn_dropout_rate, training, mode)
    o = o.transpose(1, 2).reshape(B, S, H * D)
    o = _linear(o, _u(linear_weight), _u(linear_bias))
    if ring_id >= 0:
        torch.distributed.all_reduce(o)
    o = _dropout(o, dropout_rate, training, mode)
    if add_residual:
        o = residual + o
    if not pre_layer_norm:
        o = _ln(o, _u(ln_scale), _u(ln_bias), ln_epsilon)
    if cache_kv is not None:
        return _wrap(o), _wrap(cache_out)
    return _wrap(o)


def _decode_kernel_ok(qkv, cache, mask, device_time_step, dropout_rate, training, cache_indirection=None, beam_size=1):
    """whether one decode step's attention (qkv [B, 3, H, D], the layer's cache) runs on the split-KV
    decode kernels (ops/hip.decode_attention). PHA_DECODE_ATTN=0 keeps the composite; on the GPU
    every other reason to keep it is recorded as a fallback."""
    if not qkv.is_cuda or os.environ.get("PHA_DECODE_ATTN", "1") == "0" or not _ops.fused._use_hip(qkv):
        return False
    if training and dropout_rate != 0.0:
        reason = "attention dropout"
    elif torch.is_grad_enabled() and qkv.requires_grad:
        reason = "needs a gradient (the decode kernels have no backward; run generation under no_grad)"
    elif not _ops.hip.decode_attn_supported(qkv, cache, mask, device_time_step, cache_indirection, beam_size):
        reason = (f"{qkv.dtype} D={qkv.shape[-1]} cache {cache.dtype} {tuple(cache.shape)} "
                  f"mask={None if mask is None else tuple(mask.shape)}")
    else:
        return True
    from ...ops import fallback
    fallback.note("decode_attention", reason + " -> composite on the flash kernels")
    return False


def _decode_rows_composite(q, k, v, c, ts_rows, mask, dropout_rate, training, mode):
    """the decode stage's attention with a step per batch row, on the composite: q / k / v [B, H, 1, D]
    of the new token, ``c`` the layer's [2, B, H, max_seq, D] cache, ``ts_rows`` int32 [B] on the
    cache's device. Row b appends at ts_rows[b] and attends over [0, ts_rows[b]]. Keys and values
    above a row's step are replaced by zeros before the products (an additive -inf would leave a NaN
    score NaN), so the result does not depend on what the cache holds there. On the GPU the key
    dimension is the whole cache: the host never learns max(ts_rows). As in the kernels, a row whose
    step is outside the cache leaves it alone and gets NaN."""
    B, max_seq = c.shape[1], c.shape[3]
    idx = ts_rows.reshape(-1).long()
    ok = ((idx >= 0) & (idx < max_seq))[:, None, None]
    idx = idx.clamp(0, max_seq - 1)
    rows = torch.arange(B, device=c.device)
    c[0][rows, :, idx] = torch.where(ok, k[:, :, 0], c[0][rows, :, idx])
    c[1][rows, :, idx] = torch.where(ok, v[:, :, 0], c[1][rows, :, idx])
    q = torch.where(ok[..., None], q, torch.full((), float("nan"), dtype=q.dtype, device=q.device))
    L = max_seq if c.is_cuda else min(max_seq, int(idx.max()) + 1)
    live = torch.arange(L, device=c.device)[None, :] <= idx[:, None]             # [B, L]
    zero = torch.zeros((), dtype=c.dtype, device=c.device)
    kk = torch.where(live[:, None, :, None], c[0, :, :, :L], zero)
    vv = torch.where(live[:, None, :, None], c[1, :, :, :L], zero)
    m = torch.zeros(B, 1, 1, L, dtype=torch.float32, device=c.device).masked_fill_(~live[:, None, None, :],
                                                                                   float("-inf"))
    if mask is not None:
        um = mask
        if um.dtype == torch.bool:
            um = torch.zeros(um.shape, dtype=torch.float32, device=um.device).masked_fill_(~um, float("-inf"))
        if um.shape[-1] != 1:
            um = um[..., :L]
        m = m + um.to(device=c.device, dtype=torch.float32)
    return _attention(q, kk, vv, m.to(q.dtype), dropout_rate, training, mode, causal=False)


def _decode_beam_composite(q, k, v, c, ts_rows, ind, beam, mask, dropout_rate, training, mode):
    """the decode stage's attention through a cache-indirection table, on the composite: as
    _decode_rows_composite, with row b's key position t < ts_rows[b] taken from cache row
    ``(b // beam) * beam + ind[b, t]``. The new key and value are appended to row b's own cache row;
    each row's history is gathered through the table into a temporary [2, B, H, max_seq, D] and
    _decode_rows_composite's arithmetic runs on that. A table entry outside [0, beam) leaves its key
    out (zeroed and masked); the entry at ts_rows[b] is not read. No host sync on the GPU."""
    B, max_seq = c.shape[1], c.shape[3]
    idx = ts_rows.reshape(-1).long()
    ok = ((idx >= 0) & (idx < max_seq))[:, None, None]
    at = idx.clamp(0, max_seq - 1)
    rows = torch.arange(B, device=c.device)
    c[0][rows, :, at] = torch.where(ok, k[:, :, 0], c[0][rows, :, at])
    c[1][rows, :, at] = torch.where(ok, v[:, :, 0], c[1][rows, :, at])
    t = torch.arange(max_seq, device=c.device)
    below = t[None, :] < idx[:, None]                                                  # [B, max_seq]
    valid = (ind >= 0) & (ind < beam) | ~below
    src = torch.where(below, (rows // beam * beam)[:, None] + ind.long().clamp(0, beam - 1), rows[:, None])
    zero = torch.zeros((), dtype=c.dtype, device=c.device)
    # the two index tensors are split by a slice, so their [B, max_seq] comes first: [B, max_seq, 2, H, D]
    tmp = torch.where(valid[:, :, None, None, None], c[:, src, :, t[None, :]], zero).permute(2, 0, 3, 1, 4).contiguous()
    extra = torch.zeros(B, 1, 1, max_seq, dtype=torch.float32, device=c.device).masked_fill_(
        ~valid[:, None, None, :], float("-inf"))
    if mask is not None:
        um = mask
        if um.dtype == torch.bool:
            um = torch.zeros(um.shape, dtype=torch.float32, device=um.device).masked_fill_(~um, float("-inf"))
        um = um.to(device=c.device, dtype=torch.float32)
        while um.dim() < 4:
            um = um.unsqueeze(0)
        if um.shape[-1] != 1 and um.shape[-1] < max_seq:
            extra = extra[..., :um.shape[-1]]
        extra = extra + um
    return _decode_rows_composite(q, k, v, tmp, ts_rows, extra, dropout_rate, training, mode)


def fused_multi_transformer(x, ln_scales, ln_biases, qkv_weights, qkv_biases, linear_weights, linear_biases,
                            ffn_ln_scales, ffn_ln_biases, ffn1_weights, ffn1_biases, ffn2_weights, ffn2_biases,
                            pre_layer_norm=True, epsilon=1e-05, cache_kvs=None, time_step=None, attn_mask=None,
                            dropout_rate=0.0, activation="gelu", training=False, mode="upscale_in_train",
                            trans_qkvw=True, ring_id=-1, name=None, cache_indirection=None, beam_size=1):
    """Stack of pre-LN decoder layers for generation. ``cache_kvs[i]`` is a preallocated
    [2, B, H, max_seq, D] buffer updated in place: context stage (time_step None) writes
    positions [0, S); decode stage (S == 1) writes position ``time_step`` and attends over
    [0, time_step]. On the GPU (bf16 / fp16, head dim 32 / 64 / 128, no dropout, no gradient) the
    decode stage's bias add, cache append and attention are one split-KV kernel pair
    (csrc/kernels/decode_attn.hip); with ``time_step`` an int32 device tensor that step reads it on
    the device, so it neither syncs the host nor changes shape and can be captured in a hipGraph.
    ``time_step`` may also be an int32 tensor of B elements (B > 1; on the GPU a device tensor, on the
    CPU a CPU tensor): batch row b then writes position ``time_step[b]`` and attends over
    [0, time_step[b]], whatever the cache holds above it, on the kernel pair and on the composite
    alike and without a host sync, so right-padded prompts of different lengths decode in one batch.
    PHA_DECODE_ATTN=0 keeps the composite. With at most 16 rows (B * S <= 16) and no gradient the four
    products of each layer run on the weight-streaming kernels (csrc/kernels/skinny_gemm.hip): QKV in
    either ``trans_qkvw`` layout without a transposed copy, the output projection and ffn2 with bias
    and residual add in the epilogue (where dropout is an identity and ``ring_id < 0``), ffn1 with bias + GELU / ReLU.
    ``activation`` is "gelu" (erf), "gelu_tanh" (the tanh approximation the GPT model trains with) or "relu".
    PHA_DECODE_GEMM=0 keeps the library GEMMs and the separate elementwise passes.

    ``cache_indirection`` (contiguous int32 [B, max_seq] on the device of ``x``) with ``beam_size`` K
    (it divides B) serves beam search and applies to the decode stage only (anything else is a
    ``ValueError``): the B rows are groups of K consecutive beams that share one step, and row b reads
    key position t < time_step from cache row ``(b // K) * K + cache_indirection[b, t]`` of every
    layer's cache, while the new key and value go to row b's own cache row. The kernel pair takes the
    table as it is (``ops.hip.decode_attention``); the composite gathers each row's keys and values
    through it into a temporary, without a host sync on the GPU. A scalar ``time_step`` is broadcast
    to the B rows."""
    h = _u(x)
    B, S, E = h.shape
    ts = ts_dev = ts_rows = None
    if time_step is not None:
        t = _u(time_step)
        if isinstance(t, torch.Tensor) and t.numel() > 1:
            # a step per batch row, on the device the layers run on; never read on the host
            if t.dtype != torch.int32 or t.numel() != B or t.device != h.device or S != 1 or cache_kvs is None:
                raise ValueError(f"fused_multi_transformer: a time_step of more than one element must be int32 [{B}] "
                                 f"on {h.device} in the decode stage, got {t.dtype} {tuple(t.shape)} on {t.device}")
            ts_rows = t.reshape(-1).contiguous()
            if t.is_cuda:
                ts_dev = ts_rows
        elif isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() == 1:
            ts_dev = t   # read by the decode kernel on the device; .item() only if a layer cannot use it
        else:
            ts = int(t.reshape(-1)[0].item()) if isinstance(t, torch.Tensor) else int(t)
    mask = _u(attn_mask)
    decode = cache_kvs is not None and time_step is not None and S == 1
    ind = _u(cache_indirection)
    if ind is None:
        if beam_size != 1:
            raise ValueError(f"fused_multi_transformer: beam_size={beam_size!r} needs a cache_indirection table")
    else:
        if not decode:
            raise ValueError("fused_multi_transformer: cache_indirection applies to the decode stage only "
                             "(cache_kvs, a time_step and one new token per row)")
        why = _ops.hip._cache_indirection_why_not(ind, beam_size, B, _u(cache_kvs[0]).shape[3], h.device)
        if why is not None:
            raise ValueError(f"fused_multi_transformer: {why}")
        if ts_rows is None:   # the table's paths take a step per row
            ts_rows = ts_dev.reshape(1).expand(B).contiguous() if ts_dev is not None \
                else torch.full((B,), ts, dtype=torch.int32, device=h.device)
            ts = None
            if h.is_cuda:
                ts_dev = ts_rows
    # at most 16 rows: the products may run on the weight-streaming kernels (_skinny_ok decides each)
    skinny = isinstance(h, torch.Tensor) and h.is_cuda and B * S <= _ops.hip.SKINNY_GEMM_MAX_M
    # bias and residual add go into the epilogue only where nothing stands between them and the product
    # (dropout an identity: rate 0, or inference in the upscale-in-train mode; no all-reduce)
    epi = skinny and ring_id < 0 and (dropout_rate == 0 or
                                      (not training and mode in ("upscale_in_train", "upscale-in-train")))
    for i in range(len(qkv_weights)):
        residual = h
        a = _ln(h, _u(ln_scales[i]), _u(ln_biases[i]), epsilon) if pre_layer_norm else h
        w = _u(qkv_weights[i])
        if trans_qkvw:  # [3, H, D, E]
            _, H, D, _ = w.shape
            w2 = w.reshape(3 * H * D, E)
        else:  # [E, 3, H, D]
            _, _, H, D = w.shape
            w2 = w.reshape(E, 3 * H * D)
        a2 = a.reshape(B * S, E)
        qb = _u(qkv_biases[i]) if qkv_biases is not None and qkv_biases[i] is not None else None
        if skinny and _skinny_ok(a2, w2, trans_qkvw):
            # nothing here needs a gradient, so a stand-in of the product's shape and dtype picks the
            # attention path first: the decode kernels add the QKV bias themselves, anywhere else it
            # goes into this product's epilogue
            use_decode = decode and _decode_kernel_ok(a2.as_strided((B, 3, H, D), (0, 0, 0, 0)), _u(cache_kvs[i]), mask,
                                                      ts_dev if ts_dev is not None else False, dropout_rate,
                                                      training, ind, beam_size)
            qbe = None if use_decode or qb is None else qb.reshape(-1)
            if qbe is not None and not _ops.hip.skinny_gemm_supported(a2, w2, trans_qkvw, qbe):
                qbe = None   # added below as today
            qkv = _ops.hip.skinny_gemm(a2, w2, trans_qkvw, qbe)
            if qbe is not None:
                qb = None
        else:
            qkv = a2 @ (w2.t() if trans_qkvw else w2)
            use_decode = decode and _decode_kernel_ok(qkv.reshape(B, 3, H, D), _u(cache_kvs[i]), mask,
                                                      ts_dev if ts_dev is not None else False, dropout_rate, training,
                                                      ind, beam_size)
        if use_decode:
            # one split-KV kernel pair: bias add, cache append and attention over [0, time_step]
            if qb is not None and (qb.dtype != qkv.dtype or not qb.is_contiguous()):
                qb = qb.to(qkv.dtype).contiguous()
            if ind is not None:
                o = _ops.hip.decode_attention(qkv.reshape(B, 3, H, D), None if qb is None else qb.reshape(3, H, D),
                                              _u(cache_kvs[i]), ts_dev, mask, cache_indirection=ind,
                                              beam_size=beam_size)
            else:
                o = _ops.hip.decode_attention(qkv.reshape(B, 3, H, D), None if qb is None else qb.reshape(3, H, D),
                                              _u(cache_kvs[i]), ts_dev if ts_dev is not None else ts, mask)
        else:
            if ts_dev is not None and ts is None and ts_rows is None:
                ts = int(ts_dev.item())
            if qb is not None:
                qkv = qkv + qb.reshape(-1)
            qkv = qkv.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
            q, k, v = qkv[0], qkv[1], qkv[2]
            causal = False
            if ind is not None:
                o = _decode_beam_composite(q, k, v, _u(cache_kvs[i]), ts_rows, ind, beam_size, mask, dropout_rate,
                                           training, mode)
            elif ts_rows is not None:
                o = _decode_rows_composite(q, k, v, _u(cache_kvs[i]), ts_rows, mask, dropout_rate, training, mode)
            elif cache_kvs is not None:
                c = _u(cache_kvs[i])
                if ts is None:
                    c[0, :, :, :S] = k
                    c[1, :, :, :S] = v
                    causal = mask is None
                else:
                    c[0, :, :, ts:ts + S] = k
                    c[1, :, :, ts:ts + S] = v
                    k, v = c[0, :, :, :ts + S], c[1, :, :, :ts + S]
            if ts_rows is None:
                m = mask
                if m is not None and m.shape[-1] != k.shape[2]:
                    m = m[..., :k.shape[2]]
                o = _attention(q, k, v, m, dropout_rate, training, mode, causal=causal and S > 1)
            o = o.transpose(1, 2).reshape(B, S, H * D)
        lw, lb = _u(linear_weights[i]), _u(linear_biases[i]) if linear_biases is not None else None
        o2 = _skinny_linear(o, lw, lb, "none", residual if epi else None) if skinny else None
        if o2 is not None and epi:
            h = o2
        else:
            o = o2 if o2 is not None else _linear(o, lw, lb)
            if ring_id >= 0:
                torch.distributed.all_reduce(o)
            h = residual + _dropout(o, dropout_rate, training, mode)
        if not pre_layer_norm:
            h = _ln(h, _u(ln_scales[i]), _u(ln_biases[i]), epsilon)
        residual = h
        f = _ln(h, _u(ffn_ln_scales[i]), _u(ffn_ln_biases[i]), epsilon) if pre_layer_norm else h
        w1, b1 = _u(ffn1_weights[i]), _u(ffn1_biases[i]) if ffn1_biases is not None else None
        f1 = _skinny_linear(f, w1, b1, activation) if skinny and activation in ("gelu", "gelu_tanh", "relu") else None
        f = f1 if f1 is not None else _act(f @ w1, b1, activation)
        w2f, b2 = _u(ffn2_weights[i]), _u(ffn2_biases[i]) if ffn2_biases is not None else None
        f2 = _skinny_linear(f, w2f, b2, "none", residual if epi else None) if skinny else None
        if f2 is not None and epi:
            h = f2
        else:
            f = f2 if f2 is not None else _linear(f, w2f, b2)
            if ring_id >= 0:
                torch.distributed.all_reduce(f)
            h = residual + _dropout(f, dropout_rate, training, mode)
        if not pre_layer_norm:
            h = _ln(h, _u(ffn_ln_scales[i]), _u(ffn_ln_biases[i]), epsilon)
    if cache_kvs is not None:
        return _wrap(h), cache_kvs
    return _wrap(h)
