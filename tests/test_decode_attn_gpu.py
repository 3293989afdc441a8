"""Split-KV decode attention (csrc/kernels/decode_attn.hip, ops/hip.decode_attention) against a
plain fp32 PyTorch reference built from the same rounded inputs:
softmax((q + b) K^T scale + mask) V over the keys [0, ts], row ts being the new biased key and
value rounded to the storage dtype.

Bound (derived, not tuned): the kernels accumulate in fp32 and round the output once, so the
max-normalised error is at most one ulp of the largest element: 2^-8 in bf16, 2^-10 in fp16.
Every cache row above ts is NaN before the call, so a read beyond the time step poisons the
output; the cache itself is compared bitwise. The range guard of a device-side time step is
checked by reading the kernels, not by feeding them a bad value."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H = 2, 3
BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def _hip():
    from paddle_hackathon_amd.ops import hip
    return hip


def _shape():
    C = _hip().DECODE_ATTN_CHUNK
    return C, 2 * C + 40


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def _inputs(D, dtype, ts, seed=0, bias=True):
    """qkv, bias, cache with finite rows [0, ts) and NaN rows [ts, max_seq)"""
    _, max_seq = _shape()
    g = torch.Generator(device="cuda").manual_seed(1000 * D + ts + seed)
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).to(dtype)
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.5).to(dtype) if bias else None
    cache = torch.randn(2, B, H, max_seq, D, device="cuda", generator=g).to(dtype)
    cache[:, :, :, ts:] = float("nan")
    return qkv, qb, cache


def _ref(qkv, qb, cache, ts, mask=None, scale=None):
    """(fp32 output [B, 1, H * D], new key / value rows [2, B, H, D] in the storage dtype)"""
    D = qkv.shape[-1]
    x = qkv.float() + (qb.float() if qb is not None else 0.0)            # [B, 3, H, D]
    new = x[:, 1:].to(qkv.dtype).transpose(0, 1).contiguous()             # [2, B, H, D]
    k = torch.cat([cache[0, :, :, :ts].float(), new[0].float().unsqueeze(2)], 2)   # [B, H, ts + 1, D]
    v = torch.cat([cache[1, :, :, :ts].float(), new[1].float().unsqueeze(2)], 2)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    s = (x[:, 0].unsqueeze(2) @ k.transpose(-1, -2)) * sc                 # [B, H, 1, ts + 1]
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = torch.zeros(mask.shape, device=mask.device).masked_fill_(~mask, float("-inf"))
        s = s + mask.float()[..., :ts + 1]
    o = torch.softmax(s, -1) @ v                                          # [B, H, 1, D]
    return o.transpose(1, 2).reshape(B, 1, H * D), new


def _check(qkv, qb, cache, ts, mask=None, scale=None, time_step=None):
    hip = _hip()
    before = cache.clone()
    ref, new = _ref(qkv, qb, before, ts, mask, scale)
    out = hip.decode_attention(qkv, qb, cache, ts if time_step is None else time_step, mask=mask, scale=scale)
    torch.cuda.synchronize()
    assert out.shape == (B, 1, H * qkv.shape[-1]) and out.dtype == qkv.dtype
    err = _rel(out, ref)
    print(f"D={qkv.shape[-1]} {qkv.dtype} ts={ts}: rel err {err:.3e} (bound {BOUND[qkv.dtype]:.3e})")
    assert err <= BOUND[qkv.dtype]
    # row ts is the biased key / value rounded to the dtype; every other row is untouched (NaNs included)
    want = before.clone()
    want[:, :, :, ts] = new
    assert torch.equal(cache.view(torch.int16), want.view(torch.int16))
    return out


def _ts_cases():
    C, max_seq = _shape()
    return [0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, max_seq - 1]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("ti", range(8))
def test_sweep_matches_fp32_reference_and_updates_cache(ti, D, dtype):
    """a single key, both sides of every split seam, the last slot"""
    ts = _ts_cases()[ti]
    _check(*_inputs(D, dtype, ts), ts)


@pytest.mark.parametrize("D", [32, 64, 128])
def test_null_bias(D):
    C, _ = _shape()
    _check(*_inputs(D, torch.bfloat16, C + 5, bias=False), C + 5)


def test_explicit_scale():
    _check(*_inputs(64, torch.float16, 77), 77, scale=0.3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_mask_batch_broadcast_additive(dtype):
    """[B, 1, 1, ts + 1] with -1e4 on random keys; the new key stays unmasked"""
    C, _ = _shape()
    ts = C + 37
    g = torch.Generator(device="cuda").manual_seed(5)
    mask = torch.zeros(B, 1, 1, ts + 1, device="cuda")
    mask.masked_fill_(torch.rand(B, 1, 1, ts + 1, device="cuda", generator=g) < 0.4, -1e4)
    mask[..., ts] = 0.0
    _check(*_inputs(128, dtype, ts), ts, mask=mask)


@pytest.mark.parametrize("D", [32, 64, 128])
def test_mask_whole_split_minus_inf(D):
    """[B, H, 1, max_seq] with -inf on all of split 0 and some keys of split 1 (ts in split 1):
    split 0 hands (m = -inf, l = 0) to the combine kernel"""
    C, max_seq = _shape()
    ts = C + 50
    g = torch.Generator(device="cuda").manual_seed(6)
    mask = torch.zeros(B, H, 1, max_seq, device="cuda")
    mask[..., :C] = float("-inf")
    mask[..., C:].masked_fill_(torch.rand(B, H, 1, max_seq - C, device="cuda", generator=g) < 0.3, float("-inf"))
    mask[..., ts] = 0.0
    _check(*_inputs(D, torch.bfloat16, ts), ts, mask=mask)


def test_mask_boolean_keep():
    C, _ = _shape()
    ts = 2 * C + 3
    g = torch.Generator(device="cuda").manual_seed(7)
    keep = torch.rand(B, 1, 1, ts + 1, device="cuda", generator=g) < 0.6
    keep[..., ts] = True
    _check(*_inputs(64, torch.bfloat16, ts), ts, mask=keep)


@pytest.mark.parametrize("D", [32, 64, 128])
def test_device_time_step_is_bitwise_the_host_one_and_sync_free(D):
    C, max_seq = _shape()
    ts = C + 1
    qkv, qb, cache = _inputs(D, torch.bfloat16, ts)
    mask = torch.zeros(B, 1, 1, max_seq, device="cuda")
    mask[..., 3:40] = -1e4
    cache_dev = cache.clone()
    out_host = _check(qkv, qb, cache, ts, mask=mask)
    ts_dev = torch.tensor([ts], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out_dev = _hip().decode_attention(qkv, qb, cache_dev, ts_dev, mask=mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(out_dev.view(torch.int16), out_host.view(torch.int16))
    assert torch.equal(cache_dev.view(torch.int16), cache.view(torch.int16))


def test_rejections_need_no_launch():
    hip = _hip()
    _, max_seq = _shape()
    qkv, qb, cache = _inputs(64, torch.bfloat16, 4)
    before = cache.clone()
    for bad in (max_seq, -1):
        with pytest.raises(ValueError):
            hip.decode_attention(qkv, qb, cache, bad)
    with pytest.raises(ValueError):   # a mask shorter than ts + 1
        hip.decode_attention(qkv, qb, cache, 9, mask=torch.zeros(B, 1, 1, 9, device="cuda"))
    with pytest.raises(ValueError):   # device time step of the wrong dtype
        hip.decode_attention(qkv, qb, cache, torch.tensor([4], device="cuda"))
    with pytest.raises(ValueError):   # device time step with a mask that does not span the cache
        hip.decode_attention(qkv, qb, cache, torch.tensor([4], dtype=torch.int32, device="cuda"),
                             mask=torch.zeros(B, 1, 1, 9, device="cuda"))
    assert hip.decode_attn_supported(qkv, cache, None)
    assert not hip.decode_attn_supported(qkv, cache.float(), None)
    q80 = torch.zeros(B, 3, H, 80, device="cuda", dtype=torch.bfloat16)
    assert not hip.decode_attn_supported(q80, torch.zeros(2, B, H, 16, 80, device="cuda", dtype=torch.bfloat16), None)
    assert not hip.decode_attn_supported(qkv, cache[:, :1], None)                       # batch mismatch
    assert not hip.decode_attn_supported(qkv, cache, torch.zeros(B, H, 2, 8, device="cuda"))   # two query rows
    torch.cuda.synchronize()
    assert torch.equal(cache.view(torch.int16), before.view(torch.int16))
