"""Decode attention over an int8 KV cache (csrc/kernels/decode_attn_q8.hip) against float64 attention over
``q8 * scale``, the new row quantised by the torch rule from the biased key / value rounded to the storage dtype.
Bound (derived, as in tests/test_decode_attn_gpu.py): exact fp32 operands, fp32 accumulation, one rounding of the
output: at most one ulp of the output dtype, max-normalised. Scales at or above the step are NaN before the call,
so a read beyond it poisons the output; the int8 rows there are a sentinel; cache and scales are compared bitwise."""
import math

import pytest
import torch

from paddle_hackathon_amd.ops import hip

pytestmark = pytest.mark.gpu

H, C = 3, hip.DECODE_ATTN_CHUNK
max_seq = 2 * C + 40
BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def _inputs(D, dtype, steps, bias=True):
    """qkv, bias, int8 cache and scales; row b is live on [0, steps[b]), sentinel / NaN above"""
    B = len(steps)
    g = torch.Generator(device="cuda").manual_seed(1000 * D + steps[0])
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).to(dtype)
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.5).to(dtype) if bias else None
    cache = torch.randint(-128, 128, (2, B, H, max_seq, D), device="cuda", generator=g).to(torch.int8)
    scales = torch.rand(2, B, H, max_seq, device="cuda", generator=g) * 0.02 + 0.001
    for b, ts in enumerate(steps):
        cache[:, b, :, ts:] = -77
        scales[:, b, :, ts:] = float("nan")
    return qkv, qb, cache, scales


def _check(qkv, qb, cache, scales, steps, mask=None, time_step=None, ind=None, beam=1):
    """run the kernel pair, compare with float64 and compare the cache and scales bitwise"""
    B, _, _, D = qkv.shape
    c0, s0 = cache.clone(), scales.clone()
    x = qkv.double() + (qb.double() if qb is not None else 0.0)                        # [B, 3, H, D]
    new = (qkv.float() + (qb.float() if qb is not None else 0.0))[:, 1:].to(qkv.dtype)  # rounded as the kernel does
    nq, ns = hip.kv_cache_quantize(new.transpose(0, 1))                                 # [2, B, H, D], [2, B, H]
    want_c, want_s, ref = c0.clone(), s0.clone(), []
    for b, ts in enumerate(steps):
        want_c[:, b, :, ts], want_s[:, b, :, ts] = nq[:, b], ns[:, b]
        t = torch.arange(ts, device="cuda")
        src = torch.full((ts,), b, device="cuda") if ind is None else b // beam * beam + ind[b, :ts].long()
        live = torch.ones(ts, dtype=torch.bool, device="cuda") if ind is None else (ind[b, :ts] >= 0) & (ind[b, :ts] < beam)
        src = torch.where(live, src, b)
        kv = c0[:, src, :, t].double() * s0[:, src, :, t].double()[..., None]           # [ts, 2, H, D]
        kv = torch.cat([kv.permute(1, 2, 0, 3), (nq[:, b].double() * ns[:, b].double()[..., None]).unsqueeze(2)], 2)
        s = (x[b, 0].unsqueeze(1) @ kv[0].transpose(-1, -2)) / math.sqrt(D)             # [H, 1, ts + 1]
        s[..., :ts].masked_fill_(~live, float("-inf"))
        if mask is not None:
            s = s + mask.double().expand(B, H, 1, mask.shape[-1])[b, :, :, :ts + 1]
        ref.append(torch.softmax(s, -1) @ kv[1])                                        # [H, 1, D]
    ref = torch.stack(ref).transpose(1, 2).reshape(B, 1, H * D)
    out = hip.decode_attention(qkv, qb, cache, steps[0] if time_step is None else time_step, mask=mask,
                               cache_indirection=ind, beam_size=beam, cache_scales=scales)
    torch.cuda.synchronize()
    assert out.shape == (B, 1, H * D) and out.dtype == qkv.dtype
    err = ((out.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"D={D} {qkv.dtype} steps={steps}: rel err {err:.3e} (bound {BOUND[qkv.dtype]:.3e})")
    assert err <= BOUND[qkv.dtype]
    assert torch.equal(cache, want_c) and torch.equal(scales.view(torch.int32), want_s.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("ti", range(8))
def test_sweep_matches_float64_and_appends_the_quantised_row(ti, D, dtype):
    """a single key, both sides of every split seam, the last slot"""
    ts = [0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, max_seq - 1][ti]
    _check(*_inputs(D, dtype, [ts, ts]), [ts, ts])


@pytest.mark.parametrize("D", [32, 64, 128])
def test_null_bias_device_step_and_an_all_zero_new_key(D):
    qkv, _, cache, scales = _inputs(D, torch.bfloat16, [C + 5] * 2, bias=False)
    qkv[:, 1] = 0
    _check(qkv, None, cache, scales, [C + 5] * 2, time_step=torch.tensor([C + 5], dtype=torch.int32, device="cuda"))
    assert torch.all(scales[0, :, :, C + 5] == 1.0) and torch.all(cache[0, :, :, C + 5] == 0)


@pytest.mark.parametrize("D", [32, 128])
def test_mask_whole_split_minus_inf(D):
    """split 0 hands (m = -inf, l = 0) to the combine kernel"""
    ts = C + 50
    mask = torch.zeros(2, H, 1, max_seq, device="cuda")
    mask[..., :C] = float("-inf")
    mask[..., C + 3:C + 20:2] = float("-inf")
    _check(*_inputs(D, torch.bfloat16, [ts, ts]), [ts, ts], mask=mask)


@pytest.mark.parametrize("D", [32, 64, 128])
def test_per_row_steps_straddle_a_seam(D):
    steps = [C - 1, C, 2 * C + 7]
    _check(*_inputs(D, torch.float16, steps), steps, time_step=torch.tensor(steps, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("D", [32, 64, 128])
def test_beam_table_reads_sibling_rows_and_skips_a_bad_entry(D):
    steps, beam = [C + 9] * 2 + [C - 4] * 2, 2
    qkv, qb, cache, scales = _inputs(D, torch.bfloat16, steps)
    g = torch.Generator(device="cuda").manual_seed(3)
    ind = torch.randint(0, beam, (4, max_seq), device="cuda", generator=g).to(torch.int32)
    ind[1, 5], ind[2, C - 10] = beam, -1                  # out of range: left out as if masked
    ind[:, C + 9:] = 7                                     # at or above the step: never read
    _check(qkv, qb, cache, scales, steps, time_step=torch.tensor(steps, dtype=torch.int32, device="cuda"),
           ind=ind, beam=beam)


def test_rejections_do_not_launch():
    qkv, qb, cache, scales = _inputs(64, torch.bfloat16, [5, 5])
    c0, s0 = cache.clone(), scales.clone()
    for kw in (dict(cache_scales=None), dict(cache_scales=scales.double()), dict(cache_scales=scales[..., :-1]),
               dict(cache_scales=scales.cpu()), dict(cache_scales=scales, time_step=max_seq)):
        with pytest.raises(ValueError):
            hip.decode_attention(qkv, qb, cache, kw.pop("time_step", 5), **kw)
    with pytest.raises(ValueError):
        hip.decode_attention(qkv, qb, cache.to(torch.bfloat16), 5, cache_scales=scales)
    assert not hip.decode_attn_supported(qkv, cache) and hip.decode_attn_supported(qkv, cache, cache_scales=scales)
    assert torch.equal(cache, c0) and torch.equal(scales.view(torch.int32), s0.view(torch.int32))
