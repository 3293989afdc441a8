"""The beam-indirect form of the split-KV decode attention (pha_decode_attn_beam through
ops/hip.decode_attention with ``cache_indirection`` and ``beam_size``): row b reads key position
t < ts from cache row (b // K) * K + table[b, t] and appends position ts to its own cache row.

With the identity table the call must equal the per-row form bitwise. With random tables it is
compared with an fp32 reference that gathers each row's keys through the table, within the bounds of
tests/test_decode_attn_rows_gpu.py (one ulp of the largest output element: 2^-8 in bf16, 2^-10 in
fp16). Every cache position at or above a row's step is NaN beforehand, so a key read above the step,
or the table entry at the step being followed, poisons the row; afterwards the cache is compared
bitwise: the append lands in the row's own cache row and nothing else moves. The rows of a group
share one step (the contract); the per-row mix gives each group its own.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 2
BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
DS = pytest.mark.parametrize("D", [32, 64, 128])
GROUPS = pytest.mark.parametrize("B,K", [(4, 2), (8, 4)], ids=["B4K2", "B8K4"])


def _hip():
    from paddle_hackathon_amd.ops import hip
    return hip


def _shape():
    C = _hip().DECODE_ATTN_CHUNK
    return C, 2 * C + 5


def _step_sets(B, K):
    """uniform steps at a single key, both sides of a seam and the last slot, and a mix between groups"""
    C, max_seq = _shape()
    mix = [s for g in range(B // K) for s in [(C - 1, C, 3, max_seq - 1)[g % 4]] * K]
    return [[0] * B, [C - 1] * B, [C] * B, [max_seq - 1] * B, mix]


def _inputs(B, K, D, dtype, steps, seed=0):
    """qkv, bias, cache with NaN in row b from position steps[b] on, and a random table within each group
    (entries at and above the step hold K + 3: followed, they would leave the group)"""
    _, max_seq = _shape()
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 7 * sum(steps) + 31 * K + seed)
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).to(dtype)
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.5).to(dtype)
    cache = torch.randn(2, B, H, max_seq, D, device="cuda", generator=g).to(dtype)
    ind = torch.randint(0, K, (B, max_seq), device="cuda", generator=g, dtype=torch.int32)
    for b, t in enumerate(steps):
        cache[:, b, :, t:] = float("nan")
        ind[b, t:] = K + 3
    return qkv, qb, cache, ind


def _ref_row(qkv, qb, cache, ind, K, b, ts, mask=None, skip=()):
    """fp32 output [H * D] of row b at step ts, its keys gathered through the table (positions in
    ``skip`` left out), and its new key / value [2, H, D] in the storage dtype"""
    B, D = qkv.shape[0], qkv.shape[-1]
    x = qkv[b].float() + qb.float()
    new = x[1:].to(qkv.dtype)
    src = (b // K) * K + ind[b, :ts].long()
    t = torch.arange(ts, device=cache.device)
    k = torch.cat([cache[0, src, :, t].float().transpose(0, 1), new[0].float().unsqueeze(1)], 1)   # [H, ts + 1, D]
    v = torch.cat([cache[1, src, :, t].float().transpose(0, 1), new[1].float().unsqueeze(1)], 1)
    s = (x[0].unsqueeze(1) @ k.transpose(-1, -2)) / math.sqrt(D)
    if mask is not None:
        s = s + mask.float().expand(B, H, 1, mask.shape[-1])[b][..., :ts + 1]
    for p in skip:
        s[..., p] = float("-inf")
    return (torch.softmax(s, -1) @ v).reshape(H * D), new


def _tensor(steps):
    return torch.tensor(steps, dtype=torch.int32, device="cuda")


def _check(qkv, qb, cache, ind, K, steps, mask=None, skip=None):
    B = qkv.shape[0]
    before, ind_before = cache.clone(), ind.clone()
    out = _hip().decode_attention(qkv, qb, cache, _tensor(steps), mask=mask, cache_indirection=ind, beam_size=K)
    torch.cuda.synchronize()
    assert out.shape == (B, 1, H * qkv.shape[-1]) and out.dtype == qkv.dtype
    want = before.clone()
    worst = 0.0
    for b, t in enumerate(steps):
        # the siblings of row b append at the same step in the same launch; row b reads only below it
        ref, new = _ref_row(qkv, qb, before, ind_before, K, b, t, mask, (skip or {}).get(b, ()))
        err = ((out[b, 0].float() - ref).abs().max() / ref.abs().max()).item()
        worst = max(worst, err)
        assert err <= BOUND[qkv.dtype], f"row {b} ts={t}: rel err {err:.3e} above {BOUND[qkv.dtype]:.3e}"
        want[:, b, :, t] = new
    print(f"D={qkv.shape[-1]} {qkv.dtype} B={B} K={K} steps={steps}: worst rel err {worst:.3e}")
    assert torch.equal(cache.view(torch.int16), want.view(torch.int16))
    assert torch.equal(ind, ind_before)
    return out


@DTYPES
@DS
@GROUPS
def test_identity_table_is_bitwise_the_per_row_form(B, K, D, dtype):
    hip = _hip()
    C, max_seq = _shape()
    for steps in ([C + 1] * B, _step_sets(B, K)[-1]):
        qkv, qb, cache, _ = _inputs(B, K, D, dtype, steps)
        ind = (torch.arange(B, device="cuda", dtype=torch.int32) % K)[:, None].expand(B, max_seq).contiguous()
        c1 = cache.clone()
        out = hip.decode_attention(qkv, qb, cache, _tensor(steps), cache_indirection=ind, beam_size=K)
        o1 = hip.decode_attention(qkv, qb, c1, _tensor(steps))
        assert torch.equal(out.view(torch.int16), o1.view(torch.int16))
        assert torch.equal(cache.view(torch.int16), c1.view(torch.int16))


@DTYPES
@DS
@GROUPS
@pytest.mark.parametrize("si", range(5), ids=["ts0", "tsC-1", "tsC", "last", "mix"])
def test_random_tables_match_the_gathering_reference(si, B, K, D, dtype):
    steps = _step_sets(B, K)[si]
    _check(*_inputs(B, K, D, dtype, steps), K, steps)


@DS
def test_scalar_time_steps_are_broadcast(D):
    hip = _hip()
    C, _ = _shape()
    B, K = 4, 2
    steps = [C + 2] * B
    qkv, qb, cache, ind = _inputs(B, K, D, torch.bfloat16, steps)
    c1, c2 = cache.clone(), cache.clone()
    out = hip.decode_attention(qkv, qb, cache, _tensor(steps), cache_indirection=ind, beam_size=K)
    o1 = hip.decode_attention(qkv, qb, c1, C + 2, cache_indirection=ind, beam_size=K)
    o2 = hip.decode_attention(qkv, qb, c2, _tensor(steps[:1]), cache_indirection=ind, beam_size=K)
    for o, c in ((o1, c1), (o2, c2)):
        assert torch.equal(out.view(torch.int16), o.view(torch.int16))
        assert torch.equal(cache.view(torch.int16), c.view(torch.int16))


@DTYPES
@DS
def test_cache_rows_the_table_does_not_name_are_never_read(D, dtype):
    """the table names only even beams; the odd beams' cache rows hold NaN below the step too"""
    C, _ = _shape()
    B, K = 8, 4
    steps = [C + 7] * B
    qkv, qb, cache, ind = _inputs(B, K, D, dtype, steps)
    for b, t in enumerate(steps):
        ind[b, :t] = ind[b, :t] // 2 * 2
    cache[:, 1::2] = float("nan")
    out = _check(qkv, qb, cache, ind, K, steps)
    assert bool(torch.isfinite(out.float()).all())


@DTYPES
@DS
def test_an_out_of_range_entry_leaves_its_key_out(D, dtype):
    C, _ = _shape()
    B, K = 4, 2
    steps = [C + 7] * B
    for pos, bad in ((5, K), (C + 1, -1), (C - 1, 1 << 30)):
        qkv, qb, cache, ind = _inputs(B, K, D, dtype, steps)
        ind[1, pos] = bad                     # row 1 is in group 0 of the two groups
        good = ind.clone()
        good[1, pos] = 0                      # the reference gathers a valid row there and masks the position
        before, ind_before = cache.clone(), ind.clone()
        out = _hip().decode_attention(qkv, qb, cache, _tensor(steps), cache_indirection=ind, beam_size=K)
        for b, t in enumerate(steps):
            ref, _ = _ref_row(qkv, qb, before, good, K, b, t, None, (pos,) if b == 1 else ())
            err = ((out[b, 0].float() - ref).abs().max() / ref.abs().max()).item()
            assert err <= BOUND[dtype], f"entry {bad} at {pos}, row {b}: rel err {err:.3e}"
        assert torch.equal(ind, ind_before)


@DS
@pytest.mark.parametrize("kind", ["additive", "bool"])
def test_with_a_mask(kind, D):
    C, max_seq = _shape()
    B, K = 4, 2
    steps = _step_sets(B, K)[-1]
    qkv, qb, cache, ind = _inputs(B, K, D, torch.bfloat16, steps)
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "additive":
        mask = torch.randn(B, 1, 1, max_seq, device="cuda", generator=g)
        _check(qkv, qb, cache, ind, K, steps, mask=mask)
    else:
        keep = torch.rand(B, 1, 1, max_seq, device="cuda", generator=g) > 0.3
        for b, t in enumerate(steps):
            keep[b, ..., t] = True            # every row keeps its own new key
        add = torch.zeros(keep.shape, device="cuda").masked_fill_(~keep, float("-inf"))
        before, ind_before = cache.clone(), ind.clone()
        out = _hip().decode_attention(qkv, qb, cache, _tensor(steps), mask=keep, cache_indirection=ind, beam_size=K)
        for b, t in enumerate(steps):
            ref, _ = _ref_row(qkv, qb, before, ind_before, K, b, t, add)
            assert ((out[b, 0].float() - ref).abs().max() / ref.abs().max()).item() <= BOUND[torch.bfloat16]


def test_rejections():
    hip = _hip()
    C, max_seq = _shape()
    B, K = 4, 2
    steps = [C] * B
    qkv, qb, cache, ind = _inputs(B, K, 64, torch.bfloat16, steps)
    ts = _tensor(steps)
    bad = [dict(cache_indirection=ind.long(), beam_size=K), dict(cache_indirection=ind[:, :-1], beam_size=K),
           dict(cache_indirection=ind[:2], beam_size=K), dict(cache_indirection=ind.cpu(), beam_size=K),
           dict(cache_indirection=ind.t().contiguous().t(), beam_size=K), dict(cache_indirection=ind, beam_size=3),
           dict(cache_indirection=ind, beam_size=0), dict(cache_indirection=None, beam_size=2)]
    for kw in bad:
        assert not hip.decode_attn_supported(qkv, cache, None, ts, **kw)
        with pytest.raises(ValueError):
            hip.decode_attention(qkv, qb, cache, ts, **kw)
    assert hip.decode_attn_supported(qkv, cache, None, ts, cache_indirection=ind, beam_size=K)
    assert hip.decode_attn_supported(qkv, cache, None, ts, cache_indirection=ind, beam_size=4)
