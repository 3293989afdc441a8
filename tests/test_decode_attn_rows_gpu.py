"""Per-row time steps of the split-KV decode attention (pha_decode_attn_rows through
ops/hip.decode_attention): ``time_step`` an int32 device tensor [B], batch row b appending at and
attending up to its own step.

Each row is compared with the fp32 reference of tests/test_decode_attn_gpu.py built for that row's
step, within the bounds derived there (one ulp of the largest output element: 2^-8 in bf16, 2^-10 in
fp16). Cache rows above ts_b are NaN beforehand, so a key read above a row's step poisons that row;
afterwards the cache is compared bitwise. A workgroup of (split, head, b) depends on no other batch
row, so row b of the per-row call also equals, bitwise, row b of a scalar call at ts_b.

The per-row range guard is checked by reading the kernels; no test feeds a bad step."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H = 4, 3
BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
DS = pytest.mark.parametrize("D", [32, 64, 128])


def _hip():
    from paddle_hackathon_amd.ops import hip
    return hip


def _shape():
    C = _hip().DECODE_ATTN_CHUNK
    return C, 2 * C + 40


def _steps(vi):
    """a single key, both sides of each seam and the last slot, spread over two launches"""
    C, max_seq = _shape()
    return ([0, C - 1, C, max_seq - 1], [1, C + 1, 2 * C - 1, 2 * C])[vi]


def _inputs(D, dtype, steps, seed=0):
    """qkv, bias, cache with NaN in row b from position steps[b] on"""
    _, max_seq = _shape()
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 7 * sum(steps) + seed)
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).to(dtype)
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.5).to(dtype)
    cache = torch.randn(2, B, H, max_seq, D, device="cuda", generator=g).to(dtype)
    for b, t in enumerate(steps):
        cache[:, b, :, t:] = float("nan")
    return qkv, qb, cache


def _ref_row(qkv, qb, cache, b, ts, mask=None):
    """fp32 output [H * D] of batch row b at step ts and its new key / value [2, H, D] in the storage dtype"""
    D = qkv.shape[-1]
    x = qkv[b].float() + qb.float()                                           # [3, H, D]
    new = x[1:].to(qkv.dtype)                                                 # [2, H, D]
    k = torch.cat([cache[0, b, :, :ts].float(), new[0].float().unsqueeze(1)], 1)   # [H, ts + 1, D]
    v = torch.cat([cache[1, b, :, :ts].float(), new[1].float().unsqueeze(1)], 1)
    s = (x[0].unsqueeze(1) @ k.transpose(-1, -2)) / math.sqrt(D)              # [H, 1, ts + 1]
    if mask is not None:
        s = s + mask.float().expand(B, H, 1, mask.shape[-1])[b][..., :ts + 1]
    return (torch.softmax(s, -1) @ v).reshape(H * D), new


def _tensor(steps):
    return torch.tensor(steps, dtype=torch.int32, device="cuda")


def _check(qkv, qb, cache, steps, mask=None):
    before = cache.clone()
    out = _hip().decode_attention(qkv, qb, cache, _tensor(steps), mask=mask)
    torch.cuda.synchronize()
    assert out.shape == (B, 1, H * qkv.shape[-1]) and out.dtype == qkv.dtype
    want = before.clone()
    for b, t in enumerate(steps):
        ref, new = _ref_row(qkv, qb, before, b, t, mask)
        err = ((out[b, 0].float() - ref).abs().max() / ref.abs().max()).item()
        print(f"D={qkv.shape[-1]} {qkv.dtype} row {b} ts={t}: rel err {err:.3e} (bound {BOUND[qkv.dtype]:.3e})")
        assert err <= BOUND[qkv.dtype]
        want[:, b, :, t] = new
    # row ts_b of batch b is the biased key / value rounded to the dtype; nothing else moved (NaNs included)
    assert torch.equal(cache.view(torch.int16), want.view(torch.int16))
    return out


@DTYPES
@DS
@pytest.mark.parametrize("vi", [0, 1])
def test_rows_match_fp32_reference_and_update_cache(vi, D, dtype):
    steps = _steps(vi)
    _check(*_inputs(D, dtype, steps), steps)


@DTYPES
@DS
@pytest.mark.parametrize("vi", [0, 1])
def test_each_row_is_bitwise_the_scalar_call_at_its_step(vi, D, dtype):
    hip = _hip()
    steps = _steps(vi)
    qkv, qb, cache = _inputs(D, dtype, steps)
    before = cache.clone()
    out = hip.decode_attention(qkv, qb, cache, _tensor(steps))
    for b, t in enumerate(steps):
        c1 = before.clone()
        o1 = hip.decode_attention(qkv, qb, c1, t)
        assert torch.equal(out[b].view(torch.int16), o1[b].view(torch.int16))
        assert torch.equal(cache[:, b].view(torch.int16), c1[:, b].view(torch.int16))


@DS
def test_equal_steps_are_bitwise_the_scalar_device_step(D):
    hip = _hip()
    C, _ = _shape()
    steps = [C + 1] * B
    qkv, qb, cache = _inputs(D, torch.bfloat16, steps)
    c1 = cache.clone()
    out = hip.decode_attention(qkv, qb, cache, _tensor(steps))
    o1 = hip.decode_attention(qkv, qb, c1, _tensor(steps[:1]))
    assert torch.equal(out.view(torch.int16), o1.view(torch.int16))
    assert torch.equal(cache.view(torch.int16), c1.view(torch.int16))


@DTYPES
def test_mask_batch_broadcast_additive(dtype):
    """[B, 1, 1, max_seq] with -1e4 on random keys; every row's new key stays unmasked"""
    _, max_seq = _shape()
    steps = _steps(1)
    g = torch.Generator(device="cuda").manual_seed(5)
    mask = torch.zeros(B, 1, 1, max_seq, device="cuda")
    mask.masked_fill_(torch.rand(B, 1, 1, max_seq, device="cuda", generator=g) < 0.4, -1e4)
    for b, t in enumerate(steps):
        mask[b, ..., t] = 0.0
    _check(*_inputs(128, dtype, steps), steps, mask=mask)


@DS
def test_mask_whole_split_minus_inf_in_one_row(D):
    """row 2 (ts in split 1) has -inf on all of split 0: that split hands (m = -inf, l = 0) to the
    combine kernel while the other rows' split 0 is live"""
    C, max_seq = _shape()
    steps = [C - 2, 5, C + 50, 2 * C + 7]
    mask = torch.zeros(B, H, 1, max_seq, device="cuda")
    mask[2, ..., :C] = float("-inf")
    _check(*_inputs(D, torch.bfloat16, steps), steps, mask=mask)


def test_sync_free_and_one_graph_serves_the_next_step():
    hip = _hip()
    C, _ = _shape()
    steps = [3, C - 1, C, 2 * C + 1]
    nxt = [t + 1 for t in steps]
    qkv, qb, cache = _inputs(64, torch.bfloat16, nxt)   # finite up to each row's second step
    ts = _tensor(steps)
    eager = cache.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        e0 = hip.decode_attention(qkv, qb, eager, ts)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    e1 = hip.decode_attention(qkv, qb, eager, _tensor(nxt))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip.decode_attention(qkv, qb, cache.clone(), ts)   # warm-up off the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.decode_attention(qkv, qb, cache, ts)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), e0.view(torch.int16))
    ts.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), e1.view(torch.int16))
    assert torch.equal(cache.view(torch.int16), eager.view(torch.int16))


def test_rejections_need_no_launch():
    hip = _hip()
    _, max_seq = _shape()
    steps = [4, 5, 6, 7]
    qkv, qb, cache = _inputs(64, torch.bfloat16, steps)
    before = cache.clone()
    with pytest.raises(ValueError):   # B + 1 elements
        hip.decode_attention(qkv, qb, cache, _tensor(steps + [8]))
    with pytest.raises(ValueError):   # int64
        hip.decode_attention(qkv, qb, cache, torch.tensor(steps, device="cuda"))
    with pytest.raises(ValueError):   # a CPU tensor
        hip.decode_attention(qkv, qb, cache, torch.tensor(steps, dtype=torch.int32))
    with pytest.raises(ValueError):   # a mask shorter than the cache
        hip.decode_attention(qkv, qb, cache, _tensor(steps), mask=torch.zeros(B, 1, 1, max_seq - 1, device="cuda"))
    assert hip.decode_attn_supported(qkv, cache, None, _tensor(steps))
    assert not hip.decode_attn_supported(qkv, cache, None, _tensor(steps + [8]))
    assert not hip.decode_attn_supported(qkv, cache, None, torch.tensor(steps, device="cuda"))
    assert not hip.decode_attn_supported(qkv, cache, None, torch.tensor(steps, dtype=torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(cache.view(torch.int16), before.view(torch.int16))
