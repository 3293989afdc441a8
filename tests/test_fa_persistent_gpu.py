"""Persistent launch form of the default D = 128 attention kernels (PHA_FA_PERSIST: forward, dQ,
dK/dV) against the one-workgroup-per-block grid of the same build and against fp32.

The persistent form only reschedules: a workgroup walks several items, the next item's operands
are requested under the current item's last tile, and the outputs leave through 16-byte stores.
The arithmetic and its order are those of the plain form, so every output must be bitwise equal to
it; the fp32 bounds are the ones of test_kernels_gpu.py (2e-2 on O, 3e-2 * max(1, scale) on the
gradients). PHA_FA_PERSIST_WGS sets the workgroup count, so these small shapes give several items
per workgroup, item counts that do not divide, and workgroups with no item at all."""
import functools

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

D = 128


def _ref_attn(q, k, v, causal):
    H, Hk = q.shape[2], k.shape[2]
    if Hk != H:
        k = k.repeat_interleave(H // Hk, dim=2)
        v = v.repeat_interleave(H // Hk, dim=2)
    qt, kt, vt = (t.float().transpose(1, 2) for t in (q, k, v))
    return TF.scaled_dot_product_attention(qt, kt, vt, is_causal=causal).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _case(dt, causal, B, H, Hk, S, Sk):
    """inputs, upstream gradient and the fp32 reference (o, dq, dk, dv) of one shape, made once"""
    gen = torch.Generator(device="cuda").manual_seed(1000 * S + Sk + H)
    q = torch.randn(B, S, H, D, device="cuda", generator=gen).to(dt)
    k = torch.randn(B, Sk, Hk, D, device="cuda", generator=gen).to(dt)
    v = torch.randn(B, Sk, Hk, D, device="cuda", generator=gen).to(dt)
    g = torch.randn(B, S, H, D, device="cuda", generator=gen)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_attn(qr, kr, vr, causal)
    ref.backward(g)
    return q, k, v, g.to(dt), (ref.detach(), qr.grad, kr.grad, vr.grad)


def _run(q, k, v, g, causal):
    from paddle_hackathon_amd.ops import hip
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = hip.FlashAttention.apply(q, k, v, causal, None)
    o.backward(g)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


def _check(monkeypatch, dt, causal, B, H, Hk, S, Sk, wgs):
    q, k, v, g, ref = _case(dt, causal, B, H, Hk, S, Sk)
    monkeypatch.setenv("PHA_FA_PERSIST", "0")
    plain = _run(q, k, v, g, causal)
    monkeypatch.setenv("PHA_FA_PERSIST", "7")
    if wgs is None:
        monkeypatch.delenv("PHA_FA_PERSIST_WGS", raising=False)
    else:
        monkeypatch.setenv("PHA_FA_PERSIST_WGS", str(wgs))
    pers = _run(q, k, v, g, causal)
    for name, a, b in zip(("o", "dq", "dk", "dv"), pers, plain):
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
    err = (pers[0].float() - ref[0]).abs().max().item()
    assert err < 2e-2, ("o", err)
    for name, got, want in zip(("dq", "dk", "dv"), pers[1:], ref[1:]):
        err = (got.float() - want).abs().max().item()
        scale = want.abs().max().item()
        assert err < 3e-2 * max(1.0, scale), (name, err, scale)


# S = 600: ragged last block and ragged last tile; 256: one query block per pair; 100: one tile, so
# the seam requests run inside an item's only tile. 2 workgroups: 3+ items each; 5: the item counts
# (6 / 18 query blocks, 6 / 12 / 30 key blocks) do not divide.
@pytest.mark.parametrize("wgs", [2, 5])
@pytest.mark.parametrize("S", [600, 256, 100])
def test_persistent_causal(S, wgs, monkeypatch):
    _check(monkeypatch, torch.bfloat16, True, 2, 3, 3, S, S, wgs)


@pytest.mark.parametrize("S", [256, 100])
def test_persistent_idle_workgroups(S, monkeypatch):
    """more workgroups than items: the spare ones must leave without touching memory"""
    _check(monkeypatch, torch.bfloat16, True, 2, 3, 3, S, S, 64)


# cross attention, causal with S != Sk (key blocks past the last query have no tile at all), GQA
@pytest.mark.parametrize("causal,S,Sk", [(False, 200, 520), (False, 64, 1000), (True, 520, 200)])
def test_persistent_cross_gqa(causal, S, Sk, monkeypatch):
    _check(monkeypatch, torch.bfloat16, causal, 2, 8, 2, S, Sk, 3)


@pytest.mark.parametrize("causal,S,Sk", [(True, 600, 600), (False, 200, 520)])
def test_persistent_fp16(causal, S, Sk, monkeypatch):
    _check(monkeypatch, torch.float16, causal, 2, 3, 3, S, Sk, 4)


def test_persistent_real_cu_count(monkeypatch):
    """no override: min(items, CUs) workgroups"""
    _check(monkeypatch, torch.bfloat16, True, 4, 16, 16, 512, 512, None)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal,S,wgs", [(True, 600, 2), (True, 100, 5), (False, 300, 3)])
def test_persistent_packed_qkv(causal, S, wgs, dt, monkeypatch):
    """packed [B, S, H, 3D] projections read and their gradient written in place (token stride
    3 H D), delta formed inside the dQ kernel"""
    from paddle_hackathon_amd.ops import hip
    monkeypatch.delenv("PHA_FA_DELTA_PASS", raising=False)
    B, H = 2, 3
    gen = torch.Generator(device="cuda").manual_seed(7 + S)
    qkv = torch.randn(B, S, H, 3 * D, device="cuda", generator=gen).to(dt)
    do = torch.randn(B, S, H, D, device="cuda", generator=gen).to(dt)
    res = {}
    for mode in ("0", "7"):
        monkeypatch.setenv("PHA_FA_PERSIST", mode)
        monkeypatch.setenv("PHA_FA_PERSIST_WGS", str(wgs))
        a = qkv.clone().requires_grad_()
        o = hip.FlashAttentionPacked.apply(a, causal, None)
        (da,) = torch.autograd.grad(o, a, do)
        torch.cuda.synchronize()
        res[mode] = (o.detach(), da)
    assert torch.equal(res["7"][0], res["0"][0])
    assert torch.equal(res["7"][1], res["0"][1])
    qf = qkv.float().requires_grad_()
    q, k, v = qf.split(D, dim=-1)
    ref = _ref_attn(q, k, v, causal)
    (dref,) = torch.autograd.grad(ref, qf, do.float())
    err = (res["7"][0].float() - ref).abs().max().item()
    assert err < 2e-2, err
    err = (res["7"][1].float() - dref).abs().max().item()
    assert err < 3e-2 * max(1.0, dref.abs().max().item()), err
