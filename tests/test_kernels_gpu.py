"""Numerics of the gfx950 HIP kernels vs plain PyTorch fp32 references (GPU only).

Each test asserts the native library is the code path that ran (no silent fallback).
"""
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _native():
    from paddle_hackathon_amd.ops import _lib
    assert _lib.native_available(), "libpha_kernels.so must be loaded on a GPU run"
    yield


def _tol(dt):
    return {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-3}[dt]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H", [64, 768, 1000 * 0 + 1024, 2048, 2056, 4096])
def test_layer_norm_fwd_bwd(dt, H):
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(0)
    rows = 37
    x = torch.randn(rows, H, device="cuda").to(dt)
    w = (torch.rand(H, device="cuda") + 0.5).to(dt)
    b = torch.randn(H, device="cuda").to(dt)
    y, mean, rstd = hip.layer_norm_fwd(x, w, b, 1e-5)
    ref = TF.layer_norm(x.float(), [H], w.float(), b.float(), 1e-5)
    assert torch.allclose(y.float(), ref, atol=_tol(dt) * 4, rtol=_tol(dt))
    dy = torch.randn_like(x)
    dx, dw, db = hip.layer_norm_bwd(dy, x, w, mean, rstd, True)
    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    br = b.float().requires_grad_(True)
    TF.layer_norm(xr, [H], wr, br, 1e-5).backward(dy.float())
    assert torch.allclose(dx.float(), xr.grad, atol=_tol(dt) * 8, rtol=_tol(dt) * 2)
    assert torch.allclose(dw.float(), wr.grad, atol=_tol(dt) * 40, rtol=_tol(dt) * 2)
    assert torch.allclose(db.float(), br.grad, atol=_tol(dt) * 40, rtol=_tol(dt) * 2)


def test_layer_norm_fp32_weight_bf16_input():
    from paddle_hackathon_amd.ops import hip
    x = torch.randn(64, 2048, device="cuda").bfloat16()
    w = torch.rand(2048, device="cuda") + 0.5
    b = torch.randn(2048, device="cuda")
    y, _, _ = hip.layer_norm_fwd(x, w, b, 1e-5)
    ref = TF.layer_norm(x.float(), [2048], w, b, 1e-5)
    assert torch.allclose(y.float(), ref, atol=5e-2, rtol=2e-2)


@pytest.mark.parametrize("H", [768, 2048, 4096])
@pytest.mark.parametrize("rows", [5, 3000])
def test_add_layer_norm_fused(H, rows):
    """(x, r) -> (x + r, LN(x + r)) and its backward (dx = dr = LN'(dy) + dh) vs fp32 autograd,
    bf16 activations with fp32 LN parameters (the AMP-O2 layout)."""
    from paddle_hackathon_amd.ops import fused
    torch.manual_seed(0)
    x = torch.randn(rows, H, device="cuda").bfloat16().requires_grad_(True)
    r = torch.randn(rows, H, device="cuda").bfloat16().requires_grad_(True)
    w = (torch.rand(H, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(H, device="cuda").requires_grad_(True)
    h, y = fused.add_layer_norm(x, r, w, b, 1e-5)
    hr = (x.detach() + r.detach()).float().requires_grad_(True)  # the bf16-rounded sum, as unfused
    xr, wr, br = hr, w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = TF.layer_norm(xr, [H], wr, br, 1e-5)
    assert torch.equal(h, (x + r).detach())
    assert (y.float() - yr).abs().max().item() < 5e-2
    dy, dh = torch.randn_like(yr), torch.randn_like(yr)
    torch.autograd.backward([h, y], [dh.bfloat16(), dy.bfloat16()])
    torch.autograd.backward([yr], [dy.bfloat16().float()])
    want = xr.grad + dh.bfloat16().float()
    assert (x.grad.float() - want).abs().max().item() < 6e-2 * max(1.0, want.abs().max().item() / 8)
    assert torch.equal(x.grad, r.grad)
    assert torch.allclose(w.grad, wr.grad, atol=0.5, rtol=2e-2)
    assert torch.allclose(b.grad, br.grad, atol=0.5, rtol=2e-2)


@pytest.mark.parametrize("H", [768, 2048, 4096])
@pytest.mark.parametrize("xb_dtype", [torch.float32, torch.bfloat16])
def test_add_layer_norm_folded_bias(H, xb_dtype):
    """h = x + (r + xb), y = LN(h): the branch bias xb is added in the LN kernel and its gradient is
    the column sum of the stored dx, produced by the LN backward kernel (dx_colsum)"""
    from paddle_hackathon_amd.ops import fused
    torch.manual_seed(3)
    rows = 3000
    x = torch.randn(rows, H, device="cuda").bfloat16().requires_grad_(True)
    r = torch.randn(rows, H, device="cuda").bfloat16().requires_grad_(True)
    xb = torch.randn(H, device="cuda").to(xb_dtype).requires_grad_(True)
    w = (torch.rand(H, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(H, device="cuda").requires_grad_(True)
    h, y = fused.add_layer_norm(x, r, w, b, 1e-5, xb=xb)
    hs = (x.detach() + (r.detach() + xb.detach().to(w.dtype)).bfloat16())   # the rounding the kernel does
    assert torch.equal(h, hs.detach())
    dy, dh = torch.randn(rows, H, device="cuda").bfloat16(), torch.randn(rows, H, device="cuda").bfloat16()
    torch.autograd.backward([h, y], [dh, dy])
    assert torch.equal(x.grad, r.grad)
    ref = x.grad.float().sum(0)
    assert xb.grad.dtype == xb_dtype
    assert (xb.grad.float() - ref).abs().max().item() < 2e-2 * max(1.0, ref.abs().max().item())
    # the plain path (no xb) gives the same dx
    x2, r2 = x.detach().clone().requires_grad_(True), (r.detach() + xb.detach().to(torch.bfloat16)).requires_grad_(True)
    h2, y2 = fused.add_layer_norm(x2, r2, w.detach(), b.detach(), 1e-5)
    torch.autograd.backward([h2, y2], [dh, dy])
    if xb_dtype == torch.bfloat16:
        assert torch.equal(h2, h)
        assert torch.equal(x2.grad, x.grad)


def test_gpt_deferred_bias_matches_plain():
    """GPT layers with the output-projection biases folded into the add-LN kernels (the default)
    give the plain per-layer path's loss and bias gradients"""
    import os
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models.gpt import GPTForPretraining, gpt_config
    paddle.set_device("gpu")
    try:
        paddle.seed(7)
        cfg = gpt_config("gpt-tiny", hidden_size=256, num_heads=4, ffn_hidden_size=1024)
        m = GPTForPretraining(cfg)
        m.bfloat16()   # the bf16 fused-MLP / flash-attention / add-LN kernels
        ids = paddle.to_tensor(torch.randint(0, cfg.vocab_size, (2, 128)))
        lab = paddle.to_tensor(torch.randint(0, cfg.vocab_size, (2, 128)))
        out = {}
        for mode in ("1", "0"):
            os.environ["PHA_GPT_DEFER_BIAS"] = mode
            for p in m.parameters():
                p.clear_grad()
            loss = m(ids, labels=lab)
            loss.backward()
            out[mode] = (float(loss), {n: p.grad._t.float().clone() for n, p in m.named_parameters()
                                       if n.endswith("bias") and p.grad is not None})
        os.environ.pop("PHA_GPT_DEFER_BIAS", None)
        assert abs(out["1"][0] - out["0"][0]) < 2e-2 * max(1.0, abs(out["0"][0]))
        assert out["1"][1].keys() == out["0"][1].keys()
        for n, g in out["0"][1].items():
            d = (out["1"][1][n] - g).abs().max().item()
            assert d <= 3e-2 * max(1e-3, g.abs().max().item()) + 1e-3, (n, d)
    finally:
        os.environ.pop("PHA_GPT_DEFER_BIAS", None)
        paddle.set_device("cpu")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [128, 1024, 2048, 4096])
def test_softmax(dt, H):
    from paddle_hackathon_amd.ops import hip
    x = (torch.randn(50, H, device="cuda") * 3).to(dt)
    y = hip.softmax_fwd(x)
    ref = torch.softmax(x.float(), -1)
    assert torch.allclose(y.float(), ref, atol=_tol(dt), rtol=_tol(dt) * 2)
    dy = torch.randn_like(x)
    dx = hip.softmax_bwd(dy, y)
    xr = x.float().requires_grad_(True)
    torch.softmax(xr, -1).backward(dy.float())
    assert torch.allclose(dx.float(), xr.grad, atol=_tol(dt) * 2, rtol=_tol(dt) * 4)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [512, 50304, 32000, 30522, 7])   # 30522 / 7: the element-wise (V % 8 != 0) path
def test_softmax_cross_entropy(dt, V):
    from paddle_hackathon_amd import ops
    rows = 67
    logits = (torch.randn(rows, V, device="cuda") * 2).to(dt).requires_grad_(True)
    labels = torch.randint(0, V, (rows,), device="cuda")
    labels[3] = -100
    loss = ops.softmax_cross_entropy(logits, labels, -100)
    ref_l = logits.detach().float().requires_grad_(True)
    ref = TF.cross_entropy(ref_l, labels, reduction="none", ignore_index=-100)
    assert torch.allclose(loss, ref, atol=1e-3 if dt == torch.float32 else 2e-2, rtol=1e-3)
    g = torch.rand(rows, device="cuda")
    loss.backward(g)
    ref.backward(g)
    assert torch.allclose(logits.grad.float(), ref_l.grad, atol=1e-5 if dt == torch.float32 else 2e-3, rtol=2e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("rows", [33, 2500])
def test_bias_gelu(dt, approx, rows):
    """bf16 takes the fused gx + bias-grad-partials kernel (rows split over block rows)."""
    from paddle_hackathon_amd import ops
    torch.manual_seed(0)
    x = torch.randn(rows, 4096, device="cuda").to(dt).requires_grad_(True)
    b = torch.randn(4096, device="cuda").to(dt).requires_grad_(True)
    y = ops.bias_gelu(x, b, approx)
    xr = x.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    ref = TF.gelu(xr + br, approximate="tanh" if approx else "none")
    assert torch.allclose(y.float(), ref, atol=_tol(dt) * 2, rtol=_tol(dt))
    g = torch.randn_like(ref)
    y.backward(g.to(dt))
    ref.backward(g)
    assert torch.allclose(x.grad.float(), xr.grad, atol=_tol(dt) * 4, rtol=_tol(dt) * 2)
    assert torch.allclose(b.grad.float(), br.grad, atol=_tol(dt) * 60 * max(1.0, rows / 300), rtol=_tol(dt) * 2)


def test_layer_norm_bwd_two_stage_column_sum():
    """8192 rows: dgamma/dbeta partials go through the chip-wide two-stage column sum."""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(0)
    x = torch.randn(8192, 2048, device="cuda").bfloat16()
    w = torch.rand(2048, device="cuda") + 0.5
    b = torch.randn(2048, device="cuda")
    y, mean, rstd = hip.layer_norm_fwd(x, w, b, 1e-5)
    dy = torch.randn_like(x)
    dx, dw, db = hip.layer_norm_bwd(dy, x, w, mean, rstd, True)
    xr, wr, br = x.float().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    TF.layer_norm(xr, [2048], wr, br, 1e-5).backward(dy.float())
    assert (dw - wr.grad).abs().max().item() < 1e-3 * max(1.0, wr.grad.abs().max().item())
    assert (db - br.grad).abs().max().item() < 1e-3 * max(1.0, br.grad.abs().max().item())


def test_embedding_fwd_bwd():
    from paddle_hackathon_amd import ops
    w = torch.randn(1000, 256, device="cuda").bfloat16().requires_grad_(True)
    ids = torch.randint(0, 1000, (4, 77), device="cuda")
    y = ops.embedding(ids, w)
    assert torch.equal(y, w.detach()[ids])
    y.float().sum().backward()
    ref = torch.zeros(1000, 256, device="cuda").index_add_(0, ids.reshape(-1), torch.ones(ids.numel(), 256, device="cuda"))
    assert torch.allclose(w.grad.float(), ref, atol=1e-2)


@pytest.mark.parametrize("dt,V,D,n", [(torch.bfloat16, 50304, 2048, 8192), (torch.float32, 1000, 132, 5000),
                                      (torch.float16, 77, 2060, 3000), (torch.bfloat16, 2, 768, 16384),
                                      (torch.bfloat16, 512, 768, 16384), (torch.float32, 8, 132, 5000)])
def test_embedding_bwd_deterministic(dt, V, D, n):
    """HIP embedding backward (csrc ce_gelu_embed.hip) vs an fp64 index_add; a skewed id
    distribution (one id takes 30 % of the tokens: list batching), padding_idx rows zero, and two
    launches bitwise equal. Small vocabularies (token types, positions) take the token-chunked
    path (fp32 partials per chunk, summed in chunk order)"""
    from paddle_hackathon_amd.ops import hip
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(0, V, (n,), device="cuda", generator=g)
    ids[torch.rand(n, device="cuda", generator=g) < 0.3] = 5 % V
    gy = torch.randn(n, D, device="cuda", generator=g).to(dt)
    pad = 7 % V if V > 2 else None
    gw = hip.embedding_bwd(ids, gy, V, padding_idx=pad)
    ref = torch.zeros(V, D, dtype=torch.float64, device="cuda").index_add_(0, ids, gy.double())
    if pad is not None:
        ref[pad] = 0
    tol = 1e-2 if dt != torch.float32 else 1e-5
    assert ((gw.double() - ref).abs().max() / ref.abs().max()).item() < tol
    assert torch.equal(gw, hip.embedding_bwd(ids, gy, V, padding_idx=pad))


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16])
def test_multi_tensor_adamw(pdt):
    from paddle_hackathon_amd.ops import hip, fused
    torch.manual_seed(0)
    shapes = [(1000,), (37, 129), (2048, 64), (3,)]
    ps = [torch.randn(s, device="cuda").to(pdt) for s in shapes]
    gs = [torch.randn(s, device="cuda").to(pdt) for s in shapes]
    ms = [torch.zeros(s, device="cuda") for s in shapes]
    vs = [torch.zeros(s, device="cuda") for s in shapes]
    masters = [p.float().clone() if pdt != torch.float32 else None for p in ps]
    # reference: CPU path of the same op in fp32
    rp = [p.float().cpu().clone() for p in ps]
    rg = [g.float().cpu() for g in gs]
    rm = [torch.zeros(s) for s in shapes]
    rv = [torch.zeros(s) for s in shapes]
    for step in (1, 2, 3):
        hip.multi_tensor_adam(ps, gs, ms, vs, masters, 1e-2, 0.9, 0.95, 1e-8, step, 0.0, True, None, 1.0, [0.1] * 4)
        fused.fused_adam_(rp, rg, rm, rv, None, 1e-2, 0.9, 0.95, 1e-8, step, 0.1, True, None, 1.0)
    for i in range(len(shapes)):
        got = (masters[i] if masters[i] is not None else ps[i]).float().cpu()
        assert torch.allclose(got, rp[i], atol=1e-5, rtol=1e-5), i
        assert torch.allclose(ms[i].cpu(), rm[i], atol=1e-6)


def test_multi_tensor_l2norm():
    from paddle_hackathon_amd.ops import hip
    ts = [torch.randn(s, device="cuda").bfloat16() for s in [(5000,), (128, 300), (7,)]]
    got = hip.multi_tensor_l2norm_sq(ts)
    ref = sum(t.float().pow(2).sum() for t in ts)
    assert torch.allclose(got, ref, rtol=1e-4)


def test_gpt_tiny_train_step_gpu():
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import gpt_config, GPTForPretraining
    paddle.set_device("gpu:0")
    paddle.seed(0)
    cfg = gpt_config("gpt-tiny")
    m = paddle.amp.decorate(GPTForPretraining(cfg), level="O2", dtype="bfloat16")
    opt = paddle.optimizer.AdamW(1e-3, parameters=m.parameters())
    ids = paddle.randint(0, cfg.vocab_size, [4, 64])
    losses = []
    for _ in range(30):
        loss = m(ids, ids)
        loss.backward()
        opt.step()
        opt.clear_grad()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 1.0, losses


def _ref_attn(q, k, v, causal, scale=None):
    B, S, H, D = q.shape
    Hk = k.shape[2]
    if Hk != H:
        k = k.repeat_interleave(H // Hk, dim=2)
        v = v.repeat_interleave(H // Hk, dim=2)
    qt, kt, vt = (t.float().transpose(1, 2) for t in (q, k, v))
    o = TF.scaled_dot_product_attention(qt, kt, vt, is_causal=causal, scale=scale)
    return o.transpose(1, 2)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [128, 200, 512])
def test_flash_attention_fwd_bwd(dt, D, causal, S):
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(0)
    B, H = 2, 3
    q = torch.randn(B, S, H, D, device="cuda").to(dt).requires_grad_(True)
    k = torch.randn(B, S, H, D, device="cuda").to(dt).requires_grad_(True)
    v = torch.randn(B, S, H, D, device="cuda").to(dt).requires_grad_(True)
    assert hip.flash_attn_supported(q, k, v, 0.0)
    o = hip.FlashAttention.apply(q, k, v, causal, None)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_attn(qr, kr, vr, causal)
    assert (o.float() - ref).abs().max().item() < 2e-2, (o.float() - ref).abs().max().item()
    g = torch.randn_like(ref)
    o.backward(g.to(dt))
    ref.backward(g)
    for got, want, name in ((q.grad, qr.grad, "dq"), (k.grad, kr.grad, "dk"), (v.grad, vr.grad, "dv")):
        err = (got.float() - want).abs().max().item()
        scale = want.abs().max().item()
        assert err < 3e-2 * max(1.0, scale), (name, err, scale)


@pytest.mark.parametrize("mode", ["v2", "v2dkdv", "v2dq", "fused"])
@pytest.mark.parametrize("causal,S,Sk", [(True, 300, 300), (True, 1024, 1024), (False, 200, 520), (True, 520, 200),
                                         (False, 64, 1000)])
def test_flash_attention_bwd_paths_gqa(mode, causal, S, Sk, monkeypatch):
    """The D=128 backward paths (two-kernel with the pipelined v3 dK/dV kernel, the same with the
    v2 dK/dV kernel, single-kernel with atomic fp32 dQ) against fp32, with GQA (8 query heads on 2
    kv heads), ragged lengths and cross attention."""
    from paddle_hackathon_amd.ops import hip
    monkeypatch.setenv("PHA_FA_BWD", "v2" if mode in ("v2dkdv", "v2dq") else mode)
    monkeypatch.setenv("PHA_FA_DKDV", "v2" if mode == "v2dkdv" else "v3")
    monkeypatch.setenv("PHA_FA_DQ", "v2" if mode == "v2dq" else "v3")
    torch.manual_seed(1)
    B, H, Hk, D = 2, 8, 2, 128
    q = torch.randn(B, S, H, D, device="cuda").bfloat16().requires_grad_(True)
    k = torch.randn(B, Sk, Hk, D, device="cuda").bfloat16().requires_grad_(True)
    v = torch.randn(B, Sk, Hk, D, device="cuda").bfloat16().requires_grad_(True)
    o = hip.FlashAttention.apply(q, k, v, causal, None)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_attn(qr, kr, vr, causal)
    g = torch.randn_like(ref)
    o.backward(g.bfloat16())
    ref.backward(g)
    for got, want, name in ((q.grad, qr.grad, "dq"), (k.grad, kr.grad, "dk"), (v.grad, vr.grad, "dv")):
        err = (got.float() - want).abs().max().item()
        scale = want.abs().max().item()
        assert err < 3e-2 * max(1.0, scale), (mode, name, err, scale)


@pytest.mark.parametrize("causal,S,Sk", [(True, 300, 300), (False, 200, 520), (True, 520, 200), (False, 64, 1000)])
def test_flash_attention_fwd_v2_v3(causal, S, Sk, monkeypatch):
    """The LDS-DMA forward (v3, default) and the register-staged one (v2) against fp32, GQA and
    ragged / cross-attention lengths."""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(2)
    B, H, Hk, D = 2, 8, 2, 128
    q = torch.randn(B, S, H, D, device="cuda").bfloat16()
    k = torch.randn(B, Sk, Hk, D, device="cuda").bfloat16()
    v = torch.randn(B, Sk, Hk, D, device="cuda").bfloat16()
    ref = _ref_attn(q, k, v, causal)
    for mode in ("v2", "v3", "v4"):
        monkeypatch.setenv("PHA_FA_FWD", mode)
        o = hip.FlashAttention.apply(q, k, v, causal, None)
        assert (o.float() - ref).abs().max().item() < 2e-2, mode


@pytest.mark.parametrize("causal,S", [(True, 1100), (False, 520)])
def test_flash_attention_packed_delta_in_dq(causal, S, monkeypatch):
    """packed backward with delta = rowsum(dO * O) formed inside the dQ kernel (launched before dK/dV)
    against the separate preprocess pass (PHA_FA_DELTA_PASS=1) and fp32 SDPA"""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(12)
    B, H, D = 2, 4, 128
    qkv = torch.randn(B, S, H, 3 * D, device="cuda").bfloat16()
    do = torch.randn(B, S, H, D, device="cuda").bfloat16()
    res = {}
    for mode in ("inq", "pass"):
        if mode == "pass":
            monkeypatch.setenv("PHA_FA_DELTA_PASS", "1")
        a = qkv.clone().requires_grad_()
        o = hip.FlashAttentionPacked.apply(a, causal, None)
        (res[mode],) = torch.autograd.grad(o, a, do)
    assert (res["inq"].float() - res["pass"].float()).abs().max().item() < 1e-2 * res["pass"].float().abs().max().item()
    qf = qkv.float().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in qf.split(D, dim=-1))
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2)
    (gref,) = torch.autograd.grad(ref, qf, do.float())
    assert (res["inq"].float() - gref).abs().max().item() < 3e-2 * gref.abs().max().item()


@pytest.mark.parametrize("causal,S,Sk", [(True, 1100, 1100), (False, 700, 1300), (True, 2048, 2048)])
def test_flash_attention_fwd_v4_lse_and_grads(causal, S, Sk, monkeypatch):
    """the software-pipelined forward (v4): output vs fp32, and the backward that consumes its LSE
    gives v3's gradients"""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(4)
    B, H, D = 1, 4, 128
    q = torch.randn(B, S, H, D, device="cuda").bfloat16()
    k = torch.randn(B, Sk, H, D, device="cuda").bfloat16()
    v = torch.randn(B, Sk, H, D, device="cuda").bfloat16()
    do = torch.randn(B, S, H, D, device="cuda").bfloat16()
    res = {}
    for mode in ("v3", "v4"):
        monkeypatch.setenv("PHA_FA_FWD", mode)
        qq, kk, vv = (t.clone().requires_grad_() for t in (q, k, v))
        o = hip.FlashAttention.apply(qq, kk, vv, causal, None)
        res[mode] = (o.detach(), *torch.autograd.grad(o, (qq, kk, vv), do))
    ref = _ref_attn(q, k, v, causal)
    assert (res["v4"][0].float() - ref).abs().max().item() < 2e-2
    for a, b in zip(res["v4"], res["v3"]):
        assert (a.float() - b.float()).abs().max().item() < 2e-2 * max(1.0, b.float().abs().max().item())


def test_flash_attention_gqa():
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(0)
    q = torch.randn(1, 256, 8, 128, device="cuda").bfloat16()
    k = torch.randn(1, 256, 2, 128, device="cuda").bfloat16()
    v = torch.randn(1, 256, 2, 128, device="cuda").bfloat16()
    o = hip.FlashAttention.apply(q, k, v, True, None)
    ref = _ref_attn(q, k, v, True)
    assert (o.float() - ref).abs().max().item() < 2e-2


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [256, 320])
def test_flash_attention_qkv_packed(causal, S):
    """Packed [B,S,H,3D] path (strided reads, packed dqkv) == fp32 SDPA on the split views."""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(0)
    B, H, D = 2, 4, 128
    qkv = torch.randn(B, S, H, 3 * D, device="cuda").bfloat16().requires_grad_(True)
    assert hip.flash_attn_packed_supported(qkv, H)
    o = hip.FlashAttentionPacked.apply(qkv, causal, None)
    qr = qkv.detach().float().requires_grad_(True)
    q, k, v = qr.split(D, dim=-1)
    ref = _ref_attn(q, k, v, causal)
    assert (o.float() - ref).abs().max().item() < 2e-2
    g = torch.randn_like(ref)
    o.backward(g.bfloat16())
    ref.backward(g)
    err = (qkv.grad.float() - qr.grad).abs().max().item()
    assert err < 3e-2 * max(1.0, qr.grad.abs().max().item()), err


def _packed_case(causal):
    """one 128-query block of packed [B, S, H, 3D] attention: (qkv, dO, fp32 output, fp32 dqkv)"""
    torch.manual_seed(5)
    B, S, H, D = 1, 128, 2, 128
    qkv = torch.randn(B, S, H, 3 * D, device="cuda").bfloat16()
    do = torch.randn(B, S, H, D, device="cuda").bfloat16()
    qr = qkv.float().requires_grad_(True)
    ref = _ref_attn(*qr.split(D, dim=-1), causal)
    (gref,) = torch.autograd.grad(ref, qr, do.float())
    return qkv, do, ref.detach(), gref


@pytest.mark.parametrize("causal", [False, True])
def test_flash_attention_qkv_packed_fused_bwd(causal, monkeypatch):
    """PHA_FA_BWD=fused on the packed path: preprocess + the single-kernel backward writing dq | dk |
    dv into one packed gradient (pha_flash_attn_bwd_packed_fused) == fp32 SDPA"""
    from paddle_hackathon_amd.ops import hip
    monkeypatch.setenv("PHA_FA_BWD", "fused")
    L, calls = hip._L(), []
    real = L.pha_flash_attn_bwd_packed_fused
    monkeypatch.setattr(L, "pha_flash_attn_bwd_packed_fused", lambda *a: calls.append(1) or real(*a))
    qkv, do, ref, gref = _packed_case(causal)
    a = qkv.clone().requires_grad_(True)
    o = hip.FlashAttentionPacked.apply(a, causal, None)
    assert (o.float() - ref).abs().max().item() < 2e-2
    (g,) = torch.autograd.grad(o, a, do)
    assert calls, "the packed backward did not take the fused kernel"
    err = (g.float() - gref).abs().max().item()
    assert err < 3e-2 * max(1.0, gref.abs().max().item()), err


@pytest.mark.parametrize("causal", [False, True])
def test_flash_attention_bwd_packed_entry_point(causal):
    """pha_flash_attn_bwd_packed (the packed two-kernel backward reading a delta computed by the
    separate preprocess pass; the bindings call its _od sibling) called as exported == fp32 SDPA"""
    from paddle_hackathon_amd.ops import hip
    from paddle_hackathon_amd.ops.hip import _DT, _ptr, _stream
    qkv, do, ref, gref = _packed_case(causal)
    B, S, H, D = do.shape
    L, dt, sc, st = hip._L(), _DT[qkv.dtype], 1.0 / math.sqrt(D), _stream(qkv)
    o = torch.empty_like(do)
    lse = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    delta = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    g = torch.empty_like(qkv)
    assert L.pha_flash_attn_fwd_packed(dt, _ptr(qkv), _ptr(o), _ptr(lse), B, S, H, D, sc, int(causal), st) == 0
    assert (o.float() - ref).abs().max().item() < 2e-2
    assert L.pha_flash_attn_bwd_preprocess(dt, _ptr(o), _ptr(do), _ptr(delta), B, S, H, D, st) == 0
    assert L.pha_flash_attn_bwd_packed(dt, _ptr(qkv), _ptr(do), _ptr(lse), _ptr(delta), _ptr(g), B, S, H, D, sc,
                                       int(causal), st) == 0
    err = (g.float() - gref).abs().max().item()
    assert err < 3e-2 * max(1.0, gref.abs().max().item()), err


# ----------------------------------------------------------------------------- batch norm (NHWC)
def _bn_ref(x, w, b, res, relu, eps):
    xf = x.float()
    dims = tuple(range(x.dim() - 1))
    mean = xf.mean(dims)
    var = xf.var(dims, unbiased=False)
    y = (xf - mean) / torch.sqrt(var + eps) * w + b
    if res is not None:
        y = y + res.float()
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(8, 7, 7, 64), (4, 5, 3, 2048), (2, 3, 3, 4096), (3, 1, 1, 24), (1000, 8)])
@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, True)])
def test_batch_norm_nhwc_fwd_bwd(dt, shape, res, relu):
    from paddle_hackathon_amd.ops import fused
    torch.manual_seed(0)
    C = shape[-1]
    x = (torch.randn(shape, device="cuda") * 2 + 3).to(dt)  # non-zero mean exercises the shifted stats
    w = (torch.rand(C, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(C, device="cuda").requires_grad_(True)
    r = torch.randn(shape, device="cuda").to(dt) if res else None
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    xg = x.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True) if res else None
    y = fused.batch_norm_train(xg, w, b, rm, rv, 0.9, 1e-5, -1, residual=rg, relu=relu)
    assert y.grad_fn is not None and "BatchNormNHWC" in type(y.grad_fn).__name__  # HIP path ran
    xr = x.float().requires_grad_(True)
    wr, br = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    rr = r.float().requires_grad_(True) if res else None
    ref = _bn_ref(xr, wr, br, rr, relu, 1e-5)
    tol = _tol(dt) * 10
    assert torch.allclose(y.float(), ref, atol=tol, rtol=tol), (y.float() - ref).abs().max()
    # running stats: Paddle momentum semantics with unbiased variance
    dims = tuple(range(x.dim() - 1))
    assert torch.allclose(rm, 0.1 * x.float().mean(dims), atol=1e-3, rtol=1e-3)
    assert torch.allclose(rv, 0.9 + 0.1 * x.float().var(dims, unbiased=True), atol=1e-2, rtol=1e-2)
    dy = torch.randn(shape, device="cuda").to(dt)
    y.backward(dy)
    ref.backward(dy.float())
    assert torch.allclose(xg.grad.float(), xr.grad, atol=tol * 4, rtol=tol * 4), (xg.grad.float() - xr.grad).abs().max()
    assert torch.allclose(w.grad, wr.grad, atol=tol * 20, rtol=tol), (w.grad - wr.grad).abs().max()
    assert torch.allclose(b.grad, br.grad, atol=tol * 20, rtol=tol)
    if res:
        assert torch.allclose(rg.grad.float(), rr.grad, atol=tol, rtol=tol)


def test_batch_norm_large_m_stats_precision():
    """3.2M rows/channel with mean 50, std 0.5 — E[x^2]-E[x]^2 in fp32 would lose the variance."""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(1)
    x = (torch.randn(3200000, 64, device="cuda") * 0.5 + 50.0).to(torch.bfloat16)
    w, b = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    y, mean, istd, _ = hip.bn_fwd_train(x, w, b, None, None, 1e-5, 0.9)
    xf = x.double()
    assert torch.allclose(mean.double(), xf.mean(0), atol=1e-4)
    assert torch.allclose((1 / istd.double() ** 2), xf.var(0, unbiased=False), rtol=2e-3)


def test_batch_norm_infer_fused():
    from paddle_hackathon_amd.ops import fused
    x = torch.randn(4, 6, 6, 128, device="cuda").to(torch.bfloat16)
    w, b = torch.rand(128, device="cuda") + 0.5, torch.randn(128, device="cuda")
    rm, rv = torch.randn(128, device="cuda"), torch.rand(128, device="cuda") + 0.5
    r = torch.randn_like(x)
    with torch.no_grad():
        y = fused.batch_norm_infer(x, w, b, rm, rv, 1e-5, -1, residual=r, relu=True)
    ref = torch.relu((x.float() - rm) / torch.sqrt(rv + 1e-5) * w + b + r.float())
    assert torch.allclose(y.float(), ref, atol=5e-2, rtol=2e-2)


def test_resnet50_nhwc_step_uses_fused_bn():
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.vision.models import resnet50
    paddle.seed(0)
    m = resnet50(data_format="NHWC", num_classes=10)
    m = paddle.amp.decorate(m, level="O2", dtype="bfloat16")
    opt = paddle.optimizer.Momentum(0.01, parameters=m.parameters(), multi_precision=True)
    x = paddle.to_tensor(torch.randn(4, 64, 64, 3, device="cuda").to(torch.bfloat16))
    y = paddle.to_tensor(torch.randint(0, 10, (4,), device="cuda"))
    losses = []
    for _ in range(6):
        with paddle.amp.auto_cast(level="O2", dtype="bfloat16"):
            out = m(x)
        loss = paddle.nn.functional.cross_entropy(out, y)
        loss.backward()
        opt.step()
        opt.clear_grad()
        losses.append(float(loss))
    assert all(math.isfinite(l) for l in losses) and min(losses[2:]) < losses[0]
    assert float(m.bn1._variance.numpy().mean()) != 1.0  # running stats were updated by the HIP kernel


# ----------------------------------------------------------------------------- MFMA GEMM / implicit-GEMM conv
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 136, 264), (1024, 512, 4096), (8, 64, 8)])
def test_mfma_gemm_layouts(ta, tb, M, N, K):
    from paddle_hackathon_amd.ops import conv_gemm
    if ta and M % 8:
        pytest.skip("column-major A needs M % 8 == 0")
    torch.manual_seed(0)
    a = torch.randn((K, M) if ta else (M, K), device="cuda").to(torch.bfloat16)
    b = torch.randn((N, K) if tb else (K, N), device="cuda").to(torch.bfloat16)
    c = conv_gemm.matmul(a, b, ta, tb)
    ref = (a.float().t() if ta else a.float()) @ (b.float().t() if tb else b.float())
    err = (c.float() - ref).abs().max() / ref.abs().max()
    assert err < 1e-2, err


@pytest.mark.parametrize("act", [None, "relu", "gelu"])
@pytest.mark.parametrize("splitk", [1, 4])
def test_mfma_gemm_epilogue_and_splitk(act, splitk):
    from paddle_hackathon_amd.ops import conv_gemm
    torch.manual_seed(1)
    M, N, K = 96, 256, 2048
    a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    bt = torch.randn(N, K, device="cuda").to(torch.bfloat16)
    bias = torch.randn(N, device="cuda")
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    conv_gemm.gemm_raw(conv_gemm.A_ROW, conv_gemm.B_ROW, a, K, bt, K, out, N, M, N, K, bias=bias, act=act,
                       splitk=splitk)
    ref = a.float() @ bt.float().t() + bias
    ref = {None: ref, "relu": torch.relu(ref), "gelu": TF.gelu(ref)}[act]
    assert (out.float() - ref).abs().max() / ref.abs().max() < 1e-2


def test_linear_own_gemm_fwd_bwd(monkeypatch):
    """PHA_MATMUL_IMPL=hip: linear (x @ W + b) and tied-logits (x @ E^T) forward and both
    gradients on gemm8p vs fp32 torch"""
    from paddle_hackathon_amd.ops import conv_gemm
    monkeypatch.setenv("PHA_MATMUL_IMPL", "hip")
    torch.manual_seed(5)
    x = torch.randn(2, 136, 256, device="cuda").bfloat16().requires_grad_(True)
    w = (torch.randn(256, 392, device="cuda") * 0.05).bfloat16().requires_grad_(True)
    b = torch.randn(392, device="cuda").bfloat16().requires_grad_(True)
    assert conv_gemm.linear_ok(x, w)
    y = conv_gemm.linear(x, w, b)
    xr, wr, br = (t.detach().float().requires_grad_(True) for t in (x, w, b))
    yr = xr @ wr + br
    gy = torch.randn_like(yr)
    y.backward(gy.bfloat16())
    yr.backward(gy)
    rel = lambda a, r: ((a.float() - r).abs().max() / r.abs().max()).item()
    assert rel(y, yr) < 1e-2 and rel(x.grad, xr.grad) < 1e-2 and rel(w.grad, wr.grad) < 1e-2
    assert rel(b.grad, br.grad) < 1e-2
    e = (torch.randn(504, 256, device="cuda") * 0.05).bfloat16().requires_grad_(True)
    x.grad = None
    z = conv_gemm.matmul_nt(x, e)
    er = e.detach().float().requires_grad_(True)
    xr.grad = None
    zr = xr @ er.t()
    gz = torch.randn_like(zr)
    z.backward(gz.bfloat16())
    zr.backward(gz)
    assert rel(z, zr) < 1e-2 and rel(x.grad, xr.grad) < 1e-2 and rel(e.grad, er.grad) < 1e-2


def test_conv_layout_cache_sees_optimizer_updates():
    """the conv filter re-layout cache is keyed by the parameter version: a step of the HIP
    multi-tensor optimizer (raw-pointer writes) must invalidate it"""
    import paddle_hackathon_amd as paddle
    paddle.set_device("gpu:0")
    paddle.seed(9)
    conv = paddle.nn.Conv2D(16, 32, 3, padding=1, bias_attr=False, data_format="NHWC")
    conv.to(dtype="bfloat16")
    opt = paddle.optimizer.Momentum(learning_rate=0.5, momentum=0.9, parameters=conv.parameters())
    x = paddle.to_tensor(torch.randn(2, 8, 8, 16, device="cuda").bfloat16())
    for _ in range(2):
        y = conv(x)
        (y * y).mean().backward()
        opt.step()
        opt.clear_grad()
    y = conv(x)._t.float()
    w = conv.weight._t.float()
    ref = TF.conv2d(x._t.float().permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1)
    assert (y - ref).abs().max() / ref.abs().max() < 2e-2


@pytest.mark.parametrize("cfg", [(2, 17, 15, 64, 3, 2, 1), (3, 8, 8, 16, 2, 2, 0), (2, 12, 12, 24, 3, 1, 1)])
def test_maxpool2d_nhwc(cfg):
    """NHWC max pool fwd/bwd HIP kernels vs torch (ResNet stem: 3x3 s2 p1)"""
    import paddle_hackathon_amd as paddle
    import paddle_hackathon_amd.nn.functional as F
    N, H, W, C, k, st, p = cfg
    torch.manual_seed(14)
    x = torch.randn(N, H, W, C, device="cuda").bfloat16().requires_grad_(True)
    y = F.max_pool2d(paddle.Tensor(x), k, st, p, data_format="NHWC")._t
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    yr = TF.max_pool2d(xr, k, st, p).permute(0, 2, 3, 1)
    assert torch.equal(y.float(), yr)
    gy = torch.randn_like(yr)
    y.backward(gy.bfloat16())
    yr.backward(gy.bfloat16().float())
    assert torch.allclose(x.grad.float(), xr.grad.permute(0, 2, 3, 1), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("shape", [(64, 64), (136, 200), (2048, 520)])
def test_transpose16(shape):
    from paddle_hackathon_amd.ops import conv_gemm
    t = torch.randn(*shape, device="cuda").bfloat16()
    assert torch.equal(conv_gemm._transpose2d(t), t.t().contiguous())


def test_linear_nt_forward_tracks_updates():
    """x @ W through the cached transposed weight: gradients vs fp32, and after an AdamW step
    (raw-pointer update) the cache is refreshed"""
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import conv_gemm
    paddle.set_device("gpu:0")
    paddle.seed(10)
    lin = paddle.nn.Linear(64, 96)
    lin.to(dtype="bfloat16")
    x = torch.randn(40, 64, device="cuda").bfloat16().requires_grad_(True)
    y = paddle.nn.functional.linear(paddle.Tensor(x), lin.weight, lin.bias)._t
    xr, wr, br = (t.detach().float().requires_grad_(True) for t in (x, lin.weight._t, lin.bias._t))
    gy = torch.randn(40, 96, device="cuda")
    y.backward(gy.bfloat16())
    (xr @ wr + br).backward(gy)
    for a, r in ((y.detach(), (xr @ wr + br).detach()), (x.grad, xr.grad), (lin.weight._t.grad, wr.grad),
                 (lin.bias._t.grad, br.grad)):
        assert (a.float() - r).abs().max() / r.abs().max() < 1e-2
    opt = paddle.optimizer.AdamW(learning_rate=0.1, parameters=lin.parameters())
    opt.step()
    y2 = conv_gemm.matmul_kn(x.detach(), lin.weight._t)
    ref = x.detach().float() @ lin.weight._t.float()
    assert (y2.float() - ref).abs().max() / ref.abs().max() < 1e-2


def test_linear_bias_grad_col_sum():
    """F.linear with bias on bf16: bias gradient from the HIP column-sum kernel, vs fp32 torch"""
    import paddle_hackathon_amd as paddle
    import paddle_hackathon_amd.nn.functional as F
    torch.manual_seed(8)
    x = torch.randn(3, 100, 64, device="cuda").bfloat16().requires_grad_(True)
    w = (torch.randn(64, 136, device="cuda") * 0.1).bfloat16().requires_grad_(True)
    b = torch.randn(136, device="cuda").bfloat16().requires_grad_(True)
    y = F.linear(paddle.Tensor(x), paddle.Tensor(w), paddle.Tensor(b))._t
    gy = torch.randn_like(y.float())
    y.backward(gy.bfloat16())
    xr, wr, br = (t.detach().float().requires_grad_(True) for t in (x, w, b))
    (xr @ wr + br).backward(gy)
    for a, r in ((x.grad, xr.grad), (w.grad, wr.grad), (b.grad, br.grad)):
        assert (a.float() - r).abs().max() / r.abs().max() < 1e-2


def test_adamw_fused_global_norm_clip():
    """ClipGradByGlobalNorm folded into the multi-tensor AdamW kernel == clip pass + AdamW"""
    import paddle_hackathon_amd as paddle
    torch.manual_seed(6)
    paddle.set_device("gpu:0")
    ref = None
    outs = []
    for fused in (True, False):
        paddle.seed(7)
        lin = paddle.nn.Linear(64, 32)
        opt = paddle.optimizer.AdamW(learning_rate=1e-2, parameters=lin.parameters(), weight_decay=0.1,
                                     grad_clip=paddle.nn.ClipGradByGlobalNorm(0.05))
        opt._fuses_grad_scale = fused
        for _ in range(3):
            x = paddle.to_tensor(torch.randn(16, 64, device="cuda", generator=torch.Generator("cuda").manual_seed(1)))
            loss = (lin(x) ** 2).mean() * 100.0
            loss.backward()
            opt.step()
            opt.clear_grad()
        outs.append(lin.weight._t.detach().clone())
    assert torch.allclose(outs[0], outs[1], rtol=1e-5, atol=1e-6), (outs[0] - outs[1]).abs().max()


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_dgrad_fused_bn_backward(monkeypatch, stride):
    """conv -> BN+ReLU -> conv: the second conv's dgrad epilogue reduces the BN backward sums
    (the BN skips its reduction pass); every gradient equals the unfused path"""
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import hip
    paddle.set_device("gpu:0")
    seen = []
    orig = hip.bn_bwd

    def spy(*a, **k):
        seen.append(k.get("ext_part") is not None)
        return orig(*a, **k)
    monkeypatch.setattr(hip, "bn_bwd", spy)
    grads = []
    for fused in ("1", "0"):
        monkeypatch.setenv("PHA_CONV_BN_STATS", fused)
        monkeypatch.setenv("PHA_CONV_BN_BWD", fused)
        paddle.seed(13)
        c1 = paddle.nn.Conv2D(16, 32, 1, bias_attr=False, data_format="NHWC")
        bn = paddle.nn.BatchNorm2D(32, data_format="NHWC")
        c2 = paddle.nn.Conv2D(32, 64, 3, stride=stride, padding=1, bias_attr=False, data_format="NHWC")
        for l in (c1, c2):   # BN keeps fp32 parameters / running stats (as AMP O2 does)
            l.to(dtype="bfloat16")
        x = paddle.to_tensor(torch.randn(4, 12, 12, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(2)).bfloat16())
        from paddle_hackathon_amd.vision.models.resnet import _bn_act
        y = c2(_bn_act(bn, c1(x)))
        (y.astype("float32") ** 2).mean().backward()
        grads.append([p._t.grad.float().clone() for p in (c1.weight, bn.weight, bn.bias, c2.weight)])
    assert seen[0] and not seen[-1]
    for a, b in zip(*grads):
        assert (a - b).abs().max() / b.abs().max() < 2e-2


def test_conv_epilogue_bn_stats():
    """the conv forward epilogue's batch-norm partial sums match the output, and the BN that
    consumes them gives the same normalisation / running stats as its own statistics pass"""
    from paddle_hackathon_amd.ops import conv_gemm, fused
    torch.manual_seed(4)
    x = torch.randn(4, 20, 20, 64, device="cuda").bfloat16()
    w = (torch.randn(128, 64, 3, 3, device="cuda") * 0.05).bfloat16()
    y = conv_gemm.conv2d_nhwc256(x, w, None, (1, 1), (1, 1), (1, 1))
    part, rows, ver = y._pha_bn_stats
    assert ver == y._version and rows == -(-y.numel() // 128 // 128) or rows > 0
    s = part[: rows * 2 * 128].view(rows, 2, 128).double().sum(0)
    yf = y.double().reshape(-1, 128)
    assert torch.allclose(s[0], yf.sum(0), rtol=1e-4, atol=1e-2)
    assert torch.allclose(s[1], (yf * yf).sum(0), rtol=1e-4, atol=1e-2)
    g, b = torch.rand(128, device="cuda") + 0.5, torch.randn(128, device="cuda")
    rm1, rv1 = torch.zeros(128, device="cuda"), torch.ones(128, device="cuda")
    rm2, rv2 = rm1.clone(), rv1.clone()
    out1 = fused.batch_norm_train(y, g, b, rm1, rv1, 0.9, 1e-5, -1, relu=True)
    y2 = y.clone()   # no partials attached: the BN's own statistics pass
    out2 = fused.batch_norm_train(y2, g, b, rm2, rv2, 0.9, 1e-5, -1, relu=True)
    assert (out1.float() - out2.float()).abs().max() < 2e-2
    assert torch.allclose(rm1, rm2, atol=1e-4) and torch.allclose(rv1, rv2, rtol=1e-3)


@pytest.mark.parametrize("layout", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("shape", [(264, 520, 200), (512, 768, 1024), (1024, 256, 4096)])
def test_gemm8p_layouts(layout, shape):
    """8-phase ping-pong GEMM, every operand layout (row reads / transposed reads), ragged tiles
    and K tails, bias + GELU epilogue, vs fp32 torch"""
    from paddle_hackathon_amd.ops import conv_gemm
    ako, bko = layout
    M, N, K = shape
    torch.manual_seed(3)
    a = torch.randn(K, M, device="cuda").bfloat16() if ako else torch.randn(M, K, device="cuda").bfloat16()
    b = torch.randn(K, N, device="cuda").bfloat16() if bko else torch.randn(N, K, device="cuda").bfloat16()
    A = a.t().float() if ako else a.float()
    B = b.float() if bko else b.t().float()
    ref = A @ B
    c = conv_gemm.gemm8p(a, b, ako, bko)
    assert (c.float() - ref).abs().max() / ref.abs().max() < 1e-2
    bias = torch.randn(N, device="cuda")
    c = conv_gemm.gemm8p(a, b, ako, bko, bias=bias, act="gelu")
    ref = TF.gelu(ref + bias, approximate="tanh")
    assert (c.float() - ref).abs().max() / ref.abs().max() < 1e-2


@pytest.mark.parametrize("splits", [2, 3, 8])
def test_gemm8p_split_k(splits):
    """split-K weight-gradient layout (A, B k-outer) with bias + ReLU applied by the reduction"""
    from paddle_hackathon_amd.ops import conv_gemm
    torch.manual_seed(12)
    x = torch.randn(3000, 264, device="cuda").bfloat16()
    gy = torch.randn(3000, 520, device="cuda").bfloat16()
    bias = torch.randn(520, device="cuda")
    c = conv_gemm.gemm8p(x, gy, True, True, bias=bias, act="relu", splits=splits)
    ref = torch.relu(x.float().t() @ gy.float() + bias)
    assert (c.float() - ref).abs().max() / ref.abs().max() < 1e-2
    dw = conv_gemm.weight_grad(x, gy)
    ref = x.float().t() @ gy.float()
    assert (dw.float() - ref).abs().max() / ref.abs().max() < 1e-2


@pytest.mark.parametrize("shape", [(64, 128, 1000), (512, 384, 4096), (200, 136, 77)])
@pytest.mark.parametrize("out_f32", [False, True])
def test_gemm256_tn_weight_grad(shape, out_f32):
    """C = A^T B with K-outer operands (split-K, transposed LDS reads) vs fp32 torch"""
    from paddle_hackathon_amd.ops import conv_gemm
    M, N, K = shape
    torch.manual_seed(2)
    a = torch.randn(K, M, device="cuda").to(torch.bfloat16)
    b = torch.randn(K, N, device="cuda").to(torch.bfloat16)
    c = conv_gemm.gemm256_tn(a, b, out_dtype=torch.float32 if out_f32 else None)
    ref = a.float().t() @ b.float()
    assert c.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    assert (c.float() - ref).abs().max() / ref.abs().max() < 1e-2
    acc = torch.ones(M, N, device="cuda", dtype=c.dtype)
    conv_gemm.gemm256_tn(a, b, out=acc, accumulate=True)
    assert (acc.float() - 1 - ref).abs().max() / ref.abs().max() < 1e-2


@pytest.mark.parametrize("cfg", [
    # N, H, W, Cin, Cout, k, stride, pad, dil
    (2, 14, 14, 64, 64, 1, 1, 0, 1),
    (2, 14, 14, 64, 128, 3, 1, 1, 1),
    (2, 15, 13, 32, 64, 3, 2, 1, 1),
    (2, 14, 14, 64, 128, 1, 2, 0, 1),
    (2, 32, 32, 3, 64, 7, 2, 3, 1),
    (1, 12, 12, 16, 32, 3, 1, 2, 2),
    (3, 9, 9, 24, 40, 5, 2, 2, 1),
])
def test_conv2d_nhwc_fwd_bwd(cfg):
    from paddle_hackathon_amd.nn.functional.conv import _hip_conv2d
    N, H, W, Ci, Co, k, s, p, d = cfg
    torch.manual_seed(0)
    x = torch.randn(N, H, W, Ci, device="cuda").to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(Co, Ci, k, k, device="cuda") / (Ci * k * k) ** 0.5).to(torch.bfloat16).requires_grad_(True)
    y = _hip_conv2d(x, w, None, [s, s], [p, p], [d, d], 1)
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    ref = TF.conv2d(xr, wr, None, s, p, d).permute(0, 2, 3, 1)
    assert y.shape == ref.shape
    scale = ref.abs().max()
    assert (y.float() - ref).abs().max() / scale < 2e-2
    gy = torch.randn_like(ref)
    y.backward(gy.to(torch.bfloat16))
    ref.backward(gy)
    gx = xr.grad.permute(0, 2, 3, 1)
    assert (x.grad.float() - gx).abs().max() / gx.abs().max() < 3e-2
    assert (w.grad.float() - wr.grad).abs().max() / wr.grad.abs().max() < 3e-2


def test_conv_layer_nhwc_routes_to_hip(monkeypatch):
    import paddle_hackathon_amd as paddle
    monkeypatch.setenv("PHA_CONV_IMPL", "hip")
    conv = paddle.nn.Conv2D(16, 32, 3, padding=1, data_format="NHWC")
    conv = paddle.amp.decorate(conv, level="O2", dtype="bfloat16")
    x = paddle.to_tensor(torch.randn(2, 8, 8, 16, device="cuda").to(torch.bfloat16))
    x.stop_gradient = False
    y = conv(x)
    assert "Conv2dNHWC" in type(y._t.grad_fn).__name__
    y.mean().backward()
    assert conv.weight.grad is not None and x.grad is not None


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_multi_tensor_l2norm_sq_vector_and_tail(dt):
    """global-norm partial sums (16-byte vector bulk + scalar tail, misaligned views fall back to
    the scalar loop) == fp32 torch sum of squares over chunk-crossing, odd and offset tensors"""
    from paddle_hackathon_amd.ops import hip
    torch.manual_seed(0)
    base = torch.randn(70001, device="cuda").to(dt)
    ts = [torch.randn(16384 * 3 + 5, device="cuda").to(dt), torch.randn(7, device="cuda").to(dt),
          base[3:], base[:40000], torch.randn(2048, 2048, device="cuda").to(dt)]
    got = hip.multi_tensor_l2norm_sq(ts)
    ref = sum((t.float() ** 2).sum() for t in ts)
    assert abs(float(got) - float(ref)) <= 1e-4 * float(ref)


@pytest.mark.parametrize("sched", [0, 2])
@pytest.mark.parametrize("ako,bko", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (264, 520, 128), (1024, 768, 640)])
def test_gemm4w_layouts(monkeypatch, sched, ako, bko, M, N, K):
    """one-wave-per-SIMD 256x256x64 GEMM (gemm4w.hip), every operand layout and schedule vs fp32"""
    from paddle_hackathon_amd.ops import gemm as G
    monkeypatch.setenv("PHA_G4W_SCHED", str(sched))
    torch.manual_seed(2)
    a = (torch.rand((K, M) if ako else (M, K), device="cuda") * 2 - 1).bfloat16()
    b = (torch.rand((K, N) if bko else (N, K), device="cuda") * 2 - 1).bfloat16()
    ref = (a.float().t() if ako else a.float()) @ (b.float() if bko else b.float().t())
    c = G.gemm(a, b, ako, bko)
    assert (c.float() - ref).abs().max() / ref.abs().max() < 1e-2


@pytest.mark.parametrize("sched", [0, 2])
@pytest.mark.parametrize("M,N,K", [(264, 520, 128), (4096, 2304, 256)])
def test_gemm4w_nt_epilogue_builds(monkeypatch, sched, M, N, K):
    """NT layout: plain, bias, and the dGELU + column-sum build (batched epilogue stores)"""
    from paddle_hackathon_amd.ops import gemm as G
    monkeypatch.setenv("PHA_G4W_SCHED", str(sched))
    torch.manual_seed(6)
    a = (torch.rand(M, K, device="cuda") * 2 - 1).bfloat16()
    bt = (torch.rand(N, K, device="cuda") * 2 - 1).bfloat16()
    ref = a.float() @ bt.float().t()
    c = G.gemm(a, bt, False, False)
    assert (c.float() - ref).abs().max() / ref.abs().max() < 1e-2
    bias = torch.randn(N, device="cuda")
    c = G.gemm(a, bt, False, False, bias=bias)
    assert (c.float() - ref - bias).abs().max() / ref.abs().max() < 1e-2
    pre = (torch.rand(M, N, device="cuda") * 2 - 1).bfloat16()
    dh, part = G.gemm(a, bt, False, False, act="dgelu", aux=pre, colsum=True)
    xg = pre.float().requires_grad_()
    dref = torch.autograd.grad(TF.gelu(xg, approximate="tanh"), xg, ref)[0]
    assert (dh.float() - dref).abs().max() / dref.abs().max() < 1e-2
    db = G.colsum_finish(part, torch.float32)
    assert (db - dref.sum(0)).abs().max() / dref.sum(0).abs().max() < 1e-2


def test_gemm4w_fused_epilogues():
    """bias + tanh-GELU with the pre-activation stored; dGELU against a stored pre-activation with
    the bias-gradient column sums (fused_gemm_epilogue semantics) vs fp32 torch"""
    from paddle_hackathon_amd.ops import gemm as G
    torch.manual_seed(3)
    M, N, K = 520, 768, 256
    x = (torch.rand(M, K, device="cuda") * 2 - 1).bfloat16()
    w = (torch.rand(K, N, device="cuda") * 2 - 1).bfloat16()
    bias = torch.randn(N, device="cuda")
    act, pre = G.nn(x, w, bias=bias, act="gelu", aux_out=True)
    h = x.float() @ w.float() + bias
    assert (pre.float() - h).abs().max() / h.abs().max() < 1e-2
    g = TF.gelu(h, approximate="tanh")
    assert (act.float() - g).abs().max() / g.abs().max() < 1e-2
    dy = (torch.rand(M, K, device="cuda") * 2 - 1).bfloat16()
    wt = (torch.rand(N, K, device="cuda") * 2 - 1).bfloat16()
    da = dy.float() @ wt.float().t()
    hp = pre.float().requires_grad_()
    dh_ref = torch.autograd.grad(TF.gelu(hp, approximate="tanh"), hp, da)[0]
    dh, part = G.gemm(dy, wt, False, False, act="dgelu", aux=pre, colsum=True)
    assert (dh.float() - dh_ref).abs().max() / dh_ref.abs().max() < 1e-2
    db = G.colsum_finish(part, torch.float32)   # sums of the fp32 values, before the bf16 rounding
    ref_db = dh_ref.sum(0)
    assert (db - ref_db).abs().max() / ref_db.abs().max() < 1e-2
    relu = G.gemm(x, w, False, True, bias=bias, act="relu")
    assert (relu.float() - torch.relu(h)).abs().max() / h.abs().max() < 1e-2


@pytest.mark.parametrize("sched", [0, 2])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (264, 520, 128), (1032, 768, 640), (4096, 2304, 256),
                                   (264, 576, 128)])
def test_gemm4w_transposed_store(monkeypatch, sched, M, N, K):
    """x @ W as (W^T x^T)^T on the A-K-outer layout with the transposed-store epilogue (ops/gemm.nn)
    including bias + GELU + stored pre-activation and dGELU + column sums, vs fp32"""
    from paddle_hackathon_amd.ops import gemm as G
    monkeypatch.setenv("PHA_G4W_SCHED", str(sched))
    torch.manual_seed(5)
    x = (torch.rand(M, K, device="cuda") * 2 - 1).bfloat16()
    w = (torch.rand(K, N, device="cuda") * 2 - 1).bfloat16()
    ref = x.float() @ w.float()
    c = G.nn(x, w)
    assert c.shape == (M, N) and (c.float() - ref).abs().max() / ref.abs().max() < 1e-2
    bias = torch.randn(N, device="cuda")
    act, pre = G.nn(x, w, bias=bias, act="gelu", aux_out=True)
    h = ref + bias
    assert (pre.float() - h).abs().max() / h.abs().max() < 1e-2
    assert (act.float() - TF.gelu(h, approximate="tanh")).abs().max() / h.abs().max() < 1e-2
    if N % 64:   # the dGELU product below reduces over N
        return
    dy = (torch.rand(M, N, device="cuda") * 2 - 1).bfloat16()
    hp = (torch.rand(M, K, device="cuda") * 2 - 1).bfloat16()
    dh, part = G.nn(dy, w.t().contiguous(), act="dgelu", aux=hp, colsum=True)
    xg = hp.float().requires_grad_()
    dh_ref = torch.autograd.grad(TF.gelu(xg, approximate="tanh"), xg, dy.float() @ w.float().t())[0]
    assert (dh.float() - dh_ref).abs().max() / dh_ref.abs().max() < 1e-2
    db = G.colsum_finish(part, torch.float32)
    assert (db - dh_ref.sum(0)).abs().max() / dh_ref.sum(0).abs().max() < 1e-2


@pytest.mark.parametrize("impl", ["auto", "own", "library"])
def test_gemm_picks_match_reference(impl, monkeypatch):
    """the dispatch entry points (mm_nt / mm_nn / mm_tn incl. split-K / mm_nt_bias) under every
    PHA_GEMM_IMPL policy vs fp32"""
    from paddle_hackathon_amd.ops import gemm as G
    monkeypatch.setenv("PHA_GEMM_IMPL", impl)
    torch.manual_seed(4)
    a = (torch.rand(512, 256, device="cuda") * 2 - 1).bfloat16()
    bt = (torch.rand(384, 256, device="cuda") * 2 - 1).bfloat16()
    b = (torch.rand(256, 384, device="cuda") * 2 - 1).bfloat16()
    dy = (torch.rand(512, 128, device="cuda") * 2 - 1).bfloat16()
    xk = (torch.rand(4096, 256, device="cuda") * 2 - 1).bfloat16()     # long-K weight gradient: split-K
    dk = (torch.rand(4096, 512, device="cuda") * 2 - 1).bfloat16()
    bias = torch.randn(384, device="cuda").bfloat16()
    for got, ref in [(G.mm_nt(a, bt), a.float() @ bt.float().t()), (G.mm_nn(a, b), a.float() @ b.float()),
                     (G.mm_tn(a, dy), a.float().t() @ dy.float()),
                     (G.mm_tn(xk, dk), xk.float().t() @ dk.float()),
                     (G.mm_nt_bias(a, bt, bias), a.float() @ bt.float().t() + bias.float())]:
        assert got.shape == ref.shape
        assert (got.float() - ref).abs().max() / ref.abs().max() < 1e-2


def _attn_ref(q, k, v, causal, scale, bias=None, keep=None, rate=0.0):
    """fp32 attention on [B, S, H, D] with an additive bias [*, *, S, Sk] and a fixed keep mask"""
    qt, kt, vt = (t.float().transpose(1, 2) for t in (q, k, v))
    if kt.shape[1] != qt.shape[1]:
        g = qt.shape[1] // kt.shape[1]
        kt, vt = kt.repeat_interleave(g, 1), vt.repeat_interleave(g, 1)
    s = (qt @ kt.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias
    if causal:
        S, Sk = s.shape[-2:]
        s = s.masked_fill(torch.ones(S, Sk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep / (1.0 - rate)
    return (p @ vt).transpose(1, 2)


@pytest.mark.parametrize("D", [32, 64, 80, 96, 128, 192, 256])
@pytest.mark.parametrize("mask_kind", ["keypad", "full", "bool"])
@pytest.mark.parametrize("causal", [False, True])
def test_flash_attention_mask_and_head_dims(D, mask_kind, causal, monkeypatch):
    """additive key-padding [B,1,1,Sk], full [B,H,S,Sk] and boolean masks, head dims 32..256
    (80/96/192 zero-padded), forward + all input gradients vs fp32"""
    from paddle_hackathon_amd import ops
    monkeypatch.setenv("PHA_FA_WIDE", "own")
    torch.manual_seed(11)
    B, S, H = 2, 200, 3
    q = torch.randn(B, S, H, D, device="cuda").bfloat16().requires_grad_()
    k = torch.randn(B, S, H, D, device="cuda").bfloat16().requires_grad_()
    v = torch.randn(B, S, H, D, device="cuda").bfloat16().requires_grad_()
    if mask_kind == "keypad":
        lens = torch.tensor([S - 37, S], device="cuda")
        mask = torch.where(torch.arange(S, device="cuda")[None, :] < lens[:, None], 0.0, -1e4).reshape(B, 1, 1, S)
        bias = mask
    elif mask_kind == "full":
        mask = torch.randn(B, H, S, S, device="cuda")
        bias = mask
    else:
        mask = torch.rand(B, 1, S, S, device="cuda") > 0.2
        mask[..., 0] = True
        bias = torch.zeros(mask.shape, device="cuda").masked_fill(~mask, float("-inf"))
    scale = 1.0 / math.sqrt(D)
    o = ops.flash_attention(q, k, v, causal=causal, mask=mask)
    ref = _attn_ref(q, k, v, causal, scale, bias)
    assert (o.float() - ref).abs().max() < 3e-2
    do = torch.randn_like(o)
    g = torch.autograd.grad(o, (q, k, v), do)
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    gr = torch.autograd.grad(_attn_ref(qr, kr, vr, causal, scale, bias), (qr, kr, vr), do.float())
    for a, b in zip(g, gr):
        assert (a.float() - b).abs().max() / b.abs().max() < 3e-2


@pytest.mark.parametrize("D", [160, 256])
@pytest.mark.parametrize("causal", [False, True])
def test_flash_attention_head_dim_256(D, causal, monkeypatch):
    """head dims above 128 (no mask): the own generic kernels at D = 256 (PHA_FA_WIDE=own),
    forward + gradients vs fp32, and no fallback to torch SDPA"""
    from paddle_hackathon_amd import ops
    monkeypatch.setenv("PHA_FA_WIDE", "own")
    from paddle_hackathon_amd.ops import fallback
    torch.manual_seed(5)
    B, S, H = 2, 300, 4
    q, k, v = (torch.randn(B, S, H, D, device="cuda").bfloat16().requires_grad_() for _ in range(3))
    fallback.reset()
    o = ops.flash_attention(q, k, v, causal=causal)
    assert fallback.total() == 0, fallback.counts()
    scale = 1.0 / math.sqrt(D)
    ref = _attn_ref(q, k, v, causal, scale, None)
    assert (o.float() - ref).abs().max() < 3e-2
    do = torch.randn_like(o)
    g = torch.autograd.grad(o, (q, k, v), do)
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    gr = torch.autograd.grad(_attn_ref(qr, kr, vr, causal, scale, None), (qr, kr, vr), do.float())
    for a, b in zip(g, gr):
        assert (a.float() - b).abs().max() / b.abs().max() < 3e-2


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("with_mask", [False, True])
def test_flash_attention_dropout_regenerated_in_backward(rate, with_mask):
    """in-kernel dropout: the keep mask is read back through V = I (O = dropped P), its density is
    1 - rate, and forward + backward equal the fp32 reference with that same mask"""
    from paddle_hackathon_amd import ops
    B, S, H, D = 2, 64, 2, 64
    torch.manual_seed(7)
    q = torch.randn(B, S, H, D, device="cuda").bfloat16()
    k = torch.randn(B, S, H, D, device="cuda").bfloat16()
    mask = None
    bias = None
    if with_mask:
        mask = torch.where(torch.arange(S, device="cuda") < S - 5, 0.0, -1e4).reshape(1, 1, 1, S).expand(B, 1, 1, S)
        bias = mask
    eye = torch.eye(S, device="cuda").bfloat16()[None, :, None, :].expand(B, S, H, S).contiguous()
    torch.manual_seed(123)
    pd = ops.flash_attention(q, k, eye, dropout_p=rate, training=True, mask=mask).float()   # [B, S, H, Sk]
    keep = (pd != 0).transpose(1, 2).float()                                                 # [B, H, S, Sk]
    valid = torch.ones_like(keep) if mask is None else (bias.expand_as(keep) == 0).float()
    frac = (keep * valid).sum() / valid.sum()
    assert abs(frac.item() - (1 - rate)) < 0.03, frac
    v = torch.randn(B, S, H, D, device="cuda").bfloat16()
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    torch.manual_seed(123)   # same stream as the probe above
    o = ops.flash_attention(qg, kg, vg, dropout_p=rate, training=True, mask=mask)
    scale = 1.0 / math.sqrt(D)
    ref = _attn_ref(q, k, v, False, scale, bias, keep, rate)
    assert (o.float() - ref).abs().max() / ref.abs().max() < 3e-2
    do = torch.randn_like(o)
    g = torch.autograd.grad(o, (qg, kg, vg), do)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    gr = torch.autograd.grad(_attn_ref(qr, kr, vr, False, scale, bias, keep, rate), (qr, kr, vr), do.float())
    for a, b in zip(g, gr):
        assert (a.float() - b).abs().max() / b.abs().max() < 3e-2


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rate,with_mask", [(0.1, True), (0.0, True), (0.2, False)])
def test_flash_attention_packed_ext_writes_strided_grads(D, rate, with_mask):
    """packed [B, S, H, 3D] entry with mask / dropout: dq | dk | dv written through the kernels'
    output strides equal (bitwise) the split path's dense gradients concatenated"""
    from paddle_hackathon_amd import ops
    from paddle_hackathon_amd.ops import hip
    B, S, H = 2, 136, 3
    torch.manual_seed(5)
    qkv = torch.randn(B, S, H, 3 * D, device="cuda").bfloat16()
    mask = None
    if with_mask:
        mask = torch.where(torch.arange(S, device="cuda") < S - 9, 0.0, -1e4).reshape(1, 1, 1, S).expand(B, 1, 1, S)
    a = qkv.clone().requires_grad_()
    torch.manual_seed(99)
    o1 = ops.flash_attention_qkvpacked(a, H, dropout_p=rate, training=True, mask=mask)
    assert o1.grad_fn is not None and "FlashAttentionExtPacked" in type(o1.grad_fn).__name__
    do = torch.randn_like(o1)
    (g1,) = torch.autograd.grad(o1, a, do)
    b = qkv.clone().requires_grad_()
    q, k, v = b.split(D, dim=-1)
    torch.manual_seed(99)
    o2 = hip.FlashAttentionExt.apply(q, k, v, False, 1.0 / math.sqrt(D), mask, float(rate))
    (g2,) = torch.autograd.grad(o2, b, do)
    assert torch.equal(o1, o2)
    assert torch.equal(g1, g2)


def test_bert_attention_runs_on_own_kernels():
    """BERT-base attention (dropout 0.1, key-padding mask) goes to FlashAttentionExt, not SDPA"""
    from paddle_hackathon_amd.ops import hip
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import bert_config, BertForPretraining
    calls = {"n": 0}
    orig = hip.FlashAttentionExt.forward

    def counting(ctx, *a):
        calls["n"] += 1
        return orig(ctx, *a)
    hip.FlashAttentionExt.forward = staticmethod(counting)
    try:
        paddle.set_device("gpu:0")
        cfg = bert_config("bert-tiny")
        m = paddle.amp.decorate(BertForPretraining(cfg), level="O2", dtype="bfloat16")
        ids = paddle.to_tensor(torch.randint(0, cfg.vocab_size, (2, 64), device="cuda"))
        with paddle.amp.auto_cast(level="O2", dtype="bfloat16"):
            mlm, nsp = m(ids)
        (mlm.astype("float32").mean() + nsp.astype("float32").mean()).backward()
    finally:
        hip.FlashAttentionExt.forward = orig
    assert calls["n"] >= cfg.num_layers


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_bias_dropout_residual_layer_norm_kernel(dtype):
    """fused bias + dropout + residual + LayerNorm (ops/fused.py _BiasDropoutResidualLN) vs the fp32
    composite at p = 0, and the regenerated-mask identities at p > 0."""
    from paddle_hackathon_amd.ops import fused as FU
    torch.manual_seed(0)
    R, H = 2048, 768
    x = torch.randn(R, H, device="cuda", dtype=dtype, requires_grad=True)
    r = torch.randn(R, H, device="cuda", dtype=dtype, requires_grad=True)
    xb = torch.randn(H, device="cuda", dtype=torch.float32, requires_grad=True)
    w = (torch.rand(H, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(H, device="cuda", requires_grad=True)
    y = FU.bias_dropout_residual_layer_norm(x, r, xb, w, b, 0.0, True, 1e-5)
    gy = torch.randn_like(y)
    y.backward(gy)
    got = [t.grad.float().clone() for t in (x, r, xb, w, b)]
    xs = [t.detach().float().requires_grad_(True) for t in (x, r, xb, w, b)]
    yr = TF.layer_norm(xs[1] + (xs[0] + xs[2]), (H,), xs[3], xs[4], 1e-5)
    yr.backward(gy.float())
    tol = 3e-2 if dtype == torch.bfloat16 else 1e-4
    torch.testing.assert_close(y.float(), yr, atol=tol, rtol=tol)
    for g, t in zip(got, xs):
        torch.testing.assert_close(g, t.grad, atol=tol * 8, rtol=tol)
    # p > 0: x = 1, no bias, residual 0 -> hs = mask / (1 - p); the backward regenerates that mask
    p = 0.25
    x1 = torch.ones(R, H, device="cuda", dtype=dtype, requires_grad=True)
    r0 = torch.zeros(R, H, device="cuda", dtype=dtype, requires_grad=True)
    y1 = FU.bias_dropout_residual_layer_norm(x1, r0, None, w.detach(), b.detach(), p, True, 1e-5)
    g1 = torch.randn_like(y1)
    y1.backward(g1)
    keep = x1.grad != 0
    frac = keep.float().mean().item()
    assert abs(frac - (1 - p)) < 0.01
    torch.testing.assert_close(x1.grad.float(), r0.grad.float() * keep / (1 - p), atol=1e-2, rtol=1e-2)
    hs = keep.float() / (1 - p)
    torch.testing.assert_close(y1.float(), TF.layer_norm(hs, (H,), w.detach(), b.detach(), 1e-5), atol=5e-2, rtol=3e-2)



def test_resnet_residual_grad_route(monkeypatch):
    """identity bottleneck: the fused BN-add-ReLU hands its residual gradient to conv1, whose dgrad
    epilogue adds it (conv_gemm.res_route_begin); gradients equal the unrouted autograd sum"""
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import conv_gemm
    from paddle_hackathon_amd.vision.models.resnet import BottleneckBlock
    paddle.set_device("gpu:0")
    seen = []
    orig = conv_gemm.conv256_dgrad

    def spy(*a, **k):
        seen.append(k.get("addend") is not None)
        return orig(*a, **k)
    monkeypatch.setattr(conv_gemm, "conv256_dgrad", spy)
    results = []
    for route in ("1", "0"):
        monkeypatch.setenv("PHA_RES_ROUTE", route)
        seen.clear()
        paddle.seed(5)
        blk = BottleneckBlock(64, 16, data_format="NHWC")
        blk = paddle.amp.decorate(blk, level="O2", dtype="bfloat16")
        blk.train()
        g = torch.Generator("cuda").manual_seed(9)
        xt = torch.randn(4, 14, 14, 64, device="cuda", generator=g).bfloat16().requires_grad_(True)
        x = paddle.Tensor(xt)
        with paddle.amp.auto_cast(level="O2", dtype="bfloat16"):
            y = blk(x)
        (y.astype("float32") ** 2).mean().backward()
        results.append([xt.grad.float().clone()] + [p._t.grad.float().clone() for p in blk.parameters()
                                                     if p._t.grad is not None])
        if route == "1":
            assert any(seen), "conv1's dgrad did not receive the residual gradient"
        else:
            assert not any(seen)
    for a, b in zip(*results):
        assert (a - b).abs().max() <= 2e-2 * b.abs().max() + 1e-6


@pytest.mark.parametrize("stride", [1, 2])
def test_resnet_shortcut_grad_route(monkeypatch, stride):
    """downsample bottleneck: the shortcut conv's dx is handed to conv1, whose dgrad epilogue adds
    it (no autograd add of the two gradients of the block input); gradients equal the unrouted sum"""
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd import nn
    from paddle_hackathon_amd.ops import conv_gemm
    from paddle_hackathon_amd.vision.models.resnet import BottleneckBlock
    paddle.set_device("gpu:0")
    seen = []
    orig = conv_gemm.conv256_dgrad

    def spy(*a, **k):
        seen.append(k.get("addend") is not None)
        return orig(*a, **k)
    monkeypatch.setattr(conv_gemm, "conv256_dgrad", spy)
    results = []
    for route in ("1", "0"):
        monkeypatch.setenv("PHA_RES_ROUTE", route)
        seen.clear()
        paddle.seed(6)
        ds = nn.Sequential(nn.Conv2D(64, 128, 1, stride=stride, bias_attr=False, data_format="NHWC"),
                           nn.BatchNorm2D(128, data_format="NHWC"))
        blk = BottleneckBlock(64, 32, stride=stride, downsample=ds, data_format="NHWC")
        blk = paddle.amp.decorate(blk, level="O2", dtype="bfloat16")
        blk.train()
        g = torch.Generator("cuda").manual_seed(10)
        xt = torch.randn(4, 14, 14, 64, device="cuda", generator=g).bfloat16().requires_grad_(True)
        x = paddle.Tensor(xt)
        with paddle.amp.auto_cast(level="O2", dtype="bfloat16"):
            y = blk(x)
        (y.astype("float32") ** 2).mean().backward()
        results.append([xt.grad.float().clone()] + [p._t.grad.float().clone() for p in blk.parameters()
                                                     if p._t.grad is not None])
        if route == "1":
            assert any(seen), "conv1's dgrad did not receive the shortcut conv's gradient"
        else:
            assert not any(seen)
    for a, b in zip(*results):
        assert (a - b).abs().max() <= 2e-2 * b.abs().max() + 1e-6


def test_conv_dgrad_addend():
    """the conv epilogue addend: dgrad(dy) + r in one launch equals dgrad(dy) + r"""
    from paddle_hackathon_amd.ops import conv_gemm
    g = torch.Generator("cuda").manual_seed(1)
    dy = torch.randn(2, 9, 9, 32, device="cuda", generator=g).bfloat16()
    w = torch.randn(32, 24, 1, 1, device="cuda", generator=g).bfloat16()
    r = torch.randn(2, 9, 9, 24, device="cuda", generator=g).bfloat16()
    base = conv_gemm.conv256_dgrad(dy, w, (2, 9, 9, 24), (1, 1), (0, 0), (1, 1))
    fused = conv_gemm.conv256_dgrad(dy, w, (2, 9, 9, 24), (1, 1), (0, 0), (1, 1), addend=r)
    ref = base.float() + r.float()
    # both sides round to bf16 (the epilogue after the add): within one bf16 ulp of the largest value
    assert (fused.float() - ref).abs().max() <= 8e-3 * ref.abs().max()


def test_flash_attn_nonpositive_scale_and_ragged():
    """a negative softmax scale takes the forward without the folded-scale max (v1) and still
    matches the fp32 reference; ragged S / Sk (clamped prefetch rows) match too"""
    from paddle_hackathon_amd.ops import hip
    g = torch.Generator("cuda").manual_seed(3)
    for (S, Sk, scale, causal) in ((200, 200, -0.05, False), (130, 70, None, False), (77, 77, None, True)):
        q = torch.randn(2, S, 4, 128, device="cuda", generator=g).bfloat16().requires_grad_(True)
        k = torch.randn(2, Sk, 4, 128, device="cuda", generator=g).bfloat16().requires_grad_(True)
        v = torch.randn(2, Sk, 4, 128, device="cuda", generator=g).bfloat16().requires_grad_(True)
        o = hip.FlashAttention.apply(q, k, v, causal, scale)
        do = torch.randn_like(o)
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
        # plain fp32 attention as the oracle (torch SDPA's fp32 backward returned NaN here)
        qr, kr, vr = (t.detach().float().transpose(1, 2).requires_grad_(True) for t in (q, k, v))
        sc = scale if scale is not None else 128 ** -0.5
        att = (qr @ kr.transpose(-1, -2)) * sc
        if causal:
            att = att.masked_fill(torch.ones(S, Sk, device="cuda", dtype=torch.bool).triu(1), float("-inf"))
        orf = att.softmax(-1) @ vr
        gr = torch.autograd.grad(orf, (qr, kr, vr), do.float().transpose(1, 2))
        assert (o.float() - orf.transpose(1, 2)).abs().max() < 3e-2
        for a, r in zip((dq, dk, dv), gr):
            r = r.transpose(1, 2)
            assert (a.float() - r).abs().max() <= 3e-2 * max(1.0, r.abs().max().item())


def _train_steps(model, loss_fn, opt, steps=2):
    import paddle_hackathon_amd as paddle
    for _ in range(steps):
        with paddle.amp.auto_cast(level="O2", dtype="bfloat16"):
            loss = loss_fn(model)
        loss.backward()
        opt.step()
        opt.clear_grad(set_to_zero=False)
    torch.cuda.synchronize()
    return float(loss.item())


@pytest.mark.parametrize("M,N,K", [(4, 30522, 128), (30522, 128, 4), (8, 1000, 2048), (2048, 1000, 8),
                                   (100, 72, 200)])
def test_gemm_tail_padding(M, N, K, monkeypatch):
    """odd tails (vocab 30522, 4 masked tokens, batch 8) run on the own kernels through the
    zero-padded entry points, matching an fp32 reference in every layout"""
    from paddle_hackathon_amd.ops import gemm as G, fallback
    monkeypatch.setenv("PHA_GEMM_IMPL", "own")
    fallback.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    bt = torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    ref = a.float() @ bt.float().t()
    outs = {"nt": G.mm_nt(a, bt), "nt_bias": G.mm_nt_bias(a, bt, bias), "nn": G.mm_nn(a, bt.t().contiguous()),
            "tn": G.mm_tn(a.t().contiguous(), bt.t().contiguous())}
    torch.cuda.synchronize()
    assert fallback.total() == 0, fallback.counts()
    for k, o in outs.items():
        r = ref + bias if k == "nt_bias" else ref
        assert o.shape == (M, N), (k, o.shape)
        err = (o.float() - r).abs().max().item()
        assert err <= 2e-2 * max(1.0, r.abs().max().item()), (k, err)


@pytest.mark.parametrize("impl", ["auto", "own"])
def test_headline_paths_have_no_fallbacks(impl, monkeypatch):
    """GPT (fleet bench model), BERT (vocab 30522, not a multiple of 8) and ResNet-50 (NHWC)
    training steps record no hot-path fallback (ops/fallback.py): every matmul / conv /
    attention / embedding ran on the own kernels or — under the "auto" GEMM policy — on the
    library kernels chosen for the NT layout by measurement, never as an unsupported-shape escape.
    Library products are counted apart (fallback.library_counts): none under PHA_GEMM_IMPL=own, and
    under auto only the planned NT matmuls."""
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import fallback
    from paddle_hackathon_amd.models import gpt_config, GPTForPretraining, bert_config, BertForPretraining, \
        BertPretrainingCriterion
    from paddle_hackathon_amd.vision.models import resnet50
    monkeypatch.setenv("PHA_GEMM_IMPL", impl)
    monkeypatch.setenv("PHA_FALLBACK_LOG", "1")
    paddle.set_device("gpu")
    paddle.seed(0)
    results, libs = {}, {}

    fallback.reset()
    cfg = gpt_config("gpt-tiny", hidden_size=256, num_heads=4, ffn_hidden_size=1024, vocab_size=1024,
                     max_position_embeddings=256)
    gpt = paddle.amp.decorate(GPTForPretraining(cfg), level="O2", dtype="bfloat16")
    opt = paddle.optimizer.AdamW(learning_rate=1e-4, parameters=gpt.parameters(), multi_precision=True)
    ids = paddle.to_tensor(torch.randint(0, 1024, (2, 256), device="cuda"))
    _train_steps(gpt, lambda m: m(ids, ids), opt)
    results["gpt"] = fallback.counts()
    libs["gpt"] = fallback.library_counts()

    fallback.reset()
    bcfg = bert_config("bert-tiny", vocab_size=30522, hidden_size=128, num_heads=2, intermediate_size=512,
                       max_position_embeddings=128)
    bert = paddle.amp.decorate(BertForPretraining(bcfg), level="O2", dtype="bfloat16")
    crit = BertPretrainingCriterion(bcfg.vocab_size)
    bopt = paddle.optimizer.AdamW(learning_rate=1e-4, parameters=bert.parameters(), multi_precision=True)
    bids = paddle.to_tensor(torch.randint(0, 30522, (2, 128), device="cuda"))
    tt = paddle.to_tensor(torch.zeros(2, 128, dtype=torch.long, device="cuda"))
    mpos = paddle.to_tensor(torch.tensor([3, 7, 131, 140], device="cuda"))
    mlab = paddle.to_tensor(torch.randint(0, 30522, (4,), device="cuda"))
    nlab = paddle.to_tensor(torch.randint(0, 2, (2,), device="cuda"))

    def bert_loss(m):
        mlm, nsp = m(bids, tt, masked_positions=mpos)
        return crit(mlm, nsp, mlab, nlab)
    _train_steps(bert, bert_loss, bopt)
    results["bert"] = fallback.counts()
    libs["bert"] = fallback.library_counts()

    fallback.reset()
    rn = paddle.amp.decorate(resnet50(data_format="NHWC"), level="O2", dtype="bfloat16")
    ropt = paddle.optimizer.Momentum(learning_rate=0.1, momentum=0.9, parameters=rn.parameters(),
                                     multi_precision=True)
    x = paddle.to_tensor(torch.randn(8, 64, 64, 3, device="cuda").to(torch.bfloat16))
    y = paddle.to_tensor(torch.randint(0, 1000, (8,), device="cuda"))
    _train_steps(rn, lambda m: paddle.nn.functional.cross_entropy(m(x), y), ropt)
    results["resnet50"] = fallback.counts()
    libs["resnet50"] = fallback.library_counts()
    assert all(not v for v in results.values()), results
    if impl == "own":
        assert all(not v for v in libs.values()), libs
    else:
        # by policy the NT forward / dX products (GPT / BERT projections, ResNet's fc head) stay on
        # hipBLASLt under auto; nothing else may reach a library
        assert all(set(v) <= {"matmul"} for v in libs.values()), libs


@pytest.mark.parametrize("M,N,K", [(512, 1024, 256), (264, 520, 128), (4096, 8192, 2048)])
def test_gemm4p_gelu_epilogue(M, N, K):
    """gemm4p EPI_GELU (the MLP fc1 forward): act = gelu_tanh(x W^T + b) and the pre-activation
    x W^T from one epilogue, against fp32"""
    from paddle_hackathon_amd.ops import gemm as G
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand(M, K, device="cuda", generator=g) * 2 - 1).bfloat16()
    wt = (torch.rand(N, K, device="cuda", generator=g) * 2 - 1).bfloat16()
    b = torch.randn(N, device="cuda", generator=g).bfloat16()
    act, pre = G.mm_nt_bias_gelu(x, wt, b)
    ref_pre = x.float() @ wt.float().t()
    ref_act = TF.gelu(ref_pre + b.float(), approximate="tanh")
    for got, ref, what in ((pre, ref_pre, "pre"), (act, ref_act, "act")):
        err = ((got.float() - ref).abs().max() / ref.abs().max()).item()
        assert err < 1e-2, (what, err)


@pytest.mark.parametrize("layout", ["nt", "nt_bias", "nt_gelu", "tn", "tn_split", "nn",
                                    # the fp16 builds of the NT / NN defaults (the TN ones: test_tn_colsum_gpu.py)
                                    "nt_fp16", "nt_bias_fp16", "nt_gelu_fp16", "nt_daux_fp16", "nt_adeep_fp16", "nn_fp16"])
@pytest.mark.parametrize("M,N,K", [(264, 520, 128), (1032, 2056, 512), (2048, 1024, 1024), (296, 8, 64)])
def test_gemm4p_early_schedule_bitwise(layout, M, N, K):
    """the early-release main loop (EPI_EARLY) changes only when operands are staged and waited for:
    outputs equal the default schedule's bit for bit (ragged tiles, bias, GELU aux, split-K, NN)"""
    from paddle_hackathon_amd.ops import gemm as G
    torch.manual_seed(5)
    dt = torch.float16 if layout.endswith("_fp16") else torch.bfloat16
    layout = layout[:-5] if layout.endswith("_fp16") else layout
    r = lambda *s: (torch.rand(*s, device="cuda") * 2 - 1).to(dt)   # noqa: E731
    if layout.startswith("nt"):
        if layout == "nt_adeep":   # 3 A + 2 B slots: the default from K = 4096 on, taken from K = 256 on
            K = max(K, 256)
        a, bt, bias = r(M, K), r(N, K), torch.randn(N, device="cuda")
        if layout in ("nt_gelu", "nt_daux"):   # the aux: the pre-activation, or the GELU derivative
            dv = layout == "nt_daux"
            pre0, pre1 = (torch.empty(M, N, dtype=dt, device="cuda") for _ in range(2))
            c0 = G.gemm_p(a, bt, bias=bias, gelu_aux=pre0, gelu_deriv=dv)
            c1 = G.gemm_p(a, bt, bias=bias, gelu_aux=pre1, gelu_deriv=dv, epi_extra=G.EPI_EARLY)
            assert torch.equal(pre0, pre1)
            # (both launches take the default schedule: the aux against fp32 is the check of its stores)
            ref_aux = a.float() @ bt.float().t()
            if dv:
                x = (ref_aux + bias).requires_grad_(True)
                ref_aux, = torch.autograd.grad(torch.nn.functional.gelu(x, approximate="tanh").sum(), x)
            assert (pre1.float() - ref_aux).abs().max().item() <= 2e-2 * max(1.0, ref_aux.abs().max().item())
        elif layout == "nt_adeep":
            c0 = G.gemm_p(a, bt)
            c1 = G.gemm_p(a, bt, epi_extra=G.EPI_EARLY | G.EPI_ADEEP)
        else:
            b = bias if layout == "nt_bias" else None
            c0 = G.gemm_p(a, bt, bias=b)
            c1 = G.gemm_p(a, bt, bias=b, epi_extra=G.EPI_EARLY)
        ref = a.float() @ bt.float().t() + (bias if layout not in ("nt", "nt_adeep") else 0)
        if layout in ("nt_gelu", "nt_daux"):
            ref = torch.nn.functional.gelu(ref, approximate="tanh")
    elif layout.startswith("tn"):
        if K < 256 and layout == "tn_split":
            pytest.skip("split-K needs >= 4 K-tiles per slice")
        a, b = r(K, M), r(K, N)
        sp = 2 if layout == "tn_split" else 1
        c0 = G.gemm_p(a, b, True, True, splits=sp)
        c1 = G.gemm_p(a, b, True, True, splits=sp, epi_extra=G.EPI_EARLY)
        ref = a.float().t() @ b.float()
    else:
        a, b = r(M, K), r(K, N)
        c0 = G.nn_p(a, b)
        c1 = G.nn_p(a, b, epi_extra=G.EPI_EARLY)
        ref = a.float() @ b.float()
    assert torch.equal(c0, c1), (c0.float() - c1.float()).abs().max().item()
    assert (c1.float() - ref).abs().max().item() <= 2e-2 * max(1.0, ref.abs().max().item())


def test_weight_t_batched_refresh_matches_transpose():
    """weight_t: after an in-place update of several weights, the first stale lookup refreshes all
    cached [out][in] copies in one batched transpose (in place), each equal to w.t()"""
    import paddle_hackathon_amd.ops.conv_gemm as CG
    g = torch.Generator(device="cuda").manual_seed(3)
    shapes = [(768, 2304), (768, 768), (3072, 768), (136, 3072), (64, 8)]
    ws = [torch.randn(*s, device="cuda", generator=g).bfloat16() for s in shapes]
    first = [CG.weight_t(w) for w in ws]
    for w, t in zip(ws, first):
        assert torch.equal(t, w.t())
    with torch.no_grad():
        for w in ws:
            w.mul_(-0.5).add_(0.25)   # version bump, as an optimizer step
    again = CG.weight_t(ws[2])        # refreshes every stale copy
    assert again.data_ptr() == first[2].data_ptr()
    for w in ws:
        t = CG.weight_t(w)
        assert torch.equal(t, w.t())
