"""The int8 KV cache through fused_multi_transformer and ``generate(cache_dtype="int8")`` on the GPU in bf16, with
the weights of tests/test_fused_multi_transformer_gpu.py and the model pair of tests/test_generate_gpu.py. Layer
bound: that file's, e_new <= max(2 * e_old, 2^-8), e the max-normalised error against the fp32 CPU run of the same
call (int8 caches there too), the composite (PHA_DECODE_ATTN=0) the yardstick."""
import pytest
import torch

from paddle_hackathon_amd.ops import fallback, hip
from test_fused_multi_transformer_gpu import B, E, LAYERS, _geom, _rel, _run, _to, _weights
from test_generate_gpu import NEW, _pair

pytestmark = pytest.mark.gpu


def _q8_caches(heads, device, rows=B):
    max_seq, _ = _geom()
    return ([torch.zeros(2, rows, heads, max_seq, E // heads, dtype=torch.int8, device=device) for _ in range(LAYERS)],
            [torch.zeros(2, rows, heads, max_seq, device=device) for _ in range(LAYERS)])


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_prefill_store_and_one_decode_step(heads, monkeypatch):
    _, ctx = _geom()
    w = _weights(heads, True, seed=heads)
    x = torch.randn(B, ctx + 1, E, generator=torch.Generator().manual_seed(9)).bfloat16().float()
    wg, xg = _to(w, device="cuda", dtype=torch.bfloat16), x.cuda().bfloat16()
    # prefill: the cache equals the torch quantisation of the context k / v, also through the strided beam view
    plain = [torch.zeros(2, B, heads, ctx, E // heads, dtype=torch.bfloat16, device="cuda") for _ in range(LAYERS)]
    (c8, sc), (c3, s3) = _q8_caches(heads, "cuda"), _q8_caches(heads, "cuda", 3 * B)
    with torch.no_grad():
        _run(xg[:, :ctx], wg, True, True, cache_kvs=plain)
        _run(xg[:, :ctx], wg, True, True, cache_kvs=c8, cache_kv_scales=sc)
        _run(xg[:, :ctx], wg, True, True, cache_kvs=[c[:, ::3] for c in c3], cache_kv_scales=[s[:, ::3] for s in s3])
    for p, a, s, a3, t3 in zip(plain, c8, sc, c3, s3):
        q, qs = hip.kv_cache_quantize(p)
        assert torch.equal(a[:, :, :, :ctx], q) and torch.equal(s[:, :, :, :ctx], qs) and not a[:, :, :, ctx:].any()
        assert torch.equal(a3[:, ::3], a) and torch.equal(t3[:, ::3], s) and not a3[:, 1::3].any() and not a3[:, 2::3].any()
    # one decode step on the kernel pair, on the composite and in fp32 on the CPU, from the same caches
    calls, real = [], hip.decode_attention
    monkeypatch.setattr(hip, "decode_attention", lambda *a, **k: calls.append(a[2].dtype) or real(*a, **k))
    ts = torch.tensor([ctx], dtype=torch.int32, device="cuda")
    (k8, ks), (o8, os_) = ([t.clone() for t in c8], [t.clone() for t in sc]), ([t.clone() for t in c8], [t.clone() for t in sc])
    r8, rs = [t.cpu() for t in c8], [t.cpu() for t in sc]
    with torch.no_grad():
        new = _run(xg[:, ctx:], wg, True, True, cache_kvs=k8, cache_kv_scales=ks, time_step=ts)
        assert calls == [torch.int8] * LAYERS
        monkeypatch.setenv("PHA_DECODE_ATTN", "0")
        old = _run(xg[:, ctx:], wg, True, True, cache_kvs=o8, cache_kv_scales=os_, time_step=ts)
        assert len(calls) == LAYERS
        ref = _run(x[:, ctx:], w, True, True, cache_kvs=r8, cache_kv_scales=rs, time_step=ctx)
    # the first layer sees the same input on both paths: what it appended is bitwise equal
    assert torch.equal(k8[0], o8[0]) and torch.equal(ks[0], os_[0]) and bool(ks[0][:, :, :, ctx].gt(0).all())
    e_new, e_old = _rel(new, ref), _rel(old, ref)
    print(f"D={E // heads}: e_new {e_new:.3e} e_old {e_old:.3e}")
    assert e_new <= max(2 * e_old, 2.0 ** -8)


def test_generate_stays_native_and_graph_equals_eager(monkeypatch):
    from paddle_hackathon_amd.models import GPTGenerator
    gpu, _, ids = _pair(2)
    gen = GPTGenerator(gpu)
    plain, _ = gen.generate(ids.cuda(), NEW, use_graph=False)
    calls, real = [], hip.decode_attention
    monkeypatch.setattr(hip, "decode_attention", lambda *a, **k: calls.append(a[2].dtype) or real(*a, **k))
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")              # a fallback anywhere raises
    before = fallback.total()
    eager, _ = gen.generate(ids.cuda(), NEW, use_graph=False, cache_dtype="int8")
    assert fallback.total() == before and calls == [torch.int8] * (LAYERS * (NEW - 1))
    assert gen.last_caches[0].dtype == torch.int8 and gen.last_cache_scales[0].dtype == torch.float32
    for kw in (dict(weight_only="int8"), dict(decode_strategy="beam_search", num_beams=2)):
        out, _ = gen.generate(ids.cuda(), NEW, use_graph=False, cache_dtype="int8", **kw)
        assert fallback.total() == before and tuple(out._t.shape) == tuple(eager._t.shape)
    monkeypatch.delenv("PHA_STRICT_NATIVE")
    assert gen.captures == 0
    graph, graph_scores = gen.generate(ids.cuda(), NEW, use_graph=True, cache_dtype="int8")
    assert gen.captures == 1 and torch.equal(eager._t, graph._t)            # token for token
    again, again_scores = gen.generate(ids.cuda(), NEW, cache_dtype="int8")
    assert gen.captures == 1 and torch.equal(again._t, graph._t) and torch.equal(again_scores._t, graph_scores._t)
    after, _ = gen.generate(ids.cuda(), NEW)                                # cache_dtype=None: a graph of its own
    assert gen.captures == 2 and torch.equal(after._t, plain._t)
