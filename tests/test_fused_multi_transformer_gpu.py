"""The decode stage of incubate.nn.functional.fused_multi_transformer on the split-KV decode
kernels (bf16): the kernel path is taken, its outputs are as close to an fp32 CPU run of the same
weights as the composite's (PHA_DECODE_ATTN=0) are, and one decode step with a device-side
``time_step`` is captured in a hipGraph and replayed for every token.

Numerics bound: e_new <= max(2 * e_old, 2^-8), with e the max-normalised error of a step's output
against the fp32 CPU reference; the composite is the yardstick and the factor 2 allows for a
different, not worse, rounding order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E, LAYERS, B, STEPS = 256, 2, 2, 6
DFF = 4 * E
NAMES = ("ln_scales", "ln_biases", "qkv_weights", "qkv_biases", "linear_weights", "linear_biases",
         "ffn_ln_scales", "ffn_ln_biases", "ffn1_weights", "ffn1_biases", "ffn2_weights", "ffn2_biases")


def _geom():
    from paddle_hackathon_amd.ops import hip
    C = hip.DECODE_ATTN_CHUNK
    return C + 24, C - 3   # max_seq, context length: the 6 steps cross the split seam at C


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _weights(heads, trans_qkvw, seed=0):
    """bf16-representable fp32 weights on the CPU"""
    g = torch.Generator().manual_seed(seed)
    D = E // heads

    def r(*shape, s=0.05):
        return (torch.randn(*shape, generator=g) * s).bfloat16().float()

    w = {k: [] for k in NAMES}
    for _ in range(LAYERS):
        w["ln_scales"].append((1.0 + r(E)).bfloat16().float())
        w["ln_biases"].append(r(E))
        w["qkv_weights"].append(r(3, heads, D, E) if trans_qkvw else r(E, 3, heads, D))
        w["qkv_biases"].append(r(3, heads, D))
        w["linear_weights"].append(r(E, E))
        w["linear_biases"].append(r(E))
        w["ffn_ln_scales"].append((1.0 + r(E)).bfloat16().float())
        w["ffn_ln_biases"].append(r(E))
        w["ffn1_weights"].append(r(E, DFF))
        w["ffn1_biases"].append(r(DFF))
        w["ffn2_weights"].append(r(DFF, E))
        w["ffn2_biases"].append(r(E))
    return w


def _to(w, **kw):
    return {k: [t.to(**kw) for t in v] for k, v in w.items()}


def _run(x, w, pre_ln, trans_qkvw, **kw):
    from paddle_hackathon_amd.incubate.nn import functional as FF
    out = FF.fused_multi_transformer(x, *[w[k] for k in NAMES], pre_layer_norm=pre_ln, trans_qkvw=trans_qkvw, **kw)
    out = out[0] if isinstance(out, tuple) else out
    return out._t if hasattr(out, "_t") else out


def _caches(heads, **kw):
    max_seq, _ = _geom()
    return [torch.zeros(2, B, heads, max_seq, E // heads, **kw) for _ in range(LAYERS)]


def _generate(x, w, heads, pre_ln, trans_qkvw, device_ts=False):
    """context stage + STEPS decode steps; returns (step outputs [B, STEPS, E], caches)"""
    _, ctx = _geom()
    caches = _caches(heads, device=x.device, dtype=x.dtype)
    outs = []
    with torch.no_grad():
        _run(x[:, :ctx], w, pre_ln, trans_qkvw, cache_kvs=caches)
        ts = torch.tensor([ctx], dtype=torch.int32, device=x.device) if device_ts else None
        for j in range(STEPS):
            t = ctx + j
            outs.append(_run(x[:, t:t + 1], w, pre_ln, trans_qkvw, cache_kvs=caches,
                             time_step=ts if device_ts else t))
            if device_ts:
                ts.add_(1)
    return torch.cat(outs, 1), caches


@pytest.fixture
def count_decode_calls(monkeypatch):
    from paddle_hackathon_amd.ops import hip
    calls = []
    real = hip.decode_attention

    def wrapper(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(hip, "decode_attention", wrapper)
    return calls


@pytest.mark.parametrize("pre_ln,trans_qkvw", [(True, True), (False, False)], ids=["preln", "postln_nt"])
@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_decode_steps_use_the_kernel_and_match_fp32(heads, pre_ln, trans_qkvw, count_decode_calls, monkeypatch):
    _, ctx = _geom()
    w = _weights(heads, trans_qkvw, seed=heads)
    x = torch.randn(B, ctx + STEPS, E, generator=torch.Generator().manual_seed(9)).bfloat16().float()
    ref, _ = _generate(x, w, heads, pre_ln, trans_qkvw)                       # fp32, CPU
    wg, xg = _to(w, device="cuda", dtype=torch.bfloat16), x.cuda().bfloat16()
    new, _ = _generate(xg, wg, heads, pre_ln, trans_qkvw)
    assert len(count_decode_calls) == STEPS * LAYERS                          # the kernel path ran, every layer
    monkeypatch.setenv("PHA_DECODE_ATTN", "0")
    old, _ = _generate(xg, wg, heads, pre_ln, trans_qkvw)
    assert len(count_decode_calls) == STEPS * LAYERS                          # and the switch turns it off
    for j in range(STEPS):
        e_new, e_old = _rel(new[:, j], ref[:, j]), _rel(old[:, j], ref[:, j])
        print(f"D={E // heads} pre_ln={pre_ln} trans_qkvw={trans_qkvw} step {j}: e_new {e_new:.3e} e_old {e_old:.3e}")
        assert e_new <= max(2 * e_old, 2.0 ** -8)


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_decode_step_replays_from_one_captured_graph(heads, count_decode_calls):
    max_seq, ctx = _geom()
    w = _weights(heads, True, seed=10 + heads)
    x = torch.randn(B, ctx + STEPS, E, generator=torch.Generator().manual_seed(11)).bfloat16().float()
    ref, _ = _generate(x, w, heads, True, True)                               # fp32, CPU
    wg, xg = _to(w, device="cuda", dtype=torch.bfloat16), x.cuda().bfloat16()
    eager, eager_caches = _generate(xg, wg, heads, True, True, device_ts=True)
    assert len(count_decode_calls) == STEPS * LAYERS

    caches = _caches(heads, device="cuda", dtype=torch.bfloat16)
    static_x = torch.zeros(B, 1, E, device="cuda", dtype=torch.bfloat16)
    ts = torch.tensor([ctx], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        _run(xg[:, :ctx], wg, True, True, cache_kvs=caches)
        static_x.copy_(xg[:, ctx:ctx + 1])
        _run(static_x, wg, True, True, cache_kvs=caches, time_step=ts)        # warm-up step (rewritten by replay 0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = _run(static_x, wg, True, True, cache_kvs=caches, time_step=ts)
            ts.add_(1)
        ts.fill_(ctx)   # capture launches nothing: the first replay is step 0
        outs = []
        for j in range(STEPS):
            static_x.copy_(xg[:, ctx + j:ctx + j + 1])
            graph.replay()
            outs.append(static_out.clone())
    torch.cuda.synchronize()
    assert int(ts.item()) == ctx + STEPS
    replayed = torch.cat(outs, 1)
    for j in range(STEPS):
        e_graph, e_eager = _rel(replayed[:, j], ref[:, j]), _rel(eager[:, j], ref[:, j])
        print(f"D={E // heads} step {j}: e_graph {e_graph:.3e} e_eager {e_eager:.3e}")
        assert e_graph <= max(2 * e_eager, 2.0 ** -8)
    for c, ce in zip(caches, eager_caches):
        n = ctx + STEPS
        assert torch.all(c[:, :, :, n:] == 0)                                 # nothing written past the last step
        assert _rel(c[:, :, :, :n], ce[:, :, :, :n]) <= 2.0 ** -8
