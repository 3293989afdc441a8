"""Cached generation (models/gpt_generate.py) on the GPU in bf16: hidden 256, 2 layers, vocab 520, with
2 heads (D = 128) and with 4 heads (D = 64); B = 2, prompt = DECODE_ATTN_CHUNK - 3 and 6 new tokens,
so the 5 decode steps cross a split seam of the decode attention.

Numerics: the fp32 CPU model runs once, uncached, over prompt + generated ids. At every step the
generated token's fp32 logit must be within max(2 * e_old, 2^-8) * max|logit| of that position's
largest logit, e_old being the max-normalised logit error of the existing bf16 uncached forward against
fp32: the project's own yardstick, measured here; 2^-8 is one bf16 ulp of the largest logit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NEW, LAYERS, VOCAB = 2, 6, 2, 520


def _prompt_len():
    from paddle_hackathon_amd.ops import hip
    return hip.DECODE_ATTN_CHUNK - 3


_models = {}


def _pair(heads):
    """(bf16 GPU model, fp32 CPU model) with the same bf16-representable weights, and the prompt"""
    if heads in _models:
        return _models[heads]
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import gpt_config, GPTForPretraining
    P = _prompt_len()
    cfg = dict(hidden_size=256, num_layers=LAYERS, num_heads=heads, ffn_hidden_size=1024, vocab_size=VOCAB,
               max_position_embeddings=P + 64)
    paddle.set_device("cpu")
    paddle.seed(heads)
    cpu = GPTForPretraining(gpt_config("gpt-tiny", **cfg))
    cpu.eval()
    with torch.no_grad():
        for p in cpu.parameters():
            p._t.copy_(p._t.bfloat16().float())
    paddle.set_device("gpu:0")
    try:
        gpu = paddle.amp.decorate(GPTForPretraining(gpt_config("gpt-tiny", **cfg)), level="O2", dtype="bfloat16")
        gpu.eval()
        with torch.no_grad():
            for (n1, p), (n2, q) in zip(gpu.named_parameters(), cpu.named_parameters()):
                assert n1 == n2
                p._t.copy_(q._t)
    finally:
        paddle.set_device("cpu")
    ids = torch.randint(0, VOCAB, (B, P), generator=torch.Generator().manual_seed(heads))
    _models[heads] = (gpu, cpu, ids)
    return _models[heads]


@pytest.fixture
def counters(monkeypatch):
    """call counts of the three kernels' wrappers, and the logits each sampling call saw"""
    from paddle_hackathon_amd.ops import hip
    seen = {"decode_attention": 0, "skinny_gemm": 0, "sample_logits": 0, "logits": []}

    def wrap(name):
        real = getattr(hip, name)

        def w(*a, **k):
            seen[name] += 1
            if name == "sample_logits" and not torch.cuda.is_current_stream_capturing():
                seen["logits"].append(a[0].detach().float().cpu())
            return real(*a, **k)
        monkeypatch.setattr(hip, name, w)
    for name in ("decode_attention", "skinny_gemm", "sample_logits"):
        wrap(name)
    return seen


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_greedy_takes_the_kernels_and_matches_fp32(heads, counters, monkeypatch):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import fallback
    gpu, cpu, ids = _pair(heads)
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")           # a fallback anywhere in the step raises
    before = fallback.total()
    out, scores = gpu.generate(ids.cuda(), NEW, use_graph=False)
    out, scores = out._t, scores._t
    monkeypatch.delenv("PHA_STRICT_NATIVE")
    assert fallback.total() == before
    assert out.is_cuda and tuple(out.shape) == (B, NEW) and out.dtype == torch.int64 and scores.dtype == torch.float32
    assert counters["decode_attention"] == LAYERS * (NEW - 1)      # every decode step, every layer
    assert counters["sample_logits"] == NEW                        # the prefill's token and one per step
    assert counters["skinny_gemm"] >= (NEW - 1) * (4 * LAYERS + 1)   # four products per layer and the LM head
    full = torch.cat([ids, out.cpu()], 1)
    P = ids.shape[1]
    with torch.no_grad():
        ref = cpu(paddle.to_tensor(full.numpy()))._t.float()
        paddle.set_device("gpu:0")
        try:
            old = gpu(paddle.to_tensor(full.cuda()))._t.float().cpu()
        finally:
            paddle.set_device("cpu")
    e_old = ((old - ref).abs().max() / ref.abs().max()).item()
    tol = max(2 * e_old, 2.0 ** -8)
    for j in range(NEW):
        lg = ref[:, P - 1 + j]
        short = (lg.max(-1).values - lg.gather(1, out[:, j:j + 1].cpu())[:, 0]) / lg.abs().max(-1).values
        print(f"D={256 // heads} step {j}: generated token is {short.max().item():.3e} below the fp32 maximum "
              f"(e_old {e_old:.3e}, bound {tol:.3e})")
        assert short.max().item() <= tol
    lp = torch.log_softmax(ref[:, P - 1:P - 1 + NEW], -1).gather(2, out.cpu()[:, :, None])[:, :, 0]
    # a score is a logit minus the row's log-sum-exp: each within the logit bound, so twice that bound
    assert float((scores.cpu() - lp).abs().max()) <= 2 * tol * float(ref.abs().max())


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_graph_equals_eager_and_is_reused(heads):
    from paddle_hackathon_amd.models import GPTGenerator
    gpu, _, ids = _pair(heads)
    P = ids.shape[1]
    gen = GPTGenerator(gpu)
    eager, eager_scores = gen.generate(ids.cuda(), NEW, use_graph=False)
    assert gen.captures == 0
    graph, graph_scores = gen.generate(ids.cuda(), NEW, use_graph=True)
    assert gen.captures == 1
    assert torch.equal(eager._t, graph._t)                           # token for token
    assert float((eager_scores._t - graph_scores._t).abs().max()) <= 2.0 ** -8
    again, again_scores = gen.generate(ids.cuda(), NEW)              # None: the kernel path everywhere -> graph
    assert gen.captures == 1                                         # the cached graph, no new capture
    assert torch.equal(again._t, graph._t) and torch.equal(again_scores._t, graph_scores._t)
    for c in gen.last_caches:
        assert tuple(c.shape) == (2, B, heads, P + NEW, 256 // heads)
        assert bool((c[:, :, :, P + NEW - 1:] == 0).all())            # nothing written past the last step
        assert bool((c[:, :, :, :P + NEW - 1].float().abs().amax(dim=(0, 1, 2, 4)) > 0).all())
    other = torch.randint(0, VOCAB, (B, P), generator=torch.Generator().manual_seed(99)).cuda()
    a, _ = gen.generate(other, NEW)                                  # same key, new prompt: replays, fresh result
    b, _ = gen.generate(other, NEW, use_graph=False)
    assert gen.captures == 1 and torch.equal(a._t, b._t)
    gen.clear()                                                      # graphs and their caches released
    c, _ = gen.generate(other, NEW)
    assert gen.captures == 2 and torch.equal(c._t, a._t)


def test_sampling_stays_inside_top_k_and_reproduces(counters):
    gpu, _, ids = _pair(2)
    kw = dict(decode_strategy="sampling", top_k=5, top_p=0.9, seed=1, use_graph=False)
    out, _ = gpu.generate(ids.cuda(), NEW, **kw)
    out = out._t.cpu()
    assert counters["sample_logits"] == NEW and len(counters["logits"]) == NEW
    for j, lg in enumerate(counters["logits"]):
        top5 = lg.topk(5, -1)
        for b in range(B):
            # inside the reference top-5 of the logits the step produced (ties at the 5th value count)
            assert float(lg[b, out[b, j]]) >= float(top5.values[b, -1])
    again, _ = gpu.generate(ids.cuda(), NEW, **kw)
    assert torch.equal(again._t.cpu(), out)
    g1, _ = gpu.generate(ids.cuda(), NEW, **dict(kw, use_graph=True))
    g2, _ = gpu.generate(ids.cuda(), NEW, **dict(kw, use_graph=True))
    assert torch.equal(g1._t, g2._t)
    assert bool((g1._t >= 0).all()) and bool((g1._t < VOCAB).all())


def test_eos_pads_in_graph_mode():
    gpu, _, ids = _pair(2)
    plain, _ = gpu.generate(ids.cuda(), NEW)
    eos = int(plain._t[0, 2])
    out, scores = gpu.generate(ids.cuda(), NEW, eos_token_id=eos, pad_token_id=1, use_graph=True)
    out = out._t.cpu()
    first = int((out[0] == eos).nonzero()[0])
    assert first <= 2 and bool((out[0, first + 1:] == 1).all()) and bool((scores._t[0, first + 1:] == 0).all())
    assert torch.equal(out[0, :first + 1], plain._t[0, :first + 1].cpu())
