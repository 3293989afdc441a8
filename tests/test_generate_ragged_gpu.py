"""Generation from prompts of different lengths on the GPU in bf16: the models of
tests/test_generate_gpu.py (hidden 256, 2 layers, vocab 520; 2 heads with D = 128 and 4 heads with
D = 64), B = 3, prompt lengths (C - 3, C - 70, 1) with C = DECODE_ATTN_CHUNK and 6 new tokens, so
the longest row crosses a split seam of the decode attention while the others do not.

Numerics, per row: the fp32 CPU model runs uncached over the row's own prompt plus output. Every
generated token's fp32 logit must be within max(2 * e_old, 2^-8) * max|logit| of that position's
largest logit, e_old being the max-normalised logit error of the bf16 uncached forward over the same
ids against fp32 (the yardstick of tests/test_generate_gpu.py, measured here per row)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NEW, LAYERS, VOCAB = 3, 6, 2, 520

_models = {}


def _lens():
    from paddle_hackathon_amd.ops import hip
    C = hip.DECODE_ATTN_CHUNK
    return (C - 3, C - 70, 1)


def _pair(heads):
    """(bf16 GPU model, fp32 CPU model) with the same bf16-representable weights, and the padded prompts"""
    if heads in _models:
        return _models[heads]
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import gpt_config, GPTForPretraining
    P = max(_lens())
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


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_ragged_greedy_takes_the_kernels_and_matches_fp32_per_row(heads, monkeypatch):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import fallback, hip
    gpu, cpu, ids = _pair(heads)
    lens = _lens()
    steps = []
    real = hip.decode_attention

    def counted(qkv, qkv_bias, cache, time_step, *a, **k):
        steps.append(time_step.numel() if isinstance(time_step, torch.Tensor) else 0)
        return real(qkv, qkv_bias, cache, time_step, *a, **k)
    monkeypatch.setattr(hip, "decode_attention", counted)
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")           # a fallback anywhere in the step raises
    before = fallback.total()
    out, scores = gpu.generate(ids.cuda(), NEW, seq_lens=list(lens), use_graph=False)
    out, scores = out._t, scores._t
    monkeypatch.delenv("PHA_STRICT_NATIVE")
    assert fallback.total() == before
    assert tuple(out.shape) == (B, NEW) and out.dtype == torch.int64 and scores.dtype == torch.float32
    assert steps == [B] * (LAYERS * (NEW - 1))             # every decode step, every layer, a step per row
    for b, n in enumerate(lens):
        full = torch.cat([ids[b:b + 1, :n], out[b:b + 1].cpu()], 1)
        with torch.no_grad():
            ref = cpu(paddle.to_tensor(full.numpy()))._t.float()[0]
            paddle.set_device("gpu:0")
            try:
                old = gpu(paddle.to_tensor(full.cuda()))._t.float().cpu()[0]
            finally:
                paddle.set_device("cpu")
        e_old = ((old - ref).abs().max() / ref.abs().max()).item()
        tol = max(2 * e_old, 2.0 ** -8)
        lg = ref[n - 1:n - 1 + NEW]                                               # [NEW, V]
        short = (lg.max(-1).values - lg.gather(1, out[b].cpu()[:, None])[:, 0]) / lg.abs().max(-1).values
        print(f"D={256 // heads} row {b} (len {n}): generated tokens at most {short.max().item():.3e} below the "
              f"fp32 maximum (e_old {e_old:.3e}, bound {tol:.3e})")
        assert short.max().item() <= tol
        lp = torch.log_softmax(lg, -1).gather(1, out[b].cpu()[:, None])[:, 0]
        # a score is a logit minus the row's log-sum-exp: each within the logit bound, so twice that bound
        assert float((scores[b].cpu() - lp).abs().max()) <= 2 * tol * float(ref.abs().max())


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_ragged_graph_equals_eager_and_serves_other_lengths(heads):
    from paddle_hackathon_amd.models import GPTGenerator
    gpu, _, ids = _pair(heads)
    lens = list(_lens())
    gen = GPTGenerator(gpu)
    uniform, _ = gen.generate(ids.cuda(), NEW, use_graph=True)
    assert gen.captures == 1
    eager, eager_scores = gen.generate(ids.cuda(), NEW, seq_lens=lens, use_graph=False)
    assert gen.captures == 1
    graph, graph_scores = gen.generate(ids.cuda(), NEW, seq_lens=lens, use_graph=True)
    assert gen.captures == 2                                         # the first ragged call: exactly one capture
    assert torch.equal(eager._t, graph._t)                           # token for token
    assert float((eager_scores._t - graph_scores._t).abs().max()) <= 2.0 ** -8
    other = [lens[0], 5, lens[0] - 1]                                # other lengths, the same longest prompt
    a, _ = gen.generate(ids.cuda(), NEW, seq_lens=other)             # None: the kernel path everywhere -> graph
    assert gen.captures == 2                                         # lengths are data, not part of the key
    b, _ = gen.generate(ids.cuda(), NEW, seq_lens=other, use_graph=False)
    assert torch.equal(a._t, b._t)
    again, _ = gen.generate(ids.cuda(), NEW, seq_lens=lens)
    assert gen.captures == 2 and torch.equal(again._t, graph._t)
    u2, _ = gen.generate(ids.cuda(), NEW)                            # the uniform call's graph is not disturbed
    assert gen.captures == 2 and torch.equal(u2._t, uniform._t)
