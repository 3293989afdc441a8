"""Weight-only int8 on the CPU (nn/quant/weight_only.py and what uses it): the quantiser's contract, and
that every int8 path computes what the same call computes on the dequantised weights. fp32 throughout;
no kernel runs here, the int8 kernel has tests/test_skinny_gemm_w8_gpu.py."""
import pytest
import torch

from paddle_hackathon_amd.nn import quant
from weight_only_reference import dequantised_copy

@pytest.fixture
def tiny():
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import gpt_config, GPTForPretraining
    paddle.seed(0)
    model = GPTForPretraining(gpt_config("gpt-tiny", initializer_range=0.2))   # E 64, 4 heads, FFN 256, 2 layers
    model.eval()
    return model


def test_quantize_rounds_to_the_nearest_step_per_channel():
    w = torch.randn(48, 24, generator=torch.Generator().manual_seed(0)) * torch.logspace(-3, 1, 24)
    w[:, 5] = 0                                                   # a channel that is all zero: scale 1, q 0
    q, s = (t._t for t in quant.weight_quantize(w))
    assert q.dtype == torch.int8 and tuple(q.shape) == (24, 48) and s.dtype == torch.float32 and tuple(s.shape) == (24,)
    assert int(q.min()) >= -127 and int(q.max()) <= 127 and float(s[5]) == 1.0 and not q[5].any()
    back = quant.weight_dequantize(q, s, "float32")._t
    assert tuple(back.shape) == (48, 24) and bool(((w - back).abs() <= s / 2).all())


def test_weight_only_linear_matches_float64():
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn(2, 3, 64, generator=g), torch.randn(64, 40, generator=g), torch.randn(40, generator=g)
    q, s = (t._t for t in quant.weight_quantize(w))
    out = quant.weight_only_linear(x, q, b, s)._t
    ref = (x.double() @ q.double().t()) * s.double() + b.double()
    # fp32 sum of 64 terms against float64: sqrt(64) * 2^-24 of the largest element, with a factor 4 to spare
    assert tuple(out.shape) == (2, 3, 40) and float((out.double() - ref).abs().max() / ref.abs().max()) <= 32 * 2.0 ** -24
    with pytest.raises(ValueError, match="int8"):
        quant.weight_quantize(w, algo="weight_only_int4")
    with pytest.raises(ValueError, match="int8"):
        quant.weight_only_linear(x, q, b, s, weight_dtype="int4")


def test_fused_multi_transformer_with_scales_equals_the_dequantised_call(tiny):
    from paddle_hackathon_amd.incubate.nn import functional as FF
    from paddle_hackathon_amd.models import GPTGenerator
    cfg, B, S = tiny.cfg, 2, 5
    w8 = GPTGenerator(tiny)._layer_weights("int8")                 # int8 [N, K] lists, then the four scale lists
    deq = GPTGenerator(dequantised_copy(tiny))._layer_weights()    # the same weights dequantised, QKV [E, 3, H, D]
    x = torch.randn(B, S, cfg.hidden_size, generator=torch.Generator().manual_seed(2))

    def run(w, **kw):
        caches = [torch.zeros(2, B, cfg.num_heads, S + 2, cfg.head_dim) for _ in range(cfg.num_layers)]
        ctx, _ = FF.fused_multi_transformer(x, *w, cache_kvs=caches, **kw)
        step, _ = FF.fused_multi_transformer(ctx._t[:, -1:], *w, cache_kvs=caches, time_step=S, **kw)
        return torch.cat([ctx._t, step._t], 1)

    kw = dict(zip(("qkv_weight_scales", "linear_weight_scales", "ffn1_weight_scales", "ffn2_weight_scales"), w8[12:]))
    got, ref = run(w8[:12], **kw), run(deq, trans_qkvw=False)
    # the same fp32 arithmetic up to the order of the sums: 2 layers of products of at most 256 terms
    assert float((got - ref).abs().max() / ref.abs().max()) <= 64 * 2.0 ** -24
    with pytest.raises(ValueError, match="all four"):
        run(w8[:12], **dict(kw, ffn2_weight_scales=None))
    with pytest.raises(ValueError, match="trans_qkvw"):
        run(w8[:12], trans_qkvw=False, **kw)


@pytest.mark.parametrize("beams", [None, 2], ids=["greedy", "beam2"])
def test_generate_int8_equals_the_model_with_dequantised_weights(tiny, beams):
    ids = torch.randint(0, tiny.cfg.vocab_size, (2, 7), generator=torch.Generator().manual_seed(0))
    kw = {} if beams is None else dict(decode_strategy="beam_search", num_beams=beams)
    before = [p._t.clone() for p in tiny.parameters()]
    out, scores = tiny.generate(ids, 10, weight_only="int8", **kw)
    want, want_scores = dequantised_copy(tiny).generate(ids, 10, **kw)
    assert torch.equal(out._t, want._t) and float((scores._t - want_scores._t).abs().max()) <= 1e-5
    assert all(torch.equal(a, p._t) for a, p in zip(before, tiny.parameters()))   # the model is untouched
    with torch.no_grad():                                          # a parameter moves: the int8 copies follow it
        tiny.gpt.layers[0].mlp.linear1.weight._t.mul_(-1.5)
    new = tiny.generate(ids, 10, weight_only="int8", **kw)[0]._t
    assert torch.equal(new, dequantised_copy(tiny).generate(ids, 10, **kw)[0]._t) and not torch.equal(new, out._t)
    with pytest.raises(ValueError, match="int8"):
        tiny.generate(ids, 2, weight_only="int4")
