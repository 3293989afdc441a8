"""The int8 KV cache on the CPU (fp32 ``gpt-tiny``, no kernel): the quantisation rule, fused_multi_transformer
with ``cache_kv_scales`` and ``generate(cache_dtype="int8")``. The decode-stage reference is the same step on a
float cache that holds the dequantised rows, the new one included, appending at the next position with that
position masked out: it attends over what the int8 step attends over, up to fp32 summation order."""
import pytest
import torch

from paddle_hackathon_amd.incubate.nn import functional as FF
from paddle_hackathon_amd.models import GPTGenerator
from paddle_hackathon_amd.ops import hip
from test_weight_only_cpu import tiny  # noqa: F401  (fixture: fp32 gpt-tiny, E 64, 4 heads of D 16, 2 layers)


def test_quantise_rule_against_float64():
    x = torch.randn(5, 7, 32, generator=torch.Generator().manual_seed(0)) * torch.logspace(-3, 2, 7)[:, None]
    x[1, 2] = 0                                                    # a zero row: scale 1, zeros
    x[0, 0, :4] = torch.tensor([2.5, -3.5, 0.5, 127.0])            # scale exactly 1 here: ties go to even
    x[0, 0, 4:] = x[0, 0, 4:].clamp(-100, 100)
    q, s = hip.kv_cache_quantize(x)
    assert q.dtype == torch.int8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:-1]
    amax = x.double().abs().amax(-1)
    want_s = torch.where(amax > 0, (amax / 127).float(), torch.ones(()))               # one rounding, as fp32 division
    assert torch.equal(s, want_s) and float(s[1, 2]) == 1.0 and not q[1, 2].any()
    assert q[0, 0, :4].tolist() == [2, -4, 0, 127]
    ratio = (x.double() / s.double()[..., None]).float().double()                      # the fp32 quotient
    assert torch.equal(q.double(), torch.round(ratio).clamp(-127, 127))
    hit = x.abs() == x.abs().amax(-1, keepdim=True)
    assert bool((q[hit & (x != 0)].abs() == 127).all())
    assert torch.equal(hip.kv_cache_dequantize(q, s), q.float() * s[..., None])


def _layer(x, w, caches, scales=None, **kw):
    with torch.no_grad():
        return FF.fused_multi_transformer(x, *w, cache_kvs=caches, cache_kv_scales=scales, trans_qkvw=False,
                                          activation="gelu_tanh", **kw)[0]._t


@pytest.mark.parametrize("form", ["scalar", "rows", "beam"])
def test_layers_with_int8_caches_equal_the_dequantised_float_call(tiny, form):
    cfg, B, S, L = tiny.cfg, 4, 5, 9
    H, D, n = cfg.num_heads, cfg.head_dim, cfg.num_layers
    w = GPTGenerator(tiny)._layer_weights()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S + 1, cfg.hidden_size, generator=g)
    c8 = [torch.zeros(2, B, H, L, D, dtype=torch.int8) for _ in range(n)]
    sc = [torch.full((2, B, H, L), float("nan")) for _ in range(n)]
    cf = [torch.zeros(2, B, H, L, D) for _ in range(n)]
    # context stage: the same output, and the cache holds the quantised keys and values
    assert torch.equal(_layer(x[:, :S], w, c8, sc), _layer(x[:, :S], w, cf))
    for a, s, f in zip(c8, sc, cf):
        q, qs = hip.kv_cache_quantize(f[:, :, :, :S])
        assert torch.equal(a[:, :, :, :S], q) and torch.equal(s[:, :, :, :S], qs) and not a[:, :, :, S:].any()
    # decode stage
    steps = [S] * B if form != "rows" else [S, S - 2, 1, S - 1]
    kw, ref_kw = {}, {}
    if form == "scalar":
        kw["time_step"], ref_kw["time_step"] = S, S + 1
    else:
        kw["time_step"] = torch.tensor(steps, dtype=torch.int32)
        ref_kw["time_step"] = kw["time_step"] + 1
    if form == "beam":
        ind = torch.randint(0, 2, (B, L), generator=g).to(torch.int32)
        kw.update(cache_indirection=ind, beam_size=2)
        ref_ind = ind.clone()
        ref_ind[:, S] = torch.arange(B, dtype=torch.int32) % 2     # the reference reads the new row from the row's own cache
        ref_kw.update(cache_indirection=ref_ind, beam_size=2)
    out = _layer(x[:, S:], w, c8, sc, **kw)
    mask = torch.zeros(B, 1, 1, L)
    for b, ts in enumerate(steps):
        mask[b, ..., ts + 1] = float("-inf")
    ref_c = [hip.kv_cache_dequantize(a, torch.nan_to_num(s)) for a, s in zip(c8, sc)]   # after the step: row ts included
    ref = _layer(x[:, S:], w, ref_c, attn_mask=mask, **ref_kw)
    assert float((out - ref).abs().max() / ref.abs().max()) <= 64 * 2.0 ** -24         # summation order, fp32
    for a, s, f in zip(c8, sc, ref_c):                             # the reference appended the unquantised row at ts + 1
        for b, ts in enumerate(steps):
            q, qs = hip.kv_cache_quantize(f[:, b, :, ts + 1])
            assert torch.equal(a[:, b, :, ts], q) and torch.equal(s[:, b, :, ts], qs) and bool(s[:, b, :, S + 1:].isnan().all())


def test_generate_runs_with_int8_caches(tiny):
    gen = GPTGenerator(tiny)
    ids = torch.randint(0, tiny.cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(3))
    out, _ = gen.generate(ids, 4, cache_dtype="int8")
    assert tuple(out._t.shape) == (2, 4) and all(c.dtype == torch.int8 for c in gen.last_caches)
    assert len(gen.last_cache_scales) == len(gen.last_caches) and bool(gen.last_cache_scales[0][:, :, :, :9].gt(0).all())
    beams, _ = gen.generate(ids, 4, decode_strategy="beam_search", num_beams=2, cache_dtype="int8", weight_only="int8")
    assert tuple(beams._t.shape) == (2, 4) and gen.last_caches[0].dtype == torch.int8
    gen.generate(ids, 4)
    assert gen.last_cache_scales is None and gen.last_caches[0].dtype == torch.float32
    with pytest.raises(ValueError, match="cache_dtype"):
        gen.generate(ids, 4, cache_dtype="fp8")


def test_scale_argument_errors(tiny):
    cfg = tiny.cfg
    w = GPTGenerator(tiny)._layer_weights()
    x = torch.randn(2, 3, cfg.hidden_size)
    shape = (2, 2, cfg.num_heads, 8)
    c8 = [torch.zeros(*shape, cfg.head_dim, dtype=torch.int8) for _ in range(cfg.num_layers)]
    sc = [torch.zeros(shape) for _ in range(cfg.num_layers)]
    for caches, scales in ((c8, None), ([c.float() for c in c8], sc), (c8, sc[:1]), (c8, [s.double() for s in sc]),
                           (c8, [s[..., :-1] for s in sc]), (c8, [s.to("meta") for s in sc])):
        with pytest.raises(ValueError, match="cache"):
            _layer(x, w, caches, scales)
