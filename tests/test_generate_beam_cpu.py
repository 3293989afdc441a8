"""Beam search of cached generation (models/gpt_generate.py) on the CPU: fp32 ``gpt-tiny`` on the
composites, against a plain beam search written here from uncached full forwards and the float64
step reference of tests/beam_reference.py. fp32 cached and uncached logits differ by about 1e-6; every
comparison first asserts that the reference met no step whose decisive totals were closer than 1e-3.
Also: the beam-step composite on the step cases of tests/test_beam_step_gpu.py (whose seeds are
checked here without a GPU), and fused_multi_transformer with a cache-indirection table against the
same call on physically gathered caches."""
import pytest
import torch

import beam_reference as ref

PROMPT, NEW = 7, 8


@pytest.fixture(scope="module")
def tiny():
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import gpt_config, GPTForPretraining
    paddle.seed(0)
    cfg = gpt_config("gpt-tiny", initializer_range=0.2)
    model = GPTForPretraining(cfg)
    model.eval()
    # prompt seed 8: the reference's smallest margin is 6e-3 or more in every search below (seed 0: 4e-4 at K = 4)
    ids = torch.randint(0, cfg.vocab_size, (2, PROMPT), generator=torch.Generator().manual_seed(8))
    return model, ids


def _uncached(model, prompts, K, n_new, **kw):
    """the reference beam search over ``prompts`` (a list of 1-D token tensors, one per item)"""
    import paddle_hackathon_amd as paddle

    def logits_fn(hist):
        rows = []
        with torch.no_grad():
            for r, h in enumerate(hist):
                full = torch.cat([prompts[r // K], torch.tensor(h, dtype=torch.int64)])[None]
                rows.append(model(paddle.to_tensor(full.numpy()))._t[0, -1].float())
        return torch.stack(rows)
    return ref.beam_search(logits_fn, len(prompts), K, n_new, **kw)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_beam_search_equals_the_uncached_reference(tiny, K):
    model, ids = tiny
    want, want_scores, margin = _uncached(model, list(ids), K, NEW, nret=K)
    assert margin > ref.MARGIN, f"precondition: the reference's smallest margin is {margin}"
    out, scores = model.generate(ids, NEW, decode_strategy="beam_search", num_beams=K, num_return_sequences=K)
    out, scores = out._t, scores._t
    assert out.dtype == torch.int64 and tuple(out.shape) == (2 * K, NEW) and scores.dtype == torch.float32
    assert torch.equal(out, want)
    assert float((scores.double() - want_scores).abs().max()) <= 1e-4
    best = scores.sum(1).reshape(2, K)
    assert bool((best[:, :-1] >= best[:, 1:]).all())          # best beam first


@pytest.mark.parametrize("K", [2, 4])
def test_ragged_prompts_equal_the_uncached_reference(tiny, K):
    model, ids = tiny
    lens = [PROMPT, 4]
    want, want_scores, margin = _uncached(model, [ids[b, :lens[b]] for b in range(2)], K, NEW)
    assert margin > ref.MARGIN, f"precondition: the reference's smallest margin is {margin}"
    out, scores = model.generate(ids, NEW, decode_strategy="beam_search", num_beams=K, seq_lens=lens)
    assert torch.equal(out._t, want)
    assert float((scores._t.double() - want_scores).abs().max()) <= 1e-4
    mask = torch.zeros(2, PROMPT, dtype=torch.int64)
    for b in range(2):
        mask[b, :lens[b]] = 1
    again, _ = model.generate(ids, NEW, decode_strategy="beam_search", num_beams=K, attention_mask=mask)
    assert torch.equal(again._t, want)


def test_one_beam_is_greedy_search(tiny):
    model, ids = tiny
    g, gs = model.generate(ids, NEW)
    b, bs = model.generate(ids, NEW, decode_strategy="beam_search", num_beams=1)
    assert torch.equal(g._t, b._t)
    assert float((gs._t - bs._t).abs().max()) <= 1e-5


def test_eos_length_penalty_and_num_return_sequences(tiny):
    model, ids = tiny
    K = 4
    first, _ = model.generate(ids, NEW, decode_strategy="beam_search", num_beams=K)
    eos = int(first._t[0, 2])                                  # a token the best beam of item 0 emits at step 2
    for lp in (0.0, 1.0):
        want, want_scores, margin = _uncached(model, list(ids), K, NEW, eos=eos, pad=3, length_penalty=lp, nret=2)
        assert margin > ref.MARGIN
        out, scores = model.generate(ids, NEW, decode_strategy="beam_search", num_beams=K, num_return_sequences=2,
                                     eos_token_id=eos, pad_token_id=3, length_penalty=lp)
        out, scores = out._t, scores._t
        assert tuple(out.shape) == (4, NEW)
        assert torch.equal(out, want)
        assert float((scores.double() - want_scores).abs().max()) <= 1e-4
        for r in range(4):
            hit = (out[r] == eos).nonzero()
            if len(hit):
                p = int(hit[0])
                assert bool((out[r, p + 1:] == 3).all()) and bool((scores[r, p + 1:] == 0).all())
    assert bool((want == 3).any()), "the chosen eos never ended a returned beam: the padding went untested"


def test_argument_errors(tiny):
    model, ids = tiny
    bs = dict(decode_strategy="beam_search")
    with pytest.raises(ValueError, match="num_beams"):            # beam search has no default width
        model.generate(ids, 2, **bs)
    for kw in (dict(num_beams=0, **bs), dict(num_beams=-2, **bs), dict(num_beams=2.0, **bs),
               dict(num_beams=2, num_return_sequences=3, **bs), dict(num_beams=2, num_return_sequences=0, **bs),
               dict(num_beams=2, temperature=0.7, **bs), dict(num_beams=2, top_k=5, **bs),
               dict(num_beams=2, top_p=0.9, **bs), dict(num_beams=2), dict(num_beams=2, decode_strategy="sampling"),
               dict(num_return_sequences=2), dict(decode_strategy="beam")):
        with pytest.raises(ValueError):
            model.generate(ids, 2, **kw)


# ------------------------------------------------------------------------------ the step composite
STEP_SHAPES = [(4, 1), (8, 2), (8, 4), (16, 4), (16, 16)]
STEP_CASES = [(kind, dt, V, R, K) for (R, K) in STEP_SHAPES for V in (519, 520) for dt in ("bf16", "fp16")
              for kind in ref.KINDS if K >= 2 or kind not in ("few_finite", "cross_tie")]


def test_step_composite_matches_the_reference_on_every_gpu_case():
    """the cases (and seeds) of tests/test_beam_step_gpu.py: their margins, and the composite in fp32"""
    from paddle_hackathon_amd.ops import hip
    dts = {"bf16": torch.bfloat16, "fp16": torch.float16}
    big = [("some_finished", "bf16", 50304, 8, 4), ("some_finished", "fp16", 50304, 8, 4)]
    for kind, dt, V, R, K in STEP_CASES + big:
        tag = f"{kind}-{dt}-V{V}-R{R}-K{K}"
        case = ref.make_case(kind, dts[dt], V, R, K, seed=ref.case_seed(kind, dt, V, R, K))
        want = ref.case_reference(case)
        if kind != "cross_tie":
            assert want["margin"] > ref.MARGIN, f"{tag}: margin {want['margin']}"
        c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
        assert not hip.beam_search_step_supported(c["logits"].float(), c["cum"], c["finished"], c["lengths"], K,
                                                  c["table"], c["ts"])
        tok, parent, lp = hip.beam_search_step(c["logits"].float(), c["cum"], c["finished"], c["lengths"], case["eos"],
                                               K, c["table"], c["ts"])
        assert torch.equal(tok, want["tok"]) and torch.equal(parent, want["parent"]), tag
        assert torch.equal(c["finished"], want["finished"]) and torch.equal(c["lengths"], want["lengths"]), tag
        assert torch.equal(c["table"], want["table"]), tag
        for have, exp in ((c["cum"], want["cum"]), (lp, want["logprob"])):
            inf = exp == float("-inf")
            assert torch.equal(have == float("-inf"), inf), tag
            assert float((have.double() - exp)[~inf].abs().max() if bool((~inf).any()) else 0.0) <= 1e-4, tag


def test_step_rejections_on_the_cpu():
    from paddle_hackathon_amd.ops import hip
    case = ref.make_case("random", torch.float32, 64, 4, 2, seed=3)
    a = [case["logits"], case["cum"], case["finished"], case["lengths"], 7, 2, case["table"], case["ts"]]
    for i, badv in ((1, case["cum"].double()), (2, case["finished"].bool()), (3, case["lengths"].long()), (5, 3),
                    (5, 0), (5, 65), (6, case["table"].long()), (6, case["table"][:2]), (7, ref.MAX_SEQ), (7, case["ts"][:3])):
        b = list(a)
        b[i] = badv
        with pytest.raises(ValueError):
            hip.beam_search_step(*b)


# ------------------------------------------------------------------------------ fused_multi_transformer
def _layer_weights(E, H, D, F, layers, g):
    def r(*s):
        return torch.randn(*s, generator=g) * 0.2
    return [[torch.ones(E) + r(E) for _ in range(layers)], [r(E) for _ in range(layers)],
            [r(3, H, D, E) for _ in range(layers)], [r(3, H, D) for _ in range(layers)],
            [r(H * D, E) for _ in range(layers)], [r(E) for _ in range(layers)],
            [torch.ones(E) + r(E) for _ in range(layers)], [r(E) for _ in range(layers)],
            [r(E, F) for _ in range(layers)], [r(F) for _ in range(layers)],
            [r(F, E) for _ in range(layers)], [r(E) for _ in range(layers)]]


@pytest.mark.parametrize("steps", [[9, 9, 9, 9], [9, 9, 4, 4]], ids=["uniform", "per_group"])
def test_fused_multi_transformer_with_a_table_equals_gathered_caches(steps):
    from paddle_hackathon_amd.incubate.nn import functional as FF
    import paddle_hackathon_amd as paddle
    B, K, H, D, E, F, L, S = 4, 2, 2, 16, 32, 64, 2, 12
    g = torch.Generator().manual_seed(11)
    w = _layer_weights(E, H, D, F, L, g)
    x = torch.randn(B, 1, E, generator=g)
    caches = [torch.randn(2, B, H, S, D, generator=g) for _ in range(L)]
    ind = torch.randint(0, K, (B, S), generator=g, dtype=torch.int32)
    ts = torch.tensor(steps, dtype=torch.int32)
    for b in range(B):
        ind[b, steps[b]:] = K + 1                                   # never followed
    # physically gathered caches: row b holds its own history; the per-row composite reads nothing above ts
    t = torch.arange(S)
    src = (torch.arange(B) // K * K)[:, None] + ind.long().clamp(0, K - 1)
    gathered = [c[:, src, :, t[None, :]].permute(2, 0, 3, 1, 4).contiguous() for c in caches]
    want, _ = FF.fused_multi_transformer(paddle.to_tensor(x.numpy()), *w, cache_kvs=gathered, time_step=ts)
    mine = [c.clone() for c in caches]
    got, _ = FF.fused_multi_transformer(paddle.to_tensor(x.numpy()), *w, cache_kvs=mine, time_step=ts,
                                        cache_indirection=ind, beam_size=K)
    assert float((got._t - want._t).abs().max()) <= 1e-5
    for c, c0, cg in zip(mine, caches, gathered):
        for b in range(B):                                          # the append went to the row's own cache row
            assert torch.equal(c[:, b, :, steps[b]], cg[:, b, :, steps[b]])
            c0[:, b, :, steps[b]] = c[:, b, :, steps[b]]
        assert torch.equal(c, c0)                                   # and nothing else moved
    if len(set(steps)) == 1:                                        # a scalar step is broadcast
        again = [c.clone() for c in caches]
        for b in range(B):
            for c, c2 in zip(again, caches):
                c[:, b, :, steps[b]] = torch.randn(2, H, D, generator=g)   # what the step overwrites
        got2, _ = FF.fused_multi_transformer(paddle.to_tensor(x.numpy()), *w, cache_kvs=again, time_step=steps[0],
                                             cache_indirection=ind, beam_size=K)
        assert torch.equal(got2._t, got._t)
        assert all(torch.equal(a, m) for a, m in zip(again, mine))
    with pytest.raises(ValueError):
        FF.fused_multi_transformer(paddle.to_tensor(x.numpy()), *w, cache_kvs=mine, time_step=ts, beam_size=2)
    with pytest.raises(ValueError):
        FF.fused_multi_transformer(paddle.to_tensor(x.numpy()), *w, cache_kvs=mine, time_step=ts,
                                   cache_indirection=ind, beam_size=3)
    with pytest.raises(ValueError):
        FF.fused_multi_transformer(paddle.to_tensor(x.numpy()), *w, cache_kvs=mine, time_step=ts,
                                   cache_indirection=ind.long(), beam_size=K)
    with pytest.raises(ValueError):                                 # the context stage takes no table
        FF.fused_multi_transformer(paddle.to_tensor(torch.randn(B, 3, E).numpy()), *w, cache_kvs=mine,
                                   cache_indirection=ind, beam_size=K)
