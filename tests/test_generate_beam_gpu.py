"""Beam search of cached generation on the GPU in bf16, on the tiny models of tests/test_generate_gpu.py
(hidden 256, 2 layers, vocab 520; 2 heads with D = 128 and 4 heads with D = 64): B = 2 prompts of
DECODE_ATTN_CHUNK - 3 tokens, K = 4 beams and 6 new tokens, so the 5 decode steps cross a split seam
of the decode attention with a table that has been re-ordered several times.

What pins the cache-indirection table is the teacher-forced score: the fp32 CPU model runs uncached
over prompt + every returned beam, and the sum of its log probabilities must match the returned score
within n_steps * 2 * tol * max|logit|, tol = max(2 * e_old, 2^-8) measured as in
tests/test_generate_gpu.py. A beam that attended over another beam's history scores grossly off.
Every step's inputs are also replayed through the float64 step reference (tests/beam_reference.py):
tokens and parents must be reproduced exactly, and for the committed prompts no step's decisive totals
may be closer than 1e-3."""
import pytest
import torch

import beam_reference as ref
from test_generate_gpu import B, LAYERS, NEW, VOCAB, _pair

pytestmark = pytest.mark.gpu

K = 4
HEADS = pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
# prompt seeds per model for which every step of every search below keeps its decisive totals more
# than 1e-3 apart (bf16 logits are 2^-8 apart near 1, so margins come in such lumps; the models'
# own prompts of tests/test_generate_gpu.py leave 2e-4 at D = 64)
PROMPT_SEED = {2: 100, 4: 102}


def _models(heads):
    gpu, cpu, ids = _pair(heads)
    ids = torch.randint(0, VOCAB, tuple(ids.shape), generator=torch.Generator().manual_seed(PROMPT_SEED[heads]))
    return gpu, cpu, ids


@pytest.fixture
def rec(monkeypatch):
    """call counts of the wrappers, and what every eager beam step saw and returned"""
    from paddle_hackathon_amd.ops import hip
    seen = {"decode_attention": 0, "with_table": 0, "beam_search_step": 0, "sample_logits": 0, "steps": []}
    real_da, real_bs, real_sl = hip.decode_attention, hip.beam_search_step, hip.sample_logits

    def da(*a, **k):
        seen["decode_attention"] += 1
        seen["with_table"] += k.get("cache_indirection") is not None
        return real_da(*a, **k)

    def sl(*a, **k):
        seen["sample_logits"] += 1
        return real_sl(*a, **k)

    def bs(logits, cum, finished, lengths, eos, beams, table, ts):
        seen["beam_search_step"] += 1
        if torch.cuda.is_current_stream_capturing():
            return real_bs(logits, cum, finished, lengths, eos, beams, table, ts)
        before = dict(logits=logits.detach().cpu(), cum=cum.cpu(), finished=finished.cpu(), lengths=lengths.cpu(),
                      eos=eos, K=beams, table=table.cpu(), ts=ts.cpu() if isinstance(ts, torch.Tensor) else ts)
        out = real_bs(logits, cum, finished, lengths, eos, beams, table, ts)
        seen["steps"].append((before, [t.cpu() for t in out], dict(cum=cum.cpu(), finished=finished.cpu(),
                                                                  lengths=lengths.cpu(), table=table.cpu())))
        return out
    monkeypatch.setattr(hip, "decode_attention", da)
    monkeypatch.setattr(hip, "sample_logits", sl)
    monkeypatch.setattr(hip, "beam_search_step", bs)
    return seen


def _replay(steps):
    """every recorded step through the float64 reference; returns the smallest margin"""
    margin = float("inf")
    for i, (c, out, after) in enumerate(steps):
        want = ref.case_reference(c)
        margin = min(margin, want["margin"])
        print(f"step {i}: reference margin {want['margin']:.4f}")
        if want["margin"] > ref.MARGIN:
            assert torch.equal(out[0], want["tok"]), f"step {i}: tokens"
            assert torch.equal(out[1], want["parent"]), f"step {i}: parents"
            assert torch.equal(after["finished"], want["finished"]) and torch.equal(after["lengths"], want["lengths"])
            assert torch.equal(after["table"], want["table"]), f"step {i}: table"
            fin = want["cum"] > float("-inf")
            assert float((after["cum"].double() - want["cum"])[fin].abs().max()) <= 1e-4
    return margin


def _tolerance(gpu, cpu, full):
    """(tol, max |logit|, fp32 logits of ``full``) as tests/test_generate_gpu.py measures them"""
    import paddle_hackathon_amd as paddle
    with torch.no_grad():
        fp32 = cpu(paddle.to_tensor(full.numpy()))._t.float()
        paddle.set_device("gpu:0")
        try:
            old = gpu(paddle.to_tensor(full.cuda()))._t.float().cpu()
        finally:
            paddle.set_device("cpu")
    e_old = ((old - fp32).abs().max() / fp32.abs().max()).item()
    return max(2 * e_old, 2.0 ** -8), float(fp32.abs().max()), fp32


def _teacher_forced(gpu, cpu, prompts, lens, out, scores, nret, eos=-1):
    """the returned scores against the fp32 model run over prompt + beam (see the module docstring)"""
    out, scores = out.cpu(), scores.cpu()
    for r in range(out.shape[0]):
        b = r // nret
        full = torch.cat([prompts[b, :lens[b]], out[r]])[None]
        tol, big, fp32 = _tolerance(gpu, cpu, full)
        lp = torch.log_softmax(fp32[0, lens[b] - 1:lens[b] - 1 + out.shape[1]], -1).gather(1, out[r][:, None])[:, 0]
        hit = (out[r] == eos).nonzero()
        n = int(hit[0]) + 1 if len(hit) else out.shape[1]
        diff = abs(float(lp[:n].sum()) - float(scores[r].sum()))
        bound = n * 2 * tol * big
        print(f"row {r}: score {float(scores[r].sum()):.4f}, teacher-forced {float(lp[:n].sum()):.4f}, "
              f"diff {diff:.3e} (bound {bound:.3e}, tol {tol:.3e})")
        assert diff <= bound


@HEADS
def test_beam_search_takes_the_kernels_and_scores_match_fp32(heads, rec, monkeypatch):
    from paddle_hackathon_amd.ops import fallback
    gpu, cpu, ids = _models(heads)
    P = ids.shape[1]
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")           # a fallback anywhere in the step raises
    before = fallback.total()
    out, scores = gpu.generate(ids.cuda(), NEW, decode_strategy="beam_search", num_beams=K, num_return_sequences=K,
                               use_graph=False)
    out, scores = out._t, scores._t
    monkeypatch.delenv("PHA_STRICT_NATIVE")
    assert fallback.total() == before
    assert out.is_cuda and tuple(out.shape) == (B * K, NEW) and out.dtype == torch.int64
    assert tuple(scores.shape) == (B * K, NEW) and scores.dtype == torch.float32
    assert rec["decode_attention"] == LAYERS * (NEW - 1) == rec["with_table"]   # every step, every layer, with a table
    assert rec["beam_search_step"] == NEW and rec["sample_logits"] == 0
    margin = _replay(rec["steps"])
    assert margin > ref.MARGIN, f"a step of the committed prompt has a reference margin of {margin}"
    total = scores.sum(1).reshape(B, K)
    assert bool((total[:, :-1] >= total[:, 1:]).all())     # best beam first
    assert len({tuple(r) for r in out[:K].tolist()}) == K  # the K beams of an item are K different histories
    _teacher_forced(gpu, cpu, ids, [P] * B, out, scores, K)


@HEADS
def test_one_beam_is_greedy_search_bit_for_bit(heads):
    gpu, _, ids = _models(heads)
    g, gs = gpu.generate(ids.cuda(), NEW, use_graph=False)
    b, bs = gpu.generate(ids.cuda(), NEW, decode_strategy="beam_search", num_beams=1, use_graph=False)
    assert torch.equal(g._t, b._t)
    assert torch.equal(gs._t, bs._t)


@HEADS
def test_graph_equals_eager_and_is_reused(heads):
    from paddle_hackathon_amd.models import GPTGenerator
    gpu, _, ids = _models(heads)
    P = ids.shape[1]
    gen = GPTGenerator(gpu)
    kw = dict(decode_strategy="beam_search", num_beams=K, num_return_sequences=K)
    eager, eager_scores = gen.generate(ids.cuda(), NEW, use_graph=False, **kw)
    assert gen.captures == 0
    graph, graph_scores = gen.generate(ids.cuda(), NEW, use_graph=True, **kw)
    assert gen.captures == 1
    assert torch.equal(eager._t, graph._t) and torch.equal(eager_scores._t, graph_scores._t)
    again, again_scores = gen.generate(ids.cuda(), NEW, **kw)          # None: the kernel path everywhere -> graph
    assert gen.captures == 1
    assert torch.equal(again._t, graph._t) and torch.equal(again_scores._t, graph_scores._t)
    for c in gen.last_caches:
        assert tuple(c.shape) == (2, B * K, heads, P + NEW, 256 // heads)
        assert bool((c[:, :, :, P + NEW - 1:] == 0).all())             # nothing written past the last step
        assert bool((c[:, 1::K, :, :P] == 0).all())                    # the prompt is stored once per item
    other = torch.randint(0, VOCAB, (B, P), generator=torch.Generator().manual_seed(99)).cuda()
    a, sa = gen.generate(other, NEW, **kw)                             # same key, new prompt: replays, fresh result
    b, sb = gen.generate(other, NEW, use_graph=False, **kw)
    assert gen.captures == 1 and torch.equal(a._t, b._t) and torch.equal(sa._t, sb._t)
    one, _ = gen.generate(ids.cuda(), NEW, decode_strategy="beam_search", num_beams=2)   # another K: another graph
    assert gen.captures == 2 and tuple(one._t.shape) == (B, NEW)


@HEADS
def test_ragged_prompts_equal_each_item_alone(heads, rec):
    gpu, cpu, ids = _models(heads)
    P = ids.shape[1]
    lens = [P, P - 37]
    kw = dict(decode_strategy="beam_search", num_beams=K, num_return_sequences=K, use_graph=False)
    out, scores = gpu.generate(ids.cuda(), NEW, seq_lens=lens, **kw)
    margin = _replay(rec["steps"])
    assert rec["with_table"] == LAYERS * (NEW - 1)
    _teacher_forced(gpu, cpu, ids, lens, out._t, scores._t, K)
    for b in range(B):
        rec["steps"].clear()
        alone, _ = gpu.generate(ids[b:b + 1, :lens[b]].cuda(), NEW, **kw)
        margin = min(margin, _replay(rec["steps"]))
        assert margin > ref.MARGIN, f"a step of the committed prompts has a reference margin of {margin}"
        assert torch.equal(alone._t, out._t[b * K:(b + 1) * K])         # token for token: every margin holds


@HEADS
def test_eos_ends_beams_early_and_length_penalty_orders_them(heads, rec):
    gpu, cpu, ids = _models(heads)
    P = ids.shape[1]
    kw = dict(decode_strategy="beam_search", num_beams=K, num_return_sequences=K, use_graph=False)
    first, _ = gpu.generate(ids.cuda(), NEW, **kw)
    eos = int(first._t[0, 2])                                          # the best beam of item 0 emits it at step 2
    pad = 3 if eos != 3 else 4
    rec["steps"].clear()
    for lp in (0.0, 1.0):
        out, scores = gpu.generate(ids.cuda(), NEW, eos_token_id=eos, pad_token_id=pad, length_penalty=lp, **kw)
        out, scores = out._t.cpu(), scores._t.cpu()
        ended = 0
        lengths = []
        for r in range(B * K):
            hit = (out[r] == eos).nonzero()
            n = int(hit[0]) + 1 if len(hit) else NEW
            lengths.append(n)
            ended += n < NEW
            assert bool((out[r, n:] == pad).all()) and bool((scores[r, n:] == 0).all())
        assert ended >= 1, "the chosen eos ended no returned beam early"
        rank = scores.double().sum(1) / torch.tensor(lengths, dtype=torch.float64) ** lp
        rank = rank.reshape(B, K)
        assert bool((rank[:, :-1] >= rank[:, 1:] - 1e-6).all()), f"length_penalty={lp}: {rank.tolist()}"
        _teacher_forced(gpu, cpu, ids, [P] * B, out, scores, K, eos)
    margin = _replay(rec["steps"])
    assert margin > ref.MARGIN, f"a step of the committed prompt has a reference margin of {margin}"


def test_more_than_16_rows_run_eagerly_on_the_composites(rec):
    from paddle_hackathon_amd.models import GPTGenerator
    from paddle_hackathon_amd.ops import fallback
    gpu, cpu, ids = _models(2)
    P = ids.shape[1]
    gen = GPTGenerator(gpu)
    before = fallback.total()
    out, scores = gen.generate(ids.cuda(), 3, decode_strategy="beam_search", num_beams=9)    # 18 rows
    assert gen.captures == 0 and fallback.total() > before
    assert tuple(out._t.shape) == (B, 3)
    _teacher_forced(gpu, cpu, ids, [P] * B, out._t, scores._t, 1)


def test_composite_attention_through_the_table(monkeypatch):
    """PHA_DECODE_ATTN=0: every layer gathers the beams' keys through the table on the composite; the
    scores still match the fp32 model. The composite itself must not sync the host."""
    from paddle_hackathon_amd.incubate.nn import functional as FF
    from paddle_hackathon_amd.models import GPTGenerator
    gpu, cpu, ids = _models(2)
    P = ids.shape[1]
    kw = dict(decode_strategy="beam_search", num_beams=K, num_return_sequences=K, use_graph=False)
    want, _ = GPTGenerator(gpu).generate(ids.cuda(), NEW, **kw)
    monkeypatch.setenv("PHA_DECODE_ATTN", "0")
    out, scores = GPTGenerator(gpu).generate(ids.cuda(), NEW, **kw)
    _teacher_forced(gpu, cpu, ids, [P] * B, out._t, scores._t, K)
    same = (out._t == want._t).all(1).float().mean().item()
    print(f"composite attention: {same:.2f} of the returned beams equal the kernel path's")

    g = torch.Generator(device="cuda").manual_seed(0)
    R, H, D, S = 8, 2, 64, 40
    q, k, v = (torch.randn(R, H, 1, D, device="cuda", generator=g).bfloat16() for _ in range(3))
    c = torch.randn(2, R, H, S, D, device="cuda", generator=g).bfloat16()
    ind = torch.randint(0, K, (R, S), device="cuda", generator=g, dtype=torch.int32)
    ts = torch.full((R,), 17, dtype=torch.int32, device="cuda")
    FF._decode_beam_composite(q, k, v, c.clone(), ts, ind, K, None, 0.0, False, "upscale_in_train")   # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o = FF._decode_beam_composite(q, k, v, c, ts, ind, K, None, 0.0, False, "upscale_in_train")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(o.float()).all())
