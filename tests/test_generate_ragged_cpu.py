"""Generation from prompts of different lengths (``seq_lens`` / ``attention_mask`` of
models/gpt_generate.py) on the CPU in fp32: gpt-tiny, seed 0, initializer_range 0.2, four prompt rows
of lengths (7, 4, 1, 6) and 12 new tokens. Every row of the ragged call must equal ``generate`` on
that row alone, token for token, with scores within 1e-5.

Precondition, asserted here: along every row's own continuation the uncached top-2 logit gap exceeds
1e-3, far above fp32 rounding, so the argmax cannot flip between the batched and the lone run."""
import pytest
import torch

LENS = (7, 4, 1, 6)
B, P, NEW = len(LENS), max(LENS), 12

_state = {}


def _setup():
    """(model, prompt ids [B, P], per-row reference: generate on each row alone)"""
    if not _state:
        import paddle_hackathon_amd as paddle
        from paddle_hackathon_amd.models import gpt_config, GPTForPretraining
        paddle.set_device("cpu")
        paddle.seed(0)
        model = GPTForPretraining(gpt_config("gpt-tiny", initializer_range=0.2))
        model.eval()
        ids = torch.randint(0, model.cfg.vocab_size, (B, P), generator=torch.Generator().manual_seed(0))
        alone = [model.generate(ids[b:b + 1, :LENS[b]], NEW) for b in range(B)]
        _state["v"] = (model, ids, torch.cat([a[0]._t for a in alone]), torch.cat([a[1]._t for a in alone]))
    return _state["v"]


def _mask(left):
    m = torch.zeros(B, P, dtype=torch.int64)
    for b, n in enumerate(LENS):
        if left:
            m[b, P - n:] = 1
        else:
            m[b, :n] = 1
    return m


def _same(out, ref_ids, ref_scores):
    assert torch.equal(out[0]._t, ref_ids)
    assert float((out[1]._t - ref_scores).abs().max()) <= 1e-5


def test_precondition_top2_gap():
    import paddle_hackathon_amd as paddle
    model, ids, ref_ids, _ = _setup()
    for b, n in enumerate(LENS):
        full = torch.cat([ids[b:b + 1, :n], ref_ids[b:b + 1]], 1)
        with torch.no_grad():
            lg = model(paddle.to_tensor(full.numpy()))._t[0, n - 1:n - 1 + NEW].float()
        top = lg.topk(2, -1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        print(f"row {b} (len {n}): smallest top-2 logit gap {gap:.3f}")
        assert gap > 1e-3
        assert torch.equal(lg.argmax(-1), ref_ids[b])   # the lone cached run is the uncached argmax


def test_seq_lens_rows_equal_each_row_alone():
    model, ids, ref_ids, ref_scores = _setup()
    out = model.generate(ids, NEW, seq_lens=list(LENS))
    assert tuple(out[0]._t.shape) == (B, NEW) and out[0]._t.dtype == torch.int64
    _same(out, ref_ids, ref_scores)
    _same(model.generate(ids, NEW, seq_lens=torch.tensor(LENS)), ref_ids, ref_scores)


def test_padding_content_is_ignored():
    model, ids, ref_ids, ref_scores = _setup()
    other = ids.clone()
    for b, n in enumerate(LENS):
        other[b, n:] = (other[b, n:] + 17) % model.cfg.vocab_size
    _same(model.generate(other, NEW, seq_lens=list(LENS)), ref_ids, ref_scores)


def test_attention_mask_right_padded_equals_seq_lens():
    model, ids, ref_ids, ref_scores = _setup()
    _same(model.generate(ids, NEW, attention_mask=_mask(left=False)), ref_ids, ref_scores)
    _same(model.generate(ids, NEW, attention_mask=_mask(left=False).bool()), ref_ids, ref_scores)


def test_attention_mask_left_padded_equals_seq_lens():
    model, ids, ref_ids, ref_scores = _setup()
    left = torch.zeros_like(ids)
    for b, n in enumerate(LENS):
        left[b, P - n:] = ids[b, :n]
    _same(model.generate(left, NEW, attention_mask=_mask(left=True)), ref_ids, ref_scores)


def test_trailing_all_padding_columns_are_dropped():
    model, ids, ref_ids, ref_scores = _setup()
    wide = torch.cat([ids, torch.zeros(B, 5, dtype=ids.dtype)], 1)
    pos = model.cfg.max_position_embeddings
    _same(model.generate(wide, NEW, seq_lens=list(LENS)), ref_ids, ref_scores)
    # only the longest prompt counts against the position table
    room = pos - P
    widest = torch.cat([ids, torch.zeros(B, pos - P, dtype=ids.dtype)], 1)
    out = model.generate(widest, room, seq_lens=list(LENS))
    assert tuple(out[0]._t.shape) == (B, room)


def test_full_lengths_are_bitwise_the_plain_call():
    model, ids, _, _ = _setup()
    plain = model.generate(ids, NEW)
    for kw in (dict(seq_lens=[P] * B), dict(attention_mask=torch.ones(B, P, dtype=torch.bool))):
        out = model.generate(ids, NEW, **kw)
        assert torch.equal(out[0]._t, plain[0]._t) and torch.equal(out[1]._t, plain[1]._t)


def test_eos_pads_only_its_row():
    model, ids, ref_ids, _ = _setup()
    rows = [ref_ids[b].tolist() for b in range(B)]
    # a token that one row alone emits, and not as its last one: that row finishes early, no other does
    picks = [(b, t) for b in range(B) for t in rows[b][:-1] if t != 1 and all(t not in rows[o] for o in range(B) if o != b)]
    assert picks, "no row emits a token of its own"
    row, eos = picks[0]
    first = rows[row].index(eos)
    out, scores = model.generate(ids, NEW, seq_lens=list(LENS), eos_token_id=eos, pad_token_id=1)
    out, scores = out._t, scores._t
    assert torch.equal(out[row, :first + 1], ref_ids[row, :first + 1])
    assert bool((out[row, first + 1:] == 1).all()) and bool((scores[row, first + 1:] == 0).all())
    for b in range(B):
        if b != row:
            assert torch.equal(out[b], ref_ids[b])


@pytest.mark.parametrize("case", ["zero length", "length above P", "hole", "neither edge", "both arguments",
                                  "position table"])
def test_rejections(case):
    model, ids, _, _ = _setup()
    kw, new = {}, NEW
    if case == "zero length":
        kw = dict(seq_lens=[7, 0, 1, 6])
    elif case == "length above P":
        kw = dict(seq_lens=[7, 4, P + 1, 6])
    elif case == "hole":
        m = _mask(left=False)
        m[0, 2] = 0
        kw = dict(attention_mask=m)
    elif case == "neither edge":
        m = _mask(left=False)
        m[1] = 0
        m[1, 1:4] = 1
        kw = dict(attention_mask=m)
    elif case == "both arguments":
        kw = dict(seq_lens=list(LENS), attention_mask=_mask(left=False))
    else:
        kw = dict(seq_lens=list(LENS))
        new = model.cfg.max_position_embeddings - P + 1
    with pytest.raises(ValueError):
        model.generate(ids, new, **kw)
