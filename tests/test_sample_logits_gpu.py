"""ops.hip.sample_logits on the sampling kernel (csrc/kernels/sampling.hip) against its contract in
float64 numpy (tests/sampling_reference.py) on the bf16- / fp16-valued logits. Token ids are exact.

Midpoint method: for a kept token the reference gives the interval of u that returns it; u is set to
the middle of that interval, so the kernel must return exactly that token as long as its running
masses are within half the interval's width of the reference's. Every targeted interval is asserted
to be at least 2^-8 wide (never skipped), against an fp32 summation error of about 1e-5 over
V = 50,304: a margin of more than a hundred.

Seeds: logits are N(0, std 2). Seed 0 at V = 50,304 gives a smallest kept probability of 0.0078 at
k = 50; at V = 520, B = 16 the seeds 0 - 3 leave a row whose 50th probability is below 2^-8, seed 52
(found on the CPU) gives 0.0045. In bf16 those rows have up to 4 logits tied at the k-th value of which
only some are inside the first k, which makes them the tie test as well.

All logits tensors have V + 8 columns with +inf in the 8 beyond V (row stride V + 8): an element
read past V would win every argmax and own all the mass.

Seen on an MI355X over this file: every id exact; largest logprob error 5.6e-07 (bound 1e-4); largest
prefix mass of a token returned at top_p = 0.9 on random rows 0.899459 (bound 0.9 + 2^-10)
(profiles/generate/README.md).
"""
import numpy as np
import pytest
import torch

from sampling_reference import RowRef, designed_row, random_logits

pytestmark = pytest.mark.gpu

MIN_WIDTH = 2.0 ** -8
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(3, 50304, 0), (16, 520, 52)]   # B, V, seed


def _hip():
    from paddle_hackathon_amd.ops import hip
    return hip


def _stage(x, dtype):
    """x [B, V] float64 -> (device logits [B, V] inside a [B, V + 8] buffer of +inf, their float64 values)"""
    t = torch.from_numpy(np.asarray(x)).to(dtype)
    B, V = t.shape
    buf = torch.full((B, V + 8), float("inf"), dtype=dtype, device="cuda")
    buf[:, :V] = t.cuda()
    return buf[:, :V], t.double().numpy()


_cache = {}


def _random(B, V, seed, dtype):
    key = (B, V, seed, dtype)
    if key not in _cache:
        _cache[key] = _stage(random_logits(B, V, seed), dtype)
    return _cache[key]


def _u(values):
    return torch.tensor(values, dtype=torch.float32, device="cuda")


def _check_midpoints(fn, logits, refs, **kw):
    """every kept token of every row is returned at the midpoint of its interval; returns the number checked"""
    mids = [r.midpoints() for r in refs]
    assert all(w >= MIN_WIDTH for m in mids for _, _, w in m), "precondition: an interval is below 2^-8"
    n = 0
    for j in range(max(len(m) for m in mids)):
        pick = [m[min(j, len(m) - 1)] for m in mids]
        ids, _ = fn(logits, _u([p[1] for p in pick]), **kw)
        assert ids.dtype == torch.int64 and ids.tolist() == [p[0] for p in pick], f"kept token {j}"
        n += len(pick)
    return n


@pytest.mark.parametrize("top_k", [1, 5, 50])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,V,seed", SHAPES, ids=["V50304", "V520"])
def test_random_rows_top_k_returns_every_kept_token(B, V, seed, dtype, top_k):
    hip = _hip()
    logits, x = _random(B, V, seed, dtype)
    assert logits.stride(0) == V + 8 and hip.sample_logits_supported(logits, _u([0.0] * B), 1.0, top_k, 1.0)
    refs = [RowRef(x[b], 1.0, top_k, 1.0) for b in range(B)]
    if top_k == 50 and dtype == torch.bfloat16:
        kth = [np.sort(x[b])[-top_k] for b in range(B)]
        assert any((x[b] == kth[b]).sum() > (x[b][refs[b].kept] == kth[b]).sum() for b in range(B)), \
            "no row has a tie that straddles the k-th place"
    assert _check_midpoints(hip.sample_logits, logits, refs, top_k=top_k) >= B


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 0.85), (1.0, 7, 0.75), (0.7, 0, 0.9), (1.5, 0, 0.85),
                                                     (1.5, 9, 0.8)])
def test_designed_rows_exact_top_p(dtype, temperature, top_k, top_p):
    """12 head tokens, three of them tied across the boundary, the tail 30 below: top-p is exact"""
    hip = _hip()
    rows = [designed_row(520, s)[0] for s in range(3)]
    logits, x = _stage(np.stack(rows), dtype)
    B = len(rows)
    refs = [RowRef(x[b], temperature, top_k, top_p) for b in range(B)]
    for r in refs:
        assert np.abs(r.cum - top_p).min() >= MIN_WIDTH, "precondition: a cumulative mass is within 2^-8 of top_p"
        assert 1 <= len(r.kept) < 12
    if (temperature, top_k, top_p) == (1.0, 0, 0.85):
        for b, r in enumerate(refs):   # the boundary cuts the three tied tokens: the lowest indices stay
            tied = np.nonzero(x[b] == x[b][r.order[5]])[0]
            assert len(tied) == 3 and sorted(set(tied) & set(r.kept)) == sorted(tied)[:2]
    kw = dict(temperature=temperature, top_k=top_k, top_p=top_p)
    _check_midpoints(hip.sample_logits, logits, refs, **kw)          # each kept token, the last one included
    for j in range(64):                                               # and never one outside the set
        u = (j + 0.5) / 64
        ids, _ = hip.sample_logits(logits, _u([u] * B), **kw)
        for b, t in enumerate(ids.tolist()):
            assert t in refs[b].kept, f"u={u}: token {t} is outside the kept set"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,V,seed", SHAPES, ids=["V50304", "V520"])
def test_random_rows_top_p_stays_inside_the_nucleus(B, V, seed, dtype):
    """tail steps are about 1e-5, so the boundary is fuzzy: the returned token's prefix mass in the
    reference order is below top_p + 2^-10"""
    hip = _hip()
    logits, x = _random(B, V, seed, dtype)
    refs = [RowRef(x[b]) for b in range(B)]
    worst = 0.0
    for j in range(64):
        ids, _ = hip.sample_logits(logits, _u([(j + 0.5) / 64] * B), top_p=0.9)
        for b, t in enumerate(ids.tolist()):
            worst = max(worst, refs[b].prefix_mass(t))
    print(f"V={V} {dtype}: largest prefix mass of a returned token {worst:.6f}")
    assert worst < 0.9 + 2.0 ** -10


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,V,seed", SHAPES, ids=["V50304", "V520"])
def test_logprob_matches_float64(B, V, seed, dtype):
    hip = _hip()
    logits, x = _random(B, V, seed, dtype)
    worst = 0.0
    for temperature, top_k in ((1.0, 0), (0.7, 50), (1.5, 1)):
        refs = [RowRef(x[b], temperature) for b in range(B)]
        ids, lp = hip.sample_logits(logits, _u([0.37] * B), temperature=temperature, top_k=top_k)
        assert lp.dtype == torch.float32
        for b, t in enumerate(ids.tolist()):
            worst = max(worst, abs(float(lp[b]) - refs[b].logp[t]))
    print(f"V={V} {dtype}: largest logprob error {worst:.3e}")
    assert worst <= 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_greedy_is_the_first_argmax(dtype):
    hip = _hip()
    x = random_logits(4, 520, 5)
    x[1, 400] = x[1, 17] = x[1].max() + 1.0      # a duplicated maximum
    x[2, :] = -1.25                              # one constant
    x[3, 0] = x[3, 519] = 9.0
    logits, xr = _stage(x, dtype)
    ids, _ = hip.sample_logits(logits, _u([0.99] * 4), top_k=1)
    assert ids.tolist() == [int(np.argmax(xr[b])) for b in range(4)]
    assert ids.tolist()[1:] == [17, 0, 0]
    big, xb = _random(3, 50304, 0, dtype)
    ids, _ = hip.sample_logits(big, _u([0.5] * 3), top_k=1, top_p=0.5, temperature=0.3)
    assert ids.tolist() == [int(np.argmax(xb[b])) for b in range(3)]


def test_eos_and_pad_bookkeeping():
    hip = _hip()
    x = np.full((4, 520), -5.0)
    x[0, 11] = x[1, 22] = x[2, 33] = x[3, 22] = 5.0
    logits, _ = _stage(x, torch.bfloat16)
    finished = torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device="cuda")
    ids, lp = hip.sample_logits(logits, _u([0.5] * 4), top_k=1, finished=finished, eos_token_id=22, pad_token_id=7)
    assert ids.tolist() == [11, 22, 7, 22]                 # the finished row returns pad
    assert finished.tolist() == [0, 1, 1, 1]               # the rows that returned EOS are flagged, row 2 stays
    assert float(lp[2]) == 0.0
    ids, _ = hip.sample_logits(logits, _u([0.5] * 4), top_k=1, finished=finished, eos_token_id=22, pad_token_id=7)
    assert ids.tolist() == [11, 7, 7, 7] and finished.tolist() == [0, 1, 1, 1]
    ids, _ = hip.sample_logits(logits, _u([0.5] * 4), top_k=1, finished=None, eos_token_id=22)
    assert ids.tolist() == [11, 22, 33, 22]


def test_guard_elements_are_never_read_or_written():
    hip = _hip()
    logits, x = _random(16, 520, 52, torch.bfloat16)      # +inf beyond V in every row
    B = 16
    ids_buf = torch.full((B + 16,), -77, dtype=torch.int64, device="cuda")
    lp_buf = torch.full((B + 16,), -77.0, dtype=torch.float32, device="cuda")
    for kw in (dict(top_k=1), dict(top_k=5), dict(top_p=0.9), dict()):
        ids, lp = hip.sample_logits(logits, _u([0.5] * B), out_ids=ids_buf[8:8 + B], out_logprob=lp_buf[8:8 + B], **kw)
        assert ids.data_ptr() == ids_buf[8:].data_ptr()
        assert bool((ids >= 0).all()) and bool((ids < 520).all()) and bool(torch.isfinite(lp).all())
        assert bool((ids_buf[:8] == -77).all()) and bool((ids_buf[8 + B:] == -77).all())
        assert bool((lp_buf[:8] == -77).all()) and bool((lp_buf[8 + B:] == -77).all())


@pytest.mark.parametrize("kw", [dict(top_k=1), dict(top_k=50), dict(top_p=0.9), dict(top_k=50, top_p=0.9, temperature=0.8),
                                dict()], ids=["greedy", "k50", "p09", "k50p09", "plain"])
def test_two_calls_are_bitwise_equal(kw):
    hip = _hip()
    logits, _ = _random(3, 50304, 0, torch.bfloat16)
    u = _u([0.123, 0.5, 0.877])
    a, b = hip.sample_logits(logits, u, **kw), hip.sample_logits(logits, u, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_rejections():
    hip = _hip()
    logits, _ = _random(16, 520, 52, torch.bfloat16)
    u = _u([0.5] * 16)
    bad = [
        ("logits", dict(logits=logits[0])),
        ("logits", dict(logits=logits.to(torch.float64))),
        ("logits", dict(logits=logits.t())),
        ("logits", dict(logits=torch.zeros(17, 520, dtype=torch.bfloat16, device="cuda"), u=_u([0.5] * 17))),
        ("logits", dict(logits=logits[:, :1])),
        ("u", dict(u=u[:5])),
        ("u", dict(u=u.double())),
        ("u", dict(u=u.cpu())),
        ("temperature", dict(temperature=0.0)),
        ("temperature", dict(temperature=-1.0)),
        ("top_p", dict(top_p=0.0)),
        ("top_p", dict(top_p=1.5)),
        ("top_k", dict(top_k=-1)),
        ("top_k", dict(top_k=521)),
        ("finished", dict(finished=torch.zeros(16, dtype=torch.bool, device="cuda"))),
        ("finished", dict(finished=torch.zeros(3, dtype=torch.uint8, device="cuda"))),
    ]
    for name, kw in bad:
        args = dict(logits=logits, u=u)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            hip.sample_logits(**args)
    assert hip.SAMPLE_MAX_V >= 50304
    wide = torch.zeros(1, hip.SAMPLE_MAX_V + 8, dtype=torch.bfloat16, device="cuda")
    assert hip.sample_logits_supported(wide[:, :hip.SAMPLE_MAX_V], _u([0.5]))
    assert not hip.sample_logits_supported(wide, _u([0.5]))
    assert "above the kernel" in hip.sample_logits_why_not(wide, _u([0.5]))
    assert not hip.sample_logits_supported(logits.float(), u)          # fp32 stays on the composite


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_composite_gives_the_same_ids(dtype, monkeypatch):
    hip = _hip()
    calls = []
    real = hip._sample_logits_composite
    monkeypatch.setattr(hip, "_sample_logits_composite", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for (B, V, seed), kws in ((SHAPES[0], [dict(top_k=50)]), (SHAPES[1], [dict(top_k=5), dict(top_k=1)])):
        logits, x = _random(B, V, seed, dtype)
        for kw in kws:
            refs = [RowRef(x[b], 1.0, kw["top_k"], 1.0) for b in range(B)]
            mids = [r.midpoints() for r in refs]
            for j in range(0, max(len(m) for m in mids), 7):
                pick = [m[min(j, len(m) - 1)] for m in mids]
                u = _u([p[1] for p in pick])
                monkeypatch.setenv("PHA_SAMPLE_KERNEL", "1")
                n = len(calls)
                a = hip.sample_logits(logits, u, **kw)
                assert len(calls) == n                                   # the kernel ran
                monkeypatch.setenv("PHA_SAMPLE_KERNEL", "0")
                b = hip.sample_logits(logits, u, **kw)
                assert len(calls) == n + 1                               # and the switch forces the composite
                assert a[0].tolist() == b[0].tolist() == [p[0] for p in pick]
                assert float((a[1] - b[1]).abs().max()) <= 1e-4
