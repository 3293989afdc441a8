"""The beam-search step kernels (csrc/kernels/beam_search.hip, ops.hip.beam_search_step) against the
float64 / stable-sort reference in tests/beam_reference.py.

Tokens, parents, finished flags, lengths and the re-ordered table must match exactly; cum and the
tokens' log probabilities within 1e-4, the bound tests/test_sample_logits_gpu.py uses for ``logprob``.
The order between beams depends on an fp32 sum, so every case first asserts, on the reference alone,
that adjacent totals around ranks 1 .. K + 1 are more than 1e-3 apart (exact ties inside one row
excepted: the contract orders those by index). The seeds are chosen so that this holds (the CPU test
tests/test_generate_beam_cpu.py checks the same cases without a GPU). ``cross_tie`` is the one case
that is about a tie between beams: two beams with bit-identical logits and equal cum, whose fp32
totals are bit-identical too, and the lower beam must come first.
"""
import pytest
import torch

import beam_reference as ref

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(4, 1), (8, 2), (8, 4), (16, 4), (16, 16)]     # (R, K): at least two groups, and K = 16 with B = 1


def _kinds(K):
    return [k for k in ref.KINDS if K >= 2 or k not in ("few_finite", "cross_tie")]


CASES = [(kind, dt, V, R, K) for (R, K) in SHAPES for V in (519, 520) for dt in DTYPES for kind in _kinds(K)]


def _gpu(case):
    """the case's tensors on the GPU; the logits keep their row stride"""
    lg = case["logits"]
    base = torch.empty((lg.shape[0], lg.stride(0)), dtype=lg.dtype, device="cuda")
    base.copy_(torch.as_strided(lg, (lg.shape[0], lg.stride(0)), (lg.stride(0), 1)))
    return dict(logits=base[:, :lg.shape[1]], cum=case["cum"].cuda(), finished=case["finished"].cuda(),
                lengths=case["lengths"].cuda(), table=case["table"].cuda(), ts=case["ts"].cuda())


def _check(case, want, got, d, tag):
    tok, parent, lp = got
    assert tok.dtype == torch.int64 and parent.dtype == torch.int32 and lp.dtype == torch.float32
    assert torch.equal(tok.cpu(), want["tok"]), f"{tag}: tokens {tok.cpu().tolist()} != {want['tok'].tolist()}"
    assert torch.equal(parent.cpu(), want["parent"]), f"{tag}: parents"
    assert torch.equal(d["finished"].cpu(), want["finished"]), f"{tag}: finished"
    assert torch.equal(d["lengths"].cpu(), want["lengths"]), f"{tag}: lengths"
    assert torch.equal(d["table"].cpu(), want["table"]), f"{tag}: table"
    for name, have, exp in (("cum", d["cum"], want["cum"]), ("logprob", lp, want["logprob"])):
        have, exp = have.cpu().double(), exp.double()
        inf = exp == float("-inf")
        assert torch.equal(have == float("-inf"), inf), f"{tag}: {name} -inf pattern"
        err = float((have - exp)[~inf].abs().max()) if bool((~inf).any()) else 0.0
        print(f"{tag}: {name} max error {err:.3e}")
        assert err <= 1e-4, f"{tag}: {name} off by {err}"
    # nothing above a row's step was touched
    above = torch.arange(ref.MAX_SEQ)[None, :] > case["ts"][:, None].long()
    assert bool((d["table"].cpu()[above] == ref.SENTINEL).all())


@pytest.mark.parametrize("kind,dt,V,R,K", CASES, ids=[f"{k}-{d}-V{V}-R{R}-K{K}" for k, d, V, R, K in CASES])
def test_step_matches_the_reference(kind, dt, V, R, K):
    from paddle_hackathon_amd.ops import hip
    case = ref.make_case(kind, DTYPES[dt], V, R, K, seed=ref.case_seed(kind, dt, V, R, K))
    want = ref.case_reference(case)
    if kind != "cross_tie":
        assert want["margin"] > ref.MARGIN, f"the seed of this case leaves a margin of {want['margin']}"
    d = _gpu(case)
    assert hip.beam_search_step_supported(d["logits"], d["cum"], d["finished"], d["lengths"], K, d["table"], d["ts"])
    got = hip.beam_search_step(d["logits"], d["cum"], d["finished"], d["lengths"], case["eos"], K, d["table"], d["ts"])
    _check(case, want, got, d, f"{kind} {dt} V={V} R={R} K={K}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_large_vocabulary_with_a_row_stride(dt):
    from paddle_hackathon_amd.ops import hip
    V, R, K = 50304, 8, 4
    case = ref.make_case("some_finished", DTYPES[dt], V, R, K, seed=ref.case_seed("some_finished", dt, V, R, K),
                         ld=50312)
    want = ref.case_reference(case)
    assert want["margin"] > ref.MARGIN
    d = _gpu(case)
    assert d["logits"].stride(0) == 50312
    got = hip.beam_search_step(d["logits"], d["cum"], d["finished"], d["lengths"], case["eos"], K, d["table"], d["ts"])
    _check(case, want, got, d, f"V=50304 {dt}")


@pytest.mark.parametrize("layout", ["V520", "V521_ld528", "V521_unaligned"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_one_beam_step_scores_as_the_greedy_sampler_bit_for_bit(dt, layout):
    """Both kernels stage, key and score a row through csrc/kernels/logit_keys.h, so with one beam, cum = 0
    and nothing finished the beam step must return the greedy sampler's token and, bitwise, its log
    probability. The layouts reach every staging path: 16-byte loads only; 16-byte loads and a scalar
    tail; a row base that is not 16-byte aligned, all scalar. Row 1 holds its maximum twice: the lower
    index wins in both."""
    from paddle_hackathon_amd.ops import hip
    R, V, ld = (4, 520, 520) if layout == "V520" else (4, 521, 528)
    off = 1 if layout == "V521_unaligned" else 0
    buf = torch.zeros(off + R * ld, dtype=DTYPES[dt], device="cuda")
    logits = buf[off:].view(R, ld)[:, :V]
    logits.copy_(torch.randn(R, V, generator=torch.Generator().manual_seed(V + off)).to(DTYPES[dt]))
    logits[1, 37] = logits[1, V - 1] = 9.0   # above every other logit of the row (a 520-sample normal)
    assert (logits.data_ptr() % 16 == 0) == (off == 0) and logits.stride(0) == ld
    assert int((logits[1] == logits[1].max()).sum()) == 2 and bool(torch.isfinite(logits).all())
    cum = torch.zeros(R, dtype=torch.float32, device="cuda")
    finished = torch.zeros(R, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(R, dtype=torch.int32, device="cuda")
    table = torch.zeros(R, 4, dtype=torch.int32, device="cuda")
    assert hip.beam_search_step_supported(logits, cum, finished, lengths, 1, table, 0)
    tok, parent, lp = hip.beam_search_step(logits, cum, finished, lengths, -1, 1, table, 0)
    u = torch.zeros(R, dtype=torch.float32, device="cuda")
    assert hip.sample_logits_supported(logits, u, top_k=1)
    ids, slp = hip.sample_logits(logits, u, top_k=1)
    assert torch.equal(tok, ids), f"{tok.tolist()} != {ids.tolist()}"
    assert torch.equal(lp, slp), f"{lp.tolist()} != {slp.tolist()}"
    assert int(tok[1]) == 37 and int(ids[1]) == 37
    assert torch.equal(cum, lp) and int(parent.abs().sum()) == 0


@pytest.mark.parametrize("form", ["int", "one_element"])
def test_a_uniform_time_step_is_broadcast(form):
    from paddle_hackathon_amd.ops import hip
    case = ref.make_case("random", torch.bfloat16, 520, 8, 4, seed=ref.case_seed("random", "bf16", 520, 8, 4))
    want = ref.case_reference(case)
    d = _gpu(case)
    ts = 20 if form == "int" else torch.tensor([20], dtype=torch.int32, device="cuda")
    got = hip.beam_search_step(d["logits"], d["cum"], d["finished"], d["lengths"], case["eos"], 4, d["table"], ts)
    _check(case, want, got, d, f"time_step as {form}")


@pytest.mark.parametrize("kind", ["random", "some_finished", "few_finite"])
def test_composite_matches_the_reference_on_the_gpu(kind, monkeypatch):
    from paddle_hackathon_amd.ops import hip
    monkeypatch.setenv("PHA_BEAM_KERNEL", "0")
    case = ref.make_case(kind, torch.bfloat16, 519, 8, 4, seed=ref.case_seed(kind, "bf16", 519, 8, 4))
    want = ref.case_reference(case)
    assert want["margin"] > ref.MARGIN
    d = _gpu(case)
    got = hip.beam_search_step(d["logits"], d["cum"], d["finished"], d["lengths"], case["eos"], 4, d["table"], d["ts"])
    _check(case, want, got, d, f"composite {kind}")


def test_a_step_in_a_captured_graph_equals_the_eager_one():
    from paddle_hackathon_amd.ops import hip
    case = ref.make_case("some_finished", torch.bfloat16, 520, 16, 4,
                         seed=ref.case_seed("some_finished", "bf16", 520, 16, 4))
    want = ref.case_reference(case)
    eager = _gpu(case)
    e_out = hip.beam_search_step(eager["logits"], eager["cum"], eager["finished"], eager["lengths"], case["eos"], 4,
                                 eager["table"], eager["ts"])
    d = _gpu(case)
    keep = {k: d[k].clone() for k in ("cum", "finished", "lengths", "table")}
    # warm-up
    hip.beam_search_step(d["logits"], d["cum"], d["finished"], d["lengths"], case["eos"], 4, d["table"], d["ts"])
    for k, v in keep.items():
        d[k].copy_(v)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.beam_search_step(d["logits"], d["cum"], d["finished"], d["lengths"], case["eos"], 4, d["table"],
                                   d["ts"])
    for k, v in keep.items():
        d[k].copy_(v)
    g.replay()
    torch.cuda.synchronize()
    _check(case, want, out, d, "graph")
    for a, b in zip(out, e_out):
        assert torch.equal(a, b)
    for k in keep:
        assert torch.equal(d[k], eager[k])


def test_rejections():
    from paddle_hackathon_amd.ops import hip
    case = ref.make_case("random", torch.bfloat16, 520, 8, 4, seed=1)
    d = _gpu(case)
    base = (("logits", d["logits"]), ("cum", d["cum"]), ("finished", d["finished"]), ("lengths", d["lengths"]), ("eos", 7),
            ("K", 4), ("table", d["table"]), ("ts", d["ts"]))
    args = lambda **kw: [kw.get(k, v) for k, v in base]
    bad = [dict(cum=d["cum"].double()), dict(cum=d["cum"].cpu()), dict(finished=d["finished"].bool()),
           dict(lengths=d["lengths"].long()), dict(K=3), dict(K=0), dict(K=521), dict(table=d["table"][:, ::2]),
           dict(table=d["table"].long()), dict(table=d["table"][:4]), dict(ts=d["ts"].long()), dict(ts=d["ts"][:3]),
           dict(ts=ref.MAX_SEQ), dict(ts=-1), dict(logits=d["logits"][:, ::2]), dict(logits=d["logits"][0])]
    for kw in bad:
        with pytest.raises(ValueError):
            hip.beam_search_step(*args(**kw))
        a = args(**kw)
        assert not hip.beam_search_step_supported(*(a[:4] + a[5:]))
    f32 = args(logits=d["logits"].float())
    assert not hip.beam_search_step_supported(*(f32[:4] + f32[5:]))
    assert "float32" in hip.beam_search_step_why_not(*(f32[:4] + f32[5:]))
