"""The 256 x 192 tile form of the persistent TN weight-gradient kernel (gemm4p192_kernel in
csrc/kernels/gemm4p.hip, ``gemm_p(..., bn=192)``): every output element sums its K range in the same
order as on the 256 x 256 form, so the product and the column-sum partials (the bias gradient) must
be bitwise equal to it — on tile-multiple and ragged N, a single tile, M tails, fewer work items than
workgroups and several rounds per workgroup. Then a float64 reference, the argument checks of the
entry point, and the static width policy (``ops/gemm._tn_bn``, no GPU needed)."""
import functools

import pytest
import torch

KS = (64 * 4, 64 * 9, 4096)
MS = (8, 256, 264, 520)
NS = (192, 384, 200, 392, 576)
DTS = (torch.bfloat16, torch.float16)


def _r(*s, g, dt):
    return (torch.rand(*s, device="cuda", generator=g) * 2 - 1).to(dt)


@functools.lru_cache(maxsize=None)
def _operands(K, dt):
    """x [K, 520], dy [K, 576] (every case reads a leading block of columns, through the full row
    stride) and their float64 product / column sums, computed once"""
    g = torch.Generator(device="cuda").manual_seed(K)
    x, dy = _r(K, max(MS), g=g, dt=dt), _r(K, max(NS), g=g, dt=dt)
    return x, dy, x.double().t() @ dy.double(), dy.double().sum(0)


def _grids(M, N):
    """workgroup counts: the CU count (never fewer items than it here: the spare workgroups exit),
    and for the largest grid of 3 x 3 items 4 workgroups (three rounds for the first) and 8 (the
    per-XCD chunked walk)"""
    return (0, 4, 8) if (M, N) == (520, 576) else (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dt", DTS, ids=("bf16", "fp16"))
def test_product_bitwise_equals_256_form_and_matches_float64(K, dt):
    from paddle_hackathon_amd.ops import gemm as G
    x, dy, ref, _ = _operands(K, dt)
    for M in MS:
        for N in NS:
            a, b = x[:, :M], dy[:, :N]
            want = G.gemm_p(a, b, True, True, bn=256)
            for grid in _grids(M, N):
                got = G.gemm_p(a, b, True, True, bn=192, grid=grid)
                assert torch.equal(got, want), (M, N, grid)
            # the bound of tests/test_kernels_gpu.py::test_gemm_picks_match_reference (mm_tn)
            r = ref[:M, :N]
            assert ((got.double() - r).abs().max() / r.abs().max()).item() < 1e-2, (M, N)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dt", DTS, ids=("bf16", "fp16"))
def test_colsum_bitwise_equals_256_form_and_matches_float64(K, dt):
    from paddle_hackathon_amd.ops import gemm as G
    x, dy, ref, ref_db = _operands(K, dt)
    for M in MS:
        for N in NS:
            a, b = x[:, :M], dy[:, :N]
            plain = G.gemm_p(a, b, True, True, bn=256)
            _, want = G.gemm_p(a, b, True, True, colsum=True, bn=256)
            rows = 2 * -(-M // 256)
            for grid in _grids(M, N):
                dw, part = G.gemm_p(a, b, True, True, colsum=True, bn=192, grid=grid)
                assert torch.equal(dw, plain), (M, N, grid)
                assert part.shape == (rows + 8, N)
                assert torch.equal(part[:rows], want[:rows]), (M, N, grid)
            db = G.colsum_rows_finish(part, torch.float32)
            r = ref_db[:N]
            assert ((db.double() - r).abs().max() / r.abs().max()).item() < 1e-2, (M, N)


@pytest.mark.gpu
def test_mm_tn_entry_points_take_the_policy_width(monkeypatch):
    """mm_tn / mm_tn_db on a shape the policy moves to 192 (one tile row, N = 3 x 192: the 192 form's
    three items against the 256 form's three cost 0.75 x penalty each) against PHA_TN_BN=256"""
    from paddle_hackathon_amd.ops import gemm as G
    x, dy, ref, ref_db = _operands(KS[1], torch.bfloat16)
    a, b = x[:, :256].contiguous(), dy[:, :576].contiguous()
    cus = G._num_cus(a.device)
    assert G._splits(256, 576, KS[1], a.device) == 1
    assert G._tn_bn(256, 576, 1, cus) == (192 if 0.75 * G.TN_BN192_PENALTY < 1 else 256)
    dw, db = G.mm_tn_db(a, b)
    dw1 = G.mm_tn(a, b)
    monkeypatch.setenv("PHA_TN_BN", "256")
    assert G._tn_bn(256, 576, 1, cus) == 256
    dw_old, db_old = G.mm_tn_db(a, b)
    assert torch.equal(dw, dw_old) and torch.equal(dw1, dw_old) and torch.equal(db, db_old)
    r = ref[:256, :576]
    assert ((dw.double() - r).abs().max() / r.abs().max()).item() < 1e-2


@pytest.mark.gpu
def test_192_form_refuses_what_it_does_not_build():
    from paddle_hackathon_amd.ops import gemm as G
    x, dy, _, _ = _operands(KS[0], torch.bfloat16)
    a, b = x[:, :256], dy[:, :384]
    out = torch.full((256, 384), 7.0, device="cuda", dtype=torch.bfloat16)
    bias = torch.ones(384, device="cuda")
    at, bt = a.t().contiguous(), b.t().contiguous()
    refused = [
        lambda: G.gemm_p(a, b, True, True, out=out, bn=192, splits=2),                 # split-K
        lambda: G.gemm_p(at, bt, False, False, out=out, bn=192),                       # NT
        lambda: G.gemm_p(a, b, True, True, out=out, bn=192, bias=bias),                # bias epilogue
        lambda: G.gemm_p(a, b, True, True, out=out, bn=192, epi_extra=2 << 25),        # K-start stagger
        lambda: G.gemm_p(a, b, True, True, out=out, bn=192, epi_extra=G.EPI_RING),     # NT-only build
        lambda: G.gemm_p(a, b, True, True, out=out, bn=128),                           # unknown width
    ]
    for call in refused:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to its output"
    assert torch.equal(G.gemm_p(a, b, True, True, out=out, bn=192), G.gemm_p(a, b, True, True))


@pytest.mark.parametrize("cus", [256, 304])
def test_width_policy_follows_the_round_model(cus, monkeypatch):
    """static, from the shape and the CU count alone: rounds of work items x per-item time, a
    256 x 192 item costing 0.75 x TN_BN192_PENALTY of a 256 x 256 one"""
    from paddle_hackathon_amd.ops import gemm as G
    monkeypatch.delenv("PHA_TN_BN", raising=False)
    p = G.TN_BN192_PENALTY
    assert 1.0 <= p < 4 / 3, "a 192 item does at least its share of the work; past 4/3 it never pays"

    def model(M, N):
        tm = -(-M // 256)
        t256 = -(-tm * -(-N // 256) // cus)
        t192 = -(-tm * -(-N // 192) // cus) * 0.75 * p
        return 192 if N % 192 == 0 and t192 < t256 else 256

    for M, N in [(2048, 6144), (2048, 8192), (8192, 2048), (2048, 2048), (2048, 50304), (50304, 2048), (768, 2304),
                 (4096, 12288)]:
        assert G._tn_bn(M, N, 1, cus) == model(M, N), (M, N)
        assert G._tn_bn(M, N, 2, cus) == 256, "split products stay on the 256 tile"
    if cus == 256:   # GPT-3 1.3B on MI355X: the qkv dW moves (256 items, one full round), the others stay
        assert G._tn_bn(2048, 6144, 1, cus) == 192
        assert G._tn_bn_model(2048, 6144, cus) == {256: 1.0, 192: 0.75 * p}
        for M, N in [(2048, 8192), (8192, 2048), (2048, 2048)]:
            assert G._tn_bn(M, N, 1, cus) == 256
    monkeypatch.setenv("PHA_TN_BN", "256")
    assert G._tn_bn(2048, 6144, 1, cus) == 256
