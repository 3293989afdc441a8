"""The tanh-GELU epilogue of the weight-streaming GEMM (``act="gelu_tanh"``, the activation the GPT
MLP trains with) against float64, with the bounds and the error measure of
tests/test_skinny_gemm_gpu.py: max|out - ref| / max|ref| <= 2^-8 for bf16 and 2^-10 for fp16.

Shapes: N one column tile plus 8, K two planned splits plus 8 (the smallest that cross a split), with
the planned split count (partials summed by the finish kernel) and one split (epilogue fused into the
product kernel), M = 1 / 8 / 16, both weight layouts, bias and residual.

tanh- and erf-GELU differ by at most 4.7e-4, far below those bounds at outputs of order one. With
every pre-activation in [-2.5, -2.0] all outputs are about -0.03 and the two functions differ by 1 %
of the largest one, so a swapped formula fails ``test_tanh_is_not_erf``.

Largest errors seen on an MI355X over this file: bf16 3.141e-03, fp16 4.64e-04
(profiles/generate/README.md)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def _hip():
    from paddle_hackathon_amd.ops import hip
    return hip


def _shape(nk):
    hip = _hip()
    bn, ks = hip.skinny_gemm_tile(nk)
    _, kps = hip.skinny_gemm_plan(bn, 2 * ks, nk)
    return bn + 8, 2 * kps + 8


def _ref(x, w, nk, b, r, approximate):
    y = x.double() @ (w.double().t() if nk else w.double())
    if b is not None:
        y = y + b.double()
    y = torch.nn.functional.gelu(y, approximate=approximate)
    return y if r is None else y + r.double()


def _err(out, ref):
    return ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("ns", [None, 1], ids=["planned", "fused"])
@pytest.mark.parametrize("bias,res", [(True, True), (True, False), (False, False)], ids=["br", "b", "plain"])
@pytest.mark.parametrize("M", [1, 8, 16])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("nk", [True, False], ids=["nk", "kn"])
def test_gelu_tanh_matches_float64(nk, dtype, M, bias, res, ns):
    hip = _hip()
    N, K = _shape(nk)
    if ns is None:
        assert hip.skinny_gemm_plan(N, K, nk)[0] > 1          # the planned split does cross a seam
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn((N, K) if nk else (K, N), generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, generator=g).to(dtype) if bias else None
    r = torch.randn(M, N, generator=g).to(dtype) if res else None
    out = hip.skinny_gemm(x.cuda(), w.cuda(), nk, None if b is None else b.cuda(), "gelu_tanh",
                          None if r is None else r.cuda(), nsplit=ns)
    assert out.shape == (M, N) and out.dtype == dtype
    e = _err(out, _ref(x, w, nk, b, r, "tanh"))
    print(f"nk={nk} {dtype} M={M} bias={bias} res={res} nsplit={ns}: err {e:.3e} (bound {BOUND[dtype]:.3e})")
    assert e <= BOUND[dtype]


@pytest.mark.parametrize("ns", [None, 1], ids=["planned", "fused"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_tanh_is_not_erf(dtype, ns):
    hip = _hip()
    N, K = _shape(True)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.02 * K ** -0.5).to(dtype)          # the product is about 0.02
    b = (-2.25 + 0.4 * (torch.rand(N, generator=g) - 0.5)).to(dtype)           # pre-activations in [-2.5, -2.0]
    pre = x.double() @ w.double().t() + b.double()
    assert pre.max().item() < -2.0 and pre.min().item() > -2.5
    tanh_ref, erf_ref = _ref(x, w, True, b, None, "tanh"), _ref(x, w, True, b, None, "none")
    assert _err(tanh_ref, erf_ref) > 2 * BOUND[torch.bfloat16]                 # the two functions are apart here
    out_t = hip.skinny_gemm(x.cuda(), w.cuda(), True, b.cuda(), "gelu_tanh", nsplit=ns)
    out_e = hip.skinny_gemm(x.cuda(), w.cuda(), True, b.cuda(), "gelu", nsplit=ns)
    assert _err(out_t, tanh_ref) <= BOUND[dtype] and _err(out_e, erf_ref) <= BOUND[dtype]
    assert _err(out_t, erf_ref) > BOUND[dtype] and _err(out_e, tanh_ref) > BOUND[dtype]


def test_layer_takes_gelu_tanh_on_the_skinny_route(monkeypatch):
    """one decode step of fused_multi_transformer(activation="gelu_tanh") with 8 rows: ffn1 runs on the
    kernel with the tanh epilogue and agrees with the composite (library GEMM + bias_gelu(approximate=True))
    to 2^-7 of the largest output: two bf16 results, each rounded within 2^-8 of the exact one"""
    from paddle_hackathon_amd.incubate.nn import functional as FF
    hip = _hip()
    E, H, D, F = 256, 2, 128, 1024
    g = torch.Generator().manual_seed(2)

    def r(*s, scale=0.05):
        return (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).cuda()

    w = [[1 + r(E)], [r(E)], [r(E, 3, H, D)], [r(3, H, D)], [r(E, E)], [r(E)], [1 + r(E)], [r(E)], [r(E, F)],
         [r(F, scale=1.0)], [r(F, E)], [r(E)]]
    x = r(8, 1, E, scale=1.0)

    def run(activation):
        caches = [torch.zeros(2, 8, H, 16, D, dtype=torch.bfloat16, device="cuda")]
        return FF.fused_multi_transformer(x, *w, activation=activation, trans_qkvw=False, cache_kvs=caches,
                                          time_step=3)[0]._t
    acts = []
    real = hip.skinny_gemm
    monkeypatch.setattr(hip, "skinny_gemm", lambda *a, **k: (acts.append(a[4] if len(a) > 4 else k.get("act", "none")),
                                                            real(*a, **k))[1])
    with torch.no_grad():
        new = run("gelu_tanh")
        assert "gelu_tanh" in acts
        monkeypatch.setenv("PHA_DECODE_GEMM", "0")
        old = run("gelu_tanh")
        erf = run("gelu")
    scale = old.float().abs().max()
    assert ((new.float() - old.float()).abs().max() / scale).item() <= 2.0 ** -7
    assert not torch.equal(old, erf)
    with pytest.raises(ValueError, match="activation"):
        run("swish")
