"""The weight-only int8 weight-streaming GEMM (csrc/kernels/skinny_w8.hip) against float64 on the CPU from
the same x, q, scale, bias and residual: act((x @ q^T) * scale + b) + r. Error is max|out - ref| / max|ref|,
bound 2^-8 (bf16) / 2^-10 (fp16), the rule of tests/test_skinny_gemm_gpu.py: it applies unchanged because
the kernel dequantises exactly, applies the scale to the fp32 sum and rounds once. q is uniform over all
of [-128, 127]; scale = K^-0.5 / 74 times a channel factor in [0.5, 2]: outputs are O(1). Shapes come from the
exported tile and plan; 4 and 8 K steps in one split run the pipelined loop once and three times."""
import pytest
import torch

from paddle_hackathon_amd.ops import fallback, hip

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
BOUND = {BF: 2.0 ** -8, FP: 2.0 ** -10}
WORST = {}


def _size(sym):
    bn, ks = hip.skinny_gemm_w8_tile()
    s = hip.skinny_gemm_w8_plan(bn, 2 * ks)[1]
    return {"8": 8, "bn-8": bn - 8, "bn": bn, "bn+8": bn + 8, "3bn+8": 3 * bn + 8, "16": 16, "ks-16": ks - 16, "ks": ks,
            "ks+16": ks + 16, "2s-16": 2 * s - 16, "2s+16": 2 * s + 16, "4ks+16": 4 * ks + 16, "8ks": 8 * ks}[sym]


def _inputs(M, N, K, dtype, bias=True, res=True, seed=0):
    """(x, q, scale, bias, residual) on the GPU, drawn on the CPU and rounded to their dtypes"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    q = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    s = ((K ** -0.5 / 74) * (0.5 + 1.5 * torch.rand(N, generator=g))).float()
    b, r = torch.randn(N, generator=g).to(dtype) if bias else None, torch.randn(M, N, generator=g).to(dtype) if res else None
    return [None if t is None else t.cuda() for t in (x, q, s, b, r)]


def _check(out, inputs, act, what):
    x, q, s, b, r = [None if t is None else t.cpu() for t in inputs]
    y = (x.double() @ q.double().t()) * s.double() + (0 if b is None else b.double())
    if act != "none":
        y = torch.relu(y) if act == "relu" else \
            torch.nn.functional.gelu(y, approximate="tanh" if act == "gelu_tanh" else "none")
    ref = y if r is None else y + r.double()
    e = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    WORST[x.dtype] = max(WORST.get(x.dtype, 0.0), e)
    print(f"{what}: err {e:.3e} (bound {BOUND[x.dtype]:.3e}); largest so far {x.dtype}: {WORST[x.dtype]:.3e}")
    assert e <= BOUND[x.dtype]


# K edges x split counts, the pipelined loop, N edges; M, dtype and epilogue cycle so that each occurs
SHAPES = [("bn+8", k, ns) for k in ("16", "ks-16", "ks", "ks+16", "2s-16", "2s+16") for ns in (None, 1, 2, 3)] \
    + [("bn+8", "4ks+16", 1), ("bn+8", "8ks", 2), ("3bn+8", "8ks", 1)] \
    + [(n, "ks+16", ns) for n in ("8", "bn-8", "bn", "bn+8", "3bn+8") for ns in (None, 2)]
EPI = [(b, r, a) for b in (False, True) for r in (False, True) for a in ("none", "gelu", "relu", "gelu_tanh")]
CASES = [((BF, FP)[i // 6 % 2], (1, 2, 7, 8, 15, 16)[i % 6], n, k, ns) + EPI[i % 16] for i, (n, k, ns) in enumerate(SHAPES)]


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_matches_float64(case):
    dtype, M, N, K, ns, bias, res, act = case
    N, K = _size(N), _size(K)
    x, q, s, b, r = inputs = _inputs(M, N, K, dtype, bias, res, seed=M + N + K)
    if ns is not None and (ns - 1) * (-(-(-(-K // ns)) // 16) * 16) >= K:
        with pytest.raises(ValueError, match="nsplit"):      # a forced split count that leaves a split empty
            hip.skinny_gemm_w8(x, q, s, b, act, r, nsplit=ns)
        return
    out = hip.skinny_gemm_w8(x, q, s, b, act, r, nsplit=ns)
    assert out.shape == (M, N) and out.dtype == dtype
    _check(out, inputs, act, str(case))


def test_rows_are_independent_and_calls_reproduce():
    x, q, s, b, r = _inputs(16, _size("3bn+8"), _size("2s+16"), BF, seed=3)
    full = hip.skinny_gemm_w8(x, q, s, b, "gelu", r)
    assert torch.equal(full.view(torch.int16), hip.skinny_gemm_w8(x, q, s, b, "gelu", r).view(torch.int16))
    for m in (1, 7):
        part = hip.skinny_gemm_w8(x[:m], q, s, b, "gelu", r[:m].contiguous())
        assert torch.equal(part.view(torch.int16), full[:m].view(torch.int16)), f"row block {m} depends on M"


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ns", [None, 2, 1], ids=["planned", "split2", "fused"])
def test_neighbours_are_neither_read_into_the_result_nor_written(dtype, ns):
    """NaN in the rows of x past M and its columns past K (x is a slice of a wider, taller tensor), rows of -128
    in Wq's allocation past its last, and a guard band around out"""
    M, N, K, pad = 7, _size("bn+8"), _size("2s+16"), 64
    x, q, s, b, r = inputs = _inputs(M, N, K, dtype, seed=5)
    xb = torch.full((16, K + 16), float("nan"), dtype=dtype, device="cuda")
    xb[:M, :K] = x
    qb = torch.full((N + 4, K), -128, dtype=torch.int8, device="cuda")
    qb[:N] = q
    obuf = torch.full((pad + M * N + pad,), 777.0, dtype=dtype, device="cuda")
    og = obuf[pad:pad + M * N].view(M, N)
    assert hip.skinny_gemm_w8(xb[:M, :K], qb[:N], s, b, "relu", r, nsplit=ns, out=og).data_ptr() == og.data_ptr()
    _check(og, inputs, "relu", f"guarded, NaN neighbours, nsplit={ns}")
    assert torch.all(obuf[:pad] == 777.0) and torch.all(obuf[pad + M * N:] == 777.0)
    assert torch.equal(xb[:M, :K], x) and torch.equal(qb[:N], q) and bool((qb[N:] == -128).all())   # inputs unchanged


def test_replays_from_a_captured_graph():
    M, N, K = 8, _size("3bn+8"), _size("2s+16")
    static_x, q, s, b, r = _inputs(M, N, K, BF, seed=9)
    hip.skinny_gemm_w8(static_x, q, s, b, "gelu", r)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = hip.skinny_gemm_w8(static_x, q, s, b, "gelu", r)
    for seed in (10, 11):
        xn = torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).bfloat16().cuda()
        static_x.copy_(xn)
        graph.replay()
        assert torch.equal(static_out.view(torch.int16), hip.skinny_gemm_w8(xn, q, s, b, "gelu", r).view(torch.int16))
    torch.cuda.synchronize()


def _bad(x=(4, 64, BF), wq=(32, 64, torch.int8), scale=(32, torch.float32), t=False):
    mk = lambda *a: torch.ones(*a[:-1], dtype=a[-1], device="cuda")   # noqa: E731
    return dict(x=mk(*x), wq=mk(*wq).t() if t else mk(*wq), scale=mk(*scale))


REJECTED = {"int8 x": dict(x=(4, 64, torch.int8)), "bf16 wq": dict(wq=(32, 64, BF)),
            "K%16": dict(x=(4, 72, BF), wq=(32, 72, torch.int8)), "fp16 scale": dict(scale=(32, FP)),
            "scale shape": dict(scale=(64, torch.float32)), "M=17": dict(x=(17, 64, BF)),
            "non-contiguous wq": dict(wq=(64, 32, torch.int8), t=True)}


@pytest.mark.parametrize("name", list(REJECTED))
def test_bad_arguments_raise_before_any_launch(name, monkeypatch):
    kw = _bad(**REJECTED[name])
    assert not hip.skinny_gemm_w8_supported(**kw)
    monkeypatch.setattr(hip, "_check", lambda rc, what: pytest.fail(f"{what} was launched"))   # reached only after a launch
    with pytest.raises(ValueError):
        hip.skinny_gemm_w8(**kw)


def test_weight_only_linear_records_a_fallback_for_arguments_the_kernel_cannot_take():
    from paddle_hackathon_amd.nn import quant
    x, q, s, b, _ = _inputs(4, 32, 72, BF, res=False)                # K % 16 != 0 at 4 rows on the GPU
    before = fallback.total()
    assert tuple(quant.weight_only_linear(x, q, b, s)._t.shape) == (4, 32) and fallback.total() == before + 1
