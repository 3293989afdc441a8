"""The weight-streaming GEMM for 1 <= M <= 16 rows (csrc/kernels/skinny_gemm.hip) against float64.

Reference: float64 on the CPU from the same rounded inputs, act(x @ W + b) + r. Error is
max|out - ref| / max|ref|; bound 2^-8 for bf16 and 2^-10 for fp16, one ulp of the largest element (the
rule of tests/test_decode_attn_gpu.py). The kernel accumulates in fp32 and rounds once, so half of
that is the expected size.

Shapes are the smallest at which each mechanism can go wrong, taken from the kernel's exported column
tile, K step and split plan: K around one K step and around the seam between two splits, N around
one column tile and past three, every M class, the split count planned and forced to 1, 2 and 3.

Largest errors seen on an MI355X over this file: bf16 3.551e-03, fp16 4.357e-04
(profiles/decode_gemm/README.md)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
WORST = {}


def _hip():
    from paddle_hackathon_amd.ops import hip
    return hip


def _sizes(nk):
    """the symbolic K and N values of a layout: K step, column tile and planned k_per_split"""
    hip = _hip()
    bn, ks = hip.skinny_gemm_tile(nk)
    _, kps = hip.skinny_gemm_plan(bn, 2 * ks, nk)
    K = {"8": 8, "ks-8": ks - 8, "ks": ks, "ks+8": ks + 8, "2s-8": 2 * kps - 8, "2s+8": 2 * kps + 8}
    N = {"8": 8, "bn-8": bn - 8, "bn": bn, "bn+8": bn + 8, "3bn+8": 3 * bn + 8}
    return K, N


def _inputs(M, N, K, nk, dtype, bias, res, seed=0):
    """CPU tensors rounded to dtype; outputs O(1), bias and residual as large as the product"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn((N, K) if nk else (K, N), generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, generator=g).to(dtype) if bias else None
    r = torch.randn(M, N, generator=g).to(dtype) if res else None
    return x, w, b, r


def _ref(x, w, nk, b, act, r):
    y = x.double() @ (w.double().t() if nk else w.double())
    if b is not None:
        y = y + b.double()
    if act == "gelu":
        y = torch.nn.functional.gelu(y)
    elif act == "relu":
        y = torch.relu(y)
    if r is not None:
        y = y + r.double()
    return y


def _err(out, ref, dtype, what):
    e = ((out.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    WORST[dtype] = max(WORST.get(dtype, 0.0), e)
    print(f"{what}: err {e:.3e} (bound {BOUND[dtype]:.3e}); largest so far {dtype}: {WORST[dtype]:.3e}")
    return e


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _cases():
    Ms, Ks, Ns = [1, 2, 7, 8, 15, 16], ["8", "ks-8", "ks", "ks+8", "2s-8", "2s+8"], ["8", "bn-8", "bn", "bn+8", "3bn+8"]
    splits, acts = [None, 1, 2, 3], ["none", "gelu", "relu"]
    dts = [torch.bfloat16, torch.float16]
    out, n = [], itertools.count()
    for nk in (True, False):
        for k, ns in itertools.product(Ks, splits):            # K edges x split counts
            i = next(n)
            out.append((nk, dts[i % 2], Ms[i % 6], Ns[i % 5], k, ns, i % 2 == 0, i % 3 == 0, acts[i % 3]))
        for nn, ns in itertools.product(Ns, (None, 2)):        # N edges
            i = next(n)
            out.append((nk, dts[i % 2], Ms[i % 6], nn, "ks+8", ns, i % 2 == 1, i % 3 == 1, acts[i % 3]))
        for m, dt in itertools.product(Ms, dts):               # every M class in both dtypes
            i = next(n)
            out.append((nk, dt, m, "bn+8", "2s+8", splits[i % 4], True, True, acts[i % 3]))
        for (b, r), a in itertools.product([(0, 0), (1, 0), (0, 1), (1, 1)], acts):   # every epilogue
            i = next(n)
            out.append((nk, dts[i % 2], 8, "bn+8", "ks+8", (None, 2)[i % 2], bool(b), bool(r), a))
    return out


def _id(c):
    nk, dt, M, N, K, ns, b, r, a = c
    return (f"{'nk' if nk else 'kn'}-{'bf16' if dt is torch.bfloat16 else 'fp16'}-M{M}-N{N}-K{K}-s{ns}-"
            f"{'b' if b else ''}{'r' if r else ''}{a}")


CASES = _cases()
assert len(CASES) <= 150


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_matches_float64(case):
    hip = _hip()
    nk, dtype, M, Nsym, Ksym, ns, bias, res, act = case
    Kd, Nd = _sizes(nk)
    N, K = Nd[Nsym], Kd[Ksym]
    x, w, b, r = _inputs(M, N, K, nk, dtype, bias, res, seed=M + N + K)
    xg, wg, bg, rg = _cuda(x, w, b, r)
    if ns is not None and (ns - 1) * (-(-(-(-K // ns)) // 8) * 8) >= K:
        with pytest.raises(ValueError, match="nsplit"):      # a forced split count that leaves a split empty
            hip.skinny_gemm(xg, wg, nk, bg, act, rg, nsplit=ns)
        return
    out = hip.skinny_gemm(xg, wg, nk, bg, act, rg, nsplit=ns)
    assert out.shape == (M, N) and out.dtype == dtype
    assert _err(out, _ref(x, w, nk, b, act, r), dtype, _id(case)) <= BOUND[dtype]


@pytest.mark.parametrize("nk", [True, False], ids=["nk", "kn"])
def test_rows_are_independent_and_calls_reproduce(nk):
    hip = _hip()
    Kd, Nd = _sizes(nk)
    N, K = Nd["3bn+8"], Kd["2s+8"]
    x, w, b, r = _inputs(16, N, K, nk, torch.bfloat16, True, True, seed=3)
    xg, wg, bg, rg = _cuda(x, w, b, r)
    full = hip.skinny_gemm(xg, wg, nk, bg, "gelu", rg)
    again = hip.skinny_gemm(xg, wg, nk, bg, "gelu", rg)
    assert torch.equal(full.view(torch.int16), again.view(torch.int16))           # two calls: bitwise equal
    assert _err(full, _ref(x, w, nk, b, "gelu", r), torch.bfloat16, "M=16") <= BOUND[torch.bfloat16]
    for m in (1, 7):
        part = hip.skinny_gemm(xg[:m], wg, nk, bg, "gelu", rg[:m].contiguous())
        assert torch.equal(part.view(torch.int16), full[:m].view(torch.int16)), f"row block {m} depends on M"


@pytest.mark.parametrize("nk", [True, False], ids=["nk", "kn"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_tails_are_masked_not_read_into_the_result(nk, dtype):
    """NaN in every neighbour the kernel could over-read: the rows of x past M and its columns past K
    (x is a slice of a wider, taller tensor) and the rows of W's allocation past its last"""
    hip = _hip()
    Kd, Nd = _sizes(nk)
    M, N, K = 7, Nd["bn+8"], Kd["ks+8"]
    x, w, b, r = _inputs(M, N, K, nk, dtype, True, True, seed=5)
    xb = torch.full((16, K + 8), float("nan"), dtype=dtype, device="cuda")
    xb[:M, :K] = x.cuda()
    rows = N if nk else K
    wb = torch.full((rows + 4, w.shape[1]), float("nan"), dtype=dtype, device="cuda")
    wb[:rows] = w.cuda()
    xg, wg = xb[:M, :K], wb[:rows]
    assert xg.stride(0) == K + 8 and wg.is_contiguous()
    for ns in (None, 2):
        out = hip.skinny_gemm(xg, wg, nk, b.cuda(), "none", r.cuda(), nsplit=ns)
        assert torch.isfinite(out).all()
        assert _err(out, _ref(x, w, nk, b, "none", r), dtype, f"NaN neighbours nsplit={ns}") <= BOUND[dtype]
    # a W sliced out of a wider parent is not contiguous: rejected, not read
    wide = torch.full((w.shape[0], w.shape[1] + 8), float("nan"), dtype=dtype, device="cuda")
    wide[:, :w.shape[1]] = w.cuda()
    with pytest.raises(ValueError, match="w "):
        hip.skinny_gemm(x.cuda(), wide[:, :w.shape[1]], nk)


@pytest.mark.parametrize("nk", [True, False], ids=["nk", "kn"])
@pytest.mark.parametrize("ns", [None, 1], ids=["planned", "fused"])
def test_nothing_outside_out_changes_and_inputs_are_unchanged(nk, ns):
    hip = _hip()
    Kd, Nd = _sizes(nk)
    M, N, K, dtype, pad = 7, Nd["bn+8"], Kd["2s+8"], torch.bfloat16, 64
    x, w, b, r = _inputs(M, N, K, nk, dtype, True, True, seed=6)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    obuf = torch.full((pad + M * N + pad,), 777.0, dtype=dtype, device="cuda")
    rbuf = torch.full((pad + M * N + pad,), 555.0, dtype=dtype, device="cuda")
    rg = rbuf[pad:pad + M * N].view(M, N)
    rg.copy_(r)
    og = obuf[pad:pad + M * N].view(M, N)
    x0, r0 = xg.clone(), rbuf.clone()
    ret = hip.skinny_gemm(xg, wg, nk, bg, "relu", rg, nsplit=ns, out=og)
    assert ret.data_ptr() == og.data_ptr()
    assert _err(og, _ref(x, w, nk, b, "relu", r), dtype, "guarded out") <= BOUND[dtype]
    assert torch.all(obuf[:pad] == 777.0) and torch.all(obuf[pad + M * N:] == 777.0)
    assert torch.equal(rbuf.view(torch.int16), r0.view(torch.int16))
    assert torch.equal(xg.view(torch.int16), x0.view(torch.int16))


@pytest.mark.parametrize("nk", [True, False], ids=["nk", "kn"])
def test_strided_x_equals_its_contiguous_copy(nk):
    hip = _hip()
    Kd, Nd = _sizes(nk)
    M, N, K = 8, Nd["bn+8"], Kd["ks+8"]
    x, w, _, _ = _inputs(M, N, K, nk, torch.bfloat16, False, False, seed=7)
    wide = torch.randn(M, K + 24, generator=torch.Generator().manual_seed(8)).bfloat16().cuda()
    wide[:, 8:8 + K] = x.cuda()
    xs = wide[:, 8:8 + K]                                    # stride(0) = K + 24, offset 16 bytes
    assert xs.stride(0) == K + 24 and not xs.is_contiguous() and xs.data_ptr() % 16 == 0
    a = hip.skinny_gemm(xs, w.cuda(), nk)
    c = hip.skinny_gemm(xs.contiguous(), w.cuda(), nk)
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    assert _err(a, _ref(x, w, nk, None, "none", None), torch.bfloat16, "strided x") <= BOUND[torch.bfloat16]


@pytest.mark.parametrize("nk", [True, False], ids=["nk", "kn"])
def test_replays_from_a_captured_graph(nk):
    hip = _hip()
    Kd, Nd = _sizes(nk)
    M, N, K = 8, Nd["3bn+8"], Kd["2s+8"]
    x, w, b, r = _inputs(M, N, K, nk, torch.bfloat16, True, True, seed=9)
    wg, bg, rg = _cuda(w, b, r)
    static_x = x.cuda()
    hip.skinny_gemm(static_x, wg, nk, bg, "gelu", rg)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = hip.skinny_gemm(static_x, wg, nk, bg, "gelu", rg)
    for seed in (10, 11):
        xn = torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).bfloat16().cuda()
        static_x.copy_(xn)
        graph.replay()
        got = static_out.clone()
        eager = hip.skinny_gemm(xn, wg, nk, bg, "gelu", rg)
        assert torch.equal(got.view(torch.int16), eager.view(torch.int16))
    torch.cuda.synchronize()


def _reject_cases():
    bf, dev = torch.bfloat16, "cuda"

    def t(*shape, dtype=bf, device=dev):
        return torch.ones(*shape, dtype=dtype, device=device)

    return {
        "M=0": lambda: dict(x=t(0, 64), w=t(64, 32)),
        "M=17": lambda: dict(x=t(17, 64), w=t(64, 32)),
        "K%8": lambda: dict(x=t(4, 60), w=t(60, 32)),
        "N%8": lambda: dict(x=t(4, 64), w=t(64, 36)),
        "fp32": lambda: dict(x=t(4, 64, dtype=torch.float32), w=t(64, 32, dtype=torch.float32)),
        "mixed dtypes": lambda: dict(x=t(4, 64), w=t(64, 32, dtype=torch.float16)),
        "cpu x": lambda: dict(x=t(4, 64, device="cpu"), w=t(64, 32)),
        "cpu w": lambda: dict(x=t(4, 64), w=t(64, 32, device="cpu")),
        "misaligned x": lambda: dict(x=t(4 * 64 + 8)[1:1 + 4 * 64].view(4, 64), w=t(64, 32)),
        "misaligned w": lambda: dict(x=t(4, 64), w=t(64 * 32 + 8)[1:1 + 64 * 32].view(64, 32)),
        "non-contiguous w": lambda: dict(x=t(4, 64), w=t(32, 64).t()),
        "bias shape": lambda: dict(x=t(4, 64), w=t(64, 32), bias=t(64)),
        "bias 2-D": lambda: dict(x=t(4, 64), w=t(64, 32), bias=t(1, 32)),
        "residual shape": lambda: dict(x=t(4, 64), w=t(64, 32), residual=t(4, 64)),
        "residual non-contiguous": lambda: dict(x=t(4, 64), w=t(64, 32), residual=t(32, 4).t()),
        "x row stride": lambda: dict(x=t(4, 68)[:, :64], w=t(64, 32)),
        "act": lambda: dict(x=t(4, 64), w=t(64, 32), act="tanh"),
        "empty split": lambda: dict(x=t(4, 64), w=t(64, 32), nsplit=9),
        "nsplit=0": lambda: dict(x=t(4, 64), w=t(64, 32), nsplit=0),
    }


@pytest.mark.parametrize("name", list(_reject_cases()))
def test_bad_arguments_raise_before_any_launch(name, monkeypatch):
    hip = _hip()
    kw = _reject_cases()[name]()
    launched = []
    monkeypatch.setattr(hip, "_check", lambda rc, what: launched.append(what))   # reached only after a launch
    with pytest.raises(ValueError):
        hip.skinny_gemm(kw.pop("x"), kw.pop("w"), False, **kw)
    assert not launched
    if name not in ("act", "empty split", "nsplit=0"):
        kw2 = _reject_cases()[name]()
        assert not hip.skinny_gemm_supported(kw2["x"], kw2["w"], False, kw2.get("bias"), kw2.get("residual"))


def test_plan_depends_on_shape_and_layout_alone():
    hip = _hip()
    for nk in (True, False):
        bn, ks = hip.skinny_gemm_tile(nk)
        assert bn % 16 == 0 and ks % 32 == 0
        for N, K in ((2048, 2048), (6144, 2048), (8192, 2048), (2048, 8192), (8, 8), (bn + 8, ks + 8)):
            ns, kps = hip.skinny_gemm_plan(N, K, nk)
            assert (ns, kps) == hip.skinny_gemm_plan(N, K, nk)
            assert ns >= 1 and kps % 8 == 0 and (ns - 1) * kps < K <= ns * kps
    assert hip.SKINNY_GEMM_MAX_M == 16
