"""The MLP's dGELU folded into the fc2 input-gradient GEMM (ops/mlp.py chain 3, "epi2"): the fc1
forward's gemm4p epilogue stores gelu_tanh'(x W1 + b1) (G4P_GELU_DAUX) and the fc2 dgrad's epilogue
multiplies its fp32 accumulators by it (G4P_MULAUX, ops/gemm.mm_nt_mul). Both epilogues against
fp32, on whole and ragged tiles, a one-K-tile product and a grid where every workgroup writes
several tiles; bitwise equal under both main-loop schedules; nothing read into the result or
written outside C; the chain end to end against the fp32 torch MLP and against chain 2; operands the
own kernel does not take. Tolerances are the suite's own (test_gemm4p_gelu_epilogue: 1e-2 of the
reference maximum; test_linear_and_mlp_backward_bias_grads: 1e-2 / 2e-2 norm-relative).
Reference: fused_gemm_epilogue_op.cu:298 (the dgelu epilogue of the fused linear backward)."""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu


def _r(*s, g, dt=torch.bfloat16, lo=-1.0, hi=1.0):
    return (torch.rand(*s, device="cuda", generator=g) * (hi - lo) + lo).to(dt)


def _relmax(got, ref):
    return ((got.float() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("M,N,K,dt", [(512, 1024, 256, torch.bfloat16), (264, 520, 128, torch.bfloat16),
                                      (296, 8, 64, torch.bfloat16), (4096, 8192, 128, torch.bfloat16),
                                      (264, 520, 128, torch.float16)])
def test_mul_epilogue_matches_fp32(M, N, K, dt):
    from paddle_hackathon_amd.ops import gemm as G
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x, wt = _r(M, K, g=g, dt=dt), _r(N, K, g=g, dt=dt)
    aux = _r(M, N, g=g, dt=dt, lo=-1.2, hi=1.2)
    got = G.mm_nt_mul(x, wt, aux)
    assert got is not None and got.shape == (M, N) and got.dtype == dt
    ref = (x.float() @ wt.float().t()) * aux.float()
    err = _relmax(got, ref)
    print(f"mul epilogue {M}x{N}x{K} {dt}: max err / ref max = {err:.3e}")
    assert err < 1e-2, err


@pytest.mark.parametrize("M,N,K", [(512, 1024, 256), (264, 520, 128)])
def test_derivative_aux_matches_autograd(M, N, K):
    from paddle_hackathon_amd.ops import gemm as G
    g = torch.Generator(device="cuda").manual_seed(1)
    x, wt = _r(M, K, g=g), _r(N, K, g=g)
    b = torch.randn(N, device="cuda", generator=g).bfloat16()
    act, d = G.mm_nt_bias_gelu(x, wt, b, deriv=True)
    pre = (x.float() @ wt.float().t() + b.float()).requires_grad_(True)
    ref_act = TF.gelu(pre, approximate="tanh")
    ref_d, = torch.autograd.grad(ref_act.sum(), pre)
    for got, ref, what in ((act, ref_act.detach(), "act"), (d, ref_d, "d")):
        err = _relmax(got, ref)
        print(f"derivative aux {M}x{N}x{K} {what}: max err / ref max = {err:.3e}")
        assert err < 1e-2, (what, err)
    # the activation is the pre-activation build's, bit for bit (same sigmoid, same rounding)
    act0, _ = G.mm_nt_bias_gelu(x, wt, b)
    assert torch.equal(act, act0)


@pytest.mark.parametrize("M,N,K", [(264, 520, 128), (1032, 2056, 512), (2048, 1024, 1024), (296, 8, 64)])
def test_schedule_independence_bitwise(M, N, K, monkeypatch):
    from paddle_hackathon_amd.ops import gemm as G
    g = torch.Generator(device="cuda").manual_seed(5)
    a, bt = _r(M, K, g=g), _r(N, K, g=g)
    bias = torch.randn(N, device="cuda", generator=g)
    aux = _r(M, N, g=g, lo=-1.2, hi=1.2)
    res = []
    for early in ("0", "1"):
        monkeypatch.setenv("PHA_G4P_EARLY", early)
        d = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        act = G.gemm_p(a, bt, bias=bias, gelu_aux=d, gelu_deriv=True)
        res.append((G.mm_nt_mul(a, bt, aux), act, d))
    for t0, t1, what in zip(res[0], res[1], ("mul", "act", "d")):
        assert torch.equal(t0, t1), (what, (t0.float() - t1.float()).abs().max().item())
    ref = (a.float() @ bt.float().t()) * aux.float()
    assert _relmax(res[1][0], ref) < 1e-2


@pytest.mark.parametrize("early", ["0", "1"])
def test_nothing_written_or_read_outside_c(early, monkeypatch):
    """C and aux as interior views of sentinel-filled buffers at the ragged shape: the frame around C
    keeps the sentinel (rows past M and the partial last column group are not written), and the
    result does not depend on what surrounds aux (nothing outside it is read into the product)"""
    from paddle_hackathon_amd.ops import gemm as G
    monkeypatch.setenv("PHA_G4P_EARLY", early)
    M, N, K = 264, 520, 128
    g = torch.Generator(device="cuda").manual_seed(11)
    a, bt = _r(M, K, g=g), _r(N, K, g=g)
    bias = torch.randn(N, device="cuda", generator=g)
    aux = _r(M, N, g=g, lo=-1.2, hi=1.2)
    R0, C0, RT, CT = 8, 16, M + 24, N + 40   # frame: 8 rows above / 16 below, 16 columns left / 24 right

    def framed(fill, inner=None):
        buf = torch.full((RT, CT), fill, dtype=torch.bfloat16, device="cuda")
        view = buf[R0:R0 + M, C0:C0 + N]
        if inner is not None:
            view.copy_(inner)
        return buf, view

    def frame_intact(buf, fill):
        chk = buf.clone()
        chk[R0:R0 + M, C0:C0 + N] = fill
        return bool((chk == fill).all())

    SENT = -777.0
    # the multiply: aux inside a frame of huge values, C inside a frame of sentinels
    _, aux_v = framed(3.0e38, aux)
    cbuf, c_v = framed(SENT)
    out = G.mm_nt_mul(a, bt, aux_v, out=c_v)
    assert out is not None and out.data_ptr() == c_v.data_ptr()
    assert frame_intact(cbuf, SENT)
    assert torch.equal(c_v, G.mm_nt_mul(a, bt, aux))
    # the derivative aux: both outputs inside sentinel frames
    cbuf, c_v = framed(SENT)
    dbuf, d_v = framed(SENT)
    G.gemm_p(a, bt, bias=bias, out=c_v, gelu_aux=d_v, gelu_deriv=True)
    assert frame_intact(cbuf, SENT) and frame_intact(dbuf, SENT)
    d = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    act = G.gemm_p(a, bt, bias=bias, gelu_aux=d, gelu_deriv=True)
    assert torch.equal(c_v, act) and torch.equal(d_v, d)


def _mlp_case(tokens, H, F, H2, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = _r(tokens, H, g=g)
    w1, w2 = _r(H, F, g=g) * 0.03, _r(F, H2, g=g) * 0.03
    b1, b2 = _r(F, g=g) * 0.1, _r(H2, g=g) * 0.1
    gy = _r(tokens, H2, g=g)
    xs = [t.float().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    yr = TF.gelu(xs[0] @ xs[1] + xs[2], approximate="tanh") @ xs[3] + xs[4]
    yr.backward(gy.float())
    return (x, w1, b1, w2, b2), gy, yr.detach(), [t.grad for t in xs]


def _run_chain(chain, ts, gy, monkeypatch):
    """-> (output, gradients) of fused_mlp under PHA_FUSED_MLP=chain"""
    from paddle_hackathon_amd.ops import mlp
    monkeypatch.setenv("PHA_FUSED_MLP", chain)
    leaves = [t.detach().clone().requires_grad_(True) for t in ts]
    y = mlp.fused_mlp(*leaves)
    y.backward(gy)
    return y.detach(), [t.grad for t in leaves]


def _nrel(got, ref):
    return ((got.float() - ref).norm() / ref.norm()).item()


def test_chain3_end_to_end(monkeypatch):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import gemm as G
    paddle.set_device("gpu")
    try:
        ts, gy, yr, refs = _mlp_case(2048, 1024, 4096, 1024, 7)
        calls = []
        real = G.mm_nt_mul
        monkeypatch.setattr(G, "mm_nt_mul", lambda *a, **k: calls.append(1) or real(*a, **k))
        y3, g3 = _run_chain("epi2", ts, gy, monkeypatch)
        assert calls, "chain 3 did not reach the multiply epilogue"
        y2, g2 = _run_chain("epi", ts, gy, monkeypatch)
        assert len(calls) == 1, "chain 2 took the multiply epilogue"
        assert _nrel(y3, yr) < 1e-2
        assert torch.equal(y3, y2)   # the forward activation is the same in both chains
        for name, a3, a2, ref in zip(("dx", "dw1", "db1", "dw2", "db2"), g3, g2, refs):
            e3, e2 = _nrel(a3, ref), _nrel(a2, ref)
            print(f"{name}: chain 3 {e3:.3e}  chain 2 {e2:.3e}")
            assert e3 < 2e-2, (name, e3)
            assert e3 <= 1.25 * e2, (name, e3, e2)
    finally:
        paddle.set_device("cpu")


def test_unsupported_operands_take_the_old_route(monkeypatch):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import gemm as G
    g = torch.Generator(device="cuda").manual_seed(3)
    # K = 200 (not a multiple of 64): the own kernel does not take the product
    assert G.mm_nt_mul(_r(512, 200, g=g), _r(512, 200, g=g), _r(512, 512, g=g)) is None
    paddle.set_device("gpu")
    try:
        # an MLP whose output width (the fc2 dgrad's K) is 200: chain 3 runs it as chain 2
        ts, gy, yr, refs = _mlp_case(512, 256, 512, 200, 9)
        y3, g3 = _run_chain("epi2", ts, gy, monkeypatch)
        y2, g2 = _run_chain("epi", ts, gy, monkeypatch)
        assert _nrel(y3, yr) < 1e-2
        for name, a3, a2, ref in zip(("dx", "dw1", "db1", "dw2", "db2"), g3, g2, refs):
            assert _nrel(a3, ref) < 2e-2, name
            assert torch.equal(a3, a2), name
    finally:
        paddle.set_device("cpu")
