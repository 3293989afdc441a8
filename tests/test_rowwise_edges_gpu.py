"""The row-wise HIP kernels (csrc/kernels/norm_softmax.hip, ce_gelu_embed.hip) at their edge widths,
row counts and values, against the float64 references of rowwise_reference.py (GPU only).

Widths: one per register-chunk class NCH = ceil(H / 512) -> {1, 2, 3, 4, 6, 8} (softmax also 12, 16)
at the class's tail shape. The ops/hip.py wrappers are called directly, so no fallback can satisfy a
test; the public ops functions are used only where a test says so.

Bound of every output against float64 (``check``), as the issue sets it: one rounding of the stored
dtype on |ref|, plus an fp32-arithmetic term — the error of torch's own fp32 op on the same inputs,
measured in the test, times MARGIN (the kernels sum in another order and use v_exp / v_rcp instead
of libm), scaled by the largest |ref| of the row (of the whole vector for per-row and per-column
outputs). Five named relaxations exist (RELAX) and apply only at the call sites that pass them; every
check prints its ratio under the unrelaxed bound as well, and the module's teardown lists, per kernel,
the worst ratio under both and how many checks needed their relaxation. Column sums of a stored
gradient (dx_colsum, dbias, db of bias-GELU) are judged against the float64 column sums of that
stored tensor, as the kernels define them. Exactness claims use torch.equal."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

import rowwise_reference as R

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DTYPES = [F32, BF16, F16]
LN_DTYPES = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)]   # (activation, weight)
WIDTHS = [8, 520, 1536, 2056, 2568, 3080, 4096]          # NCH 1, 2, 3, 6 (masked), 6, 8 (from 7), 8
SOFTMAX_WIDTHS = WIDTHS + [4104, 6144, 6152, 8192]       # NCH 12 (from 9), 12, 16 (from 13), 16
STRIDED = [(4100, 64), (4100, 2056)]   # past the backward's grid cap: 256 blocks x 16 waves, 512 x 8
EPS = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}
RELAX = {
    # torch's fp32 result is exact (sums of a few 16-bit values, one-row sums): the kernel's other order
    # of the same additions is held to one fp32 rounding of the scale instead of to none
    "zero32": "torch's fp32 error is exactly 0",
    # fp16 outputs below 2^-14 are subnormal: their rounding step is 2^-24 whatever |ref| is
    "f16sub": "fp16 subnormal rounding, 2^-25",
    # dx = y (dy - sum(y dy)): the sum cancels (a row with two finite entries gives dx of the order of
    # the smaller y), so the fp32 error of both torch and the kernel is relative to sum |y dy|
    "sumscale": "fp32 term relative to the magnitude of what was summed",
    # a case of ONE row: torch's error on it is a single draw, at times a fraction of one fp32 rounding of
    # the scale (measured: 9e-9 to 2e-8 where the kernel's own single draw is 4e-8 to 2e-7). It is floored
    # at 2^-24 there, so the kernel is held to 4 fp32 roundings of the scale. Five cases of rows = 1 need
    # it: softmax_fwd 1x8 fp32 (1.50 x the unrelaxed bound), softmax_bwd 1x4096 fp32 +1e4 (1.31) and
    # 1x4104 fp32 -inf (2.25), softmax_ce_bwd 1x2049 fp32 label on -inf (1.48), softmax_ce_fwd 1x2056
    # bf16 loss (1.05). The cases of 5 and 9 rows run without it.
    "onerow": "single-row sample of torch's error floored at 2^-24",
    # torch's own 16-bit softmax backward (the fallback) rounds intermediates to the dtype
    "eps_scale": "dtype rounding on the row scale (torch's 16-bit kernel)",
}
MARGIN = 4.0
LN_EPS = float(torch.tensor(1e-5, dtype=F32))            # the eps the kernels get (an fp32 argument)
INF = math.inf
_WORST, _STRICT, _NEEDED = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _native():
    from paddle_hackathon_amd.ops import _lib
    assert _lib.native_available(), "libpha_kernels.so must be loaded on a GPU run"
    yield
    for k in sorted(_WORST):   # (-s) worst error / bound per kernel: with its named relaxations, and under the issue's bound
        print(f"worst ratio {k:20s} {_WORST[k][0]:.3f} ({_WORST[k][1]}); unrelaxed {_STRICT[k][0]:.3f} "
              f"({_STRICT[k][1]}), {_NEEDED.get(k, 0)} checks over 1")


def _name(dt):
    return str(dt).replace("torch.", "")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(*shape, seed=0):
    return torch.randn(*shape, device="cuda", generator=_gen(seed))


def _rand(*shape, seed=0):
    return torch.rand(*shape, device="cuda", generator=_gen(seed))


def _worse(table, kernel, ratio, what):
    if ratio > table.setdefault(kernel, (0.0, ""))[0]:
        table[kernel] = (ratio, what)


def check(kernel, what, out, ref, t32, dt=None, relax=(), scale=None):
    """out (the kernel's) against ref (float64) within one rounding of dt plus MARGIN times the
    measured error of t32 (torch's fp32 result); non-finite ref entries must match exactly.
    relax: names from RELAX that this call site may use; scale: the magnitude for "sumscale" /
    "eps_scale". The ratio under the issue's bound (no relaxation) is computed and printed always."""
    dt = dt or out.dtype
    assert out.dtype == dt and out.shape == ref.shape and t32.shape == ref.shape, (kernel, what)
    assert all(r in RELAX for r in relax)
    o, t = out.double(), t32.double()
    fin = torch.isfinite(ref)
    assert torch.equal(o[~fin], ref[~fin]), f"{kernel} {what}: non-finite entries differ"
    assert torch.isfinite(o[fin]).all(), f"{kernel} {what}: NaN or inf where the reference is finite"
    zero = torch.zeros_like(ref)
    mag = torch.where(fin, ref.abs(), zero)
    err = torch.where(fin, (o - ref).abs(), zero)
    terr = torch.where(fin, (t - ref).abs(), zero)
    rowmax = (mag.amax(-1, keepdim=True) if ref.dim() >= 2 else mag.max()).expand_as(ref)

    def ratio_of(sc, names):
        e32 = float(torch.where(sc > 0, terr / sc.clamp_min(1e-300), zero).max())
        assert math.isfinite(e32), f"{kernel} {what}: torch's fp32 result is not finite"
        if "zero32" in names and e32 == 0.0:
            e32 = EPS[F32]
        if "onerow" in names:
            assert ref.numel() == ref.shape[-1]
            e32 = max(e32, EPS[F32])
        bound = EPS[dt] * (sc if "eps_scale" in names else mag) + MARGIN * e32 * sc
        if "f16sub" in names and dt == F16:
            bound = bound + 2.0 ** -25
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, zero + INF, zero))
        return float(r.max()), e32, float(bound.max())

    strict, e32, bmax = ratio_of(rowmax, ())
    ratio = strict
    if relax:
        sc = scale.expand_as(ref) if (scale is not None and ("sumscale" in relax or "eps_scale" in relax)) else rowmax
        ratio, _, bmax = ratio_of(sc, relax)
    _worse(_WORST, kernel, ratio, what)
    _worse(_STRICT, kernel, strict, what)
    if strict > 1.0:
        _NEEDED[kernel] = _NEEDED.get(kernel, 0) + 1
    print(f"{kernel:20s} {what:46s} err {float(err.max()):.3e} bound {bmax:.3e} fp32-op {e32:.2e} "
          f"ratio {ratio:.3f} unrelaxed {strict:.3f} {','.join(relax)}")
    assert ratio <= 1.0, f"{kernel} {what}: error / bound = {ratio:.3f} (unrelaxed {strict:.3f})"


# ------------------------------------------------------------------------------------------------
# LayerNorm forward
# ------------------------------------------------------------------------------------------------
def _ln_params(H, wdt, seed):
    return (_rand(H, seed=seed + 1) + 0.5).to(wdt), _randn(H, seed=seed + 2).to(wdt)


def _ln_fwd_check(kernel, what, x, w, b, y, mean, rstd):
    H = x.shape[-1]
    ry, rm, rr = R.layer_norm(x, w, b, LN_EPS)
    xf = x.float()
    ty = TF.layer_norm(xf, [H], w.float(), None if b is None else b.float(), 1e-5)
    check(kernel, what + " y", y, ry, ty)
    check(kernel, what + " mean", mean, rm, xf.mean(-1), F32)
    check(kernel, what + " rstd", rstd, rr, torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5), F32)
    return rr


@pytest.mark.parametrize("dt,wdt", LN_DTYPES, ids=lambda d: _name(d))
@pytest.mark.parametrize("H", WIDTHS)
def test_layer_norm_fwd(H, dt, wdt):
    """y, mean and rstd on randn, on 1000 + randn (cancellation in the variance) and with one constant
    row: 3.0, whose row sum is exact in fp32 at every width here, so its mean is exact, rstd =
    1 / sqrt(eps) up to the rounding of eps and of the reciprocal square root, and y == b exactly."""
    from paddle_hackathon_amd.ops import hip
    rows = 5
    w, b = _ln_params(H, wdt, H)
    tag = f"H={H} {_name(dt)}/{_name(wdt)}"
    for kind in ("randn", "offset", "const"):
        x = _randn(rows, H, seed=H)
        if kind == "offset":
            x = x + 1000.0
        x = x.to(dt)
        if kind == "const":
            x[2] = 3.0
        y, mean, rstd = hip.layer_norm_fwd(x, w, b, 1e-5)
        _ln_fwd_check("ln_fwd", f"{tag} {kind}", x, w, b, y, mean, rstd)
        if kind == "const":
            want = 1.0 / math.sqrt(LN_EPS)
            assert float(mean[2]) == 3.0
            assert abs(float(rstd[2]) - want) <= 4 * EPS[F32] * want
            assert torch.equal(y[2], b.to(dt))


@pytest.mark.parametrize("dt,wdt", LN_DTYPES, ids=lambda d: _name(d))
def test_layer_norm_fwd_no_bias(dt, wdt):
    from paddle_hackathon_amd.ops import hip
    H = 520
    w, _ = _ln_params(H, wdt, 7)
    x = _randn(5, H, seed=7).to(dt)
    y, mean, rstd = hip.layer_norm_fwd(x, w, None, 1e-5)
    _ln_fwd_check("ln_fwd", f"H={H} {_name(dt)}/{_name(wdt)} b=None", x, w, None, y, mean, rstd)


@pytest.mark.parametrize("i,H", list(enumerate(WIDTHS)))
def test_layer_norm_fwd_residual(i, H):
    """the fused residual add: hs is x + r rounded to the dtype, bitwise, and y = LN(hs)"""
    from paddle_hackathon_amd.ops import hip
    dt, wdt = LN_DTYPES[i % len(LN_DTYPES)]
    w, b = _ln_params(H, wdt, H)
    x, r = _randn(5, H, seed=H).to(dt), _randn(5, H, seed=H + 9).to(dt)
    y, mean, rstd, hs = hip.layer_norm_fwd(x, w, b, 1e-5, residual=r)
    assert torch.equal(hs, x + r)
    _ln_fwd_check("ln_fwd", f"H={H} {_name(dt)}/{_name(wdt)} residual", hs, w, b, y, mean, rstd)


# ------------------------------------------------------------------------------------------------
# LayerNorm backward
# ------------------------------------------------------------------------------------------------
def _ln_bwd_case(rows, H, dt, wdt, variants="ABCD"):
    """the backward judged alone: mean / rstd are the float64 statistics cast to fp32 (the reference
    is given the same two vectors). A: plain; B: dres, no bias gradient; C: dres and dx_colsum in
    fp32; D: dx_colsum in the activation dtype."""
    from paddle_hackathon_amd.ops import hip
    tag = f"{rows}x{H} {_name(dt)}/{_name(wdt)}"
    w, _ = _ln_params(H, wdt, H)
    x, dy = _randn(rows, H, seed=H).to(dt), _randn(rows, H, seed=H + 3).to(dt)
    dres = _randn(rows, H, seed=H + 4).to(dt)
    _, m64, r64 = R.layer_norm(x, w, None, LN_EPS)
    mean, rstd = m64.float(), r64.float()
    xt, wt = x.float().requires_grad_(True), w.float().requires_grad_(True)
    bt = torch.zeros(H, device="cuda", requires_grad=True)
    TF.layer_norm(xt, [H], wt, bt, 1e-5).backward(dy.float())
    for v in variants:
        use_dres = v in "BC"
        d = dres if use_dres else None
        kw = {"C": dict(dx_colsum=F32), "D": dict(dx_colsum=dt)}.get(v, {})
        res = hip.layer_norm_bwd(dy, x, w, mean, rstd, v != "B", dres=d, **kw)
        rdx, rdw, rdb, rdxs = R.layer_norm_bwd(dy, x, w, d, mean=mean, rstd=rstd)
        check("ln_bwd", f"{tag} {v} dx", res[0], rdx, xt.grad + dres.float() if use_dres else xt.grad)
        check("ln_bwd", f"{tag} {v} dw", res[1], rdw, wt.grad)
        if v == "B":
            assert res[2] is None
        else:
            check("ln_bwd", f"{tag} {v} db", res[2], rdb, bt.grad, relax=("zero32",))
        if kw:   # the column sums of the stored (rounded) dx; in fp32 nothing is rounded: the reference's own
            check("ln_bwd", f"{tag} {v} dx_colsum", res[3], R.col_sum(res[0]), res[0].float().sum(0), kw["dx_colsum"],
                  relax=("zero32",))
            if dt == F32:
                check("ln_bwd", f"{tag} {v} dx_colsum/ref", res[3], rdxs, (xt.grad + dres.float() if use_dres else xt.grad).sum(0))
        else:
            assert len(res) == 3


@pytest.mark.parametrize("dt,wdt", LN_DTYPES, ids=lambda d: _name(d))
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("rows", [1, 17])
def test_layer_norm_bwd(rows, H, dt, wdt):
    """one row, and two blocks with the second nearly empty (17 = 16 + 1 or 2 x 8 + 1 waves)"""
    _ln_bwd_case(rows, H, dt, wdt)


@pytest.mark.parametrize("dt,wdt", [(F32, F32), (BF16, F32)], ids=lambda d: _name(d))
@pytest.mark.parametrize("rows,H", STRIDED)
def test_layer_norm_bwd_grid_stride(rows, H, dt, wdt):
    """the generic branch's row loop past the block cap: 4096 rows fill the grid, 4 more stride"""
    from paddle_hackathon_amd.ops import _lib
    bw = 16 if H <= 1536 else 8
    assert _lib.loaded().pha_layer_norm_bwd_nblocks(rows, H) * bw < rows
    _ln_bwd_case(rows, H, dt, wdt, "AC")


# ------------------------------------------------------------------------------------------------
# bias + dropout + residual + LayerNorm: the three kernels regenerate one mask
# ------------------------------------------------------------------------------------------------
def _dropout_case(rows, H, p, dt, stats):
    from paddle_hackathon_amd.ops import hip
    thresh, kscale, seed = int(round(p * 65536)), 1.0 / (1.0 - p), 12345 + H
    tag = f"{rows}x{H} {_name(dt)} p={p}"
    w, b = _ln_params(H, F32, H)
    ksf = torch.tensor(kscale, dtype=F32, device="cuda")
    one, zero = torch.ones(rows, H, device="cuda", dtype=dt), torch.zeros(rows, H, device="cuda", dtype=dt)
    # forward on ones: hs is the keep pattern times kscale
    _, _, _, hs1 = hip.bdrln_fwd(one, None, zero, w, b, 1e-5, seed, thresh, kscale)
    keep = hs1 != 0
    kd = keep.to(dt)
    assert torch.equal(hs1, kd * ksf.to(dt))
    dx1, db1 = hip.dropout_bias_bwd(one, seed, thresh, kscale)
    assert db1 is None and torch.equal(dx1, hs1)
    if stats:
        n, q = keep.numel(), 1.0 - thresh / 65536.0
        assert n >= 200000
        frac = float(keep.double().mean())
        print(f"{tag}: kept {frac:.6f} of {n}, expected {q:.6f} +- {4 * math.sqrt(q * (1 - q) / n):.6f}")
        assert abs(frac - q) <= 4.0 * math.sqrt(q * (1.0 - q) / n)
    # forward on data: hs = r + dropout(x + xb), every step rounded to the dtype as a separate op would
    x, r = _randn(rows, H, seed=H + 1).to(dt), _randn(rows, H, seed=H + 2).to(dt)
    xb = _randn(H, seed=H + 3).to(dt)
    y, mean, rstd, hs = hip.bdrln_fwd(x, xb, r, w, b, 1e-5, seed, thresh, kscale)
    z = (x.float() + xb.float()).to(dt)
    zd = (z.float() * ksf).to(dt) * kd
    want_hs = (zd.float() + r.float()).to(dt)
    if dt == F32:   # no rounding between the scale and the residual add: the kernel may fuse them
        check("bdrln_fwd", tag + " hs", hs, zd.double() + r.double(), want_hs)
    else:
        assert torch.equal(hs, want_hs)
    _ln_fwd_check("bdrln_fwd", tag, hs, w, b, y, mean, rstd)
    # backward: the fused LN + dropout backward against the two separate kernels
    dy = _randn(rows, H, seed=H + 4).to(dt)
    dh0, dw0, db0 = hip.layer_norm_bwd(dy, hs, w, mean, rstd, True)
    dh, dxd, dw, db = hip.layer_norm_dropout_bwd(dy, hs, w, mean, rstd, True, seed, thresh, kscale)
    assert torch.equal(dh, dh0) and torch.equal(dw, dw0) and torch.equal(db, db0)
    want = (dh.float() * ksf).to(dt) * kd
    assert torch.equal(dxd, want)
    for bdt in (F32, dt):
        dx2, dbias = hip.dropout_bias_bwd(dh, seed, thresh, kscale, bias_dtype=bdt)
        assert torch.equal(dx2, want)
        check("dropout_bias_bwd", f"{tag} dbias {_name(bdt)}", dbias, R.col_sum(dx2), dx2.float().sum(0), bdt,
              relax=("zero32",))
    # another seed gives another mask
    _, _, _, hs2 = hip.bdrln_fwd(one, None, zero, w, b, 1e-5, seed + 1, thresh, kscale)
    assert rows * H < 64 or not torch.equal(hs2, hs1)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("H", WIDTHS)
def test_dropout_family_widths(H, p, dt):
    _dropout_case(5, H, p, dt, stats=False)


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("rows,H", STRIDED)
def test_dropout_family_grid_stride(rows, H, p):
    """the strided row loops (dropout_bias_bwd_kernel prefetches the next row) and the kept fraction,
    within 4 binomial standard deviations of 1 - thresh / 65536"""
    _dropout_case(rows, H, p, BF16, stats=True)


# ------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------
def _minus_inf_rows(rows, H, seed):
    """3 * randn with -inf in a random 70 % of each row (one entry always finite); with 5 rows, row 1 has
    a single finite entry and row 2 has its first 512 columns (H - 1 if fewer) at -inf"""
    x = 3.0 * _randn(rows, H, seed=seed)
    m = _rand(rows, H, seed=seed + 1) < 0.7
    keep = torch.randint(0, H, (rows,), device="cuda", generator=_gen(seed + 2))
    m[torch.arange(rows, device="cuda"), keep] = False
    if rows >= 3:
        m[1] = True
        m[1, keep[1]] = False
        m[2] = False
        m[2, :min(512, H - 1)] = True
    return x.masked_fill(m, -INF), keep


def _softmax_bwd_scale(dy, y):
    """sum |y dy| per row (RELAX["sumscale"])"""
    return (y.double() * dy.double()).abs().sum(-1, keepdim=True)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("H", SOFTMAX_WIDTHS)
@pytest.mark.parametrize("rows", [1, 5])
def test_softmax_fwd_bwd(rows, H, dt):
    from paddle_hackathon_amd.ops import hip
    tag = f"{rows}x{H} {_name(dt)}"
    x = (3.0 * _randn(rows, H, seed=H)).to(dt)
    xi, keep = _minus_inf_rows(rows, H, H + 5)
    inputs = [("randn", x, x), ("-inf", xi.to(dt), xi.to(dt))]
    if dt == F32:   # a multiple of 1/64 plus 1e4 is exact in fp32: the shifted row has the unshifted row's softmax
        xq = torch.round(x * 64.0) / 64.0
        assert torch.equal((xq + 1e4) - 1e4, xq)
        inputs.append(("+1e4", xq + 1e4, xq))
    for kind, xin, xref in inputs:
        y = hip.softmax_fwd(xin)
        ry = R.softmax(xref)
        one = ("onerow",) if rows == 1 else ()
        check("softmax_fwd", f"{tag} {kind}", y, ry, torch.softmax(xin.float(), -1), relax=("f16sub",) + one)
        if kind == "-inf":
            assert not y[xin == -INF].any()
            assert dt == F16 or torch.equal(y == 0, xin == -INF)   # (fp16 underflows below e^-17)
            if rows >= 3:
                assert torch.equal(y[1], TF.one_hot(keep[1], H).to(dt))
        ys = ry.to(dt)                          # the backward judged alone: y from the reference
        dy = _randn(rows, H, seed=H + 7).to(dt)
        dx = hip.softmax_bwd(dy, ys)
        check("softmax_bwd", f"{tag} {kind}", dx, R.softmax_bwd(dy, ys),
              torch._softmax_backward_data(dy.float(), ys.float(), -1, F32), relax=("sumscale", "f16sub") + one,
              scale=_softmax_bwd_scale(dy, ys))
        assert not dx[ys == 0].any()


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("H", [10, 4104, 8192, 16384])
def test_fused_softmax_public(H, dt):
    """ops.fused.softmax with autograd takes every width: rows the kernel does not hold (H % 8 != 0,
    H > 8192) go to torch instead of raising. There torch's own bf16 backward runs, which rounds
    intermediates to bf16: its dx is held to one bf16 rounding of the row's scale, not of each element."""
    from paddle_hackathon_amd.ops import fused
    tag = f"3x{H} {_name(dt)}"
    x = (3.0 * _randn(3, H, seed=H)).to(dt).requires_grad_(True)
    dy = _randn(3, H, seed=H + 1).to(dt)
    y = fused.softmax(x)
    y.backward(dy)
    xd, yd = x.detach(), y.detach()
    check("fused.softmax", f"{tag} y", yd, R.softmax(xd), torch.softmax(xd.float(), -1))
    native = H % 8 == 0 and H <= 8192
    check("fused.softmax", f"{tag} dx", x.grad, R.softmax_bwd(dy, yd),
          torch._softmax_backward_data(dy.float(), yd.float(), -1, F32), scale=_softmax_bwd_scale(dy, yd),
          relax=("sumscale", "eps_scale") if not native and dt != F32 else ("sumscale",))


# ------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ------------------------------------------------------------------------------------------------
CE_V = [8, 512, 2056, 4104, 7, 2049, 4101]    # V % 8 == 0: 16-byte vector path; else the element path


def _ce_check(tag, x, labels, ignore_index=-100, public=False):
    """forward (loss, lse) and backward of one logits / labels pair through hip.softmax_ce_fwd / bwd
    (public: through ops.softmax_cross_entropy and autograd). Returns (loss, dx)."""
    from paddle_hackathon_amd import ops
    from paddle_hackathon_amd.ops import hip
    rows, V = x.shape
    gl = _rand(rows, seed=V) + 0.5
    if public:
        xg = x.clone().requires_grad_(True)
        loss = ops.softmax_cross_entropy(xg, labels, ignore_index)
        (loss * gl).sum().backward()
        loss, dx, lse = loss.detach(), xg.grad, None
    else:
        loss, stats = hip.softmax_ce_fwd(x, labels, ignore_index)
        dx = hip.softmax_ce_bwd(gl, x, labels, stats, ignore_index)
        lse = stats[0]
    rloss, rlse = R.softmax_ce(x, labels, ignore_index)
    rdx = R.softmax_ce_bwd(gl, x, labels, ignore_index)
    # torch's fp32 op: labels the kernel ignores become its ignore_index (it rejects others out of range)
    ign = (labels == ignore_index) | (labels < 0) | (labels >= V)
    xt = x.float().requires_grad_(True)
    tl = TF.cross_entropy(xt, torch.where(ign, torch.full_like(labels, ignore_index), labels), reduction="none",
                          ignore_index=ignore_index)
    fin = torch.isfinite(tl.detach())
    (torch.where(fin, tl, torch.zeros_like(tl)) * gl).sum().backward()
    # (a row whose loss is +inf has no autograd gradient: torch's fp32 softmax minus the one-hot instead)
    onehot = TF.one_hot(labels.clamp(0, V - 1), V).float()
    tdx = torch.where(fin.unsqueeze(1), xt.grad, gl.unsqueeze(1) * (torch.softmax(x.float(), -1) - onehot))
    one = ("onerow",) if rows == 1 else ()
    check("softmax_ce_fwd", f"{tag} loss", loss, rloss, tl.detach(), F32, relax=one)
    if lse is not None:
        check("softmax_ce_fwd", f"{tag} lse", lse, rlse, torch.logsumexp(x.float(), -1), F32)
    check("softmax_ce_bwd", f"{tag} dx", dx, rdx, tdx, relax=("f16sub",) + one)
    if ign.any():
        assert not loss[ign].any() and not dx[ign].any()
    return loss, dx


def _labels(rows, V, seed):
    return torch.randint(0, V, (rows,), device="cuda", generator=_gen(seed))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("V", CE_V)
@pytest.mark.parametrize("rows", [1, 9])
def test_softmax_ce_values_and_labels(rows, V, dt):
    """2 * randn logits (and + 3e4 in fp32 / fp16) with labels 0, V - 1, ignore_index and the labels
    outside [0, V) that the kernel treats as ignored: V, V + 5, -7; and every row ignored"""
    tag = f"{rows}x{V} {_name(dt)}"
    x = 2.0 * _randn(rows, V, seed=V)
    inputs = [("randn", x.to(dt))]
    if dt != BF16:
        inputs.append(("+3e4", (x + 3e4).to(dt)))
    special = [0, V - 1, -100, V, V + 5, -7]
    for kind, xin in inputs:
        assert torch.isfinite(xin).all()
        if rows == 1:
            for lab in special:
                _ce_check(f"{tag} {kind} label={lab}", xin, torch.tensor([lab], device="cuda"))
        else:
            lab = _labels(rows, V, V + 1)
            lab[:6] = torch.tensor(special, device="cuda")
            _ce_check(f"{tag} {kind}", xin, lab)
        loss, dx = _ce_check(f"{tag} {kind} all ignored", xin, torch.full((rows,), 3, device="cuda"), ignore_index=3)
        assert not loss.any() and not dx.any()


def _ce_inf_masks(rows, V, seed):
    """the -inf column patterns; at most V - 1 columns, so a finite entry always remains"""
    col = torch.arange(V, device="cuda")
    pats = {"cols 0..7": col < min(8, V - 1), "cols 8..15": (col >= 8) & (col < 16) if V > 16 else None,
            "cols 2048..2055": (col >= 2048) & (col < 2056) if V >= 2056 else None,
            "tail 47": col >= V - 47 if V > 47 else col >= 1}
    out = {k: v.expand(rows, V) for k, v in pats.items() if v is not None}
    m = _rand(rows, V, seed=seed) < 0.5
    m[:, seed % V] = False
    out["random 50%"] = m
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("V", CE_V)
@pytest.mark.parametrize("rows", [1, 9])
def test_softmax_ce_minus_inf(rows, V, dt):
    """masked / padded vocabulary: the loss of a finite label is finite and the reference's, the
    gradient is exactly 0 at the -inf logits, and a label on a -inf logit gives loss +inf"""
    x = (2.0 * _randn(rows, V, seed=V + 2)).to(dt)
    for name, m in _ce_inf_masks(rows, V, V + 3).items():
        tag = f"{rows}x{V} {_name(dt)} -inf {name}"
        xin = x.masked_fill(m, -INF)
        # labels on finite logits: the first finite column at or after a random start (cyclic)
        start = _labels(rows, V, V + 4)
        order = (start.unsqueeze(1) + torch.arange(V, device="cuda")) % V
        first = (~m.gather(1, order)).int().argmax(1)
        lab = order.gather(1, first.unsqueeze(1)).squeeze(1)
        assert torch.isfinite(xin.gather(1, lab.unsqueeze(1))).all()
        loss, dx = _ce_check(tag, xin, lab)
        assert torch.isfinite(loss).all() and not dx[m].any()
        # row 0's label moved onto a -inf logit
        lab2 = lab.clone()
        lab2[0] = int(torch.nonzero(m[0])[0])
        loss2, dx2 = _ce_check(tag + " label on -inf", xin, lab2)
        assert float(loss2[0]) == INF and torch.isfinite(loss2[1:]).all()
        hit = m.clone()
        hit[0, lab2[0]] = False
        assert not dx2[hit].any()


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("V", [512, 2049])
def test_softmax_ce_public(V, dt):
    """ops.softmax_cross_entropy with autograd: both kernel paths, -inf in columns 0..7, and the
    special labels"""
    rows = 9
    x = (2.0 * _randn(rows, V, seed=V + 6)).to(dt)
    x[:, :8] = -INF
    lab = _labels(rows, V - 8, V + 7) + 8
    lab[:5] = torch.tensor([V - 1, -100, V, V + 5, -7], device="cuda")
    loss, dx = _ce_check(f"{rows}x{V} {_name(dt)} public", x, lab, public=True)
    assert torch.isfinite(loss).all() and not dx[:, :8].any()


# ------------------------------------------------------------------------------------------------
# bias + GELU
# ------------------------------------------------------------------------------------------------
GRID = [0.0, -0.0, 1e-4, -1e-4, 5.0, -5.0, 10.0, -10.0, 30.0, -30.0, 100.0, -100.0, 1000.0, -1000.0]
SAT = 10.0   # from here on gelu(z) is z or 0 and gelu'(z) is 1 or 0 to far below every dtype's rounding


def _gelu_inputs(rows, H, dt, bias, seed):
    """randn with the grid in row 0 (H = 8: the grid's halves in two inputs); the bias is 0 under the
    grid so that x + b is the grid value"""
    b = (0.25 * _randn(H, seed=seed + 1)).to(dt) if bias else None
    xs = []
    for part in ([GRID] if H >= len(GRID) else [GRID[:8], GRID[8:]]):   # (the second half leaves two randn entries)
        x = _randn(rows, H, seed=seed)
        x[0, :len(part)] = torch.tensor(part, device="cuda")
        xs.append(x.to(dt))
    if bias:
        b[:min(H, len(GRID))] = 0
    return xs, b


def _gelu_check(tag, x, b, gy, approximate, y, gx, db, want_db):
    dt = x.dtype
    z32 = x.float() if b is None else x.float() + b.float()
    zt = z32.clone().requires_grad_(True)
    ty = TF.gelu(zt, approximate="tanh" if approximate else "none")
    ty.backward(gy.float())
    rgx, _ = R.bias_gelu_bwd(gy, x, b, approximate)
    check("bias_gelu_fwd", tag, y, R.bias_gelu(x, b, approximate), ty.detach())
    check("bias_gelu_bwd", tag, gx, rgx, zt.grad)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    hi, lo = z32 >= SAT, z32 <= -SAT
    assert hi.any() and lo.any()
    assert torch.equal(y[hi], z32[hi].to(dt)) and not y[lo].any()
    g1 = R.gelu_grad(z32, approximate).to(dt)
    one, nul = hi & (g1 == 1), lo & (g1 == 0)   # (in fp32 and bf16 gelu'(-10) = -8e-22 is not 0; -30 is)
    assert (one.any() or float(z32.max()) < SAT) and (nul.any() or float(z32.min()) > -30.0)
    assert torch.equal(gx[one], gy[one]) and not gx[nul].any()
    if b is not None and want_db:   # the bias gradient: column sums of the stored gx
        H = x.shape[-1]
        check("bias_gelu_bwd", tag + " db", db, R.col_sum(gx.reshape(-1, H)), gx.reshape(-1, H).float().sum(0),
              relax=("zero32",))
    else:
        assert db is None


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("want_db", [True, False])
@pytest.mark.parametrize("approximate", [False, True], ids=["erf", "tanh"])
@pytest.mark.parametrize("rows,H", [(1, 8), (33, 520), (600, 72)])
def test_bias_gelu(rows, H, approximate, want_db, dt):
    """16-bit types run bias_gelu_bwd_db (want_db) / bias_gelu_bwd_rows, fp32 the flat kernel; 600 x 72:
    16 rows per block, 38 blocks, the last one ragged"""
    from paddle_hackathon_amd.ops import hip
    xs, b = _gelu_inputs(rows, H, dt, True, H)
    gy = _randn(rows, H, seed=H + 2).to(dt)
    for i, x in enumerate(xs):
        y = hip.bias_gelu_fwd(x, b, approximate)
        gx, db = hip.bias_gelu_bwd(gy, x, b, approximate, want_db=want_db)
        form = "tanh" if approximate else "erf"
        _gelu_check(f"{rows}x{H} {_name(dt)} {form} db={want_db} #{i}", x, b, gy, approximate, y, gx, db, want_db)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("approximate", [False, True], ids=["erf", "tanh"])
def test_gelu_no_bias(approximate, dt):
    from paddle_hackathon_amd.ops import hip
    rows, H = 33, 520
    xs, _ = _gelu_inputs(rows, H, dt, False, H + 5)
    gy = _randn(rows, H, seed=H + 6).to(dt)
    y = hip.bias_gelu_fwd(xs[0], None, approximate)
    gx, db = hip.bias_gelu_bwd(gy, xs[0], None, approximate)
    _gelu_check(f"{rows}x{H} {_name(dt)} {'tanh' if approximate else 'erf'} b=None", xs[0], None, gy, approximate,
                y, gx, db, True)


# ------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
@pytest.mark.parametrize("H", [8, 72, 520])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 8193])
def test_col_sum(rows, H, dt):
    """16 rows per block up to 8192 rows, 17 per block at 8193"""
    from paddle_hackathon_amd.ops import hip
    x = _randn(rows, H, seed=rows + H).to(dt)
    for odt in (dt, F32):
        out = hip.col_sum(x, odt)
        check("col_sum", f"{rows}x{H} {_name(dt)} -> {_name(odt)}", out, R.col_sum(x), x.float().sum(0), odt,
              relax=("zero32",))


def _col_sum_rows_case(P, H, odt):
    """the first P rows of a [P + 8, H] fp32 buffer; the 8 stage rows hold NaN: the single-launch
    kernel must not read them, the two-stage path writes them before it reads them"""
    from paddle_hackathon_amd.ops import hip
    part = _randn(P + 8, H, seed=P + H)
    part[P:] = math.nan
    want, t32 = R.col_sum(part[:P]), part[:P].sum(0)
    out = hip._col_sum_rows(part, P, odt)
    check("col_sum_rows", f"P={P} H={H} -> {_name(odt)}", out, want, t32, odt)


@pytest.mark.parametrize("odt", DTYPES, ids=_name)
@pytest.mark.parametrize("H", [8, 72, 200])
@pytest.mark.parametrize("P", [1, 5, 33, 1024, 1025, 3000])
def test_col_sum_rows(P, H, odt):
    """P <= 1024: col_sum_n_kernel in one launch; 1025 and 3000: col_partial_kernel + col_reduce_kernel"""
    _col_sum_rows_case(P, H, odt)


def _two_launch_child():
    """runs in the child of test_col_sum_two_launch_path (PHA_COLSUM1=0)"""
    assert os.environ.get("PHA_COLSUM1") == "0"
    from paddle_hackathon_amd.ops import _lib
    assert _lib.native_available()
    for P in (5, 33, 40):       # col_reduce_kernel alone up to 32 partial rows, both stages above
        for odt in DTYPES:
            _col_sum_rows_case(P, 72, odt)
    _ln_bwd_case(17, 520, BF16, F32, "AC")
    torch.cuda.synchronize()


def test_col_sum_two_launch_path():
    """PHA_COLSUM1=0 (read once per process, so a fresh child): small P through col_reduce_kernel and
    col_partial_kernel, and a LayerNorm backward whose dw / db / dx_colsum take that path"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_rowwise_edges_gpu as T; T._two_launch_child()"
            % (here, os.path.dirname(here)))
    r = subprocess.run([sys.executable, "-c", code], timeout=120, env=dict(os.environ, PHA_COLSUM1="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
