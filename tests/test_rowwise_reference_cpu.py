"""CPU half of tests/test_rowwise_edges_gpu.py: the float64 references in rowwise_reference.py, which
write every formula out, agree with torch's own float64 ops and autograd on small random inputs
and on the edge inputs the GPU tests use (-inf logits, a constant row, labels outside [0, V))."""
import math

import pytest
import torch
import torch.nn.functional as TF

import rowwise_reference as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert a.dtype == F64 and a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


def _randn(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("rows,H", [(1, 8), (5, 24), (7, 130)])
@pytest.mark.parametrize("bias", [True, False])
def test_layer_norm(rows, H, bias):
    x, w = 3.0 + 2.0 * _randn(rows, H), 0.5 + torch.rand(H, dtype=F64)
    b = _randn(H, seed=1) if bias else None
    y, mean, rstd = R.layer_norm(x, w, b, 1e-5)
    _close(y, TF.layer_norm(x, [H], w, b, 1e-5))
    _close(mean, x.mean(-1))
    _close(rstd, 1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5))
    # float32 inputs are taken as they are and computed in float64
    y32, _, _ = R.layer_norm(x.float(), w.float(), None if b is None else b.float(), 1e-5)
    assert y32.dtype == F64
    _close(y32, TF.layer_norm(x.float().double(), [H], w.float().double(), None if b is None else b.float().double(), 1e-5))


def test_layer_norm_constant_row():
    H, eps = 40, 1e-5
    x = _randn(3, H)
    x[1] = 7.25
    w, b = 0.5 + torch.rand(H, dtype=F64), _randn(H, seed=2)
    y, mean, rstd = R.layer_norm(x, w, b, eps)
    assert float(mean[1]) == 7.25 and float(rstd[1]) == 1.0 / math.sqrt(eps)
    assert torch.equal(y[1], b)


@pytest.mark.parametrize("rows,H", [(1, 8), (6, 24), (17, 130)])
@pytest.mark.parametrize("with_dres", [False, True])
def test_layer_norm_bwd(rows, H, with_dres):
    x = _randn(rows, H).requires_grad_(True)
    w = (0.5 + torch.rand(H, dtype=F64)).requires_grad_(True)
    b = _randn(H, seed=1).requires_grad_(True)
    dy = _randn(rows, H, seed=2)
    dres = _randn(rows, H, seed=3) if with_dres else None
    TF.layer_norm(x, [H], w, b, 1e-5).backward(dy)
    want_dx = x.grad + dres if with_dres else x.grad
    dx, dw, db, dxs = R.layer_norm_bwd(dy, x.detach(), w.detach(), dres, eps=1e-5)
    _close(dx, want_dx)
    _close(dw, w.grad)
    _close(db, b.grad)
    _close(dxs, want_dx.sum(0))
    # the saved statistics passed in give the same gradients
    _, mean, rstd = R.layer_norm(x.detach(), w.detach(), None, 1e-5)
    dx2, dw2, _, _ = R.layer_norm_bwd(dy, x.detach(), w.detach(), dres, mean=mean, rstd=rstd)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw)


@pytest.mark.parametrize("rows,H", [(1, 8), (5, 37), (3, 600)])
def test_softmax_and_bwd(rows, H):
    x = (3.0 * _randn(rows, H)).requires_grad_(True)
    dy = _randn(rows, H, seed=1)
    yt = torch.softmax(x, -1)
    yt.backward(dy)
    y = R.softmax(x.detach())
    _close(y, yt.detach())
    _close(R.softmax_bwd(dy, y), x.grad)
    # a shift of the row changes nothing beyond the rounding of x + 1e4 itself
    _close(R.softmax(x.detach() + 1e4), y, tol=1e-10)


def test_softmax_minus_inf():
    x = 3.0 * _randn(4, 600)
    x[0, :512] = -math.inf                      # the whole first chunk of a row
    x[1] = -math.inf
    x[1, 77] = 0.5                              # one finite entry: exactly one-hot
    x[2, torch.rand(600, generator=torch.Generator().manual_seed(5)) < 0.7] = -math.inf
    y = R.softmax(x)
    _close(y, torch.softmax(x, -1))
    assert torch.equal(y[1], TF.one_hot(torch.tensor(77), 600).to(F64))
    assert torch.equal(y[0, :512], torch.zeros(512, dtype=F64)) and not torch.isnan(y).any()
    assert torch.equal(y == 0, x == -math.inf)


@pytest.mark.parametrize("rows,V", [(1, 7), (9, 8), (9, 130)])
def test_softmax_ce(rows, V):
    x = (2.0 * _randn(rows, V)).requires_grad_(True)
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[0] = 0
    lab[-1] = V - 1
    if rows > 2:
        lab[1] = -100
    gl = _randn(rows, seed=4)
    lt = TF.cross_entropy(x, lab, reduction="none", ignore_index=-100)
    lt.backward(gl)
    loss, lse = R.softmax_ce(x.detach(), lab, -100)
    _close(loss, lt.detach())
    _close(lse, torch.logsumexp(x.detach(), -1))
    _close(R.softmax_ce_bwd(gl, x.detach(), lab, -100), x.grad)
    # large offset: the loss is that of the unshifted row (up to the rounding of x + 3e4)
    loss2, lse2 = R.softmax_ce(x.detach() + 3e4, lab, -100)
    _close(loss2, loss, tol=1e-10)
    _close(lse2, lse + 3e4)


def test_softmax_ce_labels_out_of_range_are_ignored():
    V = 24
    x = 2.0 * _randn(6, V)
    lab = torch.tensor([V, V + 5, -7, -100, 3, V - 1])
    loss, lse = R.softmax_ce(x, lab, -100)
    dx = R.softmax_ce_bwd(torch.ones(6, dtype=F64), x, lab, -100)
    assert torch.equal(loss[:4], torch.zeros(4, dtype=F64)) and torch.equal(dx[:4], torch.zeros(4, V, dtype=F64))
    inr = TF.cross_entropy(x[4:], lab[4:], reduction="none")
    _close(loss[4:], inr)
    _close(lse, torch.logsumexp(x, -1))
    # a different ignore_index: -100 is then just another out-of-range label; all rows ignored
    loss_all, _ = R.softmax_ce(x, torch.full((6,), 5), 5)
    assert torch.equal(loss_all, torch.zeros(6, dtype=F64))
    assert not R.softmax_ce_bwd(torch.ones(6, dtype=F64), x, torch.full((6,), 5), 5).any()


def test_softmax_ce_minus_inf():
    V = 64
    x = (2.0 * _randn(5, V))
    x[0, :8] = -math.inf
    x[1, 8:16] = -math.inf
    x[2, V - 47:] = -math.inf
    x[3, torch.rand(V, generator=torch.Generator().manual_seed(1)) < 0.5] = -math.inf
    x[4, :8] = -math.inf
    lab = torch.tensor([9, 0, 3, int(torch.nonzero(x[3] > -math.inf)[0]), 2])   # row 4: label on a -inf logit
    xr = x.clone().requires_grad_(True)
    lt = TF.cross_entropy(xr, lab, reduction="none")
    lt[:4].sum().backward()
    loss, lse = R.softmax_ce(x, lab, -100)
    assert torch.isfinite(loss[:4]).all() and loss[4] == math.inf and torch.isfinite(lse).all()
    _close(loss[:4], lt.detach()[:4])
    dx = R.softmax_ce_bwd(torch.ones(5, dtype=F64), x, lab, -100)
    assert torch.isfinite(dx).all()
    _close(dx[:4], xr.grad[:4])
    assert not dx[:4][x[:4] == -math.inf].any()
    assert dx[4, 2] == -1.0                       # the label on a -inf logit: softmax 0 minus the one-hot 1


GRID = [0.0, -0.0, 1e-4, -1e-4, 5.0, -5.0, 10.0, -10.0, 30.0, -30.0, 100.0, -100.0, 1000.0, -1000.0]


@pytest.mark.parametrize("approximate", [False, True])
@pytest.mark.parametrize("bias", [True, False])
def test_bias_gelu(approximate, bias):
    H = 24
    x = torch.cat([_randn(5, H).reshape(-1), torch.tensor(GRID, dtype=F64), torch.zeros(10, dtype=F64)]).reshape(-1, H)
    b = 0.25 * _randn(H, seed=1) if bias else None
    gy = _randn(*x.shape, seed=2)
    z = (x + b if bias else x).clone().requires_grad_(True)
    yt = TF.gelu(z, approximate="tanh" if approximate else "none")
    yt.backward(gy)
    _close(R.bias_gelu(x, b, approximate), yt.detach())
    gx, db = R.bias_gelu_bwd(gy, x, b, approximate)
    _close(gx, z.grad)
    if bias:
        _close(db, z.grad.sum(0))
    else:
        assert db is None
    assert torch.isfinite(gx).all()


@pytest.mark.parametrize("approximate", [False, True])
def test_bias_gelu_saturates(approximate):
    z = torch.tensor([30.0, 100.0, 1000.0], dtype=F64)
    assert torch.equal(R.bias_gelu(z, None, approximate), z)
    assert torch.equal(R.bias_gelu(-z, None, approximate).float().abs(), torch.zeros(3))   # (-30 Phi(-30) = -1e-196)
    # the derivative's tail (-30 phi(30) = -1e-194 in the erf form) is 0 in every dtype under test
    assert torch.equal(R.gelu_grad(z, approximate).float(), torch.ones(3))
    assert torch.equal(R.gelu_grad(-z, approximate).float().abs(), torch.zeros(3))


def test_col_sum():
    x = _randn(33, 24)
    _close(R.col_sum(x), x.sum(0))
    _close(R.col_sum(x.bfloat16()), x.bfloat16().double().sum(0))
