"""The contracts of the row-wise HIP kernels (csrc/kernels/norm_softmax.hip, ce_gelu_embed.hip) in
float64 torch: the reference of tests/test_rowwise_edges_gpu.py.

Every function takes inputs that are already rounded to the dtype under test (any dtype, any
device), computes in float64 and returns float64. The formulae are written out: none of them calls
the torch op it mirrors (tests/test_rowwise_reference_cpu.py compares them with those ops)."""
import math

import torch

F64 = torch.float64


def _d(t):
    return None if t is None else t.to(F64)


def layer_norm(x, w, b, eps):
    """y = (x - mean) * rstd * w + b over the last dim; returns (y, mean, rstd), the statistics per row
    (biased variance, rstd = 1 / sqrt(var + eps))"""
    x, w, b = _d(x), _d(w), _d(b)
    H = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / H
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / H
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * w
    if b is not None:
        y = y + b
    return y, mean.squeeze(-1), rstd.squeeze(-1)


def layer_norm_bwd(dy, x, w, dres=None, eps=1e-5, mean=None, rstd=None):
    """Gradients of layer_norm for the output gradient dy: (dx, dw, db, dx_colsum). dres is the
    gradient of a residual sum fused into the forward and is added to dx; dx_colsum = the column sums
    of that final dx. mean / rstd (per row): the saved statistics the kernel is given — by default
    those of x with eps."""
    dy, x, w, dres = _d(dy), _d(x), _d(w), _d(dres)
    H = x.shape[-1]
    if mean is None or rstd is None:
        _, mean, rstd = layer_norm(x, w, None, eps)
    mean, rstd = _d(mean).unsqueeze(-1), _d(rstd).unsqueeze(-1)
    xh = (x - mean) * rstd
    g = dy * w
    c1 = (g * xh).sum(-1, keepdim=True) / H
    c2 = g.sum(-1, keepdim=True) / H
    dx = rstd * (g - xh * c1 - c2)
    if dres is not None:
        dx = dx + dres
    dy2, xh2, dx2 = dy.reshape(-1, H), xh.reshape(-1, H), dx.reshape(-1, H)
    return dx, (dy2 * xh2).sum(0), dy2.sum(0), dx2.sum(0)


def softmax(x):
    """exp(x - max) / sum over the last dim; -inf entries give exactly 0 (a row needs a finite entry)"""
    x = _d(x)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd(dy, y):
    """dx = y * (dy - sum(y * dy)) from the stored output y"""
    dy, y = _d(dy), _d(y)
    return y * (dy - (y * dy).sum(-1, keepdim=True))


def _ignored(labels, V, ignore_index):
    return (labels == ignore_index) | (labels < 0) | (labels >= V)


def softmax_ce(logits, labels, ignore_index=-100):
    """Hard-label softmax cross-entropy of [rows, V] logits: (loss, lse) per row, lse = log sum exp.
    A label equal to ignore_index or outside [0, V) is ignored: loss 0. A label on a -inf logit
    gives loss +inf."""
    x = _d(logits)
    V = x.shape[-1]
    m = x.max(-1).values
    ls = torch.log(torch.exp(x - m.unsqueeze(-1)).sum(-1))
    ign = _ignored(labels, V, ignore_index)
    xl = x.gather(-1, labels.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    loss = torch.where(ign, torch.zeros_like(m), (m - xl) + ls)   # (m - xl): no inf - inf at xl = -inf
    return loss, m + ls


def softmax_ce_bwd(gloss, logits, labels, ignore_index=-100):
    """d loss / d logits times gloss (per row): gloss * (softmax - onehot(label)), a zero row for an
    ignored label"""
    x, g = _d(logits), _d(gloss)
    V = x.shape[-1]
    ign = _ignored(labels, V, ignore_index)
    p = softmax(x)
    onehot = torch.zeros_like(p).scatter_(-1, labels.clamp(0, V - 1).unsqueeze(-1), 1.0)
    g = torch.where(ign, torch.zeros_like(g), g).unsqueeze(-1)
    return g * (p - onehot)


_K, _C = math.sqrt(2.0 / math.pi), 0.044715


def _pre(x, b):
    x = _d(x)
    return x if b is None else x + _d(b)


def _cdf(z, approximate):
    """(Phi, 1 - Phi) of the form, each accurate in its own tail: erf form Phi(z) = erfc(-z / sqrt 2) / 2;
    tanh form (1 + tanh u) / 2 = 1 / (1 + exp(-2u)), u = k (z + c z^3)"""
    if approximate:
        u2 = 2.0 * _K * (z + _C * z * z * z)
        return 1.0 / (1.0 + torch.exp(-u2)), 1.0 / (1.0 + torch.exp(u2))
    r = z / math.sqrt(2.0)
    return 0.5 * torch.erfc(-r), 0.5 * torch.erfc(r)


def bias_gelu(x, b, approximate):
    """gelu(x + b) = z Phi(z): erf form Phi = (1 + erf(z / sqrt 2)) / 2, tanh form Phi = (1 + tanh(k (z +
    c z^3))) / 2, written so that the tail z -> -inf keeps its relative precision"""
    z = _pre(x, b)
    return z * _cdf(z, approximate)[0]


def gelu_grad(z, approximate):
    z = _d(z)
    s, t = _cdf(z, approximate)
    if approximate:   # d/dz z s(2u) = s + z s (1 - s) 2k (1 + 3c z^2)
        return s + z * s * t * 2.0 * _K * (1.0 + 3.0 * _C * z * z)
    return s + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def bias_gelu_bwd(gy, x, b, approximate):
    """(gx, db): gx = gy * gelu'(x + b), db = its column sums (None without a bias)"""
    gx = _d(gy) * gelu_grad(_pre(x, b), approximate)
    return gx, (None if b is None else gx.reshape(-1, gx.shape[-1]).sum(0))


def col_sum(x):
    """column sums of a [rows, H] matrix"""
    return _d(x).sum(0)
