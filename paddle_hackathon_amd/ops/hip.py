"""ctypes bindings to ``libpha_kernels.so`` (torch tensors in, torch tensors out).

Each call passes raw device pointers and the *current* torch HIP stream, so the
kernels order correctly with PyTorch-ROCm's own work and are capturable in HIP
graphs. Shape preconditions are checked here on the host before any launch
(a kernel reading out of bounds can take the whole GPU node down). The argument types of
every entry point are declared once, in ``_abi.SIGNATURES``, when ``_lib`` loads the library:
call sites here pass plain Python numbers and the ``_ptr`` / ``_stream`` addresses.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int

import numpy as np
import torch

from . import _lib
from ._abi import DT as _DT, check as _check, ptr as _ptr, stream as _stream

_L = _lib.loaded


# ----------------------------------------------------------------------------
# layer norm / softmax
# ----------------------------------------------------------------------------
def layer_norm_fwd(x, w, b, eps, residual=None):
    """y = LN(x) — or, with ``residual``, hs = x + residual and y = LN(hs) in one pass.
    Returns (y, mean, rstd) or (y, mean, rstd, hs)."""
    H = w.numel()
    rows = x.numel() // H
    assert x.numel() == rows * H and H % 8 == 0 and H <= 4096
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    hs = None
    if residual is not None:
        assert residual.shape == x.shape and residual.dtype == x.dtype and residual.is_contiguous()
        hs = torch.empty_like(x)
    _check(_L().pha_layer_norm_fwd2(_DT[x.dtype], _DT[w.dtype], _ptr(x), _ptr(residual), _ptr(hs), _ptr(w.contiguous()),
                                    _ptr(None if b is None else b.contiguous()), _ptr(y), _ptr(mean), _ptr(rstd), rows, H,
                                    float(eps), _stream(x)), "layer_norm_fwd")
    return (y, mean, rstd) if residual is None else (y, mean, rstd, hs)


def layer_norm_bwd(dy, x, w, mean, rstd, has_bias, dres=None, dx_colsum=None):
    """dx = LN'(dy) (+ dres: gradient of a fused residual sum). ``x`` is the normalised input.
    dx_colsum (a dtype: fp32 or x's): also return the column sums of dx in it — the gradient of a
    bias that was folded into the forward's residual sum (add_layer_norm's ``xb``)."""
    H = w.numel()
    rows = x.numel() // H
    nblocks = int(_L().pha_layer_norm_bwd_nblocks(rows, H))  # partials [nblocks, H]
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    db = torch.empty_like(w) if has_bias else None
    if dres is not None:
        assert dres.shape == x.shape and dres.dtype == x.dtype and dres.is_contiguous()
    part = torch.empty((3 if dx_colsum else 2, nblocks + 8, H), dtype=torch.float32, device=x.device)  # + stage rows
    if dx_colsum is not None:
        xs_dt = dx_colsum if dx_colsum in (torch.float32, x.dtype) else torch.float32
        dxs = torch.empty(H, dtype=xs_dt, device=x.device)
        _check(_L().pha_layer_norm_bwd3(_DT[x.dtype], _DT[w.dtype], _DT[xs_dt], _ptr(dy), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd),
                                        _ptr(dres), _ptr(dx), _ptr(dw), _ptr(db), _ptr(dxs), _ptr(part[0]),
                                        _ptr(part[1]), _ptr(part[2]), nblocks, rows, H, _stream(x)), "layer_norm_bwd3")
        return dx, dw, db, dxs
    _check(_L().pha_layer_norm_bwd2(_DT[x.dtype], _DT[w.dtype], _ptr(dy), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd),
                                    _ptr(dres), _ptr(dx), _ptr(dw), _ptr(db), _ptr(part[0]), _ptr(part[1]), nblocks, rows, H,
                                    _stream(x)), "layer_norm_bwd")
    return dx, dw, db


def dropout_seed(device):
    """(host seed, device seed word or None) for a dropout site whose mask the backward regenerates.
    Eager: a fresh host seed. Inside a hipGraph capture the host value would be baked into every
    replay, so the kernels also xor in a device word: a per-device counter bumped by a captured
    kernel (each replay advances it) and copied for this site — the copy is what the site's
    backward reads, whatever later sites did to the counter."""
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    buf = _SEED_BUFS.get(device)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dropout inside a hipGraph capture needs one eager step first")
        buf = _SEED_BUFS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    if not torch.cuda.is_current_stream_capturing():
        return seed, None
    out = torch.empty(1, dtype=torch.int32, device=device)
    # ++counter and the site's copy in one captured kernel
    _check(_L().pha_seed_bump(_ptr(buf), _ptr(out), _stream(buf)), "seed_bump")
    return seed, out


_SEED_BUFS = {}


def bdrln_fwd(x, xbias, residual, w, b, eps, seed, thresh, kscale, seed_dev=None):
    """fused_bias_dropout_residual_layer_norm forward: hs = residual + dropout(x + xbias), y = LN(hs).
    Returns (y, mean, rstd, hs)."""
    H = w.numel()
    rows = x.numel() // H
    assert x.numel() == rows * H and H % 8 == 0 and H <= 4096
    assert residual.shape == x.shape and residual.dtype == x.dtype and residual.is_contiguous() and x.is_contiguous()
    y, hs = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    xb = None if xbias is None else xbias.contiguous()
    if xb is not None and xb.dtype not in (torch.float32, x.dtype):
        xb = xb.float()
    xbdt = _DT[w.dtype] if xb is None else _DT[xb.dtype]
    _check(_L().pha_bdrln_fwd2(_DT[x.dtype], _DT[w.dtype], xbdt, _ptr(x), _ptr(xb), _ptr(residual), _ptr(hs),
                              _ptr(w.contiguous()), _ptr(None if b is None else b.contiguous()), _ptr(y), _ptr(mean),
                              _ptr(rstd), rows, H, float(eps), int(seed), int(thresh), float(kscale), _stream(x),
                              _ptr(seed_dev)),
           "bdrln_fwd")
    return y, mean, rstd, hs


def layer_norm_dropout_bwd(dy, x, w, mean, rstd, has_bias, seed, thresh, kscale, seed_dev=None):
    """The bias-free fused_bias_dropout_residual_layer_norm backward in one pass: returns
    (dh, dx, dw, db) with dh = LN'(dy) (the residual's gradient) and dx = dh * mask * kscale (the
    forward's regenerated mask) — layer_norm_bwd + dropout_bias_bwd without re-reading dh."""
    H = w.numel()
    rows = x.numel() // H
    nblocks = int(_L().pha_layer_norm_bwd_nblocks(rows, H))
    dh, dx = torch.empty_like(x), torch.empty_like(x)
    dw = torch.empty_like(w)
    db = torch.empty_like(w) if has_bias else None
    part = torch.empty((2, nblocks + 8, H), dtype=torch.float32, device=x.device)
    _check(_L().pha_layer_norm_dropout_bwd(_DT[x.dtype], _DT[w.dtype], _ptr(dy), _ptr(x), _ptr(w), _ptr(mean),
                                           _ptr(rstd), _ptr(dh), _ptr(dx), _ptr(dw), _ptr(db), _ptr(part[0]),
                                           _ptr(part[1]), nblocks, rows, H, int(seed), int(thresh), float(kscale),
                                           _stream(x), _ptr(seed_dev)),
           "layer_norm_dropout_bwd")
    return dh, dx, dw, db


def dropout_bias_bwd(dh, seed, thresh, kscale, bias_dtype=None, seed_dev=None):
    """dx = dh * mask * kscale (the forward's regenerated mask) and dbias = column sums of dx."""
    H = dh.shape[-1]
    rows = dh.numel() // H
    nblocks = int(_L().pha_layer_norm_bwd_nblocks(rows, H))
    dx = torch.empty_like(dh)
    db = torch.empty(H, dtype=bias_dtype, device=dh.device) if bias_dtype is not None else None
    wdt = _DT[bias_dtype] if bias_dtype is not None else _DT[dh.dtype]
    part = torch.empty((nblocks + 8, H), dtype=torch.float32, device=dh.device)
    _check(_L().pha_dropout_bias_bwd(_DT[dh.dtype], wdt, _ptr(dh), _ptr(dx), _ptr(db), _ptr(part), nblocks, rows, H,
                                     int(seed), int(thresh), float(kscale), _stream(dh), _ptr(seed_dev)),
           "dropout_bias_bwd")
    return dx, db


# ----------------------------------------------------------------------------
# batch norm (channels-last [M, C] view), optional fused residual-add + ReLU
# ----------------------------------------------------------------------------
def bn_supported(x, C):
    return x.is_cuda and x.dtype in _DT and x.is_contiguous() and C % 8 == 0 and x.numel() > 0 and x.shape[-1] == C


def bn_fwd_train(x, w, b, running_mean, running_var, eps, momentum, residual=None, relu=False, ext_stats=None):
    """x: [..., C] contiguous (NHWC). Returns y, save_mean, save_istd. Updates running stats in place.
    ext_stats = (partials [rows][2][C] fp32, rows): unshifted channel sums / sums of squares of x
    already computed by x's producer (the conv epilogue) — the statistics pass over x is skipped."""
    C = x.shape[-1]
    M = x.numel() // C
    assert bn_supported(x, C) and w.dtype == torch.float32 and w.numel() == C
    assert residual is None or (residual.shape == x.shape and residual.dtype == x.dtype and residual.is_contiguous())
    assert running_mean is None or (running_mean.dtype == torch.float32 and running_mean.is_contiguous())
    L = _L()
    nb = L.pha_bn_num_blocks(M, C)
    f32 = dict(dtype=torch.float32, device=x.device)
    part = torch.empty((max(nb, 64) + 64) * 2 * C, **f32)
    stats = torch.empty(4, C, **f32)  # save_mean, save_istd, scale, shift
    y = torch.empty_like(x)
    _check(L.pha_bn_fwd_train(_DT[x.dtype], _ptr(x), _ptr(residual), _ptr(y), M, C, _ptr(w), _ptr(b),
                              _ptr(running_mean), _ptr(running_var), _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]),
                              _ptr(stats[3]), _ptr(part), float(eps), float(momentum), int(relu),
                              _ptr(ext_stats[0]) if ext_stats else None, int(ext_stats[1]) if ext_stats else 0,
                              _stream(x)),
           "bn_fwd_train")
    return y, stats[0], stats[1], stats[2:4]


def bn_apply(x, scale, shift, residual=None, relu=False):
    C = x.shape[-1]
    M = x.numel() // C
    assert bn_supported(x, C) and scale.dtype == torch.float32 and scale.numel() == C and shift.numel() == C
    y = torch.empty_like(x)
    _check(_L().pha_bn_apply(_DT[x.dtype], _ptr(x), _ptr(residual), _ptr(y), M, C, _ptr(scale.contiguous()),
                             _ptr(shift.contiguous()), int(relu), _stream(x)), "bn_apply")
    return y


def bn_bwd(dy, x, y, w, save_mean, save_istd, relu=False, want_dres=False, affine=None, ext_part=None):
    """affine ([2, C] fp32 forward scale / shift): with relu and y None the ReLU mask is recomputed
    from x (no residual in the forward), so y need not be kept or read."""
    C = x.shape[-1]
    M = x.numel() // C
    assert bn_supported(x, C) and dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous()
    assert not relu or (y is not None and y.shape == x.shape) or (affine is not None and affine.shape == (2, C))
    L = _L()
    nb = L.pha_bn_num_blocks(M, C)
    f32 = dict(dtype=torch.float32, device=x.device)
    part = torch.empty((max(nb, 64) + 64) * 2 * C, **f32)
    coef = torch.empty(3 * C, **f32)
    dwb = torch.empty(2, C, **f32)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    _check(L.pha_bn_bwd(_DT[x.dtype], _ptr(dy), _ptr(x), _ptr(y), M, C, _ptr(w), _ptr(save_mean), _ptr(save_istd),
                        _ptr(dx), _ptr(dres), _ptr(dwb[0]), _ptr(dwb[1]), _ptr(part), _ptr(coef), int(relu),
                        _ptr(affine.contiguous()) if affine is not None else None,
                        _ptr(ext_part[0]) if ext_part else None, int(ext_part[1]) if ext_part else 0, _stream(x)),
           "bn_bwd")
    return dx, dwb[0], dwb[1], dres


def softmax_fwd(x):
    H = x.shape[-1]
    rows = x.numel() // H
    assert H % 8 == 0 and H <= 4096
    y = torch.empty_like(x)
    _check(_L().pha_softmax_fwd(_DT[x.dtype], _ptr(x), _ptr(y), rows, H, _stream(x)), "softmax_fwd")
    return y


def softmax_bwd(dy, y):
    H = y.shape[-1]
    rows = y.numel() // H
    dx = torch.empty_like(y)
    _check(_L().pha_softmax_bwd(_DT[y.dtype], _ptr(dy), _ptr(y), _ptr(dx), rows, H, _stream(y)), "softmax_bwd")
    return dx


# ----------------------------------------------------------------------------
# cross entropy / gelu / embedding
# ----------------------------------------------------------------------------
def softmax_ce_fwd(logits, labels, ignore_index):
    rows, V = logits.shape
    assert labels.numel() == rows and V > 0   # V % 8 != 0: the kernels' element-wise path
    loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _check(_L().pha_softmax_ce_fwd(_DT[logits.dtype], _ptr(logits), _ptr(labels), _ptr(loss), _ptr(lse), rows, V,
                                   int(ignore_index), _stream(logits)), "softmax_ce_fwd")
    return loss, lse


def softmax_ce_bwd(gloss, logits, labels, lse, ignore_index):
    rows, V = logits.shape
    dx = torch.empty_like(logits)
    _check(_L().pha_softmax_ce_bwd(_DT[logits.dtype], _ptr(gloss), _ptr(logits), _ptr(labels), _ptr(lse), _ptr(dx), rows, V,
                                   int(ignore_index), _stream(logits)), "softmax_ce_bwd")
    return dx


def bias_gelu_fwd(x, b, approximate):
    n = x.numel()
    H = x.shape[-1]
    if n % 8 or (b is not None and (H % 8 or b.numel() != H)):
        import torch.nn.functional as TF
        return TF.gelu(x + b if b is not None else x, approximate="tanh" if approximate else "none")
    y = torch.empty_like(x)
    _check(_L().pha_bias_gelu_fwd(_DT[x.dtype], _ptr(x), _ptr(b), _ptr(y), n, H, int(approximate), _stream(x)), "bias_gelu_fwd")
    return y


def bias_gelu_bwd(gy, x, b, approximate, want_db=True):
    """(d(gelu(x + b)) / dx . gy, its column sums — the bias gradient; None with want_db=False, for
    callers that take it from the next weight-gradient GEMM, ops/gemm.mm_tn_db)"""
    n = x.numel()
    H = x.shape[-1]
    if n % 8 or (b is not None and H % 8):
        xx = (x + b if b is not None else x).detach().float().requires_grad_(True)
        import torch.nn.functional as TF
        with torch.enable_grad():
            y = TF.gelu(xx, approximate="tanh" if approximate else "none")
            (gx,) = torch.autograd.grad(y, xx, gy.float())
        gx = gx.to(x.dtype)
    elif b is not None and not want_db and x.dtype != torch.float32:
        gx = torch.empty_like(x)
        rows = n // H
        rpb = max(16, -(-rows // 512))
        _check(_L().pha_bias_gelu_bwd_rows(_DT[x.dtype], _ptr(gy), _ptr(x), _ptr(b), _ptr(gx), rows, H, rpb,
                                           int(approximate), _stream(x)), "bias_gelu_bwd_rows")
        return gx, None
    elif b is not None and want_db and x.dtype != torch.float32:
        # gx and the per-row-block column sums of gx in one pass; db = sum of the partials
        gx = torch.empty_like(x)
        rows = n // H
        rpb = max(16, -(-rows // 512))   # >= 2048 blocks at 16384 x 8192: 8 per CU for streaming
        P = -(-rows // rpb)
        part = torch.empty((P + 8, H), dtype=torch.float32, device=x.device)   # + column-sum stage rows
        _check(_L().pha_bias_gelu_bwd_db(_DT[x.dtype], _ptr(gy), _ptr(x), _ptr(b), _ptr(gx), _ptr(part), rows, H, rpb,
                                         int(approximate), _stream(x)), "bias_gelu_bwd_db")
        return gx, _col_sum_rows(part, P, b.dtype)
    else:
        gx = torch.empty_like(x)
        _check(_L().pha_bias_gelu_bwd(_DT[x.dtype], _ptr(gy), _ptr(x), _ptr(b), _ptr(gx), n, H, int(approximate), _stream(x)), "bias_gelu_bwd")
    gb = gx.reshape(-1, H).sum(0, dtype=torch.float32).to(b.dtype) if b is not None and want_db else None
    return gx, gb


def col_sum(gy2d, out_dtype=None):
    """column sums of a [rows, H] bf16/fp16 tensor (a linear layer's bias gradient): row-block
    partials in fp32 on the HIP kernel, then one small reduction of the partials"""
    rows, H = gy2d.shape
    if gy2d.dtype == torch.float32 or H % 8 or not gy2d.is_contiguous():
        return gy2d.sum(0, dtype=torch.float32).to(out_dtype or gy2d.dtype)
    rpb = max(16, -(-rows // 512))
    P = -(-rows // rpb)
    part = torch.empty((P + 8, H), dtype=torch.float32, device=gy2d.device)   # + column-sum stage rows
    _check(_L().pha_col_sum_partial(_DT[gy2d.dtype], _ptr(gy2d), _ptr(part), rows, H, rpb, _stream(gy2d)),
           "col_sum_partial")
    return _col_sum_rows(part, P, out_dtype or gy2d.dtype)


def _col_sum_rows(part, P, dtype):
    """column sums of the first P rows of the fp32 partials ``part`` ([P + 8, H]: the last rows are
    the kernel's first-stage workspace) into a new [H] tensor of ``dtype``"""
    H = part.shape[1]
    if dtype not in _DT:
        return part[:P].sum(0).to(dtype)
    out = torch.empty(H, dtype=dtype, device=part.device)
    _check(_L().pha_col_sum_rows(_DT[dtype], _ptr(part), _ptr(out), P, H, _stream(part)), "col_sum_rows")
    return out


class MaxPool2dNHWC(torch.autograd.Function):
    """NHWC max pool on the HIP kernels: forward keeps the window position of each max (1 byte per
    output element), backward gathers per input pixel (no atomics, no scatter)."""

    @staticmethod
    def forward(ctx, x, k, s, p):
        N, H, W, C = x.shape
        OH = (H + 2 * p[0] - k[0]) // s[0] + 1
        OW = (W + 2 * p[1] - k[1]) // s[1] + 1
        y = torch.empty(N, OH, OW, C, dtype=x.dtype, device=x.device)
        idx = torch.empty(N, OH, OW, C, dtype=torch.uint8, device=x.device)
        _check(_L().pha_maxpool2d_nhwc_fwd(_DT[x.dtype], _ptr(x), _ptr(y), _ptr(idx), N, H, W, C, OH, OW,
                                           k[0], k[1], s[0], s[1], p[0], p[1], _stream(x)), "maxpool2d_nhwc_fwd")
        ctx.save_for_backward(idx)
        ctx.conf = (x.shape, k, s, p)
        return y

    @staticmethod
    def backward(ctx, gy):
        idx, = ctx.saved_tensors
        (N, H, W, C), k, s, p = ctx.conf
        gy = gy.contiguous()
        gx = torch.empty(N, H, W, C, dtype=gy.dtype, device=gy.device)
        _check(_L().pha_maxpool2d_nhwc_bwd(_DT[gy.dtype], _ptr(gy), _ptr(idx), _ptr(gx), N, H, W, C, idx.shape[1],
                                           idx.shape[2], k[0], k[1], s[0], s[1], p[0], p[1], _stream(gy)),
               "maxpool2d_nhwc_bwd")
        return gx, None, None, None


def maxpool_nhwc_ok(x, k, s, p):
    return (x.is_cuda and x.dim() == 4 and x.dtype in _DT and x.shape[-1] % 8 == 0 and x.is_contiguous()
            and k[0] * k[1] <= 256 and p[0] < k[0] and p[1] < k[1])


def embedding_fwd(ids, w):
    ids = ids.to(torch.int64)
    rows = ids.numel()
    D = w.shape[1]
    out = torch.empty(list(ids.shape) + [D], dtype=w.dtype, device=w.device)
    if rows == 0:
        return out
    _check(_L().pha_embedding_fwd(_ptr(ids), _ptr(w), _ptr(out), rows, D * w.element_size(), w.shape[0], _stream(w)), "embedding_fwd")
    return out


def embedding_bwd(ids, gy, vocab, padding_idx=None):
    """dW [vocab, D] of an embedding lookup: deterministic (token-order sums, no atomics, no sort)"""
    ids = ids.reshape(-1).to(torch.int64).contiguous()
    D = gy.shape[-1]
    gy2 = gy.reshape(-1, D).contiguous()
    gw = torch.empty(vocab, D, dtype=gy.dtype, device=gy.device)
    pad = -1 if padding_idx is None else int(padding_idx) % vocab
    n = ids.numel()
    # a small vocabulary (token types, positions) gives few (row, column) blocks: split the tokens
    # into chunks (>= 1024 tokens each) so ~512 blocks stream them, fp32 partials summed in order
    blocks = -(-vocab // 32) * -(-D // 1024)
    chunks = 1
    if blocks < 512 and n >= 2048:
        chunks = max(1, min(-(-512 // blocks), n // 1024, 65535))
    ws = torch.empty(chunks, vocab, D, dtype=torch.float32, device=gy.device) if chunks > 1 else None
    _check(_L().pha_embedding_bwd(_DT[gy.dtype], _ptr(ids), _ptr(gy2), _ptr(gw), n, D, vocab, pad,
                                  _stream(gy), chunks, _ptr(ws)), "embedding_bwd")
    return gw


def embedding_bwd_supported(gy, n):
    return gy.dtype in _DT and gy.shape[-1] % 4 == 0 and n < (1 << 26) and n > 0


# ----------------------------------------------------------------------------
# multi-tensor optimizers
# ----------------------------------------------------------------------------
_META_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("master", "<u8"),
                     ("n", "<i8"), ("lr", "<f4"), ("wd", "<f4")])
_NORM_DT = np.dtype([("x", "<u8"), ("n", "<i8"), ("dt", "<i4"), ("pad", "<i4")])


def _chunk():
    return _L().pha_chunk_size()


class _CaptureStaging:
    """Page-locked host staging for pointer tables built while a hipGraph is being captured.
    torch's pinned caching allocator records an event on the capturing stream, which HIP refuses,
    so a table uploaded during capture is written into a block of this hipHostMalloc arena
    (allocated on the first eager upload, i.e. before any capture) and copied by a
    hipMemcpyAsync that the graph records as a memcpy node. Blocks are never reused: the graph
    re-reads them on every replay."""
    SIZE = 8 << 20

    def __init__(self):
        import ctypes
        self._ct = ctypes
        self._hip = ctypes.CDLL("libamdhip64.so")
        self._hip.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
        self._hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                             ctypes.c_void_p]
        p = ctypes.c_void_p()
        rc = self._hip.hipHostMalloc(ctypes.byref(p), self.SIZE, 0)
        if rc != 0:
            raise RuntimeError(f"hipHostMalloc failed ({rc})")
        self._base, self._used = p.value, 0

    def upload(self, raw, device):
        n = raw.nbytes
        off = (self._used + 255) & ~255
        if off + n > self.SIZE:
            raise RuntimeError("hipGraph capture staging exhausted (pointer tables of too many captures)")
        self._used = off + n
        self._ct.memmove(self._base + off, raw.ctypes.data, n)
        dst = torch.empty(n, dtype=torch.uint8, device=device)
        rc = self._hip.hipMemcpyAsync(dst.data_ptr(), self._base + off, n, 1,
                                      torch.cuda.current_stream(device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed during capture ({rc})")
        return dst


_staging = None


def _upload(arr, device):
    global _staging
    raw = np.ascontiguousarray(arr.view(np.uint8))
    if torch.cuda.is_current_stream_capturing():
        if _staging is None:
            raise RuntimeError("pointer tables built during a hipGraph capture need one eager step first")
        return _staging.upload(raw, device)
    if _staging is None and torch.cuda.is_available():
        _staging = _CaptureStaging()
    host = torch.from_numpy(raw.copy()).pin_memory()
    return host.to(device, non_blocking=True)


def _group_by_dtype(items, key):
    groups = {}
    for it in items:
        groups.setdefault(key(it), []).append(it)
    return groups


class _TablePlan:
    """Cached (metas, chunks) device tables for a fixed list of tensors."""

    def __init__(self):
        self.key = None
        self.tables = None


_plans = {}


def _build_tables(recs, device, chunk):
    meta = np.zeros(len(recs), dtype=_META_DT)
    chunks = []
    for i, r in enumerate(recs):
        meta[i] = r
        n = int(r[5])
        for c in range((n + chunk - 1) // chunk):
            chunks.append((i, c))
    ch = np.asarray(chunks, dtype=np.int32).reshape(-1, 2)
    return _upload(meta, device), _upload(ch, device), len(chunks)


def _tables_cached(tag, recs, device):
    """Pointer tables are rebuilt only when any pointer/size changes (steady state: cached)."""
    key = tuple(tuple(r[:6]) + (r[6], r[7]) for r in recs)
    plan = _plans.get(tag)
    if plan is not None and plan[0] == key:
        return plan[1]
    t = _build_tables(recs, device, _chunk())
    _plans[tag] = (key, t)
    return t


def _flat_ok(fn, what, t, dev, n, dtype=None):
    """One buffer a kernel walks as ``n`` flat elements through its raw pointer: attribute reads
    only (this runs for every tensor on every step), ValueError before anything is launched."""
    if dtype is None:
        if t.dtype not in _DT:
            raise ValueError(f"{fn}: {what} has dtype {t.dtype}; the kernels take float32, bfloat16 and float16")
    elif t.dtype != dtype:
        raise ValueError(f"{fn}: {what} must be {dtype}, got {t.dtype}")
    if t.device != dev:
        raise ValueError(f"{fn}: {what} is on {t.device}, expected {dev}")
    if t.numel() != n:
        raise ValueError(f"{fn}: {what} has {t.numel()} elements, expected {n}")
    if not t.is_contiguous():
        raise ValueError(f"{fn}: {what} is not contiguous (the kernel would walk its storage as if flat)")


def _dev_scalar_ok(fn, what, t, dev):
    if t is not None and (t.dtype != torch.float32 or t.device != dev or t.numel() < 1):
        raise ValueError(f"{fn}: {what} must be a float32 scalar on {dev}")


def _mt_precheck(fn, params, grads, states, masters):
    """Preconditions of the multi-tensor optimizer kernels, for every entry that has a gradient:
    parameter, gradient, state tensors and master are contiguous, on one device, of the
    parameter's numel; state and master are fp32; parameter and gradient dtypes are in ``_DT``."""
    dev = params[0].device
    if dev.type != "cuda":
        raise ValueError(f"{fn}: parameters are on {dev}; the kernels need device tensors")
    for i, p in enumerate(params):
        g = grads[i]
        if g is None:
            continue
        n = p.numel()
        _flat_ok(fn, f"params[{i}]", p, dev, n)
        _flat_ok(fn, f"grads[{i}]", g, dev, n)
        for name, st in states:
            _flat_ok(fn, f"{name}[{i}]", st[i], dev, n, torch.float32)
        if masters is not None and masters[i] is not None:
            _flat_ok(fn, f"masters[{i}]", masters[i], dev, n, torch.float32)
    return dev


def multi_tensor_adam(params, grads, ms, vs, masters, lr, beta1, beta2, eps, step, weight_decay, decoupled,
                      lr_ratios, grad_scale, wds=None, gscale_dev=None, lr_dev=None, pow_dev=None):
    """gscale_dev: optional fp32 device scalar multiplied into every gradient as it is read (the
    global-norm clip factor — no separate pass over the gradients). lr_dev / pow_dev: fp32 device
    scalars (learning rate; (beta1^t, beta2^t) before this update) read by the kernel instead of
    the host values — what a hipGraph-captured step needs so that replays advance."""
    L = _L()
    dev = _mt_precheck("multi_tensor_adam", params, grads, (("ms", ms), ("vs", vs)), masters)
    _dev_scalar_ok("multi_tensor_adam", "gscale_dev", gscale_dev, dev)
    _dev_scalar_ok("multi_tensor_adam", "lr_dev", lr_dev, dev)
    if pow_dev is not None:
        _dev_scalar_ok("multi_tensor_adam", "pow_dev[0]", pow_dev[0], dev)
        _dev_scalar_ok("multi_tensor_adam", "pow_dev[1]", pow_dev[1], dev)
    items = []
    for i, p in enumerate(params):
        g = grads[i]
        if g is None:
            continue
        mst = masters[i] if masters is not None else None
        wd = wds[i] if wds is not None else weight_decay
        rec = (p.data_ptr(), g.data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(), 0 if mst is None else mst.data_ptr(),
               p.numel(), float(lr_ratios[i]) if lr_ratios is not None else 1.0, float(wd))
        items.append((p.dtype, g.dtype, rec))
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    stream = _stream(params[0])
    for (pdt, gdt), its in _group_by_dtype(items, lambda t: (t[0], t[1])).items():
        metas, chunks, n = _tables_cached(("adam", pdt, gdt), [t[2] for t in its], dev)
        _check(L.pha_multi_tensor_adam(_DT[pdt], _DT[gdt], _ptr(metas), _ptr(chunks), n, float(lr), float(beta1), float(beta2),
                                       float(eps), float(bc1), float(bc2), float(grad_scale), int(bool(decoupled)),
                                       _ptr(gscale_dev), _ptr(lr_dev), _ptr(None if pow_dev is None else pow_dev[0]),
                                       _ptr(None if pow_dev is None else pow_dev[1]), stream),
               "multi_tensor_adam")
    _bump([p for p, g in zip(params, grads) if g is not None])


def multi_tensor_momentum(params, grads, vels, masters, lr, mu, nesterov, weight_decay, lr_ratios, grad_scale, wds=None):
    L = _L()
    dev = _mt_precheck("multi_tensor_momentum", params, grads, (("vels", vels),), masters)
    items = []
    for i, p in enumerate(params):
        g = grads[i]
        if g is None:
            continue
        mst = masters[i] if masters is not None else None
        wd = wds[i] if wds is not None else weight_decay
        rec = (p.data_ptr(), g.data_ptr(), vels[i].data_ptr(), 0, 0 if mst is None else mst.data_ptr(), p.numel(),
               float(lr_ratios[i]) if lr_ratios is not None else 1.0, float(wd))
        items.append((p.dtype, g.dtype, rec))
    stream = _stream(params[0])
    for (pdt, gdt), its in _group_by_dtype(items, lambda t: (t[0], t[1])).items():
        metas, chunks, n = _tables_cached(("mom", pdt, gdt), [t[2] for t in its], dev)
        _check(L.pha_multi_tensor_momentum(_DT[pdt], _DT[gdt], _ptr(metas), _ptr(chunks), n, float(lr), float(mu),
                                           float(grad_scale), int(bool(nesterov)), stream), "multi_tensor_momentum")
    _bump([p for p, g in zip(params, grads) if g is not None])


def _bump(params):
    """The multi-tensor kernels write parameters through raw pointers, invisible to torch's
    version counters: bump them, so version-keyed caches of derived layouts (conv filter
    re-layouts, transposed linear weights) and autograd's saved-tensor checks see the update."""
    if params:
        torch.autograd.graph.increment_version(params)


def multi_tensor_l2norm_sq(tensors):
    L = _L()
    dev = tensors[0].device
    chunk = _chunk()
    meta = np.zeros(len(tensors), dtype=_NORM_DT)
    chunks = []
    for i, t in enumerate(tensors):
        assert t.is_contiguous()
        meta[i] = (t.data_ptr(), t.numel(), _DT[t.dtype], 0)
        for c in range((t.numel() + chunk - 1) // chunk):
            chunks.append((i, c))
    ch = np.asarray(chunks, dtype=np.int32).reshape(-1, 2)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    partial = torch.empty(max(1, len(chunks)), dtype=torch.float32, device=dev)
    meta_d = _upload(meta, dev)   # keep the device tables alive until the launch is enqueued
    ch_d = _upload(ch, dev)
    _check(L.pha_multi_tensor_l2sq(_ptr(meta_d), _ptr(ch_d), len(chunks), _ptr(partial), _ptr(out), _stream(tensors[0])),
           "multi_tensor_l2sq")
    # the caching allocator may hand these blocks out again once freed; tie them to the stream
    meta_d.record_stream(torch.cuda.current_stream(dev))
    ch_d.record_stream(torch.cuda.current_stream(dev))
    return out[0]


# ----------------------------------------------------------------------------
# LAMB over a flat fp32 shard (csrc/kernels/lamb.hip)
# ----------------------------------------------------------------------------
_LAMB_MAX_BLOCKS = 8192   # lamb.hip's grid_for(): the scratch lamb_sq needs


def _lamb_tables_ok(fn, pid, n, dev, per_param):
    """pid: int32 [n] element -> parameter id map; per_param: (name, tensor, numel) fp32 tables
    indexed by it. The id VALUES must lie in [0, npar): that is the caller's contract (reading
    them here would be a device sync per step)."""
    _flat_ok(fn, "pid", pid, dev, n, torch.int32)
    for name, t, numel in per_param:
        _flat_ok(fn, name, t, dev, numel, torch.float32)


def lamb_sq(g):
    """Sum of squares of the flat fp32 gradient shard ``g`` as a [1] fp32 device tensor
    (deterministic two-level reduction; the global-norm clip's input)."""
    L = _L()
    dev = g.device
    if dev.type != "cuda":
        raise ValueError(f"lamb_sq: g is on {dev}; the kernels need device tensors")
    _flat_ok("lamb_sq", "g", g, dev, g.numel(), torch.float32)
    part = torch.empty(_LAMB_MAX_BLOCKS, dtype=torch.float32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    _check(L.pha_lamb_sq(_ptr(g), g.numel(), _ptr(part), _ptr(out), _stream(g)), "lamb_sq")
    return out


def lamb_moment(g, m1, m2, w, pid, wd, norms, b1, b2, bc1, bc2, eps, gmul=1.0, clip=0.0, gsq=None):
    """In place over the shard: g *= gmul * clip / max(sqrt(gsq), clip) (the clip factor only when
    ``clip`` > 0; ``gsq`` is then the all-reduced [1] square sum on the device), moments m1 / m2
    (bias corrections bc = 1 - beta^t), the LAMB direction r written over ``g``, and the
    per-parameter sums of w^2 and r^2 ADDED into ``norms`` ([2, npar] fp32, zeroed by the caller;
    npar counts the padding slot, the last id)."""
    L = _L()
    fn = "lamb_moment"
    dev, n = g.device, g.numel()
    if dev.type != "cuda":
        raise ValueError(f"{fn}: g is on {dev}; the kernels need device tensors")
    for name, t in (("g", g), ("m1", m1), ("m2", m2), ("w", w)):
        _flat_ok(fn, name, t, dev, n, torch.float32)
    npar = wd.numel()
    _lamb_tables_ok(fn, pid, n, dev, (("wd", wd, npar), ("norms", norms, 2 * npar)))
    if clip > 0:
        if gsq is None:
            raise ValueError(f"{fn}: clip > 0 needs the gradient square sum gsq")
        _dev_scalar_ok(fn, "gsq", gsq, dev)
    _check(L.pha_lamb_moment(_ptr(g), _ptr(m1), _ptr(m2), _ptr(w), _ptr(pid), _ptr(wd), _ptr(norms), npar, n,
                             float(b1), float(b2), float(bc1), float(bc2), float(eps), float(gmul),
                             float(clip) if clip > 0 else 0.0, _ptr(gsq) if clip > 0 else None, _stream(g)), fn)


def lamb_apply(w, r, pid, norms, lr_ratio, lr, lr_dev=None):
    """w -= lr * lr_ratio[p] * trust[p] * r with trust = sqrt(norms[0, p] / norms[1, p]) (1 when
    either sum is 0). ``lr_dev``: optional fp32 device scalar read instead of the host ``lr``."""
    L = _L()
    fn = "lamb_apply"
    dev, n = w.device, w.numel()
    if dev.type != "cuda":
        raise ValueError(f"{fn}: w is on {dev}; the kernels need device tensors")
    _flat_ok(fn, "w", w, dev, n, torch.float32)
    _flat_ok(fn, "r", r, dev, n, torch.float32)
    npar = lr_ratio.numel()
    _lamb_tables_ok(fn, pid, n, dev, (("lr_ratio", lr_ratio, npar), ("norms", norms, 2 * npar)))
    _dev_scalar_ok(fn, "lr_dev", lr_dev, dev)
    _check(L.pha_lamb_apply(_ptr(w), _ptr(r), _ptr(pid), _ptr(norms), _ptr(lr_ratio), npar, n, float(lr),
                            _ptr(lr_dev), _stream(w)), fn)


# ----------------------------------------------------------------------------
# flash attention (csrc/kernels/flash_attn.hip)
# ----------------------------------------------------------------------------
def flash_attn_supported(q, k, v, dropout_p, mask=None):
    """shapes the own kernels take: bf16/fp16 [B, S, H, D] with D <= 256 (32 / 64 / 128 / 256
    natively, other multiples of 8 zero-padded up; 256 on the generic 4-wave kernels), GQA (H % Hk == 0); optional additive / boolean mask
    broadcastable to [B, H, S, Sk] that needs no gradient; optional dropout"""
    import os
    if os.environ.get("PHA_DISABLE_FLASH") == "1":
        return False
    if _lib.lib is None:
        return False
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        return False
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        return False
    B, S, H, D = q.shape
    if D > 256 or D % 8 or k.shape != v.shape or k.shape[0] != B or k.shape[3] != D:
        return False
    if D > 128 and os.environ.get("PHA_FA_WIDE", "sdpa") != "own":
        # head dims 129-256 run on the generic 4-wave kernels at one wave per SIMD (the backward
        # spills): correct and tested, but 2.5x slower than torch SDPA at D = 256
        # (profiles/fa_d256_r3.log) — opt in with PHA_FA_WIDE=own
        return False
    if H % k.shape[2] != 0:
        return False
    if dropout_p and not (0.0 < dropout_p < 1.0):
        return False
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.requires_grad or mask.dim() > 4:
            return False
        try:
            torch.broadcast_shapes(tuple(mask.shape), (B, H, S, k.shape[1]))
        except RuntimeError:
            return False
    return True


def _fa_head_dim(D):
    return D if D in (32, 64, 128, 256) else (64 if D < 64 else 128 if D < 128 else 256)


def _fa_bias(mask, B, H, S, Sk, device):
    """additive fp32 bias view [B, H, S, Sk] (broadcast dims stride 0, keys contiguous) and its
    (batch, head, query) element strides"""
    if mask.dtype == torch.bool:
        mask = torch.zeros(mask.shape, dtype=torch.float32, device=device).masked_fill_(~mask.to(device), float("-inf"))
    else:
        mask = mask.to(device=device, dtype=torch.float32)
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    if mask.stride(-1) != 1 and mask.shape[-1] != 1:
        mask = mask.contiguous()
    if mask.shape[-1] == 1:   # broadcast over keys: materialise the key dimension
        mask = mask.expand(*mask.shape[:-1], Sk).contiguous()
    mask = mask.expand(B, H, S, Sk)
    return mask, (mask.stride(0), mask.stride(1), mask.stride(2))


def _fa64_on(D, mask, Sk=None):
    """head dim 64: the 8-wave LDS-DMA kernels of flash_attn_d64.hip (packed strides, in-kernel
    dropout whose keep bits the forward stores for the backward, an additive mask read as float4 key
    quads: Sk % 4 == 0); PHA_FA64=0 keeps the generic 4-wave kernels"""
    import os
    return (D == 64 and (mask is None or (Sk is not None and Sk % 4 == 0)) and _lib.lib is not None
            and os.environ.get("PHA_FA64", "1") != "0")


def _fa64_bias(mask, B, H, S, Sk, device):
    """(bias view, (sb, sh, sq)) for the D = 64 kernels, or (None, (0, 0, 0))"""
    if mask is None:
        return None, (0, 0, 0)
    bias, st = _fa_bias(mask, B, H, S, Sk, device)
    if bias.data_ptr() % 16 or any(x % 4 for x in st):
        bias = bias.contiguous()
        st = (bias.stride(0), bias.stride(1), bias.stride(2))
    return bias, st


def _fa64_fwd(dt, qp, kp, vp, o, lse, B, S, Sk, H, Hk, sc, causal, qs, kvs, os_, dropout_p, seed, seed_dev, st,
              bias=None, bst=(0, 0, 0)):
    """qs / kvs / os_: (token, head) element strides of q, k / v and o. With dropout, returns the keep
    mask as bits (int32 [B * H][words][S up to 64]) for the backward — the reference fused attention keeps
    its dropout mask too (fmha_ref.h dropout_mask_out); PHA_FA64_MASKBITS=0 re-hashes instead"""
    import os
    L = _L()
    dmask = None
    if dropout_p and os.environ.get("PHA_FA64_MASKBITS", "1") != "0":
        dmask = torch.empty(L.pha_fa64_mask_size(B, H, S, Sk), dtype=torch.int32, device=o.device)
    _check(L.pha_fa64_fwd(dt, qp, kp, vp, _ptr(o), _ptr(lse), B, S, Sk, H, Hk, sc, int(causal), qs[0], qs[1], kvs[0],
                          kvs[1], os_[0], os_[1], float(dropout_p), seed, _ptr(seed_dev), st, _ptr(dmask),
                          _ptr(bias), bst[0], bst[1], bst[2]),
           "fa64_fwd")
    return dmask


def _fa64_bwd(dt, qp, kp, vp, do, lse, delta, dqp, dkp, dvp, B, S, Sk, H, Hk, sc, causal, qs, kvs, gqs, gkvs,
              dropout_p, seed, seed_dev, st, dmask=None, bias=None, bst=(0, 0, 0)):
    L = _L()
    _check(L.pha_fa64_bwd(dt, qp, kp, vp, _ptr(do), _ptr(lse), _ptr(delta), dqp, dkp, dvp, B, S, Sk, H, Hk, sc,
                          int(causal), qs[0], qs[1], kvs[0], kvs[1], H * 64, 64, gqs[0], gqs[1], gkvs[0], gkvs[1],
                          float(dropout_p), seed, _ptr(seed_dev), st, _ptr(dmask), _ptr(bias), bst[0], bst[1],
                          bst[2]), "fa64_bwd")


class FlashAttentionExt(torch.autograd.Function):
    """Flash attention with an additive mask and / or dropout (4-wave kernels, head dims
    32 / 64 / 128): the dropout mask is a counter-based hash of (seed, b*H+h, query, key),
    regenerated in the backward instead of stored."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, mask, dropout_p):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, S, H, D = q.shape
        Sk, Hk = k.shape[1], k.shape[2]
        sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
        bias, (sb, sh, sq) = (None, (0, 0, 0)) if mask is None else _fa_bias(mask, B, H, S, Sk, q.device)
        seed, seed_dev = dropout_seed(q.device) if dropout_p else (0, None)
        o = torch.empty_like(q)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        ctx.fa64 = _fa64_on(D, mask, Sk)
        if ctx.fa64:
            b64, bst = _fa64_bias(mask, B, H, S, Sk, q.device)
            ctx.dmask = _fa64_fwd(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), o, lse, B, S, Sk, H, Hk, sc, causal,
                                  (H * D, D), (Hk * D, D), (H * D, D), dropout_p, seed, seed_dev, _stream(q),
                                  b64, bst)
            ctx.save_for_backward(q, k, v, o, lse)
            ctx.bias, ctx.strides, ctx.seed, ctx.seed_dev = b64, bst, seed, seed_dev
            ctx.causal, ctx.scale, ctx.dropout_p = causal, sc, float(dropout_p)
            return o
        _check(_L().pha_flash_attn_fwd_ext(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), B, S, Sk, H, Hk,
                                           D, sc, int(causal), _ptr(bias), sb, sh, sq, float(dropout_p), seed,
                                           _stream(q), _ptr(seed_dev)), "flash_attn_fwd_ext")
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.bias, ctx.strides, ctx.seed, ctx.seed_dev = bias, (sb, sh, sq), seed, seed_dev
        ctx.causal, ctx.scale, ctx.dropout_p = causal, sc, float(dropout_p)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        do = do.contiguous()
        B, S, H, D = q.shape
        Sk, Hk = k.shape[1], k.shape[2]
        L = _L()
        delta = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        dq = torch.empty_like(q)
        dk = torch.empty_like(k) if Hk == H else torch.empty((B, Sk, H, D), dtype=k.dtype, device=k.device)
        dv = torch.empty_like(v) if Hk == H else torch.empty((B, Sk, H, D), dtype=v.dtype, device=v.device)
        _check(L.pha_flash_attn_bwd_preprocess(_DT[q.dtype], _ptr(o), _ptr(do), _ptr(delta), B, S, H, D, _stream(q)),
               "flash_attn_bwd_preprocess")
        if getattr(ctx, "fa64", False):
            _fa64_bwd(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), do, lse, delta, _ptr(dq), _ptr(dk), _ptr(dv), B, S, Sk,
                      H, Hk, ctx.scale, ctx.causal, (H * D, D), (Hk * D, D), (0, 0), (0, 0), ctx.dropout_p, ctx.seed,
                      ctx.seed_dev, _stream(q), ctx.dmask, ctx.bias, ctx.strides)
        else:
            sb, sh, sq = ctx.strides
            _check(L.pha_flash_attn_bwd_ext(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), _ptr(do), _ptr(lse), _ptr(delta),
                                            _ptr(dq), _ptr(dk), _ptr(dv), B, S, Sk, H, Hk, D, ctx.scale,
                                            int(ctx.causal), _ptr(ctx.bias), sb, sh, sq, ctx.dropout_p, ctx.seed,
                                            _stream(q), 0, 0, 0, 0, _ptr(ctx.seed_dev)),
                   "flash_attn_bwd_ext")
        if Hk != H:
            g = H // Hk
            dk = dk.view(B, Sk, Hk, g, D).sum(3)
            dv = dv.view(B, Sk, Hk, g, D).sum(3)
        return dq, dk, dv, None, None, None, None


class FlashAttentionExtPacked(torch.autograd.Function):
    """FlashAttentionExt on a packed [B, S, H, 3D] projection (q | k | v per head, the BERT / fused
    QKV layout): the forward takes dense copies of the three slices, the backward writes dq / dk /
    dv straight into ONE packed [B, S, H, 3D] gradient through the kernels' output strides — no
    concatenation pass (0.67 ms per BERT-base step, profiles/README.md round 5)"""

    @staticmethod
    def forward(ctx, qkv, causal, scale, mask, dropout_p):
        B, S, H, D3 = qkv.shape
        D = D3 // 3
        ctx.fa64p = _fa64_on(D, mask, S) and qkv.is_contiguous()
        if ctx.fa64p:   # head dim 64: the kernels read q | k | v in place (no slice copies)
            sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
            seed, seed_dev = dropout_seed(qkv.device) if dropout_p else (0, None)
            o = torch.empty((B, S, H, D), dtype=qkv.dtype, device=qkv.device)
            lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
            es, base = qkv.element_size(), qkv.data_ptr()
            b64, bst = _fa64_bias(mask, B, H, S, S, qkv.device)
            ctx.dmask = _fa64_fwd(_DT[qkv.dtype], base, base + D * es, base + 2 * D * es, o, lse, B, S, S, H, H, sc,
                                  causal, (3 * H * D, 3 * D), (3 * H * D, 3 * D), (H * D, D), dropout_p, seed, seed_dev,
                                  _stream(qkv), b64, bst)
            ctx.b64, ctx.bst = b64, bst
            ctx.save_for_backward(qkv, o, lse)
            ctx.seed, ctx.seed_dev, ctx.causal, ctx.scale, ctx.dropout_p = seed, seed_dev, causal, sc, float(dropout_p)
            return o
        q, k, v = (qkv[..., i * D:(i + 1) * D].contiguous() for i in range(3))
        o = FlashAttentionExt.forward(ctx, q, k, v, causal, scale, mask, dropout_p)
        return o

    @staticmethod
    def backward(ctx, do):
        if ctx.fa64p:
            qkv, o, lse = ctx.saved_tensors
            do = do.contiguous()
            B, S, H, D3 = qkv.shape
            D = D3 // 3
            L = _L()
            delta = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
            g = torch.empty_like(qkv)
            _check(L.pha_flash_attn_bwd_preprocess(_DT[qkv.dtype], _ptr(o), _ptr(do), _ptr(delta), B, S, H, D,
                                                   _stream(qkv)), "flash_attn_bwd_preprocess")
            es, base, gb = qkv.element_size(), qkv.data_ptr(), g.data_ptr()
            st = (3 * H * D, 3 * D)
            _fa64_bwd(_DT[qkv.dtype], base, base + D * es, base + 2 * D * es, do, lse, delta, gb, gb + D * es,
                      gb + 2 * D * es, B, S, S, H, H, ctx.scale, ctx.causal, st, st, st, st, ctx.dropout_p, ctx.seed,
                      ctx.seed_dev, _stream(qkv), ctx.dmask, ctx.b64, ctx.bst)
            return g, None, None, None, None
        q, k, v, o, lse = ctx.saved_tensors
        do = do.contiguous()
        B, S, H, D = q.shape
        L = _L()
        delta = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        g = torch.empty((B, S, H, 3 * D), dtype=q.dtype, device=q.device)
        _check(L.pha_flash_attn_bwd_preprocess(_DT[q.dtype], _ptr(o), _ptr(do), _ptr(delta), B, S, H, D, _stream(q)),
               "flash_attn_bwd_preprocess")
        sb, sh, sq = ctx.strides
        es = g.element_size()
        base = g.data_ptr()
        _check(L.pha_flash_attn_bwd_ext(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), _ptr(do), _ptr(lse), _ptr(delta),
                                        base, base + D * es, base + 2 * D * es, B, S, S, H, H, D, ctx.scale,
                                        int(ctx.causal), _ptr(ctx.bias), sb, sh, sq, ctx.dropout_p, ctx.seed,
                                        _stream(q), 3 * H * D, 3 * D, 3 * H * D, 3 * D, _ptr(ctx.seed_dev)),
               "flash_attn_bwd_ext(packed)")
        return g, None, None, None, None


def flash_attention_packed_ext(qkv, causal, scale, mask=None, dropout_p=0.0):
    """attention over a packed [B, S, H, 3D] projection with a mask and / or dropout (head dims 32 /
    64 / 128 / 256); None when the ext kernels cannot take it (the caller splits instead)"""
    B, S, H, D3 = qkv.shape
    D = D3 // 3
    if D3 % 3 or D not in (32, 64, 128, 256) or not qkv.is_cuda or qkv.dtype not in (torch.bfloat16, torch.float16):
        return None
    q = qkv[..., :D]
    if not flash_attn_supported(q, q, q, dropout_p, mask):
        return None
    sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
    return FlashAttentionExtPacked.apply(qkv, bool(causal), sc, mask, float(dropout_p))


def flash_attention_any(q, k, v, causal, scale, mask=None, dropout_p=0.0):
    """dispatch: the 8-wave D=128 / 4-wave D=64 kernels without mask or dropout, the extension
    kernels otherwise; head dims other than 32 / 64 / 128 are zero-padded up"""
    D = q.shape[-1]
    Dp = _fa_head_dim(D)
    sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
    if Dp != D:
        pad = (0, Dp - D)
        q, k, v = (torch.nn.functional.pad(t, pad) for t in (q, k, v))
    if mask is None and not dropout_p and Dp in (64, 128):
        o = FlashAttention.apply(q, k, v, bool(causal), sc)
    else:
        o = FlashAttentionExt.apply(q, k, v, bool(causal), sc, mask, float(dropout_p or 0.0))
    return o[..., :D] if Dp != D else o


def _bwd_fused(D):
    """Single-kernel backward (dK, dV and atomically summed dQ) when PHA_FA_BWD=fused; the default
    is the two-kernel v2 backward, measured faster at the GPT shape (0.95 vs 1.14 ms, B8 S2048
    H16 D128 causal: the fused kernel's one wave per SIMD exposes its LDS latency)."""
    import os
    return D == 128 and os.environ.get("PHA_FA_BWD", "v2") == "fused" and os.environ.get("PHA_FA_BWD_V1") != "1"


class FlashAttention(torch.autograd.Function):
    """Forward/backward on our MFMA flash-attention kernels. Layout [B, S, H, D]."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, S, H, D = q.shape
        Sk, Hk = k.shape[1], k.shape[2]
        sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
        o = torch.empty_like(q)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        ctx.fa64 = _fa64_on(D, None)
        if ctx.fa64:
            _fa64_fwd(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), o, lse, B, S, Sk, H, Hk, sc, causal, (H * D, D),
                      (Hk * D, D), (H * D, D), 0.0, 0, None, _stream(q))
        else:
            _check(_L().pha_flash_attn_fwd(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), B, S, Sk, H, Hk,
                                           D, sc, int(causal), _stream(q)), "flash_attn_fwd")
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        ctx.scale = sc
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        do = do.contiguous()
        B, S, H, D = q.shape
        Sk, Hk = k.shape[1], k.shape[2]
        L = _L()
        delta = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        dq = torch.empty_like(q)
        dk = torch.empty_like(k) if Hk == H else torch.empty((B, Sk, H, D), dtype=k.dtype, device=k.device)
        dv = torch.empty_like(v) if Hk == H else torch.empty((B, Sk, H, D), dtype=v.dtype, device=v.device)
        _check(L.pha_flash_attn_bwd_preprocess(_DT[q.dtype], _ptr(o), _ptr(do), _ptr(delta), B, S, H, D,
                                               _stream(q)), "flash_attn_bwd_preprocess")
        if getattr(ctx, "fa64", False):
            _fa64_bwd(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), do, lse, delta, _ptr(dq), _ptr(dk), _ptr(dv), B, S, Sk,
                      H, Hk, ctx.scale, ctx.causal, (H * D, D), (Hk * D, D), (0, 0), (0, 0), 0.0, 0, None, _stream(q))
        elif _bwd_fused(D):
            # single-kernel backward; dQ is summed over key blocks in an fp32 workspace
            acc = torch.empty((B, S, H, D), dtype=torch.float32, device=q.device)
            _check(L.pha_flash_attn_bwd_fused(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), _ptr(do), _ptr(lse),
                                              _ptr(delta), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(acc), B, S, Sk, H, Hk, D,
                                              ctx.scale, int(ctx.causal), _stream(q)), "flash_attn_bwd_fused")
        else:
            _check(L.pha_flash_attn_bwd(_DT[q.dtype], _ptr(q), _ptr(k), _ptr(v), _ptr(do), _ptr(lse), _ptr(delta),
                                        _ptr(dq), _ptr(dk), _ptr(dv), B, S, Sk, H, Hk, D, ctx.scale, int(ctx.causal),
                                        _stream(q)), "flash_attn_bwd")
        if Hk != H:
            g = H // Hk
            dk = dk.view(B, Sk, Hk, g, D).sum(3)
            dv = dv.view(B, Sk, Hk, g, D).sum(3)
        return dq, dk, dv, None, None


def flash_attn_packed_supported(qkv, num_heads):
    """qkv: [B, S, H, 3D] contiguous projection output (q|k|v per head), D == 128."""
    import os
    if os.environ.get("PHA_DISABLE_FLASH") == "1" or os.environ.get("PHA_FA_FWD_V1") == "1" \
            or os.environ.get("PHA_FA_BWD_V1") == "1":
        return False
    return (_lib.lib is not None and qkv.is_cuda and qkv.dim() == 4
            and qkv.dtype in (torch.bfloat16, torch.float16) and qkv.is_contiguous() and qkv.shape[2] == num_heads
            and qkv.shape[3] == 3 * 128)


class FlashAttentionPacked(torch.autograd.Function):
    """Self-attention straight from the fused QKV projection [B, S, H, 3D]: the kernels read q/k/v
    in place (strided) and the backward writes dq/dk/dv into one packed [B, S, H, 3D] gradient,
    so neither the three split copies nor the concat of their gradients exists."""

    @staticmethod
    def forward(ctx, qkv, causal, scale):
        B, S, H, D3 = qkv.shape
        D = D3 // 3
        sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
        o = torch.empty((B, S, H, D), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
        _check(_L().pha_flash_attn_fwd_packed(_DT[qkv.dtype], _ptr(qkv), _ptr(o), _ptr(lse), B, S, H, D, sc,
                                              int(causal), _stream(qkv)), "flash_attn_fwd_packed")
        ctx.save_for_backward(qkv, o, lse)
        ctx.causal, ctx.scale = causal, sc
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        do = do.contiguous()
        B, S, H, D3 = qkv.shape
        D = D3 // 3
        L = _L()
        delta = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
        dqkv = torch.empty_like(qkv)
        if not _bwd_fused(D):
            # delta = rowsum(dO * O) formed inside the dQ kernel (no separate preprocess pass)
            _check(L.pha_flash_attn_bwd_packed_od(_DT[qkv.dtype], _ptr(qkv), _ptr(o), _ptr(do), _ptr(lse),
                                                  _ptr(delta), _ptr(dqkv), B, S, H, D, ctx.scale, int(ctx.causal),
                                                  _stream(qkv)), "flash_attn_bwd_packed_od")
            return dqkv, None, None
        _check(L.pha_flash_attn_bwd_preprocess(_DT[qkv.dtype], _ptr(o), _ptr(do), _ptr(delta), B, S, H, D,
                                               _stream(qkv)), "flash_attn_bwd_preprocess")
        acc = torch.empty((B, S, H, D), dtype=torch.float32, device=qkv.device)
        _check(L.pha_flash_attn_bwd_packed_fused(_DT[qkv.dtype], _ptr(qkv), _ptr(do), _ptr(lse), _ptr(delta),
                                                 _ptr(dqkv), _ptr(acc), B, S, H, D, ctx.scale, int(ctx.causal),
                                                 _stream(qkv)), "flash_attn_bwd_packed_fused")
        return dqkv, None, None


# ----------------------------------------------------------------------------
# split-KV decode attention (csrc/kernels/decode_attn.hip)
# ----------------------------------------------------------------------------
def _decode_attn_chunk():
    return 0 if _lib.lib is None else _lib.lib.pha_decode_attn_chunk()


DECODE_ATTN_CHUNK = _decode_attn_chunk()   # key positions per split (0: library not built)


def _cache_indirection_why_not(cache_indirection, beam_size, B, max_seq, device):
    """why ``cache_indirection`` / ``beam_size`` do not fit B rows and a cache of max_seq positions on
    ``device``, or None (the check decode_attention, decode_attn_supported and the composite share)"""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or beam_size < 1 or B % beam_size:
        return f"beam_size={beam_size!r} must be a positive int that divides the {B} rows"
    t = cache_indirection
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B, max_seq) \
            or t.device != device or not t.is_contiguous():
        return f"cache_indirection must be a contiguous int32 [{B}, {max_seq}] tensor on {device}"
    return None


def decode_attn_supported(qkv, cache, mask=None, device_time_step=False, cache_indirection=None, beam_size=1):
    """what the decode kernel takes: a bf16 / fp16 [B, 3, H, D] QKV product with D in 32 / 64 / 128,
    a [2, B, H, max_seq, D] cache of the same dtype and device, and an optional additive / boolean
    mask broadcastable to [B, H, 1, keys] that needs no gradient (with a device time step its key
    dimension must span the whole cache, or be 1). ``device_time_step`` is a bool or the time-step
    tensor itself, which is then checked too: int32, on the device of ``qkv``, one element (one step
    for the batch) or B elements (a step per batch row). With ``cache_indirection`` (contiguous int32
    [B, max_seq] on the device of ``qkv``) ``beam_size`` must divide B; without it ``beam_size`` must
    be 1"""
    if not DECODE_ATTN_CHUNK:
        return False
    if not (isinstance(qkv, torch.Tensor) and isinstance(cache, torch.Tensor) and qkv.is_cuda and cache.is_cuda):
        return False
    if qkv.dtype not in (torch.bfloat16, torch.float16) or cache.dtype != qkv.dtype or cache.device != qkv.device:
        return False
    if qkv.dim() != 4 or qkv.shape[1] != 3 or cache.dim() != 5:
        return False
    B, _, H, D = qkv.shape
    if D not in (32, 64, 128) or B < 1 or H < 1 or B > 65535 or H > 65535:
        return False
    if isinstance(device_time_step, torch.Tensor):
        t = device_time_step
        if t.dtype != torch.int32 or t.device != qkv.device or t.numel() not in (1, B) or not t.is_contiguous():
            return False
        device_time_step = True
    if tuple(cache.shape[:3]) != (2, B, H) or cache.shape[4] != D or cache.shape[3] < 1 or not cache.is_contiguous():
        return False
    if cache_indirection is None:
        if beam_size != 1:
            return False
    elif _cache_indirection_why_not(cache_indirection, beam_size, B, cache.shape[3], qkv.device) is not None:
        return False
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.requires_grad or mask.dim() > 4 or mask.dim() < 1:
            return False
        if mask.dim() >= 2 and mask.shape[-2] != 1:
            return False
        try:
            torch.broadcast_shapes(tuple(mask.shape[:-1]) + (1,), (B, H, 1, 1))
        except RuntimeError:
            return False
        if device_time_step and mask.shape[-1] != 1 and mask.shape[-1] < cache.shape[3]:
            return False
    return True


def _decode_bias(mask, B, H, need, device):
    """additive fp32 view [B, H, 1, keys] of ``mask`` (broadcast dims stride 0, keys contiguous,
    at least ``need`` of them) and its (batch, head) element strides — _fa_bias for one query row"""
    if mask.dtype == torch.bool:
        mask = torch.zeros(mask.shape, dtype=torch.float32, device=device).masked_fill_(~mask.to(device), float("-inf"))
    else:
        mask = mask.to(device=device, dtype=torch.float32)
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    if mask.shape[-1] == 1:   # broadcast over keys: materialise the key dimension
        mask = mask.expand(*mask.shape[:-1], need).contiguous()
    elif mask.stride(-1) != 1:
        mask = mask.contiguous()
    if mask.shape[-1] < need:
        raise ValueError(f"decode_attention: the mask covers {mask.shape[-1]} keys, the kernel may read {need}")
    mask = mask.expand(B, H, 1, mask.shape[-1])
    return mask, (mask.stride(0), mask.stride(1))


def decode_attention(qkv, qkv_bias, cache, time_step, mask=None, scale=None, cache_indirection=None, beam_size=1):
    """One decode step of cached attention on the split-KV kernels. ``qkv`` [B, 3, H, D] is the raw
    QKV product of the new token and ``qkv_bias`` [3, H, D] (or None) its bias; the biased key and
    value are written to ``cache`` [2, B, H, max_seq, D] at ``time_step`` in place, and the biased,
    scaled query attends over the positions [0, time_step]. ``time_step`` is a Python int (checked
    here) or an int32 device tensor read by the kernels (no host sync; out of range, the cache is
    left alone and the output is NaN): one element is the step of the whole batch, B elements give
    batch row b its own step ``time_step[b]`` (row b appends at it and reads no key above it; a row
    out of range is left alone and gets NaN, the others are unaffected). At B == 1 the two forms
    coincide.

    ``cache_indirection`` (contiguous int32 [B, max_seq] on the device, checked like ``time_step``)
    with ``beam_size`` K (it divides B) is the beam-search form: the rows are groups of K consecutive
    beams, and row b reads key position t < time_step from cache row ``(b // K) * K +
    cache_indirection[b, t]``, so a beam follows its history through its group's cache rows and
    nothing is copied between them. Position ``time_step`` is appended to row b's own cache row;
    ``cache_indirection[b, time_step]`` is not read, and an entry outside [0, K) leaves its key out
    as if masked. The rows of a group must share one step. One entry point serves it with a step
    per row: a Python int or one-element ``time_step`` is broadcast to [B]. Returns [B, 1, H * D]."""
    fn = "decode_attention"
    if isinstance(time_step, torch.Tensor) and isinstance(qkv, torch.Tensor) and qkv.dim() == 4:
        if time_step.dtype != torch.int32 or time_step.device != qkv.device \
                or time_step.numel() not in (1, qkv.shape[0]) or not time_step.is_contiguous():
            raise ValueError(f"{fn}: a tensor time_step must be contiguous int32 on {qkv.device} with one element "
                             f"or one per batch row ({qkv.shape[0]})")
    if cache_indirection is None:
        if beam_size != 1:
            raise ValueError(f"{fn}: beam_size={beam_size!r} needs a cache_indirection table")
    elif isinstance(qkv, torch.Tensor) and qkv.dim() == 4 and isinstance(cache, torch.Tensor) and cache.dim() == 5:
        why = _cache_indirection_why_not(cache_indirection, beam_size, qkv.shape[0], cache.shape[3], qkv.device)
        if why is not None:
            raise ValueError(f"{fn}: {why}")
    if not decode_attn_supported(qkv, cache, mask, isinstance(time_step, torch.Tensor), cache_indirection, beam_size):
        raise ValueError(f"{fn}: unsupported arguments (see decode_attn_supported)")
    B, _, H, D = qkv.shape
    max_seq = cache.shape[3]
    dev = qkv.device
    if not qkv.is_contiguous():
        raise ValueError(f"{fn}: qkv is not contiguous")
    if qkv_bias is not None:
        if tuple(qkv_bias.shape) != (3, H, D) or qkv_bias.dtype != qkv.dtype or qkv_bias.device != dev \
                or not qkv_bias.is_contiguous():
            raise ValueError(f"{fn}: qkv_bias must be a contiguous {qkv.dtype} [3, {H}, {D}] tensor on {dev}")
    ts, ts_dev = 0, None
    if isinstance(time_step, torch.Tensor):
        ts_dev = time_step   # checked above
    else:
        ts = int(time_step)
        if ts < 0 or ts >= max_seq:
            raise ValueError(f"{fn}: time_step {ts} outside the cache's [0, {max_seq})")
    bias, (sb, sh) = (None, (0, 0))
    if mask is not None:
        bias, (sb, sh) = _decode_bias(mask, B, H, max_seq if ts_dev is not None else ts + 1, dev)
    tensors = [qkv, cache] + ([qkv_bias] if qkv_bias is not None else [])
    if any(t.data_ptr() % 16 for t in tensors) or (bias is not None and bias.data_ptr() % 4):
        raise ValueError(f"{fn}: qkv, qkv_bias and cache must be 16-byte aligned")
    nsplit = -(-max_seq // DECODE_ATTN_CHUNK)
    ws = torch.empty((B, H, nsplit, D + 2), dtype=torch.float32, device=dev)
    out = torch.empty((B, 1, H * D), dtype=qkv.dtype, device=dev)
    sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(D))
    if cache_indirection is not None:   # the beam-indirect form always takes a step per row
        if ts_dev is None:
            ts_dev = torch.full((B,), ts, dtype=torch.int32, device=dev)
        elif ts_dev.numel() != B:
            ts_dev = ts_dev.reshape(1).expand(B).contiguous()
        _check(_L().pha_decode_attn_beam(_DT[qkv.dtype], _ptr(qkv), _ptr(qkv_bias), _ptr(cache), _ptr(bias), sb, sh, sc,
                                         _ptr(ts_dev), _ptr(cache_indirection), int(beam_size), _ptr(out), _ptr(ws),
                                         B, H, D, max_seq, _stream(qkv)), fn)
        return out
    if ts_dev is not None and ts_dev.numel() > 1:   # a step per batch row
        _check(_L().pha_decode_attn_rows(_DT[qkv.dtype], _ptr(qkv), _ptr(qkv_bias), _ptr(cache), _ptr(bias), sb, sh, sc,
                                         _ptr(ts_dev), _ptr(out), _ptr(ws), B, H, D, max_seq, _stream(qkv)), fn)
        return out
    _check(_L().pha_decode_attn(_DT[qkv.dtype], _ptr(qkv), _ptr(qkv_bias), _ptr(cache), _ptr(bias), sb, sh, sc, ts,
                                _ptr(ts_dev), _ptr(out), _ptr(ws), B, H, D, max_seq, _stream(qkv)), fn)
    return out


# ----------------------------------------------------------------------------
# weight-streaming GEMM for M <= 16 rows (csrc/kernels/skinny_gemm.hip)
# ----------------------------------------------------------------------------
_SKINNY_ACT = {"none": 0, "gelu": 1, "relu": 2, "gelu_tanh": 3}
SKINNY_GEMM_MAX_M = 16   # one MFMA 16x16x32 row block


def skinny_gemm_tile(w_is_nk):
    """(column tile, K step per iteration) of the kernel for a weight layout"""
    bn, ks = c_int(0), c_int(0)
    _check(_L().pha_skinny_gemm_tile(1 if w_is_nk else 0, ctypes.byref(bn), ctypes.byref(ks)), "skinny_gemm_tile")
    return bn.value, ks.value


def skinny_gemm_plan(N, K, w_is_nk):
    """(nsplit, k_per_split) the kernel uses for an [M, K] x [K, N] product: a function of N, K and the
    weight layout alone (never M or data), so a captured graph stays valid and results reproduce"""
    L = _L()
    ns, kps = c_int(0), c_int(0)
    if int(N) < 1 or int(K) < 1:
        raise ValueError(f"skinny_gemm_plan: N={N} K={K} must be positive")
    _check(L.pha_skinny_gemm_plan(int(N), int(K), 1 if w_is_nk else 0, ctypes.byref(ns), ctypes.byref(kps)),
           "skinny_gemm_plan")
    return ns.value, kps.value


def _skinny_reject(x, w, w_is_nk, bias, residual):
    """why skinny_gemm cannot take these arguments (names the argument), or None"""
    if not (isinstance(x, torch.Tensor) and isinstance(w, torch.Tensor)):
        return "x and w must be tensors"
    if not x.is_cuda:
        return f"x is on {x.device}, not a GPU"
    if x.dtype not in (torch.bfloat16, torch.float16):
        return f"x is {x.dtype}; the kernel takes bfloat16 or float16"
    dev, dt = x.device, x.dtype
    if x.dim() != 2:
        return f"x must be 2-D, got {tuple(x.shape)}"
    if w.dim() != 2:
        return f"w must be 2-D, got {tuple(w.shape)}"
    M, K = x.shape
    if M < 1 or M > SKINNY_GEMM_MAX_M:
        return f"x has M={M} rows; the kernel takes 1 to {SKINNY_GEMM_MAX_M}"
    N, Kw = (w.shape[0], w.shape[1]) if w_is_nk else (w.shape[1], w.shape[0])
    if Kw != K:
        return f"w {tuple(w.shape)} does not match x's K={K} (w_is_nk={bool(w_is_nk)})"
    if K % 8 or N % 8 or K < 8 or N < 8:
        return f"K={K} and N={N} must be positive multiples of 8"
    if x.stride(1) != 1 or x.stride(0) % 8 or x.stride(0) < K:
        return f"x strides {tuple(x.stride())}: the last must be 1 and the first a multiple of 8 that is >= K"
    for name, t, shape in (("w", w, tuple(w.shape)), ("bias", bias, (N,)), ("residual", residual, (M, N))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt:
            return f"{name} must be a {dt} tensor on {dev}"
        if tuple(t.shape) != shape:
            return f"{name} must have shape {shape}, got {tuple(t.shape)}"
        if not t.is_contiguous():
            return f"{name} is not contiguous"
    for name, t in (("x", x), ("w", w), ("bias", bias), ("residual", residual)):
        if t is not None and t.data_ptr() % 16:
            return f"{name} is not 16-byte aligned"
    return None


def skinny_gemm_supported(x, w, w_is_nk, bias=None, residual=None):
    """what skinny_gemm takes: bf16 / fp16 tensors of one dtype on one GPU, x [M, K] with 1 <= M <= 16,
    unit inner stride and a row stride that is a multiple of 8, a contiguous w ([N, K] if ``w_is_nk``
    else [K, N]), K and N multiples of 8, contiguous bias [N] and residual [M, N], every pointer
    16-byte aligned; and an (N, K, layout, M) class that skinny_gemm_excluded does not name"""
    if _lib.lib is None or _skinny_reject(x, w, w_is_nk, bias, residual) is not None:
        return False
    N = w.shape[0] if w_is_nk else w.shape[1]
    return not skinny_gemm_excluded(N, x.shape[1], w_is_nk, x.shape[0])


def skinny_gemm_excluded(N, K, w_is_nk, M=None):
    """(N, K, layout) classes, with the row count where it decides, that lost to the library call plus
    its elementwise passes and therefore stay on the library by default (a policy, not a fallback;
    skinny_gemm itself still takes them). tools/bench_decode_gemm.py part (b) excluded none
    (profiles/decode_gemm/README.md). tools/bench_generate.py part (b) excludes one: the
    vocabulary-sized [N, K] product of the LM head (N * K >= 2^26 elements; measured at 50,304 x 2048)
    with all 16 rows, 51.6 us against 50.9 us on matmul_nt. The same shape with 1 and 8 rows wins and
    stays; 9 - 15 rows were not measured and stay with them (profiles/generate/README.md). ``M`` None
    asks about the shape alone, which is never excluded as a whole."""
    return bool(w_is_nk) and M is not None and int(M) >= 16 and int(N) * int(K) >= (1 << 26)


def skinny_gemm_why_not(x, w, w_is_nk, bias=None, residual=None):
    """the reason skinny_gemm would reject these arguments, for the fallback log"""
    if _lib.lib is None:
        return "kernel library not loaded"
    return _skinny_reject(x, w, w_is_nk, bias, residual) or "supported"


def skinny_gemm(x, w, w_is_nk, bias=None, act="none", residual=None, nsplit=None, out=None):
    """out[M, N] = act(x[M, K] @ W + bias) + residual on the weight-streaming kernels, M <= 16, fp32
    accumulation and one rounding. ``w`` is [N, K] when ``w_is_nk`` else [K, N]; ``act`` is "none",
    "gelu" (erf), "gelu_tanh" (the tanh approximation, bias_gelu's approximate=True) or "relu".
    ``nsplit`` None takes skinny_gemm_plan's deterministic split; an explicit value splits K evenly
    (in multiples of 8) and must leave no split empty. ``out``, if given, is a contiguous, 16-byte
    aligned [M, N] tensor of x's dtype on x's device that receives the result."""
    fn = "skinny_gemm"
    why = _skinny_reject(x, w, w_is_nk, bias, residual)
    if why is not None:
        raise ValueError(f"{fn}: {why}")
    if act not in _SKINNY_ACT:
        raise ValueError(f"{fn}: act must be one of {sorted(_SKINNY_ACT)}, got {act!r}")
    L = _L()
    M, K = x.shape
    N = w.shape[0] if w_is_nk else w.shape[1]
    if nsplit is None:
        ns, kps = skinny_gemm_plan(N, K, w_is_nk)
    else:
        ns = int(nsplit)
        if ns < 1:
            raise ValueError(f"{fn}: nsplit={nsplit} must be at least 1")
        kps = -(-(-(-K // ns)) // 8) * 8
        if (ns - 1) * kps >= K:
            raise ValueError(f"{fn}: nsplit={ns} leaves a split empty at K={K} (k_per_split={kps})")
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != x.dtype or out.device != x.device \
            or tuple(out.shape) != (M, N) or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError(f"{fn}: out must be a contiguous, 16-byte aligned {x.dtype} [{M}, {N}] tensor on {x.device}")
    ws = torch.empty((ns, M, N), dtype=torch.float32, device=x.device) if ns > 1 else None
    _check(L.pha_skinny_gemm(_DT[x.dtype], 1 if w_is_nk else 0, _ptr(x), x.stride(0), _ptr(w), _ptr(bias),
                             _ptr(residual), _ptr(out), _ptr(ws), M, N, K, ns, kps, _SKINNY_ACT[act], _stream(x)), fn)
    return out


# ----------------------------------------------------------------------------
# next-token sampling (csrc/kernels/sampling.hip)
# ----------------------------------------------------------------------------
SAMPLE_MAX_B = 16   # rows per call: the decode step's batch, as SKINNY_GEMM_MAX_M


def _sample_max_v():
    return 0 if _lib.lib is None else _lib.lib.pha_sample_logits_max_v()


SAMPLE_MAX_V = _sample_max_v()   # the kernel's vocabulary limit (0: library not built)


def _row_vector_check(fn, name, t, dtype, n, dev, spelled=None):
    """``t`` must be a contiguous ``dtype`` [n] tensor on ``dev``. ``spelled`` is the dtype as the message
    names it: sample_logits has always said "float32" / "uint8" for ``u`` / ``finished`` where the other
    messages print ``torch.int64`` and the like, and the tests' ``test_rejections`` match on the text."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,) or t.device != dev \
            or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous {spelled or dtype} [{n}] tensor on {dev}")


def _sample_check(logits, u, temperature, top_k, top_p, finished, out_ids=None, out_logprob=None):
    """the argument errors of sample_logits, the same on every path (each names its argument)"""
    fn = "sample_logits"
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"{fn}: logits must be a 2-D tensor [B, V]")
    if logits.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise ValueError(f"{fn}: logits are {logits.dtype}; bfloat16, float16 or float32 expected")
    B, V = logits.shape
    if B < 1 or B > SAMPLE_MAX_B:
        raise ValueError(f"{fn}: logits have B={B} rows; 1 to {SAMPLE_MAX_B} expected")
    if V < 2:
        raise ValueError(f"{fn}: logits have V={V} columns; at least 2 expected")
    if logits.stride(1) != 1 or logits.stride(0) < V:
        raise ValueError(f"{fn}: logits strides {tuple(logits.stride())}: the last must be 1 and the first >= V={V}")
    dev = logits.device
    _row_vector_check(fn, "u", u, torch.float32, B, dev, "float32")
    if not float(temperature) > 0.0:
        raise ValueError(f"{fn}: temperature={temperature} must be positive")
    if not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"{fn}: top_p={top_p} must be in (0, 1]")
    if int(top_k) != top_k or not (0 <= int(top_k) <= V):
        raise ValueError(f"{fn}: top_k={top_k} must be an integer in [0, V={V}]")
    if finished is not None:
        _row_vector_check(fn, "finished", finished, torch.uint8, B, dev, "uint8")
    if out_ids is not None:
        _row_vector_check(fn, "out_ids", out_ids, torch.int64, B, dev)
    if out_logprob is not None:
        _row_vector_check(fn, "out_logprob", out_logprob, torch.float32, B, dev)


def _sample_reject(logits):
    """why the kernel cannot take logits that passed _sample_check, or None"""
    if not logits.is_cuda:
        return f"logits are on {logits.device}, not a GPU"
    if logits.dtype not in (torch.bfloat16, torch.float16):
        return f"logits are {logits.dtype}; the kernel takes bfloat16 or float16"
    if logits.shape[1] > SAMPLE_MAX_V:
        return f"V={logits.shape[1]} is above the kernel's {SAMPLE_MAX_V} (one row of keys plus the histograms in LDS)"
    if logits.data_ptr() % 2:
        return "logits are not 2-byte aligned"
    return None


def sample_logits_excluded(B, V, top_k, top_p):
    """(B, V, filter) classes that lost to the composite in tools/bench_generate.py part (a) and stay on
    it by default (a policy, not a fallback). None: see profiles/generate/README.md."""
    return False


def sample_logits_supported(logits, u, temperature=1.0, top_k=0, top_p=1.0, finished=None):
    """what the sampling kernel takes: bf16 / fp16 logits [B, V] on a GPU with 1 <= B <= 16,
    2 <= V <= SAMPLE_MAX_V (65,536), unit inner stride and a row stride of at least V; float32 u [B];
    temperature > 0, 0 < top_p <= 1, 0 <= top_k <= V; an optional uint8 finished [B]. float32 logits
    are not taken (they stay on the composite)."""
    if _lib.lib is None:
        return False
    try:
        _sample_check(logits, u, temperature, top_k, top_p, finished)
    except ValueError:
        return False
    return _sample_reject(logits) is None and not sample_logits_excluded(logits.shape[0], logits.shape[1], top_k, top_p)


def sample_logits_why_not(logits, u, temperature=1.0, top_k=0, top_p=1.0, finished=None):
    """the reason the sampling kernel would reject these arguments, for the fallback log"""
    if _lib.lib is None:
        return "kernel library not loaded"
    try:
        _sample_check(logits, u, temperature, top_k, top_p, finished)
    except ValueError as e:
        return str(e)
    return _sample_reject(logits) or "supported"


def _sample_logits_composite(logits, u, temperature=1.0, top_k=0, top_p=1.0, finished=None, eos_token_id=-1,
                             pad_token_id=0):
    """sample_logits' contract in plain torch (any device, any float dtype, any B; no host sync)"""
    B, V = logits.shape
    dev = logits.device
    z = logits.float() / float(temperature)
    lsm = torch.log_softmax(z, -1)
    ar = torch.arange(V, device=dev)
    K = int(top_k) if 0 < int(top_k) < V else V
    if int(top_k) == 1:
        ids = torch.where(z == z.max(-1, keepdim=True).values, ar, V).min(-1).values   # lowest index on a tie
    else:
        p = torch.exp(lsm)
        if K < V or float(top_p) < 1.0:
            _, order = torch.sort(z, dim=-1, descending=True, stable=True)
            in_k = (ar < K).unsqueeze(0)
            ps = p.gather(1, order) * in_k
            keep_sorted = in_k.expand(B, V).clone()
            if float(top_p) < 1.0:
                cum = ps.cumsum(-1)
                keep_sorted &= (cum - ps) < float(top_p) * cum[:, K - 1:K]
                keep_sorted[:, 0] = True
            keep = torch.zeros((B, V), dtype=torch.bool, device=dev).scatter_(1, order, keep_sorted)
            p = p * keep
        c = p.cumsum(-1)
        ids = torch.searchsorted(c, u.unsqueeze(1) * c[:, -1:], right=True).squeeze(1).clamp_(max=V - 1)
    lp = lsm.gather(1, ids.unsqueeze(1)).squeeze(1)
    if finished is not None:
        fin = finished.bool()
        ids = torch.where(fin, int(pad_token_id), ids)
        lp = torch.where(fin, 0.0, lp)
        finished.copy_((fin | (ids == int(eos_token_id))).to(torch.uint8))
    return ids, lp


def sample_logits(logits, u, temperature=1.0, top_k=0, top_p=1.0, finished=None, eos_token_id=-1, pad_token_id=0,
                  out_ids=None, out_logprob=None):
    """Next-token ids (int64 [B]) and their log probabilities (fp32 [B]) from ``logits`` [B, V].

    ``p = softmax(logits / temperature)`` in fp32. The order is a stable descending sort by logit
    (ties: ascending index). ``top_k > 0`` keeps the first ``top_k`` of it; ``top_p < 1`` keeps the
    shortest prefix of what is left whose renormalised mass is at least ``top_p`` (always one token).
    The kept set is renormalised and walked in ascending token index; the first token whose running
    mass exceeds ``u`` (float32 [B] uniforms in [0, 1) from the caller, which makes the call a pure
    function) is returned. ``top_k == 1`` is greedy: the argmax, the lowest index on a tie, ``u``
    ignored. The log probability is that of the returned token under the unfiltered softmax.
    ``finished`` (uint8 [B], updated in place): a row whose flag is set returns ``pad_token_id`` and
    log probability 0; a row that returns ``eos_token_id`` sets its flag.

    On a GPU, bf16 / fp16 logits with 1 <= B <= 16 and V <= 65,536 (a row's keys and the histograms
    must fit one workgroup's LDS; ``sample_logits_supported`` is False above) run on one kernel
    (csrc/kernels/sampling.hip), bitwise reproducible; the row stride may exceed V and elements past V
    are never read. float32 logits, the CPU and anything else the kernel rejects run the same contract
    in plain torch (``_sample_logits_composite``; on a GPU recorded as a fallback). PHA_SAMPLE_KERNEL=0
    forces the composite. ``out_ids`` / ``out_logprob`` receive the results when given."""
    import os
    _sample_check(logits, u, temperature, top_k, top_p, finished, out_ids, out_logprob)
    B, V = logits.shape
    use = logits.is_cuda and os.environ.get("PHA_SAMPLE_KERNEL", "1") != "0"
    if use and not sample_logits_excluded(B, V, top_k, top_p):
        why = "kernel library not loaded" if _lib.lib is None else _sample_reject(logits)
        if why is None:
            ids = out_ids if out_ids is not None else torch.empty((B,), dtype=torch.int64, device=logits.device)
            lp = out_logprob if out_logprob is not None else torch.empty((B,), dtype=torch.float32,
                                                                         device=logits.device)
            _check(_L().pha_sample_logits(_DT[logits.dtype], _ptr(logits), logits.stride(0), _ptr(u), _ptr(ids),
                                          _ptr(lp), _ptr(finished), B, V, float(temperature), int(top_k), float(top_p),
                                          int(eos_token_id), int(pad_token_id), _stream(logits)), "sample_logits")
            return ids, lp
        from . import fallback
        fallback.note("sample_logits", why + " -> torch composite")
    ids, lp = _sample_logits_composite(logits, u, temperature, top_k, top_p, finished, eos_token_id, pad_token_id)
    if out_ids is not None:
        ids = out_ids.copy_(ids)
    if out_logprob is not None:
        lp = out_logprob.copy_(lp)
    return ids, lp


# ----------------------------------------------------------------------------
# beam-search step (csrc/kernels/beam_search.hip)
# ----------------------------------------------------------------------------
BEAM_MAX_R = 16   # rows per call (groups times beams): the decode step's batch, as SAMPLE_MAX_B


def _beam_limits():
    if _lib.lib is None:
        return 0, 0
    return _lib.lib.pha_beam_search_max_v(), _lib.lib.pha_beam_search_max_k()


BEAM_MAX_V, BEAM_MAX_K = _beam_limits()   # the kernel's vocabulary and beam limits (0: library not built)


def _beam_check(logits, cum, finished, lengths, beam_size, cache_indirection, time_step):
    """the argument errors of beam_search_step, the same on every path (each names its argument)"""
    fn = "beam_search_step"
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"{fn}: logits must be a 2-D tensor [R, V]")
    if logits.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise ValueError(f"{fn}: logits are {logits.dtype}; bfloat16, float16 or float32 expected")
    R, V = logits.shape
    if R < 1 or V < 2:
        raise ValueError(f"{fn}: logits are [{R}, {V}]; at least one row and two columns expected")
    if logits.stride(1) != 1 or logits.stride(0) < V:
        raise ValueError(f"{fn}: logits strides {tuple(logits.stride())}: the last must be 1 and the first >= V={V}")
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or beam_size < 1 or beam_size > V \
            or R % beam_size:
        raise ValueError(f"{fn}: beam_size={beam_size!r} must be an int in [1, V={V}] that divides the {R} rows")
    dev = logits.device
    _row_vector_check(fn, "cum", cum, torch.float32, R, dev)
    _row_vector_check(fn, "finished", finished, torch.uint8, R, dev)
    _row_vector_check(fn, "lengths", lengths, torch.int32, R, dev)
    t = cache_indirection
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != R or t.shape[1] < 1 \
            or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{fn}: cache_indirection must be a contiguous int32 [{R}, max_seq] tensor on {dev}")
    if isinstance(time_step, torch.Tensor):
        if time_step.dtype != torch.int32 or time_step.device != dev or time_step.numel() not in (1, R) \
                or not time_step.is_contiguous():
            raise ValueError(f"{fn}: a tensor time_step must be contiguous int32 on {dev} with one element or one per "
                             f"row ({R})")
    elif isinstance(time_step, bool) or not isinstance(time_step, int) or not 0 <= time_step < t.shape[1]:
        raise ValueError(f"{fn}: time_step {time_step!r} outside the table's [0, {t.shape[1]})")


def _beam_reject(logits, beam_size):
    """why the kernels cannot take arguments that passed _beam_check, or None"""
    if not logits.is_cuda:
        return f"logits are on {logits.device}, not a GPU"
    if logits.dtype not in (torch.bfloat16, torch.float16):
        return f"logits are {logits.dtype}; the kernel takes bfloat16 or float16"
    if logits.shape[0] > BEAM_MAX_R:
        return f"R={logits.shape[0]} rows are above the kernel's {BEAM_MAX_R}"
    if logits.shape[1] > BEAM_MAX_V:
        return f"V={logits.shape[1]} is above the kernel's {BEAM_MAX_V} (one row of keys plus the histograms in LDS)"
    if beam_size > BEAM_MAX_K:
        return f"beam_size={beam_size} is above the kernel's {BEAM_MAX_K}"
    if logits.data_ptr() % 2:
        return "logits are not 2-byte aligned"
    return None


def beam_search_step_excluded(R, V, beam_size):
    """(R, V, K) classes that lost to the composite in tools/bench_generate.py --beams and stay on it
    by default (a policy, not a fallback). None: see profiles/generate/README.md."""
    return False


def beam_search_step_supported(logits, cum, finished, lengths, beam_size, cache_indirection, time_step):
    """what the beam-step kernels take: bf16 / fp16 logits [R, V] on a GPU with 1 <= R <= 16,
    2 <= V <= BEAM_MAX_V (65,536), unit inner stride and a row stride of at least V; 1 <= beam_size <= 16
    dividing R; float32 cum [R], uint8 finished [R], int32 lengths [R], a contiguous int32 table
    [R, max_seq] and an int32 time step (int, one element or [R]). float32 logits are not taken."""
    if _lib.lib is None:
        return False
    try:
        _beam_check(logits, cum, finished, lengths, beam_size, cache_indirection, time_step)
    except ValueError:
        return False
    return _beam_reject(logits, beam_size) is None \
        and not beam_search_step_excluded(logits.shape[0], logits.shape[1], beam_size)


def beam_search_step_why_not(logits, cum, finished, lengths, beam_size, cache_indirection, time_step):
    """the reason the beam-step kernels would reject these arguments, for the fallback log"""
    if _lib.lib is None:
        return "kernel library not loaded"
    try:
        _beam_check(logits, cum, finished, lengths, beam_size, cache_indirection, time_step)
    except ValueError as e:
        return str(e)
    return _beam_reject(logits, beam_size) or "supported"


def _beam_ts_rows(time_step, R, device):
    """the step of every row as int32 [R] on ``device`` (no host sync)"""
    if isinstance(time_step, torch.Tensor):
        return time_step if time_step.numel() == R else time_step.reshape(1).expand(R).contiguous()
    return torch.full((R,), int(time_step), dtype=torch.int32, device=device)


def _beam_search_step_composite(logits, cum, finished, lengths, eos_token_id, beam_size, cache_indirection, time_step):
    """beam_search_step's contract in plain torch (any device, any float dtype, any R; no host sync):
    a stable descending sort of each group's flattened fp32 totals"""
    R, V = logits.shape
    K, G = int(beam_size), R // int(beam_size)
    dev, eos = logits.device, int(eos_token_id)
    ninf = float("-inf")
    lp = torch.log_softmax(logits.float(), -1)
    fin = finished.bool()
    done = torch.full((V,), ninf, dtype=torch.float32, device=dev)
    if 0 <= eos < V:
        done[eos] = 0.0
    lp = torch.where(fin[:, None], done[None, :], lp)
    total = (cum[:, None] + lp).reshape(G, K * V)
    vals, idx = torch.sort(total, dim=-1, descending=True, stable=True)
    vals, idx = vals[:, :K].reshape(R), idx[:, :K].reshape(R)
    parent = (idx // V).to(torch.int32)
    dead = vals == ninf
    tok = torch.where(dead, eos, idx % V)
    prow = (torch.arange(G, device=dev).repeat_interleave(K) * K + parent).long()
    pfin = fin[prow]
    new_len = lengths[prow] + (~pfin).to(torch.int32)
    ts = _beam_ts_rows(time_step, R, dev)
    max_seq = cache_indirection.shape[1]
    ok = ((ts >= 0) & (ts < max_seq))[:, None]
    t = torch.arange(max_seq, device=dev, dtype=torch.int32)[None, :]
    new = torch.where(t < ts[:, None], cache_indirection[prow],
                      torch.where(t == ts[:, None], parent[:, None], cache_indirection))
    cache_indirection.copy_(torch.where(ok, new, cache_indirection))
    logprob = lp.reshape(G, K * V).gather(1, idx.reshape(G, K)).reshape(R).masked_fill(dead, ninf)
    cum.copy_(vals)
    finished.copy_((pfin | dead | (tok == eos)).to(torch.uint8))
    lengths.copy_(new_len)
    return tok, parent, logprob


def beam_search_step(logits, cum, finished, lengths, eos_token_id, beam_size, cache_indirection, time_step):
    """One beam-search step over ``logits`` [R, V], R = groups * ``beam_size`` rows, row b * K + k being
    beam k of batch item b. Returns (token int64 [R], parent int32 [R], logprob fp32 [R]: the token's
    log probability under its parent row, 0 for the EOS a finished beam repeats) and replaces ``cum`` (fp32 [R],
    the beams' cumulative log probabilities), ``finished`` (uint8 [R]) and ``lengths`` (int32 [R]) in
    place.

    ``lp = log_softmax(logits)`` in fp32; a finished row has lp = 0 at ``eos_token_id`` and -inf
    elsewhere. ``total[b, k * V + v] = cum[b * K + k] + lp[b * K + k, v]``; the K largest totals of a
    group are taken in descending order, equal totals in ascending flat index (lower beam, then lower
    token). Pick j becomes new beam j: token ``idx % V``, parent ``idx // V`` (a beam number in
    [0, K)), cum the total, finished ``finished[parent] | (token == eos)``, length ``lengths[parent] +
    !finished[parent]``. A pick whose total is -inf (only where a group has fewer than K finite
    totals) carries token ``eos_token_id``, log probability -inf and is finished; the other outputs follow the same rules.
    The first step of a search passes ``cum = [0, -inf, ...]`` per group, so all K picks continue beam 0.

    ``cache_indirection`` (int32 [R, max_seq], the table of ``decode_attention``) is re-ordered in
    place for the step ``time_step`` (int, int32 tensor of one element, or [R]): for t < time_step,
    ``table'[r, t] = table[group row parent[r], t]``, then ``table'[r, time_step] = parent[r]``;
    nothing above is touched and ``time_step`` is not advanced.

    On a GPU, bf16 / fp16 logits with R <= 16, V <= 65,536 and beam_size <= 16 run on two kernel
    launches (csrc/kernels/beam_search.hip) without a host sync. float32 logits, the CPU and anything
    else the kernels reject run the same contract in plain torch (``_beam_search_step_composite``; on
    a GPU recorded as a fallback). PHA_BEAM_KERNEL=0 forces the composite."""
    import os
    _beam_check(logits, cum, finished, lengths, beam_size, cache_indirection, time_step)
    R, V = logits.shape
    K = int(beam_size)
    use = logits.is_cuda and os.environ.get("PHA_BEAM_KERNEL", "1") != "0"
    if use and not beam_search_step_excluded(R, V, K):
        why = "kernel library not loaded" if _lib.lib is None else _beam_reject(logits, K)
        if why is None:
            dev = logits.device
            tok = torch.empty((R,), dtype=torch.int64, device=dev)
            parent = torch.empty((R,), dtype=torch.int32, device=dev)
            logprob = torch.empty((R,), dtype=torch.float32, device=dev)
            cand_lp = torch.empty((R, BEAM_MAX_K), dtype=torch.float32, device=dev)
            cand_tok = torch.empty((R, BEAM_MAX_K), dtype=torch.int32, device=dev)
            ts = _beam_ts_rows(time_step, R, dev)
            _check(_L().pha_beam_search_step(_DT[logits.dtype], _ptr(logits), logits.stride(0), _ptr(cum),
                                             _ptr(finished), _ptr(lengths), _ptr(tok), _ptr(parent),
                                             _ptr(logprob), _ptr(cache_indirection), _ptr(ts), _ptr(cand_lp), _ptr(cand_tok), R, V, K,
                                             int(eos_token_id), cache_indirection.shape[1], _stream(logits)),
                   "beam_search_step")
            return tok, parent, logprob
        from . import fallback
        fallback.note("beam_search_step", why + " -> torch composite")
    return _beam_search_step_composite(logits, cum, finished, lengths, eos_token_id, beam_size, cache_indirection,
                                       time_step)
