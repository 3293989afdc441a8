"""Variable-length flash attention (csrc/kernels/flash_attn_varlen.hip) through
nn.functional.flash_attn_unpadded against plain per-sequence float64 attention of the same rounded
inputs, at the smallest lengths that reach the tile map's edges: one token, one full 64-key tile, a tile
plus one, empty sequences, three 128-row tiles, tokens allocated past cu[n], an empty key sequence.
Bounds: max|a - ref| / max|ref| below 2e-2 (output) and 3e-2 (gradients), as tests/test_fa64_gpu.py; where the
reference is all zero (dq and dk of a lone one-token sequence) the result is held to the fp32 rounding of its sums."""
import math

import pytest
import torch

from paddle_hackathon_amd.framework.core import _wrap
from paddle_hackathon_amd.nn.functional import flash_attn_unpadded
from test_flash_attn_varlen_cpu import varlen_ref

pytestmark = pytest.mark.gpu

SELF = [([1], 0), ([64], 0), ([65, 1, 63], 0), ([0, 130, 0, 7], 0), ([257, 64], 5)]   # lengths, tokens past cu[n]
CASES = [(lens, lens, pad, D, causal, H, Hk, torch.bfloat16)
         for lens, pad in SELF for D in (64, 128) for causal in (False, True) for H, Hk in ((2, 2), (4, 2))]
CASES.append(([65, 1, 63], [65, 1, 63], 0, 64, True, 4, 2, torch.float16))
CASES.append(([3, 70, 4], [100, 0, 5], 0, 128, False, 4, 2, torch.bfloat16))   # cross-attention, one without keys
BOUNDS = (("o", 2e-2), ("dq", 3e-2), ("dk", 3e-2), ("dv", 3e-2))


@pytest.mark.parametrize("lens_q,lens_k,pad,D,causal,H,Hk,dtype", CASES)
def test_varlen_matches_float64(monkeypatch, lens_q, lens_k, pad, D, causal, H, Hk, dtype):
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")
    g = torch.Generator(device="cuda").manual_seed(sum(lens_q) + D + H)
    Tq, Tk, scale = sum(lens_q) + pad, sum(lens_k) + pad, 1 / math.sqrt(D)
    q = torch.randn(Tq, H, D, device="cuda", generator=g).to(dtype).requires_grad_()
    k = torch.randn(Tk, Hk, D, device="cuda", generator=g).to(dtype).requires_grad_()
    v = torch.randn(Tk, Hk, D, device="cuda", generator=g).to(dtype).requires_grad_()
    do = torch.randn(Tq, H, D, device="cuda", generator=g).to(dtype)
    cu_q, cu_k = (_wrap(torch.tensor([0] + lens).cumsum(0).int().cuda()) for lens in (lens_q, lens_k))
    o = flash_attn_unpadded(_wrap(q), _wrap(k), _wrap(v), cu_q, cu_k, max(lens_q), max(lens_k), scale,
                            causal=causal)[0]._t
    got = (o,) + torch.autograd.grad(o, (q, k, v), do)
    want = varlen_ref(q, k, v, lens_q, lens_k, scale, causal, do)
    # an all-zero reference (dq, dk of a lone one-token sequence: dS = p (dP - delta) with dP = delta = do . v) leaves
    # the fp32 rounding of two D-term sums of the same products, times scale and a q / k element: |a| below that
    zero_ref = D * 2.0 ** -23 * (do.abs().max() * v.abs().max() * max(q.abs().max(), k.abs().max())).item() * scale
    for (name, bound), a, b, used in zip(BOUNDS, got, want, (Tq - pad, Tq - pad, Tk - pad, Tk - pad)):
        err = (a.double() - b).abs().max().item() / (b.abs().max().item() or zero_ref / bound)
        print(f"{name}: {err:.3e}")
        assert err < bound, (name, err)
        assert not a[used:].any(), f"{name}: rows past cu[n] are not zero"


def test_lengths_live_on_the_device_only(monkeypatch):
    """the same cu_seqlens tensor rewritten in place (same T, same n) gives the new lengths' result, eagerly
    and from a graph captured under the old ones: nothing on the host depends on the lengths"""
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")
    H, Hk, D = 4, 2, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(129, H, D, device="cuda", generator=g).bfloat16().requires_grad_()
    k = torch.randn(129, Hk, D, device="cuda", generator=g).bfloat16().requires_grad_()
    v = torch.randn(129, Hk, D, device="cuda", generator=g).bfloat16().requires_grad_()
    do = torch.randn(129, H, D, device="cuda", generator=g).bfloat16()
    scale, cu, graph, og = 1 / math.sqrt(D), torch.zeros(4, dtype=torch.int32, device="cuda"), None, None
    args = (_wrap(q), _wrap(k), _wrap(v), _wrap(cu), _wrap(cu), 129, 129, scale)
    for lens in ([65, 1, 63], [20, 100, 9]):
        cu.copy_(torch.tensor([0] + lens).cumsum(0))
        o = flash_attn_unpadded(*args, causal=True)[0]._t
        got = (o,) + torch.autograd.grad(o, (q, k, v), do)
        for (name, bound), a, b in zip(BOUNDS, got, varlen_ref(q, k, v, lens, lens, scale, True, do)):
            err = ((a.double() - b).abs().max() / b.abs().max()).item()
            print(f"{lens} {name}: {err:.3e}")
            assert err < bound, (lens, name, err)
        if graph is None:   # captured under the first lengths, replayed under both
            graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(graph):
                og = flash_attn_unpadded(*args, causal=True)[0]._t
        for _ in range(2):
            og.fill_(1)
            graph.replay()
            assert torch.equal(og, o), lens
