"""CTC loss, forward plus backward: the fused kernels (csrc/kernels/ctc.hip, ops.ctc_loss) against the
composite that PHA_CTC_KERNEL=0 keeps (fp32 cast + log_softmax + torch's ctc_loss, gradients through
autograd), from unnormalised logits [T, B, V] to the gradient in the logits' dtype.

Every sample has the full input length T and a random label of length L without blanks. The two paths
alternate in one process, each call on the next of several logits buffers (together above the 256 MiB
Infinity Cache, so the logits come from HBM as they do behind a model); the figure is the median over
the rounds; a round times, with device events, as many calls of a path as fill ``--window`` seconds
(counted from a short trial of that path), launch work of the host included. With --trace-iters N the
tool only runs N calls of the kernel path, for a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_ctc.py --dtype bf16 --trace-iters 50
Bytes are counted from the shapes, e = the logits' element size and N = T B V:
  kernels    forward reads N e; backward reads N e and writes N e; the [2, B, T, 2L+1] fp32 workspace
             is written by the row pass, read and written by the chains and read by the gradient pass
  composite  cast (N e read, 4 N written; none for fp32), log_softmax (4 N + 4 N), the ctc backward
             (4 N read, 4 N written), the log_softmax backward (8 N read, 4 N written) and the cast
             back (4 N + N e; none for fp32); its [B, T, 2L+1] alpha and beta are left out

Prints one markdown table. Usage: python tools/bench_ctc.py [--T 80 --B 256 --V 6625 --L 25]
                                                              [--dtype bf16 fp32] [--rounds 7] [--window 0.5]
"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_hackathon_amd import ops  # noqa: E402
from paddle_hackathon_amd.ops import fallback  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def composite(x, y, il, ll):
    return TF.ctc_loss(TF.log_softmax(x.float(), -1), y, il, ll, 0, reduction="none", zero_infinity=True)


def kernel(x, y, il, ll):
    return ops.ctc_loss(x, y, il, ll, 0, zero_infinity=True)


def timed(fn, iters):
    """ms per call: device events around ``iters`` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, window, rounds):
    """(median, min, max ms per call, calls per round) of each function, the functions taking turns within
    every round; a round of a function is as many calls as fill ``window`` seconds"""
    iters = []
    for fn in fns:
        timed(fn, 3)   # warm-up
        iters.append(max(10, math.ceil(window * 1e3 / timed(fn, 10))))
    samples = [[] for _ in fns]
    for _ in range(rounds):
        for s, fn, n in zip(samples, fns, iters):
            s.append(timed(fn, n))
    return [(statistics.median(s), min(s), max(s), n) for s, n in zip(samples, iters)]


def moved_bytes(T, B, V, L, e):
    N, ws = T * B * V, 2 * B * T * (2 * L + 1) * 4
    cast = 0 if e == 4 else 2 * (N * e + 4 * N)
    return 3 * N * e + 4 * ws, cast + 8 * N + 8 * N + 12 * N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--V", type=int, default=6625)
    ap.add_argument("--L", type=int, default=25)
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"], choices=list(DTYPES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per path and round")
    ap.add_argument("--trace-iters", type=int, default=0, help="only run this many kernel-path calls (for a trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ctc.py measures on a GPU"
    T, B, V, L = a.T, a.B, a.V, a.L
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.randint(1, V, (B, L), device="cuda", generator=g)
    il = torch.full((B,), T, device="cuda")
    ll = torch.full((B,), L, device="cuda")
    if a.trace_iters:
        x = torch.randn(T, B, V, device="cuda", generator=g).to(DTYPES[a.dtype[0]]).requires_grad_()
        for _ in range(a.trace_iters):
            x.grad = None
            kernel(x, y, il, ll).sum().backward()
        torch.cuda.synchronize()
        return
    print(f"### CTC forward + backward, T={T} B={B} V={V} L={L}: ms per call, median of {a.rounds} rounds of "
          f"{a.window} s per path (min - max) [calls per round]\n")
    print("| dtype | kernels | composite | composite / kernels | kernel bytes | composite bytes | kernels TB/s | "
          "loss rel diff | grad diff / max |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.dtype:
        dt = DTYPES[name]
        e = torch.empty(0, dtype=dt).element_size()
        n = max(2, math.ceil(600e6 / (T * B * V * e)))
        xs = [torch.randn(T, B, V, device="cuda", generator=g).to(dt).requires_grad_() for _ in range(n)]

        def step(fn):
            def run(i):
                x = xs[i % n]
                x.grad = None
                fn(x, y, il, ll).sum().backward()
            return run

        fallback.reset()
        lk = kernel(xs[0], y, il, ll)
        (gk,) = torch.autograd.grad(lk.sum(), xs[0])
        assert fallback.counts() == {}, fallback.counts()   # the kernels ran, not the composite twice
        lc = composite(xs[0], y, il, ll)
        (gc,) = torch.autograd.grad(lc.sum(), xs[0])
        dl = ((lk - lc).abs() / lc.abs()).max().item()
        dg = ((gk.float() - gc.float()).abs().max() / gc.float().abs().max()).item()
        tk, tc = alternate([step(kernel), step(composite)], a.window, a.rounds)
        bk, bc = moved_bytes(T, B, V, L, e)
        ms = lambda t: f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f}) [{t[3]}]"
        print(f"| {name} | {ms(tk)} | {ms(tc)} | {tc[0] / tk[0]:.2f} | {bk / 1e6:.0f} MB | {bc / 1e6:.0f} MB | "
              f"{bk / tk[0] / 1e9:.2f} | {dl:.1e} | {dg:.1e} |")
        del xs


if __name__ == "__main__":
    main()
