"""Forward + backward time of variable-length flash attention (csrc/kernels/flash_attn_varlen.hip, packed
[T, H, D] with device cu_seqlens) against what a ragged batch costs without it: the dense kernels on the
batch padded to its longest sequence with a key-padding mask.

32 sequences, lengths drawn once (seed 0) between 32 and 512, H = 12, D = 64, bf16, non-causal. The two
paths alternate in rounds; each round times ``--iters`` forward + backward calls between device events
after a warm-up; the medians over the rounds are printed as one JSON line (and both outputs are compared
on the real tokens first). Needs a GPU: there is no CPU fall-back.

    python tools/bench_flash_varlen.py [--rounds 7] [--iters 500]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_hackathon_amd import ops  # noqa: E402
from paddle_hackathon_amd.ops import fallback, hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=500)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flash_varlen needs a GPU"
    n, H, D = 32, 12, 64
    lens = torch.randint(32, 513, (n,), generator=torch.Generator().manual_seed(0)).tolist()
    T, S = sum(lens), (max(lens) + 3) // 4 * 4
    scale = 1 / math.sqrt(D)
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = [torch.randn(T, H, D, device="cuda", generator=g).bfloat16().requires_grad_() for _ in range(3)]
    do = torch.randn(T, H, D, device="cuda", generator=g).bfloat16()
    cu = torch.tensor([0] + lens).cumsum(0).int().cuda()
    # the padded batch: row b holds sequence b, keys past its length masked out
    idx = torch.cat([b * S + torch.arange(l) for b, l in enumerate(lens)]).cuda()
    pad = [torch.zeros(n * S, H, D, device="cuda", dtype=torch.bfloat16).index_copy_(0, idx, t.detach())
           .view(n, S, H, D).requires_grad_() for t in qkv]
    dop = torch.zeros(n * S, H, D, device="cuda", dtype=torch.bfloat16).index_copy_(0, idx, do).view(n, S, H, D)
    mask = torch.full((n, 1, 1, S), float("-inf"), device="cuda")
    for b, l in enumerate(lens):
        mask[b, :, :, :l] = 0

    def varlen():
        o = hip.flash_attention_varlen(*qkv, cu, cu, S, S, scale)
        return o, torch.autograd.grad(o, qkv, do)

    def padded():
        o = ops.flash_attention(*pad, mask=mask, scale=scale)
        return o, torch.autograd.grad(o, pad, dop)

    fallback.reset()
    ov, op = varlen()[0], padded()[0].reshape(n * S, H, D)[idx]
    assert fallback.total() == 0, fallback.counts()
    diff = (ov.float() - op.float()).abs().max().item()
    assert diff < 2e-2, diff

    def timed(fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    tv, tp = [], []
    for _ in range(args.rounds):
        tv.append(timed(varlen))
        tp.append(timed(padded))
    print(json.dumps({"bench": "flash_varlen_fwd_bwd", "device": torch.cuda.get_device_name(0), "sequences": n,
                      "heads": H, "head_dim": D, "tokens": T, "padded_tokens": n * S, "longest": max(lens),
                      "varlen_ms_median": round(statistics.median(tv), 4), "varlen_ms_all": [round(x, 4) for x in tv],
                      "padded_ms_median": round(statistics.median(tp), 4), "padded_ms_all": [round(x, 4) for x in tp],
                      "max_abs_output_difference": diff, "rounds": args.rounds, "iters": args.iters}))


if __name__ == "__main__":
    main()
