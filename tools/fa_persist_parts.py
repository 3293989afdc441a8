"""Persistent against plain launch form of the D = 128 attention kernels, per kernel, at the GPT-3
1.3B bench shape (packed QKV, B 48, H 16, S 2048, causal) — and the plain form at S 1024 / 4096 for
the fixed-cost-per-workgroup fit.

Sustained back-to-back launches on random data, timed with events; the forms alternate inside one
process (PHA_FA_PERSIST is read at every launch), `--rounds` times. The backward launches dQ and
dK/dV together, so dQ's and dK/dV's gains are read from the runs with only their bit set.

  python tools/fa_persist_parts.py [--rounds 3] [--iters 20] [--fit]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, ".")
from paddle_hackathon_amd.ops import hip  # noqa: E402

H, D = 16, 128


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def _setup(B, S):
    g = torch.Generator(device="cuda").manual_seed(S)
    qkv = torch.randn(B, S, H, 3 * D, device="cuda", generator=g).bfloat16().requires_grad_(True)
    o = hip.FlashAttentionPacked.apply(qkv, True, None)
    do = torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16()

    def fwd():
        with torch.no_grad():
            hip.FlashAttentionPacked.apply(qkv, True, None)

    def bwd():
        torch.autograd.grad(o, qkv, do, retain_graph=True)

    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--fit", action="store_true", help="plain form at S 1024 / 2048 / 4096 and the fixed-cost fit")
    args = ap.parse_args()
    os.environ.pop("PHA_FA_PERSIST_WGS", None)
    print(f"lib {os.environ.get('PHA_KERNELS_LIB', 'libpha_kernels.so')}  B {args.batch} H {H} D {D} causal packed", flush=True)

    fwd, bwd = _setup(args.batch, 2048)
    modes = (("plain", "0", fwd, bwd), ("fwd", "1", fwd, None), ("dq", "2", None, bwd), ("dkdv", "4", None, bwd),
             ("all", "7", fwd, bwd))
    for r in range(args.rounds):
        for name, bits, f, b in modes:
            os.environ["PHA_FA_PERSIST"] = bits
            tf = _time(f, args.iters) if f else float("nan")
            tb = _time(b, args.iters) if b else float("nan")
            print(f"round {r} S 2048 PHA_FA_PERSIST={bits} ({name:5s}): fwd {tf:8.1f} us  bwd (dQ + dK/dV) {tb:8.1f} us", flush=True)

    if args.fit:
        # time per CU = WGs per CU * fixed + tiles per CU * per_tile (least squares over the three S);
        # a block's four diagonal tiles, partly skipped wave by wave, also count as per-block cost
        os.environ["PHA_FA_PERSIST"] = "0"
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        rows = []
        del fwd, bwd
        for S in (1024, 2048, 4096):
            torch.cuda.empty_cache()
            f, b = _setup(args.batch, S)
            tf = min(_time(f, args.iters) for _ in range(args.rounds))
            tb = min(_time(b, args.iters) for _ in range(args.rounds))
            rows.append((S, tf, tb))
            print(f"plain S {S}: fwd {tf:8.1f} us  bwd {tb:8.1f} us", flush=True)
            del f, b
        BH = args.batch * H
        for name, col, rows_per_wg, wgk in (("fwd (256-row blocks)", 1, 256, 1), ("bwd (dQ 256-row + dK/dV 128-key blocks)", 2, 256, 3)):
            A, y = [], []
            for row in rows:
                S = row[0]
                nb = S // rows_per_wg
                wgs = BH * nb * wgk / cus                      # bwd: 1 dQ + 2 dK/dV workgroups per 256 rows
                tiles = BH * 2 * nb * (nb + 1) / cus           # 64-key tiles under the diagonal per 256-row block
                A.append([wgs, tiles])
                y.append(row[col])
            sol = torch.linalg.lstsq(torch.tensor(A, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)).solution
            S2 = 2048
            nb = S2 // rows_per_wg
            fixed_total = sol[0].item() * BH * nb * wgk / cus
            print(f"fit {name}: fixed {sol[0].item():.2f} us per workgroup, {sol[1].item():.3f} us per 64-key tile unit; "
                  f"fixed share at S 2048: {fixed_total:.1f} us of {rows[1][col]:.1f} us = {100 * fixed_total / rows[1][col]:.1f} %",
                  flush=True)


if __name__ == "__main__":
    main()
