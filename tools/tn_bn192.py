"""256 x 192 against 256 x 256 tiles on the GPT-3 1.3B weight gradients under sustained load (K =
98,304 tokens, the bench's micro-batch 48 x 2048): the qkv dW (2048 x 6144: 192 items of 256 x 256 or
256 of 256 x 192 on 256 CUs), with and without the bias-gradient column sums, and the fc1 dW
(2048 x 8192) on both forms for the policy's penalty factor
  (192-form time at a full round) / (0.75 x 256-form time at a full round)
measured on 2048 x 6144 columns of it for the 192 form (8192 is no multiple of 192; 256 items, one
full round) and on all 8192 for the 256 form (256 items, one full round). The two forms alternate in
one process over three rounds; each figure is the mean of the last second of 1.5 s back to back.
python tools/tn_bn192.py"""
import os
import sys

import torch

sys.path.insert(0, ".")
from paddle_hackathon_amd.ops import gemm as G  # noqa: E402
from tools.g4p_sustain import sustain  # noqa: E402

T = int(os.environ.get("TN_T", "98304"))
ROUNDS = int(os.environ.get("TN_ROUNDS", "3"))


def main():
    a = torch.randn(T, 2048, device="cuda").bfloat16()
    b = (torch.randn(T, 8192, device="cuda") * 0.02).bfloat16()
    bq = b[:, :6144]   # the 192 form's full round of the fc1 dW operands (row stride 8192)
    qkv = (torch.randn(T, 6144, device="cuda") * 0.02).bfloat16()
    var = {"qkv256": lambda: G.gemm_p(a, qkv, True, True, bn=256),
           "qkv192": lambda: G.gemm_p(a, qkv, True, True, bn=192),
           "qkv256+db": lambda: G.gemm_p(a, qkv, True, True, bn=256, colsum=True),
           "qkv192+db": lambda: G.gemm_p(a, qkv, True, True, bn=192, colsum=True),
           "fc1_256": lambda: G.gemm_p(a, b, True, True, bn=256),
           "fc1_192x6144": lambda: G.gemm_p(a, bq, True, True, bn=192)}
    res = {k: [] for k in var}
    for r in range(ROUNDS):
        for k, f in var.items():
            res[k].append(sustain(f))
        print(f"round {r}: " + "  ".join(f"{k} {v[-1] * 1e6:7.1f} us" for k, v in res.items()), flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    for k, n in (("qkv256", 6144), ("qkv192", 6144), ("qkv256+db", 6144), ("qkv192+db", 6144), ("fc1_256", 8192),
                 ("fc1_192x6144", 6144)):
        print(f"{k:13s} mean {mean[k] * 1e6:7.1f} us  {2.0 * T * 2048 * n / mean[k] / 1e12:6.0f} TF/s  "
              f"spread {(max(res[k]) - min(res[k])) * 1e6:5.1f} us")
    print(f"penalty = fc1_192x6144 / (0.75 x fc1_256) = {mean['fc1_192x6144'] / (0.75 * mean['fc1_256']):.3f}")
    print(f"qkv dW 192 / 256 = {mean['qkv192'] / mean['qkv256']:.3f}  with db {mean['qkv192+db'] / mean['qkv256+db']:.3f}")


if __name__ == "__main__":
    main()
