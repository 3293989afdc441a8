"""The MLP's GELU-adjacent products at the GPT-3 1.3B shape (H 2048, F 8192; tokens 98304 = the bench's
micro-batch 48 x 2048, and 32768), sustained:
backward  d pre = (dY W2^T) * gelu'(pre) (+ d b1): library NT + HIP dGELU pass / gemm4w dGELU +
column-sum epilogue / own gemm4p NT + HIP pass; the chain-3 parts: library NT alone, own gemm4p NT
alone, own gemm4p NT with the multiply-by-stored-derivative epilogue;
forward gelu(x W1 + b1) (+ pre): gemm4p GELU epilogue with the pre-activation / with the derivative
in aux / gemm4w NN GELU epilogue / library + HIP bias-GELU pass.
python tools/mlp_parts_bench.py [tokens ...]"""
import sys

import torch

sys.path.insert(0, ".")
from paddle_hackathon_amd.ops import gemm as G, hip  # noqa: E402
from paddle_hackathon_amd.ops.conv_gemm import weight_t  # noqa: E402
from tools.g4p_sustain import sustain  # noqa: E402


def parts(T, H=2048, F=8192):
    torch.manual_seed(0)
    x = torch.randn(T, H, device="cuda").bfloat16()
    w1 = (torch.randn(H, F, device="cuda") * 0.02).bfloat16()
    b1 = (torch.randn(F, device="cuda") * 0.02).bfloat16()
    w2 = (torch.randn(F, H, device="cuda") * 0.02).bfloat16()
    gy = torch.randn(T, H, device="cuda").bfloat16()
    pre = torch.randn(T, F, device="cuda").bfloat16()
    w1t = weight_t(w1)

    def bwd_lib():
        ga = gy @ w2.t()
        return hip.bias_gelu_bwd(ga, pre, b1, True, want_db=False)

    def bwd_lib_nt():
        return gy @ w2.t()

    def bwd_4w():
        g, part = G.gemm(gy, w2, False, False, act="dgelu", aux=pre, colsum=True)
        return g, G.colsum_finish(part, b1.dtype)

    def bwd_own():
        ga = G.gemm_p(gy, w2, False, False)
        return hip.bias_gelu_bwd(ga, pre, b1, True, want_db=False)

    def bwd_own_nt():
        return G.gemm_p(gy, w2, False, False)

    def bwd_own_mul():
        return G.mm_nt_mul(gy, w2, pre)

    def fwd_4p():
        return G.mm_nt_bias_gelu(x, w1t, b1)

    def fwd_4p_d():
        return G.mm_nt_bias_gelu(x, w1t, b1, deriv=True)

    def fwd_4w():
        return G.nn(x, w1, bias=b1, act="gelu", aux_out=True)

    def fwd_lib():
        h = x @ w1
        return hip.bias_gelu_fwd(h, b1, True), h

    rows = [("bwd lib NT", bwd_lib_nt), ("bwd lib NT + dGELU pass", bwd_lib),
            ("bwd gemm4p NT", bwd_own_nt), ("bwd gemm4p NT + dGELU pass", bwd_own),
            ("bwd gemm4p NT x stored derivative", bwd_own_mul),
            ("fwd gemm4p GELU epilogue (pre aux)", fwd_4p), ("fwd gemm4p GELU epilogue (deriv aux)", fwd_4p_d)]
    if T <= 32768:   # (the gemm4w chain and the library forward at the original shape only)
        rows += [("bwd gemm4w dGELU+colsum epilogue", bwd_4w), ("fwd gemm4w NN GELU epilogue", fwd_4w),
                 ("fwd lib + bias-GELU pass", fwd_lib)]
    for name, f in rows:
        t = sustain(f)
        print(f"T={T:6d} {name:38s} {t * 1e6:8.1f} us", flush=True)


def main():
    for T in [int(a) for a in sys.argv[1:]] or [98304, 32768]:
        parts(T)


if __name__ == "__main__":
    main()
