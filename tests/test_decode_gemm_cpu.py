"""PHA_DECODE_GEMM and the helper that routes small products to the weight-streaming GEMM kernels
must not disturb the CPU path: with the switch unset and set to 0, fused_multi_transformer's decode
stage and fused_linear give bitwise equal results on CPU tensors. The split plan is a pure function
of (N, K, layout)."""
import pytest
import torch

E, HEADS, LAYERS, B, MAX_SEQ, CTX = 64, 2, 2, 2, 12, 5
NAMES = ("ln_scales", "ln_biases", "qkv_weights", "qkv_biases", "linear_weights", "linear_biases",
         "ffn_ln_scales", "ffn_ln_biases", "ffn1_weights", "ffn1_biases", "ffn2_weights", "ffn2_biases")


def _weights(trans_qkvw):
    g = torch.Generator().manual_seed(0)
    D = E // HEADS

    def r(*shape, s=0.1):
        return torch.randn(*shape, generator=g) * s

    shapes = {"ln_scales": (E,), "ln_biases": (E,), "qkv_weights": (3, HEADS, D, E) if trans_qkvw else (E, 3, HEADS, D),
              "qkv_biases": (3, HEADS, D), "linear_weights": (E, E), "linear_biases": (E,), "ffn_ln_scales": (E,),
              "ffn_ln_biases": (E,), "ffn1_weights": (E, 4 * E), "ffn1_biases": (4 * E,), "ffn2_weights": (4 * E, E),
              "ffn2_biases": (E,)}
    return [[1.0 + r(*shapes[n]) if n.endswith("ln_scales") else r(*shapes[n]) for _ in range(LAYERS)] for n in NAMES]


def _decode(pre_ln, trans_qkvw):
    from paddle_hackathon_amd.incubate.nn import functional as FF
    w = _weights(trans_qkvw)
    x = torch.randn(B, CTX + 3, E, generator=torch.Generator().manual_seed(1))
    caches = [torch.zeros(2, B, HEADS, MAX_SEQ, E // HEADS) for _ in range(LAYERS)]
    outs = []
    with torch.no_grad():
        FF.fused_multi_transformer(x[:, :CTX], *w, pre_layer_norm=pre_ln, trans_qkvw=trans_qkvw, cache_kvs=caches)
        for j in range(3):
            out, _ = FF.fused_multi_transformer(x[:, CTX + j:CTX + j + 1], *w, pre_layer_norm=pre_ln,
                                                trans_qkvw=trans_qkvw, cache_kvs=caches, time_step=CTX + j)
            outs.append(out._t if hasattr(out, "_t") else out)
    return torch.cat(outs, 1), caches


@pytest.mark.parametrize("pre_ln,trans_qkvw", [(True, True), (False, False)], ids=["preln", "postln_nt"])
def test_switch_leaves_the_cpu_decode_stage_bitwise_unchanged(pre_ln, trans_qkvw, monkeypatch):
    from paddle_hackathon_amd.ops import fallback
    fallback.reset()
    monkeypatch.delenv("PHA_DECODE_GEMM", raising=False)
    a, ca = _decode(pre_ln, trans_qkvw)
    monkeypatch.setenv("PHA_DECODE_GEMM", "0")
    b, cb = _decode(pre_ln, trans_qkvw)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert all(torch.equal(p, q) for p, q in zip(ca, cb))
    assert "decode_gemm" not in fallback.counts()


@pytest.mark.parametrize("transpose_weight", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_switch_leaves_cpu_fused_linear_bitwise_unchanged(transpose_weight, dtype, monkeypatch):
    from paddle_hackathon_amd.incubate.nn import functional as FF
    from paddle_hackathon_amd.ops import fallback
    fallback.reset()
    g = torch.Generator().manual_seed(2)
    w = torch.randn((24, 40) if transpose_weight else (40, 24), generator=g).to(dtype)
    bias = torch.randn(24, generator=g).to(dtype)
    for shape in ((4, 40), (2, 3, 40), (40, 40)):
        x = torch.randn(*shape, generator=g).to(dtype)
        outs = []
        for value in (None, "0"):
            if value is None:
                monkeypatch.delenv("PHA_DECODE_GEMM", raising=False)
            else:
                monkeypatch.setenv("PHA_DECODE_GEMM", value)
            with torch.no_grad():
                o = FF.fused_linear(x, w, bias, transpose_weight=transpose_weight)
            outs.append(o._t if hasattr(o, "_t") else o)
        want = x @ (w.t() if transpose_weight else w) + bias if x.dim() == 3 else torch.addmm(bias, x, w.t() if transpose_weight else w)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], want)
    assert "decode_gemm" not in fallback.counts()


def test_plan_is_deterministic_and_leaves_no_split_empty():
    from paddle_hackathon_amd.ops import hip, _lib
    assert hip.SKINNY_GEMM_MAX_M == 16
    if _lib.lib is None or not hasattr(_lib.lib, "pha_skinny_gemm_plan"):
        pytest.skip("libpha_kernels.so is not loaded")
    # (N, K) of the QKV, output, ffn1 and ffn2 products of the 1.3B (E = 2048) and 13B (E = 5120) layers
    pairs = [(6144, 2048), (2048, 2048), (8192, 2048), (2048, 8192), (15360, 5120), (5120, 5120), (20480, 5120),
             (5120, 20480)]
    for nk in (True, False):
        bn, ks = hip.skinny_gemm_tile(nk)
        assert bn >= 16 and ks >= 32
        for N, K in pairs:
            ns, kps = hip.skinny_gemm_plan(N, K, nk)
            assert (ns, kps) == hip.skinny_gemm_plan(N, K, nk)
            assert ns >= 1 and kps >= 8 and kps % 8 == 0
            assert (ns - 1) * kps < K <= ns * kps, (N, K, nk, ns, kps)
    with pytest.raises(ValueError):
        hip.skinny_gemm_plan(0, 64, True)


def test_cpu_tensors_are_not_supported_and_are_rejected():
    from paddle_hackathon_amd.ops import hip
    x, w = torch.ones(4, 64, dtype=torch.bfloat16), torch.ones(64, 32, dtype=torch.bfloat16)
    assert not hip.skinny_gemm_supported(x, w, False)
    with pytest.raises(ValueError, match="x "):
        hip.skinny_gemm(x, w, False)
