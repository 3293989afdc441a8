"""The decode stage of incubate.nn.functional.fused_multi_transformer with an int32 [B] device
``time_step`` on the GPU in bf16, on both of its paths: the split-KV kernels and the composite that
PHA_DECODE_ATTN=0 keeps. B = 3 right-padded rows of lengths (C - 2, C - 70, 1), C = DECODE_ATTN_CHUNK,
and 4 steps, so the longest row crosses a split seam.

The reference is the same function on the CPU in fp32 with the same bf16-representable weights and
the same [B] step (tests/test_ragged_decode_cpu.py checks that one row by row). Bound, the yardstick of
tests/test_fused_multi_transformer_gpu.py taken both ways: with e the max-normalised error of a step's
output against fp32, e_kernel <= max(2 * e_composite, 2^-8) and e_composite <= max(2 * e_kernel, 2^-8);
the two paths round in a different order, neither may be worse than that. Both paths must run the
step without a host sync, and the composite must not see what the caches hold above a row's step: they
are filled with NaN there before every step."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E, LAYERS, STEPS = 256, 2, 4
DFF = 4 * E
NAMES = ("ln_scales", "ln_biases", "qkv_weights", "qkv_biases", "linear_weights", "linear_biases",
         "ffn_ln_scales", "ffn_ln_biases", "ffn1_weights", "ffn1_biases", "ffn2_weights", "ffn2_biases")


def _geom():
    from paddle_hackathon_amd.ops import hip
    C = hip.DECODE_ATTN_CHUNK
    return C + 24, (C - 2, C - 70, 1)   # max_seq, prompt lengths


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _weights(heads, seed):
    """bf16-representable fp32 weights on the CPU"""
    g = torch.Generator().manual_seed(seed)
    D = E // heads

    def r(*shape, s=0.05):
        return (torch.randn(*shape, generator=g) * s).bfloat16().float()

    w = {k: [] for k in NAMES}
    for _ in range(LAYERS):
        w["ln_scales"].append((1.0 + r(E)).bfloat16().float())
        w["ln_biases"].append(r(E))
        w["qkv_weights"].append(r(3, heads, D, E))
        w["qkv_biases"].append(r(3, heads, D))
        w["linear_weights"].append(r(E, E))
        w["linear_biases"].append(r(E))
        w["ffn_ln_scales"].append((1.0 + r(E)).bfloat16().float())
        w["ffn_ln_biases"].append(r(E))
        w["ffn1_weights"].append(r(E, DFF))
        w["ffn1_biases"].append(r(DFF))
        w["ffn2_weights"].append(r(DFF, E))
        w["ffn2_biases"].append(r(E))
    return w


def _run(x, w, **kw):
    from paddle_hackathon_amd.incubate.nn import functional as FF
    out = FF.fused_multi_transformer(x, *[w[k] for k in NAMES], pre_layer_norm=True, trans_qkvw=True, **kw)
    out = out[0] if isinstance(out, tuple) else out
    return out._t if hasattr(out, "_t") else out


def _generate(prompt, steps, w, heads, lens, poison=False, no_sync=False):
    """context stage over the padded prompts + STEPS decode steps with a [B] step -> [B, STEPS, E]"""
    max_seq, _ = _geom()
    B = prompt.shape[0]
    caches = [torch.zeros(2, B, heads, max_seq, E // heads, device=prompt.device, dtype=prompt.dtype)
              for _ in range(LAYERS)]
    outs = []
    with torch.no_grad():
        _run(prompt, w, cache_kvs=caches)
        ts = torch.tensor(lens, dtype=torch.int32, device=prompt.device)
        for j in range(STEPS):
            if poison:
                for c in caches:
                    for b, n in enumerate(lens):
                        c[:, b, :, n + j:] = float("nan")
            if no_sync:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                outs.append(_run(steps[:, j:j + 1], w, cache_kvs=caches, time_step=ts))
                ts.add_(1)
            finally:
                if no_sync:
                    torch.cuda.set_sync_debug_mode("default")
    return torch.cat(outs, 1)


@pytest.mark.parametrize("heads", [2, 4], ids=["D128", "D64"])
def test_kernel_and_composite_rows_match_fp32_without_a_sync(heads, monkeypatch):
    from paddle_hackathon_amd.ops import hip
    _, lens = _geom()
    B = len(lens)
    w = _weights(heads, seed=20 + heads)
    g = torch.Generator().manual_seed(21)
    prompt = torch.randn(B, max(lens), E, generator=g).bfloat16().float()
    steps = torch.randn(B, STEPS, E, generator=g).bfloat16().float()
    ref = _generate(prompt, steps, w, heads, lens)                            # fp32, CPU
    wg = {k: [t.to(device="cuda", dtype=torch.bfloat16) for t in v] for k, v in w.items()}
    pg, sg = prompt.cuda().bfloat16(), steps.cuda().bfloat16()
    calls = []
    real = hip.decode_attention

    def counted(qkv, qkv_bias, cache, time_step, *a, **k):
        calls.append(time_step.numel())
        return real(qkv, qkv_bias, cache, time_step, *a, **k)
    monkeypatch.setattr(hip, "decode_attention", counted)
    new = _generate(pg, sg, wg, heads, lens, poison=True, no_sync=True)
    assert calls == [B] * (STEPS * LAYERS)                                    # the kernel path, a step per row
    monkeypatch.setenv("PHA_DECODE_ATTN", "0")
    old = _generate(pg, sg, wg, heads, lens, poison=True, no_sync=True)
    assert len(calls) == STEPS * LAYERS                                       # the composite ran this time
    assert bool(torch.isfinite(new).all()) and bool(torch.isfinite(old).all())
    for j in range(STEPS):
        for b in range(B):
            e_new, e_old = _rel(new[b, j], ref[b, j]), _rel(old[b, j], ref[b, j])
            print(f"D={E // heads} step {j} row {b} (ts {lens[b] + j}): e_kernel {e_new:.3e} e_composite {e_old:.3e}")
            assert e_new <= max(2 * e_old, 2.0 ** -8)
            assert e_old <= max(2 * e_new, 2.0 ** -8)
