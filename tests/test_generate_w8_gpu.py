"""``generate(..., weight_only="int8")`` on the GPU in bf16: the model pair, prompt length and yardstick of
tests/test_generate_gpu.py with 2 heads (D = 128). The reference is the fp32 CPU model with its four matrices
per layer replaced by their dequantised values, run uncached over prompt + generated ids; e_old is the
max-normalised logit error of the bf16 uncached forward against the fp32 model it mirrors, measured here."""
import pytest
import torch

from test_generate_gpu import B, LAYERS, NEW, _pair
from weight_only_reference import dequantised_copy

pytestmark = pytest.mark.gpu


def test_greedy_runs_on_the_int8_kernel_and_matches_the_dequantised_fp32_model(monkeypatch):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.ops import fallback, hip
    gpu, cpu, ids = _pair(2)
    rows, real = [], hip.skinny_gemm_w8
    monkeypatch.setattr(hip, "skinny_gemm_w8", lambda x, *a, **k: rows.append(x.shape[0]) or real(x, *a, **k))
    monkeypatch.setenv("PHA_STRICT_NATIVE", "1")           # a fallback anywhere in the step raises
    before = fallback.total()
    out, _ = gpu.generate(ids.cuda(), NEW, use_graph=False, weight_only="int8")
    monkeypatch.delenv("PHA_STRICT_NATIVE")
    assert fallback.total() == before
    assert rows == [B] * (4 * LAYERS * (NEW - 1))           # four calls per layer per decode step, none in the prefill
    out = out._t.cpu()
    full, P = torch.cat([ids, out], 1), ids.shape[1]
    with torch.no_grad():
        ref = dequantised_copy(cpu)(paddle.to_tensor(full.numpy()))._t.float()
        plain = cpu(paddle.to_tensor(full.numpy()))._t.float()
        paddle.set_device("gpu:0")
        try:
            old = gpu(paddle.to_tensor(full.cuda()))._t.float().cpu()
        finally:
            paddle.set_device("cpu")
    e_old = ((old - plain).abs().max() / plain.abs().max()).item()
    tol = max(2 * e_old, 2.0 ** -8)
    for j in range(NEW):
        lg = ref[:, P - 1 + j]
        short = (lg.max(-1).values - lg.gather(1, out[:, j:j + 1])[:, 0]) / lg.abs().max(-1).values
        print(f"step {j}: token {short.max().item():.3e} below the dequantised fp32 maximum (e_old {e_old:.3e}, bound {tol:.3e})")
        assert short.max().item() <= tol


def test_graph_equals_eager_is_reused_and_leaves_the_bf16_mode_alone():
    from paddle_hackathon_amd.models import GPTGenerator
    gpu, _, ids = _pair(2)
    gen = GPTGenerator(gpu)
    plain, _ = gen.generate(ids.cuda(), NEW, use_graph=False)
    eager, _ = gen.generate(ids.cuda(), NEW, use_graph=False, weight_only="int8")
    assert gen.captures == 0
    graph, graph_scores = gen.generate(ids.cuda(), NEW, use_graph=True, weight_only="int8")
    assert gen.captures == 1 and torch.equal(eager._t, graph._t)          # token for token
    again, again_scores = gen.generate(ids.cuda(), NEW, weight_only="int8")
    assert gen.captures == 1 and torch.equal(again._t, graph._t) and torch.equal(again_scores._t, graph_scores._t)
    after, _ = gen.generate(ids.cuda(), NEW)                              # weight_only=None: a graph of its own
    assert gen.captures == 2 and torch.equal(after._t, plain._t)
