"""The decode step's small-batch products: the weight-streaming kernels (csrc/kernels/skinny_gemm.hip)
against the library calls that PHA_DECODE_GEMM=0 keeps.

(b) per product at M = 8, bf16: the four shapes of an E = 2048 layer (FFN 8192), the QKV one in both
    weight layouts, plus M = 1 and M = 16 for the output projection. Each arm is one captured graph
    that walks over 24 distinct weight buffers, so no weight is served from L2 or the 256 MiB
    Infinity Cache. Arms: the kernel with its epilogue; the library call it replaces; the library
    call plus the elementwise passes the epilogue absorbs (bias + GELU, residual add), as
    fused_multi_transformer runs them. The arms alternate in one process; medians over the rounds.
(c) one decode step of the 24-layer model of tools/bench_decode_attn.py part (b), PHA_DECODE_GEMM=0
    against 1, eager (device time step) and replayed from a captured graph, alternating.

--profile-step N replays the captured step N times and exits (for a kernel trace of one arm; the
switch is taken from the environment).

Prints markdown tables. Usage: python tools/bench_decode_gemm.py [--rounds 7] [--iters 40] [--skip-model]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_hackathon_amd.ops import hip, fused  # noqa: E402
from paddle_hackathon_amd.incubate.nn import functional as FF  # noqa: E402

ATTN_TBS = 5.0    # decode_attn_partial's streaming rate (profiles/decode_attn/README.md), TB/s
COPY_TBS = 6.29   # float4 copy rate of the MI355X used there, TB/s
B, H, D, MAX_SEQ, LAYERS = 8, 16, 128, 2048, 24
E, DFF = H * D, 4 * H * D


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, rounds):
    """median, min, max ms per call of each function, the functions taking turns within every round"""
    for fn in fns:
        timed(fn, min(iters, 4))
    samples = [[] for _ in fns]
    for _ in range(rounds):
        for s, fn in zip(samples, fns):
            s.append(timed(fn, iters))
    return [(statistics.median(s), min(s), max(s)) for s in samples]


def capture(fn):
    """one graph that calls fn(i) for every weight buffer in turn"""
    fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(LAYERS):
            fn(i)
    return g


def bench_products(rounds, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)

    def r(*shape, s=1.0):
        return (torch.randn(*shape, device="cuda", generator=gen) * s).bfloat16()

    # name, M, N, K, w_is_nk, bias in the epilogue, activation, residual
    cases = [("qkv [N,K]", 8, 3 * E, E, True, False, "none", False),
             ("qkv [K,N]", 8, 3 * E, E, False, False, "none", False),
             ("out proj", 8, E, E, False, True, "none", True),
             ("ffn1 + GELU", 8, DFF, E, False, True, "gelu", False),
             ("ffn2", 8, E, DFF, False, True, "none", True),
             ("out proj", 1, E, E, False, True, "none", True),
             ("out proj", 16, E, E, False, True, "none", True)]
    print(f"### (b) per product, bf16, {LAYERS} weight buffers in turn inside one graph, us per call, median of "
          f"{rounds} rounds x {iters} replays (min - max)\n")
    print("| product | M | N | K | nsplit x k | kernel | library | library + elementwise | weight bytes | kernel TB/s | "
          f"of {ATTN_TBS} | of {COPY_TBS} | stays |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")

    def us(t):
        return f"{t[0] * 1e3 / LAYERS:.2f} ({t[1] * 1e3 / LAYERS:.2f} - {t[2] * 1e3 / LAYERS:.2f})"

    for name, M, N, K, nk, has_bias, act, has_res in cases:
        ws = [r(N, K, s=K ** -0.5) if nk else r(K, N, s=K ** -0.5) for _ in range(LAYERS)]
        x, bias, res = r(M, K), (r(N) if has_bias else None), (r(M, N) if has_res else None)

        def new(i):
            return hip.skinny_gemm(x, ws[i], nk, bias, act, res)

        def lib(i):
            w = ws[i].t() if nk else ws[i]
            if bias is not None and act == "none":
                return torch.addmm(bias, x, w)      # _linear folds the bias into the library call
            return x @ w

        def lib_elt(i):
            y = lib(i)
            if act == "gelu":
                y = fused.bias_gelu(y, bias, False)
            if res is not None:
                y = res + y
            return y

        graphs = [capture(f) for f in (new, lib, lib_elt)]
        tn, tl, te = alternate([lambda _, g=g: g.replay() for g in graphs], iters, rounds)
        nbytes = N * K * 2
        tbs = nbytes / (tn[0] / LAYERS * 1e-3) / 1e12
        spread = max(tn[2] - tn[1], te[2] - te[1])
        stays = "yes" if te[0] - tn[0] > spread else "no"
        ns, kps = hip.skinny_gemm_plan(N, K, nk)
        print(f"| {name} | {M} | {N} | {K} | {ns} x {kps} | {us(tn)} | {us(tl)} | {us(te)} | {nbytes / 1e6:.1f} MB | "
              f"{tbs:.2f} | {100 * tbs / ATTN_TBS:.0f} % | {100 * tbs / COPY_TBS:.0f} % | {stays} |")
        del graphs, ws
        torch.cuda.empty_cache()
    print()


def model_step():
    ts = 1023
    g = torch.Generator(device="cuda").manual_seed(1)

    def r(*shape, s=0.02):
        return (torch.randn(*shape, device="cuda", generator=g) * s).bfloat16()

    names = ("ln_scales", "ln_biases", "qkv_weights", "qkv_biases", "linear_weights", "linear_biases",
             "ffn_ln_scales", "ffn_ln_biases", "ffn1_weights", "ffn1_biases", "ffn2_weights", "ffn2_biases")
    shapes = {"ln_scales": (E,), "ln_biases": (E,), "qkv_weights": (3, H, D, E), "qkv_biases": (3, H, D),
              "linear_weights": (E, E), "linear_biases": (E,), "ffn_ln_scales": (E,), "ffn_ln_biases": (E,),
              "ffn1_weights": (E, DFF), "ffn1_biases": (DFF,), "ffn2_weights": (DFF, E), "ffn2_biases": (E,)}
    w = [[(1.0 + r(*shapes[n])).bfloat16() if n.endswith("ln_scales") else r(*shapes[n]) for _ in range(LAYERS)]
         for n in names]
    caches = [r(2, B, H, MAX_SEQ, D, s=1.0) for _ in range(LAYERS)]
    x = r(B, 1, E, s=1.0)
    ts_dev = torch.tensor([ts], dtype=torch.int32, device="cuda")

    def step():
        out, _ = FF.fused_multi_transformer(x, *w, pre_layer_norm=True, cache_kvs=caches, time_step=ts_dev)
        return out._t

    return step


def capture_step(step, value):
    if value is not None:
        os.environ["PHA_DECODE_GEMM"] = value
    out = step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph, out


def bench_model(rounds, iters):
    step = model_step()

    def eager(value):
        def fn(_):
            os.environ["PHA_DECODE_GEMM"] = value
            step()
        return fn

    with torch.no_grad():
        g0, o0 = capture_step(step, "0")
        g1, o1 = capture_step(step, "1")
        res = alternate([eager("0"), eager("1"), lambda _: g0.replay(), lambda _: g1.replay()], iters, rounds)
    os.environ.pop("PHA_DECODE_GEMM", None)
    diff = ((o1.float() - o0.float()).abs().max() / o0.float().abs().max()).item()
    print(f"### (c) one decode step: {LAYERS} layers, E={E}, {H} heads, FFN {DFF}, B={B}, max_seq={MAX_SEQ}, ts=1023, "
          f"bf16, device time step, median of {rounds} rounds x {iters} steps (min - max)\n")
    print("| path | ms per step |")
    print("|---|---|")
    for label, (med, lo, hi) in zip(("eager, PHA_DECODE_GEMM=0 (library GEMMs)", "eager, PHA_DECODE_GEMM=1",
                                     "graph replay, PHA_DECODE_GEMM=0", "graph replay, PHA_DECODE_GEMM=1"), res):
        print(f"| {label} | {med:.3f} ({lo:.3f} - {hi:.3f}) |")
    print(f"\nmax rel diff of the step's output between the arms: {diff:.2e}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    ap.add_argument("--profile-step", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_gemm needs a GPU")
    if a.profile_step:
        with torch.no_grad():
            graph, _ = capture_step(model_step(), None)
            for _ in range(a.profile_step):
                graph.replay()
        torch.cuda.synchronize()
        print(f"replayed the captured step {a.profile_step} times (PHA_DECODE_GEMM="
              f"{os.environ.get('PHA_DECODE_GEMM', 'unset')})")
        return
    print(f"device: {torch.cuda.get_device_name(0)}\n")
    with torch.no_grad():
        if not a.skip_products:
            bench_products(a.rounds, a.iters)
        if not a.skip_model:
            bench_model(a.rounds, a.iters)


if __name__ == "__main__":
    main()
