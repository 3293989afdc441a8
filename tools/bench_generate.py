"""Cached generation: the sampling kernel, the LM head and the whole generate loop.

(a) ops.hip.sample_logits on the kernel (csrc/kernels/sampling.hip) against the torch composite that
    PHA_SAMPLE_KERNEL=0 keeps, bf16 logits [B, 50304] at B = 1 / 8 / 16: greedy, top-k 50, top-p 0.9 and
    both filters. Each arm is one captured graph of 8 calls, so neither pays launch overhead.
(b) the LM head x [M, 2048] . wte[50304, 2048]^T on skinny_gemm against ops.conv_gemm.matmul_nt, each arm
    one captured graph that alternates between two weight buffers (412 MB: past the Infinity Cache).
(c) GPTForPretraining.generate at GPT-3 1.3B, bf16, B = 8, prompt 128, 128 new tokens, once with greedy
    search and once sampling with top-k 50 + top-p 0.9: replayed from the captured graph and eager, each
    with PHA_SAMPLE_KERNEL=0 and 1; tokens/s and ms per token over the whole call (prefill included).

(d) with --ragged: the same model, B = 8, 128 new tokens, greedy, replayed from the graph: prompts of
    16..128 tokens (``seq_lens``, a time step per row) against all eight at 128.

(e) with --beams K: ops.hip.beam_search_step on the kernels (csrc/kernels/beam_search.hip) against the torch
    composite that PHA_BEAM_KERNEL=0 keeps, bf16 logits [R, 50304] at R = 4 / 8 / 16 rows in groups of K, each
    arm one captured graph of 8 calls; and
(f) beam-search generation at GPT-3 1.3B, bf16, B = 2, K beams, prompt 128, 128 new tokens: replayed from the
    captured graph and eager, each with PHA_BEAM_KERNEL=0 and 1 (ms per call, per token, tokens/s per beam row).

The arms alternate in one process; medians over the rounds with min - max. "stays" is the rule of
profiles/decode_gemm/README.md: the kernel's median is below the other arm's by more than the larger
min - max spread of the two.

Prints markdown tables. Usage: python tools/bench_generate.py [--rounds 7] [--iters 20] [--skip-model] [--ragged]
                                                     [--beams 4]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_hackathon_amd.ops import hip, conv_gemm  # noqa: E402

V, E, CALLS = 50304, 2048, 8


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
    fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(CALLS):
            fn(i)
    return g


def us(t):
    return f"{t[0] * 1e3 / CALLS:.2f} ({t[1] * 1e3 / CALLS:.2f} - {t[2] * 1e3 / CALLS:.2f})"


def stays(new, old):
    return "yes" if old[0] - new[0] > max(new[2] - new[1], old[2] - old[1]) else "no"


def bench_sampling(rounds, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    print(f"### (a) sample_logits, bf16 logits [B, {V}] (row stride {V + 8}), {CALLS} calls per graph, us per call, "
          f"median of {rounds} rounds x {iters} replays (min - max)\n")
    print("| filter | B | kernel | composite | speedup | stays |")
    print("|---|---|---|---|---|---|")
    for label, kw in (("greedy", dict(top_k=1)), ("top-k 50", dict(top_k=50)), ("top-p 0.9", dict(top_p=0.9)),
                      ("top-k 50 + top-p 0.9", dict(top_k=50, top_p=0.9))):
        for B in (1, 8, 16):
            logits = [(torch.randn(B, V + 8, device="cuda", generator=gen) * 2).bfloat16()[:, :V] for _ in range(CALLS)]
            u = torch.rand(B, device="cuda", generator=gen)

            def new(i):
                return hip.sample_logits(logits[i], u, **kw)

            def old(i):
                return hip._sample_logits_composite(logits[i], u, **kw)

            graphs = [capture(f) for f in (new, old)]
            tn, to = alternate([lambda _, g=g: g.replay() for g in graphs], iters, rounds)
            print(f"| {label} | {B} | {us(tn)} | {us(to)} | {to[0] / tn[0]:.1f}x | {stays(tn, to)} |")
            del graphs
    print()


def bench_lm_head(rounds, iters):
    gen = torch.Generator(device="cuda").manual_seed(1)
    ws = [(torch.randn(V, E, device="cuda", generator=gen) * E ** -0.5).bfloat16() for _ in range(2)]
    ns, kps = hip.skinny_gemm_plan(V, E, True)
    print(f"### (b) LM head, bf16, N = {V}, K = {E}, W [N, K] (plan {ns} x {kps}), two weight buffers in turn, "
          f"us per call, median of {rounds} rounds x {iters} replays (min - max)\n")
    print("| M | skinny_gemm | matmul_nt | weight TB/s (kernel) | stays |")
    print("|---|---|---|---|---|")
    for M in (1, 8, 16):
        x = torch.randn(M, E, device="cuda", generator=gen).bfloat16()
        graphs = [capture(lambda i: hip.skinny_gemm(x, ws[i % 2], True)),
                  capture(lambda i: conv_gemm.matmul_nt(x, ws[i % 2]))]
        tn, to = alternate([lambda _, g=g: g.replay() for g in graphs], iters, rounds)
        tbs = V * E * 2 / (tn[0] / CALLS * 1e-3) / 1e12
        print(f"| {M} | {us(tn)} | {us(to)} | {tbs:.2f} | {stays(tn, to)} |")
        del graphs
    print()


def bench_generate(rounds, B=8, prompt=128, new=128):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import GPTForPretraining, GPTGenerator, gpt_config
    paddle.set_device("gpu:0")
    paddle.seed(0)
    model = paddle.amp.decorate(GPTForPretraining(gpt_config("gpt3-1.3b")), level="O2", dtype="bfloat16")
    model.eval()
    ids = torch.randint(0, V, (B, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    gens = {"0": GPTGenerator(model), "1": GPTGenerator(model)}   # a captured graph keeps the switch it was captured with
    for label, kw in (("greedy", dict()),
                      ("sampling, top-k 50 + top-p 0.9", dict(decode_strategy="sampling", top_k=50, top_p=0.9, seed=0))):
        _generate_arms(gens, ids, new, rounds, label, kw, B, prompt)


def _generate_arms(gens, ids, new, rounds, what, kw, B, prompt):
    def arm(switch, graph):
        def fn():
            os.environ["PHA_SAMPLE_KERNEL"] = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = gens[switch].generate(ids, new, use_graph=graph, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out._t
        return fn

    arms = [("graph, PHA_SAMPLE_KERNEL=0 (composite)", arm("0", True)), ("graph, PHA_SAMPLE_KERNEL=1", arm("1", True)),
            ("eager, PHA_SAMPLE_KERNEL=0 (composite)", arm("0", False)), ("eager, PHA_SAMPLE_KERNEL=1", arm("1", False))]
    outs = [fn()[1] for _, fn in arms]   # warm-up: captures the graphs
    samples = [[] for _ in arms]
    for _ in range(rounds):
        for s, (_, fn) in zip(samples, arms):
            s.append(fn()[0])
    os.environ.pop("PHA_SAMPLE_KERNEL", None)
    print(f"### (c) generate, GPT-3 1.3B bf16, B = {B}, prompt {prompt}, {new} new tokens, {what}, whole call "
          f"(prefill included), median of {rounds} rounds (min - max)\n")
    print("| path | ms per call | ms per token | tokens/s |")
    print("|---|---|---|---|")
    for (label, _), s in zip(arms, samples):
        med, lo, hi = statistics.median(s), min(s), max(s)
        print(f"| {label} | {med:.1f} ({lo:.1f} - {hi:.1f}) | {med / new:.3f} | {B * new / med * 1e3:.0f} |")
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    print(f"\nthe four arms return {'the same' if same else 'different'} tokens\n")


def bench_ragged(rounds, B=8, prompt=128, new=128):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import GPTForPretraining, GPTGenerator, gpt_config
    paddle.set_device("gpu:0")
    paddle.seed(0)
    model = paddle.amp.decorate(GPTForPretraining(gpt_config("gpt3-1.3b")), level="O2", dtype="bfloat16")
    model.eval()
    ids = torch.randint(0, V, (B, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    lens = [round(16 + j * (prompt - 16) / (B - 1)) for j in range(B)]
    gen = GPTGenerator(model)
    arms = [(f"all prompts {prompt} (one time step)", dict()), (f"prompts {lens} (seq_lens, a step per row)",
                                                              dict(seq_lens=lens))]

    def run(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.generate(ids, new, use_graph=True, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _, kw in arms:
        run(kw)   # warm-up: captures the graph
    samples = [[] for _ in arms]
    for _ in range(rounds):
        for s, (_, kw) in zip(samples, arms):
            s.append(run(kw))
    print(f"### (d) generate, GPT-3 1.3B bf16, B = {B}, {new} new tokens, greedy, graph, whole call (prefill over "
          f"{prompt} positions included), median of {rounds} rounds (min - max); {gen.captures} captures\n")
    print("| prompts | ms per call | ms per token |")
    print("|---|---|---|")
    for (label, _), s in zip(arms, samples):
        med, lo, hi = statistics.median(s), min(s), max(s)
        print(f"| {label} | {med:.1f} ({lo:.1f} - {hi:.1f}) | {med / new:.3f} |")
    print()


def bench_beam_step(rounds, iters, K):
    gen = torch.Generator(device="cuda").manual_seed(3)
    max_seq, ts = 256, 200
    print(f"### (e) beam_search_step, bf16 logits [R, {V}] (row stride {V + 8}), K = {K}, table [R, {max_seq}] at "
          f"step {ts}, {CALLS} calls per graph, us per call, median of {rounds} rounds x {iters} replays (min - max)\n")
    print("| R | kernels | composite | speedup | stays | same picks |")
    print("|---|---|---|---|---|---|")
    for R in (4, 8, 16):
        if R % K:
            continue
        logits = [(torch.randn(R, V + 8, device="cuda", generator=gen) * 2).bfloat16()[:, :V] for _ in range(CALLS)]
        state = lambda: (-torch.rand(R, device="cuda", generator=gen) * 5, torch.zeros(R, dtype=torch.uint8, device="cuda"),
                         torch.ones(R, dtype=torch.int32, device="cuda"),
                         torch.randint(0, K, (R, max_seq), device="cuda", generator=gen, dtype=torch.int32))
        tsr = torch.full((R,), ts, dtype=torch.int32, device="cuda")
        cum0, fin0, len0, tab0 = state()
        sn, so = [t.clone() for t in (cum0, fin0, len0, tab0)], [t.clone() for t in (cum0, fin0, len0, tab0)]
        pn = hip.beam_search_step(logits[0], sn[0], sn[1], sn[2], -1, K, sn[3], tsr)
        po = hip._beam_search_step_composite(logits[0], so[0], so[1], so[2], -1, K, so[3], tsr)
        same = torch.equal(pn[0], po[0]) and torch.equal(pn[1], po[1]) and torch.equal(sn[3], so[3])

        def new(i):
            return hip.beam_search_step(logits[i], sn[0], sn[1], sn[2], -1, K, sn[3], tsr)

        def old(i):
            return hip._beam_search_step_composite(logits[i], so[0], so[1], so[2], -1, K, so[3], tsr)

        graphs = [capture(f) for f in (new, old)]
        tn, to = alternate([lambda _, g=g: g.replay() for g in graphs], iters, rounds)
        print(f"| {R} | {us(tn)} | {us(to)} | {to[0] / tn[0]:.1f}x | {stays(tn, to)} | {'yes' if same else 'no'} |")
        del graphs
    print()


def bench_beam_generate(rounds, K, B=2, prompt=128, new=128):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.models import GPTForPretraining, GPTGenerator, gpt_config
    paddle.set_device("gpu:0")
    paddle.seed(0)
    model = paddle.amp.decorate(GPTForPretraining(gpt_config("gpt3-1.3b")), level="O2", dtype="bfloat16")
    model.eval()
    ids = torch.randint(0, V, (B, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    gens = {"0": GPTGenerator(model), "1": GPTGenerator(model)}   # a captured graph keeps the switch it was captured with

    def arm(switch, graph):
        def fn():
            os.environ["PHA_BEAM_KERNEL"] = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = gens[switch].generate(ids, new, use_graph=graph, decode_strategy="beam_search", num_beams=K)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out._t
        return fn

    arms = [("graph, PHA_BEAM_KERNEL=0 (composite)", arm("0", True)), ("graph, PHA_BEAM_KERNEL=1", arm("1", True)),
            ("eager, PHA_BEAM_KERNEL=0 (composite)", arm("0", False)), ("eager, PHA_BEAM_KERNEL=1", arm("1", False))]
    outs = [fn()[1] for _, fn in arms]   # warm-up: captures the graphs
    samples = [[] for _ in arms]
    for _ in range(rounds):
        for s, (_, fn) in zip(samples, arms):
            s.append(fn()[0])
    os.environ.pop("PHA_BEAM_KERNEL", None)
    print(f"### (f) generate, beam search, GPT-3 1.3B bf16, B = {B}, K = {K} ({B * K} rows), prompt {prompt}, {new} new "
          f"tokens, whole call (prefill over the {B} prompts included), median of {rounds} rounds (min - max)\n")
    print("| path | ms per call | ms per token | row tokens/s |")
    print("|---|---|---|---|")
    for (label, _), s in zip(arms, samples):
        med, lo, hi = statistics.median(s), min(s), max(s)
        print(f"| {label} | {med:.1f} ({lo:.1f} - {hi:.1f}) | {med / new:.3f} | {B * K * new / med * 1e3:.0f} |")
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    print(f"\nthe four arms return {'the same' if same else 'different'} tokens\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-sampling", action="store_true")
    ap.add_argument("--skip-lm-head", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--ragged", action="store_true", help="part (d): prompts of different lengths")
    ap.add_argument("--beams", type=int, default=0, help="parts (e) and (f): beam search with this many beams")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate needs a GPU")
    print(f"device: {torch.cuda.get_device_name(0)}\n")
    with torch.no_grad():
        if not a.skip_sampling:
            bench_sampling(a.rounds, a.iters)
        if not a.skip_lm_head:
            bench_lm_head(a.rounds, a.iters)
        if not a.skip_model:
            bench_generate(a.rounds)
        if a.ragged:
            bench_ragged(a.rounds)
        if a.beams:
            bench_beam_step(a.rounds, a.iters, a.beams)
            if not a.skip_model:
                bench_beam_generate(a.rounds, a.beams)


if __name__ == "__main__":
    main()
