"""Decode attention for cached generation: the split-KV kernels (csrc/kernels/decode_attn.hip)
against the composite that PHA_DECODE_ATTN=0 keeps.

(a) the attention of one layer alone at B = 8, H = 16, D = 128, max_seq = 2048 and
    ts in {127, 1023, 2047}: bias add + cache append + attention over [0, ts], from the raw QKV
    product to the [B, 1, H * D] input of the output projection. The calls walk over as many
    caches as a 24-layer model has, so the keys come from HBM as they do in a model, not from the
    256 MiB Infinity Cache (one cache is 134 MB). The two paths alternate in one process; the
    figure is the median over the rounds. Bytes are the K and V rows [0, ts] the step must read.
(b) one decode step of a 24-layer, E = 2048 fused_multi_transformer (16 heads, FFN 8192) at
    ts = 1023: eager on both paths (host int time step), eager with a device time step, and the
    new path replayed from one captured graph.

Prints markdown tables. Usage: python tools/bench_decode_attn.py [--rounds 7] [--iters 960] [--skip-model]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_hackathon_amd.ops import hip  # noqa: E402
from paddle_hackathon_amd.incubate.nn import functional as FF  # noqa: E402

COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (HBM3E), TB/s
B, H, D, MAX_SEQ, LAYERS = 8, 16, 128, 2048, 24


def composite(qkv, qb, cache, ts):
    """the decode stage's attention as fused_multi_transformer runs it under PHA_DECODE_ATTN=0"""
    x = qkv.reshape(B, -1) + qb.reshape(-1)
    x = x.reshape(B, 1, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    cache[0, :, :, ts:ts + 1] = k
    cache[1, :, :, ts:ts + 1] = v
    k, v = cache[0, :, :, :ts + 1], cache[1, :, :, :ts + 1]
    o = FF._attention(q, k, v, None, 0.0, False, "upscale_in_train", causal=False)
    return o.transpose(1, 2).reshape(B, 1, H * D)


def timed(fn, iters):
    """ms per call: device events around ``iters`` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, rounds):
    """median ms per call of each function, the functions taking turns within every round"""
    for fn in fns:
        timed(fn, min(iters, 2 * LAYERS))   # warm-up
    samples = [[] for _ in fns]
    for _ in range(rounds):
        for s, fn in zip(samples, fns):
            s.append(timed(fn, iters))
    return [(statistics.median(s), min(s), max(s)) for s in samples]


def bench_attention(rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).bfloat16()
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.1).bfloat16()
    caches = [torch.randn(2, B, H, MAX_SEQ, D, device="cuda", generator=g).bfloat16() for _ in range(LAYERS)]
    print(f"### (a) attention of one layer: B={B} H={H} D={D} max_seq={MAX_SEQ} bf16, {LAYERS} caches in turn, "
          f"us per call, median of {rounds} rounds x {iters} calls (min - max)\n")
    print("Eager calls include the host's launch work; the graph columns replay one captured pass over the "
          f"{LAYERS} caches (device time only), and the bandwidth is taken from them.\n")
    print("| ts | kernel, graph | composite, graph | ratio | kernel, eager | composite, eager | ratio | K+V bytes | "
          "kernel TB/s | of 6.29 TB/s | max rel diff |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")

    def us(t, per=1):
        return f"{t[0] * 1e3 / per:.1f} ({t[1] * 1e3 / per:.1f} - {t[2] * 1e3 / per:.1f})"

    for ts in (127, 1023, 2047):
        c_new, c_old = caches[0].clone(), caches[0].clone()
        o_new = hip.decode_attention(qkv, qb, c_new, ts)
        o_old = composite(qkv, qb, c_old, ts)
        diff = ((o_new.float() - o_old.float()).abs().max() / o_old.float().abs().max()).item()
        same_cache = torch.equal(c_new.view(torch.int16), c_old.view(torch.int16))
        fns = [lambda i: hip.decode_attention(qkv, qb, caches[i % LAYERS], ts),
               lambda i: composite(qkv, qb, caches[i % LAYERS], ts)]
        graphs = []
        for fn in fns:
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for i in range(LAYERS):
                    fn(i)
            graphs.append(gr)
        new, old = alternate(fns, iters, rounds)
        gnew, gold = alternate([lambda _: graphs[0].replay(), lambda _: graphs[1].replay()],
                               max(4, iters // LAYERS), rounds)
        nbytes = 2 * B * H * (ts + 1) * D * 2
        tbs = nbytes / (gnew[0] / LAYERS * 1e-3) / 1e12
        print(f"| {ts} | {us(gnew, LAYERS)} | {us(gold, LAYERS)} | {gold[0] / gnew[0]:.2f} | {us(new)} | {us(old)} | "
              f"{old[0] / new[0]:.2f} | {nbytes / 1e6:.1f} MB | {tbs:.2f} | {100 * tbs / COPY_TBS:.0f} % | "
              f"{diff:.2e}{'' if same_cache else ' (caches differ)'} |")
    print()


def bench_model(rounds, iters):
    E, DFF, ts = H * D, 4 * H * D, 1023
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

    def step(time_step, xin=x):
        out, _ = FF.fused_multi_transformer(xin, *w, pre_layer_norm=True, cache_kvs=caches, time_step=time_step)
        return out._t

    def with_switch(value, time_step):
        def fn(_):
            os.environ["PHA_DECODE_ATTN"] = value
            step(time_step)
        return fn

    with torch.no_grad():
        step(ts_dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(ts_dev)
        res = alternate([with_switch("1", ts), with_switch("0", ts), with_switch("1", ts_dev),
                         lambda _: graph.replay()], iters, rounds)
    os.environ.pop("PHA_DECODE_ATTN", None)
    print(f"### (b) one decode step: {LAYERS} layers, E={E}, {H} heads, FFN {DFF}, B={B}, max_seq={MAX_SEQ}, "
          f"ts={ts}, bf16, median of {rounds} rounds x {iters} steps (min - max)\n")
    print("| path | ms per step |")
    print("|---|---|")
    for label, (med, lo, hi) in zip(("eager, decode kernels, host time step", "eager, composite (PHA_DECODE_ATTN=0)",
                                     "eager, decode kernels, device time step",
                                     "graph replay, decode kernels, device time step"), res):
        print(f"| {label} | {med:.3f} ({lo:.3f} - {hi:.3f}) |")
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=960)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_attn needs a GPU")
    print(f"device: {torch.cuda.get_device_name(0)}, DECODE_ATTN_CHUNK = {hip.DECODE_ATTN_CHUNK}\n")
    with torch.no_grad():
        bench_attention(a.rounds, a.iters)
    if not a.skip_model:
        bench_model(a.rounds, max(8, a.iters // LAYERS))


if __name__ == "__main__":
    main()
