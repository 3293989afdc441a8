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

(c) with --rows: the time step per batch row (an int32 [B] tensor, pha_decode_attn_rows) at the shapes
    of (a), every arm one captured graph over the 24 caches. The scalar device-step call of this tree
    against the per-row call with B equal steps and, with --parent-lib NAME, against pha_decode_attn
    of a library built from the parent commit's decode_attn.hip (a file name under
    paddle_hackathon_amd/_C/); then eight steps spread evenly over 128..2047 against all eight at 2047.
    "within" is the project's gating rule: the medians differ by no more than the larger min - max
    spread of the two arms.

(d) with --beam: the beam-indirect form (pha_decode_attn_beam) at B = 8 rows in groups of K = 4 and the
    shapes of (a), every arm one captured graph over the 24 caches. (iii) the beam kernel with the
    identity table against the per-row kernel: the price of the table. (iv) the beam kernel with a
    scrambled table against re-ordering the live part of every cache row with torch and then the
    per-row kernel: the design the table replaces.

Prints markdown tables. Usage: python tools/bench_decode_attn.py [--rounds 7] [--iters 960] [--skip-model]
                                                                 [--rows [--parent-lib NAME] [--skip-attention]]
                                                                 [--beam]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddle_hackathon_amd.ops import hip, _abi, _lib  # noqa: E402
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


def bench_rows(rounds, iters, parent_lib):
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).bfloat16()
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.1).bfloat16()
    caches = [torch.randn(2, B, H, MAX_SEQ, D, device="cuda", generator=g).bfloat16() for _ in range(LAYERS)]
    reps = max(4, iters // LAYERS)

    def us(t):
        return f"{t[0] * 1e3 / LAYERS:.2f} ({t[1] * 1e3 / LAYERS:.2f} - {t[2] * 1e3 / LAYERS:.2f})"

    def within(a, b):
        margin = max(a[2] - a[1], b[2] - b[1])
        d = (a[0] - b[0]) * 1e3 / LAYERS
        return f"{d:+.2f} us, margin {margin * 1e3 / LAYERS:.2f}: " + ("within" if abs(a[0] - b[0]) <= margin else
                                                                         "slower" if d > 0 else "faster")

    def capture(fn):
        fn(0)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(LAYERS):
                fn(i)
        return gr

    def raw(L):
        """pha_decode_attn of library L called directly, on one workspace and output of its own: the two
        libraries' arms then differ in nothing but the library"""
        nsplit = -(-MAX_SEQ // hip.DECODE_ATTN_CHUNK)
        ws = torch.empty(B, H, nsplit, D + 2, dtype=torch.float32, device="cuda")
        out = torch.empty(B, 1, H * D, dtype=torch.bfloat16, device="cuda")

        def call(cache, ts_dev):
            _abi.check(L.pha_decode_attn(_abi.DT[qkv.dtype], qkv.data_ptr(), qb.data_ptr(), cache.data_ptr(), None, 0, 0,
                                         D ** -0.5, 0, ts_dev.data_ptr(), out.data_ptr(), ws.data_ptr(), B, H, D,
                                         MAX_SEQ, _abi.stream(qkv)), "pha_decode_attn")
            return out
        return call

    parent = tree = None
    if parent_lib:
        L = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), parent_lib))
        L.pha_decode_attn.restype, L.pha_decode_attn.argtypes = _abi.SIGNATURES["pha_decode_attn"]
        parent, tree = raw(L), raw(_lib.loaded())

    print(f"### (c) per-row time steps: B={B} H={H} D={D} max_seq={MAX_SEQ} bf16, graph replay over {LAYERS} caches, "
          f"us per call, median of {rounds} rounds x {reps} replays (min - max)\n")
    print("| ts | scalar device step | per-row, equal steps | per-row - scalar |" +
          (" scalar, direct call | parent scalar, direct call | this tree - parent |" if parent else "") + " outputs |")
    print("|---|---|---|---|" + ("---|---|---|" if parent else "") + "---|")
    for ts in (127, 1023, 2047):
        one = torch.tensor([ts], dtype=torch.int32, device="cuda")
        rows = torch.full((B,), ts, dtype=torch.int32, device="cuda")
        c = [caches[0].clone() for _ in range(3)]
        outs = [hip.decode_attention(qkv, qb, c[0], one), hip.decode_attention(qkv, qb, c[1], rows)]
        if parent:
            outs.append(parent(c[2], one).clone())
        same = all(torch.equal(outs[0].view(torch.int16), o.view(torch.int16)) for o in outs[1:]) and all(
            torch.equal(c[0].view(torch.int16), x.view(torch.int16)) for x in c[1:len(outs)])
        fns = [lambda i: hip.decode_attention(qkv, qb, caches[i % LAYERS], one),
               lambda i: hip.decode_attention(qkv, qb, caches[i % LAYERS], rows)]
        if parent:
            fns += [lambda i: tree(caches[i % LAYERS], one), lambda i: parent(caches[i % LAYERS], one)]
        graphs = [capture(fn) for fn in fns]
        res = alternate([lambda _, gr=gr: gr.replay() for gr in graphs], reps, rounds)
        print(f"| {ts} | {us(res[0])} | {us(res[1])} | {within(res[1], res[0])} |" +
              (f" {us(res[2])} | {us(res[3])} | {within(res[2], res[3])} |" if parent else "") +
              f" {'bitwise equal' if same else 'DIFFER'} |")
        del graphs
    print()

    spread = [round(128 + j * (2047 - 128) / (B - 1)) for j in range(B)]
    arms = [("all at 2047", [2047] * B), ("spread evenly over 128..2047", spread)]
    graphs, live = [], []
    for _, steps in arms:
        t = torch.tensor(steps, dtype=torch.int32, device="cuda")
        graphs.append(capture(lambda i, t=t: hip.decode_attention(qkv, qb, caches[i % LAYERS], t)))
        live.append(sum(x + 1 for x in steps))
    res = alternate([lambda _, gr=gr: gr.replay() for gr in graphs], reps, rounds)
    print(f"### (c) ragged steps, same shapes: steps {spread}\n")
    print("| steps | live keys (sum over rows) | us per call | time / all-2047 | keys / all-2047 |")
    print("|---|---|---|---|---|")
    for (label, _), r, n in zip(arms, res, live):
        print(f"| {label} | {n} | {us(r)} | {r[0] / res[0][0]:.2f} | {n / live[0]:.2f} |")
    print()


def bench_beam(rounds, iters, K=4):
    """part (d): the beam-indirect form at B rows in groups of K. (iii) identity table against
    pha_decode_attn_rows: the price of the table. (iv) scrambled table against gathering the caches with
    torch and then pha_decode_attn_rows: the design the table replaces."""
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, 3, H, D, device="cuda", generator=g).bfloat16()
    qb = (torch.randn(3, H, D, device="cuda", generator=g) * 0.1).bfloat16()
    caches = [torch.randn(2, B, H, MAX_SEQ, D, device="cuda", generator=g).bfloat16() for _ in range(LAYERS)]
    reps = max(4, iters // LAYERS)
    ident = (torch.arange(B, device="cuda", dtype=torch.int32) % K)[:, None].expand(B, MAX_SEQ).contiguous()
    scram = torch.randint(0, K, (B, MAX_SEQ), device="cuda", generator=g, dtype=torch.int32)
    src = (torch.arange(B, device="cuda") // K * K)[:, None] + scram.long()          # [B, MAX_SEQ] cache rows
    pos = torch.arange(MAX_SEQ, device="cuda")[None, :]

    def us(t):
        return f"{t[0] * 1e3 / LAYERS:.2f} ({t[1] * 1e3 / LAYERS:.2f} - {t[2] * 1e3 / LAYERS:.2f})"

    def verdict(new, old):
        margin = max(new[2] - new[1], old[2] - old[1])
        d = (new[0] - old[0]) * 1e3 / LAYERS
        return f"{d:+.2f} us, margin {margin * 1e3 / LAYERS:.2f}: " + ("within" if abs(new[0] - old[0]) <= margin else
                                                                         "slower" if d > 0 else "faster")

    def capture(fn):
        fn(0)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(LAYERS):
                fn(i)
        return gr

    def gather_then_rows(cache, rows, ts):
        """what a beam step without the table does per layer: re-order the live part of every cache row,
        then the per-row kernel"""
        live = cache[:, :, :, :ts]
        cache[:, :, :, :ts] = live[:, src[:, :ts], :, pos[:, :ts]].permute(2, 0, 3, 1, 4)
        return hip.decode_attention(qkv, qb, cache, rows)

    print(f"### (d) beam-indirect form: B={B} rows, K={K}, H={H} D={D} max_seq={MAX_SEQ} bf16, graph replay over "
          f"{LAYERS} caches, us per call, median of {rounds} rounds x {reps} replays (min - max)\n")
    print("| ts | per-row kernel | beam kernel, identity table | (iii) table - none | beam kernel, scrambled table | "
          "torch gather + per-row kernel | (iv) ratio | identity output |")
    print("|---|---|---|---|---|---|---|---|")
    for ts in (127, 1023, 2047):
        rows = torch.full((B,), ts, dtype=torch.int32, device="cuda")
        c = [caches[0].clone() for _ in range(2)]
        o0 = hip.decode_attention(qkv, qb, c[0], rows)
        o1 = hip.decode_attention(qkv, qb, c[1], rows, cache_indirection=ident, beam_size=K)
        same = torch.equal(o0.view(torch.int16), o1.view(torch.int16)) and torch.equal(c[0].view(torch.int16),
                                                                                         c[1].view(torch.int16))
        fns = [lambda i: hip.decode_attention(qkv, qb, caches[i % LAYERS], rows),
               lambda i: hip.decode_attention(qkv, qb, caches[i % LAYERS], rows, cache_indirection=ident, beam_size=K),
               lambda i: hip.decode_attention(qkv, qb, caches[i % LAYERS], rows, cache_indirection=scram, beam_size=K),
               lambda i: gather_then_rows(caches[i % LAYERS], rows, ts)]
        graphs = [capture(fn) for fn in fns]
        res = alternate([lambda _, gr=gr: gr.replay() for gr in graphs], reps, rounds)
        print(f"| {ts} | {us(res[0])} | {us(res[1])} | {verdict(res[1], res[0])} | {us(res[2])} | {us(res[3])} | "
              f"{res[3][0] / res[2][0]:.1f}x | {'bitwise equal' if same else 'DIFFERS'} |")
        del graphs
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
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--rows", action="store_true", help="part (c): per-row time steps")
    ap.add_argument("--beam", action="store_true", help="part (d): the beam-indirect form")
    ap.add_argument("--parent-lib", default=None,
                    help="file name under paddle_hackathon_amd/_C/ of a library built from the parent commit's "
                         "decode_attn.hip, for the scalar arm of part (c)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_attn needs a GPU")
    print(f"device: {torch.cuda.get_device_name(0)}, DECODE_ATTN_CHUNK = {hip.DECODE_ATTN_CHUNK}\n")
    with torch.no_grad():
        if not a.skip_attention:
            bench_attention(a.rounds, a.iters)
        if a.rows:
            bench_rows(a.rounds, a.iters, a.parent_lib)
        if a.beam:
            bench_beam(a.rounds, a.iters)
    if not a.skip_model:
        bench_model(a.rounds, max(8, a.iters // LAYERS))


if __name__ == "__main__":
    main()
