"""Float64 / stable-sort reference of the beam-search step (ops.hip.beam_search_step) and of a whole
beam search, shared by the beam tests. CPU only.

Semantics. R = B * K rows, row b * K + k being beam k of item b. ``lp = log_softmax(logits)`` (a -inf
logit has lp -inf whatever the rest of its row holds); a finished row has lp = 0 at eos and -inf
elsewhere. ``total[b, k * V + v] = cum[b * K + k] + lp[b * K + k, v]``. The K largest totals of an item
are taken in descending order, equal totals in ascending flat index (a stable sort). Pick j is new
beam j: token = idx % V, parent = idx // V, cum' = total, logprob = lp[parent row, token], finished' =
finished[parent] | (token == eos), len' = len[parent] + !finished[parent]. A pick whose total is -inf
carries token eos, logprob -inf and finished' = 1. Table: for t < ts[r], table'[r, t] = table[group
row of parent[r], t]; table'[r, ts[r]] = parent[r]; nothing else changes.
"""
import torch

MARGIN = 1e-3


def log_probs(logits, finished, eos):
    """[R, V] float64 log probabilities with the finished rows replaced"""
    x = logits.detach().cpu().double()
    lp = torch.log_softmax(x, -1)
    lp = torch.where(x == float("-inf"), float("-inf"), lp)
    fin = finished.cpu().bool()
    done = torch.full((x.shape[1],), float("-inf"), dtype=torch.float64)
    if 0 <= eos < x.shape[1]:
        done[eos] = 0.0
    return torch.where(fin[:, None], done[None, :], lp)


def step(logits, cum, finished, lengths, eos, K, table, ts):
    """one step on CPU copies of the arguments (none is modified). ``ts``: int or int tensor [R].
    Returns a dict: tok int64 [R], parent int32 [R], cum float64 [R], logprob float64 [R], finished
    uint8 [R], lengths int32 [R], table int32 like ``table``, and margin: the smallest gap between
    adjacent totals among ranks 1 .. K + 1 of any group, exact ties inside one row and pairs of -inf
    left out (inf where there is no other pair)"""
    R, V = logits.shape
    G = R // K
    lp = log_probs(logits, finished, eos)
    fin = finished.cpu().bool()
    ln = lengths.cpu().to(torch.int32)
    total = (cum.cpu().double()[:, None] + lp).reshape(G, K * V)
    vals, idx = torch.sort(total, dim=-1, descending=True, stable=True)
    margin = float("inf")
    for g in range(G):
        for j in range(min(K, K * V - 1)):
            a, b = vals[g, j].item(), vals[g, j + 1].item()
            if a == float("-inf") and b == float("-inf"):
                continue
            same_row = idx[g, j].item() // V == idx[g, j + 1].item() // V
            if same_row and a == b:
                continue
            margin = min(margin, a - b)
    vals, idx = vals[:, :K].reshape(R), idx[:, :K].reshape(R)
    parent = idx // V
    dead = vals == float("-inf")
    tok = torch.where(dead, eos, idx % V)
    prow = torch.arange(G).repeat_interleave(K) * K + parent
    logprob = lp.reshape(G, K * V).gather(1, idx.reshape(G, K)).reshape(R)
    logprob = torch.where(dead, float("-inf"), logprob)
    pfin = fin[prow]
    tab = table.cpu().clone()
    new = tab.clone()
    tsr = torch.full((R,), int(ts)) if not isinstance(ts, torch.Tensor) else ts.cpu().reshape(-1).long().expand(R)
    for r in range(R):
        t = int(tsr[r])
        if 0 <= t < tab.shape[1]:
            new[r, :t] = tab[prow[r], :t]
            new[r, t] = parent[r]
    return dict(tok=tok, parent=parent.to(torch.int32), cum=vals, logprob=logprob,
                finished=(pfin | dead | (tok == eos)).to(torch.uint8), lengths=ln[prow] + (~pfin).to(torch.int32),
                table=new, margin=margin)


def beam_search(logits_fn, B, K, n_new, eos=-1, pad=0, length_penalty=0.0, nret=1):
    """a plain beam search: ``logits_fn(histories)`` takes a list of R token lists (what each beam has
    generated so far, the prompt not included; row b * K + k belongs to item b) and returns the next-token
    logits [R, V]. Returns (ids int64 [B * nret, n_new], scores float64 [B * nret, n_new], margin): the
    contract of generate(decode_strategy="beam_search"), and the smallest step margin met"""
    R = B * K
    cum = torch.tensor([0.0] + [float("-inf")] * (K - 1), dtype=torch.float64).repeat(B)
    fin = torch.zeros(R, dtype=torch.uint8)
    ln = torch.zeros(R, dtype=torch.int32)
    hist = [[] for _ in range(R)]
    lps = [[] for _ in range(R)]
    table = torch.zeros(R, 1, dtype=torch.int32)
    margin = float("inf")
    for _ in range(n_new):
        out = step(logits_fn(hist), cum, fin, ln, eos, K, table, 0)
        margin = min(margin, out["margin"])
        prow = (torch.arange(B).repeat_interleave(K) * K + out["parent"].long()).tolist()
        hist = [hist[p] + [int(t)] for p, t in zip(prow, out["tok"])]
        lps = [lps[p] + [float(v)] for p, v in zip(prow, out["logprob"])]
        cum, fin, ln = out["cum"], out["finished"], out["lengths"]
    rank = cum.reshape(B, K)
    if length_penalty != 0.0:
        rank = rank / ln.reshape(B, K).clamp(min=1).double() ** length_penalty
    order = torch.sort(rank, dim=-1, descending=True, stable=True).indices[:, :nret]
    ids = torch.full((B * nret, n_new), pad, dtype=torch.int64)
    scores = torch.zeros((B * nret, n_new), dtype=torch.float64)
    for b in range(B):
        for i in range(nret):
            r = b * K + int(order[b, i])
            ended = False
            for j in range(n_new):
                if not ended:
                    ids[b * nret + i, j] = hist[r][j]
                    scores[b * nret + i, j] = lps[r][j]
                ended = ended or hist[r][j] == eos
    return ids, scores, margin


# ------------------------------------------------------------------------------ step test cases
KINDS = ("random", "quantised", "first_step", "some_finished", "all_finished", "neg_inf", "few_finite", "cross_tie",
         "ragged_ts")
SENTINEL = 77     # table entries the step must not touch
MAX_SEQ = 37


def make_case(kind, dtype, V, R, K, seed, ld=None):
    """CPU inputs of one step: dict(logits [R, V] of ``dtype`` (a view with row stride ``ld``), cum,
    finished, lengths, eos, K, table, ts). ``few_finite`` needs K >= 2, ``cross_tie`` K >= 2."""
    g = torch.Generator().manual_seed(seed)
    G = R // K
    ld = ld or V
    x = torch.randn(R, V, generator=g) * 3.0
    eos = 7
    cum = -(torch.rand(R, generator=g) * 4.0)
    fin = torch.zeros(R, dtype=torch.uint8)
    ln = torch.randint(1, 9, (R,), generator=g, dtype=torch.int32)
    ts = torch.full((R,), 20, dtype=torch.int32)
    if kind == "quantised":      # a few distinct logits: the K-th key has many ties inside a row
        x = torch.randint(0, 4, (R, V), generator=g).float() * 0.75
        cum = -(torch.arange(R).float() * 0.37 + torch.rand(R, generator=g) * 0.2)
    elif kind == "first_step":
        cum = torch.tensor([0.0] + [float("-inf")] * (K - 1)).repeat(G)
        ln.zero_()
    elif kind == "some_finished":
        fin[torch.randperm(R, generator=g)[:max(1, R // 3)]] = 1
    elif kind == "all_finished":
        fin.fill_(1)
    elif kind == "neg_inf":
        x[torch.rand(R, V, generator=g) < 0.3] = float("-inf")
        x[:, 3] = 1.0     # every row keeps a finite logit
    elif kind == "few_finite":   # the first step of a group whose beam 0 has K - 1 finite logits
        cum = torch.tensor([0.0] + [float("-inf")] * (K - 1)).repeat(G)
        keep = torch.rand(R, V, generator=g).argsort(1)[:, :K - 1] + 2   # never tokens 0 and 1: they stay -inf
        keep = keep.clamp(max=V - 1)
        y = torch.full_like(x, float("-inf"))
        y.scatter_(1, keep, x.gather(1, keep))
        x = y
    elif kind == "cross_tie":    # beams 0 and 1 of every group: bit-identical logits and equal cum
        for b in range(G):
            x[b * K + 1] = x[b * K]
            cum[b * K + 1] = cum[b * K]
    elif kind == "ragged_ts":
        ts = torch.randint(1, MAX_SEQ, (G,), generator=g, dtype=torch.int32).repeat_interleave(K)
    buf = torch.full((R, ld), 9.0).to(dtype)     # what lies past V is a large logit: it must never be read
    buf[:, :V] = x.to(dtype)
    table = torch.full((R, MAX_SEQ), SENTINEL, dtype=torch.int32)
    for r in range(R):
        table[r, :int(ts[r])] = torch.randint(0, K, (int(ts[r]),), generator=g, dtype=torch.int32)
    return dict(logits=buf[:, :V], cum=cum.float(), finished=fin, lengths=ln, eos=eos, K=K, table=table, ts=ts)


def case_reference(case):
    return step(case["logits"], case["cum"], case["finished"], case["lengths"], case["eos"], case["K"], case["table"],
                case["ts"])


# cases whose first seed leaves two totals of different beams within MARGIN take the next one
_RESEED = {"ragged_ts-fp16-V519-R16-K16": 1, "random-fp16-V520-R16-K16": 1, "ragged_ts-fp16-V520-R16-K16": 1}


def case_seed(kind, dt, V, R, K):
    import zlib
    name = f"{kind}-{dt}-V{V}-R{R}-K{K}"
    return zlib.crc32(name.encode()) % 100000 + _RESEED.get(name, 0)
