"""The contract of ops.hip.sample_logits in float64 numpy: the reference of the sampling tests."""
import numpy as np


class RowRef:
    """one row: p (unfiltered softmax of x / temperature), order (stable descending by logit), kept
    (the kept tokens in that order), tokens (the kept tokens by ascending index) and edges (the running
    mass of the renormalised kept set in that index order, edges[0] = 0, edges[-1] = 1)"""

    def __init__(self, x, temperature=1.0, top_k=0, top_p=1.0):
        x = np.asarray(x, dtype=np.float64)
        V = x.shape[0]
        z = x / float(temperature)
        e = np.exp(z - z.max())
        self.p = e / e.sum()
        self.logp = (z - z.max()) - np.log(e.sum())
        self.order = np.argsort(-(x + 0.0), kind="stable")     # ties: ascending index (x + 0.0: -0 is +0)
        K = int(top_k) if top_k > 0 else V
        kept = self.order[:K]
        self.cum = np.cumsum(self.p[kept]) / self.p[kept].sum()   # renormalised prefix masses after top-k
        if top_p < 1.0:
            n = int(np.searchsorted(self.cum, float(top_p), side="left")) + 1   # shortest prefix with mass >= top_p
            kept = kept[:max(1, min(n, K))]
        self.kept = kept
        self.tokens = np.sort(kept)
        m = self.p[self.tokens]
        self.edges = np.concatenate([[0.0], np.cumsum(m) / m.sum()])
        self.edges[-1] = 1.0

    def draw(self, u):
        """the first kept token (ascending index) whose running mass exceeds u"""
        return int(self.tokens[int(np.searchsorted(self.edges[1:], float(u), side="right"))])

    def midpoints(self):
        """(token, u at the middle of its interval, interval width) of every kept token"""
        lo, hi = self.edges[:-1], self.edges[1:]
        return [(int(t), float(0.5 * (a + b)), float(b - a)) for t, a, b in zip(self.tokens, lo, hi)]

    def prefix_mass(self, token):
        """mass of the order's prefix that ends just before ``token`` (unfiltered, no renormalisation)"""
        pos = int(np.nonzero(self.order == token)[0][0])
        return float(self.p[self.order[:pos]].sum())


def random_logits(B, V, seed, std=2.0):
    return np.random.default_rng(seed).normal(0.0, std, size=(B, V))


def designed_row(V=520, seed=0):
    """12 head tokens at scattered indices, probabilities from about 0.3 down to 0.02, three of them
    (positions 5, 6, 7 of the order) with one logit; every other logit is 30 below the smallest head"""
    rng = np.random.default_rng(seed)
    idx = rng.choice(V, size=12, replace=False)
    probs = np.array([0.30, 0.20, 0.12, 0.09, 0.07, 0.05, 0.05, 0.05, 0.03, 0.02, 0.0125, 0.0075])
    head = np.log(probs)
    head = head - head.max() + 4.0
    x = np.full(V, head.min() - 30.0)
    x[idx] = head
    return x, idx
