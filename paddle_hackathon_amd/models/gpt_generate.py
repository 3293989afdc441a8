"""Cached text generation for ``GPTForPretraining``.

One token costs one decode step instead of a forward over the whole prefix: the prompt runs once
through the context stage of ``incubate.nn.functional.fused_multi_transformer``, which fills
preallocated ``[2, B, H, prompt + max_new, D]`` key / value caches, and every further token runs

    word + position embedding (the position gathered with the int32 device ``time_step``)
    -> fused_multi_transformer(..., time_step=ts, activation="gelu_tanh")   split-KV decode attention,
                                                                            weight-streaming GEMMs
    -> final LayerNorm -> LM head (the tied embedding, [V, E], on skinny_gemm with at most 16 rows)
    -> ops.hip.sample_logits -> time_step += 1

with nothing in the step that syncs the host, so on the GPU the whole step is captured once in a
hipGraph and replayed per token.

Prompts of different lengths (``seq_lens`` or ``attention_mask``) are right-padded to the longest:
under causal attention the padding cannot reach a real position, so the prefill runs unmasked, row
b takes its first token from position ``len_b - 1`` and then decodes with a time step of its own,
``time_step`` being int32 ``[B]``. It overwrites the stale padding rows of its cache as it goes and
never reads a key above its step, so a step streams the live keys of every row and no padding.

Beam search (``decode_strategy="beam_search"``) runs R = B * num_beams rows, row b * K + k being beam k
of item b, through the same step with ``ops.hip.beam_search_step`` in place of the sampler. A beam's
keys stay where they were written: every layer's attention reads them through one int32
``cache_indirection`` table [R, cache length] that the beam step re-orders in place, so nothing is
copied between cache rows, and the prompt is computed and stored once per item (in beam 0's cache row,
which the table names everywhere at the start).

The model's own parameters are used: ``nn.Linear`` weights are ``[in, out]``, the ``[K, N]`` layout
of the kernels, and go in as views. The one exception is the fused QKV projection, whose outputs are
ordered (head, 3, D) while the decode kernels need (3, head, D): the generator keeps one repacked
copy of each layer's QKV weight (``[E, 3, H, D]``, passed with ``trans_qkvw=False``) and bias, and
refreshes it in place when the parameter's version counter changes. At GPT-3 1.3B that copy is
25 MB per layer (600 MB for the 24 layers in bf16).
"""
from __future__ import annotations

import os

import torch

from ..framework.core import Tensor, _wrap
from .. import ops as _ops
from ..ops import conv_gemm as _cg

STRATEGIES = ("greedy_search", "sampling", "beam_search")
EOS_CHECK_EVERY = 16   # decode steps between two host reads of finished.all()


class _State:
    """the static buffers of one decode step over R rows (the batch, or batch * beams for beam search),
    and its captured graph once that exists"""

    def __init__(self, R, cache_len, cfg, dtype, device, ts_per_row, beam):
        H, D = cfg.num_heads, cfg.head_dim

        def zeros(dt, *shape):
            return torch.zeros(*shape, dtype=dt, device=device)
        self.caches = [zeros(dtype, 2, R, H, cache_len, D) for _ in range(cfg.num_layers)]
        self.tok = zeros(torch.int64, R)
        self.ts = zeros(torch.int32, R if ts_per_row else 1)   # one element: every row is at the same step
        self.finished = zeros(torch.uint8, R)
        self.u = self.cum = self.lens = self.ind = None
        if beam:
            self.cum, self.lens = zeros(torch.float32, R), zeros(torch.int32, R)
            self.ind = zeros(torch.int32, R, cache_len)   # the cache-indirection table
            carried = (self.tok, self.ts, self.cum, self.finished, self.lens, self.ind)
        else:
            self.u = zeros(torch.float32, R)   # rewritten before every step, so not carried
            carried = (self.tok, self.finished, self.ts)
        self.carried = carried   # what a step replaces: saved before the warm-up step, put back after it and after capture
        self.out = None   # what the captured step returned: the tensors a replay fills
        self.graph = None
        self.weights_at = None

    def reset(self):
        """a kept state before its next call"""
        for t in self.caches + [self.finished] + ([] if self.ind is None else [self.lens, self.ind]):
            t.zero_()


class GPTGenerator:
    """Cached generation over a ``GPTForPretraining`` (see the module docstring)."""

    def __init__(self, model):
        self.model = model
        self._qkv = {}        # layer index -> (weight version, bias version, repacked weight, repacked bias)
        self._graphs = {}     # (B, cache length, strategy, temperature, top_k, top_p, eos, pad, ragged) -> _State;
        #                       (B, cache length, "beam_search", num_beams, eos) -> _State
        self._eager = set()   # keys whose warm-up step left the kernel path: not tried again
        self.captures = 0     # hipGraph captures so far (a second generate call adds none)
        self.last_caches = None
        self.last_steps = 0   # decode steps the last call ran (fewer than max_new_tokens - 1 after an early stop)

    def clear(self):
        """drop the captured graphs with their static buffers (each key holds its own KV caches) and
        the repacked QKV copies; the next call builds what it needs again"""
        self._graphs.clear()
        self._eager.clear()
        self._qkv.clear()

    # ------------------------------------------------------------------------------ weights
    def _layer_weights(self):
        cfg = self.model.cfg
        H, D, E = cfg.num_heads, cfg.head_dim, cfg.hidden_size
        names = ("ln_s", "ln_b", "qkv_w", "qkv_b", "out_w", "out_b", "fln_s", "fln_b", "f1_w", "f1_b", "f2_w", "f2_b")
        w = {k: [] for k in names}
        for i, layer in enumerate(self.model.gpt.layers):
            qw, qb = layer.self_attn.qkv_proj.weight._t, layer.self_attn.qkv_proj.bias._t
            ent = self._qkv.get(i)
            if ent is None or ent[2].dtype != qw.dtype or ent[2].device != qw.device:
                ent = (-1, -1, torch.empty(E, 3, H, D, dtype=qw.dtype, device=qw.device),
                       torch.empty(3, H, D, dtype=qb.dtype, device=qb.device))
            if ent[0] != qw._version or ent[1] != qb._version:
                ent[2].copy_(qw.detach().view(E, H, 3, D).permute(0, 2, 1, 3))   # in place: a captured graph reads it
                ent[3].copy_(qb.detach().view(H, 3, D).permute(1, 0, 2))
                ent = (qw._version, qb._version, ent[2], ent[3])
            self._qkv[i] = ent
            w["ln_s"].append(layer.norm1.weight._t)
            w["ln_b"].append(layer.norm1.bias._t)
            w["qkv_w"].append(ent[2])
            w["qkv_b"].append(ent[3])
            w["out_w"].append(layer.self_attn.out_proj.weight._t)
            w["out_b"].append(layer.self_attn.out_proj.bias._t)
            w["fln_s"].append(layer.norm2.weight._t)
            w["fln_b"].append(layer.norm2.bias._t)
            w["f1_w"].append(layer.mlp.linear1.weight._t)
            w["f1_b"].append(layer.mlp.linear1.bias._t)
            w["f2_w"].append(layer.mlp.linear2.weight._t)
            w["f2_b"].append(layer.mlp.linear2.bias._t)
        return [w[k] for k in names]

    def _stack(self, x, weights, caches, time_step=None, **beam):
        from ..incubate.nn import functional as FF
        out, _ = FF.fused_multi_transformer(x, *weights, pre_layer_norm=True, epsilon=self.model.cfg.layer_norm_eps,
                                            cache_kvs=caches, time_step=time_step, activation="gelu_tanh",
                                            trans_qkvw=False, **beam)
        return out._t

    def _logits(self, h):
        """final LayerNorm and LM head of h [B, E] -> [B, V]"""
        from ..incubate.nn import functional as FF
        h = self.model.gpt.final_norm(_wrap(h))._t
        w = self.model.gpt.embeddings.word_embeddings.weight._t
        if h.is_cuda and h.shape[0] <= _ops.hip.SKINNY_GEMM_MAX_M and FF._skinny_ok(h, w, True):
            return _ops.hip.skinny_gemm(h, w, True)
        return _cg.matmul_nt(h, w)

    def _sample(self, logits, u, finished, s):
        top_k = 1 if s["strategy"] == "greedy_search" else s["top_k"]
        args = (logits, u, s["temperature"], top_k, s["top_p"], finished, s["eos"], s["pad"])
        if logits.shape[0] > _ops.hip.SAMPLE_MAX_B:   # more rows than a decode batch: no kernel for it
            return _ops.hip._sample_logits_composite(*args)
        return _ops.hip.sample_logits(*args)

    def _step(self, weights, st, s, host_ts=None):
        """one token: reads st.tok / st.ts, appends to st.caches (through st.ind where the state has a
        table), picks with st.u (sampling: returns (ids, logprob)) or replaces the beam state (beam search:
        returns (token, parent, logprob)), writes the new token to st.tok and advances st.ts"""
        emb = self.model.gpt.embeddings
        x = _ops.fused.embedding(st.tok, emb.word_embeddings.weight._t) \
            + emb.position_embeddings.weight._t.index_select(0, st.ts)
        beam = {} if st.ind is None else dict(cache_indirection=st.ind, beam_size=s["beams"])
        h = self._stack(x.unsqueeze(1), weights, st.caches, st.ts if host_ts is None else host_ts, **beam)
        logits = self._logits(h.reshape(h.shape[0], -1))
        if st.ind is None:
            out = self._sample(logits, st.u, st.finished, s)
        else:
            out = _ops.hip.beam_search_step(logits, st.cum, st.finished, st.lens, s["eos"], s["beams"], st.ind, st.ts)
        st.tok.copy_(out[0])
        st.ts.add_(1)
        return out

    # ------------------------------------------------------------------------------ prompts
    @staticmethod
    def _prompt_lens(ids_in, seq_lens, attention_mask):
        """(ids, lens): the prompts right-padded, trailing columns that are padding in every row
        dropped, and the B prompt lengths as Python ints; lens is None where neither argument is given.
        Reads the host once."""
        B, P = ids_in.shape
        if seq_lens is not None and attention_mask is not None:
            raise ValueError("generate: give seq_lens or attention_mask, not both")
        if seq_lens is None and attention_mask is None:
            return ids_in, None
        if seq_lens is not None:
            t = seq_lens._t if isinstance(seq_lens, Tensor) else torch.as_tensor(seq_lens)
            if t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"generate: seq_lens must be {B} ints, got {t.dtype} {tuple(t.shape)}")
            lens = [int(v) for v in t.tolist()]
            if min(lens) < 1 or max(lens) > P:
                raise ValueError(f"generate: every seq_lens entry must be in [1, {P}], got {lens}")
            return ids_in[:, :max(lens)], lens
        m = attention_mask._t if isinstance(attention_mask, Tensor) else torch.as_tensor(attention_mask)
        if tuple(m.shape) != (B, P):
            raise ValueError(f"generate: attention_mask must be [{B}, {P}], got {tuple(m.shape)}")
        m = m.cpu()
        if not bool(((m == 0) | (m == 1)).all()):
            raise ValueError("generate: attention_mask must be bool or 0 / 1")
        m = m != 0
        lens = [int(v) for v in m.sum(1).tolist()]
        first = m.int().argmax(1).tolist()   # column of the first one
        if min(lens) < 1:
            raise ValueError("generate: attention_mask has a row without a token")
        for b in range(B):
            if not bool(m[b, first[b]:first[b] + lens[b]].all()):
                raise ValueError(f"generate: attention_mask row {b} is not one contiguous run of ones")
            if first[b] != 0 and first[b] + lens[b] != P:
                raise ValueError(f"generate: attention_mask row {b} is neither right-padded (the run starts at column "
                                 f"0) nor left-padded (it ends at column {P - 1})")
        if any(first):   # left-padded rows move to the left edge: one gather
            col = torch.arange(P)[None, :] + torch.tensor(first)[:, None]
            ids_in = ids_in.gather(1, col.clamp_(max=P - 1).to(ids_in.device))
        return ids_in[:, :max(lens)], lens

    # ------------------------------------------------------------------------------ generate
    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, decode_strategy="greedy_search", temperature=1.0, top_k=0, top_p=1.0,
                 eos_token_id=None, pad_token_id=0, seed=None, use_graph=None, seq_lens=None, attention_mask=None,
                 num_beams=None, num_return_sequences=1, length_penalty=0.0):
        """``max_new_tokens`` tokens after ``input_ids`` [B, prompt]: (ids int64 [B, max_new_tokens],
        scores fp32 [B, max_new_tokens]), the score being the log probability of the token under the
        temperature-scaled, unfiltered softmax (0 at padded positions).

        ``decode_strategy`` "greedy_search" takes the argmax; "sampling" draws through
        ``ops.hip.sample_logits`` with ``temperature``, ``top_k`` and ``top_p``, its uniforms from
        ``torch.rand`` on a generator seeded with ``seed`` (None: the global generator). Within one mode
        a seed reproduces its output; eager and graph mode are required to agree for greedy search only.
        With ``eos_token_id`` a row that emits it is padded with ``pad_token_id`` from then on, and the
        loop reads ``finished.all()`` every 16 steps to stop early; nothing else syncs the host.

        Prompts of different lengths are given by one of two arguments. ``seq_lens`` (B ints or an
        int tensor): row b's prompt is ``input_ids[b, :seq_lens[b]]`` with 1 <= seq_lens[b] <= prompt, the
        rest is ignored. ``attention_mask`` ([B, prompt], bool or 0 / 1): every row is one non-empty
        contiguous run of ones that starts at column 0 (right-padded) or ends at the last column
        (left-padded; such rows are shifted to the left edge by one gather). Anything else is a
        ``ValueError``; the check reads the host once, before the loop. Row b of the output continues
        its own prompt: the prefill runs unmasked over the longest prompt (causal, so padding reaches
        no real position), the first token comes from position ``len_b - 1`` and the decode steps run
        with a time step per row, reading no padding. Without either argument, or with all lengths
        equal, the call is the uniform one, bit for bit.

        ``decode_strategy`` "beam_search" keeps the ``num_beams`` (K) best continuations of every prompt
        by cumulative log probability (no temperature, ``top_k`` or ``top_p``: a non-default value is a
        ``ValueError``, as is ``num_beams != 1`` with the other strategies). ``num_beams`` has no default
        with beam search: the call runs B * num_beams rows per step, so the width is the caller's to
        name, and leaving it out is a ``ValueError``. A beam that emits
        ``eos_token_id`` is finished and keeps its score. At the end each item's beams are ranked by
        ``score / length ** length_penalty`` (0.0: the plain score; a stable sort) and the first
        ``num_return_sequences`` are returned: ids int64 [B * num_return_sequences, max_new_tokens], the
        best beam first per item, ``pad_token_id`` after a beam's first EOS, and scores of the same
        shape, the log probability of each token along the beam's own history (0 at padded
        positions), so a row of scores sums to the beam's score. ``num_beams=1`` is greedy search, bit
        for bit. The step runs R = B * K rows; up to 16 rows it stays on the kernels and is captured
        like the other strategies (the graph is kept per (B, cache length, num_beams, eos)), above
        that it runs eagerly on the composites and library GEMMs (recorded as fallbacks). The prompt
        is prefilled once per item, not once per beam.

        The model must be in eval mode with ``tensor_parallel_degree == 1``, and
        ``longest prompt + max_new_tokens <= max_position_embeddings``.

        ``use_graph`` None captures the decode step in one hipGraph when the model is on the GPU and
        a warm-up step took the kernel path everywhere (no recorded fallback, device-side time step);
        True insists on it, False runs the same step eagerly. The graph and its static buffers are kept
        on the generator per (B, cache length, strategy, temperature, top_k, top_p, eos, pad, ragged), KV
        caches included; ``GPTGenerator.clear()`` releases them. The prompt lengths are data of the
        ragged graph, not part of its key: one capture serves every mix of lengths with the same
        longest prompt."""
        model, cfg = self.model, self.model.cfg
        if cfg.tensor_parallel_degree != 1:
            raise ValueError("generate: tensor_parallel_degree must be 1")
        if model.training:
            raise RuntimeError("generate: the model is in training mode; call model.eval() first")
        if decode_strategy not in STRATEGIES:
            raise ValueError(f"generate: decode_strategy must be one of {STRATEGIES}, got {decode_strategy!r}")
        beam = decode_strategy == "beam_search"
        if num_beams is None:
            if beam:   # there is no default width: the cost of a call is B * num_beams rows per step
                raise ValueError("generate: decode_strategy='beam_search' needs num_beams (the number of beams per "
                                 "prompt; 1 is greedy search)")
            num_beams = 1
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or num_beams < 1:
            raise ValueError(f"generate: num_beams={num_beams!r} must be an int of at least 1")
        if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) \
                or not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"generate: num_return_sequences={num_return_sequences!r} must be an int in "
                             f"[1, num_beams={num_beams}]")
        if not beam and num_beams != 1:
            raise ValueError(f"generate: num_beams={num_beams} needs decode_strategy='beam_search'")
        if beam and (float(temperature) != 1.0 or int(top_k) != 0 or float(top_p) != 1.0):
            raise ValueError("generate: beam search takes no temperature, top_k or top_p")
        ids_in = input_ids._t if isinstance(input_ids, Tensor) else torch.as_tensor(input_ids)
        if ids_in.dim() != 2 or ids_in.shape[0] < 1 or ids_in.shape[1] < 1:
            raise ValueError(f"generate: input_ids must be [B, prompt], got {tuple(ids_in.shape)}")
        B = ids_in.shape[0]
        ids_in, lens = self._prompt_lens(ids_in, seq_lens, attention_mask)
        P = ids_in.shape[1]   # the longest prompt
        ragged = lens is not None and min(lens) != P
        n_new = int(max_new_tokens)
        if n_new < 1:
            raise ValueError(f"generate: max_new_tokens={max_new_tokens} must be at least 1")
        if P + n_new > cfg.max_position_embeddings:
            raise ValueError(f"generate: prompt {P} + max_new_tokens {n_new} exceeds max_position_embeddings "
                             f"{cfg.max_position_embeddings}")
        wte = model.gpt.embeddings.word_embeddings.weight._t
        dev, dtype = wte.device, wte.dtype
        ids_in = ids_in.to(device=dev, dtype=torch.int64)
        s = dict(strategy=decode_strategy, temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                 eos=-1 if eos_token_id is None else int(eos_token_id), pad=int(pad_token_id))
        if use_graph and not wte.is_cuda:
            raise RuntimeError("generate: use_graph=True needs the model on a GPU")
        cache_len = P + n_new
        if beam:
            if num_beams > cfg.vocab_size:
                raise ValueError(f"generate: num_beams={num_beams} exceeds the vocabulary ({cfg.vocab_size})")
            s.update(beams=num_beams, nret=num_return_sequences, length_penalty=float(length_penalty))
            return self._generate_beam(ids_in, lens, n_new, s, use_graph)
        key = (B, cache_len, s["strategy"], s["temperature"], s["top_k"], s["top_p"], s["eos"], s["pad"], ragged)
        weights = self._layer_weights()
        st, want_graph = self._state_for(key, B, cache_len, ragged, False, use_graph, n_new)

        # uniforms of every step, drawn up front (no per-step generator state in a captured graph)
        gen = None
        if seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
        U = torch.rand(n_new, B, generator=gen, device=dev, dtype=torch.float32)
        out_ids = torch.full((B, n_new), s["pad"], dtype=torch.int64, device=dev)
        out_lp = torch.zeros((B, n_new), dtype=torch.float32, device=dev)

        # prefill: the context stage fills the caches; the first token comes from the last position
        # (of each row's own prompt where the lengths differ)
        x = model.gpt.embeddings(_wrap(ids_in))._t
        h = self._stack(x, weights, st.caches)
        if ragged:
            ts0 = torch.tensor(lens, dtype=torch.int32).to(dev)
            last = h[torch.arange(B, device=dev), ts0.long() - 1]
        else:
            ts0, last = P, h[:, -1]
        ids, lp = self._sample(self._logits(last.contiguous()), U[0].contiguous(), st.finished, s)
        out_ids[:, 0], out_lp[:, 0] = ids, lp
        st.tok.copy_(ids)
        if ragged:
            st.ts.copy_(ts0)   # the int32 [B] lengths
        else:
            st.ts.fill_(ts0)
        # on the CPU the composite takes a uniform step as a Python int (per-row steps stay a tensor)
        self._decode(key, st, weights, s, want_graph, bool(use_graph), n_new, (out_ids.t(), out_lp.t()), U=U,
                     host_ts=None if wte.is_cuda or ragged else P)
        return _wrap(out_ids), _wrap(out_lp)

    def _state_for(self, key, R, cache_len, ts_per_row, beam, use_graph, n_new):
        """(state, want_graph): whether this call is to replay a captured step, and its state: the one
        kept under ``key`` with its graph, reset, or a new one"""
        wte = self.model.gpt.embeddings.word_embeddings.weight._t
        want_graph = wte.is_cuda and use_graph is not False and n_new > 1 \
            and (bool(use_graph) or key not in self._eager)
        st = self._graphs.get(key) if want_graph else None
        if st is None:
            st = _State(R, cache_len, self.model.cfg, wte.dtype, wte.device, ts_per_row, beam)
        else:
            st.reset()
        self.last_caches = st.caches
        return st, want_graph

    def _decode(self, key, st, weights, s, want_graph, required, n_new, outs, U=None, host_ts=None):
        """the decode steps 1 .. n_new - 1 from a state that holds the first token and its step: on the
        captured graph where ``want_graph`` and the capture succeeds or is ``required`` (the state is then
        kept under ``key``), eagerly otherwise. Element
        i of step j's result goes to ``outs[i][j]``; ``U[j]`` are the step's uniforms. Returns the number of
        leading entries of ``outs`` that are filled (fewer than n_new after an early stop)."""
        graph = None
        if want_graph:
            graph = self._graph_for(st, weights, s, required)
            if graph is not None:
                self._graphs[key] = st
            else:
                self._eager.add(key)
        self.last_steps, T = 0, 1
        for j in range(1, n_new):
            self.last_steps = j
            if U is not None:
                st.u.copy_(U[j])
            if graph is not None:
                graph.replay()
                out = st.out
            else:
                out = self._step(weights, st, s, host_ts)
                if host_ts is not None:
                    host_ts += 1
            for o, v in zip(outs, out):
                o[j] = v
            T = j + 1
            if s["eos"] >= 0 and j % EOS_CHECK_EVERY == 0 and bool(st.finished.all()):
                break
        return T

    def _graph_for(self, st, weights, s, required):
        """the captured step of ``st`` (captured now if it is new or the weights moved), or None where
        the warm-up step shows that a piece of it left the kernel path and the graph was not required"""
        at = tuple(t.data_ptr() for group in weights for t in group)
        if st.graph is not None and st.weights_at == at:
            return st.graph
        from ..ops import fallback
        keep = [t.clone() for t in st.carried]
        before = fallback.total()
        self._step(weights, st, s)   # warm-up: what it appends at the first step is rewritten by the first replay
        # the sampling composite is captured like the kernel; the beam composite is not
        clean = fallback.total() == before and os.environ.get("PHA_DECODE_ATTN", "1") != "0" \
            and (st.ind is None or os.environ.get("PHA_BEAM_KERNEL", "1") != "0") \
            and st.caches[0].dtype in (torch.bfloat16, torch.float16) and self.model.cfg.head_dim in (32, 64, 128)
        for t, k in zip(st.carried, keep):
            t.copy_(k)
        if not clean and not required:
            for c in st.caches:   # what the warm-up step appended, at each row's first step
                c[:, torch.arange(c.shape[1], device=c.device), :, st.ts.long().expand(c.shape[1])] = 0
            return None
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st.out = self._step(weights, st, s)
        self.captures += 1
        for t, k in zip(st.carried, keep):   # capture launches nothing: the first replay is step 0
            t.copy_(k)
        st.graph, st.weights_at = g, at
        return g

    # ------------------------------------------------------------------------------ beam search
    def _generate_beam(self, ids_in, lens, n_new, s, use_graph):
        """generate()'s beam-search branch: ``ids_in`` [B, P] on the device, ``lens`` the prompt
        lengths or None"""
        model, dev = self.model, ids_in.device
        B, P = ids_in.shape
        K, eos = s["beams"], s["eos"]
        R, cache_len = B * K, P + n_new
        key = (B, cache_len, "beam_search", K, eos)
        weights = self._layer_weights()
        st, want_graph = self._state_for(key, R, cache_len, True, True, use_graph, n_new)
        # per group: beam 0 starts at 0, the others at -inf, so the first step's K picks all continue beam 0
        st.cum.copy_(torch.tensor([0.0] + [float("-inf")] * (K - 1), dtype=torch.float32).repeat(B))

        # prefill over the B prompts only, into beam 0's cache row of every group (a strided view)
        x = model.gpt.embeddings(_wrap(ids_in))._t
        h = self._stack(x, weights, [c[:, ::K] for c in st.caches])
        if lens is not None and min(lens) != P:
            ts0 = torch.tensor(lens, dtype=torch.int32).to(dev)
            last = h[torch.arange(B, device=dev), ts0.long() - 1]
            ts0 = ts0.repeat_interleave(K)
        else:
            ts0, last = torch.full((R,), P, dtype=torch.int32, device=dev), h[:, -1]
        # the first token: the B logit rows K times through the same beam step, at the prompt's last position
        logits = self._logits(last.contiguous()).repeat_interleave(K, 0)
        toks = torch.zeros((n_new, R), dtype=torch.int64, device=dev)
        pars = torch.zeros((n_new, R), dtype=torch.int64, device=dev)
        lps = torch.zeros((n_new, R), dtype=torch.float32, device=dev)
        st.ts.copy_(ts0 - 1)
        tok, parent, lp = _ops.hip.beam_search_step(logits, st.cum, st.finished, st.lens, eos, K, st.ind, st.ts)
        toks[0], pars[0], lps[0] = tok, parent, lp
        st.tok.copy_(tok)
        st.ts.copy_(ts0)
        T = self._decode(key, st, weights, s, want_graph, bool(use_graph), n_new, (toks, pars, lps))

        # back-trace the K histories, rank each group, keep the first nret
        from ..nn.functional.common import gather_tree
        par3 = pars[:T].reshape(T, B, K)
        seq = gather_tree(toks[:T].reshape(T, B, K), par3)._t           # [T, B, K]
        slp = gather_tree(lps[:T].reshape(T, B, K), par3)._t
        rank = st.cum.reshape(B, K)
        if s["length_penalty"] != 0.0:
            rank = rank / st.lens.reshape(B, K).clamp(min=1).float() ** s["length_penalty"]
        order = torch.sort(rank, dim=-1, descending=True, stable=True).indices[:, :s["nret"]]   # [B, nret]
        pick = order[None].expand(T, B, s["nret"])
        seq = seq.gather(2, pick).permute(1, 2, 0).reshape(B * s["nret"], T)
        slp = slp.gather(2, pick).permute(1, 2, 0).reshape(B * s["nret"], T)
        is_eos = seq == eos
        padded = (is_eos.cumsum(1) - is_eos.long()) > 0                   # after the beam's first EOS
        out_ids = torch.full((B * s["nret"], n_new), s["pad"], dtype=torch.int64, device=dev)
        out_lp = torch.zeros((B * s["nret"], n_new), dtype=torch.float32, device=dev)
        out_ids[:, :T] = torch.where(padded, s["pad"], seq)
        out_lp[:, :T] = torch.where(padded, 0.0, slp)
        return _wrap(out_ids), _wrap(out_lp)
