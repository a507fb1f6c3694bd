"""What the two explicit-schedule engines share (:mod:`.fused_engine`, the all-reduce schedule;
:mod:`.fused_engine_sp`, the sequence-parallel one): everything but the schedule.

* :class:`StepCtx`: what a step's forward derives once (kernel module, chunk bounds, layer
  views, RoPE table, compute-dtype weights, the fp8 map, the per-chunk state) and its backward
  reads again.
* :class:`GradBook`: the backward's gradient bookkeeping -- the gradient arena and its slots,
  the accumulation over the ping-pong chunks, the weight-gradient GEMMs, the DP buckets and the
  epilogue that hands the gradients to autograd.
* the block math as plain functions (attention forward / backward, FFN backward, the CE tail and
  backward, the norm backward).  Each returns tensors; the engine decides which collective to
  launch on them and when, so no function here waits for or launches a TP collective.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.distributed as dist

from ..ops import fp8 as F8
from ..ops import gemm_select as GS
from ..ops import reference
from ..ops.dispatch import K, emb_sort_ahead, shadow
from ..parallel import grad_sync as GSY
from ..parallel import process_manager as pm
from ..parallel import tp_comm


def _wait(h):
    if h is not None:
        h.wait()


class _Layer:
    """Parameter views of one DecoderLayer."""

    def __init__(self, layer):
        a, f = layer.attn, layer.ffn
        self.s1, self.s2 = layer.norm1.scale, layer.norm2.scale
        self.eps1, self.eps2 = layer.norm1.eps, layer.norm2.eps
        self.wqkv, self.bqkv = a.wqkv.weight, a.wqkv.bias
        self.wo, self.bo = a.wo.weight, a.wo.bias
        self.wgu, self.bgu = f.gate_up.weight, f.gate_up.bias
        self.wd, self.bd = f.down_proj.weight, f.down_proj.bias
        self.h, self.hd = a.num_local_heads, a.head_dim

    def params(self):
        return [self.s1, self.wqkv, self.bqkv, self.wo, self.bo, self.s2, self.wgu, self.bgu, self.wd, self.bd]


def collect_params(model) -> List[Optional[torch.Tensor]]:
    ps = [model.embedding.weight]
    for layer in model.layers:
        ps += _Layer(layer).params()
    ps += [model.norm.scale, model.lm_head.weight, model.lm_head.bias]
    return ps


_LAYER_KEYS = ("s1", "wqkv", "bqkv", "wo", "bo", "s2", "wgu", "bgu", "wd", "bd")
_SP_REP = ("s1", "bo", "s2", "bd")   # replicated under SP (layers.py sequence_parallel_grad)


def arena_groups(model, layers, sp: bool):
    """Gradient groups in the order the engine's backward completes them (parallel/grad_sync
    GradArena): the head, the layers top-down (layer 0 after the embedding in the all-reduce
    engine, whose embedding gradient is produced before layer 0's weight gradients), and the
    embedding (+ final norm under SP, whose grad is summed over TP after the step).

    Every slot is registered as (owner, key) -- owner "head" (emb, nf, lm_w, lm_b) or "L<i>" --
    whichever group's range it lies in, so both layouts are looked up the same way
    (``GradBook.V``)."""
    head = model.lm_head
    hp = {"emb": model.embedding.weight, "nf": model.norm.scale, "lm_w": head.weight, "lm_b": head.bias}
    heads = lambda *keys: [(("head", key), hp[key]) for key in keys]
    lay = lambda li, keep: [((f"L{li}", key), q) for key, q in zip(_LAYER_KEYS, layers[li].params()) if keep(key)]
    nL = len(layers)
    if sp:
        # the replicated gradients (norm scales, row-parallel biases: summed over TP after the
        # step) are stored together in one trailing range, "sprep", so that sum is one in-place
        # all-reduce of the arena (grad_sync.allreduce_sequence_parallel_grads)
        top_down = range(nL - 1, -1, -1)
        return ([("head", heads("lm_w", "lm_b"))]
                + [(f"L{li}", lay(li, lambda key: key not in _SP_REP)) for li in top_down]
                + [("tail", heads("emb"))]
                + [("sprep", [x for li in top_down for x in lay(li, lambda key: key in _SP_REP)] + heads("nf"))])
    every = lambda key: True
    return ([("head", heads("nf", "lm_w", "lm_b"))] + [(f"L{li}", lay(li, every)) for li in range(nL - 1, 0, -1)]
            + [("emb", heads("emb")), ("L0", lay(0, every))])


def arena_begin(model, arena) -> bool:
    """Start of a backward over the arena.  True (the common case, ``zero_grad(set_to_none)``
    before the backward): the engine assigns the arena views as the parameters' ``.grad`` itself
    and returns no gradients to autograd (nothing is copied).  False: some ``.grad`` already
    holds an accumulated gradient -- a ``.grad`` that still aliases the arena is detached
    (cloned) first, since this backward overwrites the arena, and the gradients go back through
    autograd, which adds them."""
    params = [p for p in collect_params(model) if p is not None]
    if all(p.grad is None for p in params):
        return True
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + 4 * arena.numel
    for p in params:
        if p.grad is not None and lo <= p.grad.data_ptr() < hi:
            p.grad = p.grad.clone()
    return False


def arena_end(model, grads, assign: bool):
    """The gradients to return from the engine's backward (see ``arena_begin``)."""
    if not assign:
        return grads
    for p, gr in zip(collect_params(model), grads):
        if p is not None and gr is not None:
            p.grad = gr
    return [None] * len(grads)


class StepCtx:
    """One training step's constants and per-chunk state: built by the engine's forward, kept on
    the autograd context and read again by its backward."""

    def __init__(self, model, ids, chunks: int, ignore_index: int):
        dev = ids.device
        self.model, self.ignore_index = model, ignore_index
        self.dt = dt = model.act_dtype(dev)
        self.k = K(model.embedding.weight, model.act_dtype(model.embedding.weight.device))
        self.pg = pm.pgm
        self.tp = 1 if self.pg is None else self.pg.tp_size
        B, self.T = ids.shape
        self.C = max(1, min(chunks, B))
        self.bounds = [(B * i) // self.C for i in range(self.C + 1)]
        self.layers = [_Layer(l) for l in model.layers]
        self.tab = model.rope_table(dev)
        head = model.lm_head
        self.vst = head.odim_start
        self.vvalid = max(0, min(model.vocab_size - self.vst, head.odim_partition))
        self.dim = model.args.attn_dim
        self.recompute = bool(getattr(model.args, "recompute", False))
        self.W = W = lambda w: shadow(w, dt) if w is not None else None  # bf16 compute copies
        # fp8 step: one e4m3 copy (+ transposed copy) of every projection weight, looked up by
        # ops.gemm_select for the forward and the data-gradient GEMMs of this step
        self.f8map = F8.prepare([W(w) for L in self.layers for w in (L.wqkv, L.wo, L.wgu, L.wd)]
                                + [W(head.weight)]) if getattr(model.args, "fp8", False) else None
        F8.activate(self.f8map)     # until the end of the engine's forward; again over its backward
        # per layer: whether its gate|up projection runs with SwiGLU in the GEMM epilogue
        # (GS.swiglu_epilogue: the kernel reads the natural weight with its rows interleaved in
        # 64-row blocks and the backward returns natural-layout gradients, so nothing is copied)
        for L in self.layers:
            L.swi = GS.swiglu_epilogue(self.k, W(L.wgu), getattr(model.args, "swiglu_epilogue", None))
        self.st = []              # per-chunk saved state
        self.n_valid = None

    def chunk_states(self, ids, pos, tgt, reduce, reduce_first: bool = False):
        """The per-chunk state with the embedding rows in flight: ``reduce(x)`` launches the TP
        collective on a chunk's embedding output and returns (residual stream, handle).  It runs
        after the launch of the embedding backward's sort, or before it with ``reduce_first``."""
        k, emb = self.k, self.model.embedding
        for c in range(self.C):
            b0, b1 = self.bounds[c], self.bounds[c + 1]
            ids_c = ids[b0:b1].reshape(-1).contiguous()
            x = k.embedding_fwd(ids_c, emb.weight, emb.vocab_st_idx, self.dt)
            if reduce_first:
                x, h = reduce(x)
            # the embedding backward's sort, on a side stream beside the forward
            esort = emb_sort_ahead(ids_c, emb.vocab_st_idx, emb.weight.size(0)) if k is not reference else None
            s = dict(B=b1 - b0, ids=ids_c, esort=esort, pos=pos[b0:b1].reshape(-1).contiguous(),
                     tgt=tgt[b0:b1].reshape(-1).contiguous(), pend=None, pend_bias=None, layers=[])
            s["x"], s["h"] = (x, h) if reduce_first else reduce(x)
            self.st.append(s)
        return self.st

    def loss_buffers(self, dev):
        """(running sums, loss) written by ``ce_tail``; the valid-row count is kept for backward."""
        acc = torch.empty(2, device=dev, dtype=torch.float32)
        self.n_valid = acc[1]
        return acc, torch.empty((), device=dev, dtype=torch.float32)


class _DeferredAdds:
    """Accumulation of the small fp32 gradients (bias / norm-weight column sums, embedding
    rows) over the chunks of a step.  The first chunk's kernel output is taken as the
    accumulator; later chunks' contributions are queued and added by one multi-tensor launch
    per flush (torch._foreach_add_) instead of one elementwise kernel each -- at TP 2 with two
    chunks that removes ~75 launches of ~5 us from the step (tools/tp_sim.py profile)."""

    def __init__(self):
        self.q = []

    def flush(self):
        while self.q:   # a target may appear once per launch (the foreach kernel runs lists in parallel)
            seen, now, later = set(), [], []
            for a, g in self.q:
                (later if id(a) in seen else now).append((a, g))
                seen.add(id(a))
            torch._foreach_add_([a for a, _ in now], [g for _, g in now])
            self.q = later


class _Owner(dict):
    """The gradients produced so far for one owner of arena slots ("head" or "L<i>"), by key."""

    def __init__(self, name: str):
        super().__init__()
        self.name = name


class GradBook:
    """Gradient bookkeeping of one backward, for both engines.

    fp32 gradients: every one is written straight into its slot of the model's gradient arena
    (parallel/grad_sync.GradArena; the first chunk's contribution in place, later chunks
    accumulated), so the DP all-reduce runs on arena slices with no pack / copy.

    The small fp32 gradients are summed over the chunks through a :class:`_DeferredAdds`.

    DP: each group's gradients are marked complete (``dp_reduce(name)``) as soon as the backward
    is done with them and go out as async all-reduces of contiguous arena slices (buckets of at
    least the measured knee of the DP group's all-reduce curve, parallel/grad_sync; small groups
    are merged), so they overlap the remaining layers.  The deferred sums are flushed before a
    bucket is launched: the bucketer's hook is the queue's ``flush``, not a method of this
    object, which would tie the two into a reference cycle and keep the step's context (and the
    model it names) alive until the next garbage collection."""

    def __init__(self, sc: StepCtx, sp: bool, dev):
        self.sc, self.k = sc, sc.k
        F8.activate(sc.f8map)
        self.defer = _DeferredAdds()
        self.arena = GSY.arena_for(sc.model, arena_groups(sc.model, sc.layers, sp), "sp" if sp else "tp")
        self.assign = arena_begin(sc.model, self.arena)
        self.head = _Owner("head")
        self.layer = [_Owner(f"L{li}") for li in range(len(sc.layers))]
        pg = pm.pgm
        dp = pg.dp_size if pg is not None else 1
        self.dpb = GSY.DPBucketer(self.arena, pg.dp_group if dp > 1 else None, dp,
                                  GSY.dp_bucket_bytes(pg.dp_group, dev) if dp > 1 else 0,
                                  before_launch=self.defer.flush)
        self.dp_reduce = self.dpb.add

    def V(self, G: _Owner, key):
        """The arena slot of gradient ``key`` of owner ``G``."""
        return self.arena.view(G.name, key)

    def first(self, G, key, like, numel):
        """fp32 output buffer of a gradient kernel: the arena slot for the first chunk."""
        return self.V(G, key) if G.get(key) is None else like.new_empty(numel, dtype=torch.float32)

    def add(self, G, key, g):
        """G[key] += g (None: nothing).  The first contribution lands in the gradient's arena
        slot, unless the kernel wrote it there already; later ones are queued (``_DeferredAdds``)."""
        if g is None:
            return
        acc = G.get(key)
        if acc is None:
            G[key] = view = self.V(G, key)
            if g is not view:
                view.copy_(g)
        elif g.dtype == torch.float32 and g.device == acc.device:
            self.defer.q.append((acc, g))
        else:
            acc.add_(g)

    def bias_acc(self, G, key, dy, present):
        if present is not None:
            self.add(G, key, self.k.bias_grad(dy))

    def tn(self, G, key, dy, x):
        acc = G.get(key)
        if acc is None:
            G[key] = GS.gemm_tn(self.k, dy, x, self.V(G, key))
        else:
            GS.gemm_tn(self.k, dy, x, acc, True)

    def tn_chunks(self, G, key, pairs):
        """Weight gradient summed over the chunks ((dy, x) per chunk), issued after the
        last chunk's data-gradient GEMM of the phase: chunks go two at a time through
        GS.gemm_tn_pair (one split-K launch over both chunks' rows, one reduction)."""
        i = 0
        while i < len(pairs):
            if i + 1 < len(pairs):
                (a0, b0), (a1, b1) = pairs[i], pairs[i + 1]
                if G.get(key) is None:
                    G[key] = GS.gemm_tn_pair(self.k, a0, b0, a1, b1, self.V(G, key), False)
                else:
                    GS.gemm_tn_pair(self.k, a0, b0, a1, b1, G[key], True)
                i += 2
            else:
                self.tn(G, key, *pairs[i])
                i += 1
        pairs.clear()

    def tn_multi(self, G, groups):
        """Several weight gradients of one phase ((key, pairs) each): with one or two chunks,
        ONE grouped launch (GS.gemm_tn_group, timed against separate calls); else per key."""
        if all(len(pairs) == 1 for _, pairs in groups) or all(len(pairs) == 2 for _, pairs in groups):
            # (two chunks: each item's rows continue in the other chunk's buffers)
            items = []
            for key, pairs in groups:
                acc = G.get(key)
                items.append((pairs[0][0], pairs[0][1], acc if acc is not None else self.V(G, key),
                              acc is not None) + (tuple(pairs[1]) if len(pairs) == 2 else ()))
            for (key, pairs), o in zip(groups, GS.gemm_tn_group(self.k, items)):
                G[key] = o
                pairs.clear()
            return
        for key, pairs in groups:
            self.tn_chunks(G, key, pairs)

    def finish(self):
        """End of the backward: the queued sums, the collectives' error words, the open DP
        buckets; returns the backward's result tuple (``arena_end``: the gradients are assigned
        as ``.grad`` here, or returned for autograd to add)."""
        sc, model, g = self.sc, self.sc.model, self.head
        self.defer.flush()
        tp_comm.check()   # an xGMI barrier that timed out raises here (host-mapped flag, no sync)
        if self.dpb.finish():
            model._dpfs_dp_reduced = True   # DataParallelGradSync hooks skip this step
        sc.st = None
        grads = [g.get("emb")]
        for L, G in zip(sc.layers, self.layer):
            grads += [G.get(key) if q is not None else None for key, q in zip(_LAYER_KEYS, L.params())]
        grads += [g.get("nf"), g.get("lm_w"), g.get("lm_b") if model.lm_head.bias is not None else None]
        F8.activate(None)
        return (None, None, None, None, None, None) + tuple(arena_end(model, grads, self.assign))


def _split(qkv, B, T, h, hd):
    q = qkv[:, : h * hd].view(B, T, h, hd)
    kk = qkv[:, h * hd: 2 * h * hd].view(B, T, h, hd)
    v = qkv[:, 2 * h * hd: 3 * h * hd].view(B, T, h, hd)
    return q, kk, v


def attn_fwd(sc: StepCtx, L: _Layer, s, h1, out=None):
    """Attention block of one chunk from its normed input: QKV GEMM with RoPE in the epilogue,
    attention, Wo GEMM (no bias: it is added after the collective), written into the staging
    slot ``out`` if given.  Returns (qkv, o, lse, Wo output)."""
    k, W = sc.k, sc.W
    qkv = GS.gemm_nt_rope(k, h1, W(L.wqkv), L.bqkv, s["pos"], sc.tab, 2 * L.h, L.hd)
    q, kk, v = _split(qkv, s["B"], sc.T, L.h, L.hd)
    o, lse = k.attn_fwd(q, kk, v, 1.0 / math.sqrt(L.hd), True)
    pout = GS.gemm_nt(k, o.view(qkv.size(0), L.h * L.hd), W(L.wo), None, out=out)
    return qkv, o, lse, pout


def attn_bwd(sc: StepCtx, gb: GradBook, L: _Layer, G, s, a, g2, out=None):
    """Attention block backward of one chunk from ``g2``, the gradient of the Wo output: Wo
    dgrad, attention backward (inverse RoPE fused into the dq/dk stores, the QKV bias grad into
    their epilogues), QKV dgrad into ``out`` if given.  Returns (dqkv, the input gradient to
    reduce over TP, the QKV bias gradient if that pass produced it): the last goes to
    ``attn_bwd_bias`` once the engine has launched the collective."""
    k, W = sc.k, sc.W
    do = GS.gemm_nn(k, g2, W(L.wo))
    Bc, T = s["B"], sc.T
    q, kk, v = _split(a["qkv"], Bc, T, L.h, L.hd)
    dqkv = torch.empty_like(a["qkv"])
    dq, dk, dv = _split(dqkv, Bc, T, L.h, L.hd)
    dbq = gb.first(G, "bqkv", dqkv, dqkv.size(1)) if L.bqkv is not None else None
    bq_fused = k.attn_bwd(do.view(Bc, T, L.h, L.hd), q, kk, v, a["o"], a["lse"], 1.0 / math.sqrt(L.hd),
                          True, dq, dk, dv, s["pos"], sc.tab, dbias=dbq)
    dh = GS.gemm_nn(k, dqkv, W(L.wqkv), out=out)
    return dqkv, dh, (dbq if bq_fused else None)


def attn_bwd_bias(sc: StepCtx, gb: GradBook, L: _Layer, G, dqkv, dbq):
    """Accumulate the QKV bias gradient of ``attn_bwd``.  Apart from it because it belongs after
    the collective's launch: where the attention backward did not produce the gradient
    (``dbq`` None), it is a column-sum launch of its own."""
    if L.bqkv is not None:
        gb.add(G, "bqkv", dbq if dbq is not None else sc.k.bias_grad(dqkv))


def ffn_bwd(sc: StepCtx, gb: GradBook, L: _Layer, G, a, gq, out=None):
    """FFN backward of one chunk from ``gq``, the gradient of the down projection's output: down
    dgrad with the SwiGLU backward (+ gate|up bias grad) in its epilogue, gate|up dgrad into
    ``out`` if given.  Returns (d gate|up, the input gradient to reduce over TP, the gate|up
    bias gradient or None: for ``gb.add(G, "bgu", ...)`` after the collective's launch)."""
    k, W = sc.k, sc.W
    dbgu = gb.first(G, "bgu", gq, a["gu"].size(1)) if L.bgu is not None else None
    dgu = GS.down_dgrad_swiglu(k, gq, W(L.wd), a["gu"], dbgu, L.swi)
    return dgu, GS.gemm_nn(k, dgu, W(L.wgu), out=out), dbgu


def ce_tail(sc: StepCtx, s, stats, acc, loss, ci: int):
    """Vocab-parallel CE of chunk ``ci`` from its shard's statistics: one (M, 3) all-gather over
    TP, then the loss bookkeeping in one kernel.  Returns (lse, valid)."""
    tp = sc.tp
    if tp > 1:
        allst = stats.new_empty((tp * stats.size(0), 3))
        dist.all_gather_into_tensor(allst, stats, group=sc.pg.tp_group)
        allst = allst.view(tp, -1, 3)
    else:
        allst = stats.unsqueeze(0)
    return sc.k.ce_finalize(allst, s["tgt"], sc.ignore_index, acc, loss, ci == 0, ci == sc.C - 1)


def ce_bwd(sc: StepCtx, gb: GradBook, s, gloss):
    """Two-pass CE backward of one chunk, in place over its logits (d loss / d row = valid *
    gloss / n_valid, one native launch).  Returns the lm_head bias gradient or None: for
    ``gb.add(gb.head, "lm_b", ...)`` after the collective's launch."""
    k, dl = sc.k, s["logits"]
    gs = k.ce_grad_scale(s["valid"], gloss, sc.n_valid)
    db = gb.first(gb.head, "lm_b", dl, dl.size(1)) if sc.model.lm_head.bias is not None else None
    k.ce_bwd(dl, s["tgt"], s["ce_lse"], gs, sc.vst, sc.vvalid, dl, db)    # + lm_head bias grad
    return db


def norm_bwd(sc: StepCtx, gb: GradBook, dy, x, w, r, dres, scale, below=None, dw_out=None):
    """RMSNorm backward (+ residual grad ``dres``) whose pass also yields the bias gradient of
    the projection whose output feeds this residual (column sums of the result).  ``scale`` /
    ``below``: (owner, key) of the norm's scale gradient / of that bias gradient (None: no
    bias).  ``dw_out``: where the kernel writes the scale gradient -- "first": the arena slot
    for the first chunk, a fresh buffer after; "slot": the arena slot for the first chunk, its
    own output after; None: always its own output (copied into the slot by ``gb.add``).
    Returns the input gradient."""
    db = gb.first(*below, dy, dy.size(1)) if below is not None else None
    G, key = scale
    if dw_out == "first":
        dw = gb.first(G, key, x, x.size(1))
    else:
        dw = gb.V(G, key) if dw_out == "slot" and G.get(key) is None else None
    dx, ds = sc.k.rmsnorm_bwd(dy, x, w, r, dres, db, dw_out=dw)
    if db is not None:
        gb.add(*below, db)
    gb.add(G, key, ds)
    return dx
