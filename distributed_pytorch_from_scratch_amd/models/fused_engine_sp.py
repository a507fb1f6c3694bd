"""Explicit-schedule training step with Megatron sequence parallelism (``--sp``).

Same math and kernels as :mod:`.fused_engine` (the shared pieces are in :mod:`.engine_common`),
but the residual stream between the tensor-parallel blocks is sharded over the TP group by
token rows (rank r holds rows ``[r*M/n, (r+1)*M/n)`` of every chunk):

* forward, per block: ``RS`` (reduce-scatter) of the row-parallel output replaces the
  all-reduce; bias + residual + RMSNorm run on the local rows only; an ``AG`` (all-gather) of
  the normed rows feeds the next column-parallel GEMM;
* backward, mirrored: the column-parallel input-gradient is reduce-scattered, the norm
  backward runs on the local rows, and the residual gradient is all-gathered for the
  row-parallel dgrad / wgrad.

The bytes on the wire equal the all-reduce version (RS + AG = one all-reduce), but every
per-token elementwise op (norms, residual adds) does 1/n of the work.  At TP = 8 on the
GPT-2-small bench shape that removes ~19 ms/step of replicated norm work (24 add+RMSNorm
forwards at 537 us and 24 norm backwards at 368 us for 262k rows, profiles/).  The gradients
of the replicated parameters (norm scales, row-parallel biases) come out as per-rank partial
sums over the local rows, exactly like the modular SP layers; ``TrainStep`` sums them over
the TP group (``allreduce_sequence_parallel_grads``), so they end bitwise identical on every
rank.

Chunks (ping-pong) and the per-phase interleaving work as in the all-reduce engine: each
collective is launched async and waited by the next phase of the same chunk, after the other
chunk's phase has been enqueued.  Reference parity: the reference has no sequence
parallelism; the modular layers' SP path (``parallel/comm_ops.py``
``ScatterSeq`` / ``GatherSeq``) computes the same function.
"""
from __future__ import annotations

import torch

from ..ops import fp8 as F8
from ..ops import gemm_select as GS
from ..ops.dispatch import emb_sort_take
from ..parallel import tp_comm
from .engine_common import (GradBook, StepCtx, _wait, attn_bwd, attn_bwd_bias, attn_fwd, ce_bwd, ce_tail, ffn_bwd,
                            norm_bwd)


def _rs(full: torch.Tensor, n: int):
    """Reduce-scatter rows of ``full`` -> (local rows, work)."""
    out = full.new_empty((full.size(0) // n,) + tuple(full.shape[1:]))
    return out, tp_comm.reduce_scatter(out, full, async_op=True)


def _slot(ci: int, rows: int, cols: int, dt):
    """Staging buffer (xGMI communicator slot of chunk ``ci``) for a GEMM output that feeds a
    reduce-scatter, so the collective reads it in place; None -> the GEMM allocates."""
    return tp_comm.staging(ci, (rows, cols), dt, "reduce_scatter")


def _ag(part: torch.Tensor, n: int):
    """All-gather rows of ``part`` -> (full rows, work)."""
    out = part.new_empty((part.size(0) * n,) + tuple(part.shape[1:]))
    return out, tp_comm.all_gather(out, part, async_op=True)


class DecoderTrainFnSP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, ids, pos, tgt, chunks: int, ignore_index: int, *params):
        ctx.sc = sc = StepCtx(model, ids, chunks, ignore_index)
        k, W, dt, dim, n, head = sc.k, sc.W, sc.dt, sc.dim, sc.tp, model.lm_head

        def scatter(x):
            assert x.size(0) % n == 0, "sequence parallelism: chunk rows must divide by tp_size"
            return _rs(x, n)

        st = sc.chunk_states(ids, pos, tgt, scatter, reduce_first=True)
        for L in sc.layers:
            for s in st:    # P1: (bias + residual +) norm1 on my rows -> all-gather
                _wait(s["h"])
                if s["pend"] is not None:
                    s["x"], h1s, r1 = k.add_rmsnorm_fwd(s["pend"], s["pend_bias"], s["x"], L.s1, L.eps1)
                else:
                    h1s, r1 = k.rmsnorm_fwd(s["x"], L.s1, L.eps1)
                h1, s["h"] = _ag(h1s, n)
                s["layers"].append(dict(x=s["x"], r1=r1, h1=h1))
            for ci, s in enumerate(st):    # P2: QKV (+RoPE), attention, Wo -> reduce-scatter
                _wait(s["h"])
                a = s["layers"][-1]
                qkv, o, lse, pout = attn_fwd(sc, L, s, a["h1"], out=_slot(ci, a["h1"].size(0), dim, dt))
                a.update(qkv=qkv, o=o, lse=lse)
                (s["pend"], s["h"]), s["pend_bias"] = _rs(pout, n), L.bo
            for s in st:    # P3: bias + residual + norm2 on my rows -> all-gather
                _wait(s["h"])
                a = s["layers"][-1]
                x2, h2s, r2 = k.add_rmsnorm_fwd(s["pend"], s["pend_bias"], s["x"], L.s2, L.eps2)
                h2, s["h"] = _ag(h2s, n)
                a.update(x2=x2, r2=r2, h2=h2)
                s["x"] = x2
            for ci, s in enumerate(st):    # P4: gate|up, SwiGLU, down -> reduce-scatter
                _wait(s["h"])
                a = s["layers"][-1]
                gu, sw = GS.gate_up(k, a["h2"], W(L.wgu), L.bgu, L.swi)   # SwiGLU in the epilogue
                qout = GS.gemm_nt(k, sw, W(L.wd), None, out=_slot(ci, sw.size(0), dim, dt))
                a.update(gu=gu, sw=sw)
                (s["pend"], s["h"]), s["pend_bias"] = _rs(qout, n), L.bd
                if sc.recompute:       # keep only the layer input; the rest is rebuilt in backward
                    s["layers"][-1] = {"x": a["x"]}
        for s in st:        # final norm on my rows -> all-gather
            _wait(s["h"])
            xf, hfs, rf = k.add_rmsnorm_fwd(s["pend"], s["pend_bias"], s["x"], model.norm.scale, model.norm.eps)
            hf, s["h"] = _ag(hfs, n)
            s.update(xf=xf, rf=rf, hf=hf)
            del s["pend"]
        acc, loss = sc.loss_buffers(ids.device)
        for ci, s in enumerate(st):        # lm_head shard + vocab-parallel CE statistics
            _wait(s["h"])
            logits = GS.gemm_nt(k, s["hf"], W(head.weight), head.bias)
            lse, valid = ce_tail(sc, s, k.ce_fwd_stats(logits, s["tgt"], sc.vst, sc.vvalid), acc, loss, ci)
            s.update(logits=logits, ce_lse=lse, valid=valid, h=None)
        F8.activate(None)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        sc = ctx.sc
        model, st, layers = sc.model, sc.st, sc.layers
        k, W, dt, dim, n, head = sc.k, sc.W, sc.dt, sc.dim, sc.tp, model.lm_head
        nL = len(layers)
        gb = GradBook(sc, True, gloss.device)
        g, gl, dp_reduce = gb.head, gb.layer, gb.dp_reduce

        lm_p = []
        for ci, s in enumerate(st):    # CE backward in place, lm_head dgrad -> reduce-scatter, lm_head wgrad
            db, dl = ce_bwd(sc, gb, s, gloss), s["logits"]
            s["dpend"], s["h"] = _rs(GS.gemm_nn(k, dl, W(head.weight), out=_slot(ci, dl.size(0), dim, dt)), n)
            lm_p.append((dl, s["hf"]))
            gb.add(g, "lm_b", db)
            del s["logits"], s["hf"]
        gb.tn_chunks(g, "lm_w", lm_p)

        def below(li):
            """The down projection under layer li's input (layer li-1's, or the last layer's
            under the final norm at li = nL): its bias grad comes out of that norm's backward."""
            return (gl[li - 1], "bd") if li > 0 and layers[li - 1].bd is not None else None

        for s in st:    # final norm backward on my rows -> all-gather the residual grad
            _wait(s["h"])
            s["g"] = norm_bwd(sc, gb, s["dpend"], s["xf"], model.norm.scale, s["rf"], None, (g, "nf"), below(nL))
            s["gfull"], s["h"] = _ag(s["g"], n)
            del s["xf"], s["rf"], s["dpend"]
        dp_reduce("head")

        def rebuild(L, li):
            """Activation recompute: re-run layer li's forward (with its collectives) from the
            saved layer input, up to the SwiGLU output (the down projection is not needed)."""
            for s in st:
                a = s["layers"][li]
                h1s, a["r1"] = k.rmsnorm_fwd(a["x"], L.s1, L.eps1)
                a["h1"], a["hh"] = _ag(h1s, n)
            for ci, s in enumerate(st):
                a = s["layers"][li]
                _wait(a.pop("hh"))
                a["qkv"], a["o"], a["lse"], pout = attn_fwd(sc, L, s, a["h1"],
                                                            out=_slot(ci, a["h1"].size(0), dim, dt))
                a["pend"], a["hh"] = _rs(pout, n)
            for s in st:
                a = s["layers"][li]
                _wait(a.pop("hh"))
                a["x2"], h2s, a["r2"] = k.add_rmsnorm_fwd(a.pop("pend"), L.bo, a["x"], L.s2, L.eps2)
                a["h2"], a["hh"] = _ag(h2s, n)
            for s in st:
                a = s["layers"][li]
                _wait(a.pop("hh"))
                a["gu"], a["sw"] = GS.gate_up(k, a["h2"], W(L.wgu), L.bgu, L.swi)

        for li in range(nL - 1, -1, -1):
            L, G = layers[li], gl[li]
            if sc.recompute:
                rebuild(L, li)
            wd_p, wgu_p = [], []
            for ci, s in enumerate(st):    # B4: down / SwiGLU / gate|up grads -> reduce-scatter
                _wait(s["h"])
                a, gq = s["layers"][li], s["gfull"]
                # (bd's grad, partial over my rows and summed over TP by TrainStep, came out of
                # the norm backward above this layer)
                wd_p.append((gq, a["sw"]))
                dgu, dh2, dbgu = ffn_bwd(sc, gb, L, G, a, gq, out=_slot(ci, gq.size(0), dim, dt))
                s["dpend"], s["h"] = _rs(dh2, n)
                wgu_p.append((dgu, a["h2"]))
                gb.add(G, "bgu", dbgu)
                del a["sw"], a["gu"], a["h2"], s["gfull"]
            gb.tn_multi(G, [("wd", wd_p), ("wgu", wgu_p)])       # under the chunks' reduce-scatters
            for s in st:    # B3: norm2 backward (+ residual grad) on my rows -> all-gather
                _wait(s["h"])
                a = s["layers"][li]
                s["g"] = norm_bwd(sc, gb, s["dpend"], a["x2"], L.s2, a["r2"], s["g"], (G, "s2"),
                                  (G, "bo") if L.bo is not None else None)
                s["gfull"], s["h"] = _ag(s["g"], n)
                del a["x2"], a["r2"], s["dpend"]
            wo_p, wqkv_p = [], []
            for ci, s in enumerate(st):    # B2: Wo / attention / QKV grads -> reduce-scatter
                _wait(s["h"])
                a, g2 = s["layers"][li], s["gfull"]
                wo_p.append((g2, a["o"].view(g2.size(0), -1)))
                dqkv, dh, dbq = attn_bwd(sc, gb, L, G, s, a, g2, out=_slot(ci, g2.size(0), dim, dt))
                s["dpend"], s["h"] = _rs(dh, n)
                wqkv_p.append((dqkv, a["h1"]))
                attn_bwd_bias(sc, gb, L, G, dqkv, dbq)
                for key in ("qkv", "o", "lse", "h1"):
                    a.pop(key, None)
                del s["gfull"]
            gb.tn_multi(G, [("wo", wo_p), ("wqkv", wqkv_p)])
            for s in st:    # B1: norm1 backward (+ residual grad) on my rows -> all-gather
                _wait(s["h"])
                a = s["layers"][li]
                s["g"] = norm_bwd(sc, gb, s["dpend"], a["x"], L.s1, a["r1"], s["g"], (G, "s1"), below(li))
                s["gfull"], s["h"] = _ag(s["g"], n)
                del a["x"], a["r1"], s["dpend"]
            dp_reduce(f"L{li}")
        ev = gb.V(g, "emb")
        for ci, s in enumerate(st):    # embedding backward over all rows of the chunk (vocab-sharded table)
            _wait(s["h"])
            # deterministic (sorted ids, no atomics): chunk 0 writes every row, the rest add
            perm, seg = emb_sort_take(s.pop("esort", None))
            k.embedding_bwd_sorted(s["gfull"], s["ids"], model.embedding.weight.size(0),
                                   model.embedding.vocab_st_idx, out=ev, accumulate=ci > 0, perm=perm, seg=seg)
            del s["gfull"]
        g["emb"] = ev
        dp_reduce("tail")
        dp_reduce("sprep")
        return gb.finish()
