"""Explicit-schedule forward/backward of the whole TP decoder (the training fast path).

``Transformer.loss()`` runs through :class:`DecoderTrainFn`: one autograd Function whose
forward and hand-written backward call the kernel API directly (``ops.dispatch.K``: HIP
kernels on MI355X, the PyTorch oracle on CPU) in an explicit order.  Same math as the modular
layers (``parallel/layers.py``; the CPU/gloo equivalence tests run this path), but:

* **comm/compute overlap by ping-pong chunks.**  With TP > 1 the batch is split into
  ``chunks`` halves.  Every tensor-parallel all-reduce (row-parallel outputs in forward,
  column-parallel input-grads in backward) is launched ``async_op=True`` (RCCL runs on its own
  HIP stream) and waited only by the *next* segment of the *same* half, after the other half's
  segment has been enqueued on the compute stream:

      fwd  seg1(A) seg1(B) seg2(A)* seg2(B)* ...     seg1 = norm1,QKV,RoPE,attn,Wo -> AR
                                                     seg2 = *wait+bias+residual, norm2,
                                                            gate|up, SwiGLU, down -> AR
      bwd  b2(A) b2(B) b1(A)* b1(B)* ...             b2 = down/SwiGLU/gate|up grads -> AR(dh2)
                                                     b1 = *wait, norm2 bwd, Wo/attn/QKV grads
                                                          -> AR(dh)

  so each all-reduce is hidden behind the other half's GEMMs / attention (the reference issues
  every collective synchronously).  Inside a segment the weight-gradient GEMMs
  are issued after the all-reduce launch, so they overlap it too.
* fp32 weight-gradient accumulation across chunks inside the wgrad GEMM epilogue/reduce,
  norm/bias gradients from deterministic reductions (replicated params stay bitwise identical
  across TP ranks).
* bias + residual add fused in one kernel after the all-reduce; the logits all-gather is
  replaced by the vocab-parallel cross-entropy (one (M,3) stats all-gather per chunk).
* activations saved per chunk: x, normed inputs, roped QKV, attention output + LSE, gate|up,
  SwiGLU output — no (B,H,T,T) tensors.

Supported: RMSNorm blocks without sequence parallelism (the reference architecture and all
presets).  ``ModelArgs.sequence_parallel`` / LayerNorm models use the modular autograd path.

This file is the schedule: the phase loops and every collective launch and wait.  The step
context, the gradient bookkeeping and the block math are shared with the sequence-parallel
engine (:mod:`.fused_engine_sp`) and live in :mod:`.engine_common`.
"""
from __future__ import annotations

import torch

from ..ops import _ext
from ..ops import gemm_select as GS
from ..ops import fp8 as F8
from ..ops.dispatch import emb_sort_take
from ..parallel import process_manager as pm
from ..parallel import tp_comm
from .engine_common import (GradBook, StepCtx, _wait, attn_bwd, attn_bwd_bias, attn_fwd, ce_bwd, ce_tail, ffn_bwd,
                            norm_bwd)


# A/B hook for tools/ab_attr.py, not a user switch: False keeps the two-pass CE at TP 1.
CE_ONE_PASS = True


def _ar(t: torch.Tensor):
    """Async TP all-reduce (RCCL or the xGMI peer-memory kernels: ``parallel/tp_comm.py``)."""
    p = pm.pgm
    if p is None or p.tp_size == 1:
        return None
    return tp_comm.all_reduce(t, async_op=True)


def _slot(ci: int, rows: int, cols: int, dt):
    """Staging buffer (xGMI communicator slot of chunk ``ci``) for a GEMM output that is
    all-reduced in place next (no copy-in); None -> the GEMM allocates.  The reduced tensor
    stays in the slot until the chunk's next staged GEMM, which comes after its consumers."""
    return tp_comm.staging(ci, (rows, cols), dt, "all_reduce")


class DecoderTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, ids, pos, tgt, chunks: int, ignore_index: int, *params):
        ctx.sc = sc = StepCtx(model, ids, chunks, ignore_index)
        k, W, dt, dim, layers, head = sc.k, sc.W, sc.dt, sc.dim, sc.layers, model.lm_head
        st = sc.chunk_states(ids, pos, tgt, lambda x: (x, _ar(x)))
        for L in layers:
            # seg1: (wait + residual), norm1, QKV, RoPE, attention, Wo -> async all-reduce
            for ci, s in enumerate(st):
                _wait(s["h"])
                if s["pend"] is not None:   # residual epilogue of the previous layer fused into norm1
                    s["x"], h1, r1 = k.add_rmsnorm_fwd(s["pend"], s["pend_bias"], s["x"], L.s1, L.eps1)
                else:
                    h1, r1 = k.rmsnorm_fwd(s["x"], L.s1, L.eps1)
                qkv, o, lse, pout = attn_fwd(sc, L, s, h1, out=_slot(ci, h1.size(0), dim, dt))
                s["layers"].append(dict(x=s["x"], r1=r1, h1=h1, qkv=qkv, o=o, lse=lse))
                s["pend"], s["pend_bias"], s["h"] = pout, L.bo, _ar(pout)
            # seg2: wait + bias + residual, norm2, gate|up, SwiGLU, down -> async all-reduce
            for ci, s in enumerate(st):
                _wait(s["h"])
                x2, h2, r2 = k.add_rmsnorm_fwd(s["pend"], s["pend_bias"], s["x"], L.s2, L.eps2)
                gu, sw = GS.gate_up(k, h2, W(L.wgu), L.bgu, L.swi)   # SwiGLU in the epilogue
                qout = GS.gemm_nt(k, sw, W(L.wd), None, out=_slot(ci, sw.size(0), dim, dt))
                s["layers"][-1].update(x2=x2, r2=r2, h2=h2, gu=gu, sw=sw)
                s["x"] = x2
                s["pend"], s["pend_bias"], s["h"] = qout, L.bd, _ar(qout)
                if sc.recompute:       # keep only the layer input; the rest is rebuilt in backward
                    s["layers"][-1] = {"x": s["layers"][-1]["x"]}
        # head: residual, final norm, lm_head shard, vocab-parallel CE statistics.  TP 1 with a
        # unit loss gradient (engine.TrainStep): d logits is written in the same pass over the
        # logits as the statistics (k.ce_fused), so backward does not read them again.
        # the loss bookkeeping (lse, validity, running sums, the mean) in one kernel per chunk
        acc, loss = sc.loss_buffers(ids.device)
        fuse_ce = CE_ONE_PASS and sc.tp == 1 and getattr(model, "_ce_unit_grad", False) and hasattr(k, "ce_fused")
        if fuse_ce:
            gs_all, _ = k.ce_valid_scale(tgt.reshape(-1).contiguous(), ignore_index)
        row0 = 0
        for ci, s in enumerate(st):
            _wait(s["h"])
            xf, hf, rf = k.add_rmsnorm_fwd(s["pend"], s["pend_bias"], s["x"], model.norm.scale, model.norm.eps)
            logits = GS.gemm_nt(k, hf, W(head.weight), head.bias)
            stats = None
            if fuse_ce:
                gs = gs_all[row0:row0 + s["tgt"].numel()]
                db = torch.empty(logits.size(1), device=ids.device, dtype=torch.float32) \
                    if head.bias is not None else None
                stats = k.ce_fused(logits, s["tgt"], gs, sc.vst, sc.vvalid, db)
                if stats is not None:
                    s.update(ce_done=True, ce_db=db)
            if stats is None:
                stats = k.ce_fwd_stats(logits, s["tgt"], sc.vst, sc.vvalid)
            lse, valid = ce_tail(sc, s, stats, acc, loss, ci)
            row0 += s["tgt"].numel()
            s.update(xf=xf, hf=hf, rf=rf, logits=logits, ce_lse=lse, valid=valid)
            del s["pend"], s["h"]
        F8.activate(None)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        sc = ctx.sc
        model, st, layers = sc.model, sc.st, sc.layers
        k, W, dt, dim, C, head = sc.k, sc.W, sc.dt, sc.dim, sc.C, model.lm_head
        nL = len(layers)
        gb = GradBook(sc, False, gloss.device)
        g, gl, dp_reduce = gb.head, gb.layer, gb.dp_reduce

        # ---- head: CE backward in place over the logits, lm_head dgrad -> async AR
        lm_p = []
        for ci, s in enumerate(st):
            dl = s["logits"]
            if s.pop("ce_done", False):     # d logits (and its column sums) came with the forward
                db = s.pop("ce_db")
                # the forward assumed a unit loss gradient (loss(unit_grad=True)); a caller that
                # scaled the loss afterwards would get unscaled gradients.  Checking the value
                # costs a host sync, so it runs in the debug modes (DPFS_SYNC_DEBUG / NAN_CHECK)
                if ci == 0 and (_ext.debug_sync() or _ext.nan_check()) and not bool((gloss == 1).all()):
                    raise RuntimeError("loss(unit_grad=True) was differentiated with a non-unit gradient "
                                       f"({float(gloss.float().mean())}); call loss() without unit_grad when "
                                       "scaling the loss")
            else:
                db = ce_bwd(sc, gb, s, gloss)
            dh = GS.gemm_nn(k, dl, W(head.weight), out=_slot(ci, dl.size(0), dim, dt))
            s["bh"] = _ar(dh)
            s["dpend"] = dh
            lm_p.append((dl, s["hf"]))
            gb.add(g, "lm_b", db)
            del s["logits"]
        gb.tn_chunks(g, "lm_w", lm_p)
        for s in st:
            _wait(s["bh"])
            # (+ bias grad of the last layer's down projection, same pass)
            s["g"] = norm_bwd(sc, gb, s["dpend"], s["xf"], model.norm.scale, s["rf"], None, (g, "nf"),
                              _bd_below(s, layers[-1], gl[-1]), dw_out="first")
            s["dpend"] = None       # s["g"]: grad wrt the last layer's output (residual stream)
            del s["xf"], s["hf"]
        dp_reduce("head")

        def rebuild(L, li):
            """Activation recompute: re-run layer li's forward from its saved input up to the
            SwiGLU output.  The Wo all-reduce runs unstaged: each chunk's staging slot still
            holds the pending norm1 input-grad of layer li+1."""
            for s in st:
                a = s["layers"][li]
                a["h1"], a["r1"] = k.rmsnorm_fwd(a["x"], L.s1, L.eps1)
                a["qkv"], a["o"], a["lse"], a["pout"] = attn_fwd(sc, L, s, a["h1"])
                a["hh"] = _ar(a["pout"])
            for s in st:
                a = s["layers"][li]
                _wait(a.pop("hh"))
                a["x2"], a["h2"], a["r2"] = k.add_rmsnorm_fwd(a.pop("pout"), L.bo, a["x"], L.s2, L.eps2)
                a["gu"], a["sw"] = GS.gate_up(k, a["h2"], W(L.wgu), L.bgu, L.swi)

        def finish_norm1(s, li):
            """Wait for the all-reduce of layer li's norm1 input-grad, run the norm1 backward and
            add it to the residual-stream grad (-> grad wrt layer li's input).  The bias grad of
            layer li-1's down projection (column sums of that residual grad) comes out of the
            same norm-backward pass."""
            a = s["layers"][li]
            _wait(s["bh"])
            below = _bd_below(s, layers[li - 1], gl[li - 1]) if li > 0 else None
            s["g"] = norm_bwd(sc, gb, s["dpend"], a["x"], layers[li].s1, a["r1"], s["g"], (gl[li], "s1"),
                              below, dw_out="slot")
            s["dpend"] = None
            for key in ("x", "r1", "h1"):
                a.pop(key, None)

        # ---- layers, reversed
        for li in range(nL - 1, -1, -1):
            L, G = layers[li], gl[li]
            if sc.recompute:
                rebuild(L, li)
            # b2: down / SwiGLU / gate|up grads -> AR(dh2)
            wd_p, wgu_p = [], []
            for ci, s in enumerate(st):
                if s["dpend"] is not None:     # finish the upper layer: wait, norm1 bwd, residual
                    finish_norm1(s, li + 1)
                a = s["layers"][li]
                gq = s["g"]
                if not s.pop("bd_done", False):
                    gb.bias_acc(G, "bd", gq, L.bd)
                wd_p.append((gq, a["sw"]))
                dgu, dh2, dbgu = ffn_bwd(sc, gb, L, G, a, gq, out=_slot(ci, gq.size(0), dim, dt))
                s["bh"], s["dpend"] = _ar(dh2), dh2
                wgu_p.append((dgu, a["h2"]))
                gb.add(G, "bgu", dbgu)
                del a["sw"], a["gu"]
            # With one chunk (no all-reduce to hide) the down / gate|up weight gradients wait for
            # the Wo / QKV ones: a layer's four go out as one grouped launch at the end of b1
            if C == 1:
                pend_w = [("wd", wd_p), ("wgu", wgu_p)]
            else:
                gb.tn_multi(G, [("wd", wd_p), ("wgu", wgu_p)])        # under the chunks' all-reduces
                pend_w = []
            if li + 1 < nL:
                dp_reduce(f"L{li + 1}")         # layer li+1 is complete (its norm1 grad just landed)
            # b1: wait, norm2 bwd, Wo / attention / QKV grads -> AR(dh)
            wo_p, wqkv_p = [], []
            for ci, s in enumerate(st):
                a = s["layers"][li]
                _wait(s["bh"])
                g2 = norm_bwd(sc, gb, s["dpend"], a["x2"], L.s2, a["r2"], s["g"], (G, "s2"),   # + residual grad, bo grad
                              (G, "bo") if L.bo is not None else None, dw_out="first")
                wo_p.append((g2, a["o"].view(g2.size(0), -1)))
                dqkv, dh, dbq = attn_bwd(sc, gb, L, G, s, a, g2, out=_slot(ci, g2.size(0), dim, dt))
                s["bh"], s["dpend"] = _ar(dh), dh
                wqkv_p.append((dqkv, a["h1"]))
                attn_bwd_bias(sc, gb, L, G, dqkv, dbq)
                s["g"] = g2
                for key in ("x2", "r2", "h2", "qkv", "o", "lse"):
                    a.pop(key, None)
            if li > 0:
                gb.tn_multi(G, pend_w + [("wo", wo_p), ("wqkv", wqkv_p)])
        # layer 0: the embedding gradient first, so its all-reduce (the largest DP bucket) runs
        # under layer 0's Wo / QKV weight-gradient GEMMs
        ev = gb.V(g, "emb")
        for ci, s in enumerate(st):
            finish_norm1(s, 0)
            # deterministic (sorted ids, no atomics): chunk 0 writes every row, the rest add
            perm, seg = emb_sort_take(s.pop("esort", None))
            k.embedding_bwd_sorted(s["g"], s["ids"], model.embedding.weight.size(0), model.embedding.vocab_st_idx,
                                   out=ev, accumulate=ci > 0, perm=perm, seg=seg)
        g["emb"] = ev
        dp_reduce("emb")
        gb.tn_multi(gl[0], pend_w + [("wo", wo_p), ("wqkv", wqkv_p)])
        dp_reduce("L0")
        return gb.finish()


def _bd_below(s, L, G):
    """``norm_bwd``'s ``below`` for the down projection under a norm: its bias grad comes out of
    that norm's backward, so the chunk's b2 phase must not sum it again (``bd`` can arrive from
    either place: the b2 phase produces it where no norm backward ran first)."""
    if L.bd is None:
        return None
    s["bd_done"] = True
    return (G, "bd")
