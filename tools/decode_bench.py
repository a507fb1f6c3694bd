"""Greedy decode throughput: HIP-graph-replayed decode step vs the eager step vs the
reference's full recompute per token (test.py:144-150), one GPU.

    python tools/decode_bench.py [--model gpt2-small] [--batch 1 8] [--prompt 128] [--new 256]
                                 [--temperature T --top_k K --top_p P] [--repeats R] [--sample-kernel]
                                 [--per-row] [--seeds {fixed,fresh}]
                                 [--ragged | --ragged-equal]
                                 [--prefill-chunk N [N ...]] [--continuation --t0 1024 --chunk 256]
                                 [--kv-dtype {act,fp8,both}] [--modes graph eager]
                                 [--penalties R,P,F] [--logprobs]
                                 [--ragged --kv-page N [N ...]]
                                 [--weight-dtype {act,fp8,mxfp4,both,all}] [--layers N] [--w8-kernel]

Prints one JSON line per (batch, mode): ms per generated token (per step of the batch) and
tokens/s (batch x steps / time).  ``--temperature`` > 0 decodes with the sampling step
(``sample_logits`` in place of ``argmax``; the full-recompute baseline is then skipped);
``--repeats`` times each (batch, mode) that many times; ``--sample-kernel`` times the
``sample_logits`` launch alone on bf16 rows of the model's padded vocabulary.

``--per-row`` gives the same settings as per-row lists (``generate`` with sequences: the settings
are device data, one captured graph pair serves them all) with a fresh seed list on every call;
``--seeds fixed`` keeps one seed list, and ``--seeds fresh`` without ``--per-row`` gives the scalar
path a new seed on every call, which recaptures its graphs each time.  ``--sample-kernel
--per-row`` times the ``_sample_logits_rows`` launch alone.

``--ragged`` decodes a ragged batch (``generate(..., prompt_lens=...)``, the per-row decode
kernels): the prompt lengths of a batch are spread evenly over [prompt/4, prompt] (row b of B:
``prompt/4 + b (prompt - prompt/4) / (B - 1)``), every row generates ``--new`` ids, and a
"one-by-one" line times the same prompts decoded one after the other at batch 1 (uniform path,
each with its session warm).  ``--ragged-equal`` runs the per-row path with every length =
``--prompt``: against the plain run, the price of the per-row length loads.

``--prefill-chunk N [N ...]`` times the prefill alone (``logits_step`` of a ``--prompt``-id prompt
up to the first token's logits: time to first token) whole and in pieces of each N, with the
peak allocation above the cache (``max_memory_allocated``).  ``--continuation`` times one
``--chunk``-token continuation of a cache that holds ``--t0`` ids, on the kernels
(``_kv_append_chunk`` + ``_attn_extend``) and on the framework formulation they replaced (slice
assignment, fp32 einsum / softmax / einsum over the whole cache), in interleaved rounds
(``--repeats`` of them) with the medians.

``--kv-dtype fp8`` decodes with the fp8 KV cache (``generate(..., kv_dtype="fp8")``); ``both`` runs
the activation-dtype cache and the fp8 cache in interleaved rounds (``--repeats`` of them, each
dtype's session warm) and adds one line per (batch, mode, dtype) with the median and the kept
session's cache bytes.  ``--modes`` restricts the run to the graph or the eager step.

``--penalties R,P,F`` (repetition, presence, frequency) and ``--logprobs`` add the penalised form
of the sampling launch (``generate(..., repetition_penalty=R, ..., return_logprobs=True)``) to the
same interleaved rounds: every round then times the call as the other flags give it and the same
call with the penalties / log-probabilities, and the lines of the latter carry ``"form": "pen"``.
``--sample-kernel --penalties R,P,F`` times the ``_sample_logits_pen`` launch alone.

``--ragged --kv-page N [N ...]`` decodes the ragged batch with the paged KV cache
(``generate(..., kv_page=N)``) at every N next to the contiguous per-row cache, in the same
process and interleaved rounds, and then times the decode-attention launch alone (``paged_bench``).

``--weight-dtype fp8`` decodes with fp8 projection weights (``generate(..., weight_dtype="fp8")``);
``both`` runs the bf16 and the fp8 weights in interleaved rounds (``--repeats`` of them, each
session warm; ``w8_bench``) with the median and spread per (batch, mode, weights) and whether the
tokens agree; ``mxfp4`` decodes with MXFP4 weights (``weight_dtype="mxfp4"``) and ``all`` runs bf16, fp8
and MXFP4 in the same rounds.  ``--layers N`` builds the preset with N layers (a large preset inside a short run).
``--w8-kernel`` times the projection launch alone on the preset's QKV, Wo, gate|up, down and
lm_head shapes: ``_gemv_nt_w8`` and ``_gemv_nt_w4`` against ``gemv_nt`` (M <= 16) or the ``gemm_nt``
route (M > 16), 100 launches per graph replay, with weight bytes / time (``w8_kernel_bench``).

``--quantised-prefill`` adds to ``--prefill-chunk`` and ``--continuation`` the sessions on fp8 and MXFP4
codes, with ``quantised_prefill`` off (the prefill on bf16 weights) and on (every projection on codes), in
the same interleaved rounds.  ``--wq-kernel`` times the quantised-weight GEMM launch alone
(``_gemm_nt_w8`` / ``_gemm_nt_w4``, csrc/kernels/gemm_wq.hip) against ``gemm_nt`` on the bf16 weight, on the
preset's projection shapes at every ``--batch`` M (``wq_kernel_bench``).  Where K % 128 == 0 the same rounds
also time the W8A8 route of ``quantised_prefill="a8"``: the per-token quantiser (``_quant_w8_rows`` on the rows;
``_swiglu_quant_w8_rows`` for the down projection), ``_gemm_nt_w8a8`` (csrc/kernels/gemm_w8a8.hip) and both
together; every line carries the rounds' median, min and max.

``--continuation --extend-split 0 auto N ...`` times the extend-attention launch alone, unsplit against the
split form (``_attn_extend_split``) at the rule's and at forced split counts, over short chunks and long
caches on the GPT-2 small and 7B head shapes (``extend_split_bench``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--recompute-new", type=int, default=32, help="tokens for the full-recompute baseline")
    ap.add_argument("--temperature", type=float, default=0.0, help="> 0: sampled decoding")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--sample-kernel", action="store_true", help="time the sample_logits launch alone")
    ap.add_argument("--per-row", action="store_true", help="the settings as per-row lists (device table)")
    ap.add_argument("--seeds", choices=["fixed", "fresh"], default=None,
                    help="one seed for every call, or a new one per call (default: fresh with --per-row, else fixed)")
    ap.add_argument("--ragged", action="store_true", help="ragged batch: lengths spread over [prompt/4, prompt]")
    ap.add_argument("--ragged-equal", action="store_true", help="per-row path with all lengths = prompt")
    ap.add_argument("--prefill-chunk", type=int, nargs="+", default=None, help="time the prefill whole and in pieces")
    ap.add_argument("--continuation", action="store_true", help="time one multi-token continuation")
    ap.add_argument("--t0", type=int, default=1024, help="--continuation: ids in the cache")
    ap.add_argument("--chunk", type=int, default=256, help="--continuation: new ids")
    ap.add_argument("--extend-split", nargs="+", default=None, metavar="S",
                    help="--continuation: time the extend-attention launch alone at these split counts "
                         "(0: unsplit, auto: the selection rule, N: forced)")
    ap.add_argument("--kv-dtype", choices=["act", "fp8", "both"], default="act",
                    help="KV cache storage: activation dtype, fp8 codes, or both in interleaved rounds")
    ap.add_argument("--modes", nargs="+", choices=["graph", "eager"], default=["graph", "eager"])
    ap.add_argument("--penalties", default=None, metavar="R,P,F",
                    help="repetition,presence,frequency: also time the penalised form in the same rounds")
    ap.add_argument("--logprobs", action="store_true", help="the penalised form returns log-probabilities")
    ap.add_argument("--kv-page", type=int, nargs="+", default=None, metavar="N",
                    help="--ragged: the paged KV cache at these page sizes next to the contiguous one")
    ap.add_argument("--weight-dtype", choices=["act", "fp8", "mxfp4", "both", "all"], default="act",
                    help="projection weights of the decode steps: bf16, fp8 codes, MXFP4 codes, bf16 and fp8 (both) "
                         "or all three in interleaved rounds")
    ap.add_argument("--layers", type=int, default=0, help="build the preset with this many layers (0: its own)")
    ap.add_argument("--w8-kernel", action="store_true",
                    help="time the fp8- and MXFP4-weight projection launches alone")
    ap.add_argument("--quantised-prefill", action="store_true",
                    help="--prefill-chunk / --continuation: also on fp8 and MXFP4 codes, quantised_prefill off and on")
    ap.add_argument("--wq-kernel", action="store_true",
                    help="time the quantised-weight GEMM launches (gemm_wq.hip) against gemm_nt at every --batch M")
    a = ap.parse_args()
    if a.kv_page and not (a.ragged or a.extend_split):
        ap.error("--kv-page runs the ragged decode benchmark: give --ragged")
    pen_kw = {}
    if a.penalties:
        r, p_, f = (float(v) for v in a.penalties.split(","))
        pen_kw = dict(repetition_penalty=r, presence_penalty=p_, frequency_penalty=f)
    if a.logprobs:
        pen_kw["return_logprobs"] = True
    forms = [("base", {})] + ([("pen", pen_kw)] if pen_kw else [])
    sampling = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=0)
    fresh = (a.seeds or ("fresh" if a.per_row else "fixed")) == "fresh"
    calls = [0]

    def settings(B):
        """The sampling arguments of the next generate() call at batch B."""
        calls[0] += 1
        n = calls[0] if fresh else 0
        if not a.per_row:
            return dict(sampling, seed=n)
        return dict(temperature=[a.temperature] * B, top_k=[a.top_k] * B, top_p=[a.top_p] * B,
                    seed=[n * B + b for b in range(B)])
    import torch
    from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.models.generation import generate
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29591")
    init_dist_env(rank=0, tp_size=1, world_size=1)
    args = get_preset(a.model, **({"num_layers": a.layers} if a.layers else {}))
    if a.w8_kernel:
        return w8_kernel_bench(a, args)
    if a.wq_kernel:
        return wq_kernel_bench(a, args)
    if a.continuation and a.extend_split:
        return extend_split_bench(a)
    if a.continuation and a.t0 + a.chunk > args.maxlen:     # the RoPE table must cover the continuation
        args = get_preset(a.model, maxlen=a.t0 + a.chunk)
    m = Transformer.from_args(args).cuda()
    m.reset_parameters()
    m.eval()
    if a.sample_kernel:
        return sample_kernel_bench(a, m.lm_head.weight.size(0), args.vocab_size)
    if a.continuation:
        return continuation_bench(a, m)
    if a.prefill_chunk:
        return prefill_bench(a, m)
    if a.kv_page:
        return paged_bench(a, m)
    if a.weight_dtype != "act":
        return w8_bench(a, m)
    for B in a.batch:
        prompt = torch.randint(0, args.vocab_size, (B, a.prompt), device="cuda")
        lens = None
        if a.ragged:
            lo = max(1, a.prompt // 4)
            lens = [lo + b * (a.prompt - lo) // max(1, B - 1) for b in range(B)] if B > 1 else [a.prompt]
        elif a.ragged_equal:
            lens = [a.prompt] * B
        kw = dict(prompt_lens=lens) if lens else {}
        kds = {"act": [None], "fp8": ["fp8"], "both": [None, "fp8"]}[a.kv_dtype]
        for mode in a.modes:
            os.environ["DPFS_DECODE_GRAPH"] = "1" if mode == "graph" else "0"
            for kd in kds:
                for _, fkw in forms:
                    # warm-up: GEMM choices, graph capture (reused by the same-shape call)
                    generate(m, prompt, max_new_tokens=a.new, kv_dtype=kd, **settings(B), **kw, **fkw)
            ms = {kd: [] for kd in kds}
            for _ in range(a.repeats):
                for kd, (form, fkw) in ((kd, f) for kd in kds for f in forms):      # interleaved rounds
                    st = settings(B)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    generate(m, prompt, max_new_tokens=a.new, kv_dtype=kd, **st, **kw, **fkw)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if form == "base":
                        ms[kd].append(round(1000 * dt / a.new, 3))
                    rec = {"model": a.model, "batch": B, "mode": mode, "prompt": a.prompt, "new": a.new,
                           "ms_per_step": round(1000 * dt / a.new, 3), "tokens_per_s": round(B * a.new / dt, 1)}
                    if form == "pen":
                        rec.update(form="pen", penalties=a.penalties, logprobs=a.logprobs)
                    if a.kv_dtype != "act":
                        rec["kv_dtype"] = kd or "act"
                    if lens:
                        rec.update(ragged="spread" if a.ragged else "equal", min_len=min(lens), max_len=max(lens))
                    if a.temperature > 0 or a.per_row:
                        rec.update(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                                   settings="per-row" if a.per_row else "scalar", seeds="fresh" if fresh else "fixed")
                    print(json.dumps(rec), flush=True)
            if a.kv_dtype != "act":
                kept = {k[4]: e["cache"].nbytes() for k, e in G._SESSIONS.items()}
                for kd in kds:
                    print(json.dumps({"bench": "kv_dtype", "model": a.model, "batch": B, "mode": mode, "prompt": a.prompt,
                                      "new": a.new, "kv_dtype": kd or "act", "ms_per_step": ms[kd],
                                      "ms_per_step_median": _median(ms[kd]), "session_cache_bytes": kept.get(kd)}),
                          flush=True)
        if a.ragged and B > 1:
            # the same prompts one after the other at batch 1 (uniform path, graph), each timed
            # right after its own warm-up call, so no capture is in the time
            os.environ["DPFS_DECODE_GRAPH"] = "1"
            for _ in range(a.repeats):
                dt = 0.0
                for b in range(B):
                    row = prompt[b:b + 1, :lens[b]].contiguous()
                    generate(m, row, max_new_tokens=a.new, **sampling)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    generate(m, row, max_new_tokens=a.new, **sampling)
                    torch.cuda.synchronize()
                    dt += time.perf_counter() - t0
                print(json.dumps({"model": a.model, "batch": B, "mode": "one-by-one", "prompt": a.prompt, "new": a.new,
                                  "ragged": "spread", "min_len": min(lens), "max_len": max(lens),
                                  "ms_per_step": round(1000 * dt / (B * a.new), 3),
                                  "tokens_per_s": round(B * a.new / dt, 1)}), flush=True)
        if a.temperature > 0 or a.per_row or lens or pen_kw:
            continue
        # reference formulation: every token re-runs the whole prefix (no cache)
        seq = prompt
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.inference_mode():
            for _ in range(a.recompute_new):
                T = seq.size(1)
                logits = m(seq, torch.arange(T, device="cuda").repeat(B, 1))[:, -1]
                seq = torch.cat([seq, logits.argmax(-1, keepdim=True)], 1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"model": a.model, "batch": B, "mode": "full-recompute", "prompt": a.prompt,
                          "new": a.recompute_new, "ms_per_step": round(1000 * dt / a.recompute_new, 3),
                          "tokens_per_s": round(B * a.recompute_new / dt, 1)}), flush=True)


def _new_cache(m, B, t_max):
    import torch
    from distributed_pytorch_from_scratch_amd.models.generation import KVCache
    attn = m.layers[0].attn
    return KVCache(len(m.layers), B, t_max, attn.num_local_heads, attn.head_dim, torch.bfloat16, torch.device("cuda"))


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def paged_bench(a, m):
    """``--ragged --kv-page N [N ...]``: the ragged batch of ``main`` decoded with the contiguous
    per-row cache (page 0) and with the paged cache at every N, in one process and interleaved
    rounds (``--repeats`` of them, every session warm; ``--kv-dtype`` chooses the storage).  The
    paged sessions get the pages the batch needs (``kv_pool_pages`` = the sum over the rows of
    ceil((len + new) / N)), so ``cache_bytes`` shows what paging saves against the slab.  One line
    per (batch, mode, page) with the rounds, their median and spread; then the decode-attention
    launch alone (``attn_decode`` per-row against ``_attn_decode_paged``) at T_max 1024, 200
    launches per graph replay."""
    import torch
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.ops import _ext
    kd = None if a.kv_dtype == "act" else "fp8"
    pages = [0] + list(a.kv_page)
    for B in a.batch:
        prompt = torch.randint(0, m.args.vocab_size, (B, a.prompt), device="cuda")
        lo = max(1, a.prompt // 4)
        lens = [lo + b * (a.prompt - lo) // max(1, B - 1) for b in range(B)] if B > 1 else [a.prompt]
        need = {p: sum(-(-(n + a.new) // p) for n in lens) for p in pages if p}
        kws = {p: dict(kv_page=p, kv_pool_pages=need[p]) if p else {} for p in pages}
        for mode in a.modes:
            os.environ["DPFS_DECODE_GRAPH"] = "1" if mode == "graph" else "0"
            run = lambda p: G.generate(m, prompt, max_new_tokens=a.new, prompt_lens=lens, kv_dtype=kd, **kws[p])
            toks = {p: run(p) for p in pages}                       # warm-up: GEMM choices, graph capture
            ms = {p: [] for p in pages}
            for _ in range(a.repeats):
                for p in pages:                                     # interleaved rounds
                    ms[p].append(round(_timed(lambda: run(p)) / a.new, 4))
            kept = {(k[6] if len(k) > 6 else 0): e["cache"].nbytes() for k, e in G._SESSIONS.items()}
            for p in pages:
                print(json.dumps({"bench": "kv_page", "model": a.model, "batch": B, "mode": mode, "prompt": a.prompt,
                                  "new": a.new, "min_len": min(lens), "max_len": max(lens), "kv_dtype": kd or "act",
                                  "kv_page": p, "kv_pool_pages": need.get(p), "ms_per_step": ms[p],
                                  "ms_per_step_median": _median(ms[p]), "ms_per_step_spread": round(max(ms[p]) - min(ms[p]), 4),
                                  "tokens_per_s_median": round(B / _median(ms[p]) * 1000, 1),
                                  "cache_bytes": kept.get(p), "same_tokens_as_contiguous": toks[p] == toks[0]}),
                      flush=True)
        G.clear_sessions()
    # the decode-attention launch alone
    C = _ext.require()
    attn = m.layers[0].attn
    H, hd, t_max = attn.num_local_heads, attn.head_dim, 1024
    for B in a.batch:
        kc, vc = (torch.randn(B, t_max, H, hd, device="cuda").bfloat16() for _ in range(2))
        q = torch.randn(B, 3 * H * hd, device="cuda").bfloat16()
        lens = torch.tensor([t_max // 4 + b * (3 * t_max // 4 - 1) // max(1, B - 1) for b in range(B)], dtype=torch.int32,
                            device="cuda")
        launch = {0: lambda: C.attn_decode(q, kc, vc, lens, hd ** -0.5)}
        for p in a.kv_page:
            MP = t_max // p
            tbl = torch.randperm(B * MP, device="cuda").int().view(B, MP)
            kp, vp = (torch.empty(B * MP, p, H, hd, dtype=torch.bfloat16, device="cuda") for _ in range(2))
            for pool, c in ((kp, kc), (vp, vc)):
                pool[tbl.long().flatten()] = c.view(B * MP, p, H, hd)
            launch[p] = (lambda kp=kp, vp=vp, tbl=tbl, p=p:
                         C._attn_decode_paged(q, kp, vp, None, None, tbl, lens, t_max, p, hd ** -0.5))
            assert torch.equal(launch[p](), launch[0]())
        graphs = {}
        for p, fn in launch.items():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(s)
            graphs[p] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[p]):
                for _ in range(200):
                    fn()
            graphs[p].replay()
        us = {p: [] for p in launch}
        for _ in range(max(a.repeats, 5)):
            for p, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                us[p].append(round(5 * e0.elapsed_time(e1), 2))
        for p in launch:
            print(json.dumps({"bench": "kv_page_attn", "kernel": "_attn_decode_paged" if p else "attn_decode", "batch": B,
                              "heads": H, "head_dim": hd, "t_max": t_max, "kv_page": p, "us_per_call": us[p],
                              "us_per_call_median": _median(us[p]),
                              "us_per_call_spread": round(max(us[p]) - min(us[p]), 2)}), flush=True)


def w8_bench(a, m):
    """``--weight-dtype``: the greedy decode of ``main`` with bf16, fp8 and / or MXFP4 projection weights
    in one process and interleaved rounds (every session warm); one line per (batch, mode, weights)."""
    import torch
    from distributed_pytorch_from_scratch_amd.models import generation as G
    wds = {"fp8": ["fp8"], "mxfp4": ["mxfp4"], "both": [None, "fp8"], "all": [None, "fp8", "mxfp4"]}[a.weight_dtype]
    kd = None if a.kv_dtype == "act" else "fp8"
    for B in a.batch:
        prompt = torch.randint(0, m.args.vocab_size, (B, a.prompt), device="cuda")
        for mode in a.modes:
            os.environ["DPFS_DECODE_GRAPH"] = "1" if mode == "graph" else "0"
            run = lambda wd: G.generate(m, prompt, max_new_tokens=a.new, kv_dtype=kd, weight_dtype=wd)
            toks = {wd: run(wd) for wd in wds}                      # warm-up: GEMM choices, graph capture
            ms = {wd: [] for wd in wds}
            for _ in range(a.repeats):
                for wd in wds:                                      # interleaved rounds
                    ms[wd].append(round(_timed(lambda: run(wd)) / a.new, 4))
            # generated ids equal to the bf16 weights' (quantisation may change an argmax)
            agree = {wd: sum(x == y for r, q in zip(toks[None], toks[wd]) for x, y in zip(r, q)) / (B * len(toks[None][0]))
                     for wd in wds if wd and None in toks}
            for wd in wds:
                print(json.dumps({"bench": "weight_dtype", "model": a.model, "layers": len(m.layers), "batch": B,
                                  "mode": mode, "prompt": a.prompt, "new": a.new, "kv_dtype": kd or "act",
                                  "weight_dtype": wd or "act", "ms_per_step": ms[wd],
                                  "ms_per_step_median": _median(ms[wd]),
                                  "ms_per_step_spread": round(max(ms[wd]) - min(ms[wd]), 4),
                                  "tokens_per_s_median": round(B / _median(ms[wd]) * 1000, 1),
                                  "token_agreement_with_act": agree.get(wd)}), flush=True)
        G.clear_sessions()


PEAK_HBM_TBS = 8.0     # MI355X HBM3E peak, TB/s: the floor of a launch is its weight bytes at this rate


def w8_kernel_bench(a, args):
    """``--w8-kernel``: us per projection launch on the preset's shapes at every ``--batch`` M."""
    import torch
    from distributed_pytorch_from_scratch_amd.ops import _ext
    from distributed_pytorch_from_scratch_amd.ops import gemm_select as GS
    C = _ext.require()
    d, f, v = args.attn_dim, args.ffn_dim, (args.vocab_size + 127) // 128 * 128
    shapes = [("qkv", 3 * d, d, False), ("wo", d, d, False), ("gate_up", 2 * f, d, False), ("down", d, f, True),
              ("lm_head", v, d, False)]
    for name, N, K, sw in shapes:
        # the 100 launches of a replay walk over copies of the weight that together exceed the 256 MB
        # infinity cache (600 MB of codes), so every launch streams its weight from HBM as a decode
        # step of a model larger than the cache does
        nc = min(100, -(-600 * 2 ** 20 // (N * K)))
        ws = [(torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16() for _ in range(nc)]
        qs = [C._quant_w8_rows(w) for w in ws]
        q4 = [C._quant_w4_rows(w) for w in ws] if K % 128 == 0 else None
        for M in a.batch:
            x = torch.randn(M, 2 * K if sw else K, device="cuda").bfloat16()
            ref = "gemv_nt" if M <= 16 else "gemm_nt"
            launch = {"w8": lambda i: C._gemv_nt_w8(x, qs[i % nc][0], qs[i % nc][1], None, sw),
                      ref: (lambda i: C.gemv_nt(x, ws[i % nc], None, sw)) if M <= 16 else
                           (lambda i: GS.gemm_nt(C, C.swiglu_fwd(x) if sw else x, ws[i % nc]))}
            if q4:
                launch["w4"] = lambda i: C._gemv_nt_w4(x, q4[i % nc][0], q4[i % nc][1], None, sw)
            graphs = {}
            for k_, fn in launch.items():
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for i in range(3):
                        fn(i)
                torch.cuda.current_stream().wait_stream(s)
                graphs[k_] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k_]):
                    for i in range(100):
                        fn(i)
                graphs[k_].replay()
            us = {k_: [] for k_ in launch}
            for _ in range(max(a.repeats, 5)):
                for k_, g in graphs.items():                        # interleaved rounds
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    us[k_].append(round(10 * e0.elapsed_time(e1), 2))
            for k_ in launch:
                wbytes = {"w8": N * K + 4 * N, "w4": N * K // 2 + N * K // 32}.get(k_, 2 * N * K)
                med = _median(us[k_])
                floor = wbytes / (PEAK_HBM_TBS * 1e6)
                print(json.dumps({"bench": "w8_kernel", "model": a.model, "proj": name, "M": M, "N": N, "K": K,
                                  "kernel": k_, "weight_copies": nc, "us_per_call": us[k_], "us_per_call_median": med,
                                  "us_per_call_spread": round(max(us[k_]) - min(us[k_]), 2), "weight_bytes": wbytes,
                                  "weight_TBps": round(wbytes / med / 1e6, 3), "floor_us_at_peak": round(floor, 2),
                                  "share_of_peak": round(floor / med, 3)}), flush=True)


def wq_kernel_bench(a, args):
    """``--wq-kernel``: us per launch of ``_gemm_nt_w8`` / ``_gemm_nt_w4``, of the W8A8 route (``a8_quant``: the
    per-token quantiser, ``a8_gemm``: ``_gemm_nt_w8a8``, ``a8``: both) and of ``gemm_nt`` on the bf16 weight, on the preset's projection shapes at every ``--batch`` M, 20 launches per timed window, in
    interleaved rounds; one JSON line per (projection, M, kernel)."""
    import torch
    from distributed_pytorch_from_scratch_amd.ops import _ext
    C = _ext.require()
    d, f, v = args.attn_dim, args.ffn_dim, (args.vocab_size + 127) // 128 * 128
    for name, N, K in (("qkv", 3 * d, d), ("wo", d, d), ("gate_up", 2 * f, d), ("down", d, f), ("lm_head", v, d)):
        w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
        q8, q4 = C._quant_w8_rows(w), C._quant_w4_rows(w) if K % 128 == 0 else None
        for M in a.batch:
            x = torch.randn(M, K, device="cuda").bfloat16()
            launch = {"gemm_nt": lambda: C.gemm_nt(x, w), "w8": lambda: C._gemm_nt_w8(x, *q8)}
            if q4:
                launch["w4"] = lambda: C._gemm_nt_w4(x, *q4)
            if K % 128 == 0:      # W8A8: the per-token quantiser (the fused SwiGLU one for down), the fp8 MFMA GEMM, both
                src = torch.randn(M, 2 * K, device="cuda").bfloat16() if name == "down" else x
                quant = C._swiglu_quant_w8_rows if name == "down" else C._quant_w8_rows
                xc, sa = quant(src)
                launch["a8_quant"] = lambda: quant(src)
                launch["a8_gemm"] = lambda: C._gemm_nt_w8a8(xc, sa, *q8)
                launch["a8"] = lambda: C._gemm_nt_w8a8(*quant(src), *q8)
            us = {k_: [] for k_ in launch}
            for fn in launch.values():
                fn()
            for _ in range(max(a.repeats, 5)):
                for k_, fn in launch.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us[k_].append(round(50 * e0.elapsed_time(e1), 2))
            for k_ in launch:
                med = _median(us[k_])
                print(json.dumps({"bench": "wq_kernel", "model": a.model, "proj": name, "M": M, "N": N, "K": K,
                                  "kernel": k_, "us_per_call": us[k_], "us_per_call_median": med,
                                  "us_per_call_min": min(us[k_]), "us_per_call_max": max(us[k_]),
                                  "tflops": round(2e-6 * M * N * K / med, 1),
                                  "vs_gemm_nt": round(med / _median(us["gemm_nt"]), 3)}), flush=True)


def _weight_forms(a, m):
    """(label, cache attributes) of the sessions a prefill / continuation case times: bf16 weights, and with
    ``--quantised-prefill`` the fp8 and MXFP4 codes with the option off (prefill on bf16 weights) and on."""
    from distributed_pytorch_from_scratch_amd.models.generation import quantise_weights
    forms = [("act", {})]
    if a.quantised_prefill:
        for wd, attr in (("fp8", "w8"), ("mxfp4", "w4")):
            codes = quantise_weights(m, "cuda", wd)
            forms += [(f"{wd} off", {attr: codes}), (f"{wd} on", {attr: codes, "wq_prefill": True})]
    return forms


def prefill_bench(a, m):
    """Time to first token (ms) and peak bytes above the cache of the prefill of ``--prompt`` ids,
    whole (chunk 0) and in pieces, in interleaved rounds; one JSON line per (batch, chunk, weight form)."""
    import torch
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    forms = _weight_forms(a, m)
    chunks = [(c, f) for c in [0] + [c for c in a.prefill_chunk if c > 0] for f in range(len(forms))]
    for B in a.batch:
        prompt = torch.randint(0, m.args.vocab_size, (B, a.prompt), device="cuda")
        caches = [_new_cache(m, B, a.prompt) for _ in forms]
        for cache, (_, attrs) in zip(caches, forms):
            for k_, v_ in attrs.items():
                setattr(cache, k_, v_)
        ms = {c: [] for c in chunks}
        peak = {}

        def run(c):
            caches[c[1]].reset()
            return logits_step(m, prompt, caches[c[1]], prefill_chunk=c[0]).argmax(-1)

        for c in chunks:                                    # warm-up: GEMM choices per piece shape
            run(c)
        for _ in range(a.repeats):
            for c in chunks:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ms[c].append(_timed(lambda: run(c)))
                peak[c] = torch.cuda.max_memory_allocated() - base
        for c in chunks:
            print(json.dumps({"bench": "prefill", "model": a.model, "batch": B, "prompt": a.prompt, "prefill_chunk": c[0],
                              "weights": forms[c[1]][0], "ttft_ms": [round(x, 3) for x in ms[c]], "ttft_ms_median": round(_median(ms[c]), 3),
                              "peak_bytes_above_cache": peak[c]}), flush=True)


def continuation_bench(a, m):
    """One ``--chunk``-token continuation at cache length ``--t0``: the kernel path against the
    framework formulation it replaced, in interleaved rounds; one JSON line per batch."""
    import math
    import torch
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.ops.dispatch import K

    kernel_step = G._attention_step

    def einsum_step(layer, x2d, positions, tab, cache, li, B, T, n_t=None):
        """The continuation as it ran before the kernels: host offset, fp32 copies of the whole
        cache, a materialised (B, H, T, S) score tensor."""
        attn = layer.attn
        h, hd = attn.num_local_heads, attn.head_dim
        qkv = attn.wqkv(x2d)
        K(qkv).rope_(qkv, positions, tab, 2 * h, hd, False)
        q = qkv[:, : h * hd].view(B, T, h, hd)
        t0 = cache.len
        cache.k[li][:, t0:t0 + T] = qkv[:, h * hd: 2 * h * hd].view(B, T, h, hd)
        cache.v[li][:, t0:t0 + T] = qkv[:, 2 * h * hd:].view(B, T, h, hd)
        keys = cache.k[li][:, : t0 + T].float()
        vals = cache.v[li][:, : t0 + T].float()
        s = torch.einsum("bthd,bshd->bhts", q.float(), keys) * (1.0 / math.sqrt(hd))
        S = t0 + T
        mask = torch.ones(T, S, dtype=torch.bool, device=s.device).triu(S - T + 1)
        p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
        o = torch.einsum("bhts,bshd->bthd", p, vals).to(q.dtype)
        return attn.wo(o.reshape(B * T, h * hd))

    for B in a.batch:
        ids = torch.randint(0, m.args.vocab_size, (B, a.t0 + a.chunk), device="cuda")
        cache = _new_cache(m, B, a.t0 + a.chunk)
        G.logits_step(m, ids[:, : a.t0].contiguous(), cache)
        new = ids[:, a.t0:].contiguous()
        out = {}

        codes = dict(_weight_forms(a, m))                   # --quantised-prefill: "fp8 on", "mxfp4 on" modes

        def run(mode):
            cache.len = a.t0                                # the same continuation again
            G._attention_step = einsum_step if mode == "einsum" else kernel_step
            for k_, v_ in codes.get(mode, {}).items():
                setattr(cache, k_, v_)
            try:
                out[mode] = G.logits_step(m, new, cache)
            finally:
                G._attention_step = kernel_step
                cache.w8 = cache.w4 = None
                cache.wq_prefill = False

        ms = {mode: [] for mode in ["kernel", "einsum"] + [k_ for k_ in codes if k_.endswith(" on")]}
        for mode in ms:
            run(mode)                                       # warm-up
        rel = ((out["kernel"] - out["einsum"]).norm() / out["einsum"].norm()).item()
        for _ in range(a.repeats):
            for mode in ms:
                ms[mode].append(_timed(lambda: run(mode)))
        print(json.dumps({"bench": "continuation", "model": a.model, "batch": B, "t0": a.t0, "chunk": a.chunk,
                          "kernel_ms": [round(x, 3) for x in ms["kernel"]],
                          "einsum_ms": [round(x, 3) for x in ms["einsum"]],
                          **{k_.replace(" on", "_codes_ms_median"): round(_median(v_), 3) for k_, v_ in ms.items()
                             if k_.endswith(" on")},
                          "kernel_ms_median": round(_median(ms["kernel"]), 3),
                          "einsum_ms_median": round(_median(ms["einsum"]), 3),
                          "kernel_not_slower_in_any_round": all(k <= e for k, e in zip(ms["kernel"], ms["einsum"])),
                          "logits_rel_diff": rel}), flush=True)


# --continuation --extend-split: (name, local heads, head_dim), chunk lengths and cache lengths of the sweep
EXT_SPLIT_SHAPES = (("gpt2-small", 12, 64), ("7b-heads", 32, 128))
EXT_SPLIT_CHUNKS = (8, 32, 256)
EXT_SPLIT_T0 = (4096, 16384, 32768)


def extend_split_bench(a):
    """``--continuation --extend-split 0 auto N ...``: the extend-attention launch alone, a ``chunk``-token
    step over a cache that holds ``t0`` keys (capacity t0 + 256), on the head shapes of ``EXT_SPLIT_SHAPES``
    at every ``--batch``, for the bf16 and the fp8 cache and the bf16 paged cache (``--kv-page``, first
    value, default 64).  Every mode is a split count: ``0`` is the unsplit kernel (``_attn_extend`` and kin,
    the yardstick), ``auto`` what ``generation._extend_splits`` picks, N that many splits.  One process,
    ``--repeats`` interleaved rounds, us per launch from device events over a window of launches; one JSON
    line per case with every mode's rounds, median and spread (max - min), and ``auto_ok``: auto's median is
    not above the unsplit median by more than the unsplit rounds' spread."""
    import torch
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.ops import _ext
    C = _ext.require()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    page = (a.kv_page or [64])[0]
    f8 = torch.float8_e4m3fn

    def splits_of(mode, T, B, h, t_max):
        os.environ["DPFS_EXTEND_SPLIT"] = mode
        try:
            return G._extend_splits(T, B, h, t_max, cus)
        finally:
            del os.environ["DPFS_EXTEND_SPLIT"]

    for name, h, hd in EXT_SPLIT_SHAPES:
        for B in a.batch:
            for t0 in EXT_SPLIT_T0:
                t_max = t0 + 256
                kc = torch.randn(B, t_max, h, hd, device="cuda", dtype=torch.bfloat16)
                vc = torch.randn(B, t_max, h, hd, device="cuda", dtype=torch.bfloat16)
                k8 = torch.randint(0, 0x78, (B, t_max, h, hd), device="cuda", dtype=torch.uint8).view(f8)
                v8 = torch.randint(0, 0x78, (B, t_max, h, hd), device="cuda", dtype=torch.uint8).view(f8)
                ks = torch.rand(B, t_max, h, device="cuda") * 0.01 + 0.001
                vs = torch.rand(B, t_max, h, device="cuda") * 0.01 + 0.001
                ln = torch.full((B,), t0, dtype=torch.int32, device="cuda")
                mp = -(-t_max // page)
                tbl = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp)
                pools = [torch.randn(B * mp, page, h, hd, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
                for T in EXT_SPLIT_CHUNKS:
                    q = torch.randn(B * T, 3 * h * hd, device="cuda", dtype=torch.bfloat16)[:, : h * hd]
                    scale = hd ** -0.5
                    forms = {
                        "bf16": lambda S: (C._attn_extend(q, kc, vc, ln, None, scale) if S == 1 else
                                           C._attn_extend_split(q, kc, vc, None, None, ln, None, scale, S)),
                        "fp8": lambda S: (C._attn_extend_q8(q, k8, v8, ks, vs, ln, None, scale) if S == 1 else
                                          C._attn_extend_split(q, k8, v8, ks, vs, ln, None, scale, S)),
                        f"paged{page}": lambda S: (
                            C._attn_extend_paged(q, *pools, None, None, tbl, ln, None, t_max, page, scale) if S == 1 else
                            C._attn_extend_split_paged(q, *pools, None, None, tbl, ln, None, t_max, page, scale, S)),
                    }
                    modes = {mode: splits_of(mode, T, B, h, t_max) for mode in a.extend_split}
                    for form, launch in forms.items():
                        launch(1)
                        torch.cuda.synchronize()
                        one = _timed(lambda: launch(1))                      # ms: sizes the window (>= 2 ms, 5..200 launches)
                        iters = max(5, min(200, int(2.0 / max(one, 0.01))))
                        us = {mode: [] for mode in modes}
                        for mode, S in modes.items():
                            launch(S)                                        # warm-up
                        for _ in range(a.repeats):
                            for mode, S in modes.items():
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _i in range(iters):
                                    launch(S)
                                e1.record()
                                torch.cuda.synchronize()
                                us[mode].append(1000 * e0.elapsed_time(e1) / iters)
                        line = {"bench": "extend_split", "shape": name, "heads": h, "head_dim": hd, "batch": B, "t0": t0,
                                "chunk": T, "cache": form, "cus": cus, "fill": G._EXT_FILL,
                                "min_tiles": G._EXT_MIN_TILES, "launches_per_round": iters}
                        for mode, S in modes.items():
                            line[mode] = {"splits": S, "us": [round(x, 2) for x in us[mode]],
                                          "median": round(_median(us[mode]), 2),
                                          "spread": round(max(us[mode]) - min(us[mode]), 2)}
                        if "0" in modes and "auto" in modes and modes["auto"] > 1:
                            line["auto_ok"] = line["auto"]["median"] <= line["0"]["median"] + line["0"]["spread"]
                        print(json.dumps(line), flush=True)
                del kc, vc, k8, v8, ks, vs, pools


def sample_kernel_bench(a, ld: int, vocab: int):
    """us per ``sample_logits`` launch (``--per-row``: ``_sample_logits_rows`` with the same
    settings in every row of its table; ``--penalties``: ``_sample_logits_pen`` with them, on a
    history of 128 prompt flags per row that the 200 launches count into) on (B, ld) bf16 rows:
    device events over 200 launches."""
    import torch
    from distributed_pytorch_from_scratch_amd.ops import _ext
    C = _ext.require()
    T = a.temperature if a.temperature > 0 else 1.0
    for B in a.batch:
        x = (torch.randn(B, ld, device="cuda") * 4).bfloat16()
        pos = torch.zeros(B, dtype=torch.int64, device="cuda")
        if a.per_row or a.penalties:
            tab = (torch.full((B,), 1.0 / T, dtype=torch.float64).float().cuda(),
                   torch.full((B,), a.top_k, dtype=torch.int32, device="cuda"),
                   torch.full((B,), a.top_p, dtype=torch.float64, device="cuda"),
                   torch.zeros(B, dtype=torch.int64, device="cuda"), torch.arange(B, dtype=torch.int32, device="cuda"))
            launch = lambda: C._sample_logits_rows(x, vocab, *tab, pos)
            if a.penalties:
                r, p_, f = (float(v) for v in a.penalties.split(","))
                pens = [torch.full((B,), v, dtype=torch.float64).float().cuda() for v in (r, 1.0 / r, p_, f)]
                hist = torch.zeros(B, (vocab + 7) // 8 * 8, dtype=torch.int32, device="cuda")
                hist.scatter_(1, torch.randint(0, vocab, (B, 128), device="cuda"), -2 ** 31)
                launch = lambda: C._sample_logits_pen(x, vocab, *tab, *pens, hist, pos)
        else:
            launch = lambda: C.sample_logits(x, vocab, T, a.top_k, a.top_p, 0, pos)
        # 200 launches in one graph: the replay is not paced by the host's launch rate
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                launch()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(200):
                launch()
        g.replay()
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            name = "sample_logits_pen" if a.penalties else "sample_logits_rows" if a.per_row else "sample_logits"
            print(json.dumps({"kernel": name, "batch": B,
                              "vocab": vocab, "ld": ld, "temperature": T, "top_k": a.top_k, "top_p": a.top_p,
                              "us_per_call": round(5 * e0.elapsed_time(e1), 2)}),
                  flush=True)


if __name__ == "__main__":
    main()
