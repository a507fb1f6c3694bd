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
    ap.add_argument("--kv-dtype", choices=["act", "fp8", "both"], default="act",
                    help="KV cache storage: activation dtype, fp8 codes, or both in interleaved rounds")
    ap.add_argument("--modes", nargs="+", choices=["graph", "eager"], default=["graph", "eager"])
    ap.add_argument("--penalties", default=None, metavar="R,P,F",
                    help="repetition,presence,frequency: also time the penalised form in the same rounds")
    ap.add_argument("--logprobs", action="store_true", help="the penalised form returns log-probabilities")
    ap.add_argument("--kv-page", type=int, nargs="+", default=None, metavar="N",
                    help="--ragged: the paged KV cache at these page sizes next to the contiguous one")
    a = ap.parse_args()
    if a.kv_page and not a.ragged:
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
    args = get_preset(a.model)
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


def prefill_bench(a, m):
    """Time to first token (ms) and peak bytes above the cache of the prefill of ``--prompt`` ids,
    whole (chunk 0) and in pieces, in interleaved rounds; one JSON line per (batch, chunk)."""
    import torch
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    chunks = [0] + [c for c in a.prefill_chunk if c > 0]
    for B in a.batch:
        prompt = torch.randint(0, m.args.vocab_size, (B, a.prompt), device="cuda")
        cache = _new_cache(m, B, a.prompt)
        ms = {c: [] for c in chunks}
        peak = {}

        def run(c):
            cache.reset()
            return logits_step(m, prompt, cache, prefill_chunk=c).argmax(-1)

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
            print(json.dumps({"bench": "prefill", "model": a.model, "batch": B, "prompt": a.prompt, "prefill_chunk": c,
                              "ttft_ms": [round(x, 3) for x in ms[c]], "ttft_ms_median": round(_median(ms[c]), 3),
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

        def run(mode):
            cache.len = a.t0                                # the same continuation again
            G._attention_step = kernel_step if mode == "kernel" else einsum_step
            try:
                out[mode] = G.logits_step(m, new, cache)
            finally:
                G._attention_step = kernel_step

        ms = {"kernel": [], "einsum": []}
        for mode in ms:
            run(mode)                                       # warm-up
        rel = ((out["kernel"] - out["einsum"]).norm() / out["einsum"].norm()).item()
        for _ in range(a.repeats):
            for mode in ms:
                ms[mode].append(_timed(lambda: run(mode)))
        print(json.dumps({"bench": "continuation", "model": a.model, "batch": B, "t0": a.t0, "chunk": a.chunk,
                          "kernel_ms": [round(x, 3) for x in ms["kernel"]],
                          "einsum_ms": [round(x, 3) for x in ms["einsum"]],
                          "kernel_ms_median": round(_median(ms["kernel"]), 3),
                          "einsum_ms_median": round(_median(ms["einsum"]), 3),
                          "kernel_not_slower_in_any_round": all(k <= e for k, e in zip(ms["kernel"], ms["einsum"])),
                          "logits_rel_diff": rel}), flush=True)


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
