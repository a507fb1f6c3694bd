"""The decode path at TP 2 and 4 on the MI355X: the HIP kernels at the local shapes of a tensor-parallel
rank (one local head, K 64 Wo shards, ragged lm_head shards: tests/numerics_tp.py) with the two all-reduces
per layer and the logits gather between them, for every cache and weight format of ``generate``.

Several ranks share the one GPU over gloo, as in tests/test_multiproc_gpu.py (RCCL refuses two ranks on
one device).  Every rank builds the bf16 GPU model and an fp32 CPU twin on the GPU model's bf16-rounded
shards; both issue the same collectives in the same order, so they share the group.  Per entry of the
feature matrix the GPU logits are compared with the twin's, teacher-forced on the GPU's argmax: the prefill
and 6 single-token steps (cache rows 12 .. 17: across the page seam at row 16), the bound being that of the
same comparison at TP 1, ``rel <= 3e-2`` (tests/test_gemv_w4_gpu.py).  The same worker runs at world 1 and
the values are printed side by side: what TP adds per rank is the bf16 rounding of the partial Wo / down
outputs in front of the all-reduce.  The ranks must agree to the bit on the gathered logits and on what
``generate`` returns, and a spy on ``gemm_select.small_nt*`` pins which projections ran on codes."""
import pytest
import torch

import numerics as N
import numerics_tp as TP

from dist_helpers import run_distributed

pytestmark = pytest.mark.gpu

STEPS = 6
T_MAX = 24          # two pages of 16: the prompt's 12 rows and the 6 steps end in the second
BOUND = 3e-2
ROUTE = {"fp8": "w8", "mxfp4": "w4"}


def _caches(G, gm, cm, kw):
    """A KV cache of ``T_MAX`` rows in the entry's form for the GPU model and one for the CPU twin, with the
    entry's weight codes attached; and whether the two sets of codes are byte-equal per parameter."""
    wd = kw.get("weight_dtype")
    same, out = True, []
    for m in (gm, cm):
        a, dev = m.layers[0].attn, m.lm_head.weight.device
        if kw.get("kv_page"):
            c = G.PagedKVCache(TP.LAYERS, TP.B, T_MAX, a.num_local_heads, a.head_dim, m.act_dtype(dev), dev,
                               kw["kv_page"], None, kw.get("kv_dtype"))
        else:
            c = G.KVCache(TP.LAYERS, TP.B, T_MAX, a.num_local_heads, a.head_dim, m.act_dtype(dev), dev,
                          ragged="prompt_lens" in kw, kv_dtype=kw.get("kv_dtype"))
        if wd:
            setattr(c, ROUTE[wd], G.quantise_weights(m, dev, wd))
        out.append(c)
    if wd:
        qg, qc = (getattr(c, ROUTE[wd]) for c in out)
        assert TP.coded_names(gm, qg) == TP.coded_names(cm, qc) == TP.coded(gm, wd)
        same = all(torch.equal(a[j].cpu(), b[j]) for a, b in zip(qg.values(), qc.values()) for j in (0, 1))
    return out[0], out[1], same


def _spy(GS, calls):
    """Wrap ``small_nt``, ``small_nt_w8`` and ``small_nt_w4``: every call is recorded as (route, data pointer
    of the weight or of its codes, whether a tensor came back)."""
    saved = {}
    for route, attr in (("bf16", "small_nt"), ("w8", "small_nt_w8"), ("w4", "small_nt_w4")):
        fn = saved[attr] = getattr(GS, attr)

        def wrapped(k, x, w, bias=None, swiglu=False, fn=fn, route=route):
            y = fn(k, x, w, bias, swiglu)
            calls.append((route, (w if route == "bf16" else w[0]).data_ptr(), y is not None))
            return y
        setattr(GS, attr, wrapped)
    return saved


def _routes(gm, cache, wd, calls):
    """The recorded calls as (route, projection name, returned a tensor), by the weights' data pointers."""
    from distributed_pytorch_from_scratch_amd.ops.dispatch import shadow
    dt = gm.act_dtype(gm.lm_head.weight.device)
    names = {shadow(w, dt).data_ptr(): name for name, w in TP.projections(gm)}
    if wd:
        codes = getattr(cache, ROUTE[wd])
        names.update({codes[id(w)][0].data_ptr(): name for name, w in TP.projections(gm) if id(w) in codes})
    return [(route, names.get(ptr), ok) for route, ptr, ok in calls]


def _serve(rank, world, heads, entries, transport=None):
    import os
    if transport:
        os.environ["DPFS_TP_COMM"] = transport
    torch.cuda.set_device(0)
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.ops import gemm_select as GS
    from distributed_pytorch_from_scratch_amd.parallel import tp_comm
    gm, cm, p = TP.tp_model(heads).cuda(), TP.tp_model(heads), TP.prompt()
    cm.load_state_dict({k: v.detach().bfloat16().float().cpu() for k, v in gm.state_dict().items()})
    out = {}
    for name, kw in TP.MATRIX:
        if name not in entries:
            continue
        wd, lens = kw.get("weight_dtype"), kw.get("prompt_lens")
        cg, cc, same = _caches(G, gm, cm, kw)
        lg, lc = G.logits_step(gm, p.cuda(), cg, lens), G.logits_step(cm, p, cc, lens)
        rels, logits, calls, routes = [N.rel(lg.cpu(), lc)], [lg.cpu()], [], None
        for s in range(STEPS):
            nxt = lg.argmax(-1, keepdim=True)                   # both sides are fed the GPU's id
            saved = _spy(GS, calls) if s == 0 else {}
            try:
                lg = G.logits_step(gm, nxt, cg)
            finally:
                for attr, fn in saved.items():
                    setattr(GS, attr, fn)
            lc = G.logits_step(cm, nxt.cpu(), cc)
            if s == 0:
                routes = _routes(gm, cg, wd, calls)
            rels.append(N.rel(lg.cpu(), lc))
            logits.append(lg.cpu())
        assert cg.len == cc.len == TP.T + STEPS
        want = TP.coded(gm, wd) if wd else []
        out[name] = {"rel": rels, "logits": torch.stack(logits), "same_codes": same, "routes": routes,
                     "want_routes": [(ROUTE[wd] if n in want else "bf16", n, True)
                                     for n in [x for x, _ in TP.projections(gm)][1:] + ["lm_head"]],
                     # the eager multi-step loop of a node (no graph at TP > 1)
                     "gen": G.generate(gm, p.cuda(), TP.NEW, **kw) if world > 1 else None}
    torch.cuda.synchronize()
    tp_comm.check()
    out["decision"] = tp_comm.decision()
    return out


ALL = tuple(name for name, _ in TP.MATRIX)


@pytest.fixture(scope="module")
def single():
    return {heads: run_distributed(_serve, 1, heads, ALL, timeout=120)[0]
            for heads in sorted({h for _, h in TP.WORLD_HEADS})}


@pytest.fixture(scope="module", params=TP.WORLD_HEADS, ids=lambda wh: f"tp{wh[0]}-heads{wh[1]}")
def ranks(request):
    world, heads = request.param
    return world, heads, run_distributed(_serve, world, heads, ALL, timeout=120)


def _check_logits(res, world, ref, what):
    for name in [n for n in ALL if n in res[0]]:
        worst = max(max(res[r][name]["rel"][1:]) for r in range(world))
        print(f"{what} {name}: rel(GPU logits, CPU oracle) prefill {res[0][name]['rel'][0]:.3g}, steps TP {world} "
              f"{['%.3g' % v for v in res[0][name]['rel'][1:]]}, TP 1 {['%.3g' % v for v in ref[name]['rel'][1:]]}; "
              f"worst TP {world} {worst:.3g}, TP 1 {max(ref[name]['rel'][1:]):.3g}")
    for name in [n for n in ALL if n in res[0]]:
        for r in range(world):
            assert res[r][name]["same_codes"], (name, r)
            assert max(res[r][name]["rel"][1:]) <= BOUND, (name, r, res[r][name]["rel"])
            assert torch.isfinite(res[r][name]["logits"]).all()
            # one all-gather of the same shards: the same bits on every rank, at the prefill and every step
            assert torch.equal(res[r][name]["logits"], res[0][name]["logits"]), (name, r)
        assert max(ref[name]["rel"][1:]) <= BOUND, (name, "TP 1", ref[name]["rel"])


def test_logits_follow_the_oracle_and_are_the_same_bits_on_every_rank(ranks, single):
    world, heads, res = ranks
    assert sorted(res) == list(range(world))
    _check_logits(res, world, single[heads], f"heads {heads}")


def test_generate_returns_the_same_on_every_rank(ranks):
    world, heads, res = ranks
    for name, kw in TP.MATRIX:
        g0 = res[0][name]["gen"]
        for r in range(1, world):
            assert res[r][name]["gen"] == g0, (name, r)          # "pen": tokens and log-probabilities
        toks = g0[0] if name == "pen" else g0
        assert [len(t) for t in toks] == [n + TP.NEW for n in kw.get("prompt_lens", [TP.T] * TP.B)], name
        assert all(0 <= t < TP.VOCAB for row in toks for t in row), name
    assert [len(r) for r in res[0]["pen"]["gen"][1]] == [TP.NEW] * TP.B


def test_coded_projections_run_on_their_codes_and_the_others_on_bf16(ranks, single):
    world, heads, res = ranks
    for w, rs in ((world, res), (1, {0: single[heads]})):
        for name, kw in TP.MATRIX:
            for r in range(w):
                assert rs[r][name]["routes"] == rs[r][name]["want_routes"], (name, w, r)
            wd = kw.get("weight_dtype")
            if wd:
                got = [sum(route != "bf16" for route, _, _ in rs[r][name]["routes"]) for r in range(w)]
                assert got == TP.CODED_COUNTS[wd][(w, heads)], (name, w)
    if (world, heads) == (2, 3):        # the mixed step: rank 0's Wo on MXFP4 codes, rank 1's on bf16
        assert ("w4", "0.wo", True) in res[0]["w4"]["routes"] and ("bf16", "0.wo", True) in res[1]["w4"]["routes"]


def test_all_features_over_xgmi(monkeypatch, single):
    """The "all" entry (MXFP4 weights, fp8 paged cache, ragged prompts) at two ranks, heads 3, with the TP
    collectives on the xGMI kernels: the decode all-reduce is a 3 x 192 bf16 tensor, 1152 bytes.
    ``DPFS_TP_COMM=xgmi`` routes every size class to the two-shot kernels, this message too; the route that
    ``tp_comm.decision()`` reports is asserted as it is, nothing is forced past it."""
    monkeypatch.setenv("DPFS_TP_COMM", "xgmi")
    res = run_distributed(_serve, 2, 3, ("all",), "xgmi", timeout=120)
    _check_logits(res, 2, single[3], "xgmi heads 3")
    assert res[0]["all"]["gen"] == res[1]["all"]["gen"]
    assert res[0]["all"]["routes"] == res[0]["all"]["want_routes"]
    assert res[1]["all"]["routes"] == res[1]["all"]["want_routes"]
    for r in range(2):
        assert res[r]["decision"] is not None and res[r]["decision"]["use"]["all_reduce/s"] == "xgmi", res[r]["decision"]
        assert res[r]["decision"] == res[0]["decision"]
