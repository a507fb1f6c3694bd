"""Per-element error bounds of the optimizer and of the step's backward tail, on MI355X.

The fused Adam (with the clip scale and grad_sumsq), the RMSNorm backward as the engines call it
(dres, dbias, dw_out), the column sums, bias_residual / add_bias_, the embedding pair, the
two-pass CE chain and LayerNorm, each against the fp64 oracle and the derived unit of
tests/numerics.py (``numerics.assert_within`` at ``numerics.DERIVED``; exact equality where the
operation is a gather or a sum of small integers).  tests/test_numerics.py shows on the CPU that
an fp32 evaluation attains every bound and that the planted faults do not.  Inputs come from
seeded CPU generators; outputs a kernel does not allocate start as NaN.
"""

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, dtype=torch.bfloat16):
    return torch.randn(*shape, generator=_gen(seed)).to(dtype).to(DEV)


def _slab_view(n, dtype, fill, pad=N.ADAM_PAD):
    """(slab, view): a length-n view with ``pad`` sentinel elements on each side."""
    slab = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return slab, slab[pad:pad + n]


def _pads_intact(slab, n, fill, pad=N.ADAM_PAD):
    edge = torch.cat([slab[:pad], slab[pad + n:]])
    return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


# ----------------------------------------------------------------------------- Adam ----

def _adam_table(run):
    """Device state of a run: per tensor of N.ADAM_TABLE views into sentinel slabs."""
    tensors = N.adam_inputs(run)
    rows = []
    for (n, shadow), cpu in zip(N.ADAM_TABLE, tensors):
        row = {"n": n, "slabs": []}
        for name, t in zip("pgmv", cpu):
            slab, view = _slab_view(n, torch.float32, N.ADAM_SENTINEL)
            view.copy_(t)
            row[name] = view
            row["slabs"].append((slab, torch.float32))
        row["s"] = None
        if shadow:
            slab, view = _slab_view(n, torch.bfloat16, N.ADAM_SENTINEL)
            row["s"] = view
            row["slabs"].append((slab, torch.bfloat16))
        rows.append(row)
    return rows


@pytest.mark.parametrize("run", list(N.ADAM_RUNS))
def test_adam_step_bounds(C, run):
    """One adam_k step per run of N.ADAM_RUNS over the descriptor table N.ADAM_TABLE; p, exp_avg
    and exp_avg_sq against the fp64 step from the state the kernel was given.  The fresh run goes
    on for steps 2 and 3, each compared from the kernel's own previous state, so nothing compounds."""
    step0, _, wd, eps, gscale, dscale, plant = N.ADAM_RUNS[run]
    rows = _adam_table(run)
    desc, chunks = C.adam_build([r["p"] for r in rows], [r["g"] for r in rows], [r["m"] for r in rows],
                                [r["v"] for r in rows], [r["s"] for r in rows])
    ds = torch.tensor([dscale], dtype=torch.float32, device=DEV) if dscale is not None else None
    h = N.ADAM_HYPER
    for step in ((1, 2, 3) if run == "fresh" else (step0,)):
        before = [(r["p"].clone(), r["m"].clone(), r["v"].clone()) for r in rows]
        C.adam_step(desc, chunks, h["lr"], h["b1"], h["b2"], eps, wd, step, gscale, ds)
        sc = N.adam_scalars(eps=eps, wd=wd, step=step, gscale=gscale, **h)
        for r, (p0, m0, v0) in zip(rows, before):
            ref = N.ref_adam(p0, r["g"], m0, v0, sc, 1.0 if dscale is None else N.f32(dscale))
            for name in "pmv":
                N.assert_within(r[name], ref[name], ref["unit_" + name], N.DERIVED,
                                f"adam {run} step {step} n {r['n']} {name}", {0: (N.ADAM_CHUNK, 1024, 4)})
            if r["s"] is not None:
                assert torch.equal(r["s"], r["p"].bfloat16()), f"shadow of n {r['n']}"
            if plant == "still" and step == step0:
                assert wd == 0 and torch.equal(r["p"][::5], p0[::5]), "g = m = v = 0 without decay moved p"
            for slab, dt in r["slabs"]:
                assert _pads_intact(slab, r["n"], N.ADAM_SENTINEL), f"adam {run} n {r['n']} wrote outside a {dt} tensor"


def test_grad_sumsq_bound(C):
    rows = _adam_table("step2")
    desc, chunks = C.adam_build([r["p"] for r in rows], [r["g"] for r in rows], [r["m"] for r in rows],
                                [r["v"] for r in rows], [r["s"] for r in rows])
    got = C.grad_sumsq(desc, chunks)
    ref, unit = N.ref_grad_sumsq([r["g"] for r in rows])
    assert got.dtype == torch.float32 and got.numel() == 1
    N.assert_within(got.reshape(1), torch.tensor([ref], dtype=torch.float64, device=DEV),
                    torch.tensor([unit], dtype=torch.float64, device=DEV), N.DERIVED, "grad_sumsq")
    for r, cpu in zip(rows, N.adam_inputs("step2")):   # reads only
        assert torch.equal(r["g"].cpu(), cpu[1])


@pytest.mark.parametrize("gnorm_scale", [1.0, 0.01])
def test_fused_adam_max_grad_norm(C, gnorm_scale):
    """FusedAdam(max_grad_norm=1): the device clip coefficient reaches adam_k as dscale.  Gradient
    norm above the threshold (coef < 1) and below it (coef == 1 exactly).  The oracle is fed
    coef = min(1, c / (||g|| + 1e-6)) in fp64; the fp32 coefficient the optimizer computes (sums of
    squares of at most n_max terms, three adds across the parameters, sqrt, + 1e-6, the division)
    is within ((n_max + 4) / 2 + 3) U32 of it: ref_adam's s_err."""
    from distributed_pytorch_from_scratch_amd.ops.optim import FusedAdam
    c, lr, betas, eps, wd = 1.0, 1e-3, (0.9, 0.999), 1e-8, 0.1
    g = _gen(33)
    shapes = [(4, 8), (6, 4), (5,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in shapes]
    grads = [(gnorm_scale * torch.randn(*s, generator=g)).to(DEV) for s in shapes]
    p0 = [p.detach().clone() for p in ps]
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    opt = FusedAdam(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_grad_norm=c)
    opt.step()
    norm = sum(float(gr.double().pow(2).sum()) for gr in grads) ** 0.5
    assert (norm > c) == (gnorm_scale == 1.0)
    coef = min(1.0, c / (norm + 1e-6))
    n_max = max(gr.numel() for gr in grads)
    s_err = 0.0 if coef == 1.0 else (n_max + 4) / 2 + 3
    got_norm = opt.last_grad_norm.double().reshape(1)
    N.assert_within(got_norm, torch.tensor([norm], dtype=torch.float64, device=DEV),
                    torch.tensor([((n_max + 4) / 2 + 1) * N.U32 * norm], dtype=torch.float64, device=DEV), N.DERIVED,
                    "last_grad_norm")
    sc = N.adam_scalars(lr, betas[0], betas[1], eps, wd, 1)
    for p, q, gr in zip(ps, p0, grads):
        ref = N.ref_adam(q, gr, torch.zeros_like(q), torch.zeros_like(q), sc, coef, s_err)
        st = opt.state[p]
        for name, out in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            N.assert_within(out, ref[name], ref["unit_" + name], N.DERIVED,
                            f"FusedAdam max_grad_norm {tuple(q.shape)} {name} (coef {coef:.3g})")
        if p.dim() >= 2:
            assert torch.equal(p._dpfs_shadow[1], p.detach().bfloat16())
        assert torch.equal(p.grad, gr), "the clip must not rescale the stored gradient"


# ------------------------------------------------------------------- norm backward ----

NORM_CASES = [(M, D, torch.bfloat16) for M in (3, 37, 4100) for D in (64, 768)] + [(37, 768, torch.float32)]


def _norm_inputs(M, D, dt, seed=90):
    g = _gen(seed + M + D)
    x, dy, dres = (torch.randn(M, D, generator=g).to(dt).to(DEV) for _ in range(3))
    w = (torch.rand(D, generator=g) + 0.5).to(DEV)
    b = torch.randn(D, generator=g).to(DEV)
    return x, dy, dres, w, b


@pytest.mark.parametrize("use_db", [False, True])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("M,D,dt", NORM_CASES)
def test_rmsnorm_bwd_dres_dbias_dw_out_bounds(C, M, D, dt, use_res, use_db):
    """rmsnorm_bwd as the engines call it.  M 3: fewer rows than a block's four waves; M 4100: the
    row loop's second trip past the 1024-block grid; D 64: fewer vectors than lanes.  dw_out and
    dbias are views into NaN slabs: dw_out is the returned dw, and nothing beside them is written."""
    x, dy, dres, w, _ = _norm_inputs(M, D, dt)
    bf = dt == torch.bfloat16
    rstd = C.rmsnorm_fwd(x, w, 1e-5)[1]
    dw_slab, dw_buf = _slab_view(D, torch.float32, NAN)
    db_slab, db_buf = _slab_view(D, torch.float32, NAN)
    res = dres if use_res else None
    dx, dw = C.rmsnorm_bwd(dy, x, w, rstd, res, db_buf if use_db else None, dw_out=dw_buf)
    assert dw.data_ptr() == dw_buf.data_ptr() and dw.shape == (D,)
    assert _pads_intact(dw_slab, D, NAN) and _pads_intact(db_slab, D, NAN)
    assert use_db or bool(torch.isnan(db_buf).all())
    dxr, udx, dwr, udw, dbr, udb = N.ref_rmsnorm_bwd_dbias(dy, x, w, 1e-5, res, bf)
    what = f"rmsnorm_bwd {M}x{D} {dt} dres={use_res} dbias={use_db}"
    N.assert_within(dx, dxr, udx, N.DERIVED, what + " dx", {0: (4096, 4)})
    N.assert_within(dw_buf, dwr, udw, N.DERIVED, what + " dw")
    if use_db:
        N.assert_within(db_buf, dbr, udb, N.DERIVED, what + " dbias")


@pytest.mark.parametrize("M,D,dt", [(3, 64, torch.bfloat16), (37, 768, torch.bfloat16), (37, 768, torch.float32)])
def test_layernorm_bounds(C, M, D, dt):
    x, dy, _, w, b = _norm_inputs(M, D, dt)
    bf = dt == torch.bfloat16
    y, mean, rstd = C.layernorm_fwd(x, w, b, 1e-5)
    f = N.ref_layernorm_fwd(x, w, b, 1e-5, bf)
    for name, out in (("y", y), ("mean", mean), ("rstd", rstd)):
        N.assert_within(out, f[name], f["unit_" + name], N.DERIVED, f"layernorm_fwd {name} {M}x{D} {dt}")
    dx, dw, db = C.layernorm_bwd(dy, x, w, mean, rstd)
    g = N.ref_layernorm_bwd(dy, x, w, 1e-5, bf)
    for name, out in (("dx", dx), ("dw", dw), ("db", db)):
        N.assert_within(out, g[name], g["unit_" + name], N.DERIVED, f"layernorm_bwd {name} {M}x{D} {dt}")


# --------------------------------------------------------- column sums, bias, residual ----

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Nn", [8, 264, 768])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000, 4100])
def test_bias_grad_bounds_and_exact_integer_sums(C, M, Nn, dt):
    """Column sums across the 64-row chunk edges (63, 64, 65) and many chunks: randn against the
    derived unit; small integers (|x| <= 8: every partial sum is exact in fp32) must equal the
    int64 sums, so a row dropped or counted twice at a chunk boundary shows exactly."""
    x = _randn(M, Nn, seed=100 + M + Nn, dtype=dt)
    ref, unit = N.ref_colsum(x)
    out = C.bias_grad(x)
    assert out.dtype == torch.float32
    N.assert_within(out, ref, unit, N.DERIVED, f"bias_grad {M}x{Nn} {dt}", {0: (64, 8)})
    xi = torch.randint(-8, 9, (M, Nn), generator=_gen(101 + M + Nn)).to(DEV)
    assert torch.equal(C.bias_grad(xi.to(dt)).long(), xi.sum(0)), f"integer column sums {M}x{Nn} {dt}"


def test_swiglu_bwd_dbias_many_row_chunks(C):
    """The fused bias gradient of swiglu_bwd at M 4100, F 64: one column block, so the plan takes
    ceil(4100 / 64) = 65 row chunks and the second stage adds them."""
    M, F_ = 4100, 64
    gu, dh = _randn(M, 2 * F_, seed=102), _randn(M, F_, seed=103)
    db = torch.full((2 * F_,), NAN, device=DEV)
    dgu = C.swiglu_bwd(dh, gu, db)
    ref, unit, _, dbr, dbu = N.ref_swiglu_bwd(dh.double(), gu)
    N.assert_within(dgu, ref, unit, N.DERIVED, "swiglu_bwd 4100x64")
    N.assert_within(db, dbr, dbu, N.DERIVED, "swiglu_bwd dbias 4100x64")


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M,D", [(37, 768), (5, 8)])
def test_bias_residual_and_add_bias_bounds(C, M, D, with_bias):
    y, res = _randn(M, D, seed=104), _randn(M, D, seed=105)
    b = _randn(D, seed=106, dtype=torch.float32) if with_bias else None
    ref, unit, _ = N.ref_bias_residual(y, b, res)
    N.assert_within(C.bias_residual(y, b, res), ref, unit, N.DERIVED, f"bias_residual {M}x{D} bias={with_bias}")
    if with_bias:
        y2 = y.clone()
        assert C.add_bias_(y2, b).data_ptr() == y2.data_ptr()
        ref, unit, _ = N.ref_bias_residual(y, b, torch.zeros_like(y))
        N.assert_within(y2, ref, unit, N.DERIVED, f"add_bias_ {M}x{D}")


# ------------------------------------------------------------------------ embedding ----

@pytest.mark.parametrize("M", [1, 5, 513])
@pytest.mark.parametrize("D", [4, 20, 260, 768])
def test_embedding_fwd_is_an_exact_gather(C, D, M):
    """A gather plus at most one rounding: bf16 out == w[id - start].bfloat16() on hits, 0 on
    misses; fp32 out the rows themselves.  D 260: 65 vectors, a second trip of the lane loop."""
    V, start = 50, 70
    w = _randn(V, D, seed=110 + D, dtype=torch.float32)
    ids = torch.randint(start - 20, start + V + 20, (M,), generator=_gen(111 + M))
    edge = torch.tensor([start - 1, start, start + V - 1, start + V])
    ids[: min(M, 4)] = edge[(torch.arange(min(M, 4)) + M) % 4]      # M 1 and 5 start at different edges
    if M >= 4:
        assert set(edge.tolist()) <= set(ids.tolist())
    ids = ids.to(DEV)
    keep = ids.clone()
    hit = (ids >= start) & (ids < start + V)
    rows = torch.where(hit[:, None], w[(ids - start).clamp(0, V - 1)], torch.zeros((), device=DEV))
    out16 = C.embedding_fwd(ids, w, start, torch.bfloat16)
    out32 = C.embedding_fwd(ids, w, start, torch.float32)
    assert out16.dtype == torch.bfloat16 and torch.equal(out16, rows.bfloat16())
    assert out32.dtype == torch.float32 and torch.equal(out32, rows)
    assert torch.equal(ids, keep)


@pytest.mark.parametrize("v_local", [1, 3, 300])
@pytest.mark.parametrize("M", [100, 1025, 2050])
@pytest.mark.parametrize("D", [4, 260, 768])
def test_embedding_bwd_sorted_bounds(C, D, M, v_local):
    """Segments of 0, 1, 3, 4, 5, 8 and 130 rows (the four-at-a-time loop and its tail), across the
    1024-token sort chunks, two shards, accumulate on and off: integer-valued dout must equal the
    int64 index_add exactly, randn dout stays within (count + 1) U32 sum|rows| (+ U32 |acc|)."""
    g = _gen(120 + D + M + v_local)
    dout = torch.randn(M, D, generator=g).bfloat16().to(DEV)
    dint = torch.randint(-8, 9, (M, D), generator=g).to(DEV)
    acc0 = torch.randn(v_local, D, generator=g).to(DEV)
    aint = torch.randint(-8, 9, (v_local, D), generator=g).to(DEV)
    for start in (v_local, 2 * v_local):                    # two shards of a three-shard vocabulary
        ids = N.emb_ids(M, v_local, start, 121 + M).to(DEV)
        keep = ids.clone()
        hit = (ids >= start) & (ids < start + v_local)
        want = torch.zeros(v_local, D, dtype=torch.int64, device=DEV).index_add_(0, (ids - start)[hit], dint[hit])
        for accumulate in (False, True):
            what = f"embedding_bwd_sorted D {D} M {M} v_local {v_local} start {start} accumulate={accumulate}"
            out = aint.float() if accumulate else torch.full((v_local, D), NAN, device=DEV)
            r = C.embedding_bwd_sorted(dint.bfloat16(), ids, v_local, start, out=out, accumulate=accumulate)
            assert r.data_ptr() == out.data_ptr()
            assert torch.equal(out.long(), want + (aint if accumulate else 0)) and bool(torch.isfinite(out).all()), what
            out = acc0.clone() if accumulate else torch.full((v_local, D), NAN, device=DEV)
            C.embedding_bwd_sorted(dout, ids, v_local, start, out=out, accumulate=accumulate)
            ref, unit = N.ref_embedding_bwd(dout, ids, v_local, start, acc0 if accumulate else None)
            N.assert_within(out, ref, unit, N.DERIVED, what, {1: (256, 4)})
        assert torch.equal(ids, keep)


# ---------------------------------------------------------------------- two-pass CE ----

CE2_SHARDS = [(0, 1000), (1000, 997)]
CE2_CASES = [(M, V, [(0, valid)], False, 1) for M, V, valid in N.CE_CASES] + [
    (65, 1000, CE2_SHARDS, False, 1),          # two shards: statistics gathered as (2, M, 3)
    (65, 1003, [(0, 1003)], False, 1),         # V % 8 != 0: the element-wise access path
    (65, 1000, CE2_SHARDS, False, 2),          # the loss over two row chunks (first / last)
    (65, 1000, CE2_SHARDS, True, 1),           # every target ignored
]


@pytest.mark.parametrize("M,V,shards,all_ignored,nchunk", CE2_CASES)
def test_two_pass_ce_chain_bounds(C, M, V, shards, all_ignored, nchunk):
    """ce_fwd_stats -> ce_finalize -> ce_grad_scale -> ce_bwd (+ dbias) as one chain, every stage
    against the oracle of the stage before's own fp32 output."""
    logits, tgt = N.ce2_inputs(M, V, shards, DEV, all_ignored=all_ignored)
    assert all_ignored or ((tgt == -1).any() and (tgt >= shards[-1][0] + shards[-1][1]).any())
    stats = []
    for x, (st, va) in zip(logits, shards):
        s = C.ce_fwd_stats(x, tgt, st, va)
        ref, unit = N.ref_ce_stats(x, tgt, st, va)
        N.assert_within(s, ref, unit, N.DERIVED, f"ce_fwd_stats {M}x{V} shard at {st}")
        stats.append(s)
    stats = torch.stack(stats)
    assert stats.shape == (len(shards), M, 3)
    acc = torch.full((2,), NAN, device=DEV)
    loss = torch.full((), NAN, device=DEV)
    edges = [0, M] if nchunk == 1 else [0, 40, M]
    lse, valid, run_sum, run_unit, run_cnt = [], [], 0.0, 0.0, 0.0
    for ci in range(nchunk):
        a, b = edges[ci], edges[ci + 1]
        l, v = C.ce_finalize(stats[:, a:b].contiguous(), tgt[a:b].contiguous(), -1, acc, loss, ci == 0, ci == nchunk - 1)
        f = N.ref_ce_finalize(stats[:, a:b], tgt[a:b], -1)
        N.assert_within(l, f["lse"], f["unit_lse"], N.DERIVED, f"ce_finalize lse rows {a}:{b}")
        assert torch.equal(v.double(), f["valid"])
        run_sum += float(f["loss_sum"])
        run_unit += float(f["unit_loss_sum"]) + N.U32 * abs(run_sum)         # the add into the running sum
        run_cnt += float(f["count"])
        lse.append(l)
        valid.append(v)
    lse, valid = torch.cat(lse), torch.cat(valid)
    n_valid = max(run_cnt, 1.0)
    assert float(acc[1]) == n_valid
    assert abs(float(acc[0]) - run_sum) <= N.DERIVED * run_unit
    assert abs(float(loss) - run_sum / n_valid) <= N.DERIVED * (run_unit / n_valid + N.U32 * abs(run_sum / n_valid))
    gloss = torch.tensor(1.0, device=DEV)
    gs = C.ce_grad_scale(valid, gloss, acc[1:2])
    gref = valid.double() / n_valid
    N.assert_within(gs, gref, 2 * N.U32 * gref, N.DERIVED, "ce_grad_scale")
    for x, (st, va) in zip(logits, shards):
        keep = x.clone()
        out = torch.full_like(x, NAN)
        db = torch.full((V,), NAN, device=DEV)
        C.ce_bwd(x, tgt, lse, gs, st, va, out, db)
        ref, unit, dbr, dbu = N.ref_ce_bwd(x, tgt, lse, gs, st, va)
        what = f"ce_bwd {M}x{V} shard at {st}"
        N.assert_within(out, ref, unit, N.DERIVED, what, {1: (256, 8)})
        N.assert_within(db, dbr, dbu, N.DERIVED, what + " dbias")
        assert torch.equal(x, keep)
        if all_ignored:
            assert float(loss) == 0 and not out.any() and not db.any() and n_valid == 1
