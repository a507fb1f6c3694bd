"""The per-element bounds themselves, on the CPU (tests/numerics.py).

* Every rounding-emulating reference stays within half its ``LIMITS`` entry at every shape,
  input family and seed the GPU tests use (the limit is 2 x the emulation's worst value).
* Planted faults (a wrong rounding mode, a 0.5 % scale, a mis-indexed bias row, a zeroed 16 x 16
  block, one attention row off by 3 %, one lse entry off by 1e-3, one row rotated with its
  neighbour's position) fail ``assert_within`` or the bias statistic while the global Frobenius
  ratio the older tests use stays under their threshold.
* The optimizer, step-tail and decode oracles (second half): an fp32 evaluation of each stays
  within the derived limit at the GPU tests' cases, and each planted fault fails it.
"""
import pytest
import torch

import numerics as N


def _attn_emulated(hd, T, causal, fam, rope=False):
    q, k, v, do, pos = N.attn_inputs(hd, T, fam)
    tab = N.rope_table(512, hd) if rope else None
    scale = hd ** -0.5
    ref = N.attn_refs(q, k, v, do, scale, causal, pos if rope else None, tab)
    o, lse = N.emu_attn_fwd(q, k, v, scale, causal)
    dq, dk, dv, db = N.emu_attn_bwd(do, q, k, v, o, lse, scale, causal, pos if rope else None, tab)
    return ref, {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "dbias": db}


@pytest.mark.parametrize("fam", list(N.ATTN_FAMILIES))
@pytest.mark.parametrize("hd,T,causal", N.ATTN_CASES)
def test_attention_emulation_within_half_its_limit(hd, T, causal, fam):
    ref, out = _attn_emulated(hd, T, causal, fam)
    for name in ("o", "lse", "dq", "dk", "dv"):
        e = N.LIMITS[N.attn_key(name, hd)]
        assert e["limit"] == 2 * e["measured"]
        N.assert_within(out[name], ref[name], ref["unit_" + name], 1.001 * e["measured"], f"emulated {name}",
                        N.ATTN_TILES[name])


@pytest.mark.parametrize("fam", list(N.ATTN_FAMILIES))
@pytest.mark.parametrize("hd,T", N.ATTN_ROPE_CASES)
def test_attention_rope_dbias_emulation_within_half_its_limit(hd, T, fam):
    ref, out = _attn_emulated(hd, T, True, fam, rope=True)
    for name in ("dq", "dk", "dbias"):
        e = N.LIMITS[N.attn_key(name, hd, True)]
        N.assert_within(out[name], ref[name], ref["unit_" + name], 1.001 * e["measured"], f"emulated {name} (rope)")
    N.assert_within(out["dv"], ref["dv"], ref["unit_dv"], 1.001 * N.LIMITS[N.attn_key("dv", hd)]["measured"], "dv")


@pytest.mark.parametrize("M,V,valid", N.CE_CASES)
def test_ce_emulation_within_half_its_limit(M, V, valid):
    logits, tgt, gs = N.ce_inputs(M, V, valid)
    assert (tgt == -1).any()
    ref = N.ref_ce_fused(logits, tgt, gs, valid)
    st, g, db = N.emu_ce_fused(logits, tgt, gs, valid)
    N.assert_within(g, ref["grad"], ref["unit_grad"], 1.001 * N.LIMITS["ce.grad"]["measured"], "emulated d logits")
    N.assert_within(db, ref["dbias"], ref["unit_dbias"], 1.001 * N.LIMITS["ce.dbias"]["measured"], "emulated dbias")
    N.assert_within(st, ref["stats"], ref["unit_stats"], N.DERIVED, "emulated loss statistics")
    assert not g[:, valid:].any() and not g[tgt == -1].any()


# ------------------------------------------------------------------ planted faults ----

def _gemm_case(M, Nn, K, seed=0):
    """Correctly rounded NT GEMM + bias: fp32 accumulate, round to nearest even."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=gen).bfloat16()
    b = torch.randn(Nn, K, generator=gen).bfloat16()
    bias = torch.randn(Nn, generator=gen)
    acc = a.float() @ b.float().t() + bias
    ref, mag = N.ref_gemm(a, b, "nt", bias)
    return a, b, bias, acc, ref, mag


def _caught(fn):
    with pytest.raises(AssertionError):
        fn()


TILES = {0: (256, 128, 16), 1: (256, 192, 16)}


@pytest.mark.parametrize("M,Nn,K", [(257, 264, 96), (33, 200, 32), (257, 264, 128)])
def test_gemm_correct_rounding_passes_and_rounding_faults_are_caught(M, Nn, K):
    a, b, bias, acc, ref, mag = _gemm_case(M, Nn, K)
    unit, at = N.unit_gemm_bf16(ref, mag, K), N.acc_term_gemm(mag, K)
    good = acc.bfloat16()
    worst = N.assert_within(good, ref, unit, N.DERIVED, "rounded")
    assert 0.5 < worst <= 1.0
    big = M * Nn > 50000 and K <= 96      # where the statistic applies (see test_bias_stat_restriction)
    if big:
        _, _, dropped = N.bias_stat(good, ref, at, "rounded")
        assert dropped < 0.10
    for name, bad in (("truncated", N.bf16_trunc(acc)), ("scaled by 1.005", (acc * 1.005).bfloat16())):
        assert N.rel(bad, ref) < 1e-2, name               # the old check passes
        _caught(lambda: N.assert_within(bad, ref, unit, N.DERIVED, name))
        if big:
            _caught(lambda: N.bias_stat(bad, ref, at, name))
    if big:   # a 0.1 % scale error stays inside the per-element bound for most elements: the statistic sees it
        bad = (acc * 1.001).bfloat16()
        assert N.rel(bad, ref) < 1e-2
        _caught(lambda: N.bias_stat(bad, ref, at, "scaled by 1.001"))


def test_bias_stat_restriction_drops_few_elements():
    """The share of elements whose worst-case accumulation term reaches ulp / 16, for randn
    operands: under 10 % up to K = 96 (the shapes the GPU tests apply the statistic at); it grows
    with K (the term is (K + 2) 2^-24 |a| |b| ~ K^2, an ulp of the result ~ sqrt K), which is why
    the statistic is not applied at the larger K."""
    shares = {}
    for M, Nn, K in [(257, 264, 96), (520, 392, 96), (257, 264, 32)]:
        a, b, bias, acc, ref, mag = _gemm_case(M, Nn, K, seed=3)
        shares[K] = N.bias_stat(acc.bfloat16(), ref, N.acc_term_gemm(mag, K), f"K {K}")[2]
        assert shares[K] < 0.10
    a, b, bias, acc, ref, mag = _gemm_case(257, 264, 320, seed=3)
    with pytest.raises(AssertionError, match="drops"):
        N.bias_stat(acc.bfloat16(), ref, N.acc_term_gemm(mag, 320), "K 320")


@pytest.mark.parametrize("M,Nn,K,old", [(257, 264, 128, 1e-2), (1000, 768, 96, 1e-2)])
def test_shifted_bias_row_is_caught(M, Nn, K, old):
    a, b, bias, acc, ref, mag = _gemm_case(M, Nn, K, seed=1)
    bad = acc.clone()
    bad[-1] = acc[-1] - bias + bias.roll(1)
    bad = bad.bfloat16()
    assert N.rel(bad, ref) < old
    with pytest.raises(AssertionError, match=rf"at \({M - 1}, ") as e:
        N.assert_within(bad, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, "shifted bias", TILES)
    assert f"{M - 1} % 256 = {(M - 1) % 256}" in str(e.value) and "elements over the limit" in str(e.value)


def test_zeroed_16x16_block_is_caught():
    M, Nn, K = 4096, 2304, 64
    a, b, bias, acc, ref, mag = _gemm_case(M, Nn, K, seed=2)
    bad = acc.bfloat16()
    bad[M - 16:, Nn - 16:] = 0
    assert N.rel(bad, ref) < 1e-2
    with pytest.raises(AssertionError, match="256 of"):
        N.assert_within(bad, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, "zeroed block", TILES)


def test_attention_row_and_lse_faults_are_caught():
    hd, T = 64, 300
    ref, out = _attn_emulated(hd, T, True, "randn")
    o = out["o"].float().clone()
    o[1, 200, 2] *= 1.03                                   # one query row of one head
    o = o.bfloat16()
    assert N.rel(o, ref["o"]) < 2e-2                       # the old threshold
    with pytest.raises(AssertionError, match=r"at \(1, 200, 2, "):
        N.assert_within(o, ref["o"], ref["unit_o"], N.limit(N.attn_key("o", hd)), "o row x 1.03", N.ATTN_TILES["o"])
    lse = out["lse"].clone()
    lse[0, 1, 77] += 1e-3
    assert (lse.double() - ref["lse"]).abs().max() < 2e-2  # the old absolute check
    with pytest.raises(AssertionError, match=r"at \(0, 1, 77\)"):
        N.assert_within(lse, ref["lse"], ref["unit_lse"], N.limit(N.attn_key("lse", hd)), "lse + 1e-3")


def test_rope_row_with_neighbours_position_is_caught():
    M, K, heads, hd = 1000, 64, 12, 64
    Nn = 3 * heads // 2 * hd
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=gen).bfloat16()
    b = (torch.randn(Nn, K, generator=gen) / K ** 0.5).bfloat16()
    bias = torch.randn(Nn, generator=gen)
    pos = torch.randint(0, 511, (M,), generator=gen)
    tab = N.rope_table(512, hd)
    lin, mag = N.ref_gemm(a, b, "nt", bias)
    ref, rmag = N.ref_rope(lin, pos, tab, heads, hd)
    unit = N.U16 * ref.abs() + N.ref_rope(lin, pos, tab, heads, hd, mag=N.acc_term_gemm(mag, K))[1] + 3 * N.U32 * rmag
    acc = a.float() @ b.float().t() + bias

    def emulate(p):          # the GEMM epilogue rotates the fp32 accumulator, one rounding at the store
        return N.ref_rope(acc.double(), p, tab, heads, hd)[0].float().bfloat16()
    N.assert_within(emulate(pos), ref, unit, N.DERIVED, "rope epilogue")
    wrong = pos.clone()
    wrong[613] += 1
    bad = emulate(wrong)
    assert N.rel(bad, ref) < 1e-2
    with pytest.raises(AssertionError, match=r"at \(613, "):
        N.assert_within(bad, ref, unit, N.DERIVED, "rope row", TILES)


def test_unit_zero_and_causal_query_zero():
    """Where the unit is 0 the output must be exact; and the one place an attention unit would be
    0 without the delta term: query 0 of a causal row sees only key 0, so dS == 0 and dq == 0 up
    to the bf16 o inside delta."""
    ref = torch.tensor([0.0, 1.0], dtype=torch.float64)
    unit = torch.tensor([0.0, 1e-3], dtype=torch.float64)
    assert N.assert_within(torch.tensor([0.0, 1.0005]), ref, unit, 1.0, "exact zero") < 1.0
    with pytest.raises(AssertionError, match="inf"):
        N.assert_within(torch.tensor([1e-30, 1.0]), ref, unit, 1.0, "not exact")
    with pytest.raises(AssertionError):
        N.assert_within(torch.tensor([float("nan"), 1.0]), ref, unit, 1.0, "unwritten")
    r, out = _attn_emulated(64, 65, True, "randn")
    assert r["dq"][:, 0].abs().max() < 1e-13               # exactly 0 in exact arithmetic
    assert (r["unit_dq"][:, 0] > 0).all()                  # the delta term
    assert out["dq"][:, 0].float().abs().max() > 0         # the emulation (as a kernel) is not 0 there
    N.assert_within(out["dq"][:, :1], r["dq"][:, :1], r["unit_dq"][:, :1], N.limit("attn.dq.hd64"), "dq of query 0")


# ======================================================== optimizer, step tail, decode ====
# For every oracle of these sections an fp32 evaluation of the same math (adam_fp32, norm_fp32,
# ce_*_fp32, emu_attn_decode, plain fp32 sums) stays within the DERIVED limit at the GPU tests'
# cases: a correct kernel can attain the bounds.  Each planted fault, applied to that fp32
# evaluation, fails the same check.

def _adam_case(run):
    step, _, wd, eps, gscale, dscale, plant = N.ADAM_RUNS[run]
    sc = N.adam_scalars(eps=eps, wd=wd, step=step, gscale=gscale, **N.ADAM_HYPER)
    return sc, dscale, plant, N.adam_inputs(run)


def _adam_check(out, ref, what):
    for name, o in zip("pmv", out):
        N.assert_within(o, ref[name], ref["unit_" + name], N.DERIVED, f"{what} {name}", {0: (N.ADAM_CHUNK, 1024, 4)})


@pytest.mark.parametrize("run", list(N.ADAM_RUNS))
def test_adam_fp32_evaluation_within_its_units(run):
    sc, dscale, plant, tensors = _adam_case(run)
    for (n, _), (p, g, m, v) in zip(N.ADAM_TABLE, tensors):
        ref = N.ref_adam(p, g, m, v, sc, 1.0 if dscale is None else N.f32(dscale))
        out = N.adam_fp32(p, g, m, v, sc, dscale)
        _adam_check(out, ref, f"adam {run} n {n}")
        if plant == "still":
            assert sc["wd"] == 0 and torch.equal(out[0][::5], p[::5])      # g = m = v = 0, no decay: p untouched


@pytest.mark.parametrize("fault,run", [("dscale_ignored", "dscale"), ("wd_clipped", "both"), ("bc2_not_sqrt", "step2"),
                                       ("bc2_not_sqrt", "step1000"), ("eps_before_division", "eps1e-3"),
                                       ("last_vector_skipped", "step2")])
def test_adam_planted_faults_are_caught(fault, run):
    sc, dscale, plant, tensors = _adam_case(run)
    for (n, _), (p, g, m, v) in zip(N.ADAM_TABLE, tensors):
        if fault == "last_vector_skipped" and n % 4:
            continue                                   # the scalar path has no vectors
        if plant == "still" and n == 1:
            continue                                   # its one element is a planted g = m = v = 0: no update at all
        ref = N.ref_adam(p, g, m, v, sc, 1.0 if dscale is None else N.f32(dscale))
        bad = N.adam_fp32(p, g, m, v, sc, dscale, fault)
        _caught(lambda: _adam_check(bad, ref, f"{fault} n {n}"))


def test_adam_eps_placement_passes_the_old_check():
    """test_adam_matches_torch's own run (zero moments, steps 1 to 3, eps 1e-8, absolute 1e-5 on p
    alone): eps added before the bias-correction division stays under it; a clip scale or a decay
    scaled by it cannot show there at all (no scale is passed)."""
    gen = torch.Generator().manual_seed(11)
    for n in (1000, 16384 * 2 + 7, 4096):
        p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        runs = {}
        for fault in (None, "eps_before_division"):
            p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
            for step in (1, 2, 3):
                sc = N.adam_scalars(1e-3, 0.9, 0.95, 1e-8, 0.01, step)
                p, m, v = N.adam_fp32(p, g, m, v, sc, None, fault)
            runs[fault] = p
        assert (runs[None] - runs["eps_before_division"]).abs().max() < 1e-5


def test_grad_sumsq_fp32_within_its_unit():
    grads = [t[1] for t in N.adam_inputs("step2")]
    ref, unit = N.ref_grad_sumsq(grads)
    parts = [g[c:c + N.ADAM_CHUNK].pow(2).sum() for g in grads for c in range(0, g.numel(), N.ADAM_CHUNK)]
    got = torch.stack(parts).sum()
    assert abs(float(got) - ref) <= N.DERIVED * unit
    assert abs(float(torch.stack(parts[:-2] + parts[-1:]).sum()) - ref) > N.DERIVED * unit     # a dropped full chunk


# ---- norm backward with dres / dbias, LayerNorm

def _norm_inputs(M, D, dt, seed=90):
    gen = torch.Generator().manual_seed(seed + M + D)
    x, dy, dres = (torch.randn(M, D, generator=gen).to(dt) for _ in range(3))
    w = torch.rand(D, generator=gen) + 0.5
    b = torch.randn(D, generator=gen)
    return x, dy, dres, w, b


NORM_CASES = [(M, D, torch.bfloat16) for M in (3, 37, 4100) for D in (64, 768)] + [(37, 768, torch.float32)]


@pytest.mark.parametrize("M,D,dt", NORM_CASES)
def test_rmsnorm_bwd_dres_dbias_fp32_within_its_units(M, D, dt):
    x, dy, dres, w, _ = _norm_inputs(M, D, dt)
    bf = dt == torch.bfloat16
    for use_res in (False, True):
        r = dres if use_res else None
        dxr, udx, dwr, udw, dbr, udb = N.ref_rmsnorm_bwd_dbias(dy, x, w, 1e-5, r, bf)
        dx, dw, db = N.norm_fp32(dy, x, w, 2, r)
        N.assert_within(dx, dxr, udx, N.DERIVED, f"rmsnorm_bwd dx dres={use_res}")
        N.assert_within(dw, dwr, udw, N.DERIVED, "rmsnorm_bwd dw")
        N.assert_within(db, dbr, udb, N.DERIVED, f"rmsnorm_bwd dbias dres={use_res}")


def test_norm_backward_planted_faults_are_caught():
    M, D = 4100, 768        # 1024 blocks x 4 rows: rows 4096.. belong to the second trip of the row loop
    x, dy, dres, w, _ = _norm_inputs(M, D, torch.bfloat16)
    dxr, udx, dwr, udw, dbr, udb = N.ref_rmsnorm_bwd_dbias(dy, x, w, 1e-5, dres)
    dx, dw, db = N.norm_fp32(dy, x, w, 2, dres, fault="rows_past_grid")
    _caught(lambda: N.assert_within(dw, dwr, udw, N.DERIVED, "dw without the second trip"))
    _caught(lambda: N.assert_within(db, dbr, udb, N.DERIVED, "dbias without the second trip"))
    ln = N.ref_layernorm_bwd(dy, x, w, 1e-5)
    _, dw1, db1 = N.norm_fp32(dy, x, w, 1, fault="rows_past_grid")
    _caught(lambda: N.assert_within(dw1, ln["dw"], ln["unit_dw"], N.DERIVED, "LayerNorm dw without the second trip"))
    _caught(lambda: N.assert_within(db1, ln["db"], ln["unit_db"], N.DERIVED, "LayerNorm db without the second trip"))
    # dres added after the bf16 rounding, at the old test's shape (test_rmsnorm_bwd_fused_residual_grad)
    x, dy, dres, w, _ = _norm_inputs(513, 768, torch.bfloat16)
    dxr, udx, *_ = N.ref_rmsnorm_bwd_dbias(dy, x, w, 1e-5, dres)
    bad = N.norm_fp32(dy, x, w, 0, dres, fault="dres_after_rounding")[0]
    assert N.rel(bad, dxr) < 1e-2
    _caught(lambda: N.assert_within(bad, dxr, udx, N.DERIVED, "dres after the rounding"))


@pytest.mark.parametrize("M,D,dt", [(3, 64, torch.bfloat16), (37, 768, torch.bfloat16), (37, 768, torch.float32)])
def test_layernorm_fp32_within_its_units(M, D, dt):
    x, dy, _, w, b = _norm_inputs(M, D, dt)
    bf = dt == torch.bfloat16
    f = N.ref_layernorm_fwd(x, w, b, 1e-5, bf)
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    r = torch.rsqrt((xf - mu).pow(2).mean(-1, keepdim=True) + 1e-5)
    y = ((xf - mu) * r * w + b).to(dt)
    N.assert_within(y, f["y"], f["unit_y"], N.DERIVED, "layernorm y")
    N.assert_within(mu.squeeze(1), f["mean"], f["unit_mean"], N.DERIVED, "layernorm mean")
    N.assert_within(r.squeeze(1), f["rstd"], f["unit_rstd"], N.DERIVED, "layernorm rstd")
    g = N.ref_layernorm_bwd(dy, x, w, 1e-5, bf)
    dx, dw, db = N.norm_fp32(dy, x, w, 1)
    for name, o in (("dx", dx), ("dw", dw), ("db", db)):
        N.assert_within(o, g[name], g["unit_" + name], N.DERIVED, f"layernorm {name}")
    _caught(lambda: N.assert_within((y.float() - b).to(dt), f["y"], f["unit_y"], N.DERIVED, "bias dropped"))


# ---- column sums, embedding gradient

@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000, 4100])
def test_colsum_fp32_within_its_unit_and_a_doubled_row_is_caught(M):
    gen = torch.Generator().manual_seed(91 + M)
    x = torch.randn(M, 264, generator=gen).bfloat16()
    ref, unit = N.ref_colsum(x)
    chunks = [x[c:c + 64].float().sum(0) for c in range(0, M, 64)]
    N.assert_within(torch.stack(chunks).sum(0), ref, unit, N.DERIVED, f"column sums M {M}")
    b = min(64, M) - 1                          # the last row of the first chunk, counted by the next one too
    _caught(lambda: N.assert_within(torch.stack(chunks).sum(0) + x[b].float(), ref, unit, N.DERIVED, "doubled row"))
    xi = torch.randint(-8, 9, (M, 264), generator=gen)
    assert not torch.equal(xi.sum(0) + xi[b], xi.sum(0))


def test_embedding_gradient_fp32_within_its_unit_and_a_dropped_tail_is_caught():
    M, D, V, start = 1025, 260, 300, 300
    ids = N.emb_ids(M, V, start, 92)
    gen = torch.Generator().manual_seed(92)
    dout = torch.randn(M, D, generator=gen).bfloat16()
    acc = torch.randn(V, D, generator=gen)
    for a in (None, acc):
        ref, unit = N.ref_embedding_bwd(dout, ids, V, start, a)
        for drop_tail in (False, True):
            out = torch.zeros(V, D) if a is None else a.clone()
            for r in range(V):
                rows = (ids == start + r).nonzero().flatten()
                if drop_tail:
                    rows = rows[: len(rows) // 4 * 4]
                for j in rows:
                    out[r] += dout[j].float()
            if drop_tail:
                _caught(lambda: N.assert_within(out, ref, unit, N.DERIVED, "segment tail dropped"))
            else:
                N.assert_within(out, ref, unit, N.DERIVED, f"embedding gradient accumulate={a is not None}")


# ---- two-pass CE

CE2_SHARDS = [(0, 1000), (1000, 997)]


def _ce2_fp32(M, V, shards, all_ignored=False):
    logits, tgt = N.ce2_inputs(M, V, shards, all_ignored=all_ignored)
    stats = torch.stack([N.ce_fp32(x, tgt, st, va) for x, (st, va) in zip(logits, shards)])
    return logits, tgt, stats


@pytest.mark.parametrize("M,V,shards", [(300, 1000, [(0, 997)]), (77, 6288, [(0, 6241)]), (65, 1000, CE2_SHARDS),
                                        (65, 1003, [(0, 1003)])])
def test_two_pass_ce_fp32_within_its_units(M, V, shards):
    logits, tgt, stats = _ce2_fp32(M, V, shards)
    units = []
    for x, (st, va), s in zip(logits, shards, stats):
        ref, unit = N.ref_ce_stats(x, tgt, st, va)
        N.assert_within(s, ref, unit, N.DERIVED, f"ce statistics shard at {st}")
        units.append(unit[:, 1])
    lse, valid, lsum, cnt = N.ce_finalize_fp32(stats, tgt, -1)
    f = N.ref_ce_finalize(stats, tgt, -1)
    N.assert_within(lse, f["lse"], f["unit_lse"], N.DERIVED, "lse")
    assert torch.equal(valid.double(), f["valid"]) and float(cnt) == float(f["count"])
    assert abs(float(lsum) - float(f["loss_sum"])) <= N.DERIVED * float(f["unit_loss_sum"])
    gs = valid * (torch.tensor(1.0) / cnt.clamp_min(1))
    for x, (st, va) in zip(logits, shards):
        ref, unit, dbr, dbu = N.ref_ce_bwd(x, tgt, lse, gs, st, va)
        gr, db = N.ce_bwd_fp32(x, tgt, lse, gs, st, va)
        N.assert_within(gr, ref, unit, N.DERIVED, f"ce gradient shard at {st}", {1: (256, 8)})
        N.assert_within(db, dbr, dbu, N.DERIVED, f"ce dbias shard at {st}")


def test_two_pass_ce_planted_faults_are_caught():
    M, V = 65, 1000
    logits, tgt, stats = _ce2_fp32(M, V, CE2_SHARDS)
    f = N.ref_ce_finalize(stats, tgt, -1)
    lse1 = N.ce_finalize_fp32(stats, tgt, -1, only_shard=0)[0]
    _caught(lambda: N.assert_within(lse1, f["lse"], f["unit_lse"], N.DERIVED, "lse from one shard"))
    lse, valid, _, cnt = N.ce_finalize_fp32(stats, tgt, -1)
    gs = valid / cnt
    ref, unit, dbr, dbu = N.ref_ce_bwd(logits[1], tgt, lse, gs, 1000, 997)
    gr, db = N.ce_bwd_fp32(logits[1], tgt, lse, gs, 1000, 997, onehot_start=0)
    _caught(lambda: N.assert_within(gr, ref, unit, N.DERIVED, "one-hot of the wrong shard"))
    _caught(lambda: N.assert_within(db, dbr, dbu, N.DERIVED, "dbias with the one-hot of the wrong shard"))


# ---- decode

@pytest.mark.parametrize("fam", N.DEC_FAMILIES)
@pytest.mark.parametrize("Tmax", N.DEC_TMAX)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_decode_attention_fp32_within_its_unit(hd, Tmax, fam):
    qkv, kc, vc = N.dec_inputs(hd, Tmax, fam)
    lens = N.dec_lengths(Tmax)
    for la, lb in zip(lens, reversed(lens)):          # row 0 walks up, row 1 down: every length, mixed per row
        ln = torch.tensor([la, lb], dtype=torch.int32)
        ref, unit = N.ref_attn_decode(qkv, kc, vc, ln, hd ** -0.5)
        out = N.emu_attn_decode(qkv, kc, vc, ln, hd ** -0.5)
        N.assert_within(out, ref, unit, N.DERIVED, f"decode hd {hd} Tmax {Tmax} {fam} len {la},{lb}", {1: (hd, 8)})


@pytest.mark.parametrize("fault", ["drop_newest", "wave_factor", "norm_last_split"])
def test_decode_one_head_faults_are_caught(fault):
    """One (sequence, head) of 15 wrong at the old test's geometry (B 3, H 5, T_max 700, randn,
    len 699): the per-element bound names the sequence.  With the newest key dropped the
    Frobenius ratio stays under the old 1e-2 (0.003 to 0.03 over the three heads tried); the two
    merge faults move a whole head by 3 to 10 % and the old statistic sees them too."""
    hd, Tmax = 64, 700
    qkv, kc, vc = N.dec_inputs(hd, Tmax, "randn", B=3, H=5)
    ln = torch.tensor([699] * 3, dtype=torch.int32)
    ref, unit = N.ref_attn_decode(qkv, kc, vc, ln, hd ** -0.5)
    N.assert_within(N.emu_attn_decode(qkv, kc, vc, ln, hd ** -0.5), ref, unit, N.DERIVED, "decode at the old geometry")
    rels = []
    for b, h in [(0, 0), (1, 2), (2, 4)]:
        bad = N.emu_attn_decode(qkv, kc, vc, ln, hd ** -0.5, fault=(fault, b, h))
        rels.append(N.rel(bad, ref))
        with pytest.raises(AssertionError, match=rf"at \({b}, "):
            N.assert_within(bad, ref, unit, N.DERIVED, fault, {1: (hd, 8)})
    if fault == "drop_newest":
        assert min(rels) < 1e-2, rels                  # the old check passes at least one of the three heads


def test_decode_key_selection_is_exact_in_fp32():
    """The exact key-selection inputs: q[0] = 16, k[t*, 0] = 16, every other key -16: the other
    probabilities are below e^-45, so o equals v[t*] bit for bit."""
    hd, Tmax, B, H = 64, 300, 2, 3
    qkv, kc, vc, tstar, ln = N.dec_selection_inputs(hd, Tmax, 299)
    out = N.emu_attn_decode(qkv, kc, vc, ln, hd ** -0.5)
    want = torch.stack([vc[b, tstar[b, h], h] for b in range(B) for h in range(H)]).view(B, H * hd)
    assert torch.equal(out, want)


# ---- gemv

@pytest.mark.parametrize("Nn,K", N.GEMV_CASES)
def test_gemv_fp32_within_its_unit(Nn, K):
    for swiglu in (False, True) if (Nn, K) in N.GEMV_SWIGLU_CASES else (False,):
        x, w, bias = N.gemv_inputs(5, Nn, K, swiglu)
        ref, unit = N.ref_gemv(x, w, bias, swiglu)
        if swiglu:
            g, u = x.float()[:, :K], x.float()[:, K:]
            a = (g * torch.sigmoid(g) * u).bfloat16().float()
        else:
            a = x.float()
        y = (a @ w.float().t() + bias).bfloat16()
        N.assert_within(y, ref, unit, N.DERIVED, f"gemv {Nn}x{K} swiglu={swiglu}", N.GEMV_TILES)
        bad = (a[:, : K - 32] @ w.float()[:, : K - 32].t() + bias).bfloat16()     # the last K step dropped
        _caught(lambda: N.assert_within(bad, ref, unit, N.DERIVED, "last K step dropped", N.GEMV_TILES))
