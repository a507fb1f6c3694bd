"""The per-element bounds themselves, on the CPU (tests/numerics.py).

* Every rounding-emulating reference stays within half its ``LIMITS`` entry at every shape,
  input family and seed the GPU tests use (the limit is 2 x the emulation's worst value).
* Planted faults (a wrong rounding mode, a 0.5 % scale, a mis-indexed bias row, a zeroed 16 x 16
  block, one attention row off by 3 %, one lse entry off by 1e-3, one row rotated with its
  neighbour's position) fail ``assert_within`` or the bias statistic while the global Frobenius
  ratio the older tests use stays under their threshold.
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
