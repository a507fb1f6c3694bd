"""Per-element error bounds of the fp32 compute path's HIP kernels against fp64 oracles, on MI355X.

The fp32-input MFMA GEMM (``gemm_f32``: fp32 and bf16 storage, split-K, unaligned views), the
fp32 flash attention (``attn_fwd_f32`` / ``attn_bwd_f32`` with the inverse RoPE and the QKV bias
gradient) and the shared templated kernels at fp32 storage, where a 16-byte vector holds 4
elements instead of 8 and every tail and alignment branch moves.  Every check is
``numerics.assert_within`` at ``numerics.DERIVED`` against the oracles of tests/numerics_f32.py and
tests/numerics.py, or exact equality where the operation is a sum of small integers;
tests/test_numerics_f32.py shows on the CPU that an fp32 evaluation attains the bounds and that
planted faults do not.  Inputs come from seeded CPU generators; outputs the caller allocates are
views of sentinel or NaN-filled slabs, so stray and missing writes show.
"""

import pytest
import torch

import numerics as N
import numerics_f32 as F

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=_gen(seed)).to(dtype).to(DEV)


# ----------------------------------------------------------------------------- GEMM ----

def _operands(M, Nn, K, layout, integers=False, dtype=torch.float32):
    return tuple(t.to(DEV) for t in F.gemm_operands(M, Nn, K, layout, 200, integers, dtype))


def _gemm(C, a, b, layout, bias=None, out=None, accumulate=False):
    return C.gemm_f32(a, b, F.LAYOUTS[layout], bias, out, accumulate)


def _check_f32(C, a, b, layout, bias, acc0, K, what):
    """One fp32-output GEMM (into a clone of ``acc0`` with accumulate) against the oracle."""
    out = acc0.clone() if acc0 is not None else None
    got = _gemm(C, a, b, layout, bias, out, acc0 is not None)
    assert got.dtype == torch.float32
    ref, mag = N.ref_gemm(a, b, layout, bias, acc0)
    N.assert_within(got, ref, N.unit_gemm_f32(mag, K, F.gemm_splits_for_unit(K), acc0), N.DERIVED, what, F.GEMM32_TILES)
    return got


def _variants(layout):
    """(with bias, accumulate): NT with bias and once without, NT once accumulating; TN also
    accumulating into a randn out."""
    if layout == "nt":
        return [(True, False), (False, False), (True, True)]
    return [(False, False)] + ([(False, True)] if layout == "tn" else [])


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
@pytest.mark.parametrize("M,Nn,K", F.GEMM32_SHAPES)
def test_gemm_f32_bounds_and_exact_integers(C, M, Nn, K, layout):
    """Every shape of F.GEMM32_SHAPES in the three layouts: randn operands against the derived
    unit, then operands (bias, out) drawn from the integers -8 .. 8, whose product a correct
    kernel reproduces exactly in any summation order."""
    for with_bias, accumulate in _variants(layout):
        what = f"gemm_f32 {layout} {M}x{Nn}x{K} bias={with_bias} accumulate={accumulate}"
        a, b, bias, acc = _operands(M, Nn, K, layout)
        _check_f32(C, a, b, layout, bias if with_bias else None, acc if accumulate else None, K, what)
        a, b, bias, acc = _operands(M, Nn, K, layout, integers=True)
        out = acc.clone() if accumulate else None
        got = _gemm(C, a, b, layout, bias if with_bias else None, out, accumulate)
        want = N.ref_gemm(a, b, layout, bias if with_bias else None, acc if accumulate else None)[0]
        assert torch.equal(got.double(), want), what + " (integers)"


def _views(x, kind):
    """x as a column slice of a wider sentinel buffer: "vec" leading dimension = 0 mod 4 and the
    base 4 floats in (the vector path), "off1" the same with the base 1 float in (the scalar
    path), "ld" a leading dimension != 0 mod 4."""
    c4 = (x.size(1) + 3) // 4 * 4
    ld, off = {"vec": (c4 + 8, 4), "off1": (c4 + 8, 1), "ld": (c4 + 5, 0)}[kind]
    return F.strided(x, ld, off)


@pytest.mark.parametrize("kind", ["vec", "off1", "ld"])
@pytest.mark.parametrize("layout", list(F.LAYOUTS))
@pytest.mark.parametrize("M,Nn,K", F.GEMM32_VIEW_SHAPES)
def test_gemm_f32_views_bounds(C, M, Nn, K, layout, kind):
    """Operands and output at unaligned base offsets and leading dimensions; the output is a
    column slice of a sentinel-filled wider buffer whose pads must stay intact."""
    a, b, bias, acc = _operands(M, Nn, K, layout)
    (abuf, av), (bbuf, bv) = _views(a, kind), _views(b, kind)
    assert (av.data_ptr() % 16 == 0 and av.stride(0) % 4 == 0) == (kind == "vec")
    keep_a, keep_b = abuf.clone(), bbuf.clone()
    bias = bias if layout == "nt" else None
    for accumulate in ((False, True) if layout == "tn" else (False,)):
        what = f"gemm_f32 {layout} {M}x{Nn}x{K} views={kind} accumulate={accumulate}"
        obuf, ov = F.strided(acc if accumulate else torch.full_like(acc, NAN), Nn + 5, 3)
        got = _gemm(C, av, bv, layout, bias, ov, accumulate)
        assert got.data_ptr() == ov.data_ptr()
        ref, mag = N.ref_gemm(a, b, layout, bias, acc if accumulate else None)
        unit = N.unit_gemm_f32(mag, K, F.gemm_splits_for_unit(K), acc if accumulate else None)
        N.assert_within(ov, ref, unit, N.DERIVED, what, F.GEMM32_TILES)
        assert F.pads_intact(obuf, ov), what + ": wrote outside the output view"
    assert torch.equal(abuf, keep_a) and torch.equal(bbuf, keep_b)
    ai, bi, biasi, _ = _operands(M, Nn, K, layout, integers=True)
    got = _gemm(C, _views(ai, kind)[1], _views(bi, kind)[1], layout, biasi if layout == "nt" else None)
    assert torch.equal(got.double(), N.ref_gemm(ai, bi, layout, biasi if layout == "nt" else None)[0])


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
@pytest.mark.parametrize("M,Nn,K", F.GEMM32_BF16_SHAPES)
def test_gemm_f32_bf16_storage_bounds(C, M, Nn, K, layout):
    """The instantiations gemm_select._unaligned uses: bf16 in / bf16 out for NT (+ bias) and NN
    (one rounding of the fp32 accumulator; the splits are added to K in its fp32 term), bf16 in /
    fp32 out for TN with accumulate.  The integer form equals the exact product (rounded once to
    bf16 where the output is bf16)."""
    a, b, bias, acc = _operands(M, Nn, K, layout, dtype=BF)
    ai, bi, biasi, acci = _operands(M, Nn, K, layout, integers=True, dtype=BF)
    what = f"gemm_f32 bf16 storage {layout} {M}x{Nn}x{K}"
    if layout == "tn":
        _check_f32(C, a, b, layout, None, acc, K, what + " accumulate")
        _check_f32(C, a, b, layout, None, None, K, what)
        out = acci.clone()
        _gemm(C, ai, bi, layout, None, out, True)
        assert torch.equal(out.double(), N.ref_gemm(ai, bi, layout, None, acci)[0]), what + " (integers)"
        return
    bias, biasi = (bias, biasi) if layout == "nt" else (None, None)
    got = _gemm(C, a, b, layout, bias)
    assert got.dtype == BF
    ref, mag = N.ref_gemm(a, b, layout, bias)
    N.assert_within(got, ref, N.unit_gemm_bf16(ref, mag, K + F.gemm_splits_for_unit(K)), N.DERIVED, what, F.GEMM32_TILES)
    want = N.ref_gemm(ai, bi, layout, biasi)[0]
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(_gemm(C, ai, bi, layout, biasi), want.float().bfloat16()), what + " (integers)"


def test_gemm_f32_bf16_output_rounding_mode(C):
    """The magnitude-bias statistic of the bf16 store (round to nearest even, not chopped)."""
    M, Nn, K = F.GEMM32_STAT_SHAPE
    a, b, bias, _ = _operands(M, Nn, K, "nt", dtype=BF)
    got = _gemm(C, a, b, "nt", bias)
    ref, mag = N.ref_gemm(a, b, "nt", bias)
    what = f"gemm_f32 bf16 storage nt {M}x{Nn}x{K}"
    N.assert_within(got, ref, N.unit_gemm_bf16(ref, mag, K + 1), N.DERIVED, what, F.GEMM32_TILES)
    N.bias_stat(got, ref, N.acc_term_gemm(mag, K + 1), what)


# ------------------------------------------------------------------------ attention ----

def _nan_grads(B, T, H, hd, pad=8):
    """(slab, dq, dk, dv): packed (B T, 3 H hd) gradient views at the head of a NaN slab with
    ``pad`` more NaN rows behind them: a write to a row >= T of the last batch lands in the pad."""
    slab = torch.full((B * T + pad, 3 * H * hd), NAN, device=DEV)
    return (slab,) + N.packed_views(slab, B, T, H, hd)


def _run_attention(C, hd, T, causal, fam, rope=False, B=2, H=3):
    q, k, v, do, pos = F.attn32_inputs(hd, T, fam, DEV, B, H)
    scale = F.scale_f32(hd)
    tab = N.rope_table(512, hd).to(DEV)
    ref = F.ref_attn32(q, k, v, do, scale, causal, pos if rope else None, tab if rope else None)
    o, lse = C.attn_fwd_f32(q, k, v, scale, causal)
    # the backward is fed the oracle's o and lse rounded to fp32: a forward fault cannot leak into it
    # (copied into a fresh tensor: at T = 1 a transposed view counts as contiguous with other strides)
    o_in, lse_in = torch.empty(B, T, H, hd, device=DEV).copy_(ref["o"]), ref["lse"].float().contiguous()
    slab, dq, dk, dv = _nan_grads(B, T, H, hd)
    out = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    db = torch.full((3 * H * hd,), NAN, device=DEV)
    if rope:
        assert C.attn_bwd_f32(do, q, k, v, o_in, lse_in, scale, causal, dq, dk, dv, pos, tab, db)
        out["dbias"] = db
    else:
        # no rope_pos: the table alone must not rotate; no dbias: nothing writes the spare tensor
        assert not C.attn_bwd_f32(do, q, k, v, o_in, lse_in, scale, causal, dq, dk, dv, None, tab, None)
        assert bool(torch.isnan(db).all())
    assert bool(torch.isnan(slab[B * T:]).all()), "wrote a row outside the batch"
    return ref, out


def _assert_all(ref, out, names, what):
    for name in names:
        N.assert_within(out[name], ref[name], ref["unit_" + name], N.DERIVED, f"{what} {name}", F.ATTN32_TILES[name])


@pytest.mark.parametrize("fam", list(F.ATTN32_FAMILIES))
@pytest.mark.parametrize("hd,T,causal", F.ATTN32_CASES)
def test_attention_f32_bounds(C, hd, T, causal, fam):
    """Packed fp32 QKV views, B 2, H 3: partial single tiles (T 1, 33), one key past a key tile
    (65), a second query block of one query (129), a dK/dV key block whose first query tile is
    partial (193), ragged last tiles everywhere (300); causal and not at every head_dim."""
    ref, out = _run_attention(C, hd, T, causal, fam)
    _assert_all(ref, out, ("o", "lse", "dq", "dk", "dv"), f"attn_f32 hd {hd} T {T} causal={causal} {fam}")


@pytest.mark.parametrize("fam", list(F.ATTN32_FAMILIES))
@pytest.mark.parametrize("hd,T", F.ATTN32_ROPE_CASES)
def test_attention_f32_bwd_rope_dbias_bounds(C, hd, T, fam):
    ref, out = _run_attention(C, hd, T, True, fam, rope=True)
    _assert_all(ref, out, ("dq", "dk", "dv", "dbias"), f"attn_f32 + inverse rope hd {hd} T {T} {fam}")


def test_attention_f32_dbias_second_trip_of_the_column_sum(C):
    """B 65, T 1, H 1, head_dim 32: 260 partial rows per block of the bias gradient, more than
    the 256 threads of colsum_parts_f32_k take in one trip (explicit view strides for T = 1)."""
    c = F.ATTN32_MANY_ROWS
    ref, out = _run_attention(C, c["hd"], c["T"], True, "randn", rope=True, B=c["B"], H=c["H"])
    _assert_all(ref, out, ("o", "lse", "dq", "dk", "dv", "dbias"), "attn_f32 B 65 T 1")


# ---------------------------------------------------- shared kernels at fp32 storage ----

@pytest.mark.parametrize("M,F_", [(40, 64), (333, 1024)])
def test_swiglu_fp32_storage_bounds(C, M, F_):
    """(F 66 is not run: the binding takes F in multiples of the 4-element vector at fp32.)"""
    gu, dh = _randn(M, 2 * F_, seed=77), _randn(M, F_, seed=78)
    h = C.swiglu_fwd(gu)
    assert h.dtype == torch.float32
    hr, hu, _ = N.ref_swiglu_fwd(gu, bf16_out=False)
    N.assert_within(h, hr, hu, N.DERIVED, f"swiglu_fwd fp32 {M}x{F_}", {1: (1024, 4)})
    db = torch.full((2 * F_,), NAN, device=DEV)
    dgu = C.swiglu_bwd(dh, gu, db)
    ref, unit, _, dbr, dbu = N.ref_swiglu_bwd(dh.double(), gu, bf16_out=False)
    N.assert_within(dgu, ref, unit, N.DERIVED, f"swiglu_bwd fp32 {M}x{F_}", {1: (1024, 4)})
    N.assert_within(db, dbr, dbu, N.DERIVED, f"swiglu_bwd dbias fp32 {M}x{F_}")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_packed_qkv_fp32_storage_bounds(C, hd, inverse):
    M, H = 301, 3
    qkv = _randn(M, 3 * H * hd, seed=80)
    pos = torch.randint(0, 512, (M,), generator=_gen(81)).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    out = qkv.clone()
    C.rope_(out, pos, tab, 2 * H, hd, inverse)
    ref, rmag = N.ref_rope(qkv.double(), pos, tab, 2 * H, hd, inverse)
    unit = N.unit_rope(ref, rmag, out_bf16=False)
    unit[:, 2 * H * hd:] = 0                       # the v heads come out exact
    N.assert_within(out, ref, unit, N.DERIVED, f"rope_ fp32 hd {hd} inverse={inverse}")


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M,D", [(37, 768), (5, 8)])
def test_bias_residual_and_add_bias_fp32_storage_bounds(C, M, D, with_bias):
    y, res = _randn(M, D, seed=104), _randn(M, D, seed=105)
    b = _randn(D, seed=106) if with_bias else None
    ref, unit, _ = N.ref_bias_residual(y, b, res, bf16_out=False)
    got = C.bias_residual(y, b, res)
    assert got.dtype == torch.float32
    N.assert_within(got, ref, unit, N.DERIVED, f"bias_residual fp32 {M}x{D} bias={with_bias}")
    if with_bias:
        y2 = y.clone()
        assert C.add_bias_(y2, b).data_ptr() == y2.data_ptr()
        ref, unit, _ = N.ref_bias_residual(y, b, torch.zeros_like(y), bf16_out=False)
        N.assert_within(y2, ref, unit, N.DERIVED, f"add_bias_ fp32 {M}x{D}")


@pytest.mark.parametrize("with_bias", [True, False])
def test_add_rmsnorm_fwd_fp32_storage_bounds(C, with_bias):
    M, D = 37, 768
    y, res = _randn(M, D, seed=73), _randn(M, D, seed=74)
    b = _randn(D, seed=75) if with_bias else None
    w = (torch.rand(D, generator=_gen(76)) + 0.5).to(DEV)
    x, h, r = C.add_rmsnorm_fwd(y, b, res, w, 1e-5)
    assert x.dtype == h.dtype == torch.float32
    xr, xu, hr, hu, rr, ru = N.ref_add_rmsnorm_fwd(y, b, res, w, 1e-5, x_kernel=x, bf16_out=False)
    N.assert_within(x, xr, xu, N.DERIVED, f"add_rmsnorm_fwd fp32 x bias={with_bias}")
    N.assert_within(h, hr, hu, N.DERIVED, f"add_rmsnorm_fwd fp32 h bias={with_bias}")
    N.assert_within(r, rr, ru, N.DERIVED, f"add_rmsnorm_fwd fp32 rstd bias={with_bias}")


@pytest.mark.parametrize("D", [4, 260])
def test_embedding_bwd_sorted_fp32_dout_bounds(C, D):
    """fp32 dout: a 16-byte vector is one 4-column group.  Segments of 130, 8 and 5 rows across
    the 1024-token sort chunk, two shards, accumulate on and off; integer rows sum exactly."""
    M, v_local = 1025, 3
    g = _gen(120 + D + M + v_local)
    dout = torch.randn(M, D, generator=g).to(DEV)
    dint = torch.randint(-8, 9, (M, D), generator=g).to(DEV)
    acc0 = torch.randn(v_local, D, generator=g).to(DEV)
    aint = torch.randint(-8, 9, (v_local, D), generator=g).to(DEV)
    for start in (v_local, 2 * v_local):
        ids = N.emb_ids(M, v_local, start, 121 + M).to(DEV)
        keep = ids.clone()
        hit = (ids >= start) & (ids < start + v_local)
        want = torch.zeros(v_local, D, dtype=torch.int64, device=DEV).index_add_(0, (ids - start)[hit], dint[hit])
        for accumulate in (False, True):
            what = f"embedding_bwd_sorted fp32 D {D} start {start} accumulate={accumulate}"
            out = aint.float() if accumulate else torch.full((v_local, D), NAN, device=DEV)
            C.embedding_bwd_sorted(dint.float(), ids, v_local, start, out=out, accumulate=accumulate)
            assert torch.equal(out.long(), want + (aint if accumulate else 0)) and bool(torch.isfinite(out).all()), what
            out = acc0.clone() if accumulate else torch.full((v_local, D), NAN, device=DEV)
            C.embedding_bwd_sorted(dout, ids, v_local, start, out=out, accumulate=accumulate)
            ref, unit = N.ref_embedding_bwd(dout, ids, v_local, start, acc0 if accumulate else None)
            N.assert_within(out, ref, unit, N.DERIVED, what, {1: (256, 4)})
        assert torch.equal(ids, keep)


CE2_SHARDS = [(0, 1000), (1000, 997)]
CE2_CASES = [
    (65, 1000, CE2_SHARDS, False),           # two shards, 16-byte vectors of 4
    (65, 1003, [(0, 1003)], False),          # V % 4 != 0: the element-wise access path
    (65, 1002, [(0, 1002)], False),          # V % 8 != 0 but V % 2 == 0: element-wise at fp32 too
    (65, 1000, CE2_SHARDS, True),            # every target ignored
]


@pytest.mark.parametrize("M,V,shards,all_ignored", CE2_CASES)
def test_two_pass_ce_chain_fp32_logits_bounds(C, M, V, shards, all_ignored):
    """The chain the fp32 engine runs (ce_fused declines fp32 logits): ce_fwd_stats -> ce_finalize
    -> ce_grad_scale -> ce_bwd (+ dbias), every stage against the oracle of the stage before's
    own fp32 output; the gradient's store rounds to fp32."""
    logits, tgt = N.ce2_inputs(M, V, shards, DEV, all_ignored=all_ignored, dtype=torch.float32)
    assert C.ce_fused(logits[0].clone(), tgt, torch.zeros(M, device=DEV), 0, shards[0][1], None) is None
    stats = []
    for x, (st, va) in zip(logits, shards):
        s = C.ce_fwd_stats(x, tgt, st, va)
        ref, unit = N.ref_ce_stats(x, tgt, st, va)
        N.assert_within(s, ref, unit, N.DERIVED, f"ce_fwd_stats fp32 {M}x{V} shard at {st}")
        stats.append(s)
    stats = torch.stack(stats)
    acc = torch.full((2,), NAN, device=DEV)
    loss = torch.full((), NAN, device=DEV)
    lse, valid = C.ce_finalize(stats, tgt, -1, acc, loss, True, True)
    f = N.ref_ce_finalize(stats, tgt, -1)
    N.assert_within(lse, f["lse"], f["unit_lse"], N.DERIVED, f"ce_finalize lse fp32 {M}x{V}")
    assert torch.equal(valid.double(), f["valid"])
    n_valid = max(float(f["count"]), 1.0)
    run_sum, run_unit = float(f["loss_sum"]), float(f["unit_loss_sum"])
    assert float(acc[1]) == n_valid
    assert abs(float(acc[0]) - run_sum) <= N.DERIVED * run_unit
    assert abs(float(loss) - run_sum / n_valid) <= N.DERIVED * (run_unit / n_valid + N.U32 * abs(run_sum / n_valid))
    gs = C.ce_grad_scale(valid, torch.tensor(1.0, device=DEV), acc[1:2])
    gref = valid.double() / n_valid
    N.assert_within(gs, gref, 2 * N.U32 * gref, N.DERIVED, "ce_grad_scale")
    for x, (st, va) in zip(logits, shards):
        keep = x.clone()
        out = torch.full_like(x, NAN)
        db = torch.full((V,), NAN, device=DEV)
        C.ce_bwd(x, tgt, lse, gs, st, va, out, db)
        ref, unit, dbr, dbu = N.ref_ce_bwd(x, tgt, lse, gs, st, va, bf16_out=False)
        what = f"ce_bwd fp32 {M}x{V} shard at {st}"
        N.assert_within(out, ref, unit, N.DERIVED, what, {1: (128, 4)})
        N.assert_within(db, dbr, dbu, N.DERIVED, what + " dbias")
        assert torch.equal(x, keep)
        if all_ignored:
            assert float(loss) == 0 and not out.any() and not db.any() and n_valid == 1
