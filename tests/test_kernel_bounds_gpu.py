"""Per-element error bounds of the timed step's HIP kernels against fp64 oracles, on MI355X.

Every check is ``numerics.assert_within``: max over ALL elements of |out - ref| / unit, with the
fp64 oracle and the condition-aware unit of tests/numerics.py computed on the device.  Limits are
``numerics.DERIVED`` (1.01: the unit is a proven bound) or a ``numerics.LIMITS`` entry (2 x what
the rounding-emulating reference reaches on the CPU, tests/test_numerics.py); none comes from a
kernel's output.  Shapes are the smallest that reach each path of the kernels' tile geometry.
"""

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"
# gemm4.hip: workgroup tile 256 x 256 (256 x 192: variant 2), 128 x 128 / 128 x 96 per wave, 16-row MFMA blocks
GEMM_TILES = {0: (256, 128, 16), 1: (256, 192, 128, 96, 16)}
GEMM_SHAPES = [(257, 264, 96), (257, 264, 320), (130, 200, 160), (33, 200, 32), (520, 392, 128)]


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _randn(*shape, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def _stat_applies(M, Nn, K):
    # the bias statistic's restriction keeps > 90 % of the elements up to K = 96 (randn operands;
    # tests/test_numerics.py::test_bias_stat_restriction_drops_few_elements); n large enough to see 0.2 ulp
    return K <= 96 and M * Nn >= 50000


# ----------------------------------------------------------------------------- GEMM ----

# variants 0 (v4 at its own tile width) and 2 (v4 forced to 256 x 192) everywhere; 3 (the v3 kernel)
# once per layout as a second witness
NT_CASES = [(s, wb, v) for s in GEMM_SHAPES for wb in (True, False) for v in (0, 2)] + [(GEMM_SHAPES[1], True, 3)]
NN_CASES = [(s, v) for s in GEMM_SHAPES for v in (0, 2)] + [(GEMM_SHAPES[1], 3)]


@pytest.mark.parametrize("shape,with_bias,variant", NT_CASES)
def test_gemm_nt_bounds(C, shape, with_bias, variant):
    M, Nn, K = shape
    a, b = _randn(M, K, seed=1), _randn(Nn, K, seed=2)
    bias = _randn(Nn, seed=3, dtype=torch.float32) if with_bias else None
    out = C.gemm_nt(a, b, bias, variant=variant)
    ref, mag = N.ref_gemm(a, b, "nt", bias)
    what = f"gemm_nt {M}x{Nn}x{K} bias={with_bias} variant={variant}"
    N.assert_within(out, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, what, GEMM_TILES)
    if _stat_applies(M, Nn, K):
        N.bias_stat(out, ref, N.acc_term_gemm(mag, K), what)


@pytest.mark.parametrize("shape,variant", NN_CASES)
def test_gemm_nn_bounds(C, shape, variant):
    M, Nn, K = shape
    a, b = _randn(M, K, seed=4), _randn(K, Nn, seed=5)
    out = C.gemm_nn(a, b, variant=variant)
    ref, mag = N.ref_gemm(a, b, "nn")
    what = f"gemm_nn {M}x{Nn}x{K} variant={variant}"
    N.assert_within(out, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, what, GEMM_TILES)
    if _stat_applies(M, Nn, K):
        N.bias_stat(out, ref, N.acc_term_gemm(mag, K), what)


def _m8(M):
    return (M + 7) // 8 * 8      # the TN binding takes M, N in multiples of 8 (16-byte rows of a[K, M])


@pytest.mark.parametrize("m32", [1, 0])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("M,Nn,K", GEMM_SHAPES)
def test_gemm_tn_bounds(C, M, Nn, K, splits, m32):
    M = _m8(M)
    a, b = _randn(K, M, seed=6), _randn(K, Nn, seed=7)
    acc0 = _randn(M, Nn, seed=8, dtype=torch.float32)
    ref, mag = N.ref_gemm(a, b, "tn")
    ns = splits if splits else max(1, C.gemm_tn_splits(M, Nn, K))
    what = f"gemm_tn {M}x{Nn}x{K} splits={splits} m32={m32}"
    try:
        C.gemm4_m32(m32)
        C.gemm_force(-1, splits)
        out = C.gemm_tn(a, b)
        acc = acc0.clone()
        C.gemm_tn(a, b, acc, True)
        out3 = C.gemm_tn(a, b, variant=3) if (M, Nn, K) == (264, 264, 320) and m32 == 1 else None
    finally:
        C.gemm4_m32(1)
        C.gemm_force(-1, 0)
    assert out.dtype == torch.float32
    N.assert_within(out, ref, N.unit_gemm_f32(mag, K, ns), N.DERIVED, what, GEMM_TILES)
    N.assert_within(acc, ref + acc0.double(), N.unit_gemm_f32(mag, K, ns, acc0), N.DERIVED, what + " accumulate",
                    GEMM_TILES)
    if out3 is not None:   # v3 plans its own split count: at most one per 32-deep K stage
        N.assert_within(out3, ref, N.unit_gemm_f32(mag, K, max(ns, K // 32)), N.DERIVED, what + " v3", GEMM_TILES)


@pytest.mark.parametrize("M,Nn,K,heads,hd", [(300, 1152, 768, 12, 64), (130, 768, 64, 4, 128)])
def test_gemm_nt_rope_epilogue_bounds(C, M, Nn, K, heads, hd):
    """The RoPE epilogue rotates the fp32 accumulator (+ bias) and rounds once at the store."""
    a, b = _randn(M, K, seed=9), _randn(Nn, K, seed=10, scale=K ** -0.5)
    bias = _randn(Nn, seed=11, dtype=torch.float32)
    pos = torch.randint(0, 512, (M,), generator=torch.Generator().manual_seed(12)).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    out = C.gemm_nt(a, b, bias, pos, tab, heads, hd)
    lin, mag = N.ref_gemm(a, b, "nt", bias)
    ref, rmag = N.ref_rope(lin, pos, tab, heads, hd)
    acc = N.ref_rope(lin, pos, tab, heads, hd, mag=N.acc_term_gemm(mag, K))[1]
    unit = N.U16 * ref.abs() + acc + 3 * N.U32 * rmag
    N.assert_within(out, ref, unit, N.DERIVED, f"gemm_nt + rope hd {hd}", GEMM_TILES)


def _gu_perm(x):
    """Rows of a natural [gate | up] weight / bias interleaved in 64-blocks (the fused epilogue's order)."""
    n = x.size(0)
    return x.reshape([2, n // 128, 64] + list(x.shape[1:])).transpose(0, 1).reshape(x.shape)


@pytest.mark.parametrize("K", [96, 64, 192])
@pytest.mark.parametrize("F_", [128, 320])
def test_gemm_nt_swiglu_epilogue_bounds(C, F_, K):
    """K 64 / 192: the fused kernel (fewer stages than the ring / ring wrap).  It takes only the
    descriptor-advancing stream and declines K % 64 != 0; at K 96 the bound is checked on what the
    caller then runs: the GEMM on the interleaved weight + the interleaved SwiGLU pass."""
    M = 257
    x, w = _randn(M, K, seed=13, scale=0.25), _randn(2 * F_, K, seed=14, scale=0.25)
    b = _randn(2 * F_, seed=15, dtype=torch.float32)
    wp, bp = _gu_perm(w).contiguous(), _gu_perm(b).contiguous()
    r = C.gemm_nt_swiglu(x, w, b)
    if K % 64:
        assert len(r) == 0
        gu = C.gemm_nt(x, wp, bp)
        h = C.swiglu_fwd(gu, True)
    else:
        assert len(r) == 2, "fused kernel declined the shape"
        gu, h = r
    ref, mag = N.ref_gemm(x, wp, "nt", bp)
    N.assert_within(gu, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, f"swiglu epilogue gu F {F_} K {K}", GEMM_TILES)
    href, hunit, _ = N.ref_swiglu_fwd(gu, perm=True)     # h against the SwiGLU of the kernel's own gu
    N.assert_within(h, href, hunit, N.DERIVED, f"swiglu epilogue h F {F_} K {K}", {0: (256, 128, 16), 1: (128, 64)})


@pytest.mark.parametrize("perm", [True, False])
def test_gemm_nn_swiglu_bwd_epilogue_bounds(C, perm):
    M, F_, K = 257, 320, 64
    dy, w = _randn(M, K, seed=16, scale=0.25), _randn(K, F_, seed=17, scale=0.25)
    gu = _randn(M, 2 * F_, seed=18)
    db = torch.full((2 * F_,), float("nan"), device=DEV)
    r = C.gemm_nn_swiglu_bwd(dy, w, gu, db, perm)
    assert len(r) == 1, "fused kernel declined the shape"
    ds, mag = N.ref_gemm(dy, w, "nn")
    # the epilogue rounds dy w to bf16 (where the separate pass read it): that bound goes through the derivative
    ref, unit, _, dbr, dbu = N.ref_swiglu_bwd(ds, gu, perm, dh_unit=N.unit_gemm_bf16(ds, mag, K))
    N.assert_within(r[0], ref, unit, N.DERIVED, f"swiglu-bwd epilogue dgu perm={perm}", GEMM_TILES)
    N.assert_within(db, dbr, dbu, N.DERIVED, f"swiglu-bwd epilogue dbias perm={perm}")


def test_gemm_tn_group_and_tn2_bounds(C):
    K = 512
    shapes = [(136, 200), (264, 96)]
    A = [_randn(K, m, seed=20 + i) for i, (m, _) in enumerate(shapes)]
    B = [_randn(K, n, seed=30 + i) for i, (_, n) in enumerate(shapes)]
    outs = [_randn(m, n, seed=40 + i, dtype=torch.float32) for i, (m, n) in enumerate(shapes)]
    o0 = outs[0].clone()
    assert C.gemm_tn_group(A, B, outs, [1, 0])
    for i, (a, b, o) in enumerate(zip(A, B, outs)):
        ref, mag = N.ref_gemm(a, b, "tn", acc=o0 if i == 0 else None)
        unit = N.unit_gemm_f32(mag, K, K // 64, o0 if i == 0 else None)      # a split spans >= 64 rows
        N.assert_within(o, ref, unit, N.DERIVED, f"gemm_tn_group member {i}", GEMM_TILES)
    a1, b1 = _randn(K, 136, seed=50), _randn(K, 200, seed=51)
    for accumulate in (False, True):
        out = o0.clone()
        assert C.gemm_tn2(A[0], B[0], a1, b1, out, accumulate) is not None
        r0, m0 = N.ref_gemm(A[0], B[0], "tn")
        r1, m1 = N.ref_gemm(a1, b1, "tn")
        ref = r0 + r1 + (o0.double() if accumulate else 0)
        unit = N.unit_gemm_f32(m0 + m1, 2 * K, 2 * K // 64, o0 if accumulate else None)
        N.assert_within(out, ref, unit, N.DERIVED, f"gemm_tn2 accumulate={accumulate}", GEMM_TILES)


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("M,Nn,K", [(257, 264, 320), (520, 392, 96)])
def test_gemm_placement_exact(C, M, Nn, K, variant):
    """A holds one 1 per row at column pi(i), B distinct bf16-exact integers: every output
    element is one entry of B (+ an integer bias), so the result equals the gather exactly.  A
    tile written to the wrong place, a dropped or doubled K step, a transposed store all show."""
    g = torch.Generator().manual_seed(60)
    pi = torch.randint(0, K, (M,), generator=g).to(DEV)
    a = torch.zeros(M, K, device=DEV)
    a[torch.arange(M, device=DEV), pi] = 1
    a = a.bfloat16()
    bt = (torch.arange(Nn * K, device=DEV, dtype=torch.float32).view(Nn, K) % 251).bfloat16()     # NT: b[N, K]
    bn = (torch.arange(K * Nn, device=DEV, dtype=torch.float32).view(K, Nn) % 251).bfloat16()     # NN: b[K, N]
    bias = (torch.arange(Nn, device=DEV) % 5).float()
    assert torch.equal(C.gemm_nt(a, bt, None, variant=variant).float(), bt.float()[:, pi].t())
    assert torch.equal(C.gemm_nt(a, bt, bias, variant=variant).float(), bt.float()[:, pi].t() + bias)
    assert torch.equal(C.gemm_nn(a, bn, variant=variant).float(), bn.float()[pi])
    if variant == 0:      # TN (fp32 out): a^T[M8, K] given as a[K, M8], one 1 per COLUMN of a
        M8 = _m8(M)
        pi8 = torch.randint(0, K, (M8,), generator=g).to(DEV)
        at = torch.zeros(K, M8, device=DEV)
        at[pi8, torch.arange(M8, device=DEV)] = 1
        at = at.bfloat16()
        try:
            for splits in (0, 3):
                C.gemm_force(-1, splits)
                assert torch.equal(C.gemm_tn(at, bn), bn.float()[pi8]), f"TN splits={splits}"
        finally:
            C.gemm_force(-1, 0)


# ------------------------------------------------------------------------ attention ----

def _run_attention(C, hd, T, causal, fam, rope=False):
    q, k, v, do, pos = N.attn_inputs(hd, T, fam, DEV)
    B, _, H, _ = q.shape
    scale = hd ** -0.5
    tab = N.rope_table(512, hd).to(DEV) if rope else None
    ref = N.attn_refs(q, k, v, do, scale, causal, pos if rope else None, tab)
    o, lse = C.attn_fwd(q, k, v, scale, causal)
    d = torch.full((B * T, 3 * H * hd), float("nan"), device=DEV, dtype=torch.bfloat16)   # unwritten elements show
    dq, dk, dv = N.packed_views(d, B, T, H, hd)
    out = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    if rope:
        db = torch.full((3 * H * hd,), float("nan"), device=DEV)
        assert C.attn_bwd(do, q, k, v, o, lse, scale, causal, dq, dk, dv, pos, tab, dbias=db)
        out["dbias"] = db
    else:
        C.attn_bwd(do, q, k, v, o, lse, scale, causal, dq, dk, dv)
    return ref, out


@pytest.mark.parametrize("fam", list(N.ATTN_FAMILIES))
@pytest.mark.parametrize("hd,T,causal", N.ATTN_CASES)
def test_attention_bounds(C, hd, T, causal, fam):
    """The default kernels (hd 64 / 128: the 32x32x16 forward and backward pair; hd 32: the
    16x16x32 kernels) on packed-QKV views: partial single tiles (T 1, 17, 63), one key past a
    tile (65), an unpaired query block (129, 300, 385), ragged last blocks, causal and not, flat
    and near one-hot softmax rows."""
    ref, out = _run_attention(C, hd, T, causal, fam)
    for name in ("o", "lse", "dq", "dk", "dv"):
        N.assert_within(out[name], ref[name], ref["unit_" + name], N.limit(N.attn_key(name, hd)),
                        f"attn {name} hd {hd} T {T} causal={causal} {fam}", N.ATTN_TILES[name])


@pytest.mark.parametrize("fam", list(N.ATTN_FAMILIES))
@pytest.mark.parametrize("hd,T", N.ATTN_ROPE_CASES)
def test_attention_bwd_rope_dbias_bounds(C, hd, T, fam):
    ref, out = _run_attention(C, hd, T, True, fam, rope=True)
    for name in ("dq", "dk", "dbias"):
        N.assert_within(out[name], ref[name], ref["unit_" + name], N.limit(N.attn_key(name, hd, True)),
                        f"attn {name} + inverse rope hd {hd} T {T} {fam}", N.ATTN_TILES[name])
    N.assert_within(out["dv"], ref["dv"], ref["unit_dv"], N.limit(N.attn_key("dv", hd)), f"attn dv hd {hd} T {T} {fam}",
                    N.ATTN_TILES["dv"])


# ------------------------------------------------------------ norms, elementwise, CE ----

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,D", [(37, 768), (5, 5120), (64, 128)])
def test_rmsnorm_bounds(C, dt, M, D):
    x, dy = _randn(M, D, seed=70, dtype=dt), _randn(M, D, seed=71, dtype=dt)
    w = (torch.rand(D, generator=torch.Generator().manual_seed(72)) + 0.5).to(DEV)
    bf = dt == torch.bfloat16
    y, rstd = C.rmsnorm_fwd(x, w, 1e-5)
    yr, yu, rr, ru = N.ref_rmsnorm_fwd(x, w, 1e-5, bf)
    N.assert_within(y, yr, yu, N.DERIVED, f"rmsnorm_fwd y {M}x{D} {dt}")
    N.assert_within(rstd, rr, ru, N.DERIVED, f"rmsnorm_fwd rstd {M}x{D} {dt}")
    dx, dw = C.rmsnorm_bwd(dy, x, w, rstd)
    dxr, dxu, dwr, dwu = N.ref_rmsnorm_bwd(dy, x, w, 1e-5, None, bf)
    N.assert_within(dx, dxr, dxu, N.DERIVED, f"rmsnorm_bwd dx {M}x{D} {dt}")
    N.assert_within(dw, dwr, dwu, N.DERIVED, f"rmsnorm_bwd dw {M}x{D} {dt}")


@pytest.mark.parametrize("with_bias", [True, False])
def test_add_rmsnorm_fwd_bounds(C, with_bias):
    M, D = 37, 768
    y, res = _randn(M, D, seed=73), _randn(M, D, seed=74)
    b = _randn(D, seed=75, dtype=torch.float32) if with_bias else None
    w = (torch.rand(D, generator=torch.Generator().manual_seed(76)) + 0.5).to(DEV)
    x, h, r = C.add_rmsnorm_fwd(y, b, res, w, 1e-5)
    xr, xu, hr, hu, rr, ru = N.ref_add_rmsnorm_fwd(y, b, res, w, 1e-5, x_kernel=x)   # the norm of the kernel's own x
    N.assert_within(x, xr, xu, N.DERIVED, f"add_rmsnorm_fwd x bias={with_bias}")
    N.assert_within(h, hr, hu, N.DERIVED, f"add_rmsnorm_fwd h bias={with_bias}")
    N.assert_within(r, rr, ru, N.DERIVED, f"add_rmsnorm_fwd rstd bias={with_bias}")


@pytest.mark.parametrize("M,F_", [(40, 64), (333, 1024)])
def test_swiglu_bounds(C, M, F_):
    gu, dh = _randn(M, 2 * F_, seed=77), _randn(M, F_, seed=78)
    h = C.swiglu_fwd(gu)
    hr, hu, hacc = N.ref_swiglu_fwd(gu)
    N.assert_within(h, hr, hu, N.DERIVED, f"swiglu_fwd {M}x{F_}")
    db = torch.full((2 * F_,), float("nan"), device=DEV)
    dgu = C.swiglu_bwd(dh, gu, db)
    ref, unit, acc, dbr, dbu = N.ref_swiglu_bwd(dh.double(), gu)
    N.assert_within(dgu, ref, unit, N.DERIVED, f"swiglu_bwd {M}x{F_}")
    N.assert_within(db, dbr, dbu, N.DERIVED, f"swiglu_bwd dbias {M}x{F_}")
    if M * F_ >= 50000:
        N.bias_stat(h, hr, hacc, f"swiglu_fwd {M}x{F_}")
        N.bias_stat(dgu, ref, acc, f"swiglu_bwd {M}x{F_}")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_packed_qkv_bounds(C, hd, inverse):
    """rope_ on packed QKV rows (the unfused form of the QKV epilogue's rotation): q and k heads
    rotated by their row's position, v heads untouched (unit 0 there: exact)."""
    M, H = 301, 3
    qkv = _randn(M, 3 * H * hd, seed=80)
    pos = torch.randint(0, 512, (M,), generator=torch.Generator().manual_seed(81)).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    out = qkv.clone()
    C.rope_(out, pos, tab, 2 * H, hd, inverse)
    ref, rmag = N.ref_rope(qkv.double(), pos, tab, 2 * H, hd, inverse)
    unit = N.unit_rope(ref, rmag)
    unit[:, 2 * H * hd:] = 0
    # (no bias statistic: at small angles x cos - x' sin of a bf16 x rounds back to x itself, so the
    # rounding error of a correct kernel is not uniform on +-1/2 ulp)
    N.assert_within(out, ref, unit, N.DERIVED, f"rope_ hd {hd} inverse={inverse}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,V,valid", N.CE_CASES)
def test_ce_fused_bounds(C, M, V, valid, bias):
    logits, tgt, gs = N.ce_inputs(M, V, valid, DEV)
    assert (tgt == -1).any()
    ref = N.ref_ce_fused(logits, tgt, gs, valid)
    x = logits.clone()
    db = torch.full((V,), float("nan"), device=DEV) if bias else None
    st = C.ce_fused(x, tgt, gs, 0, valid, db)
    assert st is not None
    N.assert_within(x, ref["grad"], ref["unit_grad"], N.limit("ce.grad"), f"ce_fused d logits {M}x{V}", {1: (4096, 8)})
    N.assert_within(st, ref["stats"], ref["unit_stats"], N.DERIVED, f"ce_fused loss statistics {M}x{V}")
    if bias:
        N.assert_within(db, ref["dbias"], ref["unit_dbias"], N.limit("ce.dbias"), f"ce_fused dbias {M}x{V}")
