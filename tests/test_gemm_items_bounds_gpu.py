"""Per-element fp64 bounds of the v4 GEMM family with SEVERAL ITEMS PER WORKGROUP, on MI355X.

``gemm4_k`` is persistent: min(items, CU count) workgroups walk their items ``it, it + G, ...``
with the DMA producer three steps ahead across item boundaries.  The cases of
tests/test_kernel_bounds_gpu.py have at most 12 items, so every workgroup they launch runs one.
Here every case is sized from the device's CU count through the mirror of the item order
(tests/numerics_items.py) and asserts from it that some workgroup runs three items and some
fewer than the most (the tail); the failure message names the worst element's item, workgroup
and round.  K is the smallest that reaches each DMA stream (the item count needs rows and
columns, not depth): 32 = per-lane checked, two steps of which one reads zeros; 64 = the
descriptor-advancing FAST stream, two steps; 96 = checked, four steps; 160 = checked, six.

Every limit is ``numerics.DERIVED``; outputs of up to 35 M elements are judged in row slabs
against the fp64 oracle on the device.  The K-split cases force odd split counts S: the TN and
bf16 split-K launchers round the split length up to 64, so K = 32 S and 96 S run splits of 64 and
128 rows through the checked stream with the trailing splits empty (items whose every DMA is out
of range), K = 64 S whole 64-row splits through FAST, K = 64 S - 40 a ragged last split.
"""

import pytest
import torch

import numerics as N
import numerics_items as I

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"
TILES = {0: (256, 128, 16), 1: (256, 192, 128, 96, 16)}
R = I.rounds_wanted()


@pytest.fixture(scope="module")
def C():
    return _ext.require()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _randn(*shape, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def _odd(s):
    return s | 1


def _gemm_rows(out, a, b, layout, bias, unit_of, what, items, bn):
    """assert_within over row slabs of a bf16 NT / NN output: unit_of(ref, mag) -> unit."""
    def slab(r0, r1):
        ref, mag = N.ref_gemm(a[r0:r1], b, layout, bias)
        return ref, unit_of(ref, mag)
    return I.assert_within_rows(out, slab, N.DERIVED, what, TILES, items, bn)


def _plain_items(M, Nn, cus, variant, what):
    bn = I.pick_bn(M, Nn, cus, variant)
    items = I.launch_order(M, Nn, bn, 1, cus)
    I.assert_rounds(items, R, what)
    return items, bn


# ------------------------------------------------------------------- plain NT / NN ----

PLAIN = [(v, K) for v in (0, 2, 4) for K in (32, 64, 96)] + [(0, 160)]


def _third_round_stat(out, a, b, bias, K, items, bn, what):
    """numerics.bias_stat on the elements of third-round (and later) items, subsampled with a
    fixed stride to at most 2^18 (the six-sigma bound assumes independent rounding errors;
    tests/test_numerics.py shows a correct rounding inside it at such n, not at 3e7)."""
    M, Nn = out.shape
    mask = torch.zeros(M, Nn, dtype=torch.bool, device=DEV)
    for r in range(2, max(it.round for it in items) + 1):
        mask |= I.round_mask(M, Nn, items, bn, r, DEV)
    o, rf, ac = [], [], []
    for r0 in range(0, M, 2048):
        sel = mask[r0:r0 + 2048]
        ref, mag = N.ref_gemm(a[r0:r0 + 2048], b, "nt", bias)
        o.append(out[r0:r0 + 2048][sel])
        rf.append(ref[sel])
        ac.append(N.acc_term_gemm(mag, K)[sel])
    o, rf, ac = torch.cat(o), torch.cat(rf), torch.cat(ac)
    step = I.cdiv(o.numel(), 2 ** 18)
    assert o.numel() // step >= 50000, f"{what}: {o.numel()} third-round elements"
    N.bias_stat(o[::step], rf[::step], ac[::step], what + " third-round items")


@pytest.mark.parametrize("variant,K", PLAIN)
def test_gemm_nt_items_bounds(C, cus, variant, K):
    M, Nn = I.shape_for(R, cus)
    what = f"items gemm_nt {M}x{Nn}x{K} variant={variant}"
    items, bn = _plain_items(M, Nn, cus, variant, what)
    a, b = _randn(M, K, seed=101), _randn(Nn, K, seed=102)
    bias = _randn(Nn, seed=103, dtype=torch.float32)
    out = C.gemm_nt(a, b, bias, variant=variant)
    _gemm_rows(out, a, b, "nt", bias, lambda ref, mag: N.unit_gemm_bf16(ref, mag, K), what, items, bn)
    if variant == 0 and K in (32, 64):
        _third_round_stat(out, a, b, bias, K, items, bn, what)


@pytest.mark.parametrize("variant,K", PLAIN)
def test_gemm_nn_items_bounds(C, cus, variant, K):
    M, Nn = I.shape_for(R, cus)
    what = f"items gemm_nn {M}x{Nn}x{K} variant={variant}"
    items, bn = _plain_items(M, Nn, cus, variant, what)
    a, b = _randn(M, K, seed=104), _randn(K, Nn, seed=105)
    out = C.gemm_nn(a, b, variant=variant)
    _gemm_rows(out, a, b, "nn", None, lambda ref, mag: N.unit_gemm_bf16(ref, mag, K), what, items, bn)


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_gemm_items_256_wide_bounds(C, cus, layout):
    """At shape_for's smallest shape the launcher's round model picks 192-wide tiles for variant 0;
    this is the smallest three-round shape at which it picks 256 (the plain 256-wide form)."""
    M, Nn = I.shape_for(R, cus, bn=256)
    K = 64
    what = f"items gemm_{layout} {M}x{Nn}x{K} 256-wide"
    items, bn = _plain_items(M, Nn, cus, 0, what)
    assert bn == 256
    a = _randn(M, K, seed=106)
    b = _randn(Nn, K, seed=107) if layout == "nt" else _randn(K, Nn, seed=107)
    bias = _randn(Nn, seed=108, dtype=torch.float32) if layout == "nt" else None
    out = C.gemm_nt(a, b, bias) if layout == "nt" else C.gemm_nn(a, b)
    _gemm_rows(out, a, b, layout, bias, lambda ref, mag: N.unit_gemm_bf16(ref, mag, K), what, items, bn)


def test_gemm_nt_items_no_bias_bounds(C, cus):
    """HAS_BIAS is a template flag: the other instantiation over three rounds."""
    M, Nn = I.shape_for(R, cus)
    K = 64
    what = f"items gemm_nt {M}x{Nn}x{K} no bias"
    items, bn = _plain_items(M, Nn, cus, 0, what)
    a, b = _randn(M, K, seed=109), _randn(Nn, K, seed=110)
    _gemm_rows(C.gemm_nt(a, b, None), a, b, "nt", None, lambda ref, mag: N.unit_gemm_bf16(ref, mag, K), what, items, bn)


@pytest.mark.parametrize("variant,K", [(0, 32), (0, 64), (2, 96), (4, 64)])
def test_gemm_nt_items_bias_alone_exact(C, cus, variant, K):
    """a = [v | -v], b = [w | w] in small integers: every partial sum is exact and every row's
    products sum to zero, so each output element must equal its own column's bias, arange(N) % 7,
    exactly.  A bias area that still holds the previous item's values fails by name."""
    M, Nn = I.shape_for(R, cus)
    what = f"items gemm_nt bias alone {M}x{Nn}x{K} variant={variant}"
    items, bn = _plain_items(M, Nn, cus, variant, what)
    g = torch.Generator(device=DEV).manual_seed(111)
    v = torch.randint(-4, 5, (M, K // 2), generator=g, device=DEV).float()
    w = torch.randint(-4, 5, (Nn, K // 2), generator=g, device=DEV).float()
    a, b = torch.cat([v, -v], 1).bfloat16(), torch.cat([w, w], 1).bfloat16()
    bias = (torch.arange(Nn, device=DEV) % 7).float()
    out = C.gemm_nt(a, b, bias, variant=variant)
    _exact(out, bias.expand(M, Nn), what, items, bn)


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_gemm_items_v3_witness_bounds(C, cus, layout):
    """The v3 kernel (variant 3) at the same shape: the second witness of the oracle and units."""
    M, Nn = I.shape_for(R, cus)
    K = 64
    a = _randn(M, K, seed=112)
    b = _randn(Nn, K, seed=113) if layout == "nt" else _randn(K, Nn, seed=113)
    bias = _randn(Nn, seed=114, dtype=torch.float32) if layout == "nt" else None
    out = C.gemm_nt(a, b, bias, variant=3) if layout == "nt" else C.gemm_nn(a, b, variant=3)
    _gemm_rows(out, a, b, layout, bias, lambda ref, mag: N.unit_gemm_bf16(ref, mag, K),
               f"items gemm_{layout} {M}x{Nn}x{K} v3", None, 256)


# ------------------------------------------------------------------ fused epilogues ----

@pytest.mark.parametrize("K", [64, 96])
@pytest.mark.parametrize("H,hd", [(4, 128), (4, 64)])
def test_gemm_nt_rope_epilogue_items_bounds(C, cus, H, hd, K):
    """Positions are random in [0, 512): a row rotated by the previous item's positions shows."""
    Nn = 3 * H * hd
    M = I.m_for(R, cus, Nn // 256)
    what = f"items gemm_nt + rope hd {hd} {M}x{Nn}x{K}"
    items = I.launch_order(M, Nn, 256, 1, cus)      # (the RoPE epilogue runs 256-wide tiles only)
    I.assert_rounds(items, R, what)
    a, b = _randn(M, K, seed=115), _randn(Nn, K, seed=116, scale=K ** -0.5)
    bias = _randn(Nn, seed=117, dtype=torch.float32)
    pos = torch.randint(0, 512, (M,), generator=torch.Generator().manual_seed(118)).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    out = C.gemm_nt(a, b, bias, pos, tab, 2 * H, hd)

    def slab(r0, r1):
        lin, mag = N.ref_gemm(a[r0:r1], b, "nt", bias)
        ref, rmag = N.ref_rope(lin, pos[r0:r1], tab, 2 * H, hd)
        acc = N.ref_rope(lin, pos[r0:r1], tab, 2 * H, hd, mag=N.acc_term_gemm(mag, K))[1]
        return ref, N.U16 * ref.abs() + acc + 3 * N.U32 * rmag
    I.assert_within_rows(out, slab, N.DERIVED, what, TILES, items, 256)


def _gu_perm(x):
    n = x.size(0)
    return x.reshape([2, n // 128, 64] + list(x.shape[1:])).transpose(0, 1).reshape(x.shape)


@pytest.mark.parametrize("K", [64, 192])
def test_gemm_nt_swiglu_epilogue_items_bounds(C, cus, K):
    F_ = 640
    M = I.m_for(R, cus, 2 * F_ // 256)
    what = f"items swiglu epilogue F {F_} {M}x{2 * F_}x{K}"
    items = I.launch_order(M, 2 * F_, 256, 1, cus)
    I.assert_rounds(items, R, what)
    x, w = _randn(M, K, seed=119, scale=0.25), _randn(2 * F_, K, seed=120, scale=0.25)
    b = _randn(2 * F_, seed=121, dtype=torch.float32)
    wp, bp = _gu_perm(w).contiguous(), _gu_perm(b).contiguous()
    r = C.gemm_nt_swiglu(x, w, b)
    assert len(r) == 2, "fused kernel declined the shape"
    gu, h = r
    _gemm_rows(gu, x, wp, "nt", bp, lambda ref, mag: N.unit_gemm_bf16(ref, mag, K), what + " gu", items, 256)
    # h against the SwiGLU of the kernel's own gu; an h tile is 128 wide (its item's 256 gu columns)
    items_h = [it._replace(n0=it.n0 // 2) for it in items]
    I.assert_within_rows(h, lambda r0, r1: N.ref_swiglu_fwd(gu[r0:r1], perm=True)[:2], N.DERIVED, what + " h",
                         {0: (256, 128, 16), 1: (128, 64)}, items_h, 128)


@pytest.mark.parametrize("depth", [2, 1])
@pytest.mark.parametrize("perm", [True, False])
def test_gemm_nn_swiglu_bwd_epilogue_items_bounds(C, cus, perm, depth):
    """dbias sums the partial column sums of every row tile: three rounds of them here."""
    F_, K = 640, 64
    M = I.m_for(R, cus, I.cdiv(F_, 256))
    what = f"items swiglu-bwd epilogue {M}x{F_}x{K} perm={perm} depth={depth}"
    items = I.launch_order(M, F_, 256, 1, cus)
    I.assert_rounds(items, R, what)
    dy, w = _randn(M, K, seed=122, scale=0.25), _randn(K, F_, seed=123, scale=0.25)
    gu = _randn(M, 2 * F_, seed=124)
    db = torch.full((2 * F_,), float("nan"), device=DEV)
    try:
        C.gemm4_swb_depth(depth)
        r = C.gemm_nn_swiglu_bwd(dy, w, gu, db, perm)
    finally:
        C.gemm4_swb_depth(2)
    assert len(r) == 1, "fused kernel declined the shape"
    sums = [torch.zeros(2 * F_, dtype=torch.float64, device=DEV) for _ in range(3)]

    def slab(r0, r1):
        ds, mag = N.ref_gemm(dy[r0:r1], w, "nn")
        ref, unit = N.ref_swiglu_bwd(ds, gu[r0:r1], perm, dh_unit=N.unit_gemm_bf16(ds, mag, K))[:2]
        sums[0] += ref.sum(0)
        sums[1] += unit.sum(0)
        sums[2] += ref.abs().sum(0)
        return ref, unit
    # dgu [M, 2F] natural [gate | up]: column j and column F + j come from the item of dh column j
    I.assert_within_rows(r[0][:, :F_], lambda r0, r1: tuple(t[:, :F_] for t in slab(r0, r1)), N.DERIVED,
                         what + " d gate", TILES, items, 256)
    I.assert_within_rows(r[0][:, F_:], lambda r0, r1: tuple(t[:, F_:] for t in slab(r0, r1)), N.DERIVED,
                         what + " d up", TILES, items, 256)
    # (both halves walked every slab: the sums hold each twice) ref_swiglu_bwd's dbias unit over all M rows
    dbr, dbu = sums[0] / 2, sums[1] / 2 + (M + 1) * N.U32 * sums[2] / 2
    N.assert_within(db, dbr, dbu, N.DERIVED, what + " dbias")


# ------------------------------------------------------------------------ TN, split-K ----

def _tn_case(cus):
    S = _odd(I.forced_splits(R, cus, 4))
    return 264, 264, S


@pytest.mark.parametrize("m32", [1, 0])
@pytest.mark.parametrize("kmul,kadd", [(32, 0), (64, 0), (96, 0), (64, -40)])
def test_gemm_tn_items_bounds(C, cus, kmul, kadd, m32):
    """Four tiles x S forced splits: every workgroup's items are K splits of the same few tiles."""
    M, Nn, S = _tn_case(cus)
    K = kmul * S + kadd
    what = f"items gemm_tn {M}x{Nn}x{K} splits={S} m32={m32}"
    a, b = _randn(K, M, seed=125), _randn(K, Nn, seed=126)
    acc0 = _randn(M, Nn, seed=127, dtype=torch.float32)
    try:
        C.gemm4_m32(m32)
        C.gemm_force(-1, S)
        assert C.gemm_tn_splits(M, Nn, K) == S
        out = C.gemm_tn(a, b)
        acc = acc0.clone()
        C.gemm_tn(a, b, acc, True)
    finally:
        C.gemm4_m32(1)
        C.gemm_force(-1, 0)
    items = I.launch_order(M, Nn, 256, S, cus)
    I.assert_rounds(items, R, what)
    ref, mag = N.ref_gemm(a, b, "tn")
    where = I.locator(items, 256)
    N.assert_within(out, ref, N.unit_gemm_f32(mag, K, S), N.DERIVED, what, TILES, where=where)
    N.assert_within(acc, ref + acc0.double(), N.unit_gemm_f32(mag, K, S, acc0), N.DERIVED, what + " accumulate", TILES,
                    where=where)


@pytest.mark.parametrize("layout,with_bias", [("nt", True), ("nt", False), ("nn", False)])
def test_gemm_bf16_splitk_items_bounds(C, cus, layout, with_bias):
    """The bf16 split-K slab path (fp32 slabs from gemm4_k, splitk_reduce_bf16_k: + bias, one rounding)."""
    M, Nn = 520, 392
    S = _odd(I.forced_splits(R, cus, 6))
    K = 64 * S
    what = f"items bf16 split-K gemm_{layout} {M}x{Nn}x{K} splits={S} bias={with_bias}"
    items = I.launch_order(M, Nn, 256, S, cus)
    I.assert_rounds(items, R, what)
    a = _randn(M, K, seed=128)
    b = _randn(Nn, K, seed=129) if layout == "nt" else _randn(K, Nn, seed=129)
    bias = _randn(Nn, seed=130, dtype=torch.float32) if with_bias else None
    try:
        C.gemm_force(-1, S)
        out = C.gemm_nt(a, b, bias) if layout == "nt" else C.gemm_nn(a, b)
    finally:
        C.gemm_force(-1, 0)
    ref, mag = N.ref_gemm(a, b, layout, bias)
    N.assert_within(out, ref, I.unit_splitk_bf16(ref, mag, K, S), N.DERIVED, what, TILES, where=I.locator(items, 256))


def test_gemm_bf16_splitk_rope_after_items_bounds(C, cus):
    """Split-K with RoPE: the rotation is a second pass over the already rounded output
    (dpfs_rope_after_gemm), so the first rounding goes through the rotation."""
    M, H, hd = 520, 4, 64
    Nn = 3 * H * hd
    S = _odd(I.forced_splits(R, cus, 3 * (Nn // 256)))
    K = 64 * S
    what = f"items bf16 split-K gemm_nt + rope after {M}x{Nn}x{K} splits={S}"
    items = I.launch_order(M, Nn, 256, S, cus)
    I.assert_rounds(items, R, what)
    a, b = _randn(M, K, seed=131), _randn(Nn, K, seed=132, scale=K ** -0.5)
    bias = _randn(Nn, seed=133, dtype=torch.float32)
    pos = torch.randint(0, 512, (M,), generator=torch.Generator().manual_seed(134)).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    try:
        C.gemm_force(-1, S)
        out = C.gemm_nt(a, b, bias, pos, tab, 2 * H, hd)
    finally:
        C.gemm_force(-1, 0)
    lin, mag = N.ref_gemm(a, b, "nt", bias)
    ref, unit = I.unit_rope_two_pass(lin, N.unit_gemm_f32(mag, K, S), pos, tab, 2 * H, hd)
    N.assert_within(out, ref, unit, N.DERIVED, what, TILES, where=I.locator(items, 256))


# ------------------------------------------------------------------------ grouped TN ----

GROUP_SHAPES = [(2824, 2568), (2832, 2576), (3072, 2816), (2824, 2600)]     # 12 x 11 tiles each
GROUP_SENTINEL = -7.0


def _group_outs(shapes, acc, seed):
    """The members' outputs as views of one sentinel-filled flat buffer, 64 sentinels around each."""
    pad = 64
    total = sum(m * n + pad for m, n in shapes) + pad
    buf = torch.full((total,), GROUP_SENTINEL, device=DEV)
    outs, inits, mask, off = [], [], torch.ones(total, dtype=torch.bool, device=DEV), pad
    for i, ((m, n), ac) in enumerate(zip(shapes, acc)):
        v = buf[off:off + m * n].view(m, n)
        v.copy_(_randn(m, n, seed=seed + i, dtype=torch.float32) if ac else torch.full((m, n), float("nan"), device=DEV))
        mask[off:off + m * n] = False
        outs.append(v)
        inits.append(v.clone() if ac else None)
        off += m * n + pad
    return buf, mask, outs, inits


@pytest.mark.parametrize("br_tn", [0, 2])
@pytest.mark.parametrize("K0,K1", [(512, 0), (512, 256)])
def test_gemm_tn_group_items_bounds(C, cus, K0, K1, br_tn):
    """Four members whose tiles alone exceed two rounds of the CUs (whatever split count the plan
    picks, a workgroup runs three items and crosses member boundaries); K 512 in one buffer (the
    plan's single split), K0 512 + K1 256 in two (one split per buffer)."""
    acc = [1, 0, 1, 0]
    what = f"items gemm_tn_group K {K0}+{K1} br_tn={br_tn}"
    S = 1 if K1 == 0 else 2
    items, _ = I.group_order(GROUP_SHAPES, S, cus)
    assert len(I.group_order(GROUP_SHAPES, 1, cus)[0]) > 2 * cus
    I.assert_rounds(items, R, what)
    A = [_randn(K0, m, seed=140 + i) for i, (m, _) in enumerate(GROUP_SHAPES)]
    B = [_randn(K0, n, seed=150 + i) for i, (_, n) in enumerate(GROUP_SHAPES)]
    A2 = [_randn(K1, m, seed=160 + i) for i, (m, _) in enumerate(GROUP_SHAPES)] if K1 else None
    B2 = [_randn(K1, n, seed=170 + i) for i, (_, n) in enumerate(GROUP_SHAPES)] if K1 else None
    buf, mask, outs, inits = _group_outs(GROUP_SHAPES, acc, 180)
    try:
        C.gemm4_br_tn(br_tn)
        assert C.gemm_tn_group(A, B, outs, acc, A2, B2)
    finally:
        C.gemm4_br_tn(0)
    assert bool((buf[mask] == GROUP_SENTINEL).all()), what + ": sentinel padding overwritten"
    K = K0 + K1
    for g in range(4):
        ref, mag = N.ref_gemm(A[g], B[g], "tn", acc=inits[g])
        if K1:
            r1, m1 = N.ref_gemm(A2[g], B2[g], "tn")
            ref, mag = ref + r1, mag + m1
        mine = [it for it in items if it.g == g]
        N.assert_within(outs[g], ref, N.unit_gemm_f32(mag, K, K // 64, inits[g]), N.DERIVED, f"{what} member {g}",
                        TILES, where=I.locator(mine, 256))


# -------------------------------------------------------------------------- stream-K ----

@pytest.mark.parametrize("variant", [8, 12])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_gemm_stream_k_bounds(C, cus, layout, K, variant):
    """1.5 tiles per CU: every workgroup runs a whole tile and one K half of an extra tile; the
    consumer half adds the producer's fp32 partial per 16-row block.  K 128 / 384: an even and an
    odd number of 64-deep stages per half."""
    M, Nn = I.sk_shape(cus)
    if not C.gemm_sk_applies(M, Nn, K):
        pytest.skip(f"stream-K does not apply to {M}x{Nn}x{K} on {cus} CUs")
    what = f"stream-K gemm_{layout} {M}x{Nn}x{K} variant={variant}"
    items = I.sk_order(M, Nn, cus)
    roles = [sum(it.role == r for it in items) for r in range(3)]
    assert roles == [cus, cus // 2, cus // 2] and all(len(v) == 2 for v in I.per_workgroup(items).values())
    a = _randn(M, K, seed=190)
    b = _randn(Nn, K, seed=191) if layout == "nt" else _randn(K, Nn, seed=191)
    bias = _randn(Nn, seed=192, dtype=torch.float32) if layout == "nt" else None
    run = (lambda: C.gemm_nt(a, b, bias, variant=variant)) if layout == "nt" else (lambda: C.gemm_nn(a, b, variant=variant))
    C.gemm_sk_error(True)
    out = run()
    again = run()
    torch.cuda.synchronize()
    assert C.gemm_sk_error(False) == 0, what + ": a consumer's wait for its partial timed out"
    _gemm_rows(out, a, b, layout, bias, lambda ref, mag: I.unit_gemm_sk(ref, mag, K), what, items, 256)
    assert torch.equal(out, again), what + ": a second launch differs"


# ------------------------------------------------------------------- exact placement ----

def _one_hot_rows(M, K, g):
    pi = torch.randint(0, K, (M,), generator=g, device=DEV)
    a = torch.zeros(M, K, device=DEV)
    a[torch.arange(M, device=DEV), pi] = 1
    return a.bfloat16(), pi


def _ints(rows, cols):
    return (torch.arange(rows * cols, device=DEV, dtype=torch.float32).view(rows, cols) % 251).bfloat16()


def _exact(out, ref, what, items, bn=256):
    """Every element equal to ``ref`` (unit 0), judged in row slabs; the failure names the item."""
    def slab(r0, r1):
        r = ref[r0:r1].double()
        return r, torch.zeros_like(r)
    I.assert_within_rows(out, slab, N.DERIVED, what, TILES, items, bn)


@pytest.mark.parametrize("group_m", [4, 1, 8])
def test_gemm_placement_exact_items(C, cus, group_m):
    """test_gemm_placement_exact's construction over three rounds (one 1 per row of A, distinct
    bf16-exact integers in B: the result equals a gather), at tile-row group sizes 1, 4 and 8: any
    item-to-tile error of decode / xcd_remap shows, with the item named."""
    M, Nn = I.shape_for(R, cus)
    K = 64
    g = torch.Generator(device=DEV).manual_seed(200)
    a, pi = _one_hot_rows(M, K, g)
    bt, bnn = _ints(Nn, K), _ints(K, Nn)
    bias = (torch.arange(Nn, device=DEV) % 5).float()
    bn = I.pick_bn(M, Nn, cus)
    items = I.launch_order(M, Nn, bn, 1, cus, group_m)
    I.assert_rounds(items, R, f"placement group_m={group_m}")
    Mt, Nt, S = _tn_case(cus)
    at, pit = _one_hot_rows(Mt, 64 * S, g)
    at = at.t().contiguous()
    bnt = _ints(64 * S, Nt)
    try:
        C.gemm4_group_m(group_m)
        o_nt, o_nn = C.gemm_nt(a, bt, bias), C.gemm_nn(a, bnn)
        C.gemm_force(-1, S)
        o_tn = C.gemm_tn(at, bnt)
    finally:
        C.gemm_force(-1, 0)
        C.gemm4_group_m(4)
    _exact(o_nt, bt.float()[:, pi].t() + bias, f"placement NT + bias group_m={group_m}", items, bn)
    _exact(o_nn, bnn.float()[pi], f"placement NN group_m={group_m}", items, bn)
    _exact(o_tn, bnt.float()[pit], f"placement TN splits={S} group_m={group_m}", I.launch_order(Mt, Nt, 256, S, cus, group_m))


@pytest.mark.parametrize("group_m", [4, 1, 8])
def test_gemm_tn_group_placement_exact_items(C, cus, group_m):
    K = 64
    g = torch.Generator(device=DEV).manual_seed(201)
    acc = [1, 0, 0, 0]
    items, _ = I.group_order(GROUP_SHAPES, 1, cus, group_m)
    I.assert_rounds(items, R, f"grouped placement group_m={group_m}")
    A, B, PI = [], [], []
    for m, n in GROUP_SHAPES:
        at, pi = _one_hot_rows(m, K, g)
        A.append(at.t().contiguous())
        B.append(_ints(K, n))
        PI.append(pi)
    outs = [torch.full((m, n), float("nan"), device=DEV) for m, n in GROUP_SHAPES]
    outs[0] = (torch.arange(outs[0].numel(), device=DEV) % 13).float().view_as(outs[0])
    init0 = outs[0].clone()
    try:
        C.gemm4_group_m(group_m)
        assert C.gemm_tn_group(A, B, outs, acc)
    finally:
        C.gemm4_group_m(4)
    for i in range(4):
        ref = B[i].float()[PI[i]] + (init0 if i == 0 else 0)
        _exact(outs[i], ref, f"placement grouped TN member {i} group_m={group_m}", [it for it in items if it.g == i])
