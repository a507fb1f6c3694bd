"""The multi-item checks themselves, on the CPU (tests/numerics_items.py), on scaled-down
instances: a made-up CU count of 8 makes three rounds a few dozen tiles.

* **The mirror**: ``item_order`` covers every tile of every split exactly once for ragged and exact
  shapes and tile-row groups of 1 / 4 / 8, workgroups' item counts differ by at most one, the
  stream-K assignment gives every extra tile one producer and one consumer on different
  workgroups, the grouped order gives every member its own tiles from its ``item0``.
* **The emulations**: an fp32 walk over the items of each form (plain accumulation, slab sum,
  partial hand-off, two-pass RoPE, the fused epilogues) stays within ``numerics.DERIVED``; at
  K 32 / 64 the bias statistic restricted to third-round items drops under 10 % of them and holds.
* **Eleven planted faults**, each applied through the mirror to items of round >= 1 only (what a
  one-item-per-workgroup test cannot see), each fail the new check.  For each the older tests'
  criterion -- the relative Frobenius error against the fp64 product at the same case, 1e-2 for a
  bf16 output (tests/test_kernels_gpu.py), 1e-5 for an fp32 one, 1e-3 for the SwiGLU-backward bias
  gradient -- is evaluated on the same faulty output; ``OLD_PASSES`` records which it lets
  through: none of the eleven.  At these scaled-down sizes two thirds of the items are later
  items and one tile is 1 / 18 of the output, so every fault moves the global ratio past the old
  threshold: 0.022 for the single 16-row block, 0.036 for the one missing stream-K quarter, 0.055
  for one doubled slab, 0.085 to 0.98 for the faults that touch every later item.  Only the
  single-tile faults shrink with the output: by plain arithmetic (the same error mass over the
  GPU cases' 30 M and 17 M elements) the block would give 0.003 and the stream-K quarter 0.006,
  under 1e-2; that is an extrapolation, not a measurement, and the other nine stay gross at any
  size.  What the older tests lack is therefore mostly the cases, not the sensitivity: their
  shapes with several items per workgroup cover plain NT / NN / TN only, and none of them runs
  the epilogue, slab, stream-K or grouped forms with a second item in any workgroup.  Nothing
  more is claimed.
"""
import pytest
import torch

import numerics as N
import numerics_items as I

CUS = 8
R = 3
TILES = {0: (256, 128, 16), 1: (256, 192, 16)}

# fault -> does the older global criterion pass the faulty output (True = the old suite misses it)
OLD_PASSES = {"stale_bias": False, "block_neighbour": False, "drop_last_step": False, "stale_first_step": False,
              "stale_pos": False, "sk_partial_shift": False, "sk_quarter_missing": False, "slab_twice": False,
              "group_item0": False, "k_switch_overrun": False, "dbias_missing_tile": False}


def _caught(fn):
    with pytest.raises(AssertionError):
        fn()


def _randn(*shape, seed, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


# --------------------------------------------------------------------------- mirror ----

@pytest.mark.parametrize("group_m", [1, 4, 8])
@pytest.mark.parametrize("M,Nn,bn,splits", [(513, 1288, 256, 1), (513, 1288, 192, 1), (512, 768, 256, 1),
                                            (264, 264, 256, 5), (1281, 520, 256, 3), (2305, 200, 192, 1)])
def test_item_order_covers_every_tile_of_every_split_once(M, Nn, bn, splits, group_m):
    for G in (CUS, 7, 256):
        items = I.launch_order(M, Nn, bn, splits, G, group_m)
        want = {(m0, n0, s) for m0 in range(0, M, 256) for n0 in range(0, Nn, bn) for s in range(splits)}
        got = [(it.m0, it.n0, it.split) for it in items]
        assert len(got) == len(want) and set(got) == want
        w = I.per_workgroup(items)
        counts = [len(v) for v in w.values()]
        assert max(counts) - min(counts) <= 1 and len(w) == min(G, len(items))
        for v in w.values():      # a workgroup walks it, it + G, ...
            assert [it.round for it in v] == list(range(len(v)))
            assert all(b.lin - a.lin == len(w) for a, b in zip(v, v[1:]))


def test_xcd_remap_is_a_bijection():
    for G in (1, 7, 8, 9, 255, 256, 304):
        assert sorted(I.xcd_remap(b, G) for b in range(G)) == list(range(G))
    # consecutive remapped ids share an XCD (blockIdx % 8)
    assert [I.xcd_remap(b, 16) for b in (0, 8, 1, 9)] == [0, 1, 2, 3]


@pytest.mark.parametrize("cus", [8, 256, 6])
def test_stream_k_roles(cus):
    M, Nn = I.sk_shape(cus)
    items = I.sk_order(M, Nn, cus)
    tiles = I.tile_map(items, 256)
    assert len(tiles) == 3 * cus // 2 == I.cdiv(M, 256) * I.cdiv(Nn, 256)
    pairs = [v for v in tiles.values() if len(v) == 2]
    assert len(pairs) == cus // 2 and all(len(v) in (1, 2) for v in tiles.values())
    for a, b in pairs:
        assert {a.role, b.role} == {1, 2} and a.wg != b.wg and a.g == b.g >= 0
        prod, cons = (a, b) if a.role == 1 else (b, a)
        assert prod.round == 0 and cons.round == 1      # the producer runs its half first, the consumer last
    assert all(v[0].role == 0 for v in tiles.values() if len(v) == 1)
    assert all(len(v) == 2 for v in I.per_workgroup(items).values())


def test_group_order_members_and_item0():
    shapes = [(520, 264), (264, 776), (256, 256), (1032, 8)]
    for splits in (1, 3):
        items, item0 = I.group_order(shapes, splits, CUS)
        assert item0 == [0, 6 * splits, 14 * splits, 15 * splits]
        for g, (M, Nn) in enumerate(shapes):
            mine = [(it.m0, it.n0, it.split) for it in items if it.g == g]
            want = {(m0, n0, s) for m0 in range(0, M, 256) for n0 in range(0, Nn, 256) for s in range(splits)}
            assert len(mine) == len(want) and set(mine) == want
            assert min(it.lin for it in items if it.g == g) == item0[g]


def test_shape_helpers():
    for cus in (8, 6, 256, 304):
        for rounds in (3, 4):
            M, Nn = I.shape_for(rounds, cus)
            tm, tn = I.cdiv(M, 256), I.cdiv(Nn, 256)
            assert M % 256 == 1 and Nn % 256 == 8 and tm % I.GROUP_M and tm * tn > (rounds - 1) * cus
            for variant in (0, 2):
                w = I.per_workgroup(I.launch_order(M, Nn, I.pick_bn(M, Nn, cus, variant), 1, cus))
                assert max(len(v) for v in w.values()) >= rounds
            for tiles_n in (3, 5, 6):
                Mr = I.m_for(rounds, cus, tiles_n)
                assert Mr % 256 == 1 and I.cdiv(Mr, 256) * tiles_n > (rounds - 1) * cus
        assert I.pick_bn(*I.shape_for(3, cus, bn=256), cus) == 256
        S = I.forced_splits(3, cus, 4)
        assert 4 * S > 2 * cus >= 4 * (S - 1)
    # the launcher's example: 384 tiles of 256 x 256 on 256 CUs run 192 wide, 512 tiles do not
    assert I.pick_bn(32768, 768, 256) == 192 and I.pick_bn(32768, 1024, 256) == 256
    assert I.nsteps(0, 32) == 2 and I.nsteps(0, 64) == 2 and I.nsteps(0, 96) == 4 and I.nsteps(0, 160) == 6


def test_assert_within_names_the_item():
    M, Nn = I.shape_for(R, CUS)
    items = I.launch_order(M, Nn, 256, 1, CUS)
    ref = torch.ones(M, Nn, dtype=torch.float64)
    out = ref.clone()
    it = next(it for it in items if it.round == 2)
    out[it.m0 + 3, it.n0 + 5] = 2
    with pytest.raises(AssertionError, match=rf"item {it.lin} \(workgroup {it.wg}, round 2\)"):
        I.assert_within_rows(out, lambda r0, r1: (ref[r0:r1], 1e-3 * ref[r0:r1]), N.DERIVED, "x", TILES, items, 256, rows=100)
    # the keyword's default is the old message
    with pytest.raises(AssertionError) as e:
        N.assert_within(out, ref, 1e-3 * ref, N.DERIVED, "x")
    assert "item" not in str(e.value)


# ----------------------------------------------------------------------- emulations ----

def _plain_case(K, seed=1):
    M, Nn = I.shape_for(R, CUS)
    bn = I.pick_bn(M, Nn, CUS)
    items = I.launch_order(M, Nn, bn, 1, CUS)
    I.assert_rounds(items, R, "plain")
    a, b = _randn(M, K, seed=seed), _randn(Nn, K, seed=seed + 1)
    bias = _randn(Nn, seed=seed + 2, dtype=torch.float32)
    ref, mag = N.ref_gemm(a, b, "nt", bias)
    return a, b, bias, items, bn, ref, mag


def _plain_out(a, b, bias, items, bn, K, fault=None):
    return I.emu_items(a.float(), b.float().t(), items, bn, K, I.cdiv(K, 32) * 32, bias, fault)[0].bfloat16()


@pytest.mark.parametrize("K", [32, 64, 96, 160])
def test_plain_emulation_within_derived(K):
    a, b, bias, items, bn, ref, mag = _plain_case(K)
    out = _plain_out(a, b, bias, items, bn, K)
    N.assert_within(out, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, f"emulated items K {K}", TILES,
                    where=I.locator(items, bn))
    if K in (32, 64):     # the condition under which the GPU statistic runs: it drops < 10 % and holds
        mask = I.round_mask(*ref.shape, items, bn, 2)
        assert int(mask.sum()) > 50000
        _, _, dropped = N.bias_stat(out[mask], ref[mask], N.acc_term_gemm(mag, K)[mask], f"emulated third round K {K}")
        assert dropped < 0.10
        chopped = N.bf16_trunc(a.float() @ b.float().t() + bias)        # the wrong rounding mode stays visible there
        _caught(lambda: N.bias_stat(chopped[mask], ref[mask], N.acc_term_gemm(mag, K)[mask], "chopped"))


def _split_case(layout, S, kps, M=520, Nn=392, seed=10, K=None):
    K = K or S * kps
    items = I.launch_order(M, Nn, 256, S, CUS)
    I.assert_rounds(items, R, "split")
    a = _randn(K, M, seed=seed) if layout == "tn" else _randn(M, K, seed=seed)
    b = _randn(Nn, K, seed=seed + 1) if layout == "nt" else _randn(K, Nn, seed=seed + 1)
    A = a.float().t() if layout == "tn" else a.float()
    Bm = b.float().t() if layout == "nt" else b.float()
    return a, b, A, Bm, items, K


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_slab_sum_emulation_within_derived(layout):
    S, kps = I.forced_splits(R, CUS, 6), 64
    a, b, A, Bm, items, K = _split_case(layout, S, kps)
    bias = _randn(392, seed=12, dtype=torch.float32) if layout == "nt" else None
    ref, mag = N.ref_gemm(a, b, layout, bias)
    out = I.emu_slab_sum(I.emu_items(A, Bm, items, 256, K, kps), bias).bfloat16()
    N.assert_within(out, ref, I.unit_splitk_bf16(ref, mag, K, S), N.DERIVED, f"emulated bf16 split-K {layout}", TILES)


@pytest.mark.parametrize("kmul,kadd", [(32, 0), (64, 0), (96, 0), (64, -40)])
def test_tn_slab_emulation_within_derived(kmul, kadd):
    """The TN launcher rounds the split length up to 64: K = 32 S leaves the trailing splits empty."""
    S = I.forced_splits(R, CUS, 4) | 1
    K = kmul * S + kadd
    kps = I.cdiv(I.cdiv(K, S), 64) * 64
    a, b, A, Bm, items, _ = _split_case("tn", S, kps, 264, 264, 20, K)
    acc0 = _randn(264, 264, seed=22, dtype=torch.float32)
    ref, mag = N.ref_gemm(a, b, "tn")
    slabs = I.emu_items(A, Bm, items, 256, K, kps)
    N.assert_within(I.emu_slab_sum(slabs), ref, N.unit_gemm_f32(mag, K, S), N.DERIVED, "emulated TN", TILES)
    N.assert_within(I.emu_slab_sum(slabs, acc=acc0), ref + acc0.double(), N.unit_gemm_f32(mag, K, S, acc0), N.DERIVED,
                    "emulated TN accumulate", TILES)


def _sk_case(K, seed=30):
    M, Nn = I.sk_shape(CUS)
    items = I.sk_order(M, Nn, CUS)
    a, b = _randn(M, K, seed=seed), _randn(Nn, K, seed=seed + 1)
    bias = _randn(Nn, seed=seed + 2, dtype=torch.float32)
    ref, mag = N.ref_gemm(a, b, "nt", bias)
    return a, b, bias, items, ref, mag


@pytest.mark.parametrize("K", [128, 384])
def test_stream_k_emulation_within_derived(K):
    a, b, bias, items, ref, mag = _sk_case(K)
    out = I.emu_stream_k(a.float(), b.float().t(), items, K, bias)
    N.assert_within(out, ref, I.unit_gemm_sk(ref, mag, K), N.DERIVED, f"emulated stream-K {K}", TILES,
                    where=I.locator(items, 256))


def _rope_case(hd, K, split, seed=40):
    H = 4 if hd == 64 else 2
    Nn = 3 * H * hd
    M = 520 if split else I.m_for(R, CUS, Nn // 256)
    S = I.forced_splits(R, CUS, I.cdiv(M, 256) * (Nn // 256)) if split else 1
    K = 64 * S if split else K
    items = I.launch_order(M, Nn, 256, S, CUS)
    I.assert_rounds(items, R, "rope")
    a, b = _randn(M, K, seed=seed), _randn(Nn, K, seed=seed + 1, scale=K ** -0.5)
    bias = _randn(Nn, seed=seed + 2, dtype=torch.float32)
    pos = torch.randint(0, 512, (M,), generator=torch.Generator().manual_seed(seed + 3))
    tab = N.rope_table(512, hd)
    lin, mag = N.ref_gemm(a, b, "nt", bias)
    return a, b, bias, pos, tab, 2 * H, items, S, K, lin, mag


@pytest.mark.parametrize("hd", [64, 128])
def test_two_pass_rope_emulation_within_derived(hd):
    a, b, bias, pos, tab, heads, items, S, K, lin, mag = _rope_case(hd, 0, True)
    y = I.emu_slab_sum(I.emu_items(a.float(), b.float().t(), items, 256, K, 64), bias).bfloat16()
    out = I.emu_rope(y.float(), pos, tab, heads, hd).bfloat16()
    ref, unit = I.unit_rope_two_pass(lin, N.unit_gemm_f32(mag, K, S), pos, tab, heads, hd)
    N.assert_within(out, ref, unit, N.DERIVED, f"emulated split-K + rope after hd {hd}", TILES)
    # the one-rounding unit of the fused epilogue does not hold the second pass: the units differ
    fused = N.U16 * ref.abs() + N.ref_rope(lin, pos, tab, heads, hd, mag=N.unit_gemm_f32(mag, K, S))[1]
    _caught(lambda: N.assert_within(out, ref, fused + 3 * N.U32 * N.ref_rope(lin, pos, tab, heads, hd)[1], N.DERIVED, "x"))


def _rope_epilogue_check(hd, K, faulty):
    a, b, bias, pos, tab, heads, items, _, K, lin, mag = _rope_case(hd, K, False)
    acc = I.emu_items(a.float(), b.float().t(), items, 256, K, I.cdiv(K, 32) * 32, bias)[0]
    out = I.emu_rope(acc, I.stale_positions(pos, items) if faulty else pos, tab, heads, hd).bfloat16()
    ref, rmag = N.ref_rope(lin, pos, tab, heads, hd)
    unit = N.U16 * ref.abs() + N.ref_rope(lin, pos, tab, heads, hd, mag=N.acc_term_gemm(mag, K))[1] + 3 * N.U32 * rmag
    return out, ref, unit, items


@pytest.mark.parametrize("hd,K", [(64, 64), (128, 96)])
def test_rope_epilogue_emulation_within_derived(hd, K):
    out, ref, unit, items = _rope_epilogue_check(hd, K, False)
    N.assert_within(out, ref, unit, N.DERIVED, f"emulated rope epilogue hd {hd}", TILES, where=I.locator(items, 256))


GROUP = [(520, 264), (264, 776), (512, 520), (1032, 264)]      # 6 + 8 + 6 + 10 tiles: four rounds of 8, the last short


def _group_case(K0, K1, fault=None, seed=50):
    """(outs, refs, units, items) of the grouped launch's emulation: members [1, 0, 1, 0] accumulate."""
    S, kps = (1, K0) if not K1 else (2, max(K0, K1))
    ksw = kps if K1 else None
    items, _ = I.group_order(GROUP, S, CUS)
    I.assert_rounds(items, R, "group")
    outs, refs, units = [], [], []
    for g, (M, Nn) in enumerate(GROUP):
        a, b = _randn(K0, M, seed=seed + g), _randn(K0, Nn, seed=seed + 10 + g)
        a2 = _randn(K1, M, seed=seed + 20 + g) if K1 else None
        b2 = _randn(K1, Nn, seed=seed + 30 + g) if K1 else None
        init = _randn(M, Nn, seed=seed + 40 + g, dtype=torch.float32) if g % 2 == 0 else None
        ref, mag = N.ref_gemm(a, b, "tn", acc=init)
        if K1:
            r1, m1 = N.ref_gemm(a2, b2, "tn")
            ref, mag = ref + r1, mag + m1
        mine = [it for it in items if it.g == g]
        slabs = I.emu_items(a.float().t(), b.float(), mine, 256, (ksw + K1) if K1 else K0, kps, None, fault, ksw,
                            a2.float().t() if K1 else None, b2.float() if K1 else None, K0 if K1 else None)
        outs.append(I.emu_slab_sum(slabs, acc=init))
        refs.append(ref)
        units.append(N.unit_gemm_f32(mag, K0 + K1, (K0 + K1) // 64, init))
    return outs, refs, units, items


@pytest.mark.parametrize("K0,K1", [(512, 0), (512, 256)])
def test_group_emulation_within_derived(K0, K1):
    outs, refs, units, _ = _group_case(K0, K1)
    for g in range(4):
        N.assert_within(outs[g], refs[g], units[g], N.DERIVED, f"emulated group member {g}", TILES)


def _swb_case(seed=70):
    F_, K = 640, 64
    M = I.m_for(R, CUS, I.cdiv(F_, 256))
    items = I.launch_order(M, F_, 256, 1, CUS)
    I.assert_rounds(items, R, "swiglu bwd")
    dy, w = _randn(M, K, seed=seed, scale=0.25), _randn(K, F_, seed=seed + 1, scale=0.25)
    gu = _randn(M, 2 * F_, seed=seed + 2)
    ds, mag = N.ref_gemm(dy, w, "nn")
    _, _, _, dbr, dbu = N.ref_swiglu_bwd(ds, gu, False, dh_unit=N.unit_gemm_bf16(ds, mag, K))
    return dy, w, gu, items, dbr, dbu


def test_swiglu_bwd_dbias_emulation_within_derived():
    dy, w, gu, items, dbr, dbu = _swb_case()
    N.assert_within(I.emu_swiglu_bwd_dbias(dy, w, gu, items), dbr, dbu, N.DERIVED, "emulated swiglu-bwd dbias")


# ------------------------------------------------------------------- planted faults ----

def _old(out, ref, tol):
    """The older tests' criterion: global relative Frobenius error under ``tol``."""
    return N.rel(out, ref) < tol


def _fault_plain(fault):
    K = 160
    a, b, bias, items, bn, ref, mag = _plain_case(K)
    unit = N.unit_gemm_bf16(ref, mag, K)
    out = _plain_out(a, b, bias, items, bn, K, None if fault == "block_neighbour" else fault)
    if fault == "block_neighbour":      # one 16-row block of a second-round tile taken from the neighbouring tile
        it = next(it for it in items if it.round == 1 and it.n0 + 2 * bn <= ref.size(1))
        out[it.m0:it.m0 + 16, it.n0:it.n0 + bn] = out[it.m0:it.m0 + 16, it.n0 + bn:it.n0 + 2 * bn].clone()
    check = lambda: N.assert_within(out, ref, unit, N.DERIVED, fault, TILES, where=I.locator(items, bn))
    return check, _old(out, ref, 1e-2)


def _fault_rope(fault):
    out, ref, unit, items = _rope_epilogue_check(64, 64, True)
    return (lambda: N.assert_within(out, ref, unit, N.DERIVED, fault, TILES, where=I.locator(items, 256))), _old(out, ref, 1e-2)


def _fault_sk(fault):
    K = 384
    a, b, bias, items, ref, mag = _sk_case(K)
    out = I.emu_stream_k(a.float(), b.float().t(), items, K, bias, fault)
    check = lambda: N.assert_within(out, ref, I.unit_gemm_sk(ref, mag, K), N.DERIVED, fault, TILES, where=I.locator(items, 256))
    return check, _old(out, ref, 1e-2)


def _fault_slab(fault):
    S, kps = I.forced_splits(R, CUS, 6), 64
    a, b, A, Bm, items, K = _split_case("nt", S, kps)
    ref, mag = N.ref_gemm(a, b, "nt")
    it = next(it for it in items if it.round == 1)
    out = I.emu_slab_sum(I.emu_items(A, Bm, items, 256, K, kps), twice=(it.split, it.m0, it.n0, 256)).bfloat16()
    check = lambda: N.assert_within(out, ref, I.unit_splitk_bf16(ref, mag, K, S), N.DERIVED, fault, TILES,
                                    where=I.locator(items, 256))
    return check, _old(out, ref, 1e-2)


def _fault_group(fault):
    if fault == "k_switch_overrun":
        outs, refs, units, items = _group_case(512, 256, fault)
    else:       # a tile of member 1 (round >= 1) written at member 0's item0: into member 0's first tile
        outs, refs, units, items = _group_case(512, 0)
        it = next(it for it in items if it.g == 1 and it.round >= 1)
        r, c = min(256, GROUP[1][0] - it.m0, GROUP[0][0]), min(256, GROUP[1][1] - it.n0, GROUP[0][1])
        outs[0][:r, :c] = outs[1][it.m0:it.m0 + r, it.n0:it.n0 + c]
        outs[1][it.m0:it.m0 + 256, it.n0:it.n0 + 256] = 0
    def check():
        for g in range(4):
            N.assert_within(outs[g], refs[g], units[g], N.DERIVED, f"{fault} member {g}", TILES,
                            where=I.locator([it for it in items if it.g == g], 256))
    return check, all(_old(o, r, 1e-5) for o, r in zip(outs, refs))


def _fault_dbias(fault):
    dy, w, gu, items, dbr, dbu = _swb_case()
    it = next(it for it in items if it.round == 1)
    db = I.emu_swiglu_bwd_dbias(dy, w, gu, items, missing=(it.m0, it.n0))
    return (lambda: N.assert_within(db, dbr, dbu, N.DERIVED, fault)), _old(db, dbr, 1e-3)


FAULTS = {"stale_bias": _fault_plain, "block_neighbour": _fault_plain, "drop_last_step": _fault_plain,
          "stale_first_step": _fault_plain, "stale_pos": _fault_rope, "sk_partial_shift": _fault_sk,
          "sk_quarter_missing": _fault_sk, "slab_twice": _fault_slab, "group_item0": _fault_group,
          "k_switch_overrun": _fault_group, "dbias_missing_tile": _fault_dbias}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_on_later_items_is_caught(fault):
    check, old_passes = FAULTS[fault](fault)
    _caught(check)
    print(f"{fault}: old criterion passes = {old_passes}")
    assert old_passes == OLD_PASSES[fault], f"{fault}: the older criterion {'passes' if old_passes else 'fails'} it"


def test_old_passes_count():
    assert set(OLD_PASSES) == set(FAULTS) and len(FAULTS) == 11
    assert sum(OLD_PASSES.values()) == 0
