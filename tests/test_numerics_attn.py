"""The attention launch mirror, the variants' emulations and limits, and planted faults, on the CPU
(tests/numerics_attn.py).

* **Mirror proofs**: over BH 1 .. 20, T in {1, 64, 128, 129, 300, 641, 1025} and H in {1, 3, 4, 9},
  for every kernel: each (bh, block) is owned by exactly one workgroup, the grid equals the
  launcher's formula, the empty slots are exactly bh >= BH, a head's workgroups share ``it & 7``
  in the 1-D form, the 2-D remap is a permutation, and ``locate`` inverts the enumeration.
* **Emulation limits**: every emulation, variant or not, stays within half its limit (its
  ``measured``) at every case the two GPU files run; with the flags off the copies are
  bit-identical to tests/numerics.py's.
* **Planted faults**, applied to the emulation's output through the mirror.  Each fails
  ``assert_within`` at a new case; (a) - (d) and (f) select elements only through bh >= 8 or
  p >= 2 and leave the output bit-identical at the old geometry (B 2, H 3, T <= 385), which
  proves they were unreachable there:

  (a) K / V of head bh - 8 used for bh >= 8 (o);
  (b) the dK/dV kernel's lse / delta row base taken with bh & 7 (dk, dv);
  (c) the last key tile of the heavy block dropped for pairs p >= 2 (o);
  (d) dbias misses the partial rows of bh >= 8;
  (e) the 2-D xcd_remap with its remainder r taken as 0: some blocks run twice, others are never
      written.  This one is NOT unreachable at the old geometry: 6 and 12 workgroups have r = 6 and
      4, and the mirror shows unwritten blocks there too (the existing head_dim-32 bounds catch
      it); only the old 24-workgroup launch has r = 0.  New here are q >= 2 with r in {2, .., 6};
  (f) one 32-row wave slab of o of a head bh >= 8 scaled by 1.03;
  (g) the RSM emulation's lse against the non-RSM unit and key: it fails, so the variant keys are
      needed.

  The old criterion (global Frobenius ratio < 2e-2 for o, < 3e-2 for the gradients, |lse error|
  < 2e-2) at these sizes also catches (a), (b), (d), (e) (whole heads or blocks wrong or unwritten)
  and (c) (in the near one-hot "peaked" rows a dropped tile often holds the dominant key: ratio
  0.13 with two heads); it passes (f) and (g).  ``OLD_CATCHES`` asserts this.
* **Rescale pin**: the "peaked" family, and only it, drives the forward's deferred-rescale branch.
"""
import itertools

import pytest
import torch

import numerics as N
import numerics_attn as A

T_SET = (1, 64, 128, 129, 300, 641, 1025)


# --------------------------------------------------------------------- mirror proofs ----

@pytest.mark.parametrize("kernel", list(A.KERNELS))
def test_mirror_every_block_has_one_owner_and_grids_match_the_launchers(kernel):
    form, block, by = A.KERNELS[kernel]
    for BH, T, causal in itertools.product(range(1, 21), T_SET, (True, False)):
        nb = (T + block - 1) // block
        ws = A.launch(kernel, BH, T, causal)
        owned = sorted((w.bh, w.block) for w in ws)
        assert owned == [(bh, blk) for bh in range(BH) for blk in range(nb)], (kernel, BH, T)
        if form == "paired":
            # dpfs_attn_fwd / dpfs_attn_bwd / dpfs_attn_bwd_fused: (B * H + 7) / 8 * 8 * ((n + 1) / 2)
            grid = (BH + 7) // 8 * 8 * ((nb + 1) // 2)
            rows = A.paired_launch(BH, T, causal, block, by)
            assert len(rows) == grid == A.grid_size(kernel, BH, T)
            assert [it for it, _, _, _ in rows] == list(range(grid))
            for it, bh, p, blocks in rows:
                assert (not blocks) == (bh >= BH), "empty slots are exactly bh >= BH"
                assert 0 <= p < (nb + 1) // 2 and len(blocks) == (0 if bh >= BH else (1 if 2 * p == nb - 1 else 2))
            slot = {}
            for w in ws:
                assert slot.setdefault(w.bh, w.wg & 7) == w.wg & 7 == w.xcd, "a head's workgroups share it & 7"
            # under the causal mask the block a workgroup runs first sweeps at least as many tiles
            for _, _, _, blocks in rows:
                if causal and len(blocks) == 2:
                    assert blocks[0].role == 0 and blocks[1].role == 1 and blocks[0].tiles >= blocks[1].tiles
        else:
            assert len(ws) == nb * BH == A.grid_size(kernel, BH, T)       # dim3 grid(gx, B * H)
            assert sorted(A.xcd_remap(i, nb * BH) for i in range(nb * BH)) == list(range(nb * BH)), "a permutation"
            assert [w.wg for w in ws] == list(range(nb * BH))


@pytest.mark.parametrize("H", [1, 3, 4, 9])
@pytest.mark.parametrize("kernel", list(A.KERNELS))
def test_mirror_locate_inverts_the_enumeration(kernel, H):
    block = A.KERNELS[kernel][1]
    for B, T, causal in itertools.product((1, 2, 5), T_SET, (True, False)):
        if B * H > 20:
            continue
        by_owner = {(w.bh, w.block): w for w in A.launch(kernel, B * H, T, causal)}
        for b, h, t in itertools.product(range(B), range(H), sorted({0, T // 2, T - 1, min(T - 1, block)})):
            w = A.locate(kernel, b, t, h, B, H, T, causal)
            assert w.bh == b * H + h and w.block == t // block
            assert w == by_owner[(w.bh, w.block)], (kernel, B, H, T, b, h, t)
    assert "workgroup" in A.where_fn(kernel, "lse", 2, H, 300, True)((1, H - 1, 299))


def test_mirror_tile_counts_of_the_issue_cases():
    r = A.reach("fwd3", 1, 2, 641, True)
    assert (r["blocks"], r["max_p"], r["heavy_tiles"], r["workgroups"]) == (6, 2, 11, 24)
    assert A.reach("fwd3", 1, 2, 1025, True)["unpaired"] and A.reach("fwd3", 1, 2, 1025, True)["blocks"] == 9
    assert [A.reach(k, 3, 3, 300, True)["workgroups"] for k in ("fwd", "dq", "dkdv2")] == [27, 27, 45]
    assert [A.reach(k, 2, 5, 200, True)["workgroups"] for k in ("fwd", "dkdv2")] == [20, 40]
    old = A.reach("fwd3", 2, 3, 385, True)                               # the old geometry
    assert old["groups"] == 1 and old["max_bh"] == 5 and old["max_p"] == 1 and old["blocks"] == 4


# ------------------------------------------------------------------- emulation limits ----

def test_flagless_copies_are_bit_identical_to_the_existing_emulations():
    for hd, T, causal, rope in [(64, 300, True, True), (128, 130, False, False), (32, 65, True, False)]:
        q, k, v, do, pos = N.attn_inputs(hd, T, "peaked")
        q2, k2, v2, do2, pos2 = A.attn_inputs_bh(hd, T, "peaked", 2, 3)
        assert all(torch.equal(a, b) for a, b in ((q, q2), (k, k2), (v, v2), (do, do2), (pos, pos2)))
        tab = N.rope_table(512, hd) if rope else None
        o, lse = N.emu_attn_fwd(q, k, v, hd ** -0.5, causal)
        o2, lse2 = A.emu_attn_fwd(q, k, v, hd ** -0.5, causal)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)
        a = N.emu_attn_bwd(do, q, k, v, o, lse, hd ** -0.5, causal, pos if rope else None, tab)
        b = A.emu_attn_bwd(do, q, k, v, o, lse, hd ** -0.5, causal, pos if rope else None, tab)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(A.attn_inputs_bh(64, 129, "randn", 3, 4)[0][:2, :, :3], N.attn_inputs(64, 129, "randn")[0])


def test_limit_table_follows_the_module_rule():
    for key, e in A.LIMITS_ATTN.items():
        assert e["limit"] == 2 * e["measured"] and len(e["at"]) == 7, key
        if key.endswith(".heads"):      # a key of its own only where the old key's measured is exceeded
            assert e["measured"] > N.LIMITS[key[:-6]]["measured"], key
        else:
            assert key.rsplit(".", 1)[1] in A.VARIANT_OUTPUTS and key not in N.LIMITS


def _emulation_runs():
    """The distinct (case, family, rope, forward variant, backward variant, outputs) the GPU files run."""
    runs = {}
    for case, fam, rope in A.items_cases():
        runs[(case, fam, rope, None, None)] = ("dq", "dk", "dv", "dbias") if rope else ("o", "lse", "dq", "dk", "dv")
    for _, var, _, case, fam in A.fwd_variant_cases():
        runs.setdefault((case, fam, False, var, None), ("o", "lse"))
    for _, var, _, _, case, fam, rope in A.bwd_variant_cases():
        runs.setdefault((case, fam, rope, None, var), ("dq", "dk", "dv") + (("dbias",) if rope else ()))
    return [k + (v,) for k, v in runs.items()]


@pytest.mark.parametrize("case,fam,rope,fvar,bvar,names", _emulation_runs(), ids=A.pid)
def test_attention_emulations_within_half_their_limits(case, fam, rope, fvar, bvar, names):
    _, ref, out = A.emulated(case, fam, rope, fvar, bvar)
    hd = case[2]
    for name in names:
        key = A.key_for(name, hd, rope, fvar if name in ("o", "lse") else bvar)
        N.assert_within(out[name], ref[name], ref["unit_" + name], 1.001 * A.measured(key), f"emulated {name} [{key}]",
                        N.ATTN_TILES[name])


# -------------------------------------------------------------------- planted faults ----

OLD = (2, 3, 64, 300, True)            # the old geometry: one group of eight, p <= 1
NEW = (3, 4, 64, 129, True)            # twelve heads
OLD_CATCHES = {"a": True, "b": True, "c": True, "d": True, "e": True, "f": False, "g": False}


def _bh_ge8(kernel, case):
    """(B, H) bool: the heads the mirror puts in a second or later group of eight."""
    B, H, _, T, causal = case
    form, block, _ = A.KERNELS[kernel]
    NP = (A.n_blocks(T, block) + 1) // 2
    m = torch.zeros(B, H, dtype=torch.bool)
    for w in A.launch(kernel, B * H, T, causal):
        if (w.wg >> 3) // NP >= 1:
            m[w.bh // H, w.bh % H] = True
    return m


def _shift8(x, sel, head_dim):
    """x with head bh's slice replaced by head (bh - 8)'s (= bh & 7 for 8 <= bh < 16) where ``sel``;
    x is (B, T, H, hd) (head_dim 2) or (B, H, T) (head_dim 1), heads numbered bh = b H + h."""
    B, H = sel.shape
    y = x.clone()
    for b in range(B):
        for h in range(H):
            if sel[b, h]:
                sb, sh = divmod(b * H + h - 8, H)
                if head_dim == 2:
                    y[b, :, h] = x[sb, :, sh]
                else:
                    y[b, h] = x[sb, sh]
    return y


def _fault_a(case, fam="randn"):
    (q, k, v, *_), ref, out = A.emulated(case, fam)
    sel = _bh_ge8("fwd3", case)
    o2, _ = A.emu_attn_fwd(q, _shift8(k, sel, 2), _shift8(v, sel, 2), case[2] ** -0.5, case[4])
    return ref, out["o"], torch.where(sel[:, None, :, None], o2, out["o"])


def _fault_b(case, fam="randn"):
    (q, k, v, do, *_), ref, out = A.emulated(case, fam)
    sel = _bh_ge8("dkdv3", case)
    kconst = (_shift8(out["o"], sel, 2), _shift8(out["lse"], sel, 1))
    _, dk, dv, _ = A.emu_attn_bwd(do, q, k, v, out["o"], out["lse"], case[2] ** -0.5, case[4], kconst=kconst)
    return ref, out, dk, dv


def _fault_c(case, fam="peaked"):
    B, H, hd, T, causal = case
    (q, k, v, *_), ref, out = A.emulated(case, fam)
    drop = torch.zeros(T, T, dtype=torch.bool)
    for w in A.launch("fwd3", B * H, T, causal):
        if w.role == 0 and w.p >= 2:        # the heavy block of a pair p >= 2: its last key tile never runs
            drop[w.block * 128:(w.block + 1) * 128, (w.tiles - 1) * 64:w.tiles * 64] = True
    o2, _ = A.emu_attn_fwd(q, k, v, hd ** -0.5, causal, drop=drop)
    return ref, out["o"], o2, bool(drop.any())


def _fault_d(case, fam="randn"):
    _, ref, out = A.emulated(case, fam, True)
    sel = _bh_ge8("dkdv3", case)[:, None, :, None]
    lost = torch.cat([(x.float() * sel).sum((0, 1)).reshape(-1) for x in (out["dq"], out["dk"], out["dv"])])
    return ref, out["dbias"], out["dbias"] - lost


def _remap_r0(orig, nwg):
    q, xcd = nwg // 8, orig % 8
    return xcd * q + orig // 8          # xcd_remap with r = nwg % 8 taken as 0


def _unwritten(kernel, B, H, T, causal):
    """(bh, block) no workgroup of the faulty 2-D launch writes."""
    block = A.KERNELS[kernel][1]
    run = {(w.bh, w.block) for w in A.launch(kernel, B * H, T, causal, remap=_remap_r0)}
    return sorted({(bh, blk) for bh in range(B * H) for blk in range(A.n_blocks(T, block))} - run)


def _caught(out, ref, name, key, what):
    try:
        N.assert_within(out, ref[name], ref["unit_" + name], A.limit(key), what, N.ATTN_TILES[name])
    except AssertionError:
        return True
    return False


def test_fault_a_kv_of_head_minus_8():
    ref, good, bad = _fault_a(NEW)
    assert not _caught(good, ref, "o", A.key_for("o", 64), "o") and _caught(bad, ref, "o", A.key_for("o", 64), "fault a")
    assert (N.rel(bad, ref["o"]) >= 2e-2) == OLD_CATCHES["a"]
    _, good, same = _fault_a(OLD)
    assert torch.equal(good, same), "unreachable at the old geometry"


def test_fault_b_lse_delta_row_base_with_bh_and_7():
    ref, out, dk, dv = _fault_b(NEW)
    for name, bad in (("dk", dk), ("dv", dv)):
        assert not _caught(out[name], ref, name, A.key_for(name, 64), name)
        assert _caught(bad, ref, name, A.key_for(name, 64), "fault b " + name)
    assert (N.rel(dk, ref["dk"]) >= 3e-2 or N.rel(dv, ref["dv"]) >= 3e-2) == OLD_CATCHES["b"]
    _, out, dk, dv = _fault_b(OLD)
    assert torch.equal(out["dk"], dk) and torch.equal(out["dv"], dv), "unreachable at the old geometry"


def test_fault_c_last_key_tile_of_the_heavy_block_dropped_for_p_ge_2():
    ref, good, bad, any_drop = _fault_c((1, 2, 64, 641, True))
    assert any_drop and not _caught(good, ref, "o", A.key_for("o", 64), "o")
    assert _caught(bad, ref, "o", A.key_for("o", 64), "fault c")
    assert (N.rel(bad, ref["o"]) >= 2e-2) == OLD_CATCHES["c"]
    _, good, same, any_drop = _fault_c((2, 3, 64, 385, True))
    assert not any_drop and torch.equal(good, same), "unreachable at the old geometry (p <= 1)"


def test_fault_d_dbias_misses_the_partial_rows_of_bh_ge_8():
    ref, good, bad = _fault_d(NEW)
    key = A.key_for("dbias", 64, True)
    assert not _caught(good, ref, "dbias", key, "dbias") and _caught(bad, ref, "dbias", key, "fault d")
    assert (N.rel(bad, ref["dbias"]) >= 3e-2) == OLD_CATCHES["d"]
    _, good, same = _fault_d(OLD)
    assert torch.equal(good, same), "unreachable at the old geometry"


def test_fault_e_remap_remainder_taken_as_zero():
    case = (3, 3, 32, 300, True)
    B, H, hd, T, causal = case
    _, ref, out = A.emulated(case, "randn")
    lost = _unwritten("fwd", B, H, T, causal)
    assert lost and _unwritten("dq", B, H, T, causal) and _unwritten("dkdv2", B, H, T, causal)
    bad = out["o"].float()                 # the GPU tests fill their outputs with NaN: unwritten stays NaN
    for bh, blk in lost:
        bad[bh // H, blk * 128:(blk + 1) * 128, bh % H] = float("nan")
    assert not _caught(out["o"], ref, "o", A.key_for("o", hd), "o") and _caught(bad, ref, "o", A.key_for("o", hd), "fault e")
    assert (not N.rel(bad, ref["o"]) < 2e-2) == OLD_CATCHES["e"]
    for c in A.HD32_CASES:          # every new head_dim-32 case loses blocks wherever its workgroup count % 8 != 0
        for kern in ("fwd", "dq", "dkdv2"):
            assert bool(_unwritten(kern, c[0], c[1], c[3], c[4])) == (A.grid_size(kern, c[0] * c[1], c[3]) % 8 != 0), (kern, c)
        assert _unwritten("fwd", c[0], c[1], c[3], c[4])
    # the old geometry: reachable at 6 and 12 workgroups (r = 6, 4), not at the 24 of dK/dV at T 200 (r = 0)
    assert _unwritten("fwd", 2, 3, 65, True) and _unwritten("dkdv2", 2, 3, 65, True) and _unwritten("fwd", 2, 3, 200, True)
    assert not _unwritten("dkdv2", 2, 3, 200, True)


def test_fault_f_one_wave_slab_of_a_head_ge_8_scaled():
    _, ref, out = A.emulated(NEW, "randn")
    sel = _bh_ge8("fwd3", NEW)
    b, h = [(b, h) for b in range(NEW[0]) for h in range(NEW[1]) if sel[b, h]][1]
    w = A.locate("fwd3", b, 32, h, NEW[0], NEW[1], NEW[3], True)
    assert w.bh >= 8 and w.wg >= 8
    bad = out["o"].float().clone()
    bad[b, 32:64, h] *= 1.03               # wave 1 of the block's four 32-query waves
    bad = bad.bfloat16()
    assert _caught(bad, ref, "o", A.key_for("o", 64), "fault f")
    assert (N.rel(bad, ref["o"]) >= 2e-2) == OLD_CATCHES["f"]
    assert not _bh_ge8("fwd3", OLD).any(), "unreachable at the old geometry"


def test_fault_g_rsm_lse_fails_the_default_unit_and_key():
    case = (2, 3, 64, 300, True)
    _, ref, out = A.emulated(case, "peaked", False, "rsm", None)
    _, base, _ = A.emulated(case, "peaked")
    assert not _caught(out["lse"], ref, "lse", "attn.lse.hd64.rsm", "rsm lse, rsm unit")
    assert _caught(out["lse"], base, "lse", "attn.lse.hd64", "fault g")
    assert ((out["lse"].double() - base["lse"]).abs().max() >= 2e-2) == OLD_CATCHES["g"]


# ---------------------------------------------------------------------- rescale pin ----

def _rows_with_a_jump(hd, T, fam):
    """Per (b, h): query rows whose running max over 64-key tiles (fp64 scores in log2 units, causal)
    grows by more than 8 from one tile to the next: the rows that take the deferred-rescale branch."""
    q, k, _, _, _ = N.attn_inputs(hd, T, fam)
    s = (N._bhtd(q) @ N._bhtd(k).transpose(-1, -2)) * (hd ** -0.5 * N.LOG2E)
    s = s.masked_fill(N._mask(T, s.device), float("-inf"))
    run = torch.stack([s[..., :t0 + 64].max(-1).values for t0 in range(0, T, 64)], -1)     # running max after each tile
    step = run[..., 1:] - run[..., :-1]
    return (step > 8).any(-1).sum(-1)


def test_peaked_family_alone_reaches_the_deferred_rescale():
    """Every "peaked" causal case of ATTN_CASES with T >= 129 has, in every head, query rows whose
    running max jumps by more than 2^8 between 64-key tiles, and no "randn" row does: the coverage
    of the deferred-rescale branch belongs to that family.  At least 30 rows per head wherever
    there are rows enough past the first tile (T >= 300 at head_dim 64 / 128; measured minima per
    head: 47 at (64, 300), 68 at (64, 385), 37 at (128, 300)).  Two cases cannot reach 30 and are
    held to "every head has such a row": (64, 129) has only 65 rows with a second tile (3 to 9 of
    them jump), and (32, 200), with half the head_dim's score spread, has 20 to 29."""
    cases = [(hd, T) for hd, T, causal in N.ATTN_CASES if causal and T >= 129]
    assert sorted(cases) == [(32, 200), (64, 129), (64, 300), (64, 385), (128, 300)]
    for hd, T in cases:
        rows = _rows_with_a_jump(hd, T, "peaked")
        assert int(rows.min()) >= (30 if T >= 300 else 1), (hd, T, rows.tolist())
        assert int(_rows_with_a_jump(hd, T, "randn").max()) == 0, (hd, T)
    assert int(_rows_with_a_jump(64, 300, "peaked").min()) >= 42
