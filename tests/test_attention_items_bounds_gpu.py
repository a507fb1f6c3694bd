"""Per-element bounds of the default attention kernels past eight (batch, head) pairs, past four
query blocks and past twelve workgroups of the 2-D grid, on MI355X.

tests/test_kernel_bounds_gpu.py holds these kernels to the fp64 oracle at B 2, H 3, T <= 385: one
group of eight heads with two empty slots, pairs p <= 1, 6 and 12 workgroups at head_dim 32.  The
cases here (tests/numerics_attn.py) reach what that geometry cannot: a second and third group of
eight, a partly empty last group, the lse / delta row bases and the bias-partial rows of bh >= 8,
H that does not divide 8, pairs p >= 2 with 11-tile heavy blocks before light ones, an unpaired
middle block at nqb 9, and xcd_remap at workgroup counts that are no multiple of 8.  Every test
asserts from the launch mirror that its case reaches what it is there for; a failure names the
worst element's workgroup, pair and role (``where=``).  Limits: the existing ``LIMITS`` keys, or a
``.heads`` key of ``numerics_attn.LIMITS_ATTN`` where the CPU emulation exceeds the old key's
``measured`` at these cases; none comes from a kernel's output.
"""

import pytest
import torch

import numerics as N
import numerics_attn as A

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _run(C, case, fam, rope=False, want_ref=True):
    """The default kernels on packed-QKV views with NaN-filled outputs (an unwritten element shows)."""
    B, H, hd, T, causal = case
    q, k, v, do, pos = A.attn_inputs_bh(hd, T, fam, B, H, DEV)
    scale = hd ** -0.5
    tab = N.rope_table(512, hd).to(DEV) if rope else None
    o, lse = C.attn_fwd(q, k, v, scale, causal)
    d = torch.full((B * T, 3 * H * hd), float("nan"), device=DEV, dtype=torch.bfloat16)
    dq, dk, dv = N.packed_views(d, B, T, H, hd)
    out = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "packed": d}
    if rope:
        db = torch.full((3 * H * hd,), float("nan"), device=DEV)
        assert C.attn_bwd(do, q, k, v, o, lse, scale, causal, dq, dk, dv, pos, tab, dbias=db)
        out["dbias"] = db
    else:
        C.attn_bwd(do, q, k, v, o, lse, scale, causal, dq, dk, dv)
    # (the oracle in fp64 on the device)
    return (N.attn_refs(q, k, v, do, scale, causal, pos if rope else None, tab) if want_ref else None), out


def _check(case, fam, ref, out, names, rope=False):
    B, H, hd, T, causal = case
    for name in names:
        kern = A.default_kernel(name, hd)
        N.assert_within(out[name], ref[name], ref["unit_" + name], A.limit(A.key_for(name, hd, rope)),
                        f"attn {name} B {B} H {H} hd {hd} T {T} causal={causal} rope={rope} {fam}",
                        N.ATTN_TILES[name], None if name == "dbias" else A.where_fn(kern, name, B, H, T, causal))


ALL = ("o", "lse", "dq", "dk", "dv")


@pytest.mark.parametrize("fam", A.FAMILIES)
@pytest.mark.parametrize("case", A.HEADS_CASES, ids=A.pid)
def test_attention_bounds_past_eight_heads(C, case, fam):
    """Two and three groups of eight heads in the paired 1-D launches: a partly empty last group,
    the lse / delta row bases of bh >= 8, b = bh / H and h = bh % H with H 4, 9 and 17."""
    B, H, hd, T, causal = case
    for kern in ("fwd3", "dq3", "dkdv3"):
        r = A.reach(kern, B, H, T, causal)
        assert r["max_bh"] >= 8 and r["groups"] >= 2, "some head has bh >= 8"
        assert 0 < r["last_group_heads"] < 8 and r["empty_workgroups"] > 0, "the last group is partly empty"
    if case == (3, 4, 64, 129, True):
        assert A.reach("fwd3", B, H, T, causal)["last_group_heads"] == 4          # half empty
    if case == (1, 17, 64, 300, True):
        r = A.reach("fwd3", B, H, T, causal)
        assert r["groups"] == 3 and r["last_group_heads"] == 1 and r["unpaired"] and B == 1
    if H == 9:
        assert not A.reach("fwd3", B, H, T, causal)["h_divides_8"]
    ref, out = _run(C, case, fam)
    _check(case, fam, ref, out, ALL)


@pytest.mark.parametrize("fam", A.FAMILIES)
@pytest.mark.parametrize("case", A.HD32_CASES, ids=A.pid)
def test_attention_bounds_hd32_grid(C, case, fam):
    """head_dim 32 on the 2-D grid through xcd_remap: 20 / 40 and 27 / 45 workgroups (forward and
    dQ / dK-dV), the first non-causal head_dim-32 bound (20 / 30 workgroups)."""
    B, H, hd, T, causal = case
    counts = tuple(A.reach(kern, B, H, T, causal)["workgroups"] for kern in ("fwd", "dq", "dkdv2"))
    assert counts == {(2, 5, 32, 200, True): (20, 20, 40), (3, 3, 32, 300, True): (27, 27, 45),
                      (2, 5, 32, 130, False): (20, 20, 30)}[case]
    assert all(c not in (6, 12) for c in counts), "not the 6 and 12 workgroups of the old cases"
    assert any(c % 8 for c in counts), "a workgroup count that is no multiple of 8 (xcd_remap's remainder)"
    if case == (3, 3, 32, 300, True):
        assert all(c % 8 for c in counts)
    assert A.reach("fwd", B, H, T, causal)["max_bh"] >= 8
    ref, out = _run(C, case, fam)
    _check(case, fam, ref, out, ALL)


@pytest.mark.parametrize("case", A.BLOCKS_CASES, ids=A.pid)
def test_attention_bounds_past_four_blocks(C, case):
    """nqb 6 (pairs p = 0, 1, 2: an 11-tile heavy block before a light one) and nqb 9 (an
    unpaired middle block, one token past a block): the ring numbering and the cross-block
    prefetch run on across blocks."""
    B, H, hd, T, causal = case
    f, k3 = A.reach("fwd3", B, H, T, causal), A.reach("dkdv3", B, H, T, causal)
    assert f["blocks"] >= 5 and f["max_p"] >= 2 and k3["max_p"] >= 2, "p == 2 occurs"
    assert f["heavy_tiles"] >= 11 and k3["heavy_tiles"] >= 8, "a heavy block of more than 7 tiles before a light one"
    if T == 641:
        assert f["blocks"] == 6 and f["max_p"] == 2 and not f["unpaired"] and f["heavy_tiles"] == 11
    if T == 1025:
        assert f["blocks"] == 9 and f["unpaired"] and k3["unpaired"] and T % 128 == 1
    ref, out = _run(C, case, "peaked")
    _check(case, "peaked", ref, out, ALL)


@pytest.mark.parametrize("fam", A.FAMILIES)
@pytest.mark.parametrize("case", A.ROPE_CASES, ids=A.pid)
def test_attention_bwd_rope_dbias_bounds_past_eight_heads(C, case, fam):
    """Inverse RoPE and the QKV bias gradient: the bias-partial rows (h (BH / H) + b) n + block of
    bh >= 8, across groups and across three batches."""
    B, H, hd, T, causal = case
    r = A.reach("dkdv3", B, H, T, causal)
    assert r["max_bh"] >= 8 and r["groups"] >= 2 and B >= 2 and r["blocks"] == 2
    ref, out = _run(C, case, fam, rope=True)
    _check(case, fam, ref, out, ("dq", "dk", "dv", "dbias"), rope=True)


@pytest.mark.parametrize("case", [A.HEADS_CASES[0], A.BLOCKS_CASES[0]], ids=A.pid)
def test_attention_bwd_prefetch_hook_is_bit_identical(C, case):
    """The cold-prologue forms (attn_prefetch 0) against the default cross-block prefetch, past
    eight heads and past four blocks: the arithmetic is unchanged, so every byte is."""
    B, H, hd, T, causal = case
    assert hd == 64, "the prefetch is the head_dim-64 kernels'"
    r = A.reach("dkdv3", B, H, T, causal)
    assert r["max_bh"] >= 8 or r["max_p"] >= 2
    assert r["blocks"] >= 2 and A.reach("dq3", B, H, T, causal)["blocks"] >= 2, "a second block to prefetch for"
    _, default = _run(C, case, "peaked", want_ref=False)
    try:
        C.attn_prefetch(0)
        _, cold = _run(C, case, "peaked", want_ref=False)
    finally:
        C.attn_prefetch(3)
    assert not torch.isnan(default["packed"].float()).any()
    assert torch.equal(default["packed"], cold["packed"])
    assert torch.equal(default["o"], cold["o"]) and torch.equal(default["lse"], cold["lse"])
