"""Per-element error bounds of the prefill-against-a-cache kernels (csrc/kernels/attn_extend.hip),
on MI355X.

_attn_extend against the fp64 oracle of tests/numerics_extend.py at the recorded limit (2 x the
CPU emulation's own worst err / unit; tests/test_extend_numerics.py shows on the CPU that the
emulation attains it and that planted faults do not), an exact key-selection test in which every
output row is one value row bit for bit, run-to-run identity, T = 1 beside attn_decode, and
_kv_append_chunk against a sentinel-filled cache.
"""

import pytest
import torch

import numerics as N
import numerics_extend as X

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _poison(qkv, kc, vc, lens, live, T, H, hd):
    """NaN in every q row that is not live and in every cache row past a sequence's last live key."""
    qkv, kc, vc = qkv.clone(), kc.clone(), vc.clone()
    for b, (L, m) in enumerate(zip(lens, live)):
        qkv[b * T + m: (b + 1) * T, : H * hd] = NAN
        kc[b, max(L, 0) + m:] = NAN
        vc[b, max(L, 0) + m:] = NAN
    return qkv, kc, vc


@pytest.mark.parametrize("fam", N.DEC_FAMILIES)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_extend_bounds(C, hd, fam):
    """Every (Tmax, len, T, n) case: chunks inside one tile, across tiles and waves, a diagonal on
    and beside the 32-key edges, prefixes longer than the 4-wave round, rows past the capacity and
    per-row lengths with an empty row.  Padded q rows and cache rows nobody attends are NaN: the
    live outputs must stay finite and within the bound, and rows that are not live exactly 0."""
    B, H = N.DEC_B, N.DEC_H
    scale = hd ** -0.5
    for case in X.EXT_CASES:
        Tmax, ln, T, n = case
        lens, ns = X.case_rows(case)
        live = X.live_counts(lens, ns, T, Tmax)
        qkv, kc, vc = X.ext_inputs(hd, case, fam, DEV)
        qn, kn, vn = _poison(qkv, kc, vc, lens, live, T, H, hd)
        q = qn[:, : H * hd]
        assert q.stride(0) == 3 * H * hd
        uniform = not isinstance(ln, list)
        o = C._attn_extend(q, kn, vn, _i32([ln]) if uniform else _i32(lens), None if n is None else _i32(ns), scale)
        what = f"_attn_extend hd {hd} {fam} {X.case_id(case)}"
        assert o.shape == (B * T, H * hd) and o.dtype == torch.bfloat16
        assert bool(torch.isfinite(o.float()).all()), what + ": NaN from a padded row or an unattended cache row"
        ref, unit = X.ref_attn_extend(qkv, kc, vc, lens, ns, T, scale)
        N.assert_within(o, ref, unit, X.ext_limit(hd), what, {0: (32,), 1: (hd, 32)})
        for b in range(B):
            assert not bool((o[b * T + live[b]: (b + 1) * T] != 0).any()), what + f": rows of sequence {b} that are not live"
        # the per-row form with an explicit n is the same computation
        assert torch.equal(o, C._attn_extend(q, kn, vn, _i32(lens), _i32(ns), scale)), what + ": per-row form"


@pytest.mark.parametrize("length,T,shift", [(257, 20, 0), (257, 20, 6), (40, 31, 0), (0, 9, 0)])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_extend_selects_the_key_exactly(C, hd, length, T, shift):
    """One key per query, of {0, 31, 32, 63, 64, 255, 256, the query's own row}, carries all the
    probability, and the first key the query must not see would win if it were seen: o[b t, h]
    must be v[b, t*, h] bit for bit.  A diagonal off by one, a wrong row, head or batch index, or a
    dropped tile or wave shows exactly."""
    Tmax = 300
    qkv, kc, vc, tstar, ln = X.ext_selection_inputs(hd, Tmax, length, T, shift, DEV)
    B, H = N.DEC_B, N.DEC_H
    want = torch.stack([vc[b, int(tstar[b, t, h]), h] for b in range(B) for t in range(T) for h in range(H)])
    want = want.view(B * T, H * hd)
    for l in (ln, ln[:1].contiguous()):                   # per-row and uniform
        o = C._attn_extend(qkv[:, : H * hd], kc, vc, l, None, hd ** -0.5)
        assert torch.equal(o, want), (hd, length, T, shift, l.numel(), (o != want).nonzero()[:4].tolist())


def test_attn_extend_is_deterministic(C):
    case = (520, 255, 257, None)
    for hd in N.DEC_HD:
        qkv, kc, vc = X.ext_inputs(hd, case, "randn", DEV)
        a = C._attn_extend(qkv[:, : N.DEC_H * hd], kc, vc, _i32([255]), None, hd ** -0.5)
        b = C._attn_extend(qkv[:, : N.DEC_H * hd], kc, vc, _i32([255]), None, hd ** -0.5)
        assert torch.equal(a, b)


@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_extend_one_token_beside_attn_decode(C, hd):
    """T = 1 is the decode problem: _attn_extend within its limit and attn_decode within its
    derived unit of oracles that agree with each other."""
    Tmax, fam = 300, "rising"
    qkv, kc, vc = N.dec_inputs(hd, Tmax, fam, DEV)
    H, scale = N.DEC_H, hd ** -0.5
    for pair in ((0, 299), (63, 64), (256, 31)):
        ln = _i32(list(pair))
        ref, unit = X.ref_attn_extend(qkv, kc, vc, list(pair), [1, 1], 1, scale)
        dref, dunit = N.ref_attn_decode(qkv, kc, vc, ln, scale)
        assert torch.allclose(ref, dref, rtol=1e-12, atol=1e-12)
        N.assert_within(C._attn_extend(qkv[:, : H * hd], kc, vc, ln, None, scale), ref, unit, X.ext_limit(hd),
                        f"_attn_extend T 1 hd {hd} len {pair}")
        N.assert_within(C.attn_decode(qkv, kc, vc, ln, scale), dref, dunit, N.DERIVED, f"attn_decode hd {hd} len {pair}")


@pytest.mark.parametrize("lens,ns,T", [([10], None, 40), ([5, 200, 290], [40, 0, 20], 40), ([0, 300, 299], [3, 3, 3], 3),
                                       ([7, 7, 7], [1, 40, 17], 40)])
def test_kv_append_chunk_is_exact(C, lens, ns, T):
    """Rows len[b] + t, t < n[b], inside the capacity, equal the k / v parts of the packed rows;
    every other element of the sentinel-filled caches is untouched (n 0, a full cache, a row
    clipped at the capacity, the uniform form without n)."""
    hd, H, Tmax, B = 32, N.DEC_H, 300, 3
    g = torch.Generator().manual_seed(71 + T + lens[0])
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16().to(DEV)
    kc = torch.full((B, Tmax, H, hd), -7.0, dtype=torch.bfloat16, device=DEV)
    vc = torch.full_like(kc, -9.0)
    ke, ve = kc.clone(), vc.clone()
    rows = lens * B if len(lens) == 1 else lens
    for b, (L, m) in enumerate(zip(rows, X.live_counts(rows, ns or [T] * B, T, Tmax))):
        ke[b, L:L + m] = qkv[b * T: b * T + m, H * hd: 2 * H * hd].view(m, H, hd)
        ve[b, L:L + m] = qkv[b * T: b * T + m, 2 * H * hd:].view(m, H, hd)
    C._kv_append_chunk(qkv, kc, vc, _i32(lens), None if ns is None else _i32(ns))
    assert torch.equal(kc, ke) and torch.equal(vc, ve)
