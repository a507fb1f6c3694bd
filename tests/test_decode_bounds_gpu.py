"""Per-element error bounds of the decode step's kernels (csrc/kernels/decode.hip), on MI355X.

attn_decode and gemv_nt against the fp64 oracles and derived units of tests/numerics.py
(``numerics.assert_within`` at ``numerics.DERIVED``), two exact tests (key selection, GEMV
placement) in which every output is one input value bit for bit, and rope_append at head_dim 32.
tests/test_numerics.py shows on the CPU that an fp32 evaluation of the split / wave / combine
scheme attains the attention bound and that one wrong head, merge factor or normaliser does not.
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


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _blank_past(c, lens, fill):
    """The cache with every row past a sequence's attended keys (the cached ones and the token
    being decoded) set to ``fill``."""
    c = c.clone()
    L = N.dec_attended(torch.tensor(lens), c.size(1))
    for b in range(c.size(0)):
        c[b, int(L[b]):] = fill
    return c


# ------------------------------------------------------------------------ attention ----

@pytest.mark.parametrize("fam", N.DEC_FAMILIES)
@pytest.mark.parametrize("Tmax", N.DEC_TMAX)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_decode_bounds(C, hd, Tmax, fam):
    """Capacities below one wave (16), between splits (300) and a multiple of the 256-key split
    (512); lengths at the wave and split edges up to a full cache; uniform and per-row lengths; q
    as the head of the packed qkv row and contiguous; flat, near one-hot and rising score rows (the
    row max moves through waves and splits, early waves underflow).  Cache rows past each length
    are NaN: the output must be finite and equal to the run with zeros there."""
    qkv, kc, vc = N.dec_inputs(hd, Tmax, fam, DEV)
    B, H = N.DEC_B, N.DEC_H
    scale = hd ** -0.5
    qc = qkv[:, : H * hd].contiguous()
    lens = N.dec_lengths(Tmax)
    tiles = {1: (hd, 8)}
    for la, lb in zip(lens, reversed(lens)):
        for pair in ((la, lb), (la, la)):                 # per-row lengths, then the uniform form at la
            rows = pair[0] != pair[1]
            ln = _i32(list(pair)) if rows else _i32([la])
            kn, vn = _blank_past(kc, pair, NAN), _blank_past(vc, pair, NAN)
            o = C.attn_decode(qkv, kn, vn, ln, scale)
            assert o.shape == (B, H * hd) and o.dtype == torch.bfloat16
            what = f"attn_decode hd {hd} Tmax {Tmax} {fam} len {pair} {'rows' if rows else 'uniform'}"
            assert bool(torch.isfinite(o.float()).all()), what + ": read past a length"
            assert torch.equal(o, C.attn_decode(qkv, _blank_past(kc, pair, 0), _blank_past(vc, pair, 0), ln, scale)), what
            assert torch.equal(o, C.attn_decode(qc, kn, vn, ln, scale)), what + ": contiguous q"
            ref, unit = N.ref_attn_decode(qkv, kn, vn, _i32(list(pair)), scale)
            N.assert_within(o, ref, unit, N.DERIVED, what, tiles)


@pytest.mark.parametrize("Tmax,length", [(16, 7), (300, 257), (300, 305), (512, 511), (512, 512)])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_decode_selects_the_key_exactly(C, hd, Tmax, length):
    """One key per (b, h), of {0, 63, 64, 255, 256, the newest}, carries all the probability (the
    others are below e^-45): o[b, h] must be v[b, t*, h] bit for bit.  A wrong row, head or batch
    index, or a dropped wave or split, shows exactly."""
    qkv, kc, vc, tstar, ln = N.dec_selection_inputs(hd, Tmax, length, DEV)
    B, H = tstar.shape
    lens = [length] * B
    kn, vn = _blank_past(kc, lens, NAN), _blank_past(vc, lens, NAN)
    want = torch.stack([vc[b, int(tstar[b, h]), h] for b in range(B) for h in range(H)]).view(B, H * hd)
    for l in (ln, ln[:1].contiguous()):                   # per-row and uniform
        assert torch.equal(C.attn_decode(qkv, kn, vn, l, hd ** -0.5), want), (hd, Tmax, length, l.numel(), tstar.tolist())


# ----------------------------------------------------------------------------- GEMV ----

@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("Nn,K", N.GEMV_CASES)
@pytest.mark.parametrize("M", N.GEMV_M)
def test_gemv_nt_bounds(C, M, Nn, K, with_bias):
    """gemv16_k: K-waves without work (K 64), 17 K-steps over 8 waves, a partial second load batch
    (K 3072: 12 steps per wave), the 4-wave form with 9 steps per wave (N 8208, K 1056)."""
    x, w, bias = N.gemv_inputs(M, Nn, K, device=DEV)
    b = bias if with_bias else None
    assert C.gemv_nt_ok(x, w)
    y = C.gemv_nt(x, w, b)
    assert y.shape == (M, Nn) and y.dtype == torch.bfloat16
    ref, unit = N.ref_gemv(x, w, b)
    N.assert_within(y, ref, unit, N.DERIVED, f"gemv_nt {M}x{Nn}x{K} bias={with_bias}", N.GEMV_TILES)


@pytest.mark.parametrize("Nn,K", N.GEMV_SWIGLU_CASES)
@pytest.mark.parametrize("M", N.GEMV_M)
def test_gemv_nt_swiglu_bounds(C, M, Nn, K):
    x, w, bias = N.gemv_inputs(M, Nn, K, True, DEV)
    assert C.gemv_nt_ok(x, w, True)
    y = C.gemv_nt(x, w, bias, True)
    ref, unit = N.ref_gemv(x, w, bias, True)
    N.assert_within(y, ref, unit, N.DERIVED, f"gemv_nt swiglu {M}x{Nn}x{K}", N.GEMV_TILES)


@pytest.mark.parametrize("swiglu", [False, True])
def test_gemv_nt_strided_operands(C, swiglu):
    """x and w as column slices of wider tensors: lda and ldw greater than the row width (16-byte
    aligned), values beside the slices NaN."""
    M, Nn, K = 5, 48, 3072
    x, w, bias = N.gemv_inputs(M, Nn, K, swiglu, DEV)
    xw = torch.full((M, x.size(1) + 16), NAN, dtype=torch.bfloat16, device=DEV)
    ww = torch.full((Nn, K + 32), NAN, dtype=torch.bfloat16, device=DEV)
    xs, ws = xw[:, 8:8 + x.size(1)], ww[:, 16:16 + K]
    xs.copy_(x)
    ws.copy_(w)
    assert xs.stride(0) == x.size(1) + 16 and ws.stride(0) == K + 32 and C.gemv_nt_ok(xs, ws, swiglu)
    y = C.gemv_nt(xs, ws, bias, swiglu)
    ref, unit = N.ref_gemv(x, w, bias, swiglu)
    N.assert_within(y, ref, unit, N.DERIVED, f"gemv_nt strided swiglu={swiglu}", N.GEMV_TILES)
    assert torch.equal(y, C.gemv_nt(x, w, bias, swiglu))


@pytest.mark.parametrize("M,Nn,K", [(5, 100, 64), (16, 48, 3072), (3, 8208, 1056)])
def test_gemv_nt_placement_exact(C, M, Nn, K):
    """x holds one 1 per row at column pi(i), w bf16-exact integers mod 251, the bias integers mod
    5: every output is one entry of w plus its bias, so the result equals the gather exactly."""
    pi = torch.randint(0, K, (M,), generator=torch.Generator().manual_seed(60)).to(DEV)
    x = torch.zeros(M, K, device=DEV)
    x[torch.arange(M, device=DEV), pi] = 1
    x = x.bfloat16()
    w = (torch.arange(Nn * K, device=DEV, dtype=torch.float32).view(Nn, K) % 251).bfloat16()
    bias = (torch.arange(Nn, device=DEV) % 5).float()
    assert torch.equal(C.gemv_nt(x, w).float(), w.float()[:, pi].t())
    assert torch.equal(C.gemv_nt(x, w, bias).float(), w.float()[:, pi].t() + bias)


# ---------------------------------------------------------------------- rope_append ----

@pytest.mark.parametrize("lens", [[0], [299], [300], [0, 150, 300]])
def test_rope_append_head_dim_32(C, lens):
    """rope_append at head_dim 32 (two 8-pair groups per head) == rope_ + kv_append bit for bit,
    uniform and per-row; a full cache (300) is rotated and appends nothing.  With the rope_ bound
    of test_kernel_bounds_gpu this bounds it."""
    hd, H, Tmax = 32, N.DEC_H, 300
    B = 3
    g = torch.Generator().manual_seed(61 + len(lens) + lens[0])
    kc = torch.randn(B, Tmax, H, hd, generator=g).bfloat16().to(DEV)
    vc = torch.randn(B, Tmax, H, hd, generator=g).bfloat16().to(DEV)
    qkv = torch.randn(B, 3 * H * hd, generator=g).bfloat16().to(DEV)
    pos = torch.randint(0, 512, (B,), generator=g).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    ln = _i32(lens)
    a, ka, va = qkv.clone(), kc.clone(), vc.clone()
    C.rope_append(a, pos, tab, ka, va, ln)
    b, kb, vb = qkv.clone(), kc.clone(), vc.clone()
    C.rope_(b, pos, tab, 2 * H, hd, False)
    if len(lens) > 1 or lens[0] < Tmax:
        C.kv_append(b, kb, vb, ln)
    assert torch.equal(a, b) and torch.equal(ka, kb) and torch.equal(va, vb)
    ref, rmag = N.ref_rope(qkv.double(), pos, tab, 2 * H, hd)
    unit = N.unit_rope(ref, rmag)
    unit[:, 2 * H * hd:] = 0
    N.assert_within(a, ref, unit, N.DERIVED, f"rope_append hd 32 len {lens}")
    for bi in range(B):
        L = lens[bi] if len(lens) > 1 else lens[0]
        if L < Tmax:
            assert torch.equal(ka[bi, L].reshape(-1), a[bi, H * hd: 2 * H * hd])
            assert torch.equal(va[bi, L].reshape(-1), a[bi, 2 * H * hd:])
        else:
            assert torch.equal(ka[bi], kc[bi]) and torch.equal(va[bi], vc[bi])
