"""Error bounds for the prefill-against-a-cache kernels (csrc/kernels/attn_extend.hip).

A plain helper module like ``tests/numerics.py`` (not collected), from which it takes the unit
roundoffs, the assertion and the decode shapes.  Three parts:

* ``ref_attn_extend``: the fp64 oracle.  Query (b, t) is live iff t < n[b] and len[b] + t <
  T_max; a live query is a softmax over keys [0, len[b] + t]; its unit is that of
  ``numerics.ref_attn_fwd``, U16 (|o| + sum p |v|); a query that is not live is exactly 0.
* ``emu_attn_extend``: an fp32 evaluation on the CPU that rounds where attn_extend_k rounds:
  32-key tiles dealt to 4 waves (tile kt to wave kt % 4), per wave an online softmax against the
  running max with the row sum of the UNROUNDED p, P rounded to bf16 in front of the PV product,
  the four (m, l, O) partials merged in fp32 in wave order, one bf16 rounding at the store.
* ``EXT_LIMITS``: per head_dim, 2 x the emulation's worst err / unit against the oracle over
  ``EXT_CASES`` x ``numerics.DEC_FAMILIES`` (the 2 covers summation order and the 1-ulp hardware
  exp2 / rcp, as in ``numerics.LIMITS``).  Measured on the CPU by ``measure_limits()``; no limit
  comes from a kernel's output.
"""
from __future__ import annotations

import math

import torch

from numerics import DEC_B, DEC_FAMILIES, DEC_H, DEC_HD, LOG2E, U16, bf16_round, d, worst_ratio

EXT_SEED = 61
EXT_TILE = 32     # keys per wave tile, queries per workgroup
EXT_WAVES = 4

# (Tmax, len, T, n): len / n are ints (every row) or per-row lists; n None = T.  The smallest
# shapes where the tile (32), wave (4 x 32) and capacity edges occur.
EXT_CASES = [
    (16, 0, 1, None), (16, 0, 16, None), (16, 15, 1, None),
    (16, 10, 9, None),                       # rows past the capacity give zero
    (300, 1, 2, None), (300, 31, 33, None), (300, 32, 32, None), (300, 63, 65, None), (300, 64, 100, None),
    (300, 255, 2, None), (300, 256, 44, None), (300, 257, 43, None),
    (520, 255, 257, None), (520, 0, 300, None),
    (300, [5, 200], 40, [40, 0]),
    (300, [63, 64], 33, [33, 1]),
    (300, [290, 0], 20, [20, 20]),           # row 0 is clipped at the capacity
]


def _lim(measured, at):
    return {"measured": measured, "limit": 2 * measured, "at": at}


# o: P -> bf16 before the PV MFMA, o / l -> bf16 at the store; at = ((Tmax, len, T, n), family)
EXT_LIMITS = {
    "ext.o.hd32": _lim(0.7399, ((520, 0, 300, None), "peaked")),
    "ext.o.hd64": _lim(0.7615, ((520, 0, 300, None), "peaked")),
    "ext.o.hd128": _lim(0.8863, ((300, 64, 100, None), "peaked")),
}


def ext_limit(hd):
    return EXT_LIMITS[f"ext.o.hd{hd}"]["limit"]


def case_id(case):
    Tmax, ln, T, n = case
    f = lambda x: "-".join(map(str, x)) if isinstance(x, list) else str(x)
    return f"Tmax{Tmax}.len{f(ln)}.T{T}" + ("" if n is None else f".n{f(n)}")


def case_rows(case, B=DEC_B):
    """(lens [B], n [B]) as lists of ints."""
    Tmax, ln, T, n = case
    lens = list(ln) if isinstance(ln, list) else [ln] * B
    ns = list(n) if n is not None else [T] * B
    return lens, ns


def live_counts(lens, ns, T, Tmax):
    """Live new tokens per sequence: t < n[b] and len[b] + t < Tmax."""
    return [max(0, min(m, T, Tmax - L)) for L, m in zip(lens, ns)]


def ext_inputs(hd, case, family, device="cpu", B=DEC_B, H=DEC_H, seed=EXT_SEED):
    """(qkv packed [B T, 3 H hd], k cache, v cache [B, Tmax, H, hd]) bf16 from a seeded CPU
    generator (families as ``numerics.dec_inputs``: peaked: q and k x 3; rising: key t x
    (1 + 6 t / Tmax)).  q is ``qkv[:, :H hd]``, a view with the packed row stride."""
    Tmax, _, T, _ = case
    gen = torch.Generator().manual_seed(seed + 1000 * hd + 7 * Tmax + T)
    qkv = torch.randn(B * T, 3 * H * hd, generator=gen)
    kc = torch.randn(B, Tmax, H, hd, generator=gen)
    vc = torch.randn(B, Tmax, H, hd, generator=gen)
    if family == "peaked":
        qkv[:, : H * hd] *= 3
        kc *= 3
    elif family == "rising":
        kc *= (1 + 6 * torch.arange(Tmax).float() / Tmax).view(1, Tmax, 1, 1)
    return qkv.bfloat16().to(device), kc.bfloat16().to(device), vc.bfloat16().to(device)


def ref_attn_extend(q, kc, vc, lens, ns, T, scale):
    """q [B T, >= H hd] (the first H hd columns), caches [B, Tmax, H, hd], lens / ns lists ->
    (o [B T, H hd] fp64, unit).  Rows that are not live and cache rows nobody attends are never
    read (they may be NaN); a row that is not live is 0 with unit 0."""
    B, Tmax, H, hd = kc.shape
    o = torch.zeros(B, T, H, hd, dtype=torch.float64, device=kc.device)
    unit = torch.zeros_like(o)
    for b, (L, m) in enumerate(zip(lens, live_counts(lens, ns, T, Tmax))):
        if m == 0:
            continue
        S = L + m
        qb = d(q[b * T: b * T + m, : H * hd]).view(m, H, hd).transpose(0, 1)         # [H, m, hd]
        kb = d(kc[b, :S]).transpose(0, 1)                                            # [H, S, hd]
        vb = d(vc[b, :S]).transpose(0, 1)
        s = (qb @ kb.transpose(-1, -2)) * scale
        mask = torch.ones(m, S, dtype=torch.bool, device=s.device).triu(L + 1)
        p = torch.softmax(s.masked_fill(mask, float("-inf")), -1)
        ob = p @ vb
        o[b, :m] = ob.transpose(0, 1)
        unit[b, :m] = (U16 * (ob.abs() + p @ vb.abs())).transpose(0, 1)
    return o.view(B * T, H * hd), unit.view(B * T, H * hd)


EXT_FAULTS = ("diag_far", "diag_short", "drop_first_tile", "len0", "pad_nonzero", "norm_last_tile")


def _emu_rows(qb, kb, vb, L, m, c2, fault=None):
    """One sequence (or one head of it): qb [Hs, m, hd] live queries, kb / vb [Hs, >= L + m, hd]
    fp32 (NaN-free), cache length L -> o [Hs, m, hd] fp32 before the store's rounding."""
    Hs, _, hd = qb.shape
    S = min(L + m + (1 if fault == "diag_far" else 0), kb.size(1))
    t = torch.arange(m)[:, None]
    key = torch.arange(S)[None, :]
    lastkey = L + t + {"diag_far": 1, "diag_short": -1}.get(fault, 0)
    seen = key <= lastkey                                                            # [m, S]
    if fault == "drop_first_tile":
        seen = seen & (key >= EXT_TILE)
    ninf = torch.tensor(float("-inf"))
    mw = torch.full((EXT_WAVES, Hs, m), float("-inf"))
    lw = torch.zeros(EXT_WAVES, Hs, m)
    ln = torch.zeros(EXT_WAVES, Hs, m)          # the normaliser (differs from lw under a fault)
    ow = torch.zeros(EXT_WAVES, Hs, m, hd)
    nkt = (S - 1) // EXT_TILE + 1
    for kt in range(nkt):
        w = kt % EXT_WAVES
        k0, k1 = kt * EXT_TILE, min((kt + 1) * EXT_TILE, S)
        if k0 >= k1:
            break
        x = (qb @ kb[:, k0:k1].transpose(-1, -2)) * c2
        x = torch.where(seen[None, :, k0:k1], x, ninf)
        mnew = torch.maximum(mw[w], x.max(-1).values)
        ms = torch.where(torch.isfinite(mnew), mnew, torch.zeros_like(mnew))
        alpha = torch.exp2(mw[w] - ms)
        p = torch.exp2(x - ms[..., None])
        mw[w] = mnew
        psum = p.sum(-1)
        lw[w] = lw[w] * alpha + psum
        ln[w] = ln[w] * alpha + (0 if (fault == "norm_last_tile" and kt == nkt - 1) else psum)
        ow[w] = ow[w] * alpha[..., None] + bf16_round(p) @ vb[:, k0:k1]
    M = mw.max(0).values
    acc = torch.zeros(Hs, m, hd)
    ls = torch.zeros(Hs, m)
    for w in range(EXT_WAVES):   # wave order
        f = torch.where(torch.isfinite(mw[w]), torch.exp2(mw[w] - M), torch.zeros_like(M))
        acc = acc + f[..., None] * ow[w]
        ls = ls + f * ln[w]
    return acc * (1.0 / ls)[..., None]


def emu_attn_extend(q, kc, vc, lens, ns, T, scale, fault=None):
    """fp32 evaluation of attn_extend_k on the CPU (see the module docstring) -> o [B T, H hd]
    bf16.  ``fault`` = (name, b, h) plants one of ``EXT_FAULTS`` on one (sequence, head):
    "diag_far" (sees key len + t + 1), "diag_short" (misses its own key), "drop_first_tile" (keys
    0..31 not attended), "len0" (len[0] used for sequence b), "pad_nonzero" (a row that is not
    live left non-zero), "norm_last_tile" (the normaliser without the last key tile)."""
    B, Tmax, H, hd = kc.shape
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    o = torch.zeros(B, T, H, hd)
    lives = live_counts(lens, ns, T, Tmax)
    for b, (L, m) in enumerate(zip(lens, lives)):
        if m == 0:
            continue
        qb = q[b * T: b * T + m, : H * hd].float().view(m, H, hd).transpose(0, 1)
        kb = torch.nan_to_num(kc[b].float()).transpose(0, 1)
        vb = torch.nan_to_num(vc[b].float()).transpose(0, 1)
        o[b, :m] = _emu_rows(qb, kb, vb, L, m, c2).transpose(0, 1)
        if fault and fault[1] == b and fault[0] != "pad_nonzero":
            h = fault[2]
            Lf = lens[0] if fault[0] == "len0" else L
            mf = min(m, Tmax - Lf)
            o[b, :mf, h] = _emu_rows(qb[h:h + 1, :mf], kb[h:h + 1], vb[h:h + 1], Lf, mf, c2, fault[0])[0]
    if fault and fault[0] == "pad_nonzero":
        b, h = fault[1], fault[2]
        assert lives[b] < T, "pad_nonzero needs a row that is not live"
        o[b, lives[b], h] = 2.0 ** -20
    return o.view(B * T, H * hd).to(torch.bfloat16)


def measure_limits(hds=DEC_HD, cases=EXT_CASES, families=DEC_FAMILIES):
    """{hd: (worst err / unit of the emulation, (case, family))} on the CPU: the source of
    ``EXT_LIMITS`` (python tests/numerics_extend.py prints it)."""
    out = {}
    for hd in hds:
        worst = (0.0, None)
        for case in cases:
            Tmax, _, T, _ = case
            lens, ns = case_rows(case)
            for fam in families:
                qkv, kc, vc = ext_inputs(hd, case, fam)
                scale = 1.0 / math.sqrt(hd)
                ref, unit = ref_attn_extend(qkv, kc, vc, lens, ns, T, scale)
                w = worst_ratio(emu_attn_extend(qkv, kc, vc, lens, ns, T, scale), ref, unit)[0]
                if w > worst[0]:
                    worst = (w, (case, fam))
        out[hd] = worst
    return out


# ------------------------------------------------------------------ exact selection ----

EXT_SEL_KEYS = (0, 31, 32, 63, 64, 255, 256, "own")


def ext_selection_inputs(hd, Tmax, length, T, shift=0, device="cpu", B=DEC_B, H=DEC_H, seed=EXT_SEED):
    """The exact key-selection case, in the style of ``numerics.dec_selection_inputs``.  Query t
    is q = 16 e_0 + 16 e_(1+t) (T <= hd - 1); every key is -16 e_0.  Per (b, h) one choice of
    ``EXT_SEL_KEYS`` (those inside the prefix, rotated by ``shift``): a prefix key t* gets
    +16 e_0 (score +256 for every query), or with "own" key len + t gets +32 e_(1+t) (score +256
    for query t alone).  Every other visible key scores -256.  The trap: key len + t + 1, the
    first one query t must not see, carries +32 e_(1+t) and would score +256 for query t (and
    -256 for every later query, which sees it).  The scores differ by 512 hd^-1/2 >= 45, so
    o[b t, h] == v[b, t*, h] bit for bit.  Returns (qkv, kc, vc, tstar [B, T, H], len int32 [B])."""
    assert T <= hd - 1 and length + T <= Tmax
    gen = torch.Generator().manual_seed(seed + hd + Tmax + length + T)
    cands = [c for c in EXT_SEL_KEYS if c == "own" or c < length]
    qkv = torch.zeros(B, T, 3 * H * hd)
    kc = torch.zeros(B, Tmax, H, hd)
    kc[..., 0] = -16
    tstar = torch.zeros(B, T, H, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            c = cands[(b * H + h + shift) % len(cands)]
            for t in range(T):
                qkv[b, t, h * hd] = 16
                qkv[b, t, h * hd + 1 + t] = 16
                if length + t + 1 < Tmax:
                    kc[b, length + t + 1, h, 1 + t] += 32          # the trap of query t
                if c == "own":
                    kc[b, length + t, h, 1 + t] += 32
                    tstar[b, t, h] = length + t
                else:
                    tstar[b, t, h] = c
            if c != "own":
                kc[b, c, h, 0] = 16
    vc = torch.randn(B, Tmax, H, hd, generator=gen)
    ln = torch.full((B,), length, dtype=torch.int32)
    return (qkv.view(B * T, 3 * H * hd).bfloat16().to(device), kc.bfloat16().to(device), vc.bfloat16().to(device),
            tstar, ln.to(device))


if __name__ == "__main__":
    for hd_, (w_, at_) in measure_limits().items():
        print(f'    "ext.o.hd{hd_}": _lim({w_:.4g}, {at_}),')
