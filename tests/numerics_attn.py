"""The attention launches mirrored in Python, the variants' rounding, and what the many-head tests build on them.

A plain helper module (not a conftest, not collected, no GPU import), beside tests/numerics.py:

* **The launch mirror.**  Two launch forms carry every attention kernel:

  - the *paired 1-D* form (``attn_fwd3_k``, ``attn_bwd_dq3_k``: 128-query blocks;
    ``attn_bwd_dkdv3_k``: 128-key blocks; ``attn_bwd_dkdv4_k``, ``attn_bwd_fused_k``: 256-key
    blocks).  ``items = ceil(BH / 8) * 8 * NP`` workgroups, ``NP = (blocks + 1) / 2``; workgroup
    ``it`` serves head ``bh = (it >> 3) / NP * 8 + (it & 7)`` and pair ``p = (it >> 3) % NP``: the
    blocks ``p`` and ``blocks - 1 - p`` (one block when they coincide: the unpaired middle one).
    ``bh >= BH`` is an empty slot.  The query-block kernels run block ``blocks - 1 - p`` first, the
    key-block kernels block ``p`` first; in both that first block is the *heavy* one under the
    causal mask (it sweeps the more tiles).
  - the *2-D* form (``attn_fwd_k``, ``attn_bwd_dq_k``: ``gx = ceil(T / 128)``, heaviest query
    block first; ``attn_bwd_dkdv2_k``: ``gx = ceil(T / 64)``), grid ``(gx, BH)``, workgroup
    ``x + gx * y`` mapped through ``xcd_remap`` to ``xl``; ``bh = xl / gx``, block from ``xl % gx``.

  ``paired_launch`` / ``grid_launch`` list every workgroup of a launch; ``locate`` gives the
  ``Where`` of an output element (workgroup, workgroup % 8, pair, role, tiles the block runs);
  ``where_fn`` is the ``where=`` callable of ``numerics.assert_within``; ``reach`` summarises what
  a case reaches (head groups, empty slots, largest pair, unpaired block, workgroup count), which
  every GPU test asserts so a later change of shape cannot silently empty it.

* **Inputs**: ``attn_inputs_bh``: ``numerics.attn_inputs``' recipe with B and H in the seed
  (B 2, H 3 gives the existing values).

* **Variant emulations** (``emu_attn_fwd`` / ``emu_attn_bwd``): copies of the emulations of
  tests/numerics.py with keyword flags, bit-identical to them with every flag off
  (tests/test_numerics_attn.py asserts it).  The rounding points, read from the kernels:

  - ``rsm`` (forward impl 6, ``attn_fwd3_k<HD, 0, true>``): the row sum is one more MFMA over the
    bf16 P operand, ``osum = MFMA32(ones, pk[k4], osum)`` with ``pk[k4][j] = (bf16)s[..]`` and
    ``ls = RSM ? osum[0] : pair_sum(lsum)``: l sums bf16(p).
  - ``mf`` (forward impl 8, ``attn_fwd3_k<HD, 0, false, true>``):
    ``qf[ks][j] = (bf16)((float)qf[ks][j] * c2)``: Q' = bf16(Q c2) feeds the score MFMA and
    p = exp2(s) takes no further multiply; the running max enters as a B column ``qx[0] =
    (bf16)(-m)`` with ``mnew = (float)(bf16)(m + mr)``: m is bf16-exact, a shift common to p and
    l, no error.
  - ``ksc`` (backward impls 9 and 7): ``attn_bwd_dkdv3_k<HD, DIAG, true>`` and
    ``attn_bwd_dkdv4_k`` scale their K operand once per key block, ``kf[ks][j] =
    (bf16)((float)kf[ks][j] * c2)``, and K' feeds ONLY S = Q K'^T there (``sc = MFMA32(fa, kf,
    sc)``): dP = dO V^T, dV^T += dO^T P and dK^T += Q^T dS do not read K.  ``attn_bwd_dq3_k<HD,
    true>`` does NOT scale K: its KSC switches only the row constant it writes for the dK/dV
    kernel (``LSN_OUT = KSC ? -lse_r * kLog2e : -lse_r / scale``); its own p is
    ``exp2(fmaf(sc, c2, lc))`` from the unscaled K in both forms.  So ``ksc`` changes dk and dv
    and leaves dq bit-identical to the default pair's.
  - Same rounding points as the default kernels, so the existing units and ``LIMITS`` keys hold:
    forward impl 1 (``attn_fwd_k``: ``ps += pv`` sums the unrounded p, ``pack_pt`` rounds P for
    the PV MFMA, ``(bf16)(o * inv)`` at the store); backward impl 2 (``attn_bwd_dq_k`` /
    ``attn_bwd_dkdv2_k``: ``s *= dp`` then ``pack_pt`` = dS rounded before the scale, ``pack_pt``
    of p for dV, ``dq *= scale`` / ``dk *= scale`` after the MFMAs, one rounding at the store);
    the fused backward impl 6 (``attn_bwd_fused_k``: ``pp = (bf16)sc``, ``pd = (bf16)vmulf(sc,
    dp)``, dS shared through LDS as that bf16, fp32 dQ partials added in key-block order by
    ``attn_dq_reduce_k``, which scales, rotates and rounds once: ``v[j] = (bf16)x[dt][j]``).

* **Variant units** (``variant_units``): the first-order term each added rounding contributes,
  derived in its docstring, on top of the units of tests/numerics.py.

* **Limits** (``LIMITS_ATTN``): the module rule of tests/numerics.py and nothing else: a limit
  that cannot be derived is 2 x the matching emulation's worst err / unit against the fp64 oracle
  over the cases the GPU tests run, measured on the CPU (tests/test_numerics_attn.py holds every
  emulation to its ``measured``).  ``.heads`` keys: the default rounding at the many-head /
  many-block cases, only for the groups whose emulation exceeds the ``measured`` of the existing
  key there (the existing entries are not touched); every other group keeps its existing key.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

import numerics as N
from numerics_items import cdiv, xcd_remap

U16, U32 = N.U16, N.U32

# ============================================================================ mirror ====

# kernel: (launch form, block size, what a block holds: queries "q" or keys "k")
KERNELS = {
    "fwd3": ("paired", 128, "q"), "dq3": ("paired", 128, "q"),
    "dkdv3": ("paired", 128, "k"), "dkdv4": ("paired", 256, "k"), "fused": ("paired", 256, "k"),
    "fwd": ("grid", 128, "q"), "dq": ("grid", 128, "q"), "dkdv2": ("grid", 64, "k"),
}
ROLES = ("heavy", "light", "unpaired", "single")

# wg: blockIdx (linear: x + gx * y on the 2-D grid); xcd: wg % 8 (workgroups are dealt to the
# eight XCDs round-robin); bh: the (batch, head) pair; p: the pair (-1 on the 2-D grid); block;
# role: index of ROLES; order: the block's position in its workgroup's walk; tiles: the 64-key
# (query-block kernels) or 64-query (key-block kernels) tiles the block sweeps
Where = namedtuple("Where", "wg xcd bh p block role order tiles")


def n_blocks(T, block):
    return cdiv(T, block)


def block_tiles(blk, T, causal, block, by):
    """Tiles of 64 a block sweeps: a query block its keys [0, min(T, (blk + 1) block)) under the
    causal mask (``nkv``), a key block the queries from (blk block / 64) 64 on (``nq``); all of T
    without the mask."""
    if by == "q":
        return cdiv(min(T, (blk + 1) * block) if causal else T, 64)
    return cdiv(T - ((blk * block) // 64 * 64 if causal else 0), 64)


def paired_grid(BH, T, block):
    """The launchers' `items`: (B * H + 7) / 8 * 8 * ((blocks + 1) / 2)."""
    return cdiv(BH, 8) * 8 * ((n_blocks(T, block) + 1) // 2)


def paired_launch(BH, T, causal, block, by):
    """Every workgroup of the paired 1-D launch, in blockIdx order: (it, bh, p, [Where, ...]);
    an empty slot (bh >= BH) has no blocks."""
    nb = n_blocks(T, block)
    NP = (nb + 1) // 2
    out = []
    for it in range(paired_grid(BH, T, block)):
        bh, p = (it >> 3) // NP * 8 + (it & 7), (it >> 3) % NP
        blocks = []
        if bh < BH:
            far = nb - 1 - p
            walk = [far] if far == p else ([far, p] if by == "q" else [p, far])
            for order, blk in enumerate(walk):
                role = 2 if far == p else (0 if order == 0 else 1)
                blocks.append(Where(it, it & 7, bh, p, blk, role, order, block_tiles(blk, T, causal, block, by)))
        out.append((it, bh, p, blocks))
    return out


def grid_launch(BH, T, causal, block, by, remap=xcd_remap):
    """Every workgroup of the 2-D launch, in linear blockIdx order x + gx * y: one Where each
    (p = -1, role "single").  ``remap``: the planted faults pass a wrong one."""
    gx = n_blocks(T, block)
    nwg = gx * BH
    out = []
    for wg in range(nwg):
        xl = remap(wg, nwg)
        bh, r = xl // gx, xl % gx
        blk = gx - 1 - r if by == "q" else r
        out.append(Where(wg, wg % 8, bh, -1, blk, 3, 0, block_tiles(blk, T, causal, block, by)))
    return out


def launch(kernel, BH, T, causal, remap=xcd_remap):
    """All Where of a kernel's launch (empty slots carry none)."""
    form, block, by = KERNELS[kernel]
    if form == "paired":
        return [w for _, _, _, blocks in paired_launch(BH, T, causal, block, by) for w in blocks]
    return grid_launch(BH, T, causal, block, by, remap)


def grid_size(kernel, BH, T):
    form, block, _ = KERNELS[kernel]
    return paired_grid(BH, T, block) if form == "paired" else n_blocks(T, block) * BH


@functools.lru_cache(maxsize=None)
def _inverse_remap(nwg):
    inv = [0] * nwg
    for wg in range(nwg):
        inv[xcd_remap(wg, nwg)] = wg
    return tuple(inv)


def locate(kernel, b, t, h, B, H, T, causal):
    """The Where of output element (b, t, h) of ``kernel`` (t: the query of o / lse / dq, the key
    of dk / dv), from the index arithmetic alone (the 2-D form inverts xcd_remap over the launch's
    gx * B * H workgroups)."""
    form, block, by = KERNELS[kernel]
    bh, blk, nb = b * H + h, t // block, n_blocks(T, block)
    tiles = block_tiles(blk, T, causal, block, by)
    if form == "paired":
        NP = (nb + 1) // 2
        p = min(blk, nb - 1 - blk)
        it = ((bh // 8) * NP + p) * 8 + bh % 8
        first = nb - 1 - p if by == "q" else p
        role = 2 if nb - 1 - p == p else (0 if blk == first else 1)
        return Where(it, it & 7, bh, p, blk, role, 0 if blk == first else 1, tiles)
    wg = _inverse_remap(nb * B * H)[bh * nb + (nb - 1 - blk if by == "q" else blk)]
    return Where(wg, wg % 8, bh, -1, blk, 3, 0, tiles)


def default_kernel(name, hd):
    """The kernel that writes output ``name`` under the default impl."""
    big = hd in (64, 128)
    if name in ("o", "lse"):
        return "fwd3" if big else "fwd"
    if name == "dq":
        return "dq3" if big else "dq"
    return "dkdv3" if big else "dkdv2"


def where_fn(kernel, name, B, H, T, causal):
    """``where=`` of numerics.assert_within: names the worst element's workgroup, XCD slot, pair,
    role and tile count.  o / dq / dk / dv are (B, T, H, hd), lse (B, H, T)."""
    def where(idx):
        b, t, h = (idx[0], idx[2], idx[1]) if name == "lse" else (idx[0], idx[1], idx[2])
        w = locate(kernel, b, t, h, B, H, T, causal)
        return (f"{kernel}: workgroup {w.wg} (% 8 = {w.xcd}), bh {w.bh}, pair {w.p}, block {w.block} "
                f"({ROLES[w.role]}, {'second' if w.order else 'first'} in its workgroup), {w.tiles} tiles")
    return where


def reach(kernel, B, H, T, causal):
    """What a case reaches in ``kernel``'s launch, for the tests' reachability assertions."""
    BH = B * H
    ws = launch(kernel, BH, T, causal)
    block = KERNELS[kernel][1]
    grid = grid_size(kernel, BH, T)
    heavy = [w for w in ws if w.role == 0]
    return {
        "workgroups": grid,
        "groups": cdiv(BH, 8),                                    # groups of eight heads
        "last_group_heads": BH - 8 * (cdiv(BH, 8) - 1),           # < 8: the last group is partly empty
        "empty_workgroups": grid - len({w.wg for w in ws}),
        "max_bh": max(w.bh for w in ws),
        "blocks": n_blocks(T, block),
        "max_p": max(w.p for w in ws),
        "unpaired": any(w.role == 2 for w in ws),
        "max_tiles": max(w.tiles for w in ws),
        "heavy_tiles": max((w.tiles for w in heavy), default=0),
        "h_divides_8": 8 % H == 0,
    }


# ============================================================================ inputs ====

def attn_inputs_bh(hd, T, family, B, H, device="cpu", seed=N.ATTN_SEED):
    """``numerics.attn_inputs`` with B and H in the seed: packed-QKV views, do and RoPE positions
    from a CPU generator.  (B 2, H 3) is exactly ``numerics.attn_inputs(hd, T, family)``, so the
    existing cases keep their values."""
    return N.attn_inputs(hd, T, family, device, B, H, seed + 7919 * (B - 2) + 104729 * (H - 3))


# ======================================================================== emulations ====

def _lagging_max(x, tile=64, defer=8.0):
    """The forward kernels' running max (log2 units) over 64-key tiles of the masked scores x:
    per element the m its tile's p was taken against, and the row's last m.  m starts at -inf (the
    first tile sets it: every row has key 0) and moves to a tile's max only when that exceeds it
    by more than ``defer``."""
    m = torch.full(x.shape[:-1] + (1,), float("-inf"))
    m_at = torch.empty_like(x)
    for t0 in range(0, x.size(-1), tile):
        mx = x[..., t0:t0 + tile].max(-1, keepdim=True).values
        m = torch.where(mx > m + defer, mx, m)
        m_at[..., t0:t0 + tile] = m
    return m_at, m


def emu_attn_fwd(q, k, v, scale, causal, rsm=False, mf=False, drop=None):
    """``numerics.emu_attn_fwd`` (bit-identical with the flags off) with the variants' rounding:

    ``rsm`` (attn_fwd3_k RSM, forward impl 6): `osum = MFMA32(ones, pk[k4], osum)` with
    `pk[k4][j] = (bf16)s[k4 >> 1][8 * (k4 & 1) + j]`: l is the sum of the bf16-ROUNDED p (the
    MFMA accumulates in fp32), and `ls = RSM ? osum[0] : pair_sum(lsum)` feeds 1 / l and lse.
    Here the deferred rescale is no longer a common factor: p is rounded against the LAGGING max
    (`if (ballot(mx * c2 > m + kDefer))`: m moves only when a 64-key tile's max exceeds it by
    2^8, and the first tile sets it), so in a near one-hot row the dominant p is some 2^x <= 2^8
    with a full rounding error instead of exactly 1.  ``_lagging_max`` follows the kernel's m per
    tile; earlier tiles' rounded p are carried by the exact-in-fp32 factors exp2(m_old - m_new)
    (`osum *= alpha`).

    ``mf`` (attn_fwd3_k MF, forward impl 8): `qf[ks][j] = (bf16)((float)qf[ks][j] * c2)`:
    Q' = bf16(Q c2) is the score MFMA's operand and `e0 = exp2f(MF ? s[kh][i] : fmaf(..))` takes
    the accumulator as it is; `mnew = (float)(bf16)(m + mr)`, `qx[0] = (bf16)(-m)`: the max is
    subtracted inside the MFMA as a bf16-exact value (here: the row max rounded to bf16; any
    common shift of p and l cancels in o and in lse).

    ``drop``: a bool mask of scores removed on top of the causal mask (the planted faults)."""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(N.LOG2E, dtype=torch.float32)
    if mf:
        qf = N.bf16_round(qf * c2)
    sc = torch.zeros(qf.shape[:-1] + (kf.size(-2),))
    for i in range(qf.size(-1)):
        sc += qf[..., :, None, i] * kf[..., None, :, i]
    x = sc if mf else sc * c2
    if causal:
        x = x.masked_fill(N._mask(x.size(-1), x.device), float("-inf"))
    if drop is not None:
        x = x.masked_fill(drop, float("-inf"))
    if rsm:
        m_at, m = _lagging_max(x)
        pr = N.bf16_round(torch.exp2(x - m_at)) * torch.exp2(m_at - m)
        l = torch.zeros_like(m)
        for j in range(pr.size(-1)):
            l += pr[..., j:j + 1]
        o = (pr @ vf) * (1.0 / l)
        lse = ((m + torch.log2(l)) * torch.tensor(N.LN2, dtype=torch.float32)).squeeze(-1)
        return o.transpose(1, 2).to(torch.bfloat16), lse
    m = x.max(-1, keepdim=True).values
    if mf:
        m = N.bf16_round(m)
    p = torch.exp2(x - m)
    l = torch.zeros_like(m)
    for j in range(p.size(-1)):
        l += p[..., j:j + 1]
    o = (N.bf16_round(p) @ vf) * (1.0 / l)
    lse = ((m + torch.log2(l)) * torch.tensor(N.LN2, dtype=torch.float32)).squeeze(-1)
    return o.transpose(1, 2).to(torch.bfloat16), lse


def emu_attn_bwd(do, q, k, v, o, lse, scale, causal, pos=None, tab=None, ksc=False, kconst=None):
    """``numerics.emu_attn_bwd`` (bit-identical with the flags off) with the K pre-scale:

    ``ksc`` (attn_bwd_dkdv3_k KSC / attn_bwd_dkdv4_k, backward impls 9 / 7):
    `kf[ks][j] = (bf16)((float)kf[ks][j] * c2)`: K' = bf16(K c2) is the B operand of S = Q K'^T in
    the dK/dV kernel only, whose accumulator starts at LSN = -lse log2 e and goes to exp2 as it is
    (`exp2f(KSC ? sc[0][i] : sc[0][i] * c2)`); dk and dv use that p.  dq comes from
    attn_bwd_dq3_k, which never scales K (its KSC switches `LSN_OUT` only), so dq is the default's.

    ``kconst`` = (o, lse) the dK/dV kernel's row constants (delta, lse) are taken from instead
    (the planted faults)."""
    qf, kf, vf, dof, of = (t.float().transpose(1, 2) for t in (q, k, v, do, o))
    L2E = torch.tensor(N.LOG2E, dtype=torch.float32)
    c2 = torch.tensor(scale, dtype=torch.float32) * L2E
    x = (qf @ kf.transpose(-1, -2)) * c2 - (lse.float() * L2E)[..., None]
    p = torch.exp2(x)
    if causal:
        p = p.masked_fill(N._mask(p.size(-1), p.device), 0.0)
    delta = (dof * of).sum(-1, keepdim=True)
    dp = dof @ vf.transpose(-1, -2) - delta
    ds = N.bf16_round(p * dp)
    pk, dsk = p, ds
    if ksc or kconst is not None:
        lse_k, dpk = lse, dp
        if kconst is not None:
            lse_k = kconst[1]
            dpk = dof @ vf.transpose(-1, -2) - (dof * kconst[0].float().transpose(1, 2)).sum(-1, keepdim=True)
        if ksc:
            xk = qf @ N.bf16_round(kf * c2).transpose(-1, -2) - (lse_k.float() * L2E)[..., None]
        else:
            xk = (qf @ kf.transpose(-1, -2)) * c2 - (lse_k.float() * L2E)[..., None]
        pk = torch.exp2(xk)
        if causal:
            pk = pk.masked_fill(N._mask(pk.size(-1), pk.device), 0.0)
        dsk = N.bf16_round(pk * dpk)
    dv = N.bf16_round(pk).transpose(-1, -2) @ dof
    dq = (ds @ kf) * scale
    dk = (dsk.transpose(-1, -2) @ qf) * scale
    dq, dk, dv = (t.transpose(1, 2) for t in (dq, dk, dv))
    if pos is not None:
        B, T, H, hd = dq.shape
        h2 = hd // 2
        t = tab.float()[pos.long()].view(B, T, 1, hd)
        c, s = t[..., :h2], t[..., h2:]
        rot = lambda y: torch.cat([y[..., :h2] * c + y[..., h2:] * s, y[..., h2:] * c - y[..., :h2] * s], -1)
        dq, dk = rot(dq), rot(dk)
    dbias = torch.cat([t.sum((0, 1)).reshape(-1) for t in (dq, dk, dv)])
    return dq.to(torch.bfloat16), dk.to(torch.bfloat16), dv.to(torch.bfloat16), dbias


# ============================================================================= units ====

def variant_units(r, q, k, v, do, scale, causal, variant, pos=None, tab=None):
    """A copy of the oracle dict ``r`` (numerics.attn_refs; left unchanged) whose units carry the
    variant's extra first-order term.  With eps_ij = U16 smag_ij, smag = scale |q| . |k| (the
    score's absolute-value product, as ref_attn_fwd builds it):

    ``rsm``: each addend of l is rounded, |bf16(p) - p| <= U16 p, so |dl| <= U16 l and
    |d lse| = |d ln l| <= U16 to first order: unit_lse += U16.  (o = sum bf16(p) v / sum bf16(p)
    keeps its unit: U16 (|o| + P |v|) already bounds a U16-relative change of every p and of l.)

    ``mf``: Q' = bf16(Q c2) moves each score by |ds_ij| <= U16 scale sum_d |q_id| |k_jd| = eps_ij
    (natural-log units).  lse = ln sum exp s: d lse = sum_j p_j ds_j, so unit_lse += ebar_i =
    sum_j p_ij eps_ij.  p_j = exp(s_j - lse): dp_j = p_j (ds_j - d lse), |dp_j| <= p_j (eps_j +
    ebar); o = sum_j p_j v_j: unit_o += sum_j p_j eps_j |v_j| + ebar sum_j p_j |v_j|.

    ``ksc``: K' = bf16(K c2) in the dK/dV kernel's S only, with lse given (no renormalisation):
    dp_ij = p_ij ds_ij, |dp_ij| <= p_ij eps_ij.  dv = P^T dO: unit_dv += (P eps)^T |dO|.
    dS = p (dP - delta): |d dS_ij| <= eps_ij |dS_ij|; dk = scale dS^T Q: unit_dk += scale
    (eps |dS|)^T |Q| (rotated with |cos|, |sin| under the inverse RoPE).  dq: unchanged (the dQ
    kernel does not scale K).  dbias sums its addends' units: the dk and dv terms are added."""
    out = dict(r)
    if variant is None:
        return out
    qf, kf, vf, dof = (N._bhtd(t) for t in (q, k, v, do))
    p = r["p"]
    eps = U16 * (qf.abs() @ kf.abs().transpose(-1, -2)) * scale
    if variant == "rsm":
        out["unit_lse"] = r["unit_lse"] + U16
    elif variant == "mf":
        w = p * eps
        ebar = w.sum(-1)
        out["unit_lse"] = r["unit_lse"] + ebar
        out["unit_o"] = r["unit_o"] + (w @ vf.abs() + ebar[..., None] * (p @ vf.abs())).transpose(1, 2)
    elif variant == "ksc":
        of = r["o"].transpose(1, 2)
        ds = p * (dof @ vf.transpose(-1, -2) - (dof * of).sum(-1, keepdim=True))
        add_dv = ((p * eps).transpose(-1, -2) @ dof.abs()).transpose(1, 2)
        add_dk = (scale * ((eps * ds.abs()).transpose(-1, -2) @ qf.abs())).transpose(1, 2)
        if pos is not None:
            add_dk = N._rot_bthd(add_dk, pos, tab, True)
        out["unit_dv"] = r["unit_dv"] + add_dv
        out["unit_dk"] = r["unit_dk"] + add_dk
        zero = torch.zeros_like(add_dk).sum((0, 1)).reshape(-1)
        out["unit_dbias"] = r["unit_dbias"] + torch.cat([zero, add_dk.sum((0, 1)).reshape(-1), add_dv.sum((0, 1)).reshape(-1)])
    else:
        raise ValueError(variant)
    return out


# ============================================================================= cases ====
# (B, H, hd, T, causal), shared by the GPU tests and the CPU measurement.

HEADS_CASES = [(3, 4, 64, 129, True), (1, 17, 64, 300, True), (2, 9, 128, 129, True), (3, 4, 64, 130, False),
               (2, 9, 128, 130, False)]
HD32_CASES = [(2, 5, 32, 200, True), (3, 3, 32, 300, True), (2, 5, 32, 130, False)]
BLOCKS_CASES = [(1, 2, 64, 641, True), (1, 2, 64, 1025, True), (1, 1, 128, 641, True), (1, 2, 64, 641, False)]
ROPE_CASES = [(3, 4, 64, 129, True), (2, 9, 128, 129, True)]
FAMILIES = list(N.ATTN_FAMILIES)


def pid(x):
    """Readable pytest ids: a case tuple as B3H4hd64T129c (c causal, n not), None as "default"."""
    if isinstance(x, tuple) and all(isinstance(e, str) for e in x):
        return "+".join(x)
    if isinstance(x, tuple) and len(x) == 5:
        return "B%dH%dhd%dT%d%s" % (x[:4] + ("c" if x[4] else "n",))
    if isinstance(x, bool):
        return "rope" if x else "norope"
    return "default" if x is None else str(x)


def items_cases():
    """(case, family, rope) of tests/test_attention_items_bounds_gpu.py ("peaked" only past four blocks)."""
    return ([(c, f, False) for c in HEADS_CASES + HD32_CASES for f in FAMILIES]
            + [(c, "peaked", False) for c in BLOCKS_CASES] + [(c, f, True) for c in ROPE_CASES for f in FAMILIES])


def variant_shapes(hd, wide):
    """The variants' shapes; ``wide``: the 256-key-block kernels (head_dim 64) also past four blocks."""
    s = [(2, 3, hd, 300, True), (2, 3, hd, 130, False), (3, 4, hd, 129, True)]
    return s + [(1, 2, 64, 641, True)] if wide else s


# forward: (impl, variant, kernel, head_dims); backward: (impl, variant, dq kernel, dk/dv kernel, head_dims)
FWD_VARIANTS = [(1, None, "fwd", (64, 128)), (6, "rsm", "fwd3", (64, 128)), (8, "mf", "fwd3", (64, 128))]
BWD_VARIANTS = [(2, None, "dq", "dkdv2", (64, 128)), (6, None, "fused", "fused", (64,)),
                (7, "ksc", "dq3", "dkdv4", (64,)), (9, "ksc", "dq3", "dkdv3", (64, 128))]


def fwd_variant_cases():
    return [(impl, var, kern, c, f) for impl, var, kern, hds in FWD_VARIANTS for hd in hds
            for c in variant_shapes(hd, False) for f in FAMILIES]


def bwd_variant_cases():
    return [(impl, var, kq, kk, c, f, rope) for impl, var, kq, kk, hds in BWD_VARIANTS for hd in hds
            for c in variant_shapes(hd, impl in (6, 7)) for f in FAMILIES for rope in (False, True)]


# ============================================================================ limits ====
# Measured on the CPU (tests/test_numerics_attn.py: every emulation against the fp64 oracle at
# every case the two GPU files run): `measured` is the emulation's worst err / unit, `limit` =
# 2 x measured, `at` = (B, H, hd, T, causal, family, rope) of the worst case.
#   .heads: the default rounding (default impl, forward impl 1, backward impls 2 and 6) at the
#           cases of this module, for the groups that exceed the existing key's `measured` there
#   .rsm / .mf / .ksc: the variants' emulations against the variants' units
_lim = N._lim
LIMITS_ATTN = {
    # the default rounding past eight heads / four blocks / on the 2-D grid past 12 workgroups
    "attn.dbias.hd128.rope.heads": _lim(0.05087, (2, 9, 128, 129, True, 'peaked', True)),
    "attn.dbias.hd64.rope.heads": _lim(0.03261, (2, 3, 64, 130, False, 'peaked', True)),
    "attn.dk.hd128.heads": _lim(0.6527, (2, 9, 128, 129, True, 'randn', False)),
    "attn.dk.hd128.rope.heads": _lim(0.6753, (2, 9, 128, 129, True, 'randn', True)),
    "attn.dk.hd32.heads": _lim(0.7614, (3, 3, 32, 300, True, 'randn', False)),
    "attn.dk.hd64.heads": _lim(0.7078, (1, 17, 64, 300, True, 'randn', False)),
    "attn.dq.hd128.heads": _lim(0.4525, (3, 4, 128, 129, True, 'peaked', False)),
    "attn.dq.hd32.heads": _lim(0.5697, (3, 3, 32, 300, True, 'peaked', False)),
    "attn.dq.hd64.rope.heads": _lim(0.4482, (1, 2, 64, 641, True, 'peaked', True)),
    "attn.dv.hd32.heads": _lim(0.9036, (3, 3, 32, 300, True, 'peaked', False)),
    "attn.dv.hd64.heads": _lim(0.9597, (1, 17, 64, 300, True, 'peaked', False)),
    "attn.lse.hd32.heads": _lim(0.1457, (3, 3, 32, 300, True, 'randn', False)),
    "attn.o.hd128.heads": _lim(0.8551, (3, 4, 128, 129, True, 'peaked', False)),
    "attn.o.hd32.heads": _lim(0.7991, (2, 5, 32, 200, True, 'peaked', False)),
    # forward impl 6: l sums bf16(p), rounded against the lagging max (unit_lse + U16)
    "attn.lse.hd128.rsm": _lim(0.7655, (2, 3, 128, 300, True, 'peaked', False)),
    "attn.lse.hd64.rsm": _lim(0.879, (2, 3, 64, 300, True, 'peaked', False)),
    "attn.o.hd128.rsm": _lim(0.8042, (2, 3, 128, 300, True, 'peaked', False)),
    "attn.o.hd64.rsm": _lim(0.9858, (2, 3, 64, 300, True, 'peaked', False)),
    # forward impl 8: Q' = bf16(Q c2) (unit_o, unit_lse + the score perturbation's terms)
    "attn.lse.hd128.mf": _lim(0.2088, (3, 4, 128, 129, True, 'peaked', False)),
    "attn.lse.hd64.mf": _lim(0.2957, (2, 3, 64, 130, False, 'peaked', False)),
    "attn.o.hd128.mf": _lim(0.1137, (2, 3, 128, 130, False, 'peaked', False)),
    "attn.o.hd64.mf": _lim(0.1581, (2, 3, 64, 300, True, 'randn', False)),
    # backward impls 7 / 9: K' = bf16(K c2) in the dK/dV kernel's S (unit_dk, unit_dv, unit_dbias + its terms)
    "attn.dbias.hd128.rope.ksc": _lim(0.01132, (2, 3, 128, 130, False, 'peaked', True)),
    "attn.dbias.hd64.rope.ksc": _lim(0.01873, (2, 3, 64, 130, False, 'peaked', True)),
    "attn.dk.hd128.ksc": _lim(0.2368, (3, 4, 128, 129, True, 'randn', False)),
    "attn.dk.hd128.rope.ksc": _lim(0.2357, (3, 4, 128, 129, True, 'randn', True)),
    "attn.dk.hd64.ksc": _lim(0.2783, (3, 4, 64, 129, True, 'randn', False)),
    "attn.dk.hd64.rope.ksc": _lim(0.2654, (2, 3, 64, 300, True, 'peaked', True)),
    "attn.dv.hd128.ksc": _lim(0.2673, (3, 4, 128, 129, True, 'randn', False)),
    "attn.dv.hd64.ksc": _lim(0.3258, (3, 4, 64, 129, True, 'randn', False)),
}


def limit(key):
    return (LIMITS_ATTN[key] if key in LIMITS_ATTN else N.LIMITS[key])["limit"]


def measured(key):
    return (LIMITS_ATTN[key] if key in LIMITS_ATTN else N.LIMITS[key])["measured"]


def key_for(name, hd, rope=False, variant=None):
    """The limit key of an output at this module's cases.  A variant's changed outputs have keys of
    their own (``attn.<name>.hd<hd>[.rope].<variant>``); everything with the default rounding
    takes the ``.heads`` key where one exists, else the existing key of tests/numerics.py."""
    base = N.attn_key(name, hd, rope and name in ("dq", "dk", "dbias"))
    if variant is not None and name in VARIANT_OUTPUTS[variant]:
        return f"{base}.{variant}"
    return base + ".heads" if base + ".heads" in LIMITS_ATTN else base


# the outputs a variant's rounding reaches (dbias sums dk and dv; o under rsm: l enters 1 / l)
VARIANT_OUTPUTS = {"rsm": ("o", "lse"), "mf": ("o", "lse"), "ksc": ("dk", "dv", "dbias")}


# ======================================================================= CPU emulated ====

@functools.lru_cache(maxsize=6)
def emulated(case, fam, rope=False, fvar=None, bvar=None):
    """(inputs, oracle dict with the variants' units, emulated outputs) of one case on the CPU.
    The backward takes o and lse from the DEFAULT forward emulation, as the step would."""
    B, H, hd, T, causal = case
    q, k, v, do, pos = attn_inputs_bh(hd, T, fam, B, H)
    tab = N.rope_table(512, hd) if rope else None
    rp = pos if rope else None
    scale = hd ** -0.5
    ref = N.attn_refs(q, k, v, do, scale, causal, rp, tab)
    for var in (fvar, bvar):
        ref = variant_units(ref, q, k, v, do, scale, causal, var, rp, tab)
    o, lse = emu_attn_fwd(q, k, v, scale, causal)
    dq, dk, dv, db = emu_attn_bwd(do, q, k, v, o, lse, scale, causal, rp, tab, ksc=bvar == "ksc")
    if fvar is not None:
        o, lse = emu_attn_fwd(q, k, v, scale, causal, rsm=fvar == "rsm", mf=fvar == "mf")
    return (q, k, v, do, pos, tab), ref, {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "dbias": db}
