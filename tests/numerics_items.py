"""The persistent GEMM's item order, mirrored in Python, and what the multi-item tests build on it.

A plain helper module (not a conftest, not collected, no GPU import).  ``gemm4_k``
(csrc/kernels/gemm4.hip) is persistent: its launchers start G = min(items, CU count) workgroups,
workgroup ``b`` starts at item ``xcd_remap(b, G)`` and walks ``it, it + G, it + 2 G, ...``; the
LDS-DMA producer runs three 32-deep steps ahead of the consumer, across item boundaries.  What an
item inherits from the one before it in its workgroup (ring slot, fragment register set, lane
offsets, the bias area, the store count every wait subtracts) is invisible to a test whose
workgroups run one item each, so the tests of tests/test_gemm_items_bounds_gpu.py size their
cases from this mirror and assert from it that some workgroup runs three items.

* **The mirror**: ``xcd_remap`` (csrc/kernels/common.h), ``decode`` (``decode<BN>``),
  ``item_order`` (the plain / split-K launch), ``sk_order`` (``gdecode``'s stream-K branch),
  ``group_order`` (the grouped TN launch: ``item0`` per member), ``pick_bn`` (the launcher's
  256- or 192-wide choice), ``nsteps``.  Every item carries its tile origin, split, workgroup
  (the ``blockIdx.x`` that runs it) and round (0 = the workgroup's first item).
* **Shape helpers** take the CU count as an argument (the GPU tests pass the device's, the CPU
  tests 256 and small made-up counts): ``shape_for``, ``m_for``, ``forced_splits``.
* **Units** the multi-item cases need beyond tests/numerics.py, all derived (their docstrings):
  ``unit_splitk_bf16``, ``unit_rope_two_pass``, ``unit_gemm_sk``.
* ``assert_within_rows``: ``numerics.assert_within`` over row slabs, so the fp64 oracle of a
  30 M-element output stays near 1 GB; ``where`` turns the worst element into its item.

Three rounds: ``nsteps`` rounds an item's 32-deep steps up to an even count, so the ring phase
(slot mod 4) at an item boundary is 0 or 2; three items in a workgroup show both boundary kinds
(0 -> 2 and 2 -> 0) whenever an item's step count is 2 mod 4, and two same-phase boundaries
otherwise.
"""
from __future__ import annotations

import functools
import os
from collections import namedtuple

import torch

import numerics as N

GROUP_M = 4          # G4Knobs::group_m
BM = 256             # tile rows
ROLES = ("whole tile", "producer half", "consumer half")

# lin: linear item; m0, n0: tile origin; split: K split (its slab); wg: the blockIdx.x that runs
# it; round: its position in that workgroup's walk; role: index of ROLES (stream-K); g: the
# grouped launch's member (stream-K: the extra tile's partial slot, -1 for a whole tile < G)
Item = namedtuple("Item", "lin m0 n0 split wg round role g")


def rounds_wanted():
    """DPFS_BOUNDS_ROUNDS (default 3) may raise the rounds of a manual run, never lower them."""
    return max(3, int(os.environ.get("DPFS_BOUNDS_ROUNDS", "3")))


def cdiv(a, b):
    return (a + b - 1) // b


def xcd_remap(orig, nwg):
    """common.h xcd_remap: workgroup ``orig`` of ``nwg`` -> its first item (bijective)."""
    q, r = divmod(nwg, 8)
    xcd = orig % 8
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + orig // 8


def _wg_of(G):
    """first item -> blockIdx.x (the inverse of xcd_remap)."""
    inv = [0] * G
    for b in range(G):
        inv[xcd_remap(b, G)] = b
    assert sorted(xcd_remap(b, G) for b in range(G)) == list(range(G))
    return inv


def decode(lin, nwg, tiles_m, tiles_n, group_m, bn):
    """decode<BN>: (m0, n0, split) of linear item ``lin`` (tile rows in groups of ``group_m``,
    column-major inside a group; the last group may be short)."""
    split, wg = divmod(lin, nwg)
    per_group = group_m * tiles_n
    gid = wg // per_group
    first_m = gid * group_m
    gsz = min(tiles_m - first_m, group_m)
    r = wg - gid * per_group
    return (first_m + r % gsz) * BM, (r // gsz) * bn, split


def nsteps(kb, ke):
    """32-deep steps of an item, rounded up to an even count."""
    n = max(1, cdiv(ke - kb, 32))
    return (n + 1) & ~1


def pick_bn(M, Nn, cus, variant=0):
    """Tile width of a non-split bf16 NT / NN launch without RoPE (dpfs_gemm4_launch): 192 forced
    by variant 2 / 6, else 192 where its rounds over the CUs, priced at 0.8, come out shorter."""
    if variant & 3 == 2:
        return 192
    tm = cdiv(M, BM)
    r256 = cdiv(tm * cdiv(Nn, 256), cus)
    r192 = cdiv(tm * cdiv(Nn, 192), cus)
    return 192 if r192 * 0.8 < r256 * 0.95 else 256


def item_order(M, Nn, bn, splits, group_m, G):
    """Every item of a plain (splits = 1) or split-K launch of G workgroups, in linear order."""
    tiles_m, tiles_n = cdiv(M, BM), cdiv(Nn, bn)
    nwg = tiles_m * tiles_n
    inv = _wg_of(G)
    out = []
    for lin in range(nwg * splits):
        m0, n0, split = decode(lin, nwg, tiles_m, tiles_n, group_m, bn)
        out.append(Item(lin, m0, n0, split, inv[lin % G], lin // G, 0, 0))
    return out


def launch_order(M, Nn, bn, splits, cus, group_m=GROUP_M):
    """item_order at the launchers' grid, min(items, CU count)."""
    return item_order(M, Nn, bn, splits, group_m, min(cdiv(M, BM) * cdiv(Nn, bn) * splits, cus))


def sk_order(M, Nn, G, group_m=GROUP_M):
    """The stream-K launch (gdecode's SK branch): G workgroups, E = G / 2 extra tiles, two items per
    workgroup.  Workgroup slot c < E: the first K half of tile G + c (role 1), then whole tile c;
    c >= E: whole tile c, then the second K half of tile G + c - E (role 2)."""
    tiles_m, tiles_n = cdiv(M, BM), cdiv(Nn, 256)
    nwg, E = tiles_m * tiles_n, G // 2
    assert 2 * nwg == 3 * G and G % 2 == 0, "stream-K: tiles at exactly 1.5 per workgroup"
    inv = _wg_of(G)
    out = []
    for lin in range(2 * G):
        second, c = lin >= G, lin % G
        if c < E:
            tile, role = (c, 0) if second else (G + c, 1)
        else:
            tile, role = (G + c - E, 2) if second else (c, 0)
        m0, n0, _ = decode(tile, nwg, tiles_m, tiles_n, group_m, 256)
        out.append(Item(lin, m0, n0, 0, inv[c], int(second), role, tile - G if role else -1))
    return out


def group_order(shapes, splits, G, group_m=GROUP_M):
    """The grouped TN launch: member g owns the items [item0[g], item0[g + 1]) = its tiles x
    ``splits``, decoded on its own tile grid.  Returns (items, item0)."""
    item0, total = [], 0
    for M, Nn in shapes:
        item0.append(total)
        total += cdiv(M, BM) * cdiv(Nn, 256) * splits
    G = min(G, total)
    inv = _wg_of(G)
    out = []
    for lin in range(total):
        g = max(i for i in range(len(shapes)) if lin >= item0[i])
        tm, tn = cdiv(shapes[g][0], BM), cdiv(shapes[g][1], 256)
        m0, n0, split = decode(lin - item0[g], tm * tn, tm, tn, group_m, 256)
        out.append(Item(lin, m0, n0, split, inv[lin % G], lin // G, 0, g))
    return out, item0


def per_workgroup(items):
    """workgroup -> its items in the order it runs them."""
    w = {}
    for it in items:
        w.setdefault(it.wg, []).append(it)
    for v in w.values():
        v.sort(key=lambda it: it.round)
    return w


def previous(items):
    """lin -> the item its workgroup ran just before it (None in round 0)."""
    prev = {}
    for v in per_workgroup(items).values():
        for a, b in zip([None] + v[:-1], v):
            prev[b.lin] = a
    return prev


def assert_rounds(items, rounds, what):
    """The precondition of a multi-item case: some workgroup runs ``rounds`` items and some
    workgroup fewer than the maximum (the tail, where a producer runs past the last item while
    other workgroups still compute)."""
    counts = [len(v) for v in per_workgroup(items).values()]
    assert max(counts) >= rounds, f"{what}: at most {max(counts)} items per workgroup, {rounds} wanted"
    assert min(counts) < max(counts), f"{what}: every workgroup runs {max(counts)} items, no tail"
    return max(counts)


# ---------------------------------------------------------------------- shape helpers ----

def _ragged(tiles, rem):
    return (tiles - 1) * 256 + rem


@functools.lru_cache(maxsize=None)
def shape_for(rounds, cus, tn=None, bn=None):
    """The smallest (M, N) whose 256 x 256 tile count exceeds (rounds - 1) * cus with M % 256 == 1
    (the last row tile is one row), N % 256 == 8 (the last column tile is one 16-byte store wide)
    and a row-tile count that is no multiple of ``GROUP_M`` (the last tile-row group is short).
    ``tn``: the column-tile count is given.  ``bn`` 256 / 192: additionally the width the
    launcher's round model picks for a plain bf16 launch of that shape."""
    need = (rounds - 1) * cus + 1
    best = None
    for tiles_n in ([tn] if tn else range(1, need + 1)):
        tiles_m, found = cdiv(need, tiles_n), False
        while tiles_m * tiles_n < 4 * need and not found:      # (a width some column counts never get)
            M, Nn = _ragged(tiles_m, 1), _ragged(tiles_n, 8)
            found = bool(tiles_m % GROUP_M) and (bn is None or pick_bn(M, Nn, cus) == bn) and \
                (tn is not None or max(tiles_m, tiles_n) <= 4 * min(tiles_m, tiles_n))     # no sliver of tiles
            tiles_m += 0 if found else 1
        if not found:
            continue
        key = (tiles_m * tiles_n, abs(tiles_m - tiles_n), M * Nn)      # fewest tiles, then nearest to square
        if best is None or key < best[0]:
            best = (key, (M, Nn))
    return best[1]


def m_for(rounds, cus, tiles_n):
    """Rows (M % 256 == 1, row tiles no multiple of GROUP_M) for ``rounds`` rounds at a fixed column-tile count."""
    return shape_for(rounds, cus, tn=tiles_n)[0]


def forced_splits(rounds, cus, tiles):
    """The smallest split count with tiles * S > (rounds - 1) * cus."""
    return (rounds - 1) * cus // tiles + 1


def sk_shape(cus):
    """(M, N) of 1.5 * cus tiles of 256 x 256 with ragged last row and column tiles: three column
    tiles (N = 520), cus / 2 row tiles, the last of 8 rows."""
    assert cus % 2 == 0
    return _ragged(cus // 2, 8), _ragged(3, 8)


# ------------------------------------------------------------ element -> item, masks ----

def tile_map(items, bn):
    """(m0, n0) -> the tile's items (one per split, or the stream-K pair)."""
    t = {}
    for it in items:
        t.setdefault((it.m0, it.n0), []).append(it)
    return t


def locator(items, bn, row0=0):
    """The ``where`` callable of assert_within: names the item(s) that wrote element (i, j)."""
    tm = tile_map(items, bn)

    def where(idx):
        i, j = idx[-2] + row0, idx[-1]
        its = tm.get((i // BM * BM, j // bn * bn), [])
        if not its:
            return f"element ({i}, {j}) belongs to no item"
        s = ", ".join(f"item {it.lin} (workgroup {it.wg}, round {it.round}"
                      + (f", split {it.split}" if len(its) > 1 and not it.role else "")
                      + (f", {ROLES[it.role]}" if any(x.role for x in its) else "") + ")" for it in its[:3])
        return f"row {i}: tile ({i // BM}, {j // bn}) = {s}" + (f" and {len(its) - 3} more" if len(its) > 3 else "")
    return where


def round_mask(M, Nn, items, bn, rnd, device="cpu"):
    """bool [M, N]: the elements written by items of round ``rnd`` (non-split launches)."""
    mask = torch.zeros(M, Nn, dtype=torch.bool, device=device)
    for it in items:
        if it.round == rnd:
            mask[it.m0:it.m0 + BM, it.n0:it.n0 + bn] = True
    return mask


def assert_within_rows(out, slab_ref, limit, what, tiles=None, items=None, bn=256, rows=2048):
    """``numerics.assert_within`` over row slabs of ``out`` [M, N]: ``slab_ref(r0, r1)`` returns
    (ref64, unit) of rows [r0, r1).  Every slab is judged; the assertion (and the one recorded
    row) is the worst slab's.  Returns the worst ratio."""
    worst = (-1.0, 0, None, None)
    for r0 in range(0, out.size(0), rows):
        r1 = min(out.size(0), r0 + rows)
        ref, unit = slab_ref(r0, r1)
        w = N.worst_ratio(out[r0:r1], ref, unit)[0]
        if w > worst[0]:
            worst = (w, r0, ref, unit)
        if w > limit:
            break
    w, r0, ref, unit = worst
    where = locator(items, bn, r0) if items is not None else None
    return N.assert_within(out[r0:r0 + ref.size(0)], ref, unit, limit, what, tiles, where=where)


# ------------------------------------------------------------------------------ units ----

def unit_splitk_bf16(ref, mag, K, S):
    """bf16 output of the split-K slab path (gemm4_k fp32 slabs + splitk_reduce_bf16_k): each slab
    accumulates its share of the K products in fp32, the reduction adds the S slabs in fp32, then
    the bias, and rounds ONCE to bf16.  K products + S slab additions + the bias addition are
    ``numerics.unit_gemm_f32``'s (K + S + 2) U32 mag (mag includes |bias|); the store adds
    U16 |ref|."""
    return N.U16 * ref.abs() + N.unit_gemm_f32(mag, K, S)


def unit_rope_two_pass(lin, f32_term, pos, tab, heads, hd):
    """(ref, unit) of a GEMM whose bf16 output is rotated by a SECOND pass (``rope_`` after the
    GEMM: dpfs_rope_after_gemm on the split-K path, head dims the epilogue does not fuse).

    The first pass stores y = bf16(lin + e), |e| <= ``f32_term`` (its fp32 accumulation bound), so
    |y - lin| <= u_lin = U16 |lin| + (1 + U16) f32_term.  The rotation is linear: rot(y) - rot(lin)
    is bounded by u_lin mixed with |cos|, |sin| (``ref_rope(..., mag=u_lin)``, the way the fused
    epilogue's unit carries the accumulator term) = P.  The second pass evaluates two products and
    an add in fp32 on y (3 U32 rmag(|y|) <= 3 U32 (rmag + P)) and rounds rot(y) once more
    (U16 |rot(y)| <= U16 (|ref| + P)):
        unit = U16 |ref| + (1 + U16 + 3 U32) P + 3 U32 rmag      on the rotated columns,
        unit = u_lin                                             on the others (left untouched)."""
    ref, rmag = N.ref_rope(lin, pos, tab, heads, hd)
    u_lin = N.U16 * lin.abs() + (1 + N.U16) * f32_term
    P = N.ref_rope(lin, pos, tab, heads, hd, mag=u_lin)[1]
    unit = N.U16 * ref.abs() + (1 + N.U16 + 3 * N.U32) * P + 3 * N.U32 * rmag
    unit[:, heads * hd:] = u_lin[:, heads * hd:]
    return ref, unit


def unit_gemm_sk(ref, mag, K):
    """bf16 output of the stream-K kernel: an extra tile's first K half goes out as an fp32
    partial (stored exactly), the consumer accumulates the second half and ADDS the partial
    before bias and the one rounding: one fp32 addition more than the plain kernel, so
    ``numerics.unit_gemm_bf16`` with (K + 3) in place of (K + 2).  Whole tiles are the plain
    kernel's and lie inside it."""
    return N.U16 * ref.abs() + (K + 3) * N.U32 * mag


# ------------------------------------------------------------------------ emulations ----
# fp32 evaluations on the CPU that walk the items of the mirror the way the kernels do: a tile's
# accumulator is a sum of 32-deep steps, rounded where the kernels round.  They exist to show
# that the derived units are attainable on scaled-down instances (a made-up CU count) and that
# the planted faults of tests/test_numerics_items.py, applied to items of round >= 1 only, are not.

def _crop(X, r0, nr, c0, nc):
    """X[r0 : r0 + nr, c0 : c0 + nc] with zeros past the edges (an out-of-range DMA reads zeros)."""
    out = X.new_zeros(nr, nc)
    if r0 < X.size(0) and c0 < X.size(1):
        blk = X[r0:r0 + nr, c0:c0 + nc]
        out[:blk.size(0), :blk.size(1)] = blk
    return out


def _live_steps(kb, ke):
    return [(k, min(k + 32, ke)) for k in range(kb, ke, 32)]


def emu_items(A, Bm, items, bn, K, kps, bias=None, fault=None, k_switch=None, A2=None, B2=None, k0=None):
    """fp32 slabs [S, M, N] of a launch: A [M, K] and Bm [K, N] fp32 (any layout brought to this
    form), item by item, each a sum of its live 32-deep steps (+ the item's own bias columns when
    ``bias`` is given: the non-split bf16 kernel).  ``k_switch`` / ``A2`` / ``B2`` / ``k0``: the rows
    past k_switch come from the second buffers (the first holds k0 rows).  Faults, on items of
    round >= 1: "stale_bias" the bias of the previous item's columns; "drop_last_step" the last
    live step skipped; "stale_first_step" the first step's operands are the previous item's last
    step's (a ring slot not refilled); "k_switch_overrun" an item of the second buffers reads the
    first past k_switch (zeros past its descriptor)."""
    M, Nn = A.size(0), Bm.size(1)
    S = max(it.split for it in items) + 1
    slabs = torch.zeros(S, M, Nn)
    prev = previous(items)

    def krange(it):
        kb = it.split * kps
        ke = min(K, kb + kps)
        a, b = A, Bm
        if k_switch is not None and kb >= k_switch:
            kb, ke = kb - k_switch, ke - k_switch
            if not (fault == "k_switch_overrun" and it.round >= 1):
                a, b = A2, B2
            else:
                kb, ke = kb + k_switch, ke + k_switch
        elif k0 is not None:
            ke = min(ke, k0)
        return a, b, kb, ke

    for it in items:
        a, b, kb, ke = krange(it)
        steps = _live_steps(kb, ke)
        later = it.round >= 1
        if fault == "drop_last_step" and later:
            steps = steps[:-1]
        acc = torch.zeros(BM, bn)
        for i, (s0, s1) in enumerate(steps):
            if fault == "stale_first_step" and later and i == 0:
                p = prev[it.lin]
                pa, pb, pkb, pke = krange(p)
                q0, q1 = _live_steps(pkb, pke)[-1]
                acc += _crop(pa, p.m0, BM, q0, q1 - q0) @ _crop(pb, q0, q1 - q0, p.n0, bn)
            else:
                acc += _crop(a, it.m0, BM, s0, s1 - s0) @ _crop(b, s0, s1 - s0, it.n0, bn)
        if bias is not None:
            n0 = prev[it.lin].n0 if (fault == "stale_bias" and later) else it.n0
            acc += _crop(bias[None, :], 0, 1, n0, bn)
        blk = slabs[it.split, it.m0:it.m0 + BM, it.n0:it.n0 + bn]
        blk.copy_(acc[:blk.size(0), :blk.size(1)])
    return slabs


def emu_slab_sum(slabs, bias=None, acc=None, twice=None):
    """The slab reductions: slabs added in split order, then bias (splitk_reduce_bf16_k) or the add
    into ``acc`` (splitk_reduce_k).  ``twice`` = (split, m0, n0, bn): that tile's slab counted twice."""
    s = torch.zeros_like(slabs[0])
    for k in range(slabs.size(0)):
        s += slabs[k]
        if twice is not None and twice[0] == k:
            _, m0, n0, bn = twice
            s[m0:m0 + BM, n0:n0 + bn] += slabs[k, m0:m0 + BM, n0:n0 + bn]
    if bias is not None:
        s += bias
    if acc is not None:
        s += acc
    return s


def emu_stream_k(A, Bm, items, K, bias=None, fault=None):
    """The stream-K kernel: whole tiles as the plain kernel; an extra tile's producer accumulates
    the first K half and hands it over as an fp32 partial, its consumer accumulates the second half,
    adds the partial, then bias and the rounding.  Faults (the consumers are second-round items):
    "sk_partial_shift" the partial added to the next 16-row block; "sk_quarter_missing" the first
    consumer does not add it in one wave's 128 x 128 quarter."""
    M, Nn = A.size(0), Bm.size(1)
    out = torch.zeros(M, Nn)
    part = {}
    first_consumer = min(it.lin for it in items if it.role == 2)
    for it in sorted(items, key=lambda it: it.role == 2):      # producers before their consumers
        kb, ke = (0, K) if it.role == 0 else ((0, K // 2) if it.role == 1 else (K // 2, K))
        acc = torch.zeros(BM, 256)
        for s0, s1 in _live_steps(kb, ke):
            acc += _crop(A, it.m0, BM, s0, s1 - s0) @ _crop(Bm, s0, s1 - s0, it.n0, 256)
        if it.role == 1:
            part[it.g] = acc
            continue
        if it.role == 2:
            p = part[it.g]
            if fault == "sk_partial_shift":
                p = torch.roll(p, 16, 0)
            if fault == "sk_quarter_missing" and it.lin == first_consumer:
                p = p.clone()
                p[:128, :128] = 0
            acc = acc + p
        if bias is not None:
            acc = acc + _crop(bias[None, :], 0, 1, it.n0, 256)
        blk = out[it.m0:it.m0 + BM, it.n0:it.n0 + 256]
        blk.copy_(acc[:blk.size(0), :blk.size(1)])
    return out.bfloat16()


def emu_rope(x, pos, tab, heads, hd):
    """rope_ / the RoPE epilogue's rotation in fp32: x1 c - x2 s | x2 c + x1 s on the first heads."""
    M, h2 = x.size(0), hd // 2
    t = tab.float()[pos.long()]
    c, s = t[:, None, :h2], t[:, None, h2:]
    out = x.clone()
    v = x[:, :heads * hd].reshape(M, heads, hd)
    x1, x2 = v[..., :h2], v[..., h2:]
    out[:, :heads * hd] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(M, -1)
    return out


def stale_positions(pos, items):
    """pos with the rows of every item of round >= 1 replaced by the positions of the previous
    item's rows (the planted RoPE-epilogue fault)."""
    out = pos.clone()
    prev = previous(items)
    M = pos.numel()
    for it in items:
        p = prev[it.lin]
        if p is not None and p.m0 != it.m0:
            n = min(BM, M - it.m0, M - p.m0)
            out[it.m0:it.m0 + n] = pos[p.m0:p.m0 + n]
    return out


def emu_swiglu_bwd_dbias(dy, w, gu, items, missing=None):
    """The SwiGLU-backward epilogue's bias gradient in fp32: dh = bf16(dy w), dgu from it, column
    sums per 128-row half of every row tile (the partials), the partials summed.  ``missing``: a
    row-tile origin whose partials are left out for the columns of one item (the planted fault:
    (m0, n0) of an item)."""
    F_ = w.size(1)
    dh = (dy.float() @ w.float()).bfloat16().float()
    g, u = gu.float()[:, :F_], gu.float()[:, F_:]
    s = torch.sigmoid(g)
    dgu = torch.cat([dh * u * s * (1 + g * (1 - s)), dh * g * s], 1)
    db = torch.zeros(2 * F_)
    for m0 in range(0, dy.size(0), 128):
        p = dgu[m0:m0 + 128].sum(0)
        if missing is not None and m0 // BM * BM == missing[0]:
            n0, n1 = missing[1], min(missing[1] + 256, F_)
            p[n0:n1] = 0
            p[F_ + n0:F_ + n1] = 0
        db += p
    return db
