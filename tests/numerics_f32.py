"""Error bounds for the fp32 compute path (csrc/kernels/fp32.hip): GEMM and flash attention.

A plain helper module like ``tests/numerics.py`` (not collected), from which it takes the unit
roundoffs, the GEMM oracle and units, the RoPE helpers and the assertion.  In fp32 there is no
bf16 rounding to hide behind: every unit here is a derived worst-case fp32 bound and every limit
is ``numerics.DERIVED``; nothing is measured on a kernel.

* ``ref_attn32``: the fp64 oracle of the forward (o, lse) and backward (dq, dk, dv, with the
  inverse RoPE and the QKV bias gradient) with their units.  ``scale`` is the fp32 value the
  binding passes (``scale_f32``: float32(hd ** -0.5), not exact at head_dim 32 or 128).
* ``emu_attn32_fwd`` / ``emu_attn32_bwd``: fp32 evaluations of the kernels' algorithm on the CPU
  (64-key tiles, online max and rescale, sequential row sums; the backward from lse), with the
  planted faults of tests/test_numerics_f32.py.  They show that the bounds are attainable and
  that the faults are not; no limit is taken from them.
* ``gemm_plan`` / ``emu_gemm32``: the K-split plan of ``dpfs_gemm_f32`` and an fp32 matmul that
  sums its slabs in split order, with the planted GEMM faults.
* the case tables shared by tests/test_fp32_bounds_gpu.py and tests/test_numerics_f32.py.

Units, in multiples of U32 = 2^-24 and from fp64 quantities: s the scaled scores, smag =
scale |q| |k|, p the softmax, smax the row max, n_i the keys query i attends to, nt_i =
ceil(n_i / 64) the forward's key tiles, nk_j the queries that attend to key j.

Forward.  E_ij = (hd + 3) smag_ij + |s_ij - smax_i| + 3 bounds the relative error of one
exponential: the fma chain of hd products, c2 = scale log2 e and its product, the subtraction of
the running max (absolute, hence |s - smax|) and the 1-ulp exp2.  W_i = sum_j p_ij E_ij is that
of the row sum.
  unit_o   = (p E) |v| + (n + nt + 2) (p |v|) + |o| (W + n + 2 nt + 3)
             (the weights, the PV sum of n terms with one rescale per tile, the row sum l with its
             n adds and 2 roundings per tile, the reciprocal, product and store)
  unit_lse = W + n + 2 nt + 3 + 2 |smax| + 3 |lse| + 4
             (l's relative error, m + log2 l, the division by log2 e, the 1-ulp log2 absolute)

Backward, fed o and lse equal to the oracle's rounded to fp32 (known inputs: a forward fault
cannot leak into it).  E'_ij = (hd + 4) smag_ij + 3 |lse_i| + 3 (p = exp2(c2 S - lse log2 e):
lse's own rounding, its product and the subtraction are absolute in |lse|); dpmag = |do| |v|^T,
dmag_i = sum_d |do_id| |o_id| (delta = sum do o of hd products from an o rounded to fp32);
  G       = |dS| (E' + 2) + p ((hd + 1) dpmag + (hd + 2) dmag)
  unit_dq = scale (G |k| + (n + 2) |dS| |k|)
  unit_dk = scale (G^T |q| + (nk + 2) |dS|^T |q|)
  unit_dv = (p E')^T |do| + (nk + 1) p^T |do|
With the inverse RoPE the unit becomes rot_abs(unit) + 3 rot_abs(|ref|) of the pre-rotation
reference (two products and an add).  dbias: (B T + 9) sum|addend| + sum unit over each of the
three blocks (B T addends in any order over waves, partial rows and the 256-thread tree).

What these bounds cannot see: errors below roughly 1e-5 relative.  The units are worst cases
over n + hd roundings, so an exp2 approximation good to 2^-18, or one rounding too many, stays
inside them; they catch wrong masks, tiles, rescales, operands, pairings and precisions (a
10-bit significand gives 11 x the unit or more), not the last bits.

The CPU emulation's worst err / unit against the oracle over ATTN32_CASES x ATTN32_FAMILIES and,
for the ".rope" rows, ATTN32_ROPE_CASES (information only, no limit is taken from it; at =
(T, causal, family)):
  o     hd 32: 0.072 (300, False, peaked)  hd 64: 0.042 (193, False, peaked)  hd 128: 0.019 (193, False, peaked)
  lse   hd 32: 0.110 (193, False, peaked)  hd 64: 0.061 (300, False, peaked)  hd 128: 0.038 (33, True, peaked)
  dq    hd 32: 0.108 (193, True, peaked)   hd 64: 0.050 (300, True, peaked)   hd 128: 0.032 (300, False, peaked)
  dk    hd 32: 0.125 (193, True, peaked)   hd 64: 0.050 (33, True, peaked)    hd 128: 0.030 (300, False, peaked)
  dv    hd 32: 0.139 (193, True, peaked)   hd 64: 0.072 (300, True, peaked)   hd 128: 0.038 (193, False, peaked)
  dq.rope     hd 32: 0.049 (65)   hd 64: 0.048 (300)   hd 128: 0.022 (129)     (causal, peaked)
  dk.rope     hd 32: 0.051 (65)   hd 64: 0.045 (300)   hd 128: 0.018 (129)
  dbias.rope  hd 32: 0.007 (65)   hd 64: 0.002 (300)   hd 128: 0.001 (129)
"""
from __future__ import annotations

import torch

from numerics import LOG2E, U32, _mask, _rot_bthd, d, packed_views, ref_gemm, rope_table  # noqa: F401

# ------------------------------------------------------------------------------ GEMM ----

GEMM32_TILES = {0: (128, 64, 32), 1: (128, 64, 32)}   # workgroup tile, per wave, MFMA block (K stages: 32)
GEMM32_SPLIT_CAP = 64
LAYOUTS = {"nt": 0, "nn": 1, "tn": 2}
# (M, N, K): degenerate; every leading dimension != 0 mod 4 (all-scalar loads); a second tile of
# one row and two columns with a K tail of 1; vector loads and whole stages; two even K splits;
# 576-row splits whose last is 513 deep (a tail of 1); 64 splits planned, 61 launched
GEMM32_SHAPES = [(1, 1, 1), (65, 67, 7), (129, 130, 33), (200, 136, 64), (8, 12, 1024), (130, 8, 1089), (8, 8, 33000)]
GEMM32_VIEW_SHAPES = [(129, 130, 33), (130, 8, 1089)]
GEMM32_BF16_SHAPES = [(65, 67, 7), (129, 130, 33), (8, 12, 1089)]
GEMM32_STAT_SHAPE = (257, 200, 33)
GEMM32_SENTINEL = -7.0


def gemm_splits_for_unit(K):
    """The split count of the unit: the cap where the plan may split (K >= 1024), else 1."""
    return GEMM32_SPLIT_CAP if K >= 1024 else 1


def gemm_plan(M, N, K):
    """(planned splits, K rows per split, launched splits) as dpfs_gemm_f32 plans them: about
    1024 workgroups, each split at least 512 deep and a multiple of the 32-deep stage, at most 64."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    sp = max(1, min((1024 + tiles - 1) // tiles, max(1, K // 512), GEMM32_SPLIT_CAP))
    if sp == 1:
        return 1, K, 1
    kps = ((K + sp - 1) // sp + 31) // 32 * 32
    return sp, kps, (K + kps - 1) // kps


def gemm_operands(M, N, K, layout, seed, integers=False, dtype=torch.float32):
    """(a, b, bias, acc) on the CPU for a layout of LAYOUTS: randn, or integers in -8 .. 8 (every
    partial sum of the product stays below 2^24: a correct kernel has zero error in any order)."""
    g = torch.Generator().manual_seed(seed + 7 * M + 11 * N + 13 * K)
    mk = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if integers else (lambda *s: torch.randn(*s, generator=g))
    a = mk(K, M) if layout == "tn" else mk(M, K)
    b = mk(N, K) if layout == "nt" else mk(K, N)
    return a.to(dtype), b.to(dtype), mk(N), mk(M, N)


def strided(x, ld, offset, fill=GEMM32_SENTINEL):
    """(buffer, view): x copied into a column slice of a ``fill``-filled buffer with leading
    dimension ``ld`` whose first element lies ``offset`` elements into the allocation."""
    rows, cols = x.shape
    buf = torch.full((offset + rows * ld,), fill, dtype=x.dtype, device=x.device)
    view = buf[offset:].view(rows, ld)[:, :cols]
    view.copy_(x)
    return buf, view


def pads_intact(buf, view, fill=GEMM32_SENTINEL):
    """Every element of ``buf`` outside ``view`` still holds ``fill``."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    off = view.storage_offset() - buf.storage_offset()
    rows, cols = view.shape
    mask[off:off + rows * view.stride(0)].view(rows, view.stride(0))[:, :cols] = False
    return bool((buf[mask] == fill).all())


def tf32(x):
    """Chop an fp32 tensor to a 10-bit significand (the planted reduced-precision operand)."""
    return (x.float().contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def emu_gemm32(a, b, layout, bias=None, acc=None, out_bf16=False, fault=None):
    """gemm_f32_k + splitk_sum_f32_k in fp32 on the CPU: a plain fp32 matmul per split, the slabs
    summed in split order, then bias, the add into ``acc``, one rounding at the store.  Faults:
    "tf32" operands chopped to 10 bits; "k_tail" the last K element dropped; "split_overlap" the
    first K row of every later split also counted in the split before; "bias_per_split";
    "overwrite" (accumulate ignored); "slab_short" the slab sum stops one split early;
    "chopped" the bf16 store truncates."""
    a, b = a.float(), b.float()
    if layout == "nt":
        b = b.t()
    elif layout == "tn":
        a = a.t()
    M, K = a.shape
    if fault == "tf32":
        a, b = tf32(a), tf32(b)
    if fault == "k_tail":
        K -= 1
    _, kps, sx = gemm_plan(M, b.size(1), a.size(1))
    out = torch.zeros(M, b.size(1))
    for s in range(sx - 1 if fault == "slab_short" else sx):
        lo, hi = s * kps, min(K, (s + 1) * kps)
        if fault == "split_overlap" and s + 1 < sx:
            hi += 1
        out = out + a[:, lo:hi] @ b[lo:hi]
        if bias is not None and fault == "bias_per_split" and s > 0:
            out = out + bias.float()
    if bias is not None:
        out = out + bias.float()
    if acc is not None and fault != "overwrite":
        out = acc.float() + out
    if out_bf16:
        return (out.view(torch.int32) & -65536).view(torch.float32).bfloat16() if fault == "chopped" else out.bfloat16()
    return out


# ------------------------------------------------------------------------- attention ----

ATTN32_SEED = 10
ATTN32_FAMILIES = {"randn": 1.0, "peaked": 3.0}     # q and k scaled: flat softmax / near one-hot rows
# T 1, 33: partial single tiles; 65: one key past a key tile; 129: a second 128-query block of one
# query (at head_dim 64 the prefetch guard); 193: a dK/dV key block whose first query tile is
# partial; 300: ragged last tiles everywhere
ATTN32_CASES = [(hd, T, causal) for hd in (32, 64, 128) for T in (1, 33, 65, 129, 193, 300) for causal in (True, False)]
ATTN32_ROPE_CASES = [(32, 65), (64, 300), (128, 129)]   # (32, 65): the c / c + 16 pairing inside one MFMA tile
ATTN32_MANY_ROWS = dict(B=65, T=1, H=1, hd=32)          # 260 partial rows: a second trip of the column-sum loop
ATTN32_TILES = {"o": {1: (128, 64, 32)}, "dq": {1: (128, 64, 32)}, "dk": {1: (128, 64, 32)}, "dv": {1: (128, 64, 32)},
                "lse": {2: (128, 64, 32)}, "dbias": {}}


def scale_f32(hd):
    """hd ** -0.5 as the fp32 value the binding hands the kernels."""
    return float(torch.tensor(hd ** -0.5, dtype=torch.float32))


def attn32_inputs(hd, T, family, device="cpu", B=2, H=3, seed=ATTN32_SEED):
    """q, k, v as views of a packed (B T, 3 H hd) fp32 buffer (the step's strides), do, and RoPE
    positions; generated on the CPU so the CPU emulation and the GPU tests see the same values."""
    gen = torch.Generator().manual_seed(seed + 1000 * hd + T + 7 * B)
    qkv = torch.randn(B * T, 3 * H * hd, generator=gen)
    qkv[:, : 2 * H * hd] *= ATTN32_FAMILIES[family]
    q, k, v = packed_views(qkv.to(device), B, T, H, hd)
    do = torch.randn(B, T, H, hd, generator=gen).to(device)
    pos = torch.randint(0, 512, (B * T,), generator=gen).to(device)
    return q, k, v, do, pos


def _bhtd(x):
    return d(x).transpose(1, 2)


def ref_attn32(q, k, v, do, scale, causal, pos=None, tab=None):
    """q, k, v, do (B, T, H, hd) fp32 -> dict o, dq, dk, dv (B, T, H, hd), lse (B, H, T), dbias
    (3 H hd) and unit_<name>, all fp64 (the module docstring carries the derivations).  With
    ``pos`` / ``tab`` dq and dk carry the inverse RoPE."""
    qf, kf, vf, dof = _bhtd(q), _bhtd(k), _bhtd(v), _bhtd(do)
    B, H, T, hd = qf.shape
    s = (qf @ kf.transpose(-1, -2)) * scale
    smag = (qf.abs() @ kf.abs().transpose(-1, -2)) * scale
    keep = torch.ones(T, T, dtype=torch.bool, device=s.device)
    if causal:
        keep = keep.tril()
    s = s.masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    smax = s.max(-1).values
    n = keep.sum(-1).double()
    nt = torch.ceil(n / 64)
    nk = keep.sum(0).double()
    E = (hd + 3) * smag + (s - smax[..., None]).abs().masked_fill(~keep, 0) + 3
    W = (p * E).sum(-1)
    o = p @ vf
    unit_o = (p * E) @ vf.abs() + (n + nt + 2)[:, None] * (p @ vf.abs()) + o.abs() * (W + n + 2 * nt + 3)[..., None]
    unit_lse = W + n + 2 * nt + 3 + 2 * smax.abs() + 3 * lse.abs() + 4
    Eb = (hd + 4) * smag + 3 * lse.abs()[..., None] + 3
    dp = dof @ vf.transpose(-1, -2)
    dpmag = dof.abs() @ vf.abs().transpose(-1, -2)
    delta = (dof * o).sum(-1, keepdim=True)
    dmag = (dof.abs() * o.abs()).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    G = ds.abs() * (Eb + 2) + p * ((hd + 1) * dpmag + (hd + 2) * dmag)
    dq, dk = scale * (ds @ kf), scale * (ds.transpose(-1, -2) @ qf)
    dv = p.transpose(-1, -2) @ dof
    unit_dq = scale * (G @ kf.abs() + (n + 2)[:, None] * (ds.abs() @ kf.abs()))
    unit_dk = scale * (G.transpose(-1, -2) @ qf.abs() + (nk + 2)[:, None] * (ds.abs().transpose(-1, -2) @ qf.abs()))
    unit_dv = (p * Eb).transpose(-1, -2) @ dof.abs() + (nk + 1)[:, None] * (p.transpose(-1, -2) @ dof.abs())
    r = {"o": o.transpose(1, 2), "unit_o": U32 * unit_o.transpose(1, 2), "lse": lse, "unit_lse": U32 * unit_lse}
    for name, x, u in (("dq", dq, unit_dq), ("dk", dk, unit_dk), ("dv", dv, unit_dv)):
        x, u = x.transpose(1, 2), U32 * u.transpose(1, 2)
        if pos is not None and name != "dv":
            u = _rot_bthd(u, pos, tab, True) + 3 * U32 * _rot_bthd(x.abs(), pos, tab, True)
            x = _rot_bthd(x, pos, tab)
        r[name], r["unit_" + name] = x, u
    cat = lambda f: torch.cat([f(name).sum((0, 1)).reshape(-1) for name in ("dq", "dk", "dv")])
    r["dbias"] = cat(lambda name: r[name])
    r["unit_dbias"] = (B * T + 9) * U32 * cat(lambda name: r[name].abs()) + cat(lambda name: r["unit_" + name])
    return r


def emu_attn32_fwd(q, k, v, scale, causal, fault=None):
    """attn_fwd_f32_k in fp32 on the CPU: 64-key tiles, scores by a sequential fma-order chain,
    x = S c2 with c2 = scale log2 e, online max with the rescale alpha = exp2(m - m_new) of l and
    o, sequential row sums, o / l and lse = (m + log2 l) / log2 e at the end.  Returns (o (B, T, H,
    hd), lse (B, H, T)).  Faults: "diag" the diagonal key masked (key < q) in (b, h) = (0, 0);
    "tail" keys >= T of the last tile left unmasked (they read as zeros); "alpha" o not rescaled
    in the second tile while l is; "log2" lse left in log2 units."""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    B, H, T, hd = qf.shape
    L2 = torch.tensor(LOG2E, dtype=torch.float32)
    c2 = torch.tensor(scale, dtype=torch.float32) * L2
    m = torch.full((B, H, T, 1), float("-inf"))
    l = torch.zeros(B, H, T, 1)
    o = torch.zeros(B, H, T, hd)
    qi = torch.arange(T)[:, None]
    for kv0 in range(0, T, 64):
        kt, vt = kf[:, :, kv0:kv0 + 64], vf[:, :, kv0:kv0 + 64]
        if fault == "tail" and kt.size(2) < 64:
            pad = torch.zeros(B, H, 64 - kt.size(2), hd)
            kt, vt = torch.cat([kt, pad], 2), torch.cat([vt, pad], 2)
        nkeys = kt.size(2)
        sc = torch.zeros(B, H, T, nkeys)
        for i in range(hd):
            sc += qf[..., :, None, i] * kt[..., None, :, i]
        x = sc * c2
        key = kv0 + torch.arange(nkeys)[None, :]
        ok = ((key <= qi) if causal else torch.ones(T, nkeys, dtype=torch.bool)).expand(B, H, T, nkeys).clone()
        if causal and fault == "diag":
            ok[0, 0] = key < qi
        x = x.masked_fill(~ok, float("-inf"))
        mn = torch.maximum(m, x.max(-1, keepdim=True).values)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mn))
        pp = torch.where(torch.isinf(mn), torch.zeros_like(x), torch.exp2(x - mn))
        ps = torch.zeros_like(l)
        for j in range(nkeys):
            ps += pp[..., j:j + 1]
        l = l * alpha + ps
        o = o if (fault == "alpha" and kv0 == 64) else o * alpha
        for j in range(nkeys):
            o += pp[..., j:j + 1] * vt[..., j:j + 1, :]
        m = mn
    lse = m + torch.log2(l)
    if fault != "log2":
        lse = lse / L2
    return (o * (1.0 / l)).transpose(1, 2), lse.squeeze(-1)


def emu_attn32_bwd(do, q, k, v, o, lse, scale, causal, pos=None, tab=None, fault=None):
    """attn_bwd_dq_f32_k + attn_bwd_dkdv_f32_k + colsum_parts_f32_k in fp32 on the CPU: delta =
    sum do o, p = exp2(S c2 - lse log2 e), dS = p (dP - delta), dq / dk = (dS k / dS^T q) scale,
    inverse RoPE, the bias gradient as fp32 column sums.  Returns (dq, dk, dv (B, T, H, hd),
    dbias).  Faults: "delta_head" delta from the neighbouring head's o; "sin_sign" the sign of sin
    flipped in the inverse RoPE; "pairing" head_dim 32 sent through the general pairing loop
    (tile d with tile d + tiles / 2), which at one tile runs no trip: dq / dk left unrotated;
    "dbias_wave" the partial row of the first 32 queries of (b, h) = (0, 0) missing from dbias;
    "dbias_row" a row >= T (the next batch's first token) included in batch 0's dk sums (its dq
    is zero in a causal case: query 0 has dS == 0);
    "dk_scale" dk without scale."""
    qf, kf, vf, dof, of = (t.float().transpose(1, 2) for t in (q, k, v, do, o))
    L2 = torch.tensor(LOG2E, dtype=torch.float32)
    sc = torch.tensor(scale, dtype=torch.float32)
    T = qf.size(2)
    x = (qf @ kf.transpose(-1, -2)) * (sc * L2) - (lse.float() * L2)[..., None]
    p = torch.exp2(x)
    if causal:
        p = p.masked_fill(_mask(T, p.device), 0.0)
    delta = (dof * (of.roll(1, 1) if fault == "delta_head" else of)).sum(-1, keepdim=True)
    ds = p * (dof @ vf.transpose(-1, -2) - delta)
    dq = (ds @ kf) * sc
    dk = ds.transpose(-1, -2) @ qf
    if fault != "dk_scale":
        dk = dk * sc
    dv = p.transpose(-1, -2) @ dof
    dq, dk, dv = (t.transpose(1, 2) for t in (dq, dk, dv))
    if pos is not None and fault != "pairing":
        B, T, H, hd = dq.shape
        h2 = hd // 2
        t = tab.float()[pos.long()].view(B, T, 1, hd)
        c, s = t[..., :h2], t[..., h2:]
        if fault == "sin_sign":
            s = -s
        rot = lambda y: torch.cat([y[..., :h2] * c + y[..., h2:] * s, y[..., h2:] * c - y[..., :h2] * s], -1)
        dq, dk = rot(dq), rot(dk)
    sums = [t.sum((0, 1)) for t in (dq, dk, dv)]          # (H, hd) each
    if fault == "dbias_wave":
        sums[0][0] -= dq[0, :32, 0].sum(0)
    if fault == "dbias_row":
        sums[1] += dk[-1, 0]
    return dq, dk, dv, torch.cat([t.reshape(-1) for t in sums])
