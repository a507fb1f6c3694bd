"""Per-element error bounds for the step's kernels: fp64 oracles, error units, one assertion.

A plain helper module (not a conftest, not collected).  Three layers:

* **Oracles** (``ref_*``): each operation written from its math, fp64 throughout, on whatever
  device its inputs live on.  They return the exact result and the absolute-value products the
  error units are built from.  ``ops/reference.py`` (fp32, the CPU compute path) is not used.
* **Error units** (``unit_*``): a per-element fp64 tensor bounding what a correct kernel may
  deviate by.  ``U16 = 2^-8`` is the unit roundoff of bf16 (8-bit significand, round to nearest:
  |fl(x) - x| <= 2^-8 |x|), ``U32 = 2^-24`` that of fp32.  A sum of n fp32 terms in any order,
  products included, deviates by at most (n + 1) U32 sum|terms| to first order (Higham, Accuracy
  and Stability of Numerical Algorithms, section 4.2); the units use that worst case, so limits
  built on them are derived, not measured.
* **Emulations** (``emu_*``): fp32 evaluations that round to bf16 (fp16 for the CE's stored
  exponentials) exactly where the kernels do.  Where a limit cannot be derived (attention, its
  lse, the CE gradient) it is 2 x the emulation's own worst ``err / unit`` against the oracle
  (the 2 covers summation order and the 1-ulp hardware exp2 / log2 / rcp), recorded in
  ``LIMITS``.  No limit comes from a kernel's output.

The GEMM epilogues need no emulation: the RoPE epilogue rotates the fp32 accumulator (+ bias)
and rounds once at the store, and the SwiGLU epilogues compute from the bf16 gu / dy w they also
store, so each output is one rounding of an fp32 value of known inputs and its bound is derived
(``ref_rope`` / ``ref_swiglu_*`` propagate the input's bound through the operation).

The optimizer, the step's backward tail (norm backward with dres / dbias, column sums, the
embedding pair, the two-pass CE chain, LayerNorm) and the decode kernels (attn_decode, gemv_nt)
follow in their own sections: all their units are derived (their docstrings carry the
derivations), and their ``*_fp32`` / ``emu_attn_decode`` evaluations exist only to show on the CPU
that the bounds are attainable and that planted faults are not (tests/test_numerics.py).

``assert_within`` is the one assertion; ``bias_stat`` is the magnitude-bias statistic that
catches a wrong rounding mode or a slightly wrong scale, which stay inside the per-element
bound.  With ``DPFS_BOUNDS_RECORD=<file>`` in the environment both append what they measured
(case, worst err / unit, limit) to that file: the source of profiles/kernel_error_bounds.txt.
"""
from __future__ import annotations

import math
import os

import torch

U16 = 2.0 ** -8     # bf16 unit roundoff
U32 = 2.0 ** -24    # fp32 unit roundoff
U_F16 = 2.0 ** -11  # fp16 unit roundoff (the one-pass CE keeps exp(x - m_i) as fp16)
DERIVED = 1.01      # limit on err / unit where the unit is a proven bound (1 % for second-order terms)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def d(x):
    return x.double()


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round to the nearest bf16 (ties to even), keep the input's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """Chop an fp32 tensor to bf16 (the planted wrong rounding mode)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def bf16_ulp(ref64: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |ref| (normal range)."""
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -120)))
    return torch.exp2(e - 7)


def rel(a, b):
    """The suite's old statistic: global Frobenius ratio."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------ assertion ----

_RECORD = os.environ.get("DPFS_BOUNDS_RECORD")


def worst_ratio(out, ref64, unit):
    """(max err / unit, flat index); an element with unit == 0 counts as 0 when exact, inf if not."""
    err = (out.double() - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))   # nan = unwritten
    ratio = torch.where(unit > 0, err / unit.clamp_min(1e-300),
                        torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    flat = ratio.reshape(-1)
    i = int(flat.argmax())
    return float(flat[i]), i, ratio


def assert_within(out, ref64, unit, limit, what, tiles=None, where=None):
    """max(err / unit) <= limit over every element (unit == 0 demands err == 0).  ``tiles`` maps a
    dimension to the kernel's tile sizes along it, e.g. {0: (256, 128, 16), 1: (256, 192)}: the
    failure message gives the worst element's index modulo each, so an edge fault names itself.
    ``where``: a callable from the worst element's index to a string appended to the failure
    message (tests/numerics_items.py: the persistent GEMM's item, workgroup and round).
    Returns the worst ratio."""
    assert out.shape == ref64.shape == unit.shape, (what, out.shape, ref64.shape, unit.shape)
    worst, i, ratio = worst_ratio(out, ref64, unit)
    if _RECORD:
        with open(_RECORD, "a") as f:
            f.write(f"{what}\t{worst:.4g}\t{limit:.4g}\n")
    if worst <= limit:
        return worst
    idx = []
    for s in reversed(out.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    mods = "; ".join(f"dim {dim}: " + ", ".join(f"{idx[dim]} % {t} = {idx[dim] % t}" for t in ts)
                     for dim, ts in (tiles or {}).items())
    n_over = int((ratio > limit).sum())
    raise AssertionError(
        f"{what}: worst err/unit {worst:.4g} > {limit:.4g} at {idx}"
        f" (out {float(out[idx]):.8g}, ref {float(ref64[idx]):.8g}, unit {float(unit[idx]):.3g})"
        + (f" [{mods}]" if mods else "") + (f" [{where(idx)}]" if where is not None else "")
        + f"; {n_over} of {ratio.numel()} elements over the limit")


def bias_stat(out, ref64, acc_term, what, max_drop=0.10):
    """Magnitude bias of a single bf16 rounding: mean(sign(ref) (out - ref) / ulp(ref)) over the
    elements whose fp32 error term ``acc_term`` is below ulp / 16.  A round-to-nearest-even error
    is uniform on +-1/2 ulp (variance 1/12), so the mean of n of them lies within
    6 sqrt(1 / (12 n)) of 0 (six sigma); truncation gives -0.5, a 0.1 % scale error about +-0.2.
    The share of elements the restriction drops is asserted below ``max_drop``.
    Returns (mean, bound, dropped share)."""
    ulp = bf16_ulp(ref64)
    keep = (acc_term < ulp / 16) & (ref64 != 0)
    n = int(keep.sum())
    dropped = 1.0 - n / ref64.numel()
    assert dropped < max_drop, f"{what}: bias statistic drops {dropped:.1%} of the elements (limit {max_drop:.0%})"
    t = (torch.sign(ref64) * (out.double() - ref64) / ulp)[keep]
    mean, bound = float(t.mean()), 6.0 * math.sqrt(1.0 / (12.0 * n))
    if _RECORD:
        with open(_RECORD, "a") as f:
            f.write(f"{what} [bias, ulp]\t{mean:.4g}\t{bound:.4g}\n")
    assert abs(mean) <= bound, (f"{what}: magnitude bias {mean:+.4f} ulp over {n} elements, outside +-{bound:.4f} "
                                f"(wrong rounding mode or scale); {dropped:.1%} of the elements dropped")
    return mean, bound, dropped


# ----------------------------------------------------------------------------- GEMM ----

def ref_gemm(a, b, layout, bias=None, acc=None):
    """(ref, mag): layout "nt" a[M,K] b[N,K]^T (+ bias), "nn" a[M,K] b[K,N], "tn" a[K,M]^T b[K,N]
    (+ acc).  mag = |a| |b| (+ |bias|), the products' absolute sum."""
    a, b = d(a), d(b)
    if layout == "nt":
        b = b.t()
    elif layout == "tn":
        a = a.t()
    ref, mag = a @ b, a.abs() @ b.abs()
    if bias is not None:
        ref, mag = ref + d(bias), mag + d(bias).abs()
    if acc is not None:
        ref = ref + d(acc)
    return ref, mag


def acc_term_gemm(mag, K):
    """Worst-case fp32 accumulation of K products (+ bias) in any order."""
    return (K + 2) * U32 * mag


def unit_gemm_bf16(ref, mag, K):
    """bf16 output of an fp32 accumulator: round to nearest of the accumulator + its own error."""
    return U16 * ref.abs() + acc_term_gemm(mag, K)


def unit_gemm_f32(mag, K, splits, acc=None):
    """fp32 output, K products over ``splits`` slabs summed afterwards (+ the add into ``acc``)."""
    u = (K + splits + 2) * U32 * mag
    return u + U32 * d(acc).abs() if acc is not None else u


# ----------------------------------------------------------------------------- RoPE ----

def ref_rope(x64, pos, tab, n_heads, hd, inverse=False, mag=None):
    """Rotate-half RoPE of the first n_heads heads of each row of x64[M, cols] (fp64).  Returns
    (ref, rmag): rmag = |x1| |c| + |x2| |s| (or the same mix of ``mag``, an error bound of x64's
    elements, which the rotation propagates)."""
    M, h2 = x64.size(0), hd // 2
    t = d(tab)[pos.long()]
    c, s = t[:, None, :h2], t[:, None, h2:]
    if inverse:
        s = -s
    ref = x64.clone()
    m = x64.abs() if mag is None else mag
    rmag = m.clone()
    v = x64[:, : n_heads * hd].reshape(M, n_heads, hd)
    mv = m[:, : n_heads * hd].reshape(M, n_heads, hd)
    x1, x2, m1, m2 = v[..., :h2], v[..., h2:], mv[..., :h2], mv[..., h2:]
    ref[:, : n_heads * hd] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(M, -1)
    rmag[:, : n_heads * hd] = torch.cat([m1 * c.abs() + m2 * s.abs(), m2 * c.abs() + m1 * s.abs()], -1).reshape(M, -1)
    return ref, rmag


def unit_rope(ref, rmag, out_bf16=True):
    """Two products and an add in fp32 (3 roundings), then the store's rounding."""
    return (U16 if out_bf16 else U32) * ref.abs() + 3 * U32 * rmag


# --------------------------------------------------------------------------- SwiGLU ----

def gu_unperm64(gu, perm):
    """Natural [gate | up] (fp64) of a packed tensor; ``perm``: stored interleaved in 64-blocks
    (positions [128 b, 128 b + 64) = gate block b, the next 64 = up block b)."""
    gu = d(gu)
    if perm:
        sh = list(gu.shape)
        gu = gu.reshape(sh[:-1] + [sh[-1] // 128, 2, 64]).transpose(-2, -3).reshape(sh)
    F_ = gu.size(-1) // 2
    return gu[..., :F_], gu[..., F_:]


def _exp_terms(g):
    # fp32 evaluation of sigmoid(g): exp's argument g log2 e is rounded (relative error of the
    # exponential <= |g| U32 ln 2 log2 e ~ |g| U32), the 1-ulp exp2 and rcp, the add: <= (4 + |g|) U32
    return 4 + g.abs()


def ref_swiglu_fwd(gu, perm=False, bf16_out=True):
    """(h, unit, fp32 term): h = silu(gate) up; unit = one rounding at the store (bf16, or fp32
    with ``bf16_out`` off: fp32 storage) + the fp32 evaluation's terms."""
    g, u = gu_unperm64(gu, perm)
    h = g * torch.sigmoid(g) * u
    acc = (_exp_terms(g) + 3) * U32 * h.abs()
    return h, (U16 if bf16_out else U32) * h.abs() + acc, acc


def ref_swiglu_bwd(dh64, gu, perm=False, dh_unit=None, bf16_out=True):
    """(dgu natural layout, unit, fp32 term, column sums, their unit).  ``dh_unit``: an error
    bound of dh64's elements (the fused epilogue's dh is a bf16-rounded GEMM result), propagated
    through the derivative.  ``bf16_out`` off: fp32 storage, the store rounds to fp32."""
    g, u = gu_unperm64(gu, perm)
    s = torch.sigmoid(g)
    kg = u * s * (1 + g * (1 - s))
    kg_mag = u.abs() * s * (1 + g.abs() * (1 - s))      # (1 + g (1 - s) cancels near g = -1.28)
    ku = g * s
    ref = torch.cat([dh64 * kg, dh64 * ku], -1)
    mag = torch.cat([dh64.abs() * kg_mag, dh64.abs() * ku.abs()], -1)
    et = torch.cat([_exp_terms(g) + 6 + g.abs(), _exp_terms(g) + 3], -1)
    acc = et * U32 * mag
    if dh_unit is not None:
        acc = acc + torch.cat([dh_unit * kg.abs(), dh_unit * ku.abs()], -1)
    unit = (U16 if bf16_out else U32) * ref.abs() + acc
    M = ref.size(0)
    return ref, unit, acc, ref.sum(0), unit.sum(0) + (M + 1) * U32 * ref.abs().sum(0)


# ---------------------------------------------------------------------------- norms ----

def ref_rmsnorm_fwd(x, w, eps, bf16_out=True):
    """(y, unit_y, rstd, unit_rstd).  The bf16 kernel rounds x rstd to bf16 before the weight
    multiply (the reference model's rounding), so y carries two bf16 roundings."""
    x, w = d(x), d(w)
    D = x.size(-1)
    r = torch.rsqrt(x.pow(2).mean(-1) + eps)
    y = x * r[:, None] * w
    # ss: (D + 1) U32 relative (sum of D squares); rsqrt halves it; divide, add eps, 1-ulp rsqrt
    ur = (0.5 * (D + 1) + 4) * U32
    uy = (ur + 3 * U32) * y.abs()
    if bf16_out:
        uy = uy + (2 * U16 + U16 * U16) * y.abs()
    else:
        uy = uy + U32 * y.abs()
    return y, uy, r, ur * r


def ref_rmsnorm_bwd(dy, x, w, eps, dres=None, bf16_out=True):
    """(dx, unit_dx, dw, unit_dw) with rstd recomputed in fp64 from x (the kernel reads the fp32
    rstd of its forward: its (D/2 + 4) U32 relative error is inside the fp32 term)."""
    dy, x, w = d(dy), d(x), d(w)
    M, D = x.shape
    r = torch.rsqrt(x.pow(2).mean(-1) + eps)[:, None]
    xh, g = x * r, dy * w
    dot = (g * xh).sum(-1, keepdim=True) / D
    dx = r * (g - xh * dot)
    mag = r * (g.abs() + xh.abs() * (g * xh).abs().sum(-1, keepdim=True) / D)
    if dres is not None:
        dx, mag = dx + d(dres), mag + d(dres).abs()
    # row dot of D products on top of rstd's own (D/2 + 4) U32 and the few elementwise roundings
    udx = (1.5 * D + 16) * U32 * mag + (U16 if bf16_out else U32) * dx.abs()
    dw = (dy * xh).sum(0)
    udw = (M + 0.5 * D + 8) * U32 * (dy * xh).abs().sum(0)
    return dx, udx, dw, udw


def ref_bias_residual(y, bias, res, bf16_out=True):
    """(x, unit, fp32 term) of x = y + bias + res, fp32 adds, one rounding to bf16 (to fp32 with
    ``bf16_out`` off: fp32 storage)."""
    y, res = d(y), d(res)
    ref, mag = y + res, y.abs() + res.abs()
    if bias is not None:
        ref, mag = ref + d(bias), mag + d(bias).abs()
    acc = 2 * U32 * mag
    return ref, (U16 if bf16_out else U32) * ref.abs() + acc, acc


def ref_add_rmsnorm_fwd(y, bias, res, w, eps, x_kernel=None, bf16_out=True):
    """The fused residual add + RMSNorm: x = y + bias + res rounded once to bf16 (to fp32 with
    ``bf16_out`` off: fp32 storage), then the norm of that ROUNDED x.  Returns (x, unit_x, h,
    unit_h, rstd, unit_rstd); h / rstd are taken from ``x_kernel`` (the kernel's own x output)
    when given, else from the correctly rounded x."""
    x, ux, _ = ref_bias_residual(y, bias, res, bf16_out)
    xin = x_kernel if x_kernel is not None else x.to(torch.bfloat16 if bf16_out else torch.float32)
    h, uh, r, ur = ref_rmsnorm_fwd(xin, w, eps, bf16_out)
    return x, ux, h, uh, r, ur


# ------------------------------------------------------------------------ attention ----

def _bhtd(x):
    return d(x).transpose(1, 2)


def _mask(T, dev):
    return torch.ones(T, T, dtype=torch.bool, device=dev).triu(1)


def ref_attn_fwd(q, k, v, scale, causal):
    """q, k, v (B, T, H, hd) -> dict: o (B, T, H, hd), lse (B, H, T), their units, and p."""
    qf, kf, vf = _bhtd(q), _bhtd(k), _bhtd(v)
    T, hd = qf.size(-2), qf.size(-1)
    s = (qf @ kf.transpose(-1, -2)) * scale
    smag = (qf.abs() @ kf.abs().transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_mask(T, s.device), float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ vf
    unit_o = U16 * (o.abs() + p @ vf.abs())
    # lse in fp32: the scores' accumulation (softmax-weighted), the running max, exp2 / log2 and
    # the sum of up to T terms that are <= 1 relative to the row sum
    smax = s.max(-1).values
    unit_lse = U32 * (lse.abs() + smax.abs() + (hd + 2) * (p * smag).sum(-1) + 4)
    return {"o": o.transpose(1, 2), "unit_o": unit_o.transpose(1, 2), "lse": lse, "unit_lse": unit_lse, "p": p}


def _rot_bthd(x, pos, tab, absolute=False):
    """Inverse RoPE of (B, T, H, hd) fp64 (``absolute``: with |cos|, |sin| and sums: the bound)."""
    B, T, H, hd = x.shape
    h2 = hd // 2
    t = d(tab)[pos.long()].view(B, T, 1, hd)
    c, s = t[..., :h2], t[..., h2:]
    x1, x2 = x[..., :h2], x[..., h2:]
    if absolute:
        return torch.cat([x1 * c.abs() + x2 * s.abs(), x2 * c.abs() + x1 * s.abs()], -1)
    return torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)


def ref_attn_bwd(do, q, k, v, scale, causal, pos=None, tab=None):
    """The exact gradients (o and lse recomputed in fp64) -> dict of dq / dk / dv (B, T, H, hd),
    their units, and with ``pos`` / ``tab`` the inverse RoPE on dq / dk; "dbias" = column sums of
    dq | dk | dv with its unit.

    Units (x 2^-8): |dq| + scale |dS| |k| for the bf16 dS feeding the MFMA and the store, and
    scale P (sum_d |do| |o|) |k| for the bf16-rounded o inside delta = sum do o (without it the
    unit is 0 where dS cancels: query 0 of a causal row has dS == 0); dk mirrors dq;
    dv: |dv| + P^T |do|."""
    f = ref_attn_fwd(q, k, v, scale, causal)
    p = f["p"]
    qf, kf, vf, dof = _bhtd(q), _bhtd(k), _bhtd(v), _bhtd(do)
    of = f["o"].transpose(1, 2)
    dv = p.transpose(-1, -2) @ dof
    unit_dv = U16 * (dv.abs() + p.transpose(-1, -2) @ dof.abs())
    dp = dof @ vf.transpose(-1, -2)
    delta = (dof * of).sum(-1, keepdim=True)
    dmag = (dof.abs() * of.abs()).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    wq = scale * (ds.abs() + p * dmag)          # bound of the bf16 dS and of delta's bf16 o
    dq, dk = scale * (ds @ kf), scale * (ds.transpose(-1, -2) @ qf)
    in_q, in_k = wq @ kf.abs(), wq.transpose(-1, -2) @ qf.abs()
    dq, dk, dv, in_q, in_k, unit_dv = (t.transpose(1, 2) for t in (dq, dk, dv, in_q, in_k, unit_dv))
    if pos is not None:
        dq, dk = _rot_bthd(dq, pos, tab), _rot_bthd(dk, pos, tab)
        in_q, in_k = _rot_bthd(in_q, pos, tab, True), _rot_bthd(in_k, pos, tab, True)
    r = {"dq": dq, "dk": dk, "dv": dv, "unit_dq": U16 * (dq.abs() + in_q), "unit_dk": U16 * (dk.abs() + in_k),
         "unit_dv": unit_dv}
    B, T = dq.size(0), dq.size(1)
    cat = lambda a, b, c: torch.cat([t.sum((0, 1)).reshape(-1) for t in (a, b, c)])
    # fp32 column sums over B T tokens in any order + each addend's own bound
    r["dbias"] = cat(dq, dk, dv)
    r["unit_dbias"] = B * T * U32 * cat(dq.abs(), dk.abs(), dv.abs()) + cat(r["unit_dq"], r["unit_dk"], r["unit_dv"])
    return r


def emu_attn_fwd(q, k, v, scale, causal):
    """fp32 emulation of the flash forward (attention.hip attn_fwd3_k / attn_fwd_k): scores by
    fp32-accumulating MFMA, p = exp2(S c2 - m) with c2 = scale log2 e, the row sum of the
    UNROUNDED p in fp32, P rounded to bf16 as the PV MFMA's operand (`pk[k4][j] = (bf16)s[..]`),
    o = acc / l rounded to bf16 at the store, lse = (m + log2 l) ln 2 in fp32.  (The kernel's
    deferred rescale lets m lag the running max by up to 2^8: a common factor of p and l, no
    extra rounding.)  Returns (o bf16 (B, T, H, hd), lse fp32 (B, H, T))."""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    # scores and row sum accumulated in a fixed order by elementwise fp32 operations (one head
    # column / one key at a time), so the fp32-only lse does not depend on a BLAS's blocking
    sc = torch.zeros(qf.shape[:-1] + (kf.size(-2),))
    for i in range(qf.size(-1)):
        sc += qf[..., :, None, i] * kf[..., None, :, i]
    x = sc * c2
    if causal:
        x = x.masked_fill(_mask(x.size(-1), x.device), float("-inf"))
    m = x.max(-1, keepdim=True).values
    p = torch.exp2(x - m)
    l = torch.zeros_like(m)
    for j in range(p.size(-1)):
        l += p[..., j:j + 1]
    o = (bf16_round(p) @ vf) * (1.0 / l)
    lse = ((m + torch.log2(l)) * torch.tensor(LN2, dtype=torch.float32)).squeeze(-1)
    return o.transpose(1, 2).to(torch.bfloat16), lse


def emu_attn_bwd(do, q, k, v, o, lse, scale, causal, pos=None, tab=None):
    """fp32 emulation of the backward pair (attn_bwd_dq3_k + attn_bwd_dkdv3_k; the 16x16x32 pair
    rounds at the same points): delta = sum do o in fp32 from the bf16 o; p = exp2(S c2 - lse
    log2 e); dS = p (dP - delta) rounded to bf16 BEFORE the scale (`pd[..] = (bf16)vmulf(sc, dp)`),
    the operand of the dQ / dK MFMAs; P rounded to bf16 for the dV MFMA (`pp[..] = (bf16)sc`);
    dq / dk = acc * scale, inverse RoPE in fp32, one rounding at the store; the bias gradient
    sums the fp32 values before the store.  Returns (dq, dk, dv bf16 (B, T, H, hd), dbias fp32)."""
    qf, kf, vf, dof, of = (t.float().transpose(1, 2) for t in (q, k, v, do, o))
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    x = (qf @ kf.transpose(-1, -2)) * c2 - (lse.float() * torch.tensor(LOG2E, dtype=torch.float32))[..., None]
    p = torch.exp2(x)
    if causal:
        p = p.masked_fill(_mask(p.size(-1), p.device), 0.0)
    delta = (dof * of).sum(-1, keepdim=True)
    dp = dof @ vf.transpose(-1, -2) - delta
    ds = bf16_round(p * dp)
    dv = bf16_round(p).transpose(-1, -2) @ dof
    dq = (ds @ kf) * scale
    dk = (ds.transpose(-1, -2) @ qf) * scale
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


# ---------------------------------------------------------------------- one-pass CE ----

def ref_ce_fused(logits, tgt, gs, valid):
    """One-pass CE (single shard, vocab_start 0) in fp64 -> dict: stats (M, 3) = [max, sum exp(x -
    max), target logit or 0] with units, grad (M, V) = (softmax - onehot) g (0 past ``valid``)
    with its unit, dbias = column sums with unit.

    The gradient's unit: one bf16 rounding; the kernel's stored e = exp(x - m_i) (m_i the max of
    the element's 16-byte vector) is fp16: 2^-11 relative, 2^-25 absolute below fp16's normal
    range; the fp32 terms of the row sum (valid terms, any order) and of the exponentials'
    arguments."""
    x = d(logits)
    M, V = x.shape
    xv = x[:, :valid]
    mx = xv.max(1).values
    e = torch.exp(xv - mx[:, None])
    S = e.sum(1)
    hit = (tgt >= 0) & (tgt < valid)
    tl = torch.where(hit, xv.gather(1, tgt.clamp(0, valid - 1)[:, None]).squeeze(1), torch.zeros_like(mx))
    lse = mx + torch.log(S)
    g = d(gs)[:, None]
    p = torch.zeros_like(x)
    p[:, :valid] = torch.exp(xv - lse[:, None])
    onehot = torch.zeros_like(x)
    onehot[hit, tgt[hit]] = 1.0
    grad = (p - onehot) * g
    # per-16-byte-vector max (8 columns; V % 8 == 0), masked past valid
    xm = x.clone()
    xm[:, valid:] = float("-inf")
    mi = xm.view(M, V // 8, 8).max(-1, keepdim=True).values.expand(M, V // 8, 8).reshape(M, V)
    sc = torch.where(torch.isfinite(mi), torch.exp(mi - lse[:, None]), torch.zeros_like(mi))
    xabs = xv.abs().max(1).values[:, None]
    # arguments x log2 e - m log2 e (two roundings each, twice: e and the rescale), 1-ulp exp2 x 2,
    # log2, the multiplies; the row sum of `valid` terms in any order
    f32 = (valid + 16 + 8 * LOG2E * xabs) * U32 * p * g.abs()
    unit = U16 * grad.abs() + U_F16 * p * g.abs() + 2.0 ** -25 * sc * g.abs() + f32
    unit[:, valid:] = 0.0
    stats = torch.stack([mx, S, tl], 1)
    unit_S = (valid + 16 + 8 * LOG2E * xabs.squeeze(1)) * U32 * S
    unit_stats = torch.stack([torch.zeros_like(mx), unit_S, torch.zeros_like(mx)], 1)
    return {"stats": stats, "unit_stats": unit_stats, "grad": grad, "unit_grad": unit, "lse": lse,
            "dbias": grad.sum(0), "unit_dbias": unit.sum(0) + (M + 1) * U32 * grad.abs().sum(0)}


def emu_ce_fused(logits, tgt, gs, valid):
    """fp32 emulation of ce_fused_k (embedding_ce.hip): per 16-byte vector its max m_i,
    e = exp2(x log2 e - m_i log2 e) summed in fp32 and STORED AS fp16 (`v_cvt_f16_f32`), the
    (max, sum) pairs merged, p = fp16(e) * exp2(m_i log2 e - lse2) * g (- g at the target),
    rounded to bf16 at the store; the bias gradient sums the fp32 p.  Returns (stats fp32 (M, 3),
    grad bf16 (M, V), dbias fp32 (V))."""
    x = logits.float()
    M, V = x.shape
    L2E = torch.tensor(LOG2E, dtype=torch.float32)
    xm = x.clone()
    xm[:, valid:] = float("-inf")
    xg = xm.view(M, V // 8, 8)
    mi = xg.max(-1, keepdim=True).values
    ms = torch.where(torch.isfinite(mi), mi * L2E, torch.zeros_like(mi))
    e = torch.exp2(xg * L2E - ms)
    sm = e.sum(-1, keepdim=True)
    e16 = e.to(torch.float16).float()
    mx = mi.max(1, keepdim=True).values
    S = (sm * torch.where(torch.isfinite(mi), torch.exp2(ms - mx * L2E), torch.zeros_like(mi))).sum(1, keepdim=True)
    lse2 = mx * L2E + torch.log2(S)
    g = gs.float().view(M, 1, 1)
    sc = torch.where(torch.isfinite(mi), torch.exp2(ms - lse2), torch.zeros_like(mi)) * g
    p = (e16 * sc).reshape(M, V)
    hit = (tgt >= 0) & (tgt < valid)
    p[hit, tgt[hit]] -= gs.float()[hit]
    tl = torch.where(hit, x.gather(1, tgt.clamp(0, valid - 1)[:, None]).squeeze(1), torch.zeros(M, device=x.device))
    stats = torch.stack([mx.view(M), S.view(M), tl], 1)
    return stats, p.to(torch.bfloat16), p.sum(0)


# --------------------------------------------------------------------------- limits ----
# Measured on the CPU by tests/test_numerics.py's cases (the emulation against the fp64 oracle
# at every shape, family and seed the GPU tests use): `measured` is the emulation's worst
# err / unit, `limit` = 2 x measured (rounded up to two digits).  `at` names the case that
# produced the worst value.  Rounding points modelled: see emu_attn_fwd / emu_attn_bwd /
# emu_ce_fused (P before the PV and dV MFMAs, dS before the dQ / dK MFMAs, the output stores,
# the fp16 e of the one-pass CE).
ATTN_SEED = 10
def _lim(measured, at):
    return {"measured": measured, "limit": 2 * measured, "at": at}


# attention: at = (head_dim, T, causal, input family, seed), B 2, H 3; ".rope": with the inverse
# RoPE and the QKV bias gradient; CE: at = (M, V, valid, seed)
LIMITS = {
    # o: P -> bf16 before the PV MFMA, o / l -> bf16 at the store
    "attn.o.hd32": _lim(0.7519, (32, 200, True, "peaked", 10)),
    "attn.o.hd64": _lim(0.8721, (64, 63, True, "peaked", 10)),
    "attn.o.hd128": _lim(0.7808, (128, 130, False, "peaked", 10)),
    # lse: fp32 throughout (scores, exp2 against the running max, row sum, log2); no bf16 rounding;
    # the emulation accumulates scores and row sum sequentially (a fixed order on every CPU)
    "attn.lse.hd32": _lim(0.1114, (32, 200, True, "randn", 10)),
    "attn.lse.hd64": _lim(0.06716, (64, 385, True, "randn", 10)),
    "attn.lse.hd128": _lim(0.02288, (128, 300, False, "randn", 10)),
    # dq: bf16 o inside delta, dS = p (dP - delta) -> bf16 before the dQ MFMA (scale after), store
    "attn.dq.hd32": _lim(0.5168, (32, 65, True, "peaked", 10)),
    "attn.dq.hd64": _lim(0.5253, (64, 63, True, "randn", 10)),
    "attn.dq.hd128": _lim(0.4008, (128, 300, True, "peaked", 10)),
    "attn.dq.hd64.rope": _lim(0.3613, (64, 300, True, "peaked", 10)),
    "attn.dq.hd128.rope": _lim(0.3852, (128, 300, True, "randn", 10)),
    # dk: the same dS -> bf16 before the dK MFMA, scale and inverse RoPE in fp32, store
    "attn.dk.hd32": _lim(0.6189, (32, 200, True, "randn", 10)),
    "attn.dk.hd64": _lim(0.6934, (64, 300, True, "randn", 10)),
    "attn.dk.hd128": _lim(0.5989, (128, 300, True, "randn", 10)),
    "attn.dk.hd64.rope": _lim(0.7598, (64, 300, True, "randn", 10)),
    "attn.dk.hd128.rope": _lim(0.5575, (128, 300, True, "randn", 10)),
    # dv: P -> bf16 before the dV MFMA, store
    "attn.dv.hd32": _lim(0.8894, (32, 200, True, "peaked", 10)),
    "attn.dv.hd64": _lim(0.9468, (64, 385, True, "peaked", 10)),
    "attn.dv.hd128": _lim(0.9262, (128, 300, True, "peaked", 10)),
    # dbias: fp32 column sums of the dq | dk | dv accumulators before their bf16 stores (the unit
    # sums the addends' worst cases, so independent rounding errors stay far below it)
    "attn.dbias.hd64.rope": _lim(0.02848, (64, 300, True, "peaked", 10)),
    "attn.dbias.hd128.rope": _lim(0.03431, (128, 300, True, "peaked", 10)),
    # one-pass CE gradient: e = exp2(x log2 e - m_i log2 e) -> fp16 in place of the input,
    # p = e exp2(m_i log2 e - lse2) g (- g at the target) -> bf16 at the store
    "ce.grad": _lim(0.9866, (77, 6288, 6241, 17)),
    # its bias-gradient partials: fp32 column sums of p before the store
    "ce.dbias": _lim(0.06239, (77, 6288, 6241, 17)),
}


def limit(key):
    return LIMITS[key]["limit"]


# the GPU tests' attention cases, shared with the CPU measurement: (hd, T, causal)
ATTN_CASES = ([(64, T, True) for T in (1, 17, 63, 65, 129, 300, 385)] + [(128, T, True) for T in (65, 300)]
              + [(32, T, True) for T in (65, 200)] + [(hd, T, False) for hd in (64, 128) for T in (130, 300)])
ATTN_FAMILIES = {"randn": 1.0, "peaked": 3.0}     # q and k scaled: flat softmax / near one-hot rows
ATTN_ROPE_CASES = [(64, 300), (128, 300)]
CE_CASES = [(300, 1000, 997), (77, 6288, 6241)]
CE_SEED = 17


def packed_views(qkv, B, T, H, hd):
    """The q | k | v column blocks of a packed (B T, 3 H hd) buffer as (B, T, H, hd) views with the
    step's batch and token strides (explicit strides: a plain view of T = 1 gets others)."""
    ld = qkv.size(1)
    return tuple(qkv.as_strided((B, T, H, hd), (T * ld, ld, hd, 1), i * H * hd) for i in range(3))


def attn_inputs(hd, T, family, device="cpu", B=2, H=3, seed=ATTN_SEED):
    """q, k, v as views of a packed (B T, 3 H hd) bf16 buffer (the step's strides), do, and RoPE
    positions / table.  Generated on the CPU so the CPU measurement and the GPU tests see the
    same values."""
    gen = torch.Generator().manual_seed(seed + 1000 * hd + T)
    qkv = torch.randn(B * T, 3 * H * hd, generator=gen)
    qkv[:, : 2 * H * hd] *= ATTN_FAMILIES[family]
    qkv = qkv.bfloat16().to(device)
    q, k, v = packed_views(qkv, B, T, H, hd)
    do = torch.randn(B, T, H, hd, generator=gen).bfloat16().to(device)
    pos = torch.randint(0, 512, (B * T,), generator=gen).to(device)
    return q, k, v, do, pos


def ce_inputs(M, V, valid, device="cpu", seed=CE_SEED):
    gen = torch.Generator().manual_seed(seed + V)
    logits = (3 * torch.randn(M, V, generator=gen)).bfloat16()
    tgt = torch.randint(0, valid, (M,), generator=gen)
    tgt[::7] = -1                                   # ignore_index rows: g = 0
    gs = (tgt >= 0).float() / max(1, int((tgt >= 0).sum()))
    return logits.to(device), tgt.to(device), gs.to(device)


def rope_table(maxlen, hd, theta=10000.0):
    """fp32 (maxlen, hd) table [cos | sin] of the hd / 2 frequencies (an input of the kernels)."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    ang = torch.arange(maxlen).float().unsqueeze(1) * inv
    return torch.cat([torch.cos(ang), torch.sin(ang)], 1)


def attn_refs(q, k, v, do, scale, causal, pos=None, tab=None):
    """Forward and backward oracles in one dict: o, lse, dq, dk, dv, dbias and unit_<name>."""
    r = ref_attn_fwd(q, k, v, scale, causal)
    r.update(ref_attn_bwd(do, q, k, v, scale, causal, pos, tab))
    return r


def attn_key(name, hd, rope=False):
    """LIMITS key of an attention output: per output and head_dim (the kernels differ per head_dim);
    the inverse-RoPE form of dq / dk / dbias separately."""
    return f"attn.{name}.hd{hd}" + (".rope" if rope else "")


ATTN_TILES = {"o": {1: (128, 64, 32)}, "dq": {1: (128, 64, 32)}, "dk": {1: (128, 64, 32)}, "dv": {1: (128, 64, 32)},
              "lse": {2: (128, 64, 32)}, "dbias": {}}


# ============================================================================== Adam ====

ADAM_CHUNK = 16384            # adam.hip kAdamChunk: elements per workgroup
# (elements, bf16 shadow): below one 16-byte vector (scalar path), one vector, a 4-element last
# chunk on the vector path (16384 + 4), the scalar path across chunks (2 * 16384 + 7)
ADAM_TABLE = [(1, False), (3, True), (4, True), (1000, False), (16384, True), (16384 + 4, False), (2 * 16384 + 7, True)]
ADAM_SENTINEL = -7.0          # fills the slabs the tensors are views of (exact in bf16)
ADAM_PAD = 64                 # sentinel elements on each side (keeps the views 16-byte aligned)
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999)
# name: (step, random moments, weight decay, eps, grad_scale, dscale, planted zeros)
#   planted "v0": v = 0 on every third element (eps placement); "still": g = m = v = 0 on every
#   fifth element, which with wd = 0 must leave p bit-identical
ADAM_RUNS = {
    "fresh":      (1, False, 0.0, 1e-8, 1.0, None, "still"),
    "step2":      (2, True, 0.1, 1e-8, 1.0, None, None),
    "step1000":   (1000, True, 0.0, 1e-8, 1.0, None, "still"),
    "eps1e-3":    (2, True, 0.1, 1e-3, 1.0, None, "v0"),
    "gscale":     (2, True, 0.1, 1e-8, 0.5, None, None),
    "dscale":     (2, True, 0.1, 1e-8, 1.0, 0.25, None),
    "both":       (1000, True, 0.1, 1e-8, 0.5, 0.25, None),
}


def f32(x):
    """A Python float rounded to fp32 (what `(float)x` gives the kernels), as a Python float."""
    return float(torch.tensor(x, dtype=torch.float64).float())


def adam_scalars(lr, b1, b2, eps, wd, step, gscale=1.0):
    """The kernel arguments as csrc/bindings/optim.cpp rounds them: bc1 = 1 - b1^step and
    sqrt(1 - b2^step) are evaluated in double from the double betas and rounded once; 1 - b1 and
    1 - b2 are fp32 subtractions of the rounded betas (adam_k's `1.f - b1`)."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return {"lr": f32(lr), "b1": f32(b1), "b2": f32(b2), "eps": f32(eps), "wd": f32(wd),
            "bc1": f32(1.0 - math.pow(b1, step)), "bc2s": f32(math.sqrt(1.0 - math.pow(b2, step))),
            "gscale": f32(gscale),
            "omb1": float(one - torch.tensor(b1, dtype=torch.float32)),
            "omb2": float(one - torch.tensor(b2, dtype=torch.float32))}


def ref_adam(p, g, m, v, sc, dscale=1.0, s_err=0.0):
    """One Adam step (torch.optim.Adam semantics, L2 decay in the gradient) in fp64 from fp32
    state -> dict p, m, v and unit_p, unit_m, unit_v.  ``dscale``: the fp32 device scalar;
    ``s_err``: a bound, in units of U32, of that scalar's own relative error against the exact
    coefficient the oracle is fed (0 when it is given exactly).

    Units, with u = U32 and every fp32 operation within u relative (an FMA contraction only
    removes roundings).  The build has no fast-math flag and hipcc rounds fp32 `/` and sqrtf
    correctly by default, so the three divisions (lr / bc1, sqrt(v) / bc2s, the update's) and the
    square root are taken as correctly rounded: 1 u each, none gets an extra ulp.
      G  = g s + wd p          s = gscale * dscale (1), the two products (1 each), the add (1):
                               e_G = (3 + s_err) u |g s| + 3 u |wd p|
      m' = b1 m + (1 - b1) G   e_m = (1 - b1) e_G + 2 u (|b1 m| + (1 - b1) |G|)
      v' = b2 v + (1 - b2) G G e_v = 2 (1 - b2) |G| e_G + 3 u v'
      D  = sqrt(v') / bc2s + eps:  |sqrt a - sqrt b| <= min(|a - b| / sqrt a, sqrt |a - b|), then
                               the root, the division and the add: e_D = e_rt / bc2s + 3 u D
      upd = (lr / bc1) m' / D  e_upd = 3 u |upd| + (lr / bc1) e_m / D + |upd| e_D / D
      p' = p - upd             e_p = u |p'| + e_upd"""
    p, g, m, v = d(p), d(g), d(m), d(v)
    s = sc["gscale"] * dscale
    gs, wp = g * s, sc["wd"] * p
    G = gs + wp
    eG = U32 * ((3 + s_err) * gs.abs() + 3 * wp.abs())
    b1m = sc["b1"] * m
    m1 = b1m + sc["omb1"] * G
    um = sc["omb1"] * eG + 2 * U32 * (b1m.abs() + sc["omb1"] * G.abs())
    v1 = sc["b2"] * v + sc["omb2"] * G * G
    uv = 2 * sc["omb2"] * G.abs() * eG + 3 * U32 * v1
    rt = v1.sqrt()
    ert = torch.minimum(uv / rt.clamp_min(1e-300), uv.sqrt())
    D = rt / sc["bc2s"] + sc["eps"]
    uD = ert / sc["bc2s"] + 3 * U32 * D
    step = sc["lr"] / sc["bc1"]
    upd = step * m1 / D
    uupd = 3 * U32 * upd.abs() + step * um / D + upd.abs() * uD / D
    p1 = p - upd
    return {"p": p1, "m": m1, "v": v1, "unit_p": U32 * p1.abs() + uupd, "unit_m": um, "unit_v": uv}


def adam_fp32(p, g, m, v, sc, dscale=None, fault=None):
    """adam_k's own expression evaluated in fp32 on the CPU (the attainability proof), with the
    planted faults of tests/test_numerics.py.  Returns (p, m, v) fp32."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    p, g, m, v = p.float().clone(), g.float(), m.float().clone(), v.float().clone()
    scale = t(sc["gscale"]) * (t(1.0) if dscale is None or fault == "dscale_ignored" else t(dscale))
    wd = t(sc["wd"]) * (scale if fault == "wd_clipped" else t(1.0))
    b1, b2, bc2s, eps = t(sc["b1"]), t(sc["b2"]), t(sc["bc2s"]), t(sc["eps"])
    if fault == "bc2_not_sqrt":
        bc2s = bc2s * bc2s
    step = t(sc["lr"]) / t(sc["bc1"])
    gg = g * scale + wd * p
    m1 = b1 * m + (t(1.0) - b1) * gg
    v1 = b2 * v + (t(1.0) - b2) * gg * gg
    den = (v1.sqrt() + eps) / bc2s if fault == "eps_before_division" else v1.sqrt() / bc2s + eps
    p1 = p - step * m1 / den
    if fault == "last_vector_skipped":      # the last 16-byte vector of every chunk left as it was
        n = p.numel()
        for c1 in list(range(ADAM_CHUNK, n, ADAM_CHUNK)) + [n]:
            lo = max(c1 - 4, 0)
            p1[lo:c1], m1[lo:c1], v1[lo:c1] = p[lo:c1], m[lo:c1], v[lo:c1]
    return p1, m1, v1


def adam_inputs(run, seed=31):
    """Per tensor of ADAM_TABLE the CPU fp32 (p, g, m, v) of a run of ADAM_RUNS."""
    step, rand_moments, wd, eps, gscale, dscale, plant = ADAM_RUNS[run]
    gen = torch.Generator().manual_seed(seed + step)
    out = []
    for n, _ in ADAM_TABLE:
        p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        m = 0.1 * torch.randn(n, generator=gen) if rand_moments else torch.zeros(n)
        v = (0.1 * torch.randn(n, generator=gen)) ** 2 if rand_moments else torch.zeros(n)
        if plant == "v0":
            v[::3] = 0
        if plant == "still":
            g[::5], m[::5], v[::5] = 0, 0, 0
        out.append((p, g, m, v))
    return out


def ref_grad_sumsq(grads):
    """(sum of squares of every gradient in fp64, unit): sumsq_k adds a chunk's squares (products
    included: n_chunk + 1 roundings at worst), the host adds the n_chunks partials."""
    s = sum(float(d(g).pow(2).sum()) for g in grads)
    n_chunks = sum((g.numel() + ADAM_CHUNK - 1) // ADAM_CHUNK for g in grads)
    return s, (ADAM_CHUNK + n_chunks + 2) * U32 * s


# ===================================================================== the step's tail ====

def ref_colsum(x, extra_unit=None):
    """(column sums in fp64, unit): M fp32 addends in any order over chunks and stages; with
    ``extra_unit`` the addends' own error bounds summed on top."""
    x = d(x)
    M = x.size(0)
    u = (M + 2) * U32 * x.abs().sum(0)
    return x.sum(0), u if extra_unit is None else u + extra_unit.sum(0)


def ref_rmsnorm_bwd_dbias(dy, x, w, eps, dres=None, bf16_out=True):
    """ref_rmsnorm_bwd + (dbias, unit_dbias): the column sums of the UNROUNDED fp32 dx (+ dres)
    (MODE 2 sums before the store), so the addends carry the fp32 term of unit_dx only."""
    dx, udx, dw, udw = ref_rmsnorm_bwd(dy, x, w, eps, dres, bf16_out)
    f32_term = udx - (U16 if bf16_out else U32) * dx.abs()
    db, udb = ref_colsum(dx, f32_term)
    return dx, udx, dw, udw, db, udb


EMB_SEG_LENS = (130, 8, 5, 4, 3, 1, 0)   # per local row, longest first (v_local 1: 130; 3: 130, 8, 5)


def emb_ids(M, v_local, start, seed):
    """M token ids for the shard [start, start + v_local): the first local rows get the segment
    lengths EMB_SEG_LENS (the four-at-a-time loop, its tail of 1 to 3, an empty row; without the
    130 when M < 200), the rest are spread over the other local rows and both neighbouring
    shards, with the boundary ids start - 1, start + v_local - 1 and start + v_local."""
    gen = torch.Generator().manual_seed(seed)
    lens = (EMB_SEG_LENS if M >= 200 else EMB_SEG_LENS[1:])[:v_local]
    ids = [start + r for r, n in enumerate(lens) for _ in range(n)] + [start + v_local]
    if start > 0:
        ids.append(start - 1)
    if v_local > len(lens):
        ids.append(start + v_local - 1)
    fill = torch.randint(start + len(lens), start + 2 * v_local + 8, (M - len(ids),), generator=gen)
    if start > 0:
        below = torch.randint(0, start, fill.shape, generator=gen)
        fill = torch.where(torch.rand(fill.shape, generator=gen) < 0.25, below, fill)
    ids = torch.cat([torch.tensor(ids, dtype=torch.int64), fill])
    return ids[torch.randperm(M, generator=gen)]


def ref_embedding_bwd(dout, ids, v_local, start, acc=None):
    """(dw fp64 (v_local, D), unit): rows summed per id in fp64; unit (count + 1) U32 sum|rows|
    (+ U32 |acc| with accumulate).  The rows enter the fp32 sum unrounded whether dout is bf16 or
    fp32, so the unit holds for both."""
    dd = d(dout)
    hit = (ids >= start) & (ids < start + v_local)
    loc = (ids - start)[hit]
    D = dd.size(1)
    dw = torch.zeros(v_local, D, dtype=torch.float64, device=dd.device).index_add_(0, loc, dd[hit])
    mag = torch.zeros_like(dw).index_add_(0, loc, dd[hit].abs())
    cnt = torch.zeros(v_local, dtype=torch.float64, device=dd.device).index_add_(0, loc, torch.ones_like(loc, dtype=torch.float64))
    unit = (cnt[:, None] + 1) * U32 * mag
    if acc is not None:
        dw, unit = dw + d(acc), unit + U32 * d(acc).abs()
    return dw, unit


# ----------------------------------------------------------------------- two-pass CE ----
# The vocab-parallel chain: ce_fwd_stats per shard -> ce_finalize over the gathered (nsh, M, 3)
# statistics -> ce_grad_scale -> ce_bwd (+ dbias) per shard.  Every stage is checked from the
# kernel's own previous stage (its fp32 lse and gs are the next oracle's inputs), so nothing
# compounds and every limit is DERIVED.

def ce_levels(valid):
    """Merges an element's exponential passes through in ce_stats_k: a thread's trips over the row
    (256 threads), six butterfly steps, three wave merges, its own vector's sum."""
    return (valid + 255) // 256 + 10


def ref_ce_stats(logits, tgt, start, valid):
    """(stats (M, 3) fp64, unit).  max and target logit are selections: exact.  sum exp(x - max):
    each term reaches the result through `levels` merges s exp(m_old - m_new); the maxima only
    grow, so the exponents' arguments telescope to max - x <= R (R = max - min of the row) and the
    argument roundings (the subtraction and the x log2 e inside __expf, U32 |argument| each) sum
    to 2 R U32; each level adds an __expf (3 ulp allowed), a product and an add: 5 U32; the
    eight-term sum inside a vector 8 U32.  Nothing assumes bf16 inputs: with fp32 logits a
    vector holds four terms and a thread makes at most as many trips, so the same unit holds."""
    x = d(logits)[:, :valid]
    M = x.size(0)
    z = torch.zeros(M, dtype=torch.float64, device=x.device)
    if valid == 0:
        return torch.stack([z - float("inf"), z, z], 1), torch.zeros(M, 3, dtype=torch.float64, device=x.device)
    mx = x.max(1).values
    S = torch.exp(x - mx[:, None]).sum(1)
    R = mx - x.min(1).values
    loc = tgt - start
    hit = (loc >= 0) & (loc < valid)
    tl = torch.where(hit, x.gather(1, loc.clamp(0, valid - 1)[:, None]).squeeze(1), z)
    uS = (5 * ce_levels(valid) + 8 + 2 * R) * U32 * S
    return torch.stack([mx, S, tl], 1), torch.stack([z, uS, z], 1)


def ref_ce_finalize(stats, tgt, ignore, unit_S=None):
    """From gathered fp32 statistics (nsh, M, 3) (the kernels' own) -> dict lse, unit_lse, valid,
    loss_sum, unit_loss_sum, count.  lse = mx + log(sum_sh S exp(m - mx)): per shard an __expf
    ((3 + 2 |m - mx|) U32), a product and an add; __logf = log2 ln 2 (3 U32 |log| and an absolute
    4 U32 for the hardware log2 near 1); the add (U32 |lse|).  ``unit_S``: the statistics' own
    bound when the oracle is fed exact ones."""
    st = d(stats)
    nsh, M, _ = st.shape
    mx = st[..., 0].max(0).values
    fin = torch.isfinite(st[..., 0])
    w = torch.where(fin, torch.exp(st[..., 0] - mx), torch.zeros_like(mx))
    terms = st[..., 1] * w
    se = terms.sum(0)
    dm = torch.where(fin, (st[..., 0] - mx).abs(), torch.zeros_like(mx))
    use = ((5 + 2 * dm) * U32 * terms).sum(0) + nsh * U32 * se
    if unit_S is not None:
        use = use + (unit_S * w).sum(0)
    lg = torch.log(se)
    lse = mx + lg
    unit_lse = use / se + U32 * (3 * lg.abs() + 4 + lse.abs())
    valid = (tgt != ignore).double()
    tl = st[..., 2].sum(0)
    row = (lse - tl) * valid
    # tl: nsh - 1 adds of zeros and one value (exact); l - tl one rounding; the sum over M rows
    unit_sum = ((unit_lse + U32 * row.abs()) * valid).sum() + (M + 2) * U32 * row.abs().sum()
    return {"lse": lse, "unit_lse": unit_lse, "valid": valid, "loss_sum": row.sum(), "unit_loss_sum": unit_sum,
            "count": valid.sum()}


def ref_ce_bwd(logits, tgt, lse, gs, start, valid, bf16_out=True):
    """(grad (M, V) fp64, unit, dbias, unit_dbias) from the fp32 lse and gs the kernel is given:
    grad = (exp(x - lse) - onehot) gs, 0 past ``valid``.  fp32 term: the argument x - lse rounded
    (U32 (|x| + |lse|)), __expf's x log2 e (the same) and 3 ulp, the subtraction of 1 and the
    product: p (2 (|x| + |lse|) + 3) U32 |gs| + 2 U32 |grad|; then one rounding at the store.
    dbias sums the fp32 values before the store."""
    x = d(logits)
    M, V = x.shape
    l, g = d(lse)[:, None], d(gs)[:, None]
    p = torch.exp(x - l)
    p[:, valid:] = 0
    loc = tgt - start
    hit = (loc >= 0) & (loc < valid)
    onehot = torch.zeros_like(x)
    onehot[hit, loc[hit]] = 1.0
    grad = (p - onehot) * g
    f32t = p * (2 * (x.abs() + l.abs()) + 3) * U32 * g.abs() + 2 * U32 * grad.abs()
    unit = (U16 if bf16_out else U32) * grad.abs() + f32t
    db, udb = ref_colsum(grad, f32t)
    return grad, unit, db, udb


def ce_fp32(logits, tgt, start, valid):
    """ce_stats_k's math in fp32 on the CPU (the attainability proof): per 8-vector max and sum,
    merged pairwise.  Returns stats fp32 (M, 3)."""
    x = logits.float()[:, :valid]
    M = x.size(0)
    pad = (-valid) % 8
    xp = torch.cat([x, torch.full((M, pad), float("-inf"))], 1).view(M, -1, 8)
    m = xp.max(-1).values
    s = torch.exp(xp - m[..., None]).sum(-1)
    while m.size(1) > 1:
        if m.size(1) % 2:
            m = torch.cat([m, torch.full((M, 1), float("-inf"))], 1)
            s = torch.cat([s, torch.zeros(M, 1)], 1)
        ma, mb, sa, sb = m[:, 0::2], m[:, 1::2], s[:, 0::2], s[:, 1::2]
        mm = torch.maximum(ma, mb)
        s = sa * torch.exp(ma - mm) + torch.where(torch.isfinite(mb), sb * torch.exp(mb - mm), torch.zeros_like(sb))
        m = mm
    loc = tgt - start
    hit = (loc >= 0) & (loc < valid)
    tl = torch.where(hit, logits.float().gather(1, loc.clamp(0, max(valid - 1, 0))[:, None]).squeeze(1), torch.zeros(M))
    return torch.stack([m[:, 0], s[:, 0], tl], 1)


def ce_finalize_fp32(stats, tgt, ignore, only_shard=None):
    """ce_finalize_rows_k in fp32 -> (lse, valid, loss sum, count); ``only_shard``: the planted
    fault (the lse from one shard's statistics)."""
    st = stats.float() if only_shard is None else stats.float()[only_shard:only_shard + 1]
    mx = st[..., 0].max(0).values
    se = (st[..., 1] * torch.exp(st[..., 0] - mx)).sum(0)
    lse = mx + torch.log(se)
    valid = (tgt != ignore).float()
    return lse, valid, ((lse - stats.float()[..., 2].sum(0)) * valid).sum(), valid.sum()


def ce_bwd_fp32(logits, tgt, lse, gs, start, valid, onehot_start=None):
    """ce_bwd_k in fp32 -> (grad in the logits' dtype, dbias fp32); ``onehot_start``: the planted
    fault (the target looked up with another shard's vocab_start)."""
    x = logits.float()
    p = torch.exp(x - lse.float()[:, None])
    p[:, valid:] = 0
    loc = tgt - (start if onehot_start is None else onehot_start)
    hit = (loc >= 0) & (loc < valid)
    p[hit, loc[hit]] -= 1.0
    gr = p * gs.float()[:, None]
    return gr.to(logits.dtype), gr.sum(0)


CE2_SEED = 19


def ce2_inputs(M, V, shards, device="cpu", seed=CE2_SEED, all_ignored=False, dtype=torch.bfloat16):
    """Per shard of ``shards`` = [(vocab_start, valid), ...] logits (M, V) of ``dtype`` (bf16, or
    fp32 for the fp32 engine's storage), and the targets: in every shard, beyond the last one (a
    valid row without a target logit), every seventh -1."""
    gen = torch.Generator().manual_seed(seed + V + len(shards))
    logits = [(3 * torch.randn(M, V, generator=gen)).to(dtype).to(device) for _ in shards]
    top = shards[-1][0] + shards[-1][1]
    tgt = torch.randint(0, top + 5, (M,), generator=gen)
    for i, (st, va) in enumerate(shards):
        if 2 * i + 1 < M:
            tgt[2 * i + 1] = st + va - 1          # the last valid column of each shard
    if M > 4:
        tgt[4] = top + 2                          # beyond every shard: a valid row, target logit 0
    tgt[::7] = -1
    if all_ignored:
        tgt[:] = -1
    return logits, tgt.to(device)


# ------------------------------------------------------------------------- LayerNorm ----

def ref_layernorm_fwd(x, w, b, eps, bf16_out=True):
    """dict y, mean, rstd and units.  mean: D adds and the division, (D + 2) U32 sum|x| / D.
    var = sum (x - mean)^2 / D: each centred value carries the mean's error and its own
    rounding; rstd: half the variance's relative error, the division, the add and the 1-ulp
    rsqrt (4 U32).  y = (x - mean) rstd w + b: three products / differences and the add in fp32,
    one rounding at the store."""
    x, w, b = d(x), d(w), d(b)
    D = x.size(-1)
    mu = x.mean(-1, keepdim=True)
    umu = (D + 2) * U32 * x.abs().sum(-1, keepdim=True) / D
    c = x - mu
    var = c.pow(2).mean(-1, keepdim=True)
    uvar = (2 * c.abs() * (umu + U32 * c.abs())).sum(-1, keepdim=True) / D + (D + 3) * U32 * var
    r = torch.rsqrt(var + eps)
    ur_rel = 0.5 * uvar / (var + eps) + 4 * U32
    t = c * r * w
    y = t + b
    uy = t.abs() * (ur_rel + 4 * U32) + w.abs() * r * umu + U32 * (t.abs() + b.abs()) + (U16 if bf16_out else U32) * y.abs()
    return {"y": y, "unit_y": uy, "mean": mu.squeeze(-1), "unit_mean": umu.squeeze(-1), "rstd": r.squeeze(-1),
            "unit_rstd": (ur_rel * r).squeeze(-1), "_ur_rel": ur_rel, "_umu": umu}


def ref_layernorm_bwd(dy, x, w, eps, bf16_out=True):
    """dict dx, dw, db and units, mean / rstd recomputed in fp64 (the kernel reads the fp32 ones
    of its forward: their bounds enter through xh).  dx = rstd (g - mean(g) - xh mean(g xh)),
    g = dy w, xh = (x - mean) rstd; dw = sum_rows dy xh, db = sum_rows dy."""
    f = ref_layernorm_fwd(x, w, torch.zeros_like(w), eps, bf16_out)
    dy, x, w = d(dy), d(x), d(w)
    M, D = x.shape
    r, ur_rel, umu = f["rstd"][:, None], f["_ur_rel"], f["_umu"]
    xh = (x - f["mean"][:, None]) * r
    uxh = r * umu + xh.abs() * (ur_rel + 2 * U32)
    g = dy * w
    dot = (g * xh).mean(-1, keepdim=True)
    udot = (D + 3) * U32 * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * uxh).mean(-1, keepdim=True)
    gs = g.mean(-1, keepdim=True)
    ugs = (D + 3) * U32 * g.abs().mean(-1, keepdim=True)
    inner = g - gs - xh * dot
    uin = (U32 * g.abs() + ugs + xh.abs() * udot + dot.abs() * uxh + U32 * (xh * dot).abs()
           + 2 * U32 * (g.abs() + gs.abs() + (xh * dot).abs()))
    dx = r * inner
    udx = r * uin + dx.abs() * (ur_rel + U32) + (U16 if bf16_out else U32) * dx.abs()
    dw = (dy * xh).sum(0)
    udw = (dy.abs() * uxh).sum(0) + (M + 3) * U32 * (dy * xh).abs().sum(0)
    db, udb = ref_colsum(dy)
    return {"dx": dx, "unit_dx": udx, "dw": dw, "unit_dw": udw, "db": db, "unit_db": udb}


def norm_fp32(dy, x, w, mode, dres=None, eps=1e-5, fault=None, grid_rows=4096):
    """norm_bwd_k's math in fp32 on the CPU: mode 0 / 2 RMSNorm (2: + column sums of the fp32 dx),
    1 LayerNorm.  Returns (dx in x's dtype, dw, db or None).  Faults: "rows_past_grid" (dw / db
    without the rows past the first ``grid_rows``), "dres_after_rounding" (dres added to the
    rounded dx)."""
    xf, dyf, wf = x.float(), dy.float(), w.float()
    D = xf.size(1)
    mu = xf.mean(-1, keepdim=True) if mode == 1 else torch.zeros(xf.size(0), 1)
    r = torch.rsqrt((xf - mu).pow(2).mean(-1, keepdim=True) + eps)
    xh, g = (xf - mu) * r, dyf * wf
    dot = (g * xh).sum(-1, keepdim=True) / D
    gs = g.sum(-1, keepdim=True) / D if mode == 1 else 0.0
    o = r * (g - gs - xh * dot)
    if dres is not None:
        o = o.to(x.dtype).float() + dres.float() if fault == "dres_after_rounding" else o + dres.float()
    n = grid_rows if fault == "rows_past_grid" else xf.size(0)
    dw = (dyf * xh)[:n].sum(0)
    db = dyf[:n].sum(0) if mode == 1 else (o[:n].sum(0) if mode == 2 else None)
    return o.to(x.dtype), dw, db


# ============================================================================ decode ====

DEC_B, DEC_H = 2, 3
DEC_HD = (32, 64, 128)
DEC_TMAX = (16, 300, 512)
DEC_FAMILIES = ("randn", "peaked", "rising")
DEC_SEED = 41


def dec_lengths(Tmax):
    """The cache lengths a capacity is run at: 0, 1, the 64-key wave and 256-key split edges that
    fit, and T_max - 1, T_max, T_max + 5 (the last two: a full cache, T_max keys attended)."""
    return sorted({t for t in (0, 1, 62, 63, 64, 255, 256, 257) if t < Tmax - 1} | {Tmax - 1, Tmax, Tmax + 5})


def dec_inputs(hd, Tmax, family, device="cpu", B=DEC_B, H=DEC_H, seed=DEC_SEED):
    """(qkv packed [B, 3 H hd], k cache, v cache [B, Tmax, H, hd]) bf16 from a seeded CPU
    generator.  peaked: q and k x 3; rising: key t x (1 + 6 t / Tmax)."""
    gen = torch.Generator().manual_seed(seed + 1000 * hd + Tmax)
    qkv = torch.randn(B, 3 * H * hd, generator=gen)
    kc = torch.randn(B, Tmax, H, hd, generator=gen)
    vc = torch.randn(B, Tmax, H, hd, generator=gen)
    if family == "peaked":
        qkv[:, : H * hd] *= 3
        kc *= 3
    elif family == "rising":
        kc *= (1 + 6 * torch.arange(Tmax).float() / Tmax).view(1, Tmax, 1, 1)
    return qkv.bfloat16().to(device), kc.bfloat16().to(device), vc.bfloat16().to(device)


def dec_selection_inputs(hd, Tmax, length, device="cpu", B=DEC_B, H=DEC_H, seed=DEC_SEED):
    """The exact key-selection case: per (b, h) one key t* of {0, 63, 64, 255, 256, the newest}
    (those inside the attended keys) has k[t*, 0] = 16, every other key -16, q[0] = 16, all other
    q / k entries 0.  The scores differ by 512 hd^-1/2 >= 45, so the other probabilities are
    below e^-45 and o[b, h] == v[b, t*, h] bit for bit.  Returns (qkv, kc, vc, tstar [B, H], len [B])."""
    gen = torch.Generator().manual_seed(seed + hd + Tmax + length)
    L = min(length + 1, Tmax)
    cands = [t for t in (0, 63, 64, 255, 256) if t < L - 1] + [L - 1]
    tstar = torch.tensor([[cands[(b * H + h) % len(cands)] for h in range(H)] for b in range(B)])
    qkv = torch.zeros(B, 3 * H * hd)
    qkv[:, : H * hd : hd] = 16
    kc = torch.zeros(B, Tmax, H, hd)
    kc[..., 0] = -16
    for b in range(B):
        for h in range(H):
            kc[b, tstar[b, h], h, 0] = 16
    vc = torch.randn(B, Tmax, H, hd, generator=gen)
    ln = torch.full((B,), length, dtype=torch.int32)
    return qkv.bfloat16().to(device), kc.bfloat16().to(device), vc.bfloat16().to(device), tstar, ln.to(device)


def dec_attended(lens, Tmax):
    """Keys attended per sequence: the cached ones and the token being decoded, inside the cache."""
    return torch.clamp(lens.long() + 1, max=Tmax)


def ref_attn_decode(q, kc, vc, lens, scale):
    """q [B, >= H hd] (the first H hd columns), caches [B, Tmax, H, hd], lens [B] -> (o [B, H hd]
    fp64, unit).  Cache rows past each sequence's attended keys are never read (they may be NaN).

    The kernels keep p in fp32 and merge waves and splits in fp32, so o is ONE bf16 rounding of
    fp32 arithmetic.  With w_t the weight of key t (the product of up to three __expf: against
    the wave's max, the split's, the global one; the maxima themselves cancel exactly), o =
    sum w_t v_t / sum w_t, and a relative error e_t of w_t moves o by at most
    sum p_t e_t |v_t| + (sum p_t |v_t|) (sum p_t e_t).  e_t collects
      * the score: q scale rounded, hd FMAs: (hd + 2) U32 scale sum |q| |k_t|;
      * three subtractions of scores (each |difference| <= 2 A, A = max |s|): 6 A U32;
      * three __expf = exp2(x log2 e): the argument's rounding |x| U32 and an allowance of
        3 ulp each for v_exp_f32 and its range handling: 3 (3 + 2 A) U32;
      * the two merge multiplications: 2 U32.
    Both sums accumulate L terms in fp32 in some order ((L + 1) U32 each, Higham 4.2), then the
    reciprocal, the product and the bf16 store: 3 U32 and U16 |o|."""
    B, Tmax, H, hd = kc.shape
    L = dec_attended(lens, Tmax).to(kc.device)
    live = torch.arange(Tmax, device=kc.device)[None, :] < L[:, None]                 # [B, T]
    z = torch.zeros((), dtype=torch.float64, device=kc.device)
    k = torch.where(live[:, :, None, None], d(kc), z).permute(0, 2, 1, 3)              # [B, H, T, hd]
    v = torch.where(live[:, :, None, None], d(vc), z).permute(0, 2, 1, 3)
    qh = d(q)[:, : H * hd].reshape(B, H, 1, hd)
    s = (qh * k).sum(-1) * scale                                                      # [B, H, T]
    smag = (qh.abs() * k.abs()).sum(-1) * scale
    neg = torch.full_like(s, float("-inf"))
    s = torch.where(live[:, None, :], s, neg)
    p = torch.softmax(s, -1)
    A = torch.where(live[:, None, :], s.abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
    e = U32 * ((hd + 2) * smag + 6 * A + 3 * (3 + 2 * A) + 2)
    o = (p[..., None] * v).sum(2)                                                     # [B, H, hd]
    pv = (p[..., None] * v.abs()).sum(2)
    err = ((p * e)[..., None] * v.abs()).sum(2) + pv * (p * e).sum(-1, keepdim=True)
    Lf = L.double().view(B, 1, 1)
    unit = U16 * o.abs() + err + (2 * (Lf + 1) + 3) * U32 * pv
    return o.reshape(B, H * hd), unit.reshape(B, H * hd)


def emu_attn_decode(q, kc, vc, lens, scale, fault=None):
    """fp32 evaluation of attn_decode_split_k + attn_decode_combine_k on the CPU: 256-key splits
    of four 64-key waves, p = exp(s - wave max), the waves merged by exp(m_w - M) and the splits
    by exp(M_s - M), one bf16 rounding at the store.  ``fault`` = (name, b, h) plants on one
    (sequence, head): "drop_newest" (the token being decoded not attended), "wave_factor" (wave 1
    merged with wave 0's factor), "norm_last_split" (the normaliser without the last live split)."""
    B, Tmax, H, hd = kc.shape
    L = dec_attended(lens, Tmax)
    Tp = (Tmax + 255) // 256 * 256
    ns = Tp // 256
    live = torch.arange(Tp)[None, None, :] < L.view(B, 1, 1)
    live = live.expand(B, H, Tp).clone()
    if fault and fault[0] == "drop_newest":
        live[fault[1], fault[2], int(L[fault[1]]) - 1] = False
    pad = lambda c: torch.cat([c.float(), torch.zeros(B, Tp - Tmax, H, hd)], 1).permute(0, 2, 1, 3)
    k, v = torch.nan_to_num(pad(kc)), torch.nan_to_num(pad(vc))
    qf = q.float()[:, : H * hd].reshape(B, H, 1, hd) * torch.tensor(scale, dtype=torch.float32)
    s = torch.zeros(B, H, Tp)
    for i in range(hd):
        s += qf[..., i] * k[..., i]
    s = torch.where(live, s, torch.full_like(s, float("-inf"))).view(B, H, ns, 4, 64)
    vw = v.reshape(B, H, ns, 4, 64, hd)
    m = s.max(-1).values                                                              # [B, H, ns, 4]
    fin = torch.isfinite(m)
    p = torch.where(fin[..., None], torch.exp(s - torch.where(fin, m, torch.zeros_like(m))[..., None]), torch.zeros_like(s))
    lsum = p.sum(-1)
    ow = (p[..., None] * vw).sum(-2)                                                  # [B, H, ns, 4, hd]
    Ms = m.max(-1).values                                                             # [B, H, ns]
    sfin = torch.isfinite(Ms)
    f = torch.where(fin, torch.exp(m - torch.where(sfin, Ms, torch.zeros_like(Ms))[..., None]), torch.zeros_like(m))
    if fault and fault[0] == "wave_factor":
        f[fault[1], fault[2], :, 1] = f[fault[1], fault[2], :, 0] * fin[fault[1], fault[2], :, 1]
    acc = (f[..., None] * ow).sum(-2)                                                 # [B, H, ns, hd]
    ls = (f * lsum).sum(-1)
    Mg = Ms.max(-1).values
    f2 = torch.where(sfin, torch.exp(Ms - Mg[..., None]), torch.zeros_like(Ms))
    num = (f2[..., None] * acc).sum(-2)
    f2n = f2.clone()
    if fault and fault[0] == "norm_last_split":
        b, h = fault[1], fault[2]
        f2n[b, h, (int(L[b]) - 1) // 256] = 0
    den = (f2n * ls).sum(-1)
    return (num * (1.0 / den)[..., None]).reshape(B, H * hd).to(torch.bfloat16)


# gemv16_k: (N, K): K-waves with no work; 17 K-steps over 8 waves; per 12 (a partial second load
# batch); the 4-wave form (N > 8192) with per 9; a plain odd N
GEMV_CASES = [(100, 64), (37, 544), (48, 3072), (8208, 1056), (17, 512)]
GEMV_M = (1, 5, 16)
GEMV_SWIGLU_CASES = [(48, 3072), (100, 64)]
GEMV_TILES = {1: (16,)}


def gemv_inputs(M, Nn, K, swiglu=False, device="cpu", seed=51):
    gen = torch.Generator().manual_seed(seed + M + Nn + K)
    x = torch.randn(M, 2 * K if swiglu else K, generator=gen).bfloat16()
    w = (torch.randn(Nn, K, generator=gen) / math.sqrt(K)).bfloat16()
    bias = torch.randn(Nn, generator=gen)
    return x.to(device), w.to(device), bias.to(device)


def ref_gemv(x, w, bias, swiglu=False):
    """(ref, unit) of y = x w^T (+ bias), or with ``swiglu`` of silu(gate) up -> bf16 -> w^T.  The
    fused operand is bf16_round of the fp64 SwiGLU; the kernel's fp32 evaluation (within
    ref_swiglu_fwd's fp32 term) rounds to another bf16 neighbour only where that term reaches the
    rounding boundary: there the operand may be off by one bf16 ulp, which goes through |w|."""
    K = w.size(1)
    if not swiglu:
        ref, mag = ref_gemm(x, w, "nt", bias)
        return ref, unit_gemm_bf16(ref, mag, K)
    h, _, acc = ref_swiglu_fwd(x)
    hr = bf16_round(h)
    ulp = bf16_ulp(h)
    flips = (ulp / 2 - (h - hr).abs()) <= acc
    ref, mag = ref_gemm(hr, w, "nt", bias)
    return ref, unit_gemm_bf16(ref, mag, K) + torch.where(flips, ulp, torch.zeros_like(ulp)) @ d(w).abs().t()
