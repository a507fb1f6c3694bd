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


def assert_within(out, ref64, unit, limit, what, tiles=None):
    """max(err / unit) <= limit over every element (unit == 0 demands err == 0).  ``tiles`` maps a
    dimension to the kernel's tile sizes along it, e.g. {0: (256, 128, 16), 1: (256, 192)}: the
    failure message gives the worst element's index modulo each, so an edge fault names itself.
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
        + (f" [{mods}]" if mods else "") + f"; {n_over} of {ratio.numel()} elements over the limit")


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


def ref_swiglu_fwd(gu, perm=False):
    """(h, unit, fp32 term): h = silu(gate) up; unit = one bf16 rounding + the fp32 evaluation's
    terms."""
    g, u = gu_unperm64(gu, perm)
    h = g * torch.sigmoid(g) * u
    acc = (_exp_terms(g) + 3) * U32 * h.abs()
    return h, U16 * h.abs() + acc, acc


def ref_swiglu_bwd(dh64, gu, perm=False, dh_unit=None):
    """(dgu natural layout, unit, fp32 term, column sums, their unit).  ``dh_unit``: an error
    bound of dh64's elements (the fused epilogue's dh is a bf16-rounded GEMM result), propagated
    through the derivative."""
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
    unit = U16 * ref.abs() + acc
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


def ref_bias_residual(y, bias, res):
    """(x, unit, fp32 term) of x = y + bias + res, fp32 adds, one rounding to bf16."""
    y, res = d(y), d(res)
    ref, mag = y + res, y.abs() + res.abs()
    if bias is not None:
        ref, mag = ref + d(bias), mag + d(bias).abs()
    acc = 2 * U32 * mag
    return ref, U16 * ref.abs() + acc, acc


def ref_add_rmsnorm_fwd(y, bias, res, w, eps, x_kernel=None):
    """The fused residual add + RMSNorm: x = y + bias + res rounded once to bf16, then the norm
    of that ROUNDED x.  Returns (x, unit_x, h, unit_h, rstd, unit_rstd); h / rstd are taken from
    ``x_kernel`` (the kernel's own x output) when given, else from the correctly rounded x."""
    x, ux, _ = ref_bias_residual(y, bias, res)
    xin = x_kernel if x_kernel is not None else x.to(torch.bfloat16)
    h, uh, r, ur = ref_rmsnorm_fwd(xin, w, eps)
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
