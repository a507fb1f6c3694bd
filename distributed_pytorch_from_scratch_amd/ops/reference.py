"""Pure-PyTorch reference kernels: the CPU compute path and the numerical oracle.

Every function here has the *same signature and semantics* as the HIP kernel of the same
name in ``csrc/kernels`` (exported by ``_C``).  Tests compare the two; on CPU the model runs
on these.  Math is done in fp32 and results are cast to the input dtype, matching the GPU
kernels' accumulate-in-fp32 policy.

Reference parity notes (``/root/reference``):

* ``rmsnorm_fwd``: ``models/layers.py:145-155`` (``scale * (x * rsqrt(mean(x^2)+eps))``).
* ``rope_``: ``models/model.py:17-46`` (HF rotate-half; cos/sin tables with duplicated
  halves, angles ``pos * theta`` in fp32).
* ``attention``: ``models/model.py:73-77`` (causal, softmax(QK^T/sqrt(hd)) V).
* ``swiglu``: ``models/model.py:94-95``.
* ``embedding_fwd``: ``models/layers.py:134-141`` without the in-place mutation of the ids.
* ``vocab-parallel CE``: extension; the reference all-gathers logits and calls
  ``F.cross_entropy(ignore_index=-1)`` (``train.py:101-104``).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------- GEMM ----

def gemm_nt(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, rope_pos=None, rope_tab=None,
            rope_heads: int = 0, rope_hd: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """c[M,N] = a[M,K] @ b[N,K]^T (+ bias[N]); output dtype = a.dtype.  With ``rope_pos`` the first
    ``rope_heads`` heads of each row are then rotated (the GPU kernel fuses this into its
    epilogue)."""
    c = a.float() @ b.float().t()
    if bias is not None:
        c = c + bias.float()
    c = c.to(a.dtype)
    if rope_pos is not None and rope_heads > 0:
        rope_(c, rope_pos, rope_tab, rope_heads, rope_hd, False)
    return out.copy_(c) if out is not None else c


def gemm_nn(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """c[M,N] = a[M,K] @ b[K,N]; output dtype = a.dtype (written into ``out`` when given)."""
    c = (a.float() @ b.float()).to(a.dtype)
    return out.copy_(c) if out is not None else c


def gemm_tn(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None,
            accumulate: bool = False) -> torch.Tensor:
    """c[M,N] (fp32) = a[K,M]^T @ b[K,N]  (+= into ``out`` if ``accumulate``)."""
    c = a.float().t() @ b.float()
    if out is None:
        return c
    if accumulate:
        out.add_(c)
    else:
        out.copy_(c)
    return out


def gemm_tn2(a0: torch.Tensor, b0: torch.Tensor, a1: torch.Tensor, b1: torch.Tensor,
             out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """c[M,N] (fp32) = a0^T b0 + a1^T b1: a TN GEMM whose reduction dim is split over two
    buffers (+= into ``out`` if ``accumulate``)."""
    c = gemm_tn(a0, b0, out, accumulate)
    return gemm_tn(a1, b1, c, True)


def add_bias_(y: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """y[M,N] += bias[N] in place (fp32 add, rounded to y.dtype); returns y."""
    y.copy_((y.float() + bias.float()).to(y.dtype))
    return y


def bias_residual(y: torch.Tensor, bias: Optional[torch.Tensor], residual: torch.Tensor) -> torch.Tensor:
    """out = residual + y (+ bias), fp32 math, rounded once to y.dtype."""
    out = y.float() + residual.float()
    if bias is not None:
        out = out + bias.float()
    return out.to(y.dtype)


def bias_grad(dy: torch.Tensor) -> torch.Tensor:
    """fp32 column sums of dy[M,N]."""
    return dy.float().sum(0)


# -------------------------------------------------------------------------- norms ----

def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
    y = (xf * rstd[:, None]).to(x.dtype).float() * w.float()
    return y.to(x.dtype), rstd


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, rstd: torch.Tensor,
                dres: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None,
                dw_out: Optional[torch.Tensor] = None):
    """Returns (dx [+ dres if given, fused residual-grad add], dw fp32); with ``dbias`` (fp32
    [D]) also writes the column sums of dx there (the bias grad of the layer below); with
    ``dw_out`` (fp32 [D]) dw is written there and returned."""
    xf, dyf, wf = x.float(), dy.float(), w.float()
    xhat = xf * rstd[:, None]
    dw = (dyf * xhat).sum(0)
    g = dyf * wf
    d = xf.size(-1)
    dx = rstd[:, None] * (g - xhat * (g * xhat).sum(-1, keepdim=True) / d)
    if dres is not None:
        dx = dx + dres.float()
    if dbias is not None:
        dbias.copy_(dx.sum(0))
    if dw_out is not None:
        dw = dw_out.copy_(dw)
    return dx.to(x.dtype), dw


def add_rmsnorm_fwd(y: torch.Tensor, bias: Optional[torch.Tensor], res: torch.Tensor, w: torch.Tensor,
                    eps: float):
    """(x = y + bias + res rounded to y.dtype, rmsnorm_fwd(x)) — the fused residual epilogue."""
    x = bias_residual(y, bias, res)
    h, rstd = rmsnorm_fwd(x, w, eps)
    return x, h, rstd


def layernorm_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float):
    xf = x.float()
    mean = xf.mean(-1)
    var = (xf - mean[:, None]).pow(2).mean(-1)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean[:, None]) * rstd[:, None] * w.float() + b.float()
    return y.to(x.dtype), mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd):
    xf, dyf, wf = x.float(), dy.float(), w.float()
    xhat = (xf - mean[:, None]) * rstd[:, None]
    dw = (dyf * xhat).sum(0)
    db = dyf.sum(0)
    g = dyf * wf
    d = xf.size(-1)
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).sum(-1, keepdim=True) / d)
    return dx.to(x.dtype), dw, db


# --------------------------------------------------------------------------- RoPE ----

def rope_table(maxlen: int, head_dim: int, theta: float, device=None) -> torch.Tensor:
    """fp32 ``(maxlen, head_dim)`` table: columns [cos(pos*inv_freq) | sin(pos*inv_freq)] for
    the ``head_dim/2`` frequencies (the reference duplicates each half; we store it once).
    ``inv_freq`` is computed on CPU in fp32 exactly as ``models/model.py:38``."""
    assert head_dim % 2 == 0
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    pos = torch.arange(maxlen).float().unsqueeze(1)
    ang = pos * inv
    tab = torch.cat([torch.cos(ang), torch.sin(ang)], dim=1)
    return tab.to(device) if device is not None else tab


def rope_(qkv: torch.Tensor, positions: torch.Tensor, table: torch.Tensor, n_rot_heads: int,
          head_dim: int, inverse: bool = False) -> torch.Tensor:
    """Rotate (in place) the first ``n_rot_heads`` heads of each row of ``qkv[M, *]``.

    ``positions[M]`` indexes ``table``.  ``inverse`` applies the transpose rotation (the RoPE
    backward).  Rotate-half convention: out1 = x1 c - x2 s, out2 = x2 c + x1 s.
    """
    M = qkv.size(0)
    h2 = head_dim // 2
    tab = table[positions.long()]  # (M, hd)
    c = tab[:, None, :h2]
    s = tab[:, None, h2:]
    if inverse:
        s = -s
    view = qkv[:, : n_rot_heads * head_dim].view(M, n_rot_heads, head_dim)
    x1 = view[..., :h2].float()
    x2 = view[..., h2:].float()
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    view[..., :h2] = o1.to(qkv.dtype)
    view[..., h2:] = o2.to(qkv.dtype)
    return qkv


# ---------------------------------------------------------------------- attention ----

def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
             causal: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """q,k,v: (B, T, H, hd) (any strides). Returns o (B, T, H, hd) contiguous and the
    natural-log LSE (B, H, T) fp32 of the scaled scores."""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))  # B H T hd
    s = (qf @ kf.transpose(-1, -2)) * scale
    if causal:
        T, S = s.shape[-2], s.shape[-1]
        mask = torch.ones(T, S, dtype=torch.bool, device=s.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = (p @ vf).transpose(1, 2).contiguous()
    return o.to(q.dtype), lse


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, len: torch.Tensor,
                scale: float) -> torch.Tensor:
    """One query row per (sequence, head) against cache rows [0, len]: q [B, >= H*hd] rows,
    caches (B, T_max, H, hd), len a 1-element int tensor, or one of B elements (sequence b
    attends rows [0, min(len[b] + 1, T_max))).  Returns o [B, H*hd] in q.dtype."""
    B, Tmax, H, hd = k_cache.shape
    if len.numel() != 1:
        assert len.numel() == B, "len must have 1 or B elements"
        return torch.cat([attn_decode(q[b:b + 1], k_cache[b:b + 1], v_cache[b:b + 1],
                                      len.reshape(-1)[b:b + 1].clamp(max=Tmax - 1), scale) for b in range(B)])
    L = int(len.reshape(-1)[0]) + 1
    qf = q[:, : H * hd].float().view(B, H, 1, hd)
    kf = k_cache[:, :L].float().transpose(1, 2)          # B H L hd
    vf = v_cache[:, :L].float().transpose(1, 2)
    p = torch.softmax((qf @ kf.transpose(-1, -2)) * scale, dim=-1)
    return (p @ vf).reshape(B, H * hd).to(q.dtype)


def kv_append(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, len: torch.Tensor) -> None:
    """cache[:, len] = the k / v parts of the packed qkv rows [B, 3*H*hd]; with a B-element
    len, cache[b, len[b]], and a full row (len[b] >= T_max) appends nothing."""
    B, Tmax, H, hd = k_cache.shape
    if len.numel() != 1:
        assert len.numel() == B, "len must have 1 or B elements"
        for b, t in enumerate(len.reshape(-1).tolist()):
            if 0 <= t < Tmax:
                kv_append(qkv[b:b + 1], k_cache[b:b + 1], v_cache[b:b + 1], len.reshape(-1)[b:b + 1])
        return
    t = int(len.reshape(-1)[0])
    k_cache[:, t] = qkv[:, H * hd: 2 * H * hd].view(B, H, hd).to(k_cache.dtype)
    v_cache[:, t] = qkv[:, 2 * H * hd: 3 * H * hd].view(B, H, hd).to(v_cache.dtype)


def _chunk_rows(len: torch.Tensor, n: Optional[torch.Tensor], B: int, T: int, Tmax: int):
    """Per sequence (cache length before the chunk, live new tokens): token t of row b is live
    iff t < n[b] (``n`` None: T) and len[b] + t < T_max."""
    assert len.numel() in (1, B), "len must have 1 or B elements"
    assert n is None or n.numel() == B, "n must have B elements"
    lens = len.reshape(-1).expand(B).tolist()
    ns = [T] * B if n is None else n.reshape(-1).tolist()
    return [(L, 0 if L < 0 else max(0, min(m, T, Tmax - L))) for L, m in zip(lens, ns)]


def _kv_append_chunk(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, len: torch.Tensor,
                     n: Optional[torch.Tensor] = None) -> None:
    """The multi-row kv_append: the k / v parts of packed row b*T + t of qkv [B*T, 3*H*hd] go to
    cache row len[b] + t, for t < n[b] (``n`` None: T) and len[b] + t < T_max; every other cache
    element is left as it is."""
    B, Tmax, H, hd = k_cache.shape
    T = qkv.size(0) // B
    rows = qkv.view(B, T, -1)
    for b, (L, m) in enumerate(_chunk_rows(len, n, B, T, Tmax)):
        if m > 0:
            k_cache[b, L:L + m] = rows[b, :m, H * hd: 2 * H * hd].view(m, H, hd).to(k_cache.dtype)
            v_cache[b, L:L + m] = rows[b, :m, 2 * H * hd: 3 * H * hd].view(m, H, hd).to(v_cache.dtype)


def _attn_extend(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, len: torch.Tensor,
                 n: Optional[torch.Tensor], scale: float) -> torch.Tensor:
    """A chunk of T new queries per sequence against the cache (which already holds the chunk's
    keys and values, ``_kv_append_chunk``): q [B*T, >= H*hd] rows, row b*T + t = new token t of
    sequence b; it attends cache rows [0, len[b] + t].  A token with t >= n[b] (``n`` None: T)
    or len[b] + t >= T_max reads nothing and gives zeros.  fp32 math, any cache dtype.  Returns
    o [B*T, H*hd] in q.dtype."""
    B, Tmax, H, hd = k_cache.shape
    T = q.size(0) // B
    qf = q[:, : H * hd].float().view(B, T, H, hd)
    o = torch.zeros(B, T, H, hd, dtype=torch.float32, device=q.device)
    for b, (L, m) in enumerate(_chunk_rows(len, n, B, T, Tmax)):
        if m == 0:
            continue
        S = L + m
        keys = k_cache[b, :S].float()                        # (S, H, hd)
        vals = v_cache[b, :S].float()
        s = torch.einsum("thd,shd->hts", qf[b, :m], keys) * scale
        mask = torch.ones(m, S, dtype=torch.bool, device=s.device).triu(L + 1)
        p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
        o[b, :m] = torch.einsum("hts,shd->thd", p, vals)
    return o.view(B * T, H * hd).to(q.dtype)


# ------------------------------------------------------------------- fp8 KV cache ----
# Storage: e4m3 codes k8 / v8 (B, T_max, H, hd) torch.float8_e4m3fn and one fp32 scale per cached
# (token, head) row, ks / vs (B, T_max, H).  The format is the contract of the GPU kernels
# (csrc/kernels/kv8.h), which produce the same codes and scales bit for bit.

def _kv_quant_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows ``x[..., hd]`` -> (codes ``[..., hd]`` float8_e4m3fn, inv ``[...]`` fp32):
    amax = max(max_j |x_j|, 1e-12), scale = 448 / amax, code_j = e4m3fn(clamp(x_j * scale, +-448))
    (fp32 product, round to nearest even), inv = 1 / scale; the row represents f32(code_j) * inv.
    fp32 arithmetic, operation for operation that of ``ops/fp8.py`` per row."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True).clamp_min(1e-12)
    # tensor / tensor: IEEE fp32 divisions (a Python scalar over a tensor multiplies by the reciprocal)
    scale = torch.full_like(amax, 448.0) / amax
    codes = (xf * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return codes, (torch.ones_like(scale) / scale).squeeze(-1)


def _kv_dequant(c8: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    return c8.float() * cs[..., None]


def _kv_append_chunk_q8(qkv: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
                        len: torch.Tensor, n: Optional[torch.Tensor] = None) -> None:
    """The quantising ``_kv_append_chunk``: the k / v parts of packed row b*T + t of qkv
    [B*T, 3*H*hd] go, as codes and a scale per head, to cache row len[b] + t, for t < n[b] (``n``
    None: T) and len[b] + t < T_max; every other code and scale is left as it is."""
    B, Tmax, H, hd = k8.shape
    T = qkv.size(0) // B
    rows = qkv.view(B, T, -1)
    for b, (L, m) in enumerate(_chunk_rows(len, n, B, T, Tmax)):
        if m > 0:
            k8[b, L:L + m], ks[b, L:L + m] = _kv_quant_rows(rows[b, :m, H * hd: 2 * H * hd].view(m, H, hd))
            v8[b, L:L + m], vs[b, L:L + m] = _kv_quant_rows(rows[b, :m, 2 * H * hd: 3 * H * hd].view(m, H, hd))


def _rope_append_q8(qkv: torch.Tensor, pos: torch.Tensor, table: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor,
                    ks: torch.Tensor, vs: torch.Tensor, len: torch.Tensor) -> None:
    """rope_ on the q and k heads of the packed rows [B, 3*H*hd], then the quantising append of the
    rotated k row and the v row at len / len[b] (a full cache or row appends nothing)."""
    H, hd = k8.size(2), k8.size(3)
    rope_(qkv, pos, table, 2 * H, hd, False)
    _kv_append_chunk_q8(qkv, k8, v8, ks, vs, len)


def _attn_decode_q8(q: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
                    len: torch.Tensor, scale: float) -> torch.Tensor:
    """``attn_decode`` over the dequantised caches ``code.float() * inv[..., None]``.  Rows past
    the attended keys are not read (they may hold NaN codes and scales)."""
    B, Tmax, H, hd = k8.shape
    L = min(int(len.max()) + 1, Tmax)
    kf = torch.zeros(B, Tmax, H, hd, dtype=torch.float32, device=k8.device)
    vf = torch.zeros_like(kf)
    kf[:, :L], vf[:, :L] = _kv_dequant(k8[:, :L], ks[:, :L]), _kv_dequant(v8[:, :L], vs[:, :L])
    return attn_decode(q, kf, vf, len, scale)


def _attn_extend_q8(q: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
                    len: torch.Tensor, n: Optional[torch.Tensor], scale: float) -> torch.Tensor:
    """``_attn_extend`` over the dequantised caches ``code.float() * inv[..., None]``."""
    return _attn_extend(q, _kv_dequant(k8, ks), _kv_dequant(v8, vs), len, n, scale)


# ----------------------------------------------------------------- paged KV cache ----
# Storage (csrc/kernels/kv_page.h is the contract): per layer and side one pool (P, page, H, hd),
# bf16 / fp32, or float8_e4m3fn with fp32 scale pools ks / vs (P, page, H); one block table tbl
# int32 (B, MP), MP = ceil(t_max / page); key t of sequence b lives in pool row
# tbl[b, t // page] * page + t % page, an entry that maps nothing is -1.  Always per-row: len [B].
# An append through an entry outside [0, P) is dropped; a read through one takes page 0.

def _paged_view(pool: torch.Tensor, tbl: torch.Tensor, t_max: int) -> torch.Tensor:
    """The contiguous (B, t_max, ...) cache a pool (P, page, ...) holds through ``tbl`` (a copy)."""
    P, page = pool.size(0), pool.size(1)
    e = tbl.long()
    e = torch.where((e >= 0) & (e < P), e, torch.zeros_like(e))
    raw = pool.view(torch.uint8) if pool.dtype == torch.float8_e4m3fn else pool
    g = raw[e]                                               # (B, MP, page, ...)
    return g.reshape(e.size(0), e.size(1) * page, *pool.shape[2:])[:, :t_max].contiguous().view(pool.dtype)


def _paged_put(pool: torch.Tensor, tbl: torch.Tensor, b: int, t0: int, rows: torch.Tensor) -> None:
    """``rows`` (m, ...) become keys [t0, t0 + m) of sequence b: scattered through the table, rows
    whose entry maps no page of the pool dropped."""
    P, page = pool.size(0), pool.size(1)
    t = torch.arange(t0, t0 + rows.size(0), device=pool.device)
    e = tbl[b, t // page].long()
    ok = (e >= 0) & (e < P)
    dst = (e * page + t % page)[ok]
    fp8 = pool.dtype == torch.float8_e4m3fn
    flat = (pool.view(torch.uint8) if fp8 else pool).view(P * page, *pool.shape[2:])
    src = rows.to(pool.dtype)
    flat[dst] = (src.view(torch.uint8) if fp8 else src)[ok]


def _kv_append_chunk_paged(qkv: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                           ks: Optional[torch.Tensor], vs: Optional[torch.Tensor], tbl: torch.Tensor,
                           len: torch.Tensor, n: Optional[torch.Tensor], t_max: int, page: int) -> None:
    """``_kv_append_chunk`` (``ks`` / ``vs`` None) or ``_kv_append_chunk_q8`` into pools: what the
    contiguous op writes at cache row len[b] + t goes to the pool row the table gives that key."""
    P, PS, H, hd = k_pool.shape
    assert PS == page and tbl.size(1) == -(-t_max // page), "pool / table do not fit (t_max, page)"
    B = tbl.size(0)
    assert len.numel() == B, "a paged cache is per-row: len must have B elements"
    T = qkv.size(0) // B
    rows = qkv.view(B, T, -1)
    for b, (L, m) in enumerate(_chunk_rows(len, n, B, T, t_max)):
        if m == 0:
            continue
        kx = rows[b, :m, H * hd: 2 * H * hd].view(m, H, hd)
        vx = rows[b, :m, 2 * H * hd: 3 * H * hd].view(m, H, hd)
        if ks is None:
            _paged_put(k_pool, tbl, b, L, kx)
            _paged_put(v_pool, tbl, b, L, vx)
        else:
            for x, pool, sc in ((kx, k_pool, ks), (vx, v_pool, vs)):
                codes, inv = _kv_quant_rows(x)
                _paged_put(pool, tbl, b, L, codes)
                _paged_put(sc, tbl, b, L, inv)


def _rope_append_paged(qkv: torch.Tensor, pos: torch.Tensor, table: torch.Tensor, k_pool: torch.Tensor,
                       v_pool: torch.Tensor, ks: Optional[torch.Tensor], vs: Optional[torch.Tensor],
                       tbl: torch.Tensor, len: torch.Tensor, t_max: int, page: int) -> None:
    """rope_ on the q and k heads of the packed rows [B, 3*H*hd], then the (quantising) append of
    the rotated k row and the v row at key len[b] of the pools (a full row appends nothing)."""
    H, hd = k_pool.size(2), k_pool.size(3)
    rope_(qkv, pos, table, 2 * H, hd, False)
    _kv_append_chunk_paged(qkv, k_pool, v_pool, ks, vs, tbl, len, None, t_max, page)


def _attn_decode_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, ks: Optional[torch.Tensor],
                       vs: Optional[torch.Tensor], tbl: torch.Tensor, len: torch.Tensor, t_max: int, page: int,
                       scale: float) -> torch.Tensor:
    """``attn_decode`` (per-row) / ``_attn_decode_q8`` on the contiguous view of the pools."""
    assert k_pool.size(1) == page and len.numel() == tbl.size(0)
    kc, vc = _paged_view(k_pool, tbl, t_max), _paged_view(v_pool, tbl, t_max)
    if ks is None:
        return attn_decode(q, kc, vc, len, scale)
    return _attn_decode_q8(q, kc, vc, _paged_view(ks, tbl, t_max), _paged_view(vs, tbl, t_max), len, scale)


def _attn_extend_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, ks: Optional[torch.Tensor],
                       vs: Optional[torch.Tensor], tbl: torch.Tensor, len: torch.Tensor, n: Optional[torch.Tensor],
                       t_max: int, page: int, scale: float) -> torch.Tensor:
    """``_attn_extend`` / ``_attn_extend_q8`` on the contiguous view of the pools."""
    assert k_pool.size(1) == page and len.numel() == tbl.size(0)
    kc, vc = _paged_view(k_pool, tbl, t_max), _paged_view(v_pool, tbl, t_max)
    if ks is None:
        return _attn_extend(q, kc, vc, len, n, scale)
    return _attn_extend_q8(q, kc, vc, _paged_view(ks, tbl, t_max), _paged_view(vs, tbl, t_max), len, n, scale)


def gemv_nt_ok(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False) -> bool:
    return True


def gemv_nt(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
            swiglu: bool = False) -> torch.Tensor:
    """y = a w^T (+ bias) in x.dtype, a = x, or with ``swiglu`` a = silu(g) * u of the packed
    x = [g | u] rounded to x.dtype (the GPU kernel's fused operand; swiglu_fwd's rounding)."""
    if swiglu:
        K = w.size(1)
        g, u = x[:, :K].float(), x[:, K:].float()
        a = (g / (1.0 + torch.exp(-g)) * u).to(x.dtype)
    else:
        a = x
    y = a.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)


def rope_append(qkv: torch.Tensor, pos: torch.Tensor, table: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, len: torch.Tensor) -> None:
    """rope_ on the q and k heads of the packed rows, then kv_append (one GPU kernel)."""
    H, hd = k_cache.size(2), k_cache.size(3)
    rope_(qkv, pos, table, 2 * H, hd, False)
    kv_append(qkv, k_cache, v_cache, len)


def step_advance(len: torch.Tensor, pos: torch.Tensor) -> None:
    """End of a decode step, one length for the batch: len += 1, pos[:] = len."""
    assert len.numel() == 1, "per-row lengths: _step_advance_rows(len, pos, t_max)"
    len += 1
    pos.fill_(int(len.reshape(-1)[0]))


def _step_advance_rows(len: torch.Tensor, pos: torch.Tensor, t_max: int) -> None:
    """End of a decode step with one length per sequence: len[b] = min(len[b] + 1, t_max),
    pos[b] = min(len[b], t_max - 1), so a row that fills its cache (capacity ``t_max``) is frozen
    there.  (The leading underscore follows the native module, whose recorded public surface
    keeps the two-argument ``step_advance``.)"""
    assert len.numel() == pos.numel(), "len must have one element per pos entry"
    len.copy_((len + 1).clamp(max=t_max))
    pos.copy_(len.reshape(pos.shape).clamp(max=t_max - 1))


# ----------------------------------------------------------------------- sampling ----

_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123) on Python integers: ``counter`` 4 and ``key`` 2
    32-bit words -> 4 output words.  Counter 0 with key 0 gives word 0 = 0x6627E8D5."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def sample_uniform(seed: int, pos: int, row: int) -> float:
    """The sampling uniform of (seed, position, row): key (seed lo32, seed hi32), counter
    (pos lo32, pos hi32, row, 0), u = (x0 >> 8) * 2^-24 in [0, 1) (exact in fp32)."""
    s, p = int(seed) & 0xFFFFFFFFFFFFFFFF, int(pos) & 0xFFFFFFFFFFFFFFFF
    x0 = philox4x32_10((p & _M32, p >> 32, row, 0), (s & _M32, s >> 32))[0]
    return (x0 >> 8) * 2.0 ** -24


def sample_logits(logits: torch.Tensor, vocab: int, temperature: float, top_k: int, top_p: float, seed: int,
                  pos: torch.Tensor, u: Optional[torch.Tensor] = None):
    """Temperature / top-k / top-p sampling of one token per row of ``logits`` (B, >= vocab);
    columns >= vocab are padding.  z = fp32(logit) * fp32(1/T) (one fp32 multiply), weights
    exp(z - max z) and every mass in fp64.  Top-k keeps ``logit >= v_k`` (the k-th largest;
    ties all kept; 0 or >= vocab: off); top-p then keeps, of the survivors, ``logit >= t*`` with
    t* the largest value present whose upper set holds a share >= p of the survivors' mass
    (ties kept whole; 1: off).  The token is the smallest kept index j whose inclusive kept
    mass C_j (vocabulary order) exceeds u * C_last, u = ``sample_uniform(seed, pos[b], b)``
    unless ``u`` (B,) supplies it.  Returns (ids int64, kept int32, thresh fp32 -- the final
    cutoff as a raw logit, the row minimum with both filters off --, u fp32), each (B,)."""
    assert temperature > 0 and 0 < top_p <= 1 and top_k >= 0 and 1 <= vocab <= logits.size(1)
    dev = logits.device
    if u is None:
        u = torch.tensor([sample_uniform(seed, p, b) for b, p in enumerate(pos.tolist())], dtype=torch.float32,
                         device=dev)
    inv_t = torch.tensor(1.0 / temperature, dtype=torch.float32, device=dev)
    return _sample_with(logits, vocab, inv_t, top_k, top_p, u)


def _sample_with(logits: torch.Tensor, vocab: int, inv_t: torch.Tensor, top_k: int, top_p: float, u: torch.Tensor):
    """``sample_logits`` from the fp32 scale ``inv_t`` = fp32(1 / temperature) (0-d) and the
    uniforms ``u`` (B,): what the scalar and the per-row oracle share."""
    B, dev = logits.size(0), logits.device
    x = logits[:, :vocab].float()
    z = (x * inv_t).double()
    w = torch.exp(z - z.max(-1, keepdim=True).values)
    thresh = x.min(-1).values
    if 0 < top_k < vocab:
        thresh = x.topk(top_k, dim=-1).values[:, -1]
    keep = x >= thresh[:, None]
    if top_p < 1:
        xs, order = x.sort(dim=-1, descending=True, stable=True)
        ks = keep.gather(-1, order)
        cum = (w.gather(-1, order) * ks).cumsum(-1)
        total = cum[:, -1:]
        # S(value) = the cumulative mass at the end of the value's run of ties
        last = torch.ones_like(ks)
        last[:, :-1] = xs[:, :-1] != xs[:, 1:]
        run_end = torch.where(last, cum, torch.full_like(cum, float("inf"))).flip(-1).cummin(-1).values.flip(-1)
        ok = ks & (run_end >= top_p * total)
        first = ok.to(torch.int8).argmax(-1, keepdim=True)      # descending order: the largest value
        thresh = xs.gather(-1, first)[:, 0]
        keep = keep & (x >= thresh[:, None])
    u = u.to(device=dev, dtype=torch.float32)
    wk = w * keep
    C = wk.cumsum(-1)
    hit = keep & (C > u.double()[:, None] * C[:, -1:])
    ids = hit.to(torch.int8).argmax(-1)
    # rounding left no C_j above u * M: the last kept index with a non-zero weight
    idx = torch.arange(vocab, device=dev).expand(B, vocab)
    fallback = torch.where(wk > 0, idx, torch.zeros_like(idx)).max(-1).values
    ids = torch.where(hit.any(-1), ids, fallback)
    return ids, keep.sum(-1).to(torch.int32), thresh, u


def sample_logits_rows(logits: torch.Tensor, vocab: int, inv_t: torch.Tensor, top_k: torch.Tensor,
                       top_p: torch.Tensor, seed: torch.Tensor, rid: torch.Tensor, pos: torch.Tensor,
                       u: Optional[torch.Tensor] = None):
    """``sample_logits`` with the settings of every row as data, (B,) each: ``inv_t`` fp32 =
    fp32(1 / temperature), 0 marks a greedy row; ``top_k`` int32, <= 0 or >= vocab is off;
    ``top_p`` fp64, >= 1 is off; ``seed`` int64; ``rid`` int32, the row word of the Philox counter
    (what the scalar form fills with b).  A sampled row b is ``sample_logits`` of
    ``logits[b:b+1]`` with that row's scalars and u = ``sample_uniform(seed[b], pos[b], rid[b])``
    unless ``u`` (B,) supplies it.  A greedy row gives the first maximum of its valid columns
    (``argmax``), kept = the number of maxima, thresh = the maximum and u = 0.  Returns
    (ids int64, kept int32, thresh fp32, u fp32), each (B,)."""
    B, dev = logits.size(0), logits.device
    assert 1 <= vocab <= logits.size(1)
    for t, dt in ((inv_t, torch.float32), (top_k, torch.int32), (top_p, torch.float64), (seed, torch.int64),
                  (rid, torch.int32)):
        assert t.dtype == dt and t.shape == (B,), "one setting per row, in the dtype of its array"
    ids = torch.empty(B, dtype=torch.int64, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    thresh = torch.empty(B, dtype=torch.float32, device=dev)
    uo = torch.empty(B, dtype=torch.float32, device=dev)
    rows = zip(inv_t.tolist(), top_k.tolist(), top_p.tolist(), seed.tolist(), rid.tolist(), pos.tolist())
    for b, (it, k, p, s, r, ps) in enumerate(rows):
        if it == 0.0:
            x = logits[b, :vocab].float()
            out = x.argmax(), (x == x.max()).sum(), x.max(), 0.0
        else:
            ub = torch.tensor([sample_uniform(s, ps, r)], dtype=torch.float32) if u is None else u[b:b + 1]
            out = (t[0] for t in _sample_with(logits[b:b + 1], vocab, inv_t[b], k if 0 < k < vocab else 0,
                                              min(p, 1.0), ub))
        ids[b], kept[b], thresh[b], uo[b] = out
    return ids, kept, thresh, uo


# the name the kernel sets share (the native module binds the per-row form with a leading
# underscore: its recorded public surface is left as it is)
_sample_logits_rows = sample_logits_rows


def penalised_logits(logits: torch.Tensor, vocab: int, rep: torch.Tensor, inv_rep: torch.Tensor, pres: torch.Tensor,
                     freq: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """The fp32 (B, vocab) row ``sample_logits_pen`` samples from.  ``hist`` int32 (B, >= vocab):
    bit 31 of a word says that the id occurs in the row's prompt, bits 0..30 are c, the number of
    times it has been drawn; seen = word != 0.  In the vLLM order (repetition over prompt and
    output, presence and frequency over the output only), every step one rounded fp32 operation:

        x = fp32(logit);  seen: x = x * inv_rep if x > 0 else x * rep;  x = x - freq * fp32(c);
        c > 0: x = x - pres."""
    x = logits[:, :vocab].float()
    h = hist[:, :vocab]
    c = h & 0x7FFFFFFF
    col = lambda t: t.to(torch.float32)[:, None]
    x = torch.where(h != 0, torch.where(x > 0, x * col(inv_rep), x * col(rep)), x)
    x = x - col(freq) * c.to(torch.float32)
    return torch.where(c > 0, x - col(pres), x)


def sample_logprobs_fp64(logits: torch.Tensor, vocab: int, x: torch.Tensor, inv_t: torch.Tensor,
                         thresh: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """The two log-probabilities of ``sample_logits_pen`` before their rounding to fp32, fp64
    (B, 2): of ids[b] under softmax(raw logits), and under the distribution drawn from, the
    weights exp(z - max z), z = fp32(x * inv_t), of the kept columns {x >= thresh} of the
    penalised row ``x`` (a greedy row: z = 0, every maximum weighs 1)."""
    at = ids[:, None]
    lp_model = torch.log_softmax(logits[:, :vocab].double(), -1).gather(-1, at)[:, 0]
    z = (x * inv_t[:, None]).double()
    z = z - z.max(-1, keepdim=True).values
    mass = (torch.exp(z) * (x >= thresh[:, None])).sum(-1)
    return torch.stack([lp_model, z.gather(-1, at)[:, 0] - torch.log(mass)], -1)


def sample_logits_pen(logits: torch.Tensor, vocab: int, inv_t: torch.Tensor, top_k: torch.Tensor,
                      top_p: torch.Tensor, seed: torch.Tensor, rid: torch.Tensor, rep: torch.Tensor,
                      inv_rep: torch.Tensor, pres: torch.Tensor, freq: torch.Tensor, hist: torch.Tensor,
                      pos: torch.Tensor, u: Optional[torch.Tensor] = None, update: bool = True):
    """``sample_logits_rows`` on ``penalised_logits`` (x in place of the logit everywhere: z =
    x * inv_t, top-k / top-p / ties, the greedy first maximum; ``kept`` and ``thresh`` in units of
    x), with the penalties ``rep`` / ``inv_rep`` = fp32(1 / rep, the quotient in fp64) / ``pres`` /
    ``freq`` fp32 (B,) and the history ``hist`` int32 (B, >= vocab) as data.  Returns (ids, kept,
    thresh, u, logp, hist): ``logp`` fp32 (B, 2), computed in fp64, holds the log-probability of
    ids[b] under the model's own distribution (softmax of the raw logits: temperature 1, no
    penalty, no filter) and under the distribution the draw used (log of the id's share of the
    kept, penalised, tempered mass; -log(number of maxima) on a greedy row).  With ``update``
    hist[b, ids[b]] += 1, in place as the kernel does it; the table is returned either way."""
    B = logits.size(0)
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.size(0) == B and hist.size(1) >= vocab
    for t in (rep, inv_rep, pres, freq):
        assert t.dtype == torch.float32 and t.shape == (B,), "one fp32 penalty per row"
    x = penalised_logits(logits, vocab, rep, inv_rep, pres, freq, hist)
    ids, kept, thresh, uo = sample_logits_rows(x, vocab, inv_t, top_k, top_p, seed, rid, pos, u)
    logp = sample_logprobs_fp64(logits, vocab, x, inv_t, thresh, ids).float()
    if update:
        hist[torch.arange(B, device=hist.device), ids] += 1
    return ids, kept, thresh, uo, logp, hist


_sample_logits_pen = sample_logits_pen


def _rot_bthd(x: torch.Tensor, positions: torch.Tensor, table: torch.Tensor, inverse: bool) -> torch.Tensor:
    """Rotate-half RoPE of an fp32 (B, T, H, hd) tensor; ``positions`` is flat [B*T]."""
    B, T, H, hd = x.shape
    h2 = hd // 2
    tab = table[positions.long()].view(B, T, 1, hd)
    c, s = tab[..., :h2], tab[..., h2:]
    if inverse:
        s = -s
    x1, x2 = x[..., :h2], x[..., h2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def attn_bwd(do, q, k, v, o, lse, scale: float, causal: bool, dq_out, dk_out, dv_out, rope_pos=None,
             rope_tab=None, dbias=None):
    """Writes dq/dk/dv into the given (B, T, H, hd) views (packed dqkv buffer).  With
    ``rope_pos`` the inverse RoPE is applied to dq and dk (fused into the stores on the GPU).
    With ``dbias`` (fp32 [3 * H * hd]) also the packed QKV bias gradient: the column sums of
    dq | dk | dv over all tokens.  Returns whether ``dbias`` was written."""
    qf, kf, vf, dof, of = (t.float().transpose(1, 2) for t in (q, k, v, do, o))
    s = (qf @ kf.transpose(-1, -2)) * scale
    if causal:
        T, S = s.shape[-2], s.shape[-1]
        mask = torch.ones(T, S, dtype=torch.bool, device=s.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.exp(s - lse[..., None])
    dv = p.transpose(-1, -2) @ dof
    dp = dof @ vf.transpose(-1, -2)
    delta = (dof * of).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = ds @ kf
    dk = ds.transpose(-1, -2) @ qf
    dq, dk = dq.transpose(1, 2), dk.transpose(1, 2)
    if rope_pos is not None:
        dq = _rot_bthd(dq, rope_pos, rope_tab, True)
        dk = _rot_bthd(dk, rope_pos, rope_tab, True)
    dq_out.copy_(dq)
    dk_out.copy_(dk)
    dv_out.copy_(dv.transpose(1, 2))
    if dbias is None:
        return False
    dbias.copy_(torch.cat([t.float().sum((0, 1)).reshape(-1) for t in (dq, dk, dv.transpose(1, 2))]))
    return True


# ------------------------------------------------------------------------- SwiGLU ----

def gu_perm(x: torch.Tensor, dim: int = 0) -> torch.Tensor:
    """Interleave a packed [gate | up] dimension (size 2F, F % 64 == 0) in 64-blocks: positions
    [128 b, 128 b + 64) = gate [64 b, 64 b + 64), the next 64 = up [64 b, 64 b + 64).  The fused
    gate|up GEMM epilogue (csrc/kernels/gemm4.hip SwiOut) then holds each gate / up pair in one
    lane.  ``gu_unperm`` is the inverse."""
    n = x.size(dim)
    sh = list(x.shape)
    v = x.reshape(sh[:dim] + [2, n // 128, 64] + sh[dim + 1:])
    return v.transpose(dim, dim + 1).reshape(sh)


def gu_unperm(x: torch.Tensor, dim: int = 0) -> torch.Tensor:
    n = x.size(dim)
    sh = list(x.shape)
    v = x.reshape(sh[:dim] + [n // 128, 2, 64] + sh[dim + 1:])
    return v.transpose(dim, dim + 1).reshape(sh)


def _gate_up(gu: torch.Tensor, perm: bool):
    if perm:
        gu = gu_unperm(gu, gu.dim() - 1)
    F_ = gu.size(-1) // 2
    return gu[..., :F_].float(), gu[..., F_:].float()


def swiglu_fwd(gu: torch.Tensor, perm: bool = False) -> torch.Tensor:
    """h = silu(gate) * up of a packed gate|up tensor (``perm``: interleaved, see gu_perm)."""
    g, u = _gate_up(gu, perm)
    return (F.silu(g) * u).to(gu.dtype)


def gemm_nt_swiglu(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """Gate|up projection with the SwiGLU of the fused GPU epilogue: b / bias in the natural
    [gate | up] layout, multiplied with the rows interleaved by gu_perm -> [gu (interleaved,
    a.dtype), h = silu(gate) * up (a.dtype)]."""
    gu = gemm_nt(a, gu_perm(b), gu_perm(bias) if bias is not None else None)
    return [gu, swiglu_fwd(gu, True)]


def swiglu_bwd(dh: torch.Tensor, gu: torch.Tensor, dbias: Optional[torch.Tensor] = None,
               perm: bool = False) -> torch.Tensor:
    """d gate|up in the natural [gate | up] layout (``perm``: gu is read interleaved); with
    ``dbias`` (fp32 [2F]) also writes the bias gradient (column sums)."""
    g, u = _gate_up(gu, perm)
    dhf = dh.float()
    sig = torch.sigmoid(g)
    silu = g * sig
    dg = dhf * u * sig * (1 + g * (1 - sig))
    du = dhf * silu
    d = torch.cat([dg, du], dim=-1)
    if dbias is not None:
        dbias.copy_(d.sum(0))
    return d.to(gu.dtype)


def gemm_nn_swiglu_bwd(dy: torch.Tensor, w: torch.Tensor, gu: torch.Tensor, dbias: Optional[torch.Tensor] = None,
                       perm: bool = True):
    """The down projection's data gradient fused with the SwiGLU backward (the GPU kernel's
    epilogue form): ds = dy w rounded to dy.dtype, then swiglu_bwd(ds, gu, dbias, perm).
    Returns [dgu]."""
    return [swiglu_bwd(gemm_nn(dy, w), gu, dbias, perm)]


# ---------------------------------------------------------------------- embedding ----

def embedding_fwd(ids: torch.Tensor, weight: torch.Tensor, vocab_start: int,
                  out_dtype: torch.dtype) -> torch.Tensor:
    """Rows of the local vocab shard for ids in [vocab_start, vocab_start+V_local), zeros
    elsewhere.  Does not mutate ``ids`` (the reference does, ``layers.py:138``)."""
    vl = weight.size(0)
    local = ids.long() - vocab_start
    m = (local >= 0) & (local < vl)
    out = weight[local.clamp(0, vl - 1)].float() * m[:, None].float()
    return out.to(out_dtype)


def embedding_bwd(dout: torch.Tensor, ids: torch.Tensor, v_local: int, vocab_start: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 dW[v_local, D] of the masked embedding (rows ADDED to ``out`` when given)."""
    local = ids.long() - vocab_start
    m = (local >= 0) & (local < v_local)
    dw = out if out is not None else torch.zeros(v_local, dout.size(-1), dtype=torch.float32, device=dout.device)
    dw.index_add_(0, local[m], dout[m].float())
    return dw


def embedding_bwd_sorted(dout: torch.Tensor, ids: torch.Tensor, v_local: int, vocab_start: int,
                         out: Optional[torch.Tensor] = None, accumulate: bool = False, perm=None,
                         seg=None) -> torch.Tensor:
    """``embedding_bwd`` that WRITES every row of ``out`` (``accumulate``: adds, as the later
    chunks of the engines), summing each vocab row's gradient rows in row order.  (``perm`` /
    ``seg``: the native kernel's precomputed sort, see ``emb_sort_ahead``; unused here.)"""
    if out is None:
        out = torch.zeros(v_local, dout.size(-1), dtype=torch.float32, device=dout.device)
    elif not accumulate:
        out.zero_()
    return embedding_bwd(dout, ids, v_local, vocab_start, out)


def emb_sort(ids: torch.Tensor, vocab_start: int, v_local: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(perm, seg): the ids' stable order by local vocab row with the ids outside the shard last,
    and each local row's segment start (seg[v_local] = number of in-shard ids)."""
    local = ids.reshape(-1).long() - vocab_start
    key = torch.where((local >= 0) & (local < v_local), local, torch.full_like(local, 0xFFFF))
    sk, perm = torch.sort(key, stable=True)
    seg = torch.searchsorted(sk, torch.arange(v_local + 1, device=ids.device))
    return perm, seg


def emb_sort_ahead(ids: torch.Tensor, vocab_start: int, v_local: int):
    """The embedding backward's sort (see ops.dispatch.emb_sort_ahead); nothing to do here."""
    return None


# ------------------------------------------------------------ vocab-parallel CE ----

def ce_fwd_stats(logits: torch.Tensor, targets: torch.Tensor, vocab_start: int,
                 vocab_valid: int) -> torch.Tensor:
    """Per-row local statistics of one vocab shard: (M, 3) fp32 = [max, sum(exp(x-max)),
    target_logit (0 if the target is not in this shard)].  Columns ``>= vocab_valid`` (the
    padded vocab tail inside this shard) are excluded."""
    x = logits.float()
    if vocab_valid < x.size(1):
        x = x[:, :vocab_valid]
    mx = x.max(dim=1).values
    se = torch.exp(x - mx[:, None]).sum(1)
    local = targets.long() - vocab_start
    hit = (local >= 0) & (local < x.size(1))
    tl = torch.where(hit, x.gather(1, local.clamp(0, max(x.size(1) - 1, 0))[:, None]).squeeze(1),
                     torch.zeros_like(mx))
    return torch.stack([mx, se, tl], dim=1)


def ce_combine(stats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """stats: (n_shards, M, 3) gathered from every TP rank -> (lse[M], target_logit[M])."""
    mx = stats[..., 0].max(0).values
    se = (stats[..., 1] * torch.exp(stats[..., 0] - mx[None])).sum(0)
    lse = mx + torch.log(se)
    tl = stats[..., 2].sum(0)
    return lse, tl


def ce_finalize(stats: torch.Tensor, targets: torch.Tensor, ignore_index: int, acc: torch.Tensor,
                loss: torch.Tensor, first: bool, last: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Loss bookkeeping from the gathered (n_shards, M, 3) statistics: returns (lse[M], valid[M]
    as 1.0 / 0.0); ``acc[0:2]`` holds the running (sum over valid rows of lse - target logit,
    valid count), overwritten when ``first``; with ``last`` the count is clamped to >= 1 and
    ``loss`` (0-d) gets the mean."""
    lse, tl = ce_combine(stats)
    valid = (targets != ignore_index).float()
    part = torch.stack([torch.where(valid > 0, lse - tl, torch.zeros_like(lse)).sum(), valid.sum()])
    if first:
        acc[:2] = part
    else:
        acc[:2] += part
    if last:
        acc[1] = acc[1].clamp_min(1.0)
        loss.copy_(acc[0] / acc[1])
    return lse, valid


def ce_valid_scale(targets: torch.Tensor, ignore_index: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(gs[M], n_valid): 1 / max(#valid, 1) on the valid rows, 0 on the ignored ones."""
    valid = (targets != ignore_index).float()
    n = valid.sum().clamp_min(1.0)
    return valid / n, n


def ce_grad_scale(valid: torch.Tensor, gloss: torch.Tensor, n_valid: torch.Tensor) -> torch.Tensor:
    """Per-row gradient scale of the CE backward: valid * gloss / n_valid."""
    return valid * (gloss.float().reshape(()) / n_valid.reshape(()))


def ce_bwd(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, gscale: torch.Tensor,
           vocab_start: int, vocab_valid: int, out: torch.Tensor,
           dbias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d logits = (softmax - onehot) * gscale[row] (gscale = 0 on ignored rows); padded
    columns get 0.  Written to ``out`` (may alias ``logits``: the GPU kernel runs in place)."""
    x = logits.float()
    p = torch.exp(x - lse[:, None])
    local = targets.long() - vocab_start
    hit = (local >= 0) & (local < vocab_valid)
    p[hit, local[hit]] -= 1.0
    p = p * gscale[:, None]
    if vocab_valid < x.size(1):
        p[:, vocab_valid:] = 0
    if dbias is not None:
        dbias.copy_(p.sum(0))
    out.copy_(p)
    return out


def ce_fused(logits: torch.Tensor, targets: torch.Tensor, gscale: torch.Tensor, vocab_start: int,
             vocab_valid: int, dbias: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Single-shard CE forward and backward in one pass (TP 1: the shard is the whole vocab, so
    the row's lse is local): returns the :func:`ce_fwd_stats` rows and overwrites ``logits``
    with :func:`ce_bwd`'s (softmax - onehot) * gscale[row] (+ the column sums into ``dbias``)."""
    stats = ce_fwd_stats(logits, targets, vocab_start, vocab_valid)
    lse = stats[:, 0] + torch.log(stats[:, 1])
    ce_bwd(logits, targets, lse, gscale, vocab_start, vocab_valid, logits, dbias)
    return stats


# -------------------------------------------------------------------------- Adam ----

def adam_step(params, grads, exp_avgs, exp_avg_sqs, shadows, lr: float, beta1: float,
              beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0):
    """In-place Adam (torch.optim.Adam semantics, L2 ``weight_decay`` added to the gradient
    as in ``torch.optim.Adam``); also refreshes optional low-precision shadow copies."""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    for i, p in enumerate(params):
        g = grads[i].float() * grad_scale
        if weight_decay != 0:
            g = g + weight_decay * p
        m, v = exp_avgs[i], exp_avg_sqs[i]
        m.mul_(beta1).add_(g, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / bc1)
        if shadows is not None and shadows[i] is not None:
            shadows[i].copy_(p)
