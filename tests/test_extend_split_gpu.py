"""The split form of the extend attention (csrc/kernels/attn_extend.hip: attn_extend_k<SPLIT> +
attn_extend_combine_k) on MI355X, through ``_attn_extend_split`` / ``_attn_extend_split_paged``.

The cases, oracle and limit are those of tests/test_extend_bounds_gpu.py (tests/numerics_extend.py): a
split adds only fp32 merge roundings (2^-24 each) to the bf16 roundings the unit is made of, so the
limit is not raised.  At the 1..17 key tiles of ``EXT_CASES``, 2 / 3 / 7 splits give split counts that
do not divide the tiles, splits of fewer than four tiles (idle waves), splits past the last tile
(empty), the diagonal tile in the last split, an empty row and rows that are not live.

Worst err / unit on an MI355X over EXT_CASES x families, the same at 2, 3 and 7 splits (limit): hd 32
0.7399 (1.48), hd 64 0.7615 (1.523), hd 128 0.8863 (1.773): the emulation's own figures, i.e. the worst
element is a bf16 rounding of the output that the splits do not move (profiles/kernel_error_bounds.txt).
"""
import os

import pytest
import torch

import numerics as N
import numerics_extend as X
import numerics_kv8 as Q

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402
from distributed_pytorch_from_scratch_amd.ops import reference as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
B, H = N.DEC_B, N.DEC_H
_REFS = {}


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _case(hd, case, fam):
    """The poisoned inputs (NaN in q rows that are not live and in cache rows nobody attends) and the
    fp64 reference of one case, computed once for every split count."""
    key = (hd, X.case_id(case), fam)
    if key not in _REFS:
        Tmax, _, T, _ = case
        lens, ns = X.case_rows(case)
        live = X.live_counts(lens, ns, T, Tmax)
        qkv, kc, vc = X.ext_inputs(hd, case, fam, DEV)
        ref, unit = X.ref_attn_extend(qkv, kc, vc, lens, ns, T, hd ** -0.5)
        for b, (L, m) in enumerate(zip(lens, live)):
            qkv[b * T + m: (b + 1) * T, : H * hd] = NAN
            kc[b, max(L, 0) + m:] = NAN
            vc[b, max(L, 0) + m:] = NAN
        _REFS[key] = (qkv[:, : H * hd], kc, vc, lens, ns, live, ref, unit)
    return _REFS[key]


@pytest.mark.parametrize("splits", [2, 3, 7])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_split_bounds(C, hd, splits):
    worst = 0.0
    for case in X.EXT_CASES:
        T = case[2]
        for fam in N.DEC_FAMILIES:
            q, kc, vc, lens, ns, live, ref, unit = _case(hd, case, fam)
            what = f"_attn_extend_split hd {hd} splits {splits} {fam} {X.case_id(case)}"
            uniform = not isinstance(case[1], list)
            o = C._attn_extend_split(q, kc, vc, None, None, _i32([case[1]]) if uniform else _i32(lens),
                                     None if case[3] is None else _i32(ns), hd ** -0.5, splits)
            assert o.shape == (B * T, H * hd) and o.dtype == torch.bfloat16
            assert bool(torch.isfinite(o.float()).all()), what + ": NaN from a padded row or an unattended cache row"
            worst = max(worst, N.assert_within(o, ref, unit, X.ext_limit(hd), what, {0: (32,), 1: (hd, 32)}))
            for b in range(B):
                assert not bool((o[b * T + live[b]: (b + 1) * T] != 0).any()), what + f": rows of sequence {b} not live"
    print(f"_attn_extend_split hd {hd} splits {splits}: worst err / unit {worst:.4g}, limit {X.ext_limit(hd):.4g}")


@pytest.mark.parametrize("splits", [2, 5])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_split_selects_the_key_exactly(C, hd, splits):
    """One key of {0, 31, 32, 63, 64, 255, 256, own} carries all of a query's probability: the output is
    that value row bit for bit, so a dropped split, tile or wave, or a wrong partial slot, shows."""
    for length, T, shift in [(257, 20, 0), (257, 20, 6), (40, 31, 0), (0, 9, 0)]:
        qkv, kc, vc, tstar, ln = X.ext_selection_inputs(hd, 300, length, T, shift, DEV)
        want = torch.stack([vc[b, int(tstar[b, t, h]), h] for b in range(B) for t in range(T) for h in range(H)])
        o = C._attn_extend_split(qkv[:, : H * hd], kc, vc, None, None, ln, None, hd ** -0.5, splits)
        assert torch.equal(o, want.view(B * T, H * hd)), (hd, splits, length, T, shift)


def _paged(cache, page, perm):
    """(pool (P, page, ...), tbl (B, MP)) holding ``cache`` (B, Tmax % page == 0, ...) on permuted pages."""
    MP = cache.size(1) // page
    pool = torch.empty((B * MP, page) + tuple(cache.shape[2:]), dtype=cache.dtype, device=DEV)
    pool.view(torch.uint8)[perm] = cache.reshape(pool.shape).view(torch.uint8)
    return pool, perm.view(B, MP).to(torch.int32)


@pytest.mark.parametrize("hd", N.DEC_HD)
def test_split_identities(C, hd):
    """No tolerance: splits = 1 is _attn_extend; two runs at 3 splits agree; the fp8 form is the bf16 split
    form on caches dequantised by the kv8.h expression; the paged forms (page 16: two pages per key
    tile) are the contiguous split forms on the same content."""
    Tmax, T, page, scale = 528, 257, 16, hd ** -0.5
    qkv, kc, vc = X.ext_inputs(hd, (Tmax, 255, T, None), "randn", DEV)
    q, ln, n = qkv[:, : H * hd], _i32([255, 100]), _i32([T, 40])
    assert torch.equal(C._attn_extend_split(q, kc, vc, None, None, ln, n, scale, 1), C._attn_extend(q, kc, vc, ln, n, scale))
    a = C._attn_extend_split(q, kc, vc, None, None, ln, n, scale, 3)
    assert torch.equal(a, C._attn_extend_split(q, kc, vc, None, None, ln, n, scale, 3))
    (k8, ks), (v8, vs) = R._kv_quant_rows(kc), R._kv_quant_rows(vc)
    a8 = C._attn_extend_split(q, k8, v8, ks, vs, ln, n, scale, 3)
    assert torch.equal(a8, C._attn_extend_split(q, Q.dequant_bf16(k8, ks), Q.dequant_bf16(v8, vs), None, None, ln, n, scale, 3))
    perm = torch.randperm(B * Tmax // page, generator=torch.Generator().manual_seed(hd)).to(DEV)
    (kp, tbl), (vp, _) = _paged(kc, page, perm), _paged(vc, page, perm)
    assert torch.equal(a, C._attn_extend_split_paged(q, kp, vp, None, None, tbl, ln, n, Tmax, page, scale, 3))
    pools8 = [_paged(c, page, perm)[0] for c in (k8, v8, ks, vs)]
    assert torch.equal(a8, C._attn_extend_split_paged(q, *pools8, tbl, ln, n, Tmax, page, scale, 3))


def test_model_continuation_on_the_split_kernel(C, monkeypatch):
    """gpt2-small (2 layers): a 30-token continuation of a 70-token cache through logits_step with
    DPFS_EXTEND_SPLIT=3 against =0, at the tolerance tests/test_chunked_prefill_gpu.py holds a
    continuation to; the split binding is the one that ran."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29591")
    from distributed_pytorch_from_scratch_amd.models import Transformer, get_preset
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.utils.dist import destroy_dist_env, init_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    try:
        m = Transformer.from_args(get_preset("gpt2-small", num_layers=2)).cuda()
        m.reset_parameters()
        m.eval()
        ids = torch.randint(0, m.args.vocab_size, (2, 100), generator=torch.Generator().manual_seed(5)).cuda()
        attn = m.layers[0].attn
        calls, real = [], C._attn_extend_split
        monkeypatch.setattr(C, "_attn_extend_split", lambda *a: calls.append(a[-1]) or real(*a))
        out = {}
        for env in ("0", "3"):
            monkeypatch.setenv("DPFS_EXTEND_SPLIT", env)
            cache = G.KVCache(2, 2, 128, attn.num_local_heads, attn.head_dim, torch.bfloat16, torch.device("cuda"))
            G.logits_step(m, ids[:, :70].contiguous(), cache)
            seen = len(calls)
            out[env] = G.logits_step(m, ids[:, 70:].contiguous(), cache).float()
            assert calls[seen:] == ([3, 3] if env == "3" else []), (env, calls)
        rel = ((out["3"] - out["0"]).norm() / out["0"].norm()).item()
        print("split 3 vs unsplit, relative:", rel)
        assert rel < 3e-2, rel
    finally:
        G.clear_sessions()
        destroy_dist_env()
