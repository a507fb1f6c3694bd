"""The paged KV cache kernels (csrc/kernels/kv_page.h; the PAGED forms in decode.hip,
attn_extend.hip and kv8.hip) against the contiguous kernels on the same logical cache content.

The paged launches take their splits and tiles over the logical key index and only address the
cache differently, so every comparison here is exact: outputs bit for bit, appended caches byte for
byte.  A paged cache is built by scattering a contiguous one into a pool through a permuted,
row-interleaved table; pool rows nobody owns hold NaN (bf16) or 0x7f codes with NaN scales (fp8),
so a read through a wrong page shows.  Every pool is the middle of a larger allocation with one
guard page in front and one behind: an index of -1 or P used unchecked lands in memory the test owns.
"""
import os
import random

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402
from distributed_pytorch_from_scratch_amd.ops import reference as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F8 = torch.float8_e4m3fn
B, H = N.DEC_B, N.DEC_H
PAGES = (16, 64, 256)
SENT = 0x55                      # byte sentinel of unwritten fp8 codes


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _bits(x):
    return x.view(torch.uint8) if x.dtype == F8 else x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _table(t_max, page, seed, spare=2):
    """(tbl int32 (B, MP) on the device, P): a permutation of the P = B * MP + spare pages, dealt to
    the rows in turn, so physical pages are non-contiguous and interleaved between the rows."""
    MP = -(-t_max // page)
    P = B * MP + spare
    perm = list(range(P))
    random.Random(seed).shuffle(perm)
    return _i32([perm[b::B][:MP] for b in range(B)]), P


def _guarded(P, page, tail, dtype, fill):
    """(whole, pool): ``pool`` (P, page, *tail) is pages 1 .. P of ``whole`` (P + 2 pages), all ``fill``."""
    if dtype == F8:
        whole = torch.full((P + 2, page) + tail, fill, dtype=torch.uint8, device=DEV).view(F8)
    else:
        whole = torch.full((P + 2, page) + tail, fill, dtype=dtype, device=DEV)
    pool = whole[1:P + 1]
    assert pool.is_contiguous() and pool.data_ptr() % 16 == 0
    return whole, pool


def _blank(x):
    """The fill of pool rows nobody owns, by what the pool holds: NaN, or for codes the NaN code 0x7f."""
    return 0x7F if x.dtype == F8 else NAN


def _scatter(cache, tbl, page, P, fill=None):
    """(whole, pool) holding ``cache`` (B, T, ...) through ``tbl``; every other pool row is ``fill``."""
    whole, pool = _guarded(P, page, tuple(cache.shape[2:]), cache.dtype, _blank(cache) if fill is None else fill)
    T = cache.size(1)
    t = torch.arange(T, device=DEV)
    flat = _bits(pool).view(P * page, *_bits(pool).shape[2:])
    for b in range(cache.size(0)):
        rows = tbl[b, t // page].long() * page + t % page
        flat[rows] = _bits(cache)[b]
    return whole, pool


def _gather(pool, tbl, t_max):
    return R._paged_view(pool, tbl, t_max)


def _owned_rows(tbl, page, P, t_max, lens=None):
    """bool (P * page,): the pool rows some (b, t < t_max [t < lens[b]]) maps to."""
    own = torch.zeros(P * page, dtype=torch.bool, device=DEV)
    for b in range(tbl.size(0)):
        t = torch.arange(t_max if lens is None else min(lens[b], t_max), device=DEV)
        e = tbl[b, t // page].long()
        ok = (e >= 0) & (e < P)
        own[(e * page + t % page)[ok]] = True
    return own


def _caches(t_max, hd, fp8, seed):
    """Contiguous caches of random rows: (kc, vc) bf16, or (k8, v8, ks, vs)."""
    g = torch.Generator().manual_seed(seed)
    kc = torch.randn(B, t_max, H, hd, generator=g).bfloat16().to(DEV)
    vc = torch.randn(B, t_max, H, hd, generator=g).bfloat16().to(DEV)
    if not fp8:
        return [kc, vc]
    (k8, ks), (v8, vs) = R._kv_quant_rows(kc), R._kv_quant_rows(vc)
    return [k8, v8, ks, vs]


def _pools(caches, tbl, page, P):
    """The paged operands (k_pool, v_pool, ks | None, vs | None) of contiguous ``caches``, and the wholes."""
    pairs = [_scatter(c, tbl, page, P) for c in caches]
    pools = [p for _, p in pairs] + [None] * (4 - len(pairs))
    return pools, [w for w, _ in pairs]


# ------------------------------------------------------------------------ 1. decode ----
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("t_max", N.DEC_TMAX)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_decode_paged_is_bit_identical(C, hd, t_max, page, fp8):
    """T_max 16 / 300 / 512: one split, two splits with a partial last page, exact.  Both rows walk
    the lengths {0, PS - 1, PS, PS + 1, 255, 256, 257, T_max - 1, T_max} clipped to T_max."""
    caches = _caches(t_max, hd, fp8, 100 + hd + t_max)
    tbl, P = _table(t_max, page, seed=page + t_max)
    pools, _ = _pools(caches, tbl, page, P)
    g = torch.Generator().manual_seed(hd)
    q = torch.randn(B, 3 * H * hd, generator=g).bfloat16().to(DEV)
    scale = hd ** -0.5
    Ls = sorted({min(v, t_max) for v in (0, page - 1, page, page + 1, 255, 256, 257, t_max - 1, t_max)})
    for i, a in enumerate(Ls):
        lens = _i32([a, Ls[(i + 3) % len(Ls)]])
        want = C._attn_decode_q8(q, *caches, lens, scale) if fp8 else C.attn_decode(q, *caches, lens, scale)
        got = C._attn_decode_paged(q, *pools, tbl, lens, t_max, page, scale)
        assert torch.equal(_bits(got), _bits(want)), (lens.tolist(), (got.float() - want.float()).abs().max().item())
        assert not torch.isnan(got.float()).any()


# ------------------------------------------------------------------------ 2. extend ----
EXT_TMAX = 160


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("length,T", [(1, 33), (95, 40), (127, 33), (150, 20)])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_extend_paged_is_bit_identical(C, hd, length, T, page, fp8):
    """The (len, T) cases of tests/test_kv_fp8_gpu.py at T_max 160 (the last runs past the capacity),
    with per-row len and n and a row with n = 0."""
    caches = _caches(EXT_TMAX, hd, fp8, 200 + hd + length)
    tbl, P = _table(EXT_TMAX, page, seed=page + length)
    pools, _ = _pools(caches, tbl, page, P)
    g = torch.Generator().manual_seed(hd + T)
    q = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16().to(DEV)
    scale = hd ** -0.5
    for lens, n in (([length, length // 2], [T, 0]), ([length // 3, length], [T - 3, T]), ([length, length], None)):
        lens, n = _i32(lens), (None if n is None else _i32(n))
        want = C._attn_extend_q8(q, *caches, lens, n, scale) if fp8 else C._attn_extend(q, *caches, lens, n, scale)
        got = C._attn_extend_paged(q, *pools, tbl, lens, n, EXT_TMAX, page, scale)
        assert torch.equal(_bits(got), _bits(want)), (lens.tolist(), (got.float() - want.float()).abs().max().item())
        assert not torch.isnan(got.float()).any()
    out = C._attn_extend_paged(q, *pools, tbl, _i32([length, 5]), _i32([T, 0]), EXT_TMAX, page, scale)
    assert not out.view(B, T, -1)[1].any()                  # a row with n = 0 gives zeros


# ----------------------------------------------------------------------- 3. appends ----
def _sentinel_caches(t_max, hd, fp8):
    if fp8:
        k8 = torch.full((B, t_max, H, hd), SENT, dtype=torch.uint8, device=DEV).view(F8)
        ks = torch.full((B, t_max, H), NAN, device=DEV)
        return [k8, k8.clone(), ks, ks.clone()]
    kc = torch.full((B, t_max, H, hd), NAN, dtype=torch.bfloat16, device=DEV)
    return [kc, kc.clone()]


def _sentinel_pools(caches, tbl, page, P):
    """Sentinel pools in guarded allocations: fill = the contiguous caches' own sentinel."""
    fills = [SENT if c.dtype == F8 else NAN for c in caches]
    pairs = [_guarded(P, page, tuple(c.shape[2:]), c.dtype, f) for c, f in zip(caches, fills)]
    return [p for _, p in pairs] + [None] * (4 - len(pairs)), [w for w, _ in pairs], fills


def _is_fill(x, fill):
    return (_bits(x) == SENT).all() if x.dtype == F8 else torch.isnan(x.float()).all()


def _check_appended(pools, wholes, fills, caches, tbl, page, P, t_max):
    for pool, whole, fill, cache in zip(pools, wholes, fills, caches):
        assert torch.equal(_bits(_gather(pool, tbl, t_max)), _bits(cache))        # exactly the contiguous cache
        own = _owned_rows(tbl, page, P, t_max)
        flat = pool.view(P * page, *pool.shape[2:])
        assert _is_fill(flat[~own], fill)                                         # rows nobody maps: untouched
        assert _is_fill(whole[0], fill) and _is_fill(whole[P + 1], fill)          # the guards


APP_SHAPES = [(16, 40), (64, 136), (256, 520)]          # (page, T_max): three pages, the last one partial


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page,t_max", APP_SHAPES)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_kv_append_chunk_paged_exact(C, hd, page, t_max, fp8):
    """Chunks of 5 rows on both sides of a page boundary, a full row, and per-row n with n = 0."""
    T = 5
    g = torch.Generator().manual_seed(hd + page)
    tbl, P = _table(t_max, page, seed=hd + page)
    caches = _sentinel_caches(t_max, hd, fp8)
    pools, wholes, fills = _sentinel_pools(caches, tbl, page, P)
    cases = [([page - 2, t_max], None), ([page, 2 * page - 5], None), ([2 * page - 1, 0], [3, 5]),
             ([t_max - 2, page - 5], [5, 0])]
    for lens, n in cases:
        qkv = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16().to(DEV)
        lens, n = _i32(lens), (None if n is None else _i32(n))
        (C._kv_append_chunk_q8 if fp8 else C._kv_append_chunk)(qkv, *caches, lens, n)
        C._kv_append_chunk_paged(qkv, *pools, tbl, lens, n, t_max, page)
        _check_appended(pools, wholes, fills, caches, tbl, page, P, t_max)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page,t_max", APP_SHAPES)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_rope_append_paged_exact(C, hd, page, t_max, fp8):
    """The fused decode-step append: the same rotated qkv rows, the same cache bytes; lengths on both
    sides of a page boundary, 0, the last row and a full row."""
    g = torch.Generator().manual_seed(hd + page + 1)
    tbl, P = _table(t_max, page, seed=hd + page + 1)
    caches = _sentinel_caches(t_max, hd, fp8)
    pools, wholes, fills = _sentinel_pools(caches, tbl, page, P)
    tab = R.rope_table(t_max, hd, 10000.0, device=DEV)
    for lens in ([page - 1, page], [t_max, 2 * page], [0, t_max - 1], [2 * page - 1, t_max]):
        qkv = torch.randn(B, 3 * H * hd, generator=g).bfloat16().to(DEV)
        qa, qb = qkv.clone(), qkv.clone()
        lens_t = _i32(lens)
        pos = lens_t.clamp(max=t_max - 1).long()
        (C._rope_append_q8 if fp8 else C.rope_append)(qa, pos, tab, *caches, lens_t)
        C._rope_append_paged(qb, pos, tab, *pools, tbl, lens_t, t_max, page)
        assert torch.equal(_bits(qa), _bits(qb))
        _check_appended(pools, wholes, fills, caches, tbl, page, P, t_max)


# ------------------------------------------------------------------ 4. table safety ----
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_bad_table_entries_stay_inside_the_pools(C, hd, page, fp8):
    """Row 0's table has -1 and P inside its live range.  Appends leave the guards and every page
    the table does not name untouched, row 1's pages and attention outputs are those of the clean
    run bit for bit, and nothing is asserted about row 0's values."""
    t_max = 3 * page + 8
    T = 5
    tbl, P = _table(t_max, page, seed=hd + page + 2)
    bad = tbl.clone()
    bad[0, 0], bad[0, 2] = -1, P
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(hd + page + 2)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16().to(DEV)
    q1 = torch.randn(B, 3 * H * hd, generator=g).bfloat16().to(DEV)
    tab = R.rope_table(t_max, hd, 10000.0, device=DEV)
    # appends through the bad table: a chunk over the bad page 0 / a good page 1, a chunk into the
    # bad page 2, and a decode-step append into each
    shape = _sentinel_caches(t_max, hd, fp8)
    clean, _, _ = _sentinel_pools(shape, tbl, page, P)
    pools, wholes, fills = _sentinel_pools(shape, tbl, page, P)
    for lens in ([page - 2, page - 2], [2 * page - 2, 2 * page - 2]):
        for t, ps in ((tbl, clean), (bad, pools)):
            C._kv_append_chunk_paged(qkv, *ps, t, _i32(lens), None, t_max, page)
    for lens in ([3, 3], [2 * page + 3, 2 * page + 3]):
        pos = _i32(lens).long()
        for t, ps in ((tbl, clean), (bad, pools)):
            C._rope_append_paged(q1.clone(), pos, tab, *ps, t, _i32(lens), t_max, page)
    torch.cuda.synchronize()
    named = torch.zeros(P, dtype=torch.bool, device=DEV)
    named[bad.flatten()[(bad.flatten() >= 0) & (bad.flatten() < P)].long()] = True
    for pool, whole, fill, ref in zip(pools, wholes, fills, clean):
        assert _is_fill(whole[0], fill) and _is_fill(whole[P + 1], fill)
        assert _is_fill(pool[~named], fill)                   # row 0's dropped rows went nowhere
        assert _is_fill(pool[int(tbl[0, 0])], fill) and _is_fill(pool[int(tbl[0, 2])], fill)
        for e in tbl[1].tolist() + [int(tbl[0, 1])]:
            assert torch.equal(_bits(pool[e]), _bits(ref[e]))
    # attention through the bad table: row 1 is the clean run's, no access leaves the pools
    caches = _caches(t_max, hd, fp8, 300 + hd)
    pools, wholes = _pools(caches, tbl, page, P)
    before = [w.clone() for w in wholes]
    lens = _i32([t_max - 1, 2 * page + 1])
    want = C._attn_decode_paged(q1, *pools, tbl, lens, t_max, page, scale)
    got = C._attn_decode_paged(q1, *pools, bad, lens, t_max, page, scale)
    assert torch.equal(_bits(got[1]), _bits(want[1]))
    lens = _i32([2 * page + 1, page + 3])
    want = C._attn_extend_paged(qkv, *pools, tbl, lens, None, t_max, page, scale)
    got = C._attn_extend_paged(qkv, *pools, bad, lens, None, t_max, page, scale)
    assert torch.equal(_bits(got.view(B, T, -1)[1]), _bits(want.view(B, T, -1)[1]))
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(w), _bits(b_)) for w, b_ in zip(wholes, before))


def test_paged_bindings_check_their_arguments(C):
    hd, page, t_max = 64, 16, 40
    caches = _caches(t_max, hd, False, 1)
    tbl, P = _table(t_max, page, seed=1)
    pools, _ = _pools(caches, tbl, page, P)
    q = torch.zeros(B, 3 * H * hd, dtype=torch.bfloat16, device=DEV)
    lens = _i32([1, 2])
    ok = lambda **kw: C._attn_decode_paged(**{**dict(q=q, k_pool=pools[0], v_pool=pools[1], ks=None, vs=None, tbl=tbl,
                                                     len=lens, t_max=t_max, page=page, scale=0.125), **kw})
    ok()
    for kw, msg in ((dict(page=32), "page"), (dict(page=24), "power of two"), (dict(tbl=tbl[:, :2].contiguous()), "tbl"),
                    (dict(tbl=tbl.long()), "tbl"), (dict(tbl=tbl.t().contiguous().t()), "tbl"),
                    (dict(len=_i32([1])), "len"), (dict(k_pool=pools[0].float()), "pools"),
                    (dict(k_pool=pools[0].transpose(0, 1)), "pools"), (dict(ks=torch.zeros(P, page, H, device=DEV)), "ks"),
                    (dict(t_max=page * 3 + 1), "tbl")):
        with pytest.raises(RuntimeError, match=msg):
            ok(**kw)


# ----------------------------------------------------------------------- 5. model ----
@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29579")
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    yield
    destroy_dist_env()


@pytest.fixture(scope="module")
def model(dist1):
    """gpt2-small with 2 layers, as tests/test_kv_fp8_gpu.py builds it."""
    from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m = Transformer.from_args(get_preset("gpt2-small", num_layers=2)).cuda()
    m.reset_parameters()
    m.eval()
    yield m
    G.clear_sessions()


LENS, LENS2, NEW = [100, 37, 1], [9, 100, 64], 40        # t_max 140: 9 pages of 16, 3 of 64
CONFIGS = {"ragged": {}, "chunked": dict(prefill_chunk=32),
           "sampled": dict(temperature=0.8, top_k=50, top_p=0.9, seed=3)}


@pytest.fixture(scope="module")
def prompt(model):
    g = torch.Generator().manual_seed(31)
    return torch.randint(0, model.args.vocab_size, (3, 100), generator=g).cuda()


@pytest.fixture(scope="module")
def contiguous_tokens(model, prompt):
    """The contiguous per-row generate() of every (cache dtype, configuration), computed once."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    out = {}
    for kd in (None, "fp8"):
        for name, kw in CONFIGS.items():
            out[kd, name] = G.generate(model, prompt, max_new_tokens=NEW, prompt_lens=LENS, kv_dtype=kd, **kw)
        out[kd, "lens2"] = G.generate(model, prompt, max_new_tokens=NEW, prompt_lens=LENS2, kv_dtype=kd)
    G.clear_sessions()
    return out


def _permuted(monkeypatch):
    """Sessions hand their pages out odd pages first, highest first: non-contiguous, interleaved."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    real = G.PagedKVCache
    order = lambda P: list(range(P))[1::2][::-1] + list(range(P))[0::2][::-1]
    monkeypatch.setattr(G, "PagedKVCache", lambda *a, **k: real(*a, page_order=order, **k))


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("kd", [None, "fp8"], ids=["bf16", "fp8"])
def test_generate_paged_returns_the_contiguous_tokens(model, prompt, contiguous_tokens, monkeypatch, kd, page):
    """Eager and graph, a ragged batch, with prefill_chunk, and one sampled configuration; a second
    call with other lengths reuses the session's cache and graphs (the table is device data)."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    _permuted(monkeypatch)
    G.clear_sessions()
    for name, kw in CONFIGS.items():
        for graph in ("0", "1"):
            monkeypatch.setenv("DPFS_DECODE_GRAPH", graph)
            got = G.generate(model, prompt, max_new_tokens=NEW, prompt_lens=LENS, kv_dtype=kd, kv_page=page, **kw)
            assert got == contiguous_tokens[kd, name], (name, graph)
            assert [len(o) for o in got] == [n + NEW for n in LENS]
    (key,) = G._SESSIONS
    sess = G._SESSIONS[key]
    assert key[4] == kd and key[5] is True and key[6:] == (page, None)
    cache, graphs, held = sess["cache"], sess["graphs"], dict(sess["graphs"])
    assert cache.page == page and cache.fp8 == (kd == "fp8") and sorted(k for k in held if isinstance(k, int)) == [1, 8]
    flat = [e for row in cache.tbl_host.tolist() for e in row if e >= 0]
    assert len(flat) == len(set(flat)) and flat[0] % 2 == 1                  # the permuted order was used
    got = G.generate(model, prompt, max_new_tokens=NEW, prompt_lens=LENS2, kv_dtype=kd, kv_page=page)
    assert got == contiguous_tokens[kd, "lens2"]
    (sess2,) = G._SESSIONS.values()
    assert sess2["cache"] is cache and sess2["graphs"] is graphs
    assert all(graphs[k] is v for k, v in held.items()) and len(graphs) == len(held)      # no new capture
    G.clear_sessions()


@pytest.mark.parametrize("kd", [None, "fp8"], ids=["bf16", "fp8"])
def test_generate_paged_with_a_small_pool(model, prompt, contiguous_tokens, monkeypatch, kd):
    """The rows reach 140, 77 and 41 tokens: 9 + 5 + 3 pages of 16 instead of the 27 of B * MP give
    the same tokens; 10 pages raise on the host, and the device is left clean."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    _permuted(monkeypatch)
    G.clear_sessions()
    for graph in ("0", "1"):
        monkeypatch.setenv("DPFS_DECODE_GRAPH", graph)
        got = G.generate(model, prompt, max_new_tokens=NEW, prompt_lens=LENS, kv_dtype=kd, kv_page=16, kv_pool_pages=17)
        assert got == contiguous_tokens[kd, "ragged"]
        with pytest.raises(RuntimeError, match=r"pages wanted, \d+ free"):
            G.generate(model, prompt, max_new_tokens=NEW, prompt_lens=LENS, kv_dtype=kd, kv_page=16, kv_pool_pages=10)
        torch.cuda.synchronize()
    small = [e["cache"] for k, e in G._SESSIONS.items() if k[6:] == (16, 17)]
    full = G.PagedKVCache(2, 3, 140, 12, 64, torch.bfloat16, torch.device(DEV), 16, None, kd)
    assert len(small) == 1 and small[0].pool_pages == 17 and full.pool_pages == 27
    assert small[0].nbytes() - small[0].tbl.numel() * 4 == (full.nbytes() - full.tbl.numel() * 4) * 17 // 27
    G.clear_sessions()
