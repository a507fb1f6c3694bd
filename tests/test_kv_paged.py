"""The paged KV cache on the CPU: the page allocator of ``PagedKVCache``, the paged reference ops
(``ops/reference.py``) against the contiguous ones on the same logical cache content (exact: the
paged ops gather / scatter through the table and call the contiguous ops), ``generate(kv_page=...)``
against ``generate`` token for token, and the argument checks.  The GPU kernels are compared in
tests/test_kv_paged_gpu.py."""
import random

import pytest
import torch

import numerics as N
from dist_helpers import run_distributed

from distributed_pytorch_from_scratch_amd.ops import reference as R

B, H = N.DEC_B, N.DEC_H


def _cache(page=16, t_max=40, pool=None, order=None, kd=None, B_=2):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    return G.PagedKVCache(2, B_, t_max, 2, 32, torch.float32, torch.device("cpu"), page, pool, kd, order)


# ------------------------------------------------------------------------- allocator --
def test_reserve_grows_row_by_row_and_never_hands_a_page_out_twice():
    c = _cache()                                   # MP = 3, P = 6
    assert c.max_pages == 3 and c.pool_pages == 6 and c.ragged and c.tbl.shape == (2, 3)
    assert c.tbl.tolist() == [[-1] * 3] * 2 and c.uploads == 0
    c.reserve([1, 17])
    assert c.mapped == [1, 2] and c.uploads == 1
    c.reserve([16, 32])                            # the same pages cover it: no upload
    assert c.mapped == [1, 2] and c.uploads == 1
    c.reserve([33, 0])                             # a row never shrinks
    assert c.mapped == [3, 2] and c.uploads == 2
    c.reserve([1000, 1000])                        # clamped at t_max
    assert c.mapped == [3, 3] and c.uploads == 3 and not c.free
    live = [e for row in c.tbl_host.tolist() for e in row]
    assert sorted(live) == list(range(6))
    assert torch.equal(c.tbl.cpu(), c.tbl_host)


def test_permuted_order_and_reset():
    order = [4, 1, 5, 0, 3, 2]
    c = _cache(order=order)
    c.reserve([17, 16])
    assert c.tbl_host.tolist() == [[4, 1, -1], [5, -1, -1]]
    c.reserve([17, 33])
    assert c.tbl_host.tolist() == [[4, 1, -1], [5, 0, 3]]
    c.set_lens([17, 33])
    up = c.uploads
    c.reset()
    assert c.lens == [0, 0] and c.len == 0 and c.mapped == [0, 0] and len(c.free) == 6
    assert c.tbl.tolist() == [[-1] * 3] * 2 and c.uploads == up + 1
    c.reset()                                      # nothing mapped: nothing to upload
    assert c.uploads == up + 1
    c.reserve([1, 1])                              # the order starts over
    assert c.tbl_host.tolist() == [[4, -1, -1], [1, -1, -1]]
    c2 = _cache(order=lambda P: list(reversed(range(P))))
    c2.reserve([16, 16])
    assert c2.tbl_host[:, 0].tolist() == [5, 4]
    with pytest.raises(ValueError, match="permutation"):
        _cache(order=[0, 1, 2, 3, 4, 4])


def test_exhaustion_raises_and_maps_nothing():
    c = _cache(pool=3)
    c.reserve([17, 16])                            # 2 + 1 pages: the pool is used up
    before, up = c.tbl_host.clone(), c.uploads
    with pytest.raises(RuntimeError, match=r"2 pages wanted, 0 free"):
        c.reserve([33, 17])
    assert torch.equal(c.tbl_host, before) and c.mapped == [2, 1] and c.uploads == up
    c2 = _cache(pool=3)
    with pytest.raises(RuntimeError, match=r"4 pages wanted, 3 free"):
        c2.reserve([20, 20])
    assert c2.mapped == [0, 0] and len(c2.free) == 3 and c2.uploads == 0


def test_shapes_bytes_and_argument_errors():
    c = _cache(page=16, t_max=40, pool=4)
    assert c.k[0].shape == (4, 16, 2, 32) and len(c.k) == 2 and not c.fp8
    assert c.nbytes() == 2 * 2 * 4 * 16 * 2 * 32 * 4 + 2 * 3 * 4
    c8 = _cache(pool=4, kd="fp8")
    assert c8.fp8 and c8.k[0].dtype == torch.float8_e4m3fn and c8.ks[0].shape == (4, 16, 2)
    assert c8.nbytes() == 2 * 2 * 4 * 16 * 2 * (32 + 4) + 2 * 3 * 4
    assert c8.sample_rows().inv_t.shape == (2,)    # the batch, not the pool
    for bad in (8, 24, 512, 0, -16):
        with pytest.raises(ValueError, match="kv_page"):
            _cache(page=bad)
    with pytest.raises(ValueError, match="pool_pages"):
        _cache(pool=0)


# --------------------------------------------------------------------- reference ops --
def _scatter(cache, page, P, tbl, fill):
    """A pool (P, page, ...) that holds ``cache`` (B, T, ...) through ``tbl``; other rows ``fill``."""
    pool = torch.full((P, page) + tuple(cache.shape[2:]), fill, dtype=torch.float32).to(cache.dtype)
    for b in range(cache.size(0)):
        for t in range(cache.size(1)):
            pool[tbl[b, t // page], t % page] = cache[b, t]
    return pool


def _table(t_max, page, seed):
    MP = -(-t_max // page)
    perm = list(range(B * MP + 2))
    random.Random(seed).shuffle(perm)
    return torch.tensor([perm[b::B][:MP] for b in range(B)], dtype=torch.int32), B * MP + 2   # row-interleaved


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("hd,page,t_max", [(32, 16, 16), (64, 16, 300), (128, 64, 300), (32, 256, 512)])
def test_reference_paged_ops_equal_the_contiguous_ones(hd, page, t_max, fp8):
    g = torch.Generator().manual_seed(hd + page + t_max)
    tbl, P = _table(t_max, page, 3)
    kc = torch.randn(B, t_max, H, hd, generator=g)
    vc = torch.randn(B, t_max, H, hd, generator=g)
    lens = torch.tensor([min(page + 1, t_max - 1), t_max // 2], dtype=torch.int32)
    if fp8:
        (kc, ksc), (vc, vsc) = R._kv_quant_rows(kc), R._kv_quant_rows(vc)
        pools = [_scatter(x, page, P, tbl, float("nan")) for x in (kc, vc, ksc, vsc)]
        cont = [kc.clone(), vc.clone(), ksc.clone(), vsc.clone()]
    else:
        pools = [_scatter(x, page, P, tbl, float("nan")) for x in (kc, vc)] + [None, None]
        cont = [kc.clone(), vc.clone()]
    scale = hd ** -0.5
    # decode step: rope + append at len[b], then attention over [0, len[b]]
    qkv = torch.randn(B, 3 * H * hd, generator=g)
    pos = lens.long()
    tab = R.rope_table(t_max, hd, 10000.0)
    qa, qb = qkv.clone(), qkv.clone()
    if fp8:
        R._rope_append_q8(qa, pos, tab, *cont, lens)
        want = R._attn_decode_q8(qa, *cont, lens, scale)
    else:
        R.rope_append(qa, pos, tab, *cont, lens)
        want = R.attn_decode(qa, *cont, lens, scale)
    R._rope_append_paged(qb, pos, tab, *pools, tbl, lens, t_max, page)
    got = R._attn_decode_paged(qb, *pools, tbl, lens, t_max, page, scale)
    assert torch.equal(qa, qb) and torch.equal(got, want)
    # a chunk of T tokens at len[b] + 1 (row 1: n = 0 when the cache is that short), then extend
    lens1 = (lens + 1).clamp(max=t_max)
    T = 5
    n = torch.tensor([T, 0 if t_max == 16 else 3], dtype=torch.int32)
    ch = torch.randn(B * T, 3 * H * hd, generator=g)
    if fp8:
        R._kv_append_chunk_q8(ch, *cont, lens1, n)
        want = R._attn_extend_q8(ch, *cont, lens1, n, scale)
    else:
        R._kv_append_chunk(ch, *cont, lens1, n)
        want = R._attn_extend(ch, *cont, lens1, n, scale)
    R._kv_append_chunk_paged(ch, *pools, tbl, lens1, n, t_max, page)
    got = R._attn_extend_paged(ch, *pools, tbl, lens1, n, t_max, page, scale)
    assert torch.equal(got, want)
    # the pools hold exactly the contiguous caches, and nothing else was written
    u8 = lambda x: x.view(torch.uint8) if x.dtype == torch.float8_e4m3fn else x.view(torch.int32)
    for pool, c in zip(pools, cont):
        if pool is None:
            continue
        assert torch.equal(u8(R._paged_view(pool, tbl, t_max)), u8(c))
        owned = torch.zeros(P, dtype=torch.bool)
        owned[tbl.long().flatten()] = True
        rest = pool[~owned].float()
        assert torch.isnan(rest).all()


def test_reference_append_through_a_bad_entry_is_dropped():
    hd, page, t_max = 32, 16, 40
    tbl, P = _table(t_max, page, 1)
    tbl[0, 1] = -1
    tbl[1, 0] = P
    pools = [torch.zeros(P, page, H, hd), torch.zeros(P, page, H, hd), None, None]
    ch = torch.ones(B * 20, 3 * H * hd)
    R._kv_append_chunk_paged(ch, *pools, tbl, torch.tensor([10, 10], dtype=torch.int32), None, t_max, page)
    k = pools[0]
    assert k[tbl[0, 0], 10:].eq(1).all() and k[tbl[0, 0], :10].eq(0).all()     # keys 10..15 of row 0
    assert k[tbl[1, 1], :14].eq(1).all() and k[tbl[1, 1], 14:].eq(0).all()     # keys 16..29 of row 1
    assert int(k.sum()) == (6 + 14) * H * hd


# ------------------------------------------------------------------------ model level --
def _tiny_model():
    """The small model of tests/test_kv_fp8.py (two heads: head_dim 32)."""
    from distributed_pytorch_from_scratch_amd.models import ModelArgs, Transformer
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    args = ModelArgs(attn_dim=64, ffn_dim=128, num_heads=2, num_layers=2, vocab_size=96, maxlen=64, vocab_pad_to=1)
    m = Transformer.from_args(args)
    set_seed(0)
    m.reset_parameters()
    m.eval()
    g = torch.Generator().manual_seed(5)
    return m, torch.randint(3, 96, (2, 21), generator=g)


def _model_level(rank, world):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, ids = _tiny_model()
    out = {"same": {}, "errs": {}}
    real = G.PagedKVCache
    G.PagedKVCache = lambda *a, **k: real(*a, page_order=lambda P: [p for i in range(2) for p in range(P)[i::2]][::-1], **k)
    try:
        for name, kw in (("ragged", dict(prompt_lens=[21, 15])), ("ragged_chunked", dict(prompt_lens=[21, 15], prefill_chunk=6)),
                         ("ragged_fp8", dict(prompt_lens=[21, 15], kv_dtype="fp8")),
                         ("sampled", dict(prompt_lens=[17, 21], temperature=0.8, top_k=20, seed=3))):
            G.clear_sessions()
            want = G.generate(m, ids, 24, **kw)
            got = G.generate(m, ids, 24, kv_page=16, **kw)
            out["same"][name] = got == want and len(got[0]) > kw["prompt_lens"][0] + 12
        G.clear_sessions()
        want = G.generate(m, ids, 24, prompt_lens=[21, 21])        # a uniform paged call is the per-row call
        out["same"]["uniform"] = G.generate(m, ids, 24, kv_page=16) == want
        out["same"]["uniform_vs_uniform"] = G.generate(m, ids, 24) == want
        # a pool of the pages the rows need (3 + 3 of MP = 3 each ... at t_max 45: 3 pages a row)
        out["same"]["small_pool"] = G.generate(m, ids, 11, prompt_lens=[21, 5], kv_page=16, kv_pool_pages=3) == \
            G.generate(m, ids, 11, prompt_lens=[21, 5])
        try:
            G.generate(m, ids, 11, prompt_lens=[21, 5], kv_page=16, kv_pool_pages=2)
        except RuntimeError as ex:
            out["errs"]["pool"] = str(ex)
        for bad in (8, 24, 512):
            try:
                G.generate(m, ids, 2, kv_page=bad)
            except ValueError as ex:
                out["errs"][bad] = str(ex)
        try:
            G.generate(m, ids, 2, kv_pool_pages=4)
        except ValueError as ex:
            out["errs"]["pool_only"] = str(ex)
    finally:
        G.PagedKVCache = real
        G.clear_sessions()
    return out


@pytest.fixture(scope="module")
def model_level():
    return run_distributed(_model_level, 1)[0]


def test_generate_paged_equals_generate_token_for_token(model_level):
    assert model_level["same"] and all(model_level["same"].values()), model_level["same"]


def test_generate_argument_and_pool_errors(model_level):
    errs = model_level["errs"]
    assert set(errs) == {"pool", 8, 24, 512, "pool_only"}
    assert all("kv_page" in errs[k] for k in (8, 24, 512, "pool_only"))
    assert "pages wanted" in errs["pool"] and "free" in errs["pool"]


def test_kv_page_cli_flags():
    from distributed_pytorch_from_scratch_amd.evaluate import get_test_args, main
    base = ["--data_path", "d", "--ckpt_dir", "c"]
    a = get_test_args(base)
    assert a.kv_page == 0 and a.kv_pool_pages == 0
    a = get_test_args(base + ["--kv_page", "64", "--kv_pool_pages", "12"])
    assert a.kv_page == 64 and a.kv_pool_pages == 12
    with pytest.raises(ValueError, match="kv_page"):
        main(base + ["--kv_page", "16", "--no_kv_cache"])
    for bad in ("8", "24", "512"):
        with pytest.raises(ValueError, match="kv_page"):
            main(base + ["--kv_page", bad])
    with pytest.raises(ValueError, match="kv_page"):
        main(base + ["--kv_pool_pages", "4"])
