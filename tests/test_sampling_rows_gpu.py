"""``_sample_logits_rows`` (csrc/kernels/sample.hip, the per-row form) on the MI355X: bit for bit
against the scalar kernel row by row, greedy rows against ``argmax``, the contract against the
fp64 oracle, the binding's argument checks, and ``generate()`` with per-row settings on the graph
and eager paths.

The comparison with the scalar kernel needs no tolerance: both instantiations run the same
integer sums on the same row.  Tolerance of the mass checks, eps = 1e-4, as in
tests/test_sampling_gpu.py (the arithmetic of a sampled row is unchanged).  It bounds the error
in the share of a row's mass that the kernel attributes to a token or to a nucleus, and is a cap
over the terms a correct kernel can incur, not a fit to what the kernel gives:

* rounding of the scaled logit: the kernel multiplies (z - max z) by log2(e) in fp32 before the
  hardware exp2, an error of |z| 2^-23 in the exponent; |z| <= 40 for these inputs (|logit| <
  20 after ``randn * 4``, 1/T <= 2), so 5e-6 relative per weight, counted twice because a
  share is a ratio of two sums of weights: 1e-5;
* the hardware exponential: 2^-22 relative = 2.4e-7 (again twice);
* the 2^40 fixed-point accumulation: each weight is truncated by < 2^-40 of the row maximum's
  weight, V 2^-40 = 4.6e-8 of the mass at V = 50257 (the total mass is >= the maximum's);
* the fp64 roundings of ``p * total`` and ``u * M``: 2^-52.

Together under 2e-5; the cap leaves a factor of about 5.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-4

# rows, valid vocab, row stride, dtype
SHAPES = {
    "bf16_1000": (4, 1000, 1024, torch.bfloat16),          # baseline bf16 row
    "bf16_50257": (3, 50257, 50304, torch.bfloat16),       # full-vocab row over every wave's range, padded
    "fp32_96": (2, 96, 96, torch.float32),                 # fewer columns than threads
    "fp32_4099": (33, 4099, 4104, torch.float32),          # ragged tail, more rows than one wave of workgroups
}
SETTINGS = {"off": (0, 1.0), "k1": (1, 1.0), "kV": (1 << 20, 1.0), "k50": (50, 1.0), "p0.9": (0, 0.9),
            "k50_p0.9": (50, 0.9)}
TEMPS = (0.5, 1.0, 1.7)
COMBOS = [(T, k, p) for T in TEMPS for k, p in SETTINGS.values()]


@pytest.fixture(scope="module")
def C():
    from distributed_pytorch_from_scratch_amd.ops import _ext
    return _ext.require()


@pytest.fixture(scope="module")
def R():
    from distributed_pytorch_from_scratch_amd.ops import reference
    return reference


@pytest.fixture(scope="module")
def rows():
    """Per shape: the logits in their dtype (``randn * 4``, so the bf16 rows tie; the padding
    columns hold the largest values of the row), their fp32 valid part, and the uniforms."""
    out = {}
    for i, (name, (B, V, ld, dt)) in enumerate(SHAPES.items()):
        g = torch.Generator().manual_seed(100 + i)
        x = (torch.randn(B, ld, generator=g) * 4).to(dt)
        x[:, V:] = 30.0
        u = torch.rand(B, generator=g)
        u[0] = 0.0
        out[name] = (x, x[:, :V].float(), u)
    return out


def _table(temps, ks, ps, seeds, rids):
    """The five settings tensors (host) from per-row lists; temperature 0 is a greedy row."""
    inv_t = torch.tensor([1.0 / t if t > 0 else 0.0 for t in temps], dtype=torch.float64).float()
    return (inv_t, torch.tensor(ks, dtype=torch.int32), torch.tensor(ps, dtype=torch.float64),
            torch.tensor(seeds, dtype=torch.int64), torch.tensor(rids, dtype=torch.int32))


def _run(C, x, V, tab, pos, u=None):
    B = x.size(0)
    got = C._sample_logits_rows(x.cuda(), V, *(t.cuda() for t in tab), pos.cuda(), None if u is None else u.cuda())
    torch.cuda.synchronize()
    ids, kept, thresh, uo = got
    assert ids.dtype == torch.int64 and kept.dtype == torch.int32 and thresh.dtype == uo.dtype == torch.float32
    assert all(t.shape == (B,) for t in got)
    return tuple(t.cpu() for t in got)


def _check(xv, T, k, p, u, ids, kept, thresh, uo):
    """Every row against the contract, from the fp32 valid logits ``xv`` (B, V) alone."""
    B, V = xv.shape
    assert torch.equal(uo, u)
    assert bool(((ids >= 0) & (ids < V)).all())
    surv = torch.ones_like(xv, dtype=torch.bool)
    if 0 < k < V:
        vk = xv.topk(k, dim=-1).values[:, -1]
        surv = xv >= vk[:, None]
        assert bool((thresh >= vk).all())
        if p >= 1:
            assert torch.equal(thresh, vk)
    elif p >= 1:
        assert torch.equal(thresh, xv.min(-1).values)
    keep = surv & (xv >= thresh[:, None])
    assert torch.equal(kept.long(), keep.sum(-1))
    assert bool((xv == thresh[:, None]).any(-1).all())                  # a value present in the row
    chosen = xv.gather(-1, ids[:, None])[:, 0]
    assert bool((chosen >= thresh).all()) and bool(keep.gather(-1, ids[:, None]).all())
    z = (xv * torch.tensor(1.0 / T, dtype=torch.float32)).double()
    w = torch.exp(z - z.max(-1, keepdim=True).values)
    if p < 1:
        total = (w * surv).sum(-1)
        share = (w * keep).sum(-1) / total
        assert bool((share >= p - EPS).all()), (share - p).min()
        # the next larger distinct value present among the survivors must not suffice
        above = surv & (xv > thresh[:, None])
        nxt = torch.where(above, xv, torch.full_like(xv, float("inf"))).min(-1).values
        share_up = (w * (surv & (xv >= nxt[:, None]))).sum(-1) / total
        has = above.any(-1)
        assert bool((share_up[has] < p + EPS).all()), (share_up[has] - p).max()
    wk = w * keep
    cum = wk.cumsum(-1)
    M = cum[:, -1]
    hi = cum.gather(-1, ids[:, None])[:, 0] / M
    lo = hi - wk.gather(-1, ids[:, None])[:, 0] / M
    ud = u.double()
    assert bool((wk.gather(-1, ids[:, None])[:, 0] > 0).all())
    assert bool(((lo - EPS <= ud) & (ud <= hi + EPS)).all()), ((lo - ud).max(), (ud - hi).max())


def _launches(B):
    """Settings of the B rows for as many launches as it takes to give every (T, top_k, top_p)
    of COMBOS to some row."""
    return [[COMBOS[(start + b) % len(COMBOS)] for b in range(B)] for start in range(0, len(COMBOS), B)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_match_the_scalar_kernel_bit_for_bit(C, rows, shape):
    """Row id 0 with a seed, a position and settings of its own per row: row b equals the scalar
    kernel on ``x[b:b+1]`` with that row's scalars (whose row index, the counter word, is 0), in
    all four outputs.  Equal settings, one seed and row id b: one scalar call on all rows."""
    B, V, _, _ = SHAPES[shape]
    x, _, _ = rows[shape]
    xc = x.cuda()
    pos = torch.arange(B, dtype=torch.int64) * 977 + 3
    pos[-1] = 2 ** 33 + 5
    pc = pos.cuda()
    for n, combo in enumerate(_launches(B)):
        temps, ks, ps = (list(c) for c in zip(*combo))
        seeds = [1234 + 7 * b + 100 * n for b in range(B)]
        seeds[0], seeds[-1] = -7 - n, 2 ** 62 + 3 + n
        got = _run(C, x, V, _table(temps, ks, ps, seeds, [0] * B), pos)
        for b in range(B):
            want = C.sample_logits(xc[b:b + 1], V, temps[b], ks[b], ps[b], seeds[b], pc[b:b + 1])
            for g, w in zip(got, want):
                assert torch.equal(g[b:b + 1], w.cpu()), (b, combo[b])
    for T, k, p in ((0.8, 50, 0.9), (1.7, 0, 1.0)):
        got = _run(C, x, V, _table([T] * B, [k] * B, [p] * B, [5] * B, list(range(B))), pos)
        want = C.sample_logits(xc, V, T, k, p, 5, pc)
        assert all(torch.equal(g, w.cpu()) for g, w in zip(got, want))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_greedy_rows(C, rows, shape):
    """inv_t = 0: ids = ``argmax`` over the valid columns (the first of the planted duplicate
    maxima), kept = the number of maxima, thresh = the maximum, u = 0, whatever top_k / top_p /
    a supplied u say; mixed with sampled rows in one launch, which equal the scalar kernel."""
    B, V, _, dt = SHAPES[shape]
    x, _, u = rows[shape]
    x = x.clone()
    g = torch.Generator().manual_seed(3)
    greedy = [b % 3 != 1 for b in range(B)]                 # B = 2: one greedy, one sampled row
    want_kept = []
    for b in range(B):
        n = 1 + b % 4                                       # 1 .. 4 maxima
        cols = torch.randperm(V, generator=g)[:n]
        if b == 0:
            cols[0] = V - 1                                 # the last valid column, next to the padding
        if b == B - 1:
            cols[0] = 0
        x[b, cols] = 25.0
        want_kept.append(int(cols.unique().numel()))
    xv = x[:, :V].float()
    temps = [0.0 if gr else 0.8 for gr in greedy]
    ks, ps = [(5, 0, 1)[b % 3] for b in range(B)], [(0.5, 1.0, 0.9)[b % 3] for b in range(B)]
    seeds, pos = [11 + b for b in range(B)], torch.arange(B, dtype=torch.int64)
    tab = _table(temps, ks, ps, seeds, [0] * B)
    xc, pc = x.cuda(), pos.cuda()
    for uu in (None, u):
        ids, kept, thresh, uo = _run(C, x, V, tab, pos, uu)
        gi = [b for b in range(B) if greedy[b]]
        assert torch.equal(ids[gi], xv[gi].argmax(-1))
        assert kept[gi].tolist() == [want_kept[b] for b in gi]
        assert torch.equal(kept[gi].long(), (xv[gi] == xv[gi].max(-1, keepdim=True).values).sum(-1))
        assert bool((thresh[gi] == 25.0).all()) and bool((uo[gi] == 0.0).all())
        for b in range(B):
            if not greedy[b]:
                want = C.sample_logits(xc[b:b + 1], V, temps[b], ks[b], ps[b], seeds[b], pc[b:b + 1],
                                       None if uu is None else uu[b:b + 1].cuda())
                assert all(torch.equal(t[b:b + 1], w.cpu()) for t, w in zip((ids, kept, thresh, uo), want)), b
    # every row greedy, ties among all columns of a constant row: index 0, kept = V
    flat = torch.full_like(x, 1.5)
    flat[:, V:] = 30.0
    ids, kept, thresh, uo = _run(C, flat, V, _table([0.0] * B, [0] * B, [1.0] * B, [0] * B, [0] * B), pos)
    assert bool((ids == 0).all()) and bool((kept == V).all()) and bool((thresh == 1.5).all()) and bool((uo == 0).all())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_match_contract(C, R, rows, shape):
    """Supplied uniforms, settings per row: every row against the contract (fp64 masses), and
    with top-p off against the oracle's kept / thresh exactly."""
    B, V, _, _ = SHAPES[shape]
    x, xv, u = rows[shape]
    pos = torch.zeros(B, dtype=torch.int64)
    for combo in _launches(B):
        temps, ks, ps = (list(c) for c in zip(*combo))
        tab = _table(temps, ks, ps, [0] * B, [0] * B)
        got = _run(C, x, V, tab, pos, u)
        for b, (T, k, p) in enumerate(combo):
            _check(xv[b:b + 1], T, k, p, u[b:b + 1], *(t[b:b + 1] for t in got))
        if V <= 4099:       # the oracle row by row (the full-vocab rows are covered by _check)
            _, kept_r, thresh_r, _ = R.sample_logits_rows(x, V, *tab, pos, u)
            off = [b for b, (_, _, p) in enumerate(combo) if p >= 1]
            assert torch.equal(got[1][off], kept_r[off]) and torch.equal(got[2][off], thresh_r[off])


def test_generator_matches_oracle(C, R, rows):
    """Without ``u`` the uniform of row b is ``sample_uniform(seed[b], pos[b], rid[b])``."""
    x, _, _ = rows["fp32_4099"]
    B = 33
    pos = torch.arange(B, dtype=torch.int64) * 977
    pos[1] = 2 ** 33 + 5
    seeds = [(-1) ** b * (2 ** (b % 62) + b) for b in range(B)]
    rids = [(5 * b) % 7 for b in range(B)]
    rids[2] = 2 ** 31 - 1
    got = _run(C, x, 4099, _table([1.7] * B, [0] * B, [0.9] * B, seeds, rids), pos)
    want = torch.tensor([R.sample_uniform(s, int(p), r) for s, p, r in zip(seeds, pos, rids)], dtype=torch.float32)
    assert torch.equal(got[3], want)


def test_argument_checks(C, rows):
    x, _, _ = rows["fp32_96"]
    xc, pos = x.cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    good = [t.cuda() for t in _table([1.0, 0.0], [0, 3], [1.0, 0.9], [1, 2], [0, 0])]
    names = ("inv_t", "top_k", "top_p", "seed", "rid")
    wrong_dtype = (torch.float64, torch.int64, torch.float32, torch.int32, torch.int64)
    C._sample_logits_rows(xc, 96, *good, pos)
    for i, name in enumerate(names):
        for bad in (good[i].to(wrong_dtype[i]), torch.cat([good[i], good[i]]), good[i][:1], good[i].cpu(),
                    torch.stack([good[i], good[i]], 1)[:, 0]):          # dtype, length x2, device, stride
            args = list(good)
            args[i] = bad
            with pytest.raises(RuntimeError, match=name):
                C._sample_logits_rows(xc, 96, *args, pos)
    for V in (97, 0):
        with pytest.raises(RuntimeError, match="sample_logits_rows"):
            C._sample_logits_rows(xc, V, *good, pos)
    with pytest.raises(RuntimeError, match="pos"):
        C._sample_logits_rows(xc, 96, *good, pos.int())
    with pytest.raises(RuntimeError, match="pos"):
        C._sample_logits_rows(xc, 96, *good, pos[:1])
    with pytest.raises(RuntimeError):
        C._sample_logits_rows(xc.half(), 96, *good, pos)
    with pytest.raises(RuntimeError, match="u "):
        C._sample_logits_rows(xc, 96, *good, pos, torch.zeros(3, device="cuda"))


def test_fp32_logits_reach_the_kernel(C, rows, monkeypatch):
    """fp32 logits on the GPU dispatch to the HIP kernel (through ``fp32_native``), not to the
    oracle's tensor ops."""
    from distributed_pytorch_from_scratch_amd.ops import fp32_native, reference
    from distributed_pytorch_from_scratch_amd.ops.dispatch import K
    x, xv, u = rows["fp32_96"]
    xc = x.cuda()
    assert K(xc) is fp32_native and K(xc.bfloat16()) is C
    monkeypatch.setattr(reference, "sample_logits_rows", None)     # the oracle must not be what runs
    monkeypatch.setattr(reference, "_sample_logits_rows", None)
    tab = [t.cuda() for t in _table([1.0, 1.7], [10, 0], [0.9, 0.8], [0, 0], [0, 0])]
    got = [t.cpu() for t in K(xc)._sample_logits_rows(xc, 96, *tab, torch.zeros(2, dtype=torch.int64).cuda(), u.cuda())]
    _check(xv[0:1], 1.0, 10, 0.9, u[0:1], *(t[0:1] for t in got))
    _check(xv[1:2], 1.7, 0, 0.8, u[1:2], *(t[1:2] for t in got))


@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29568")
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    yield
    destroy_dist_env()


@pytest.fixture(scope="module")
def model(dist1):
    from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
    args = get_preset("gpt2-small", num_layers=2)
    m = Transformer.from_args(args).cuda()
    m.reset_parameters()
    m.eval()
    prompt = torch.randint(0, args.vocab_size, (3, 240), device="cuda",
                           generator=torch.Generator("cuda").manual_seed(1))
    return m, prompt


ROWS_A = dict(temperature=[0.8, 1.3, 0.5], top_k=[40, 0, 5], top_p=[0.95, 0.9, 1.0], seed=[3, 4, 5])
ROWS_B = dict(temperature=[1.0, 0.7, 0.9], top_k=[0, 100, 40], top_p=[1.0, 0.8, 0.95], seed=[13, -4, 2 ** 40])
ROWS_C = dict(temperature=[0.6, 0, 1.1], top_k=[20, 3, 0], top_p=0.9, seed=[7, 8, 9])     # a greedy row in the middle
SCALAR = dict(temperature=0.8, top_k=40, top_p=0.95, seed=3)


def test_generate_rows_graph_matches_eager_and_shares_two_graphs(model, monkeypatch):
    """Per-row settings decode the same tokens on the eager step and on the captured graphs;
    lists of equal settings with a scalar seed give the scalar sampled call; all-zero
    temperatures give greedy; three calls with three different settings and seed lists capture
    (1, "rows") and (8, "rows") once and replay the same graph objects; the scalar sampled call
    still keys its graphs on its settings; the greedy row of a mixed batch decodes as in the
    all-greedy call."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, prompt = model
    vocab = m.args.vocab_size
    gen = lambda **kw: G.generate(m, prompt, max_new_tokens=40, **kw)
    G.clear_sessions()
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    eager = {n: gen(**s) for n, s in (("a", ROWS_A), ("b", ROWS_B), ("c", ROWS_C), ("scalar", SCALAR))}
    eager_greedy = gen()
    assert not G._SESSIONS
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    greedy = gen()
    assert greedy == eager_greedy
    (sess,) = G._SESSIONS.values()
    assert sorted(map(str, sess["graphs"])) == sorted(map(str, [1, 8]))
    a = gen(**ROWS_A)
    assert a == eager["a"] and a != greedy
    assert all(len(o) == 280 and all(0 <= t < vocab for t in o) for o in a)
    held = dict(sess["graphs"])
    want_keys = sorted(map(str, [1, 8, (1, "rows"), (8, "rows")]))
    assert sorted(map(str, held)) == want_keys
    assert gen(**ROWS_B) == eager["b"]
    c = gen(**ROWS_C)
    assert c == eager["c"]
    assert gen(**ROWS_A) == a                                           # the table is rewritten by every call
    (sess2,) = G._SESSIONS.values()
    assert sess2["graphs"] is sess["graphs"] and sorted(map(str, sess2["graphs"])) == want_keys
    assert all(sess2["graphs"][k] is v for k, v in held.items())
    # all-greedy lists: the greedy tokens, through the per-row graphs
    all_greedy = gen(temperature=[0, 0, 0], top_k=[5, 0, 1], top_p=0.5, seed=[1, 2, 3])
    assert all_greedy == greedy
    assert sorted(map(str, sess["graphs"])) == want_keys
    # the greedy row of a mixed batch: no decode kernel has a cross-row data dependence
    assert c[1] == all_greedy[1] and c[0] != greedy[0] and c[2] != greedy[2]
    # the scalar path: its own keys, its own tokens, and the lists that reproduce them
    scalar = gen(**SCALAR)
    assert scalar == eager["scalar"]
    sk = (0.8, 40, 0.95, 3)
    assert sorted(map(str, sess["graphs"])) == sorted(map(str, [1, 8, (1, "rows"), (8, "rows"), (1, sk), (8, sk)]))
    lists = gen(temperature=[0.8] * 3, top_k=[40] * 3, top_p=[0.95] * 3, seed=3)
    assert lists == scalar
    assert gen(temperature=[0.8] * 3, top_k=[40] * 3, top_p=[0.95] * 3, seed=[3, 3, 3])[0] == scalar[0]   # row id 0
    assert all(sess["graphs"][k] is v for k, v in held.items())
    G.clear_sessions()


def test_generate_rows_ragged_graph_matches_eager(model, monkeypatch):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, prompt = model
    lens = [240, 101, 7]
    G.clear_sessions()
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    eager = G.generate(m, prompt, max_new_tokens=40, prompt_lens=lens, **ROWS_C)
    eager_greedy = G.generate(m, prompt, max_new_tokens=40, prompt_lens=lens)
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    graph = G.generate(m, prompt, max_new_tokens=40, prompt_lens=lens, **ROWS_C)
    assert graph == eager
    assert [len(o) for o in graph] == [n + 40 for n in lens]
    assert graph[1] == eager_greedy[1] and graph[0] != eager_greedy[0]
    (sess,) = G._SESSIONS.values()
    assert sorted(map(str, sess["graphs"])) == sorted(map(str, [(1, "rows"), (8, "rows")]))
    G.clear_sessions()
