"""``sample_logits`` (csrc/kernels/sample.hip) on the MI355X against the fp64 oracle
(``ops/reference.sample_logits``), and sampled ``generate()`` on the graph and eager paths.

Tolerance of the mass checks, eps = 1e-4.  It bounds the error in the share of a row's mass
that the kernel attributes to a token or to a nucleus, and is a cap over the terms a correct
kernel can incur, not a fit to what the kernel gives:

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
import statistics

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
SETTINGS = {"off": (0, 1.0), "k1": (1, 1.0), "k50": (50, 1.0), "p0.9": (0, 0.9), "k50_p0.9": (50, 0.9)}
TEMPS = (0.5, 1.0, 1.7)


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


def _run(C, x, V, T, k, p, u=None, seed=0, pos=None):
    B = x.size(0)
    pos = torch.zeros(B, dtype=torch.int64) if pos is None else pos
    got = C.sample_logits(x.cuda(), V, T, k, p, seed, pos.cuda(), None if u is None else u.cuda())
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


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sample_logits_matches_contract(C, R, rows, shape, setting):
    _, V, _, _ = SHAPES[shape]
    k, p = SETTINGS[setting]
    x, xv, u = rows[shape]
    for T in TEMPS:
        got = _run(C, x, V, T, k, p, u)
        _check(xv, T, k, p, u, *got)
        if p >= 1:      # no mass enters the cutoff: the oracle's kept / thresh hold exactly
            _, kept_r, thresh_r, _ = R.sample_logits(x, V, T, k, p, 0, torch.zeros(x.size(0), dtype=torch.int64), u)
            assert torch.equal(got[1], kept_r) and torch.equal(got[2], thresh_r)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_top_k_1_is_argmax(C, rows, shape):
    B, V, _, _ = SHAPES[shape]
    x, _, u = rows[shape]
    x = x.clone()
    col = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(3))
    col[0], col[-1] = V - 1, 0
    x[torch.arange(B), col] = 25.0                     # a unique maximum among the valid columns
    for T in TEMPS:
        ids, kept, thresh, _ = _run(C, x, V, T, 1, 1.0, u)
        assert torch.equal(ids, col) and bool((kept == 1).all()) and bool((thresh == 25.0).all())
        assert torch.equal(_run(C, x, V, T, 1, 0.5, u)[0], col)


def test_unpadded_and_sliced_rows(C, rows):
    """Rows that are not a whole number of 16-byte vectors, and a column slice of a wider
    buffer (unaligned rows): the same answers as the padded layout."""
    x, xv, u = rows["bf16_1000"]
    for V in (1000, 997, 63, 1):
        want = _run(C, x, V, 0.9, 7, 0.8, u)
        _check(xv[:, :V], 0.9, 7, 0.8, u, *want)
        sl = x.cuda()[:, :V]
        got = C.sample_logits(sl, V, 0.9, 7, 0.8, 0, torch.zeros(4, dtype=torch.int64).cuda(), u.cuda())
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
        off = torch.cat([x[:, :1], x[:, :V]], 1).cuda()[:, 1:]           # rows start 2 bytes off
        got = C.sample_logits(off, V, 0.9, 7, 0.8, 0, torch.zeros(4, dtype=torch.int64).cuda(), u.cuda())
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
    x32, xv32, u32 = rows["fp32_4099"]
    want = _run(C, x32, 4099, 1.0, 50, 0.9, u32)
    got = _run(C, x32[:, :4099].contiguous(), 4099, 1.0, 50, 0.9, u32)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_generator_matches_oracle_and_is_deterministic(C, R, rows):
    x, xv, _ = rows["bf16_50257"]
    pos = torch.tensor([0, 2 ** 33 + 5, 1023], dtype=torch.int64)
    for seed in (0, 1234, -7, 2 ** 62 + 3):
        a = _run(C, x, 50257, 0.8, 50, 0.9, None, seed, pos)
        b = _run(C, x, 50257, 0.8, 50, 0.9, None, seed, pos)
        assert all(torch.equal(s, t) for s, t in zip(a, b))                 # bit-identical, all four
        want = torch.tensor([R.sample_uniform(seed, int(p), r) for r, p in enumerate(pos)], dtype=torch.float32)
        assert torch.equal(a[3], want)
        _check(xv, 0.8, 50, 0.9, want, *a)
    x32, _, _ = rows["fp32_4099"]
    pos = torch.arange(33, dtype=torch.int64) * 977
    a = _run(C, x32, 4099, 1.7, 0, 0.9, None, 5, pos)
    assert all(torch.equal(s, t) for s, t in zip(a, _run(C, x32, 4099, 1.7, 0, 0.9, None, 5, pos)))
    assert torch.equal(a[3], torch.tensor([R.sample_uniform(5, int(p), r) for r, p in enumerate(pos)],
                                          dtype=torch.float32))


def test_argument_checks(C, rows):
    x, _, _ = rows["fp32_96"]
    xc, pos = x.cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    for bad in (dict(T=0.0), dict(T=-1.0), dict(p=0.0), dict(p=1.5), dict(V=97), dict(V=0), dict(k=-1)):
        a = dict(V=96, T=1.0, k=0, p=1.0)
        a.update(bad)
        with pytest.raises(RuntimeError, match="sample_logits"):
            C.sample_logits(xc, a["V"], a["T"], a["k"], a["p"], 0, pos)
    with pytest.raises(RuntimeError, match="pos"):
        C.sample_logits(xc, 96, 1.0, 0, 1.0, 0, pos.int())
    with pytest.raises(RuntimeError):
        C.sample_logits(xc.half(), 96, 1.0, 0, 1.0, 0, pos)


def test_fp32_logits_reach_the_kernel(C, rows, monkeypatch):
    """fp32 logits on the GPU dispatch to the HIP kernel (through ``fp32_native``), not to the
    oracle's tensor ops."""
    from distributed_pytorch_from_scratch_amd.ops import fp32_native, reference
    from distributed_pytorch_from_scratch_amd.ops.dispatch import K
    x, xv, u = rows["fp32_96"]
    xc = x.cuda()
    assert K(xc) is fp32_native and K(xc.bfloat16()) is C
    monkeypatch.setattr(reference, "sample_logits", None)          # the oracle must not be what runs
    got = K(xc).sample_logits(xc, 96, 1.0, 10, 0.9, 0, torch.zeros(2, dtype=torch.int64).cuda(), u.cuda())
    _check(xv, 1.0, 10, 0.9, u, *(t.cpu() for t in got))


@pytest.mark.parametrize("mode", ["rows", "positions"])
def test_distribution_through_the_generator(C, R, mode):
    """Pearson's chi-squared of 8192 draws against the oracle's probabilities, below the
    alpha = 1e-6 critical value for 11 degrees of freedom (Wilson-Hilferty, ~49.9): once as
    8192 rows at position 0, once as 8192 positions of row 0.  Seed fixed: deterministic."""
    V, N, T, seed = 512, 8192, 0.8, 7
    g = torch.Generator().manual_seed(0)
    cols = torch.randperm(V, generator=g)[:12]
    vals = torch.tensor([4.0] + [3.5 - 0.25 * i for i in range(11)])
    row = torch.full((V,), -12.0)
    row[cols] = vals
    if mode == "rows":
        x = row.to(torch.bfloat16).repeat(N, 1).cuda()
        ids, kept, _, _ = C.sample_logits(x, V, T, 12, 1.0, seed, torch.zeros(N, dtype=torch.int64).cuda())
        ids = ids.cpu()
        assert bool((kept == 12).all())
    else:
        x = row.view(1, V).cuda()
        pos = torch.arange(N, dtype=torch.int64).cuda()
        ids = torch.cat([C.sample_logits(x, V, T, 12, 1.0, seed, pos[i:i + 1])[0] for i in range(N)]).cpu()
    prob = torch.softmax(vals.double() / T, 0)
    counts = torch.stack([(ids == c).sum() for c in cols]).double()
    assert int(counts.sum()) == N                                      # only the 12 survivors are drawn
    expect = N * prob
    assert float(expect.min()) > 60
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    df = 11
    zq = statistics.NormalDist().inv_cdf(1 - 1e-6)
    crit = df * (1 - 2 / (9 * df) + zq * (2 / (9 * df)) ** 0.5) ** 3
    assert 49 < crit < 51
    assert chi2 < crit, chi2


@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29567")
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    yield
    destroy_dist_env()


def test_sampled_generate_graph_matches_eager(dist1, monkeypatch):
    """Sampled decoding gives the same tokens on the eager step and on the captured 8-step
    graphs (the draw is a function of seed, row and position alone); a second call reuses the
    session's graphs; greedy decoding before and after is unchanged and has its own graphs."""
    from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
    from distributed_pytorch_from_scratch_amd.models import generation as G
    args = get_preset("gpt2-small", num_layers=2)
    m = Transformer.from_args(args).cuda()
    m.reset_parameters()
    m.eval()
    prompt = torch.randint(0, args.vocab_size, (3, 240), device="cuda")
    s = dict(temperature=0.8, top_k=40, top_p=0.95, seed=3)
    G.clear_sessions()
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    greedy = G.generate(m, prompt, max_new_tokens=40)
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    eager = G.generate(m, prompt, max_new_tokens=40, **s)
    assert G.generate(m, prompt, max_new_tokens=40) == greedy
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    graph = G.generate(m, prompt, max_new_tokens=40, **s)
    assert graph == eager and graph != greedy
    assert all(len(o) == 280 and all(0 <= t < args.vocab_size for t in o) for o in graph)
    (sess,) = G._SESSIONS.values()
    held = dict(sess["graphs"])
    assert sorted(map(str, held)) == sorted(map(str, [1, 8, (1, (0.8, 40, 0.95, 3)), (8, (0.8, 40, 0.95, 3))]))
    assert G.generate(m, prompt, max_new_tokens=40, **s) == graph
    (sess2,) = G._SESSIONS.values()
    assert sess2["graphs"] is sess["graphs"] and all(sess2["graphs"][k] is v for k, v in held.items())
    assert len(sess2["graphs"]) == len(held)
    assert G.generate(m, prompt, max_new_tokens=40, **{**s, "seed": 4}) != graph
    assert G.generate(m, prompt, max_new_tokens=40) == greedy
    assert G.generate(m, prompt, max_new_tokens=40, temperature=0, top_k=40, top_p=0.95, seed=3) == greedy
    G.clear_sessions()
