"""``_sample_logits_pen`` (csrc/kernels/sample.hip, the ``PEN`` form: penalised logits, device
token history, two log-probabilities per row) on the MI355X.

**Selection: no tolerance.**  With ``update=False`` the launch must equal ``_sample_logits_rows``
on the fp32 row penalised on the host by the oracle's fp32 operations
(``reference.penalised_logits``) in ``ids``, ``kept``, ``thresh`` and ``u`` exactly: both kernels
then run the same integer sums on the same fp32 values.

**Log-probabilities: a derived cap.**  Per row |kernel - fp64 oracle| <= 1.01 unit,

    unit = c (span 2^-23 + 2^-22) + V 2^-40 + 2^-24 |logp| + 2^-50   [+ the two terms below]

with the terms of tests/test_sampling_rows_gpu.py, here for a logarithm of a sum of weights
instead of a share of it (d log S = dS / S, so relative errors of the sum are absolute errors of
the result):

* the exponent: the kernel forms a = z - max z in fp32 (relative 2^-24 of |a|; the oracle's
  difference is exact in fp64) and multiplies it by log2(e) in fp32 before the hardware exp2
  (another 2^-24 |a|): span 2^-23 per weight, and so per sum of weights; span is the row's
  largest |z - max z| among the weights that do not truncate to 0 (|a| <= 40 ln 2);
* the hardware exp2: 2^-22 relative per weight;
* c: the model value log(exp(l_id - l_max) / S1) has the id's term exactly (one fp32 subtract,
  covered by the rounding term below, and a logarithm that is never taken), so only S1 errs:
  c = 1; the sampled value log(m_id / M) is a ratio of two such quantities: c = 2;
* the 2^40 fixed point: every weight is truncated by < 2^-40 of the maximum's weight, V 2^-40 of
  a sum that holds the maximum (S1 always; M too, the maximum is always kept);
* the result's rounding to fp32: 2^-24 |logp| (the oracle's figure is taken in fp64, before its
  own rounding: ``reference.sample_logprobs_fp64``);
* the fp64 logarithms and the fp64 subtraction: 2^-50.

Two terms the list above lacks, added here with their derivation rather than by a wider factor:

* log2(e) itself is an fp32 constant in the kernel's exponential: |fp32(log2 e) / log2 e - 1| =
  1.34e-8 < 2^-26, an error of |a| 2^-26 in every exponent: c span 2^-26;
* the sampled value takes the logarithm of the id's own truncated weight m_id, whose truncation
  (< 1 in units of 2^-40) is relative to m_id, not to a sum that holds the maximum: with t =
  2^-40 / w_id, w_id = exp(z_id - max z), the logarithm moves by at most log(m / (m - 1)) =
  -log(1 - t) (not linearised: an id may be drawn at a weight of a few units; t >= 1 bounds
  nothing).  The other terms come to about 7e-6, so this one leads the cap once the id drawn
  weighs less than about 2^-23 of the maximum (a supplied u = 0 under top-k draws such ids).

What the kernel reaches is recorded in profiles/kernel_error_bounds.txt.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FLAG = -2 ** 31

# rows, valid vocab, row stride, dtype: the smallest shapes that reach each code path
SHAPES = {
    "bf16_5": (1, 5, 8, torch.bfloat16),                   # less than one vector
    "fp32_96": (2, 96, 96, torch.float32),
    "bf16_1000": (4, 1000, 1024, torch.bfloat16),
    "bf16_1003": (3, 1003, 1003, torch.bfloat16),          # unaligned rows: scalar loads
    "bf16_8200": (2, 8200, 8200, torch.bfloat16),          # past 16 waves x 64 lanes x 8: a second vector per lane
    "fp32_4099": (33, 4099, 4104, torch.float32),
    "bf16_50257": (2, 50257, 50304, torch.bfloat16),       # the full vocabulary, once
}
SMALL = [s for s in SHAPES if s != "bf16_50257"]
# (temperature, top_k, top_p): greedy, sampled unfiltered, k50, p0.9, k50_p0.9
KINDS = ((0.0, 0, 1.0), (1.7, 0, 1.0), (0.5, 50, 1.0), (1.0, 0, 0.9), (0.8, 50, 0.9))
# (repetition, presence, frequency)
PENS = ((1.3, 0.0, 0.0), (1.0, 0.7, 0.4), (0.8, -0.5, 0.25), (1.0, 0.0, 0.0))
COMBOS = [(KINDS[i % 5], PENS[(i + i // 5) % 4]) for i in range(20)]      # every kind with every penalty


@pytest.fixture(scope="module")
def C():
    from distributed_pytorch_from_scratch_amd.ops import _ext
    return _ext.require()


@pytest.fixture(scope="module")
def R():
    from distributed_pytorch_from_scratch_amd.ops import reference
    return reference


def _ld_h(V, aligned):
    """An aligned history stride (whole 16-byte vectors past V), or ld_h = V made odd."""
    return (V + 7) // 8 * 8 if aligned else V | 1


def _history(B, V, ld_h, x, g):
    """A few hundred random counts in 0..5 plus random prompt flags per row; the row maximum is a
    flagged id; in the last row every id is seen."""
    h = torch.zeros(B, ld_h, dtype=torch.int32)
    n = min(V, 300)
    for b in range(B):
        h[b, torch.randperm(V, generator=g)[:n]] = torch.randint(0, 6, (n,), generator=g, dtype=torch.int32)
        h[b, torch.randperm(V, generator=g)[:max(n // 2, 1)]] |= FLAG
        h[b, x[b, :V].float().argmax()] |= FLAG
    h[B - 1, :V] |= FLAG
    h[:, V:] = 7                                            # padding words: never read as history
    return h


@pytest.fixture(scope="module")
def rows():
    """Per shape: the logits in their dtype (``randn * 4``: the bf16 rows tie; the padding
    columns hold the largest values of the row), the uniforms, and the history at an aligned
    and at an odd stride (the same words)."""
    out = {}
    for i, (name, (B, V, ld, dt)) in enumerate(SHAPES.items()):
        g = torch.Generator().manual_seed(300 + i)
        x = (torch.randn(B, ld, generator=g) * 4).to(dt)
        x[:, V:] = 30.0
        u = torch.rand(B, generator=g)
        u[0] = 0.0
        ha = _history(B, V, _ld_h(V, True), x, g)
        ho = torch.full((B, _ld_h(V, False)), 7, dtype=torch.int32)
        ho[:, :V] = ha[:, :V]
        out[name] = (x, u, {True: ha, False: ho})
    return out


def _table(temps, ks, ps, seeds, rids):
    inv_t = torch.tensor([1.0 / t if t > 0 else 0.0 for t in temps], dtype=torch.float64).float()
    return (inv_t, torch.tensor(ks, dtype=torch.int32), torch.tensor(ps, dtype=torch.float64),
            torch.tensor(seeds, dtype=torch.int64), torch.tensor(rids, dtype=torch.int32))


def _pens(combo):
    r = torch.tensor([p[0] for _, p in combo], dtype=torch.float64)
    return (r.float(), (1.0 / r).float(), torch.tensor([p[1] for _, p in combo], dtype=torch.float32),
            torch.tensor([p[2] for _, p in combo], dtype=torch.float32))


def _launches(B, once=False):
    """Settings of the B rows for as many launches as it takes to give every (kind, penalty) of
    COMBOS to some row; ``once``: the first launch, shifted so that two rows filter and sample."""
    if once:
        return [[COMBOS[(4 + 2 * b) % 20] for b in range(B)]]
    return [[COMBOS[(start + b) % 20] for b in range(B)] for start in range(0, 20, B)]


def _settings(combo, n=0):
    B = len(combo)
    temps, ks, ps = (list(c) for c in zip(*(k for k, _ in combo)))
    return _table(temps, ks, ps, [1234 + 7 * b + 100 * n for b in range(B)], [0] * B), _pens(combo)


def _cuda(ts):
    return [t.cuda() for t in ts]


def _pen(C, x, V, tab, pens, hist_c, pos, u=None, update=False):
    B = x.size(0)
    got = C._sample_logits_pen(x.cuda(), V, *_cuda(tab), *_cuda(pens), hist_c, pos.cuda(),
                               None if u is None else u.cuda(), update)
    torch.cuda.synchronize()
    ids, kept, thresh, uo, logp = got
    assert ids.dtype == torch.int64 and kept.dtype == torch.int32 and thresh.dtype == uo.dtype == torch.float32
    assert logp.dtype == torch.float32 and logp.shape == (B, 2) and all(t.shape == (B,) for t in got[:4])
    return tuple(t.cpu() for t in got)


def _positions(B):
    pos = torch.arange(B, dtype=torch.int64) * 977 + 3
    pos[-1] = 2 ** 33 + 5
    return pos


@pytest.mark.parametrize("aligned", [True, False], ids=["ldh_aligned", "ldh_odd"])
@pytest.mark.parametrize("shape", SMALL)
def test_pen_matches_the_rows_kernel_on_penalised_logits(C, R, rows, shape, aligned):
    """The main check: all four selection outputs, bit for bit, for every (kind, penalty)."""
    B, V, _, _ = SHAPES[shape]
    x, u, hists = rows[shape]
    hist = hists[aligned]
    hc = hist.cuda()
    pos = _positions(B)
    for n, combo in enumerate(_launches(B)):
        tab, pens = _settings(combo, n)
        x_pen = R.penalised_logits(x, V, *pens, hist)
        for uu in (None, u):
            got = _pen(C, x, V, tab, pens, hc, pos, uu)
            want = C._sample_logits_rows(x_pen.cuda(), V, *_cuda(tab), pos.cuda(), None if uu is None else uu.cuda())
            for g, w, name in zip(got, want, ("ids", "kept", "thresh", "u")):
                assert torch.equal(g, w.cpu()), (name, combo)
    assert torch.equal(hc.cpu(), hist)                       # update=False writes nothing


@pytest.mark.parametrize("pen", [(1.3, 0.7, 0.4), (1.1, 0.3, 0.7)], ids=["r1.3_p0.7_f0.4", "r1.1_p0.3_f0.7"])
@pytest.mark.parametrize("dt,V,ld,ld_h", [(torch.float32, 96, 96, 97), (torch.bfloat16, 203, 208, 208),
                                          (torch.bfloat16, 203, 203, 203)], ids=["fp32_96", "bf16_203", "bf16_203_scalar"])
def test_every_penalised_value_is_the_oracles(C, R, dt, V, ld, ld_h, pen):
    """The penalised value of every column, exactly.  The selection outputs show the penalised row
    only at the threshold and at the crossing, so here one row is sampled V times in one launch
    with top_k = 1 .. V: ``thresh[k - 1]`` is the k-th largest penalised value, ``kept`` its rank
    with ties, and together they are the whole sorted row.  Every id has been drawn 3 or 5 times
    and the frequency penalties are 0.4 and 0.7, so every product freq * fp32(c) is inexact, as
    are the repetition products: a multiply fused into the subtract that follows it (one rounding
    instead of two) moves about a tenth of the columns by an ulp and fails this test."""
    g = torch.Generator().manual_seed(11)
    row = (torch.randn(ld, generator=g) * 4).to(dt)
    row[V:] = 30.0
    x = row.repeat(V, 1).contiguous()
    h = torch.full((ld_h,), 7, dtype=torch.int32)
    h[:V] = torch.where(torch.rand(V, generator=g) < 0.5, 3, 5).int()
    h[:V][torch.rand(V, generator=g) < 0.5] |= FLAG
    hist = h.repeat(V, 1).contiguous()
    tab = _table([1.0] * V, list(range(1, V + 1)), [1.0] * V, [0] * V, [0] * V)
    pens = _pens([((1.0, 0, 1.0), pen)] * V)
    x_pen = R.penalised_logits(x, V, *pens, hist)
    # the inputs do what the docstring says: the two-step value differs from the fused one somewhere
    c = (hist[0, :V] & 0x7FFFFFFF).double()
    seen = torch.where(x[0, :V].float() > 0, x[0, :V].float() * pens[1][0], x[0, :V].float() * pens[0][0])
    fused = (seen.double() - pens[3][0].double() * c).float() - pens[2][0]
    assert int((fused != x_pen[0]).sum()) >= V // 20
    got = _pen(C, x, V, tab, pens, hist.cuda(), torch.zeros(V, dtype=torch.int64))
    want = x_pen[0].sort(descending=True).values
    assert torch.equal(got[2], want), int((got[2] != want).sum())
    assert torch.equal(got[1].long(), (x_pen[0][None, :] >= want[:, None]).sum(-1))


def test_pen_full_vocabulary_once(C, R, rows):
    """50,257 columns: selection bit for bit and the log-probabilities under the cap, one launch."""
    shape = "bf16_50257"
    B, V, _, _ = SHAPES[shape]
    x, u, hists = rows[shape]
    (combo,) = _launches(B, once=True)
    tab, pens = _settings(combo)
    pos = _positions(B)
    x_pen = R.penalised_logits(x, V, *pens, hists[True])
    got = _pen(C, x, V, tab, pens, hists[True].cuda(), pos, u)
    want = C._sample_logits_rows(x_pen.cuda(), V, *_cuda(tab), pos.cuda(), u.cuda())
    assert all(torch.equal(g, w.cpu()) for g, w in zip(got, want))
    _check_logp(R, shape, x, V, x_pen, tab, got)


@pytest.mark.parametrize("shape", [s for s in SMALL if SHAPES[s][3] == torch.bfloat16])
def test_neutral_penalties_on_bf16_are_the_rows_kernel(C, rows, shape):
    """Neutral penalties, bf16 storage, any history: ``_sample_logits_rows`` on the stored row
    (2 radix rounds on bf16 keys there, 4 on fp32 keys here: the same choice)."""
    B, V, _, _ = SHAPES[shape]
    x, u, hists = rows[shape]
    pos = _positions(B)
    for n, combo in enumerate(_launches(B)):
        combo = [(k, PENS[3]) for k, _ in combo]
        tab, pens = _settings(combo, n)
        got = _pen(C, x, V, tab, pens, hists[True].cuda(), pos)
        want = C._sample_logits_rows(x.cuda(), V, *_cuda(tab), pos.cuda())
        assert all(torch.equal(g, w.cpu()) for g, w in zip(got, want)), combo


@pytest.mark.parametrize("aligned", [True, False], ids=["ldh_aligned", "ldh_odd"])
@pytest.mark.parametrize("shape", SMALL)
def test_update_adds_one_at_the_id(C, rows, shape, aligned):
    """``update=True``: exactly one word per row changes, by +1, at ids[b]; the padding words and
    the sentinel rows in front of and behind the table are intact; the outputs are those of
    ``update=False``."""
    B, V, _, _ = SHAPES[shape]
    x, u, hists = rows[shape]
    hist = hists[aligned]
    ld_h = hist.size(1)
    buf = torch.full((B + 2, ld_h), 0x5A5A5A5A, dtype=torch.int32)
    buf[1:B + 1] = hist
    bc = buf.cuda()
    tab, pens = _settings(_launches(B)[0])
    pos = _positions(B)
    dry = _pen(C, x, V, tab, pens, bc[1:B + 1], pos, u, update=False)
    assert torch.equal(bc.cpu(), buf)
    got = _pen(C, x, V, tab, pens, bc[1:B + 1], pos, u, update=True)
    assert all(torch.equal(g, d) for g, d in zip(got, dry))
    want = buf.clone()
    want[torch.arange(B) + 1, got[0]] += 1
    assert torch.equal(bc.cpu(), want)
    # the flag bit survives the count
    assert bool(((bc.cpu()[1:B + 1, :V] < 0) == (hist[:, :V] < 0)).all())


@pytest.mark.parametrize("shape", ["fp32_96", "bf16_1000", "bf16_1003"])
def test_eight_chained_launches_follow_the_oracle(C, R, rows, shape):
    """Eight launches on one table (what one graph replay runs): the ids and the history equal
    the oracle's chain; the frequency-penalised greedy row never repeats an id."""
    B, V, _, _ = SHAPES[shape]
    x, _, hists = rows[shape]
    hist = hists[False].clone()
    hist[:, :V] &= FLAG                                     # flags only: counts start at 0
    hc = hist.cuda()
    combo = [(KINDS[(2 * b) % 5], (PENS + ((1.0, 0.0, 1e4),))[(b + 4) % 5]) for b in range(B)]   # row 0: greedy, freq 1e4
    tab, pens = _settings(combo)
    drawn = []
    for s in range(8):
        pos = torch.full((B,), 100 + s, dtype=torch.int64)
        ids = _pen(C, x, V, tab, pens, hc, pos, update=True)[0]
        want = R.sample_logits_pen(x, V, *tab, *pens, hist, pos)
        assert torch.equal(ids, want[0]), s
        assert torch.equal(hc.cpu(), hist), s
        drawn.append(ids)
    drawn = torch.stack(drawn, 1)
    assert len(set(drawn[0].tolist())) == min(8, V)
    assert torch.equal((hist[:, :V] & 0x7FFFFFFF).sum(-1), torch.full((B,), 8))


def _own_truncation(w_id: float) -> float:
    """-log(1 - t), t = 2^-40 / w_id: the id's own truncated weight under the logarithm."""
    t = 2.0 ** -40 / w_id
    return -math.log1p(-t) if t < 1 else math.inf


def _check_logp(R, name, x, V, x_pen, tab, got, record=None):
    """Both log-probabilities of every row against the fp64 oracle at the kernel's own ids and
    threshold (which the bit-for-bit tests pin), under the cap of the module docstring."""
    ids, _, thresh, _, logp = got
    want = R.sample_logprobs_fp64(x, V, x_pen, tab[0], thresh, ids)
    worst = 0.0
    for b in range(x.size(0)):
        for j, z in enumerate((x[b, :V].double(), (x_pen[b] * tab[0][b]).double())):
            c = j + 1
            d = (z - z.max()).abs()
            span = float(d[torch.exp(-d) * 2.0 ** 40 >= 1].max())
            lp = float(want[b, j])
            unit = c * (span * 2.0 ** -23 + 2.0 ** -22) + V * 2.0 ** -40 + 2.0 ** -24 * abs(lp) + 2.0 ** -50
            unit += c * span * 2.0 ** -26                                   # fp32(log2 e)
            if j == 1:
                unit += _own_truncation(float(torch.exp(-d[ids[b]])))
            worst = max(worst, abs(float(logp[b, j]) - lp) / unit)
    print(f"logp {name:<60} {worst:12.4g}")
    if record is not None:
        record.append(worst)
    assert worst <= 1.01, (name, worst)


@pytest.mark.parametrize("shape", SMALL)
def test_logprobs_against_the_fp64_oracle(C, R, rows, shape):
    B, V, _, _ = SHAPES[shape]
    x, u, hists = rows[shape]
    hist = hists[True]
    pos = _positions(B)
    for n, combo in enumerate(_launches(B)):
        tab, pens = _settings(combo, n)
        x_pen = R.penalised_logits(x, V, *pens, hist)
        got = _pen(C, x, V, tab, pens, hist.cuda(), pos, u)
        _check_logp(R, f"{shape} launch {n}", x, V, x_pen, tab, got)
        greedy = [b for b, (k, _) in enumerate(combo) if k[0] == 0]
        for b in greedy:      # -log(number of maxima), and the maximum is what was taken
            assert float(got[4][b, 1]) == pytest.approx(-float(torch.log(got[1][b].double())), abs=1e-7)
            assert got[0][b] == x_pen[b].argmax()


def test_argument_checks(C, rows):
    x, _, hists = rows["fp32_96"]
    xc, pos = x.cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    tab, pens = _settings(_launches(2)[0])
    good = _cuda(tab) + _cuda(pens)
    hc = hists[True].cuda()
    names = ("inv_t", "top_k", "top_p", "seed", "rid", "rep", "inv_rep", "pres", "freq")
    wrong = (torch.float64, torch.int64, torch.float32, torch.int32, torch.int64) + (torch.float64,) * 4
    assert len(C._sample_logits_pen(xc, 96, *good, hc, pos)) == 5
    for i, name in enumerate(names):
        for bad in (good[i].to(wrong[i]), torch.cat([good[i], good[i]]), good[i][:1], good[i].cpu()):
            args = list(good)
            args[i] = bad
            with pytest.raises(RuntimeError, match=name):
                C._sample_logits_pen(xc, 96, *args, hc, pos)
    for bad in (hc.long(), hc.cpu(), hc[:1], hc[:, :95], hc[:, :95].contiguous(), hc.t().contiguous().t(), hc[0]):
        with pytest.raises(RuntimeError, match="hist"):      # dtype, device, rows, ld_h < vocab, stride, rank
            C._sample_logits_pen(xc, 96, *good, bad, pos)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="hist"):
            C._sample_logits_pen(xc, 96, *good, hc.to("cuda:1"), pos)
    for V in (97, 0):
        with pytest.raises(RuntimeError, match="sample_logits_pen"):
            C._sample_logits_pen(xc, V, *good, hc, pos)
    with pytest.raises(RuntimeError, match="pos"):
        C._sample_logits_pen(xc, 96, *good, hc, pos.int())
    with pytest.raises(RuntimeError, match="u "):
        C._sample_logits_pen(xc, 96, *good, hc, pos, torch.zeros(3, device="cuda"))
    with pytest.raises(RuntimeError):
        C._sample_logits_pen(xc.half(), 96, *good, hc, pos)


def test_fp32_logits_reach_the_kernel(C, R, rows, monkeypatch):
    from distributed_pytorch_from_scratch_amd.ops import fp32_native, reference
    from distributed_pytorch_from_scratch_amd.ops.dispatch import K
    x, u, hists = rows["fp32_96"]
    xc = x.cuda()
    assert K(xc) is fp32_native
    tab, pens = _settings(_launches(2)[0])
    want = _pen(C, x, 96, tab, pens, hists[True].cuda(), torch.zeros(2, dtype=torch.int64), u)
    monkeypatch.setattr(reference, "sample_logits_pen", None)      # the oracle must not be what runs
    monkeypatch.setattr(reference, "_sample_logits_pen", None)
    got = K(xc)._sample_logits_pen(xc, 96, *_cuda(tab), *_cuda(pens), hists[True].cuda(),
                                   torch.zeros(2, dtype=torch.int64).cuda(), u.cuda(), False)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


# ------------------------------------------------------------------------- model level ----

@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
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
    prompt = torch.randint(0, args.vocab_size, (3, 24), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    return m, prompt


ROWS = dict(temperature=[0.8, 0, 1.3], top_k=[40, 0, 0], top_p=[0.95, 1.0, 0.9], seed=[3, 4, 5])
PEN_A = dict(repetition_penalty=[1.3, 1.2, 1.0], presence_penalty=[0.0, 0.5, 0.7], frequency_penalty=[0.0, 0.3, 0.4])
PEN_B = dict(repetition_penalty=0.8, presence_penalty=[-0.5, 0.0, 0.2], frequency_penalty=0.25)
N_NEW = 20      # 1 + 8 + 8 + 3 single steps: both graphs of the form replay


def test_generate_pen_graph_matches_eager_and_shares_two_graphs(model, monkeypatch):
    """Penalties and log-probabilities decode the same tokens and the same log-probabilities on
    the eager step and on the captured graphs; two calls with different penalties replay the
    same (1, "pen") and (8, "pen") graph objects; a penalty-free call afterwards returns the
    eager penalty-free tokens from graphs of its own."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, prompt = model
    gen = lambda **kw: G.generate(m, prompt, max_new_tokens=N_NEW, **kw)
    G.clear_sessions()
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    eager_a = gen(**ROWS, **PEN_A, return_logprobs=True)
    eager_b = gen(**ROWS, **PEN_B, return_logprobs=True)
    eager_plain = gen(**ROWS)
    eager_lp = gen(**ROWS, return_logprobs=True)
    assert not G._SESSIONS
    assert eager_lp[0] == eager_plain and eager_a[0] != eager_plain and eager_a[0] != eager_b[0]
    assert all(len(r) == N_NEW and all(a <= 0 and b <= 0 for a, b in r) for r in eager_a[1])
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    a = gen(**ROWS, **PEN_A, return_logprobs=True)
    assert a == eager_a
    (sess,) = G._SESSIONS.values()
    want_keys = sorted(map(str, [(1, "pen"), (8, "pen")]))
    assert sorted(map(str, sess["graphs"])) == want_keys
    held = dict(sess["graphs"])
    assert gen(**ROWS, **PEN_B, return_logprobs=True) == eager_b
    assert gen(**ROWS, **PEN_A) == eager_a[0]                               # tokens alone: the same path
    assert gen(**ROWS, return_logprobs=True) == eager_lp
    assert sorted(map(str, sess["graphs"])) == want_keys and all(sess["graphs"][k] is v for k, v in held.items())
    plain = gen(**ROWS)
    assert plain == eager_plain
    assert sorted(map(str, sess["graphs"])) == sorted(map(str, [(1, "pen"), (8, "pen"), (1, "rows"), (8, "rows")]))
    assert all(sess["graphs"][k] is v for k, v in held.items())
    assert gen(**ROWS, **PEN_A, return_logprobs=True) == eager_a            # and back: the history is reloaded
    G.clear_sessions()


def test_generate_pen_ragged_graph_matches_eager(model, monkeypatch):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, prompt = model
    lens = [24, 11, 3]
    gen = lambda **kw: G.generate(m, prompt, max_new_tokens=N_NEW, prompt_lens=lens, **kw)
    G.clear_sessions()
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    eager = gen(**ROWS, **PEN_A, return_logprobs=True)
    eager_plain = gen(**ROWS)
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    graph = gen(**ROWS, **PEN_A, return_logprobs=True)
    assert graph == eager and graph[0] != eager_plain
    assert [len(o) for o in graph[0]] == [n + N_NEW for n in lens] and all(len(r) == N_NEW for r in graph[1])
    (sess,) = G._SESSIONS.values()
    assert sorted(map(str, sess["graphs"])) == sorted(map(str, [(1, "pen"), (8, "pen")]))
    assert gen(**ROWS) == eager_plain
    G.clear_sessions()


def test_decode_step_model_logprob(model, R):
    """One eager ``decode_step`` with the table: ``logp[:, 0]`` against ``log_softmax`` of the
    fp32 logits the step returns, under the cap of the module docstring (c = 1)."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, prompt = model
    B, T0 = prompt.shape
    V = m.vocab_size
    attn0 = m.layers[0].attn
    dev = prompt.device
    with torch.inference_mode():
        cache = G.KVCache(len(m.layers), B, T0 + 4, attn0.num_local_heads, attn0.head_dim, m.act_dtype(dev), dev)
        first = G.logits_step(m, prompt, cache).argmax(-1)
        host = G._row_settings(B, ROWS["temperature"], ROWS["top_k"], ROWS["top_p"], ROWS["seed"]) + \
            G._penalty_settings(B, *PEN_A.values())
        table = cache.sample_pen(V).load(host).load_history(prompt)
        before = table.hist.clone()
        cache.sync_device_len()
        pos = cache.device_pos()
        nxt, logits = G.decode_step(m, first.view(B, 1), pos, cache, table)
        torch.cuda.synchronize()
    assert logits.dtype == torch.float32 and logits.shape == (B, V)
    change = (table.hist - before).cpu()
    assert torch.equal(change.nonzero(), torch.stack([torch.arange(B), nxt.cpu()], 1)) and bool((change.sum(-1) == 1).all())
    lg = logits.cpu()
    want = torch.log_softmax(lg.double(), -1).gather(-1, nxt.cpu()[:, None])[:, 0]
    worst = 0.0
    for b in range(B):
        d = (lg[b].double() - lg[b].double().max()).abs()
        span = float(d[torch.exp(-d) * 2.0 ** 40 >= 1].max())
        lp = float(want[b])
        unit = span * (2.0 ** -23 + 2.0 ** -26) + 2.0 ** -22 + V * 2.0 ** -40 + 2.0 ** -24 * abs(lp) + 2.0 ** -50
        worst = max(worst, abs(float(table.logp[b, 0]) - lp) / unit)
    print(f"logp {'decode_step gpt2-small 2 layers, model value':<60} {worst:12.4g}")
    assert worst <= 1.01, worst
