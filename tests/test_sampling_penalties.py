"""Repetition / presence / frequency penalties and log-probabilities on the CPU: the oracle
``ops/reference.sample_logits_pen`` (the contract of the ``PEN`` kernel and the CPU compute path),
an fp32 emulation of the kernel's log-probability arithmetic with planted faults, and
``generate()`` with penalties and ``return_logprobs`` on the uniform and the ragged path.

The bound of the emulation is the one of tests/test_sampling_penalties_gpu.py (derived there)."""
import math

import pytest
import torch

from dist_helpers import run_distributed

from distributed_pytorch_from_scratch_amd.ops import reference as R

V, LD = 200, 208
FLAG = -2 ** 31


def _table(temps, ks, ps, seeds, rids):
    inv_t = torch.tensor([1.0 / t if t > 0 else 0.0 for t in temps], dtype=torch.float64).float()
    return (inv_t, torch.tensor(ks, dtype=torch.int32), torch.tensor(ps, dtype=torch.float64),
            torch.tensor(seeds, dtype=torch.int64), torch.tensor(rids, dtype=torch.int32))


def _pens(reps, pres, freq):
    r = torch.tensor(reps, dtype=torch.float64)
    return (r.float(), (1.0 / r).float(), torch.tensor(pres, dtype=torch.float32),
            torch.tensor(freq, dtype=torch.float32))


def _logits(B, seed=0):
    x = (torch.randn(B, LD, generator=torch.Generator().manual_seed(seed)) * 4).bfloat16().float()
    x[:, V:] = 30.0                                     # padding columns hold the largest values
    return x


def _hist(B, seed=0, flags=30, counts=40):
    g = torch.Generator().manual_seed(50 + seed)
    h = torch.zeros(B, LD, dtype=torch.int32)
    for b in range(B):
        h[b, torch.randperm(V, generator=g)[:counts]] = torch.randint(1, 6, (counts,), generator=g, dtype=torch.int32)
        h[b, torch.randperm(V, generator=g)[:flags]] |= FLAG
    return h


def test_oracle_neutral_penalties_are_the_rows_form():
    B = 6
    x, h = _logits(B), _hist(B)
    tab = _table([0.8, 0, 1.3, 0.5, 1.0, 1.7], [40, 3, 0, 1, 300, 50], [0.95, 0.5, 1.0, 1.0, 0.9, 0.9],
                 [3, 4, 5, 6, 7, 8], [0, 1, 2, 0, 0, 5])
    pos = torch.arange(B, dtype=torch.int64) * 977 + 2 ** 33
    want = R.sample_logits_rows(x, V, *tab, pos)
    before = h.clone()
    got = R.sample_logits_pen(x, V, *tab, *_pens([1.0] * B, [0.0] * B, [0.0] * B), h, pos, None, False)
    assert len(got) == 6 and got[4].shape == (B, 2) and got[4].dtype == torch.float32
    assert all(torch.equal(g, w) for g, w in zip(got[:4], want))
    assert got[5] is h and torch.equal(h, before)            # update=False leaves the table
    assert R._sample_logits_pen is R.sample_logits_pen


def test_oracle_penalised_logit():
    """The prompt flag triggers repetition only; presence and frequency need c > 0; a positive
    logit takes inv_rep, a negative one (and zero) rep; one rounded fp32 operation each."""
    x = torch.tensor([[2.5, -2.5, 2.5, -2.5, 2.5, -2.5, 0.0, 3.25]])
    h = torch.tensor([[FLAG, FLAG, 3, 3, FLAG | 2, FLAG | 2, FLAG, 0]], dtype=torch.int32)
    rep, inv, pres, freq = _pens([1.3], [0.7], [0.4])
    got = R.penalised_logits(x, 8, rep, inv, pres, freq, h)[0]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    up, down = f(2.5) * inv[0], f(-2.5) * rep[0]
    want = [up, down,
            (up - freq[0] * f(3.0)) - pres[0], (down - freq[0] * f(3.0)) - pres[0],
            (up - freq[0] * f(2.0)) - pres[0], (down - freq[0] * f(2.0)) - pres[0],
            f(0.0) * rep[0], f(3.25)]
    assert got.tolist() == [float(w) for w in want]
    assert abs(float(got[0]) - 2.5 / 1.3) < 1e-6 and abs(float(got[1]) + 2.5 * 1.3) < 1e-6
    # negative penalties reward: the values move the other way
    rep, inv, pres, freq = _pens([0.8], [-0.5], [0.25])
    got = R.penalised_logits(x, 8, rep, inv, pres, freq, h)[0]
    assert got[0] > 2.5 and got[1] > -2.5 and got[7] == 3.25
    assert float(got[2]) == float((f(2.5) * inv[0] - freq[0] * f(3.0)) - pres[0])


def _fp64_rows(x, h, tab, pens, ids, thresh):
    """(log_softmax of the raw row at the id, log of the id's share of the kept mass), fp64."""
    xp = R.penalised_logits(x, V, *pens, h)
    lp0 = torch.log_softmax(x[:, :V].double(), -1).gather(-1, ids[:, None])[:, 0]
    z = (xp * tab[0][:, None]).double()
    w = torch.exp(z - z.max(-1, keepdim=True).values) * (xp >= thresh[:, None])
    lp1 = torch.log(w.gather(-1, ids[:, None])[:, 0] / w.sum(-1))
    return lp0, lp1


def test_oracle_logprobs():
    B = 5
    x, h = _logits(B, 1), _hist(B, 1)
    tab = _table([0.8, 0, 1.3, 0.5, 1.7], [40, 0, 0, 5, 0], [0.95, 1.0, 1.0, 1.0, 0.9], [3, 4, 5, 6, 7], [0] * B)
    pens = _pens([1.3, 1.3, 1.0, 0.8, 1.0], [0.0, 0.7, 0.7, -0.5, 0.0], [0.0, 0.0, 0.4, 0.25, 0.0])
    x[1, 7] = x[1, 9] = 50.0                             # a greedy row with two maxima (unseen ids)
    h[1, 7] = h[1, 9] = 0
    pos = torch.arange(B, dtype=torch.int64)
    ids, kept, thresh, u, logp, _ = R.sample_logits_pen(x, V, *tab, *pens, h, pos, None, False)
    lp0, lp1 = _fp64_rows(x, h, tab, pens, ids, thresh)
    assert torch.allclose(logp[:, 0].double(), lp0, rtol=2 ** -23, atol=0)
    assert torch.allclose(logp[:, 1].double(), lp1, rtol=2 ** -23, atol=1e-12)
    assert ids[1] == 7 and kept[1] == 2 and float(logp[1, 1]) == pytest.approx(-math.log(2.0), rel=1e-7)
    # kept / thresh are in units of the penalised logit
    xp = R.penalised_logits(x, V, *pens, h)
    assert torch.equal(kept.long(), (xp >= thresh[:, None]).sum(-1)) and bool((xp == thresh[:, None]).any(-1).all())
    assert kept[3] == 5 and kept[2] == V


def test_oracle_history_chain():
    """hist after K chained calls = the flags plus ``bincount`` of the ids drawn."""
    B, K_ = 4, 12
    x, h = _logits(B, 2), torch.zeros(B, LD, dtype=torch.int32)
    h[:, :40:3] = FLAG
    start = h.clone()
    tab = _table([0.8, 0, 1.3, 0], [5, 0, 3, 0], [1.0, 1.0, 1.0, 1.0], [3, 4, 5, 6], [0] * B)
    pens = _pens([1.0, 1.0, 1.2, 1.0], [0.0, 0.0, 0.5, 0.0], [0.0, 1e4, 0.3, 0.0])
    drawn = []
    for s in range(K_):
        out = R.sample_logits_pen(x, V, *tab, *pens, h, torch.full((B,), s, dtype=torch.int64))
        assert out[5] is h
        drawn.append(out[0])
    drawn = torch.stack(drawn, 1)
    for b in range(B):
        want = start[b].clone()
        want[:V] += torch.bincount(drawn[b], minlength=V).int()
        assert torch.equal(h[b], want)
    assert len(set(drawn[1].tolist())) == K_                # greedy under a huge frequency penalty: no repeats
    assert len(set(drawn[3].tolist())) == 1                 # the unpenalised greedy row repeats its maximum


# ------------------------------------------------------------------ the kernel's algorithm ----

def _unit(c, span, n, logp, w_id=None):
    """The bound of tests/test_sampling_penalties_gpu.py (derived in its docstring)."""
    unit = c * (span * 2.0 ** -23 + 2.0 ** -22) + n * 2.0 ** -40 + 2.0 ** -24 * abs(logp) + 2.0 ** -50
    unit += c * span * 2.0 ** -26                            # fp32(log2 e)
    if w_id is not None:        # the sampled value: the id's own truncated weight under the logarithm
        t = 2.0 ** -40 / w_id
        unit += -math.log1p(-t) if t < 1 else math.inf
    return unit


def _emulate(x, h, tab, pens, u, fault=None):
    """One launch as the kernel computes it, in fp32 with truncated 2^40 weights and integer
    sums, filters off; ``fault`` plants one of the mistakes the tests must catch."""
    f32 = torch.float32
    inv_t = tab[0]
    rep, inv, pres, freq = (t[:, None] for t in pens)
    lg = x[:, :V].to(f32)
    hw = h[:, :V]
    c = hw & 0x7FFFFFFF
    cf = c + (hw < 0).int() if fault == "prompt_in_frequency" else c
    cp = (hw != 0) if fault == "presence_on_flag" else (c > 0)

    def pen(v):
        v = torch.where(hw != 0, torch.where(v > 0, v * inv, v * rep), v)
        v = v - freq * cf.to(f32)
        return torch.where(cp, v - pres, v)

    if fault == "penalty_after_temperature":
        z = pen(lg * inv_t[:, None])
        xp = z
    else:
        xp = pen(lg)
        z = xp * inv_t[:, None]
    greedy = inv_t == 0
    zmax = z.max(-1, keepdim=True).values
    keep = torch.where(greedy[:, None], xp == xp.max(-1, keepdim=True).values, torch.ones_like(xp, dtype=torch.bool))
    m = (torch.exp(z - zmax) * 2.0 ** 40).to(torch.int64) * keep
    lmax = (xp if fault == "penalised_max" else lg).max(-1, keepdim=True).values
    S1 = (torch.exp(lg - lmax) * 2.0 ** 40).to(torch.int64).sum(-1)
    M = m.sum(-1)
    uu = torch.where(greedy, torch.zeros_like(u), u)
    need = (uu.double() * M.double()).to(torch.int64).clamp(max=M - 1) + 1
    ids = (m.cumsum(-1) >= need[:, None]).to(torch.int8).argmax(-1)
    at = ids[:, None]
    lp0 = (lg.gather(-1, at) - lmax)[:, 0].double() - torch.log(S1.double() * 2.0 ** -40)
    lp1 = torch.log(m.gather(-1, at)[:, 0].double()) - torch.log(M.double())
    if fault != "no_update":
        h[torch.arange(x.size(0)), ids] += 1
    return ids, torch.stack([lp0, lp1], -1).float()


def _chain(fault):
    """Three chained launches, emulation against oracle: True when every id, the history and
    every log-probability (under the bound) agree."""
    B, steps = 4, 3
    x = _logits(B, 4)
    x[:, 11] = 21.0                                      # the raw maximum of every row: a flagged id
    h = torch.zeros(B, LD, dtype=torch.int32)
    h[:, 3:120:4] = FLAG                                 # 30 prompt ids, column 11 among them
    h[:, 5:60:5] += 2
    tab = _table([0.7, 0, 1.6, 0], [0] * B, [1.0] * B, [0] * B, [0] * B)
    # (row 3 rewards its drawn ids by 40: the penalised maximum lies far above the raw one, where
    # the raw row's 2^40 weights all truncate to 0 if they are taken against it)
    pens = _pens([1.3, 1.3, 0.8, 1.0], [0.7, 0.7, -0.5, -40.0], [0.4, 1e4, 0.25, 0.0])
    ho, he = h.clone(), h.clone()
    ok = True
    for s in range(steps):
        u = torch.rand(B, generator=torch.Generator().manual_seed(70 + s))
        pos = torch.full((B,), s, dtype=torch.int64)
        xp = R.penalised_logits(x, V, *pens, ho)
        ids, _, thresh, _, _, _ = R.sample_logits_pen(x, V, *tab, *pens, ho, pos, u)
        logp = R.sample_logprobs_fp64(x, V, xp, tab[0], thresh, ids)
        ids_e, logp_e = _emulate(x, he, tab, pens, u, fault)
        ok = ok and torch.equal(ids, ids_e) and torch.equal(ho, he)
        for b in range(B):
            for j, z in enumerate((x[b, :V].double(), (xp[b] * tab[0][b]).double())):
                d = (z - z.max()).abs()
                span = float(d[torch.exp(-d) * 2.0 ** 40 >= 1].max())
                w_id = float(torch.exp(-d[ids[b]])) if j == 1 else None
                err = abs(float(logp_e[b, j]) - float(logp[b, j]))
                ok = ok and err <= 1.01 * _unit(j + 1, span, V, float(logp[b, j]), w_id)
    return ok


def test_kernel_algorithm_emulation_stays_in_bound():
    assert _chain(None)


@pytest.mark.parametrize("fault", ["prompt_in_frequency", "penalty_after_temperature", "penalised_max", "no_update",
                                   "presence_on_flag"])
def test_kernel_algorithm_planted_faults_are_caught(fault):
    assert not _chain(fault)


# --------------------------------------------------------------------------- generate() ----

def _generate(rank, world):
    from distributed_pytorch_from_scratch_amd.models import Transformer, get_preset
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    args = get_preset("plumbing")
    m = Transformer.from_args(args)
    set_seed(0)
    m.reset_parameters()
    m.eval()
    vocab = m.vocab_size
    B, N, T0 = 3, 12, 9
    prompt = torch.randint(3, vocab, (B, T0), generator=torch.Generator().manual_seed(5))
    gen = lambda *a, **kw: G.generate(m, prompt, N, *a, **kw)
    out = {"vocab": vocab, "T0": T0, "N": N}
    s = dict(temperature=[0.8, 0, 1.3], top_k=[20, 0, 0], top_p=[0.9, 1.0, 1.0], seed=[5, 6, 7])
    pen = dict(repetition_penalty=[1.3, 1.2, 1.0], presence_penalty=[0.0, 0.5, 0.7], frequency_penalty=[0.0, 0.3, 0.4])
    out["pen"], out["pen_lp"] = gen(**s, **pen, return_logprobs=True)
    out["pen_tokens_only"] = gen(**s, **pen)

    # the same by hand: logits_step + the oracle
    attn0 = m.layers[0].attn
    dev = prompt.device
    cache = G.KVCache(len(m.layers), B, T0 + N, attn0.num_local_heads, attn0.head_dim, m.act_dtype(dev), dev)
    tab = _table(s["temperature"], s["top_k"], s["top_p"], s["seed"], [0] * B)
    pens = _pens(pen["repetition_penalty"], pen["presence_penalty"], pen["frequency_penalty"])
    hist = torch.zeros(B, vocab, dtype=torch.int32)
    hist.scatter_(1, prompt, FLAG)
    toks, lps = [], []
    ids = prompt
    for step in range(N):
        logits = G.logits_step(m, ids, cache)
        pos = torch.full((B,), T0 - 1 + step, dtype=torch.int64)
        nxt, _, _, _, lp, _ = R.sample_logits_pen(logits, vocab, *tab, *pens, hist, pos)
        toks.append(nxt.tolist())
        lps.append(lp.tolist())
        ids = nxt.view(B, 1)
    out["hand"] = [prompt[b].tolist() + [t[b] for t in toks] for b in range(B)]
    out["hand_lp"] = [[tuple(l[b]) for l in lps] for b in range(B)]
    out["hand_hist_counts"] = (hist & 0x7FFFFFFF).sum(-1).tolist()

    out["plain"] = gen(**s)
    out["lp_only"], out["lp_only_lp"] = gen(**s, return_logprobs=True)
    out["greedy"] = gen()
    out["greedy_lp"] = gen(return_logprobs=True)
    out["no_repeat"] = gen(frequency_penalty=1e4)
    out["scalar_pen"] = gen(temperature=0.8, top_k=20, seed=11, repetition_penalty=1.2, presence_penalty=0.1)
    out["scalar_pen_lists"] = gen(temperature=[0.8] * B, top_k=20, seed=11, repetition_penalty=[1.2] * B,
                                  presence_penalty=(0.1,) * B, frequency_penalty=torch.zeros(B))
    out["mixed"] = gen(**s, repetition_penalty=[1.0, 1.0, 1.5], presence_penalty=[0.0, 0.0, 0.7])

    # ragged: only the real ids of a row are flagged, whatever the padding holds
    lens = [9, 4, 1]
    out["lens"] = lens
    flags = G.SamplePen(B, vocab, dev).load_history(prompt, lens).hist
    out["flags_ok"] = all(sorted(torch.nonzero(flags[b])[:, 0].tolist()) == sorted(set(prompt[b, :n].tolist()))
                          for b, n in enumerate(lens)) and bool(((flags == 0) | (flags == FLAG)).all())
    other = prompt.clone()
    for b, n in enumerate(lens):
        other[b, n:] = torch.randint(3, vocab, (T0 - n,), generator=torch.Generator().manual_seed(b))
    rp = dict(repetition_penalty=3.0, presence_penalty=0.5)
    out["r_pen"], out["r_pen_lp"] = gen(prompt_lens=lens, return_logprobs=True, **s, **rp)
    out["r_pen_other_padding"] = G.generate(m, other, N, prompt_lens=lens, **s, **rp)
    out["r_plain"] = gen(prompt_lens=lens, **s)

    # a row that stops at EOS: one pair per id it kept
    eos = out["pen"][1][T0 + 3]
    out["eos"] = eos
    out["eos_out"], out["eos_lp"] = gen(**s, **pen, return_logprobs=True, eos_id=eos)
    out["empty"] = G.generate(m, prompt, 0, return_logprobs=True)

    errors = []
    inf, nan = float("inf"), float("nan")
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=inf),
                dict(repetition_penalty=nan), dict(repetition_penalty=[1.0, 1.0]), dict(repetition_penalty=[1.0, 0.0, 1.0]),
                dict(repetition_penalty=1e-46), dict(repetition_penalty=1e46),     # fp32(1 / r) inf / 0
                dict(presence_penalty=inf), dict(presence_penalty=[0.0, nan, 0.0]), dict(presence_penalty=[0.1] * 4),
                dict(frequency_penalty=-inf), dict(frequency_penalty=[0.0, 0.0, nan]), dict(frequency_penalty=[0.1]),
                dict(frequency_penalty=[0.1, 0.2], prompt_lens=lens),
                dict(temperature=[0.8, 0.8], return_logprobs=True), dict(temperature=-1.0, return_logprobs=True),
                dict(top_p=0.0, presence_penalty=0.5)):
        try:
            gen(**bad)
            errors.append((str(bad), "no error"))
        except ValueError:
            pass
    out["errors"] = errors
    return out


@pytest.fixture(scope="module")
def gen1():
    return run_distributed(_generate, 1)[0]


def test_generate_matches_a_hand_rolled_loop(gen1):
    """``generate`` with penalties = ``logits_step`` plus the oracle step by step: the first token
    is penalised by the prompt flags and counted, the draws are keyed on (seed, 0, position)."""
    assert gen1["pen"] == gen1["hand"]
    assert gen1["pen_lp"] == gen1["hand_lp"]
    assert gen1["pen_tokens_only"] == gen1["pen"]
    assert gen1["hand_hist_counts"] == [gen1["N"]] * 3
    assert gen1["pen"] != gen1["plain"]


def test_generate_logprobs_alone_change_no_token(gen1):
    assert gen1["lp_only"] == gen1["plain"]
    assert gen1["greedy_lp"][0] == gen1["greedy"]
    n = gen1["N"]
    assert all(len(r) == n and all(len(p) == 2 for p in r) for r in gen1["lp_only_lp"])
    assert all(a <= 0 and b <= 0 for r in gen1["lp_only_lp"] for a, b in r)
    assert all(b == 0.0 for b in (p[1] for p in gen1["greedy_lp"][1][0]))      # a unique maximum: log 1
    # row 2 samples at T = 1.3 without filters: the drawn distribution is not the model's
    assert any(a != b for a, b in gen1["lp_only_lp"][2])


def test_generate_frequency_penalty_forbids_repeats(gen1):
    t0 = gen1["T0"]
    for row, plain in zip(gen1["no_repeat"], gen1["greedy"]):
        new = row[t0:]
        assert len(new) == gen1["N"] and len(set(new)) == len(new)
        assert new[0] == plain[t0]                          # nothing drawn yet: the first token is greedy's


def test_generate_rows_mix_neutral_and_penalised(gen1):
    assert gen1["mixed"][0] == gen1["plain"][0] and gen1["mixed"][1] == gen1["plain"][1]
    assert gen1["mixed"][2] != gen1["plain"][2]
    assert gen1["scalar_pen"] == gen1["scalar_pen_lists"]


def test_generate_ragged(gen1):
    lens, n = gen1["lens"], gen1["N"]
    assert gen1["flags_ok"]
    assert gen1["r_pen"] == gen1["r_pen_other_padding"]
    assert gen1["r_pen"] != gen1["r_plain"]
    assert [len(o) for o in gen1["r_pen"]] == [m + n for m in lens]
    assert all(len(r) == n for r in gen1["r_pen_lp"])


def test_generate_logprobs_of_a_row_that_stops(gen1):
    t0, eos = gen1["T0"], gen1["eos"]
    out, lp = gen1["eos_out"], gen1["eos_lp"]
    assert out[1] == gen1["pen"][1][:len(out[1])] and out[1][-1] == eos and len(out[1]) < t0 + gen1["N"]
    assert [len(r) for r in lp] == [len(o) - t0 for o in out]
    assert lp[1] == gen1["pen_lp"][1][:len(lp[1])]
    assert gen1["empty"] == ([o[:t0] for o in gen1["pen"]], [[], [], []])


def test_generate_errors(gen1):
    assert gen1["errors"] == []
