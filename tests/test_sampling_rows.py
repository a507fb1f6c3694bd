"""Per-row sampling settings on the CPU: the oracle ``ops/reference.sample_logits_rows`` (the
contract of the kernel and the CPU compute path), ``generate()`` with sequences of settings on
the uniform and the ragged path, and the ``--per_prompt_seed`` flag of the CLI."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from dist_helpers import _free_port, run_distributed

from distributed_pytorch_from_scratch_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (top_k, top_p) of a sampled row: off, k = 1, k >= vocab, p = 0.9, k = 50 with p = 0.9
FILTERS = ((0, 1.0), (1, 1.0), (300, 1.0), (0, 0.9), (50, 0.9))
TEMPS = (0.5, 1.0, 1.7)
V, LD = 200, 208


def _table(temps, ks, ps, seeds, rids):
    inv_t = torch.tensor([1.0 / t if t > 0 else 0.0 for t in temps], dtype=torch.float64).float()
    return (inv_t, torch.tensor(ks, dtype=torch.int32), torch.tensor(ps, dtype=torch.float64),
            torch.tensor(seeds, dtype=torch.int64), torch.tensor(rids, dtype=torch.int32))


def _logits(B, seed=0):
    x = (torch.randn(B, LD, generator=torch.Generator().manual_seed(seed)) * 4).bfloat16().float()
    x[:, V:] = 30.0                                     # padding columns hold the largest values
    return x


def test_oracle_sampled_rows_match_the_scalar_oracle():
    """Every sampled row equals ``sample_logits`` of that row alone with the row's scalars, in
    all four outputs; the uniform is that of (seed[b], pos[b], rid[b])."""
    rows = [(T, k, p) for T in TEMPS for k, p in FILTERS]
    B = len(rows)
    x = _logits(B)
    temps, ks, ps = (list(c) for c in zip(*rows))
    seeds = [7 + 13 * b for b in range(B)]
    seeds[1], seeds[2] = -5, 2 ** 62 + 3
    rids = [(3 * b) % 5 for b in range(B)]
    pos = torch.arange(B, dtype=torch.int64) * 977 + 2 ** 33
    got = R.sample_logits_rows(x, V, *_table(temps, ks, ps, seeds, rids), pos)
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.float32, torch.float32]
    assert all(t.shape == (B,) for t in got)
    for b, (T, k, p) in enumerate(rows):
        u = torch.tensor([R.sample_uniform(seeds[b], int(pos[b]), rids[b])], dtype=torch.float32)
        want = R.sample_logits(x[b:b + 1], V, T, k, p, 0, pos[b:b + 1], u)
        for g, w in zip(got, want):
            assert torch.equal(g[b:b + 1], w), (b, T, k, p)
    # supplied uniforms are used as given
    u = torch.rand(B, generator=torch.Generator().manual_seed(1))
    got = R.sample_logits_rows(x, V, *_table(temps, ks, ps, seeds, rids), pos, u)
    for b, (T, k, p) in enumerate(rows):
        want = R.sample_logits(x[b:b + 1], V, T, k, p, 0, pos[b:b + 1], u[b:b + 1])
        assert all(torch.equal(g[b:b + 1], w) for g, w in zip(got, want)), b
    # rid = b with one seed is the scalar call on the whole batch
    got = R.sample_logits_rows(x, V, *_table([0.8] * B, [40] * B, [0.95] * B, [3] * B, list(range(B))), pos)
    want = R.sample_logits(x, V, 0.8, 40, 0.95, 3, pos)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # a row's outputs do not depend on its slot (rid is data, not the row index)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(2))
    tab = _table(temps, ks, ps, seeds, rids)
    a = R.sample_logits_rows(x, V, *tab, pos)
    b_ = R.sample_logits_rows(x[perm], V, *(t[perm] for t in tab), pos[perm])
    assert all(torch.equal(s[perm], t) for s, t in zip(a, b_))


def test_oracle_greedy_rows():
    """inv_t = 0: the first maximum of the valid columns (``argmax``) with planted ties, padding
    columns that hold larger values, kept = the number of maxima, thresh = the maximum, u = 0;
    mixed with sampled rows in one call."""
    B = 6
    x = _logits(B, 3)
    x[0, [V - 1, 17, 120]] = 25.0                       # three maxima, the last valid column among them
    x[1, [0, 5]] = 25.0
    x[2, 63] = 25.0                                     # unique
    x[4, [64, 65, 199]] = 26.0
    temps = [0, 0, 0, 0.8, 0, 1.3]
    tab = _table(temps, [5, 0, 1, 40, 0, 0], [0.5, 1.0, 1.0, 0.95, 0.9, 1.0], [1, 2, 3, 4, 5, 6], [0] * B)
    pos = torch.arange(B, dtype=torch.int64)
    u_in = torch.full((B,), 0.999)
    for u in (None, u_in):                              # a supplied uniform does not move a greedy row
        ids, kept, thresh, uo = R.sample_logits_rows(x, V, *tab, pos, u)
        g = [b for b, t in enumerate(temps) if t == 0]
        xv = x[:, :V]
        assert torch.equal(ids[g], xv[g].argmax(-1))
        assert ids[g].tolist() == [17, 0, 63, 64]
        assert kept[g].tolist() == [3, 2, 1, 3]
        assert torch.equal(thresh[g], xv[g].max(-1).values) and thresh[g].tolist() == [25.0, 25.0, 25.0, 26.0]
        assert uo[g].tolist() == [0.0] * 4
        for b in (3, 5):                                # the sampled rows between them are untouched
            ub = torch.tensor([R.sample_uniform(int(tab[3][b]), b, 0)]) if u is None else u[b:b + 1]
            want = R.sample_logits(x[b:b + 1], V, temps[b], int(tab[1][b]), float(tab[2][b]), 0, pos[b:b + 1], ub)
            assert all(torch.equal(t[b:b + 1], w) for t, w in zip((ids, kept, thresh, uo), want))


def _generate(rank, world):
    from distributed_pytorch_from_scratch_amd.evaluate import greedy_decode, greedy_decode_batch
    from distributed_pytorch_from_scratch_amd.models import Transformer, get_preset
    from distributed_pytorch_from_scratch_amd.models.generation import generate
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    args = get_preset("plumbing")
    m = Transformer.from_args(args)
    set_seed(0)
    m.reset_parameters()
    m.eval()
    B, N = 3, 12
    prompt = torch.randint(3, args.vocab_size, (B, 9), generator=torch.Generator().manual_seed(5))
    s = dict(temperature=0.8, top_k=20, top_p=0.9)
    out = {"greedy": generate(m, prompt, N), "scalar": generate(m, prompt, N, seed=11, **s)}
    # equal settings as lists with a scalar seed; a tuple, a tensor and a single list also select the rows mode
    out["lists"] = generate(m, prompt, N, temperature=[0.8] * B, top_k=[20] * B, top_p=[0.9] * B, seed=11)
    out["one_list"] = generate(m, prompt, N, temperature=0.8, top_k=(20,) * B, top_p=0.9, seed=11)
    out["tensor"] = generate(m, prompt, N, temperature=torch.tensor([0.8] * B), top_k=20, top_p=0.9, seed=11)
    out["all_greedy"] = generate(m, prompt, N, temperature=[0] * B, top_k=[5, 0, 1], top_p=0.5, seed=[1, 2, 3])
    out["mixed"] = generate(m, prompt, N, temperature=[0.8, 0, 1.3], top_k=[20, 7, 0], top_p=[0.9, 0.3, 1.0], seed=11)
    # a seed per row: the stream of a request is its own, whatever its slot
    out["seeds"] = generate(m, prompt, N, seed=[21, 22, 23], **s)
    out["seeds_again"] = generate(m, prompt, N, seed=[21, 22, 23], **s)
    out["seeds_swapped"] = generate(m, prompt[[2, 1, 0]], N, seed=[23, 22, 21], **s)
    out["alone"] = [generate(m, prompt[b:b + 1], N, seed=[21 + b], **s)[0] for b in range(B)]
    # ragged
    lens = [9, 4, 1]
    out["r_greedy"] = generate(m, prompt, N, prompt_lens=lens)
    out["r_scalar"] = generate(m, prompt, N, seed=11, prompt_lens=lens, **s)
    out["r_lists"] = generate(m, prompt, N, temperature=[0.8] * B, top_k=[20] * B, top_p=[0.9] * B, seed=11,
                              prompt_lens=lens)
    out["r_all_greedy"] = generate(m, prompt, N, temperature=[0.0] * B, prompt_lens=lens)
    out["r_mixed"] = generate(m, prompt, N, temperature=[0.8, 0, 1.3], top_k=[20, 7, 0], top_p=[0.9, 0.3, 1.0],
                              seed=[5, 6, 7], prompt_lens=lens)
    out["lens"] = lens
    errors = []
    for bad in (dict(temperature=[0.8, 0.8]), dict(top_k=[1, 2, 3, 4]), dict(top_p=[0.9]), dict(seed=[1, 2]),
                dict(temperature=[0.8, -1.0, 0.8]), dict(top_k=[1, -2, 3]), dict(top_p=[0.9, 0.0, 0.5]),
                dict(top_p=[0.9, 1.5, 0.5]), dict(temperature=[0.8, float("nan"), 0.8]), dict(seed=[1, 2 ** 63, 3]),
                # fp32(1 / T) would be 0, the greedy mark, or inf
                dict(temperature=[0.8, 1e46, 0.8]), dict(temperature=[0.8, 1e-46, 0.8]),
                dict(temperature=[0.8, 0.8], prompt_lens=lens), dict(top_p=[0.9, 0.0, 0.5], prompt_lens=lens)):
        try:
            generate(m, prompt, N, **{**dict(temperature=0.8, top_k=20, top_p=0.9, seed=1), **bad})
            errors.append((bad, "no error"))
        except ValueError:
            pass
    out["errors"] = errors
    if world == 1:
        dev = torch.device("cpu")
        prompts = [prompt[b, :n].tolist() for b, n in enumerate(lens)]
        out["cli_batch"] = greedy_decode_batch(m, prompts, 0, 1, 20, dev, seed=[31, 32, 33], **s)
        out["cli_single"] = [greedy_decode(m, p, 0, 1, 20, dev, seed=[31 + b], **s) for b, p in enumerate(prompts)]
    return out


@pytest.fixture(scope="module")
def gen1():
    return run_distributed(_generate, 1)[0]


def test_generate_lists_match_scalars(gen1):
    """Lists of equal settings with a scalar seed keep the row ids 0..B-1: the scalar call's tokens."""
    assert gen1["scalar"] != gen1["greedy"]
    assert gen1["lists"] == gen1["scalar"] and gen1["one_list"] == gen1["scalar"] and gen1["tensor"] == gen1["scalar"]
    assert all(len(o) == 21 and all(0 <= t < 1024 for t in o) for o in gen1["lists"])


def test_generate_all_greedy_lists(gen1):
    assert gen1["all_greedy"] == gen1["greedy"]


def test_generate_mixed_batch(gen1):
    """Row 1 is greedy between two sampled rows: it decodes as in the all-greedy call (every row
    is computed alone on the oracle path), the sampled rows leave the greedy tokens, and row 0,
    with the scalar call's settings, seed and row id, draws the scalar call's tokens."""
    mixed, greedy = gen1["mixed"], gen1["greedy"]
    assert mixed[1] == greedy[1]
    assert mixed[0] != greedy[0] and mixed[2] != greedy[2]
    assert mixed[0] == gen1["scalar"][0]


def test_generate_seed_per_row_is_slot_independent(gen1):
    assert gen1["seeds"] == gen1["seeds_again"] and gen1["seeds"] != gen1["scalar"]
    assert gen1["seeds_swapped"] == gen1["seeds"][::-1]
    assert gen1["alone"] == gen1["seeds"]


def test_generate_errors(gen1):
    assert gen1["errors"] == []


def test_generate_ragged(gen1):
    lens = gen1["lens"]
    assert gen1["r_lists"] == gen1["r_scalar"] and gen1["r_scalar"] != gen1["r_greedy"]
    assert gen1["r_all_greedy"] == gen1["r_greedy"]
    m, g = gen1["r_mixed"], gen1["r_greedy"]
    assert m[1] == g[1] and m[0] != g[0] and m[2] != g[2]
    assert [len(o) for o in m] == [n + 12 for n in lens]
    assert all(o[:n] == r[:n] for o, r, n in zip(m, g, lens))
    # greedy_decode_batch passes the sequences through: a prompt decodes as it does alone
    assert gen1["cli_batch"] == gen1["cli_single"]


def test_generate_rows_tp2_ranks_agree(gen1):
    r = run_distributed(_generate, 2)
    for key in ("lists", "mixed", "seeds", "r_mixed", "all_greedy"):
        assert r[0][key] == r[1][key], key
    assert r[0]["lists"] == r[0]["scalar"] and r[0]["all_greedy"] == r[0]["greedy"]
    assert r[0]["errors"] == [] and r[1]["errors"] == []


def _run(args, timeout=600):
    e = dict(os.environ)
    e.update({"PYTHONPATH": ROOT, "MASTER_ADDR": "127.0.0.1"})
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)


def test_cli_per_prompt_seed(tmp_path):
    """test.py --per_prompt_seed: prompt i samples with seed sample_seed + i and row id 0, so the
    continuations are the same one by one and in batches of any size; without the flag the
    defaults are unchanged."""
    from distributed_pytorch_from_scratch_amd.evaluate import get_test_args, main
    base = ["--data_path", "d", "--ckpt_dir", "c"]
    assert get_test_args(base).per_prompt_seed is False
    assert get_test_args(base + ["--per_prompt_seed"]).per_prompt_seed is True
    with pytest.raises(ValueError, match="no_kv_cache"):
        main(base + ["--no_kv_cache", "--per_prompt_seed"])
    g = torch.Generator().manual_seed(0)
    data = {s: [torch.randint(3, 1024, (int(torch.randint(5, 40, (1,), generator=g)),), generator=g).tolist()
                for _ in range(6)] for s in ("train", "validation")}
    data["special_ids"] = {"<BOS>": 0, "<EOS>": 1, "<UNK>": 2}
    data["vocab_size"] = 1024
    path = tmp_path / "tokens.json"
    path.write_text(json.dumps(data))
    ck = tmp_path / "ck"
    r = _run(["train.py", "--tp_size", "1", "--data_path", str(path), "--model", "plumbing", "-b", "2", "--max_steps", "2",
              "--log_interval", "2", "--save_interval", "2", "--save_dir", str(ck), "--device", "cpu",
              "--master_port", str(_free_port())])
    assert r.returncode == 0, r.stdout + r.stderr

    def decoded(extra):
        r = _run(["test.py", "--tp_size", "1", "--ckpt_dir", str(ck), "--data_path", str(path), "--model", "plumbing",
                  "--max_decode_len", "16", "--synthetic_prompts", "--device", "cpu", "--temperature", "0.8",
                  "--top_k", "20", "--sample_seed", "5", "--master_port", str(_free_port())] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [l for l in r.stdout.splitlines() if re.match(r"^\[.*\] -> \[.*\]$", l)]
        assert len(lines) == 4, r.stdout
        return lines

    one = decoded(["--per_prompt_seed"])
    assert decoded(["--per_prompt_seed", "--decode_batch", "4"]) == one
    assert decoded(["--per_prompt_seed", "--decode_batch", "3"]) == one      # prompt 3 alone in the second batch
    plain = decoded([])
    assert plain[0] == one[0] and plain != one          # prompt 0: seed 5, row id 0 either way
