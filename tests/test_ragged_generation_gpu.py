"""Ragged batches (per-row prompt and cache lengths) through the decode kernels on the MI355X:
``generate(..., prompt_lens=...)`` and ``logits_step(..., lens=...)`` on gpt2-small (2 layers),
eager and captured in HIP graphs."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29569")
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    yield
    destroy_dist_env()


@pytest.fixture(scope="module")
def model(dist1):
    from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
    from distributed_pytorch_from_scratch_amd.models import generation as G
    args = get_preset("gpt2-small", num_layers=2)
    m = Transformer.from_args(args).cuda()
    m.reset_parameters()
    m.eval()
    yield m
    G.clear_sessions()


def _prompt(m, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, m.args.vocab_size, (B, T), generator=g).cuda()


def _both(monkeypatch, fn):
    """fn() on the eager step, then on the captured graphs."""
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    eager = fn()
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    return eager, fn()


@pytest.mark.parametrize("sampling", [{}, dict(temperature=0.8, top_k=40, top_p=0.95, seed=3)], ids=["greedy", "sampled"])
def test_equal_lengths_match_the_uniform_path(model, monkeypatch, sampling):
    """Same shapes and GEMM choices, only the length kernels differ: the per-row path at equal
    lengths returns exactly the uniform path's tokens, eager and graph."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    B, T0, new = 3, 50, 21
    prompt = _prompt(model, B, T0, 1)
    ue, ug = _both(monkeypatch, lambda: G.generate(model, prompt, max_new_tokens=new, **sampling))
    re_, rg = _both(monkeypatch, lambda: G.generate(model, prompt, max_new_tokens=new, prompt_lens=[T0] * B, **sampling))
    assert ue == ug == re_ == rg
    assert all(len(o) == T0 + new for o in rg)
    (key,) = G._SESSIONS                                   # the per-row path has a session of its own
    assert key[-1] is True and G._SESSIONS[key]["cache"].len_t.numel() == B


def _ragged_logits(m, prompt, lens, steps=4):
    from distributed_pytorch_from_scratch_amd.models.generation import KVCache, logits_step
    attn = m.layers[0].attn
    cache = KVCache(len(m.layers), len(lens), 128, attn.num_local_heads, attn.head_dim, torch.bfloat16,
                    torch.device("cuda"), ragged=True)
    out = [logits_step(m, prompt, cache, lens)]
    for _ in range(steps):
        out.append(logits_step(m, out[-1].argmax(-1, keepdim=True), cache))
    return out


def test_ragged_logits_match_recompute_and_ignore_padding(model):
    """Ragged prefill + 4 single-token steps: every row's logits against the full forward of that
    row alone at its true length (the cached-vs-recompute bf16 tolerance of the uniform test);
    the padding ids change nothing, bit for bit."""
    lens = [100, 37, 1]
    prompt = _prompt(model, 3, 100, 2)
    zero_pad, rand_pad = prompt.clone(), prompt.clone()
    for b, n in enumerate(lens):
        zero_pad[b, n:] = 0
        rand_pad[b, n:] = _prompt(model, 1, 100 - n, 7 + b)[0]
    la = _ragged_logits(model, zero_pad, lens)
    seqs = [prompt[b, :n] for b, n in enumerate(lens)]
    for step, lc in enumerate(la):
        for b, seq in enumerate(seqs):
            with torch.inference_mode():
                full = model(seq.view(1, -1), torch.arange(seq.numel(), device="cuda").view(1, -1))[0, -1].float()
            rel = ((lc[b] - full).norm() / full.norm()).item()
            print("step", step, "row", b, "rel", rel)
            assert rel < 3e-2, (step, b, rel)
        nxt = lc.argmax(-1)
        seqs = [torch.cat([s, nxt[b:b + 1]]) for b, s in enumerate(seqs)]
    lb = _ragged_logits(model, rand_pad, lens)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    with pytest.raises(ValueError):                         # ragged multi-token continuation
        from distributed_pytorch_from_scratch_amd.models.generation import KVCache, logits_step
        attn = model.layers[0].attn
        c = KVCache(2, 3, 128, attn.num_local_heads, attn.head_dim, torch.bfloat16, torch.device("cuda"), ragged=True)
        logits_step(model, zero_pad, c, lens)
        logits_step(model, zero_pad[:, :2], c)


def test_padding_does_not_change_the_tokens(model, monkeypatch):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    lens = [100, 37, 1]
    prompt = _prompt(model, 3, 100, 2)
    zero_pad = prompt.clone()
    for b, n in enumerate(lens):
        zero_pad[b, n:] = 0
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
    a = G.generate(model, zero_pad, max_new_tokens=12, prompt_lens=lens)
    b_ = G.generate(model, prompt, max_new_tokens=12, prompt_lens=torch.tensor(lens))
    assert a == b_ and [len(o) for o in a] == [n + 12 for n in lens]
    assert all(o[:n] == prompt[i, :n].tolist() for i, (o, n) in enumerate(zip(a, lens)))


def test_ragged_graph_matches_eager_and_session_is_reused(model, monkeypatch):
    """Row 0 crosses the 256-key split boundary alone; the graphs replay what the eager step
    computes.  A second call with other lengths of the same (B, t_max) reuses the cache and the
    captured graphs: the lengths are device data."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    prompt = _prompt(model, 3, 250, 3)
    lens, lens2, new = [250, 100, 7], [250, 9, 64], 40
    G.clear_sessions()
    eager, graph = _both(monkeypatch, lambda: G.generate(model, prompt, max_new_tokens=new, prompt_lens=lens))
    assert eager == graph and [len(o) for o in graph] == [n + new for n in lens]
    (sess,) = G._SESSIONS.values()
    graphs, held = sess["graphs"], dict(sess["graphs"])
    assert sorted(held) == [1, 8]
    graph2 = G.generate(model, prompt, max_new_tokens=new, prompt_lens=lens2)
    (sess2,) = G._SESSIONS.values()
    assert sess2["graphs"] is graphs and sess2["cache"] is sess["cache"]
    assert all(graphs[k] is v for k, v in held.items()) and len(graphs) == len(held)
    monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
    assert G.generate(model, prompt, max_new_tokens=new, prompt_lens=lens2) == graph2
    assert [len(o) for o in graph2] == [n + new for n in lens2]
    assert graph2[0] == graph[0]                            # row 0 is the same prompt in both calls


def test_a_row_that_fills_the_cache_is_frozen(model, monkeypatch):
    """max_len stops row 0 after 5 new tokens (its cache fills) while the others produce 20."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    lens, new = [60, 20, 10], 20
    prompt = _prompt(model, 3, 60, 4)
    eager, graph = _both(monkeypatch, lambda: G.generate(model, prompt, max_new_tokens=new, max_len=65, prompt_lens=lens))
    assert eager == graph
    assert [len(o) for o in graph] == [65, 20 + new, 10 + new]


_KASSERT_SCRIPT = r"""
import os, torch
from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
from distributed_pytorch_from_scratch_amd.models.generation import generate
from distributed_pytorch_from_scratch_amd.ops import _ext
init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
m = Transformer.from_args(get_preset("gpt2-small", num_layers=2)).cuda()
m.reset_parameters()
m.eval()
ids = torch.randint(0, 50257, (3, 60), device="cuda")
out = []
for graph in ("0", "1"):
    os.environ["DPFS_DECODE_GRAPH"] = graph
    out.append(generate(m, ids, max_new_tokens=20, max_len=65, prompt_lens=[60, 20, 10]))
torch.cuda.synchronize()
print("KASSERT_OK", os.path.basename(_ext.so_path()), out[0] == out[1], [len(o) for o in out[1]])
destroy_dist_env()
"""


def test_kernel_assert_build_runs_the_per_row_kernels_clean():
    """The bounds-assert build (DPFS_KERNEL_ASSERT=1, _C_kassert) carries the per-row kernels'
    asserts (len[b] >= 0, pos[b] >= 0): a ragged decode with a row that freezes trips none."""
    import glob
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not glob.glob(os.path.join(root, "distributed_pytorch_from_scratch_amd", "_C_kassert*.so")):
        pytest.fail("_C_kassert not built (python tools/build_ext.py --kernel-assert)")
    env = dict(os.environ, PYTHONPATH=root, MASTER_ADDR="127.0.0.1", MASTER_PORT="29585", DPFS_KERNEL_ASSERT="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _KASSERT_SCRIPT], cwd=root, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "KASSERT_OK _C_kassert" in r.stdout and "True [65, 40, 30]" in r.stdout, r.stdout
