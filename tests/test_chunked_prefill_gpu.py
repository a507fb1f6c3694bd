"""Prefill against a KV cache through the kernels of csrc/kernels/attn_extend.hip on the MI355X:
chunked prompts, multi-token continuations of a ragged cache and ``generate(prefill_chunk=...)``
on gpt2-small (2 layers)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29573")
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


def _cache(m, B, t_max, ragged=False):
    from distributed_pytorch_from_scratch_amd.models.generation import KVCache
    attn = m.layers[0].attn
    return KVCache(len(m.layers), B, t_max, attn.num_local_heads, attn.head_dim, torch.bfloat16, torch.device("cuda"),
                   ragged=ragged)


def _full(m, seq):
    with torch.inference_mode():
        return m(seq.view(1, -1), torch.arange(seq.numel(), device="cuda").view(1, -1))[0, -1].float()


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_chunked_prefill_logits_match_the_whole_prefill(model):
    """Teacher-forced: a 100-id prompt in pieces of 32 (flash prefill, then three continuation
    chunks, the last of 4 ids) and 4 single-token steps with the whole prefill's ids, against the
    whole prefill and against the full forward (the cached-vs-recompute bf16 tolerance)."""
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    B = 2
    prompt = _prompt(model, B, 100, 11)
    cw, cc = _cache(model, B, 128), _cache(model, B, 128)
    lw, lc = logits_step(model, prompt, cw), logits_step(model, prompt, cc, prefill_chunk=32)
    seq = prompt
    for step in range(5):
        for b in range(B):
            full = _full(model, seq[b])
            rw, rc, rf = _rel(lc[b], lw[b]), _rel(lc[b], full), _rel(lw[b], full)
            print("step", step, "row", b, "chunked vs whole", rw, "chunked vs full", rc, "whole vs full", rf)
            assert rw < 3e-2 and rc < 3e-2, (step, b, rw, rc)
        if step == 4:
            break
        nxt = lw.argmax(-1, keepdim=True)                   # the same ids into both caches
        seq = torch.cat([seq, nxt], 1)
        lw, lc = logits_step(model, nxt, cw), logits_step(model, nxt, cc)
    assert cw.len == cc.len == 104


def test_ragged_continuation_matches_each_rows_full_forward(model):
    """Rows of 100, 37 and 1 cached ids take 20, 5 and 20 more in one right-padded step: every
    row's logits against its own full forward; the padding ids change nothing, bit for bit."""
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    lens, more = [100, 37, 1], [20, 5, 20]
    ids = _prompt(model, 3, 120, 12)
    new = torch.stack([ids[b, n:n + 20] for b, n in enumerate(lens)])
    zero_pad, rand_pad = new.clone(), new.clone()
    for b, n in enumerate(more):
        zero_pad[b, n:] = 0
        rand_pad[b, n:] = _prompt(model, 1, 20 - n, 17 + b)[0]
    outs = []
    for pad in (zero_pad, rand_pad):
        c = _cache(model, 3, 128, ragged=True)
        logits_step(model, ids[:, :100].contiguous(), c, lens)
        outs.append(logits_step(model, pad, c, lens=more))
        assert c.lens == [120, 42, 21]
        outs.append(logits_step(model, outs[-1].argmax(-1, keepdim=True), c))   # and a decode step after it
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    seqs = [ids[b, :n + k] for b, (n, k) in enumerate(zip(lens, more))]
    for b, seq in enumerate(seqs):
        rel = _rel(outs[0][b], _full(model, seq))
        rel1 = _rel(outs[1][b], _full(model, torch.cat([seq, outs[0][b].argmax(-1, keepdim=True)])))
        print("row", b, "rel", rel, "next step", rel1)
        assert rel < 3e-2 and rel1 < 3e-2, (b, rel, rel1)
    with pytest.raises(ValueError):                         # without lens it is still refused
        logits_step(model, zero_pad, c)


def test_generate_with_prefill_chunk_eager_and_graph(model, monkeypatch):
    """generate(prefill_chunk=32), uniform and ragged: the decode steps after a chunked prefill
    give the same tokens eager and from the captured graphs."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    prompt = _prompt(model, 3, 100, 13)
    for kw in ({}, dict(prompt_lens=[100, 37, 1])):
        monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
        eager = G.generate(model, prompt, max_new_tokens=20, prefill_chunk=32, **kw)
        monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
        graph = G.generate(model, prompt, max_new_tokens=20, prefill_chunk=32, **kw)
        assert eager == graph
        assert [len(o) for o in graph] == [n + 20 for n in kw.get("prompt_lens", [100] * 3)]
    with pytest.raises(ValueError, match="prefill_chunk"):
        G.generate(model, prompt, max_new_tokens=4, prefill_chunk=-2)


def test_chunked_prefill_lowers_the_peak_memory(model):
    """Prompt 1024, B 2: the peak allocation of the prefill in pieces of 128 is strictly below
    the whole prefill's (the cache is allocated before the measurement in both)."""
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    prompt = _prompt(model, 2, 1024, 14)
    peaks = {}
    for chunk in (0, 128):
        c = _cache(model, 2, 1024)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        logits_step(model, prompt, c, prefill_chunk=chunk)
        torch.cuda.synchronize()
        peaks[chunk] = torch.cuda.max_memory_allocated() - base
        del c
    print("prefill peak bytes above the cache: whole", peaks[0], "chunks of 128", peaks[128])
    assert peaks[128] < peaks[0], peaks


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
out = [generate(m, ids, max_new_tokens=8, max_len=65, prompt_lens=[60, 20, 10], prefill_chunk=c) for c in (0, 16)]
torch.cuda.synchronize()
print("KASSERT_OK", os.path.basename(_ext.so_path()), [len(o) for o in out[1]], [len(o) for o in out[0]])
destroy_dist_env()
"""


def test_kernel_assert_build_runs_the_extend_kernels_clean():
    """The bounds-assert build (DPFS_KERNEL_ASSERT=1, _C_kassert) carries the asserts of
    attn_extend_k and kv_append_chunk_k (len[b] >= 0): a ragged chunked prefill, with rows that
    have no real id in the later pieces, trips none."""
    import glob
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not glob.glob(os.path.join(root, "distributed_pytorch_from_scratch_amd", "_C_kassert*.so")):
        pytest.fail("_C_kassert not built (python tools/build_ext.py --kernel-assert)")
    env = dict(os.environ, PYTHONPATH=root, MASTER_ADDR="127.0.0.1", MASTER_PORT="29587", DPFS_KERNEL_ASSERT="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _KASSERT_SCRIPT], cwd=root, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "KASSERT_OK _C_kassert" in r.stdout and "[65, 28, 18] [65, 28, 18]" in r.stdout, r.stdout
