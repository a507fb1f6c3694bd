"""Prefill against a KV cache on the CPU oracle path (fp32, gloo, TP 1 and 2): a prompt fed in
pieces, multi-token continuations of uniform and ragged caches, ``generate(prefill_chunk=...)``
and the CLI flag.  Everything must compute what the whole prefill / the full forward computes."""
import os
import re
import subprocess
import sys

import pytest
import torch

from dist_helpers import run_distributed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [7, 3]
MORE = [4, 2]
T0 = 7


def _tiny_model():
    from distributed_pytorch_from_scratch_amd.models import ModelArgs, Transformer
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    args = ModelArgs(attn_dim=64, ffn_dim=128, num_heads=4, num_layers=2, vocab_size=96, maxlen=64, vocab_pad_to=1)
    m = Transformer.from_args(args)
    set_seed(0)
    m.reset_parameters()
    m.eval()
    g = torch.Generator().manual_seed(5)
    return m, torch.randint(3, 96, (2, 12), generator=g)


def _full(m, seq):
    with torch.inference_mode():
        return m(seq.view(1, -1), torch.arange(seq.numel()).view(1, -1))[0, -1]


def _chunked(rank, world):
    from distributed_pytorch_from_scratch_amd.models.generation import KVCache, generate, logits_step
    m, ids = _tiny_model()
    dev = torch.device("cpu")
    hl = m.layers[0].attn.num_local_heads
    new = lambda ragged=False: KVCache(2, 2, 24, hl, 16, torch.float32, dev, ragged=ragged)
    out = {}
    # a prompt in pieces of 3 against the whole prefill, then a single-token step on both caches
    cw, cc = new(), new()
    whole = logits_step(m, ids, cw)
    piece = logits_step(m, ids, cc, prefill_chunk=3)
    out["chunk_vs_whole"] = float((piece - whole).abs().max())
    assert cc.len == cw.len == 12
    nxt = whole.argmax(-1, keepdim=True)
    out["chunk_then_step"] = float((logits_step(m, nxt, cc) - logits_step(m, nxt, cw)).abs().max())
    # uniform continuation: 7 ids, then 5 at once, against the full forward of the 12
    c = new()
    logits_step(m, ids[:, :7].contiguous(), c)
    cont = logits_step(m, ids[:, 7:].contiguous(), c)
    out["uniform_cont"] = max(float((cont[b] - _full(m, ids[b])).abs().max()) for b in range(2))
    assert c.len == 12
    # ragged continuation: rows of 7 and 3 ids, then 4 and 2 more (right-padded)
    c = new(True)
    logits_step(m, ids[:, :7].contiguous(), c, LENS)
    more = torch.stack([ids[0, 7:11], torch.cat([ids[1, 3:5], ids[1, :2]])])
    with pytest.raises(ValueError):                      # a ragged continuation needs lens
        logits_step(m, more, c)
    c2 = new(True)
    logits_step(m, ids[:, :7].contiguous(), c2, LENS)
    rag = logits_step(m, more, c, lens=MORE)
    assert c.lens == [11, 5] and c.len == 11
    seqs = [ids[0, :11], ids[1, :5]]
    out["ragged_cont"] = max(float((rag[b] - _full(m, seqs[b])).abs().max()) for b in range(2))
    other = more.clone()
    other[1, 2:] = 95                                    # other padding ids
    out["ragged_pad_equal"] = bool(torch.equal(logits_step(m, other, c2, lens=MORE), rag))
    # ... and in pieces of 3 (row 1 has no real id in the second piece)
    c3 = new(True)
    logits_step(m, ids[:, :7].contiguous(), c3, LENS)
    out["ragged_cont_chunked"] = float((logits_step(m, more, c3, lens=MORE, prefill_chunk=3) - rag).abs().max())
    assert c3.lens == [11, 5]
    one = logits_step(m, rag.argmax(-1, keepdim=True), c)  # single-token steps go on from there
    seqs = [torch.cat([s, rag[b].argmax(-1, keepdim=True)]) for b, s in enumerate(seqs)]
    out["ragged_then_step"] = max(float((one[b] - _full(m, seqs[b])).abs().max()) for b in range(2))
    # generate: the tokens do not depend on the piece size
    p = ids[:, :T0].contiguous()
    out["gen"] = generate(m, p, 10)
    out["gen_chunk"] = {k: generate(m, p, 10, prefill_chunk=k) for k in (1, 3, T0, T0 + 5)}
    out["gen_ragged"] = generate(m, p, 10, prompt_lens=LENS)
    out["gen_ragged_chunk"] = {k: generate(m, p, 10, prompt_lens=LENS, prefill_chunk=k) for k in (1, 3, T0, T0 + 5)}
    with pytest.raises(ValueError, match="prefill_chunk"):
        generate(m, p, 10, prefill_chunk=-1)
    return out


@pytest.fixture(scope="module")
def tp1():
    return run_distributed(_chunked, 1)[0]


@pytest.fixture(scope="module")
def tp2():
    return run_distributed(_chunked, 2)


def _all(tp1, tp2):
    return [tp1] + list(tp2.values())


def test_chunked_prefill_logits_match_the_whole_prefill(tp1, tp2):
    for r in _all(tp1, tp2):
        assert r["chunk_vs_whole"] < 1e-4 and r["chunk_then_step"] < 1e-4, r


def test_uniform_continuation_matches_the_full_forward(tp1, tp2):
    assert all(r["uniform_cont"] < 1e-4 for r in _all(tp1, tp2))


def test_ragged_continuation_matches_each_rows_full_forward(tp1, tp2):
    for r in _all(tp1, tp2):
        assert r["ragged_cont"] < 1e-4 and r["ragged_then_step"] < 1e-4 and r["ragged_cont_chunked"] < 1e-4, r
        assert r["ragged_pad_equal"]


def test_generate_tokens_do_not_depend_on_prefill_chunk(tp1, tp2):
    for k, toks in tp1["gen_chunk"].items():
        assert toks == tp1["gen"], k
    for k, toks in tp1["gen_ragged_chunk"].items():
        assert toks == tp1["gen_ragged"], k
    assert tp2[0]["gen"] == tp2[1]["gen"] == tp1["gen"]
    assert all(t == tp1["gen"] for r in tp2.values() for t in r["gen_chunk"].values())
    assert all(t == tp1["gen_ragged"] for r in tp2.values() for t in r["gen_ragged_chunk"].values())


def test_prefill_chunk_cli_flag():
    from distributed_pytorch_from_scratch_amd.evaluate import get_test_args, main
    base = ["--data_path", "d", "--ckpt_dir", "c"]
    assert get_test_args(base).prefill_chunk == 0
    assert get_test_args(base + ["--prefill_chunk", "4"]).prefill_chunk == 4
    with pytest.raises(ValueError, match="prefill_chunk"):
        main(base + ["--prefill_chunk", "-1"])
    with pytest.raises(ValueError, match="prefill_chunk"):
        main(base + ["--prefill_chunk", "4", "--no_kv_cache"])


def _run(args, timeout=600):
    e = dict(os.environ)
    e.update({"PYTHONPATH": ROOT, "MASTER_ADDR": "127.0.0.1"})
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)


def test_cli_decodes_the_same_text_with_prefill_chunk(tmp_path):
    """test.py with --prefill_chunk 4 (prompts of 9 ids: three pieces), one by one and as a ragged
    batch, prints the continuations it prints without the flag."""
    import json
    from dist_helpers import _free_port
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
                  "--max_decode_len", "16", "--synthetic_prompts", "--device", "cpu",
                  "--master_port", str(_free_port())] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [l for l in r.stdout.splitlines() if re.match(r"^\[.*\] -> \[.*\]$", l)]
        assert len(lines) == 4, r.stdout
        return lines

    whole = decoded([])
    assert decoded(["--prefill_chunk", "4"]) == whole
    assert decoded(["--prefill_chunk", "4", "--decode_batch", "4"]) == whole
