"""Ragged batches in KV-cached decoding (per-row cache lengths) on the CPU oracle path: fp32,
gloo, TP 1 and 2.  Every row of a right-padded batch must decode exactly as it does alone."""
import pytest
import torch

from dist_helpers import run_distributed

LENS = [7, 3, 1]


def _tiny_model():
    from distributed_pytorch_from_scratch_amd.models import ModelArgs, Transformer
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    args = ModelArgs(attn_dim=64, ffn_dim=128, num_heads=4, num_layers=2, vocab_size=96, maxlen=64, vocab_pad_to=1)
    m = Transformer.from_args(args)
    set_seed(0)
    m.reset_parameters()
    m.eval()
    g = torch.Generator().manual_seed(5)
    return m, torch.randint(3, 96, (3, 7), generator=g)


def _ragged(rank, world):
    from distributed_pytorch_from_scratch_amd.evaluate import greedy_decode, greedy_decode_batch
    from distributed_pytorch_from_scratch_amd.models.generation import KVCache, generate, logits_step
    m, prompt = _tiny_model()
    dev = torch.device("cpu")
    B = len(LENS)
    # last-position logits: ragged prefill + 3 single-token steps against each row's own recompute
    cache = KVCache(2, B, 16, m.layers[0].attn.num_local_heads, 16, torch.float32, dev, ragged=True)
    lc = logits_step(m, prompt, cache, LENS)
    seqs = [prompt[b, :n] for b, n in enumerate(LENS)]
    worst = 0.0
    for step in range(4):
        for b, seq in enumerate(seqs):
            with torch.inference_mode():
                full = m(seq.view(1, -1), torch.arange(seq.numel()).view(1, -1))[0, -1]
            worst = max(worst, float((lc[b] - full).abs().max()))
            assert torch.allclose(lc[b], full, atol=1e-4), (step, b, (lc[b] - full).abs().max())
        if step == 3:
            break
        nxt = lc.argmax(-1, keepdim=True)
        seqs = [torch.cat([s, nxt[b]]) for b, s in enumerate(seqs)]
        lc = logits_step(m, nxt, cache)
    assert cache.lens == [n + 3 for n in LENS] and cache.len_t.tolist() == cache.lens
    with pytest.raises(ValueError):                      # ragged multi-token continuation
        logits_step(m, prompt[:, :2], cache)
    out = {"worst": worst}
    out["ragged"] = generate(m, prompt, 20, prompt_lens=LENS)
    out["alone"] = [generate(m, prompt[b:b + 1, :n], 20)[0] for b, n in enumerate(LENS)]
    out["tensor_lens"] = generate(m, prompt, 20, prompt_lens=torch.tensor(LENS))
    other_pad = prompt.clone()
    for b, n in enumerate(LENS):
        other_pad[b, n:] = 95
    out["other_pad"] = generate(m, other_pad, 20, prompt_lens=LENS)
    out["equal"] = generate(m, prompt, 20, prompt_lens=[7] * B)
    out["uniform"] = generate(m, prompt, 20)
    # a row stops at its own max_len / EOS while the others go on
    out["max_len"] = generate(m, prompt, 20, max_len=12, prompt_lens=LENS)
    eos = out["ragged"][1][LENS[1] + 4]                  # row 1's 5th new token as EOS
    out["eos"] = generate(m, prompt, 20, eos_id=eos, prompt_lens=LENS)
    out["eos_id"] = eos
    s = dict(temperature=0.8, top_k=20, top_p=0.9)
    out["a"] = generate(m, prompt, 20, seed=11, prompt_lens=LENS, **s)
    out["a2"] = generate(m, prompt, 20, seed=11, prompt_lens=LENS, **s)
    out["b"] = generate(m, prompt, 20, seed=12, prompt_lens=LENS, **s)
    prompts = [prompt[b, :n].tolist() for b, n in enumerate(LENS)]
    out["cli_batch"] = greedy_decode_batch(m, prompts, 0, 1, 26, dev)
    out["cli_single"] = [greedy_decode(m, p, 0, 1, 26, dev) for p in prompts]
    out["cli_batch_short"] = greedy_decode_batch(m, prompts, 0, 1, 9, dev)
    out["cli_single_short"] = [greedy_decode(m, p, 0, 1, 9, dev) for p in prompts]
    for bad in ([7, 3], [7, 3, 0], [8, 3, 1], torch.tensor([7, 3, 1, 1])):
        with pytest.raises(ValueError, match="prompt_lens"):
            generate(m, prompt, 20, prompt_lens=bad)
    return out


@pytest.fixture(scope="module")
def tp1():
    return run_distributed(_ragged, 1)[0]


@pytest.fixture(scope="module")
def tp2():
    return run_distributed(_ragged, 2)


def test_ragged_logits_match_per_row_recompute(tp1, tp2):
    assert tp1["worst"] < 1e-4 and all(r["worst"] < 1e-4 for r in tp2.values())


def test_ragged_greedy_tokens_match_each_prompt_alone(tp1, tp2):
    assert tp1["ragged"] == tp1["alone"]
    assert [len(o) for o in tp1["ragged"]] == [n + 20 for n in LENS]
    assert tp1["tensor_lens"] == tp1["ragged"] and tp1["other_pad"] == tp1["ragged"]
    assert tp1["equal"] == tp1["uniform"]
    assert tp2[0]["ragged"] == tp2[1]["ragged"] == tp1["ragged"]
    assert tp2[0]["alone"] == tp1["alone"]


def test_rows_stop_on_their_own(tp1):
    r = tp1["ragged"]
    assert tp1["max_len"] == [r[0][:12], r[1][:12], r[2][:12]]       # totals reach max_len = 12
    e, eos = tp1["eos"], tp1["eos_id"]
    for b, n in enumerate(LENS):
        new = r[b][n:]
        want = r[b][: n + new.index(eos) + 1] if eos in new else r[b]
        assert e[b] == want, b
    assert len(e[1]) <= LENS[1] + 5 and e[1][-1] == eos


def test_ragged_sampling_repeats_and_ranks_agree(tp1, tp2):
    assert tp1["a"] == tp1["a2"] and tp1["a"] != tp1["b"] and tp1["a"] != tp1["ragged"]
    assert all(o[:n] == g[:n] and len(o) == n + 20 and all(0 <= t < 96 for t in o)
               for o, g, n in zip(tp1["a"], tp1["ragged"], LENS))
    assert tp2[0]["a"] == tp2[1]["a"] == tp1["a"] and tp2[0]["b"] == tp2[1]["b"]


def test_greedy_decode_batch_matches_greedy_decode(tp1):
    assert tp1["cli_batch"] == tp1["cli_single"]
    assert tp1["cli_batch_short"] == tp1["cli_single_short"]
    assert all(len(o) <= 9 for o in tp1["cli_single_short"])         # at most max_len + 1 tokens less BOS


def test_oracle_per_row_lengths_and_freeze():
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    torch.manual_seed(3)
    B, T, H, hd = 3, 6, 2, 4
    kc, vc = torch.randn(B, T, H, hd), torch.randn(B, T, H, hd)
    qkv = torch.randn(B, 3 * H * hd)
    ln = torch.tensor([0, 4, 6], dtype=torch.int32)                  # row 2 is full
    k1, v1 = kc.clone(), vc.clone()
    R.kv_append(qkv, k1, v1, ln)
    for b, t in enumerate([0, 4]):
        ku, vu = kc.clone(), vc.clone()
        R.kv_append(qkv, ku, vu, torch.tensor([t], dtype=torch.int32))
        assert torch.equal(k1[b], ku[b]) and torch.equal(v1[b], vu[b])
    assert torch.equal(k1[2], kc[2]) and torch.equal(v1[2], vc[2])
    o = R.attn_decode(qkv, k1, v1, ln, 0.5)
    for b, t in enumerate([0, 4, 5]):                                # a full row attends its T rows
        ou = R.attn_decode(qkv, k1, v1, torch.tensor([t], dtype=torch.int32), 0.5)
        assert torch.equal(o[b], ou[b])
    pos = torch.tensor([0, 4, 5])
    for want_len, want_pos in (([1, 5, 6], [1, 5, 5]), ([2, 6, 6], [2, 5, 5]), ([3, 6, 6], [3, 5, 5])):
        R._step_advance_rows(ln, pos, T)
        assert ln.tolist() == want_len and pos.tolist() == want_pos
    one, p1 = torch.tensor([4], dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    R.step_advance(one, p1)                                          # the uniform form is unchanged
    assert one.tolist() == [5] and p1.tolist() == [5, 5, 5]
    with pytest.raises(AssertionError):
        R.step_advance(ln, pos)                                      # per-row lengths need the capacity


def test_decode_batch_cli_flag():
    from distributed_pytorch_from_scratch_amd.evaluate import get_test_args, main
    base = ["--data_path", "d", "--ckpt_dir", "c"]
    assert get_test_args(base).decode_batch == 1
    assert get_test_args(base + ["--decode_batch", "8"]).decode_batch == 8
    with pytest.raises(ValueError, match="decode_batch"):
        main(base + ["--decode_batch", "4", "--no_kv_cache"])
