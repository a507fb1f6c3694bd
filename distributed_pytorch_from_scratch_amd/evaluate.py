"""Evaluation + greedy decoding entrypoint (the reference's ``test.py``).

Reference parity: ``test.py:23-172`` — CLI ``--master_addr --master_port --tp_size
--data_path/-d --tokenizer_path/-t --ckpt_dir --use_vallina_impl --max_decode_len
--random_seed``; for every ``tprank-{r}_iter-*_loss-*.pth`` of this rank (sorted by iteration)
the validation loss (batch 1, bf16) is written to ``{ckpt_dir}/val/tprank-{r}_val.txt`` and TB
``val/loss``; then the last checkpoint greedily continues 8 fixed prompts until EOS or
``max_decode_len``.

Fixed reference bugs: the decode loads ``ckpt_paths[-1]`` (the reference
indexes the last *character* of a path string, ``test.py:124``), and the embedding no longer
mutates the token buffer, so TP>1 decoding is correct.  Extensions: ``--synthetic_prompts``
(token-id prompts when no tokenizer file is available), the vocab-parallel loss, and sampled
decoding (``--temperature --top_k --top_p --sample_seed``; the defaults decode greedily;
``--per_prompt_seed`` gives prompt i the seed ``sample_seed + i`` and a stream of its own, the
same one by one and in any batch; ``--repetition_penalty --presence_penalty
--frequency_penalty`` penalise the ids of the prompt and of the continuation as ``generate``
does, and ``--logprobs`` prints the sum and the mean of the model's log-probabilities of the
generated ids after each completion), and
``--decode_batch N``: the prompts are decoded N at a time as one ragged batch (per-row KV
lengths, ``models/generation.py``) instead of one by one.
"""
from __future__ import annotations

import os
import re
from argparse import ArgumentParser

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .constants import BOS_TOKEN, EOS_TOKEN, IGNORE_INDEX
from .data.dataset import get_dataloader
from .models import Transformer, get_preset
from .parallel import process_manager as pm
from .utils import checkpoint as ck
from .utils.dist import destroy_dist_env, init_dist_env, set_seed
from .utils.tb import SummaryWriter

PROMPTS = [
    "Nice to meet you, it's",
    "Great empire never falls, it only",
    "Your majesty, it's my duty ",
    "I shall be glad ",
    "What a glory to ",
    "Shame for the weak, it's",
    "The brave man ne",
    "Poor old man, it's",
]


def _backend(use_cuda: bool) -> str:
    """RCCL on GPUs; ``DPFS_BACKEND=gloo`` runs several ranks on one GPU (the TP collectives
    then go through ``DPFS_TP_COMM``'s transports, e.g. the xGMI kernels)."""
    return os.environ.get("DPFS_BACKEND") or ("nccl" if use_cuda else "gloo")


def get_test_args(argv=None):
    p = ArgumentParser()
    g = p.add_argument_group("distributed")
    g.add_argument("--master_addr", type=str, default="127.0.0.1")
    g.add_argument("--master_port", type=str, default="23333")
    g.add_argument("--tp_size", type=int, default=2)
    g = p.add_argument_group("data")
    g.add_argument("--data_path", "-d", type=str, required=True)
    g.add_argument("--tokenizer_path", "-t", type=str, default=None)
    g = p.add_argument_group("model")
    g.add_argument("--use_vallina_impl", action="store_true")
    g.add_argument("--model", type=str, default="reference")
    p.add_argument("--ckpt_dir", type=str, required=True)
    g = p.add_argument_group("decode")
    g.add_argument("--max_decode_len", type=int, default=128)
    g.add_argument("--synthetic_prompts", action="store_true")
    g.add_argument("--no_kv_cache", action="store_true", help="re-run the full prefix per token (reference)")
    g.add_argument("--temperature", type=float, default=0.0, help="0: greedy (reference); > 0: sample")
    g.add_argument("--top_k", type=int, default=0, help="sample from the k largest logits (0: off)")
    g.add_argument("--top_p", type=float, default=1.0, help="sample from the top-p nucleus (1: off)")
    g.add_argument("--sample_seed", type=int, default=0, help="seed of the sampling draws")
    g.add_argument("--per_prompt_seed", action="store_true",
                   help="prompt i samples with seed sample_seed + i, whatever batch row decodes it")
    g.add_argument("--repetition_penalty", type=float, default=1.0,
                   help="> 1 discourages ids of the prompt and the continuation (1: off)")
    g.add_argument("--presence_penalty", type=float, default=0.0,
                   help="subtracted once from the logit of every id generated so far (0: off)")
    g.add_argument("--frequency_penalty", type=float, default=0.0,
                   help="subtracted from a logit once per time its id was generated (0: off)")
    g.add_argument("--logprobs", action="store_true",
                   help="print the sum and mean model log-probability of the generated ids")
    g.add_argument("--decode_batch", type=int, default=1,
                   help="prompts decoded together as one ragged batch (1: one by one, the reference)")
    g.add_argument("--prefill_chunk", type=int, default=0,
                   help="prefill a prompt in pieces of at most this many tokens (0: whole)")
    g.add_argument("--kv_cache_dtype", choices=["act", "fp8"], default="act",
                   help="KV cache storage: the activation dtype, or e4m3 codes with per-row fp32 scales")
    g.add_argument("--kv_page", type=int, default=0,
                   help="keep the KV cache in pages of this many tokens (a power of two in [16, 256]; 0: contiguous)")
    g.add_argument("--kv_pool_pages", type=int, default=0,
                   help="pages per pool of the paged KV cache (0: batch * ceil(t_max / kv_page), which cannot run out)")
    g = p.add_argument_group("other")
    g.add_argument("--random_seed", type=int, default=0)
    g.add_argument("--device", type=str, default=None)
    return p.parse_args(argv)


@torch.inference_mode()
def calc_loss(model: Transformer, dataloader, dev) -> float:
    total, n = 0.0, 0
    for batch in dataloader:
        ids = batch["input_ids"].to(dev)
        tgt = batch["target_ids"].to(dev)
        pos = batch["position_ids"].to(dev)
        logits = model(ids, pos)
        loss = F.cross_entropy(logits.float().reshape(-1, logits.size(-1)), tgt.reshape(-1),
                               ignore_index=IGNORE_INDEX, reduction="mean")
        total += float(loss.item())
        n += 1
    return total / max(1, n)


@torch.inference_mode()
def greedy_decode(model: Transformer, prompt_ids, bos: int, eos: int, max_len: int, dev, kv_cache: bool = True,
                  temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                  prefill_chunk: int = 0, kv_dtype=None, repetition_penalty=1.0, presence_penalty=0.0,
                  frequency_penalty=0.0, return_logprobs: bool = False, kv_page: int = 0, kv_pool_pages=None):
    """Greedy continuation of ``[bos] + prompt`` until EOS or ``max_len + 1`` tokens (the
    reference's stopping rule, ``test.py:144-150``); returns the ids after BOS without EOS.
    ``kv_cache`` decodes one token per step against cached keys/values
    (``models/generation.py``); ``False`` re-runs the whole prefix per token like the reference.
    ``temperature`` > 0 samples instead (``top_k`` / ``top_p`` / ``seed`` as in ``generate``, a
    one-element sequence for the per-row form: ``seed=[s]`` draws with (s, position) alone);
    sampling runs in the KV-cached decode step only.  ``prefill_chunk`` > 0 prefills the prompt
    in pieces of at most that many tokens (KV-cached decoding only); ``kv_dtype`` "fp8" keeps the
    KV cache as e4m3 codes (``generate``).  The three penalties are ``generate``'s (KV-cached
    decoding only); ``return_logprobs`` returns (ids, the model's log-probability of every
    generated id, a final EOS included) instead of the ids.  ``kv_page`` / ``kv_pool_pages`` page
    the KV cache (``generate``; KV-cached decoding only)."""
    pen = (repetition_penalty, presence_penalty, frequency_penalty) != (1.0, 0.0, 0.0) or return_logprobs
    if not kv_cache and (temperature != 0 or isinstance(seed, (list, tuple, torch.Tensor)) or pen):
        raise ValueError("sampling (--temperature > 0), penalties and log-probabilities run in the KV-cached decode "
                         "step: drop --no_kv_cache")
    if kv_cache:
        from .models.generation import generate
        n0 = 1 + len(prompt_ids)
        tokens = torch.tensor([bos] + list(prompt_ids), dtype=torch.long, device=dev).view(1, -1)
        out = generate(model, tokens, max_new_tokens=max(1, max_len + 1 - n0), eos_id=eos, temperature=temperature,
                       top_k=top_k, top_p=top_p, seed=seed, prefill_chunk=prefill_chunk, kv_dtype=kv_dtype,
                       repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                       frequency_penalty=frequency_penalty, return_logprobs=return_logprobs, kv_page=kv_page,
                       kv_pool_pages=kv_pool_pages)
        out, lps = (out[0][0], out[1][0]) if return_logprobs else (out[0], None)
        out = out[1:]
        if out and out[-1] == eos and len(out) > len(prompt_ids):
            out = out[:-1]
        return (out, [a for a, _ in lps]) if return_logprobs else out
    tokens = torch.tensor([bos] + list(prompt_ids), dtype=torch.long, device=dev).view(1, -1)
    while True:
        pos = torch.arange(tokens.size(1), device=dev).unsqueeze(0)
        logits = model(tokens, pos)[0, -1]
        nxt = int(logits.argmax(-1).item())
        tokens = torch.cat([tokens, torch.tensor([[nxt]], device=dev)], dim=1)
        if nxt == eos or tokens.size(1) > max_len:
            out = tokens[0, 1:]
            if nxt == eos:
                out = out[:-1]
            return out.tolist()


@torch.inference_mode()
def greedy_decode_batch(model: Transformer, prompts, bos: int, eos: int, max_len: int, dev, temperature: float = 0.0,
                        top_k: int = 0, top_p: float = 1.0, seed: int = 0, prefill_chunk: int = 0, kv_dtype=None,
                        repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                        return_logprobs: bool = False, kv_page: int = 0, kv_pool_pages=None):
    """``greedy_decode`` of several prompts (lists of ids of any lengths) as one ragged KV-cached
    batch: per prompt, the ids after BOS without a trailing EOS, each row stopped by the
    reference's rule (EOS, or ``max_len + 1`` tokens in all).  With sampling, row b draws with
    (``seed``, b, position).  Each of ``temperature``, ``top_k``, ``top_p`` and ``seed`` may be a
    sequence with one value per prompt (``generate``): with a seed per prompt, row b draws with
    (``seed[b]``, position) alone.  The penalties (scalars here) and ``return_logprobs`` are
    ``greedy_decode``'s: with the latter every prompt gives (ids, model log-probabilities)."""
    from .models.generation import generate
    prompts = [list(p) for p in prompts]
    if not prompts:
        return []
    lens = [1 + len(p) for p in prompts]
    if max(lens) > max_len:   # such a prompt still gets its one token (greedy_decode): one by one
        seq = lambda v: isinstance(v, (list, tuple, torch.Tensor))
        row = lambda v, b: [v[b]] if seq(v) else v                # a prompt's own value, still per row
        return [greedy_decode(model, p, bos, eos, max_len, dev, True, row(temperature, b), row(top_k, b),
                              row(top_p, b), row(seed, b), prefill_chunk, kv_dtype, repetition_penalty,
                              presence_penalty, frequency_penalty, return_logprobs, kv_page, kv_pool_pages)
                for b, p in enumerate(prompts)]
    tokens = torch.zeros(len(prompts), max(lens), dtype=torch.long, device=dev)
    for b, p in enumerate(prompts):
        tokens[b, :lens[b]] = torch.tensor([bos] + p, dtype=torch.long, device=dev)
    outs = generate(model, tokens, max_new_tokens=max_len + 1 - min(lens), eos_id=eos, max_len=max_len + 1,
                    temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, prompt_lens=lens,
                    prefill_chunk=prefill_chunk, kv_dtype=kv_dtype, repetition_penalty=repetition_penalty,
                    presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                    return_logprobs=return_logprobs, kv_page=kv_page, kv_pool_pages=kv_pool_pages)
    outs, lps = outs if return_logprobs else (outs, [None] * len(prompts))
    res = []
    for p, out, lp in zip(prompts, outs, lps):
        out = out[1:]
        if out and out[-1] == eos and len(out) > len(p):
            out = out[:-1]
        res.append((out, [a for a, _ in lp]) if return_logprobs else out)
    return res


def _decode_all(model, prompts, ds, args, dev, sampling):
    """Continuations of ``prompts`` (lists of ids): one by one, or ``--decode_batch`` at a time.
    With ``--logprobs`` every element is (ids, model log-probabilities of the generated ids)."""
    n = args.decode_batch
    # --per_prompt_seed: prompt i draws with (sample_seed + i, position), one by one and in a batch
    seeds = lambda i, m: {"seed": [sampling["seed"] + j for j in range(i, i + m)]} if args.per_prompt_seed else {}
    if n <= 1:
        return [greedy_decode(model, ids, ds.bos, ds.eos, args.max_decode_len, dev, not args.no_kv_cache,
                              **{**sampling, **seeds(i, 1)})
                for i, ids in enumerate(prompts)]
    outs = []
    for i in range(0, len(prompts), n):
        part = prompts[i:i + n]
        outs += greedy_decode_batch(model, part, ds.bos, ds.eos, args.max_decode_len, dev,
                                    **{**sampling, **seeds(i, len(part))})
    return outs


def test(rank, args):
    set_seed(args.random_seed)
    use_cuda = (args.device or ("cuda" if torch.cuda.is_available() else "cpu")) == "cuda"
    p = init_dist_env(args, rank, world_size=args.tp_size, backend=_backend(use_cuda))
    dev = torch.device("cuda", torch.cuda.current_device()) if use_cuda else torch.device("cpu")
    margs = get_preset(args.model)
    model = Transformer.from_args(margs).to(dev)
    model.reset_parameters()
    model.eval()
    dtype = torch.bfloat16 if use_cuda else torch.float32
    model.set_compute_dtype(dtype)

    paths = ck.list_checkpoints(args.ckpt_dir, p.tp_rank)
    if not paths:
        raise ValueError(f"[TP Rank {p.tp_rank}]: No checkpoints found in {args.ckpt_dir}")
    print(f"[TP Rank {p.tp_rank}]: Found {len(paths)} checkpoints.", flush=True)

    loader = get_dataloader(args.data_path, 1, IGNORE_INDEX, split="validation", maxlen=margs.maxlen,
                            shuffle=False)
    save_path = os.path.join(args.ckpt_dir, "val", f"tprank-{p.tp_rank}_val.txt")
    os.makedirs(os.path.dirname(save_path), exist_ok=True)
    writer = SummaryWriter(os.path.join(args.ckpt_dir, f"tprank-{p.tp_rank}"))
    results = []
    with open(save_path, "a") as f:
        f.write("Ckpt -> Validation loss\n")
        for path in paths:
            it = ck.parse_iter(path)
            ck.load_model(model, path)   # fp32 master weights; bf16 compute via the kernels
            loss = calc_loss(model, loader, dev)
            f.write(f"{path} -> {loss:.4f}\n")
            writer.add_scalar("val/loss", loss, it)
            results.append((it, loss))
    writer.close()

    ck.load_model(model, paths[-1])
    ds = loader.dataset
    sampling = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.sample_seed,
                    prefill_chunk=args.prefill_chunk)
    if args.kv_cache_dtype != "act":
        sampling["kv_dtype"] = args.kv_cache_dtype
    pens = dict(repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty,
                frequency_penalty=args.frequency_penalty)
    if pens != dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
        sampling.update(pens)
    if args.logprobs:
        sampling["return_logprobs"] = True
    if args.kv_page:
        sampling.update(kv_page=args.kv_page, kv_pool_pages=args.kv_pool_pages or None)
    split = lambda outs: zip(*outs) if args.logprobs else (outs, [None] * len(outs))
    decoded = []
    if args.synthetic_prompts or not args.tokenizer_path:
        prompts = [torch.randint(3, margs.vocab_size, (8,), generator=torch.Generator().manual_seed(i)).tolist()
                   for i in range(4)]
        outs, lps = split(_decode_all(model, prompts, ds, args, dev, sampling))
        for ids, out, lp in zip(prompts, outs, lps):
            assert out[:len(ids)] == ids
            decoded.append((str(ids), str(out[len(ids):]), lp))
    else:
        from tokenizers import Tokenizer
        tok = Tokenizer.from_file(args.tokenizer_path)
        assert tok.token_to_id(BOS_TOKEN) == ds.bos and tok.token_to_id(EOS_TOKEN) == ds.eos
        texts = [t.strip() for t in PROMPTS]
        outs, lps = split(_decode_all(model, [tok.encode(t).ids for t in texts], ds, args, dev, sampling))
        for t, out, lp in zip(texts, outs, lps):
            text = tok.decode(out).strip()
            decoded.append((t, text[len(t):] if text.startswith(t) else text, lp))
    with open(save_path, "a") as fp:
        print("\n\nInput texts -> Decoded texts", file=fp)
        for a_, b_, lp in decoded:
            lines = [f"{a_} -> {b_}"]
            if lp is not None:      # --logprobs: the model's own distribution, whatever the ids were drawn from
                lines.append(f"  logprob sum {sum(lp):.4f} mean {sum(lp) / max(1, len(lp)):.4f} over {len(lp)} ids")
            for line in lines:
                print(line, file=fp)
                if p.tp_rank == 0:
                    print(line, flush=True)
    dist.barrier()
    destroy_dist_env()
    return results


def check_kv_page_args(args) -> None:
    """--kv_page / --kv_pool_pages: the page size is ``generate``'s (a power of two in [16, 256]), and
    a paged cache is a KV cache."""
    if args.kv_page < 0 or args.kv_pool_pages < 0:
        raise ValueError("--kv_page and --kv_pool_pages must be >= 0")
    if args.kv_page == 0 and args.kv_pool_pages > 0:
        raise ValueError("--kv_pool_pages sizes the pools of a paged KV cache: give --kv_page too")
    if args.kv_page > 0:
        if args.no_kv_cache:
            raise ValueError("--kv_page pages the KV cache: drop --no_kv_cache")
        if args.kv_page < 16 or args.kv_page > 256 or args.kv_page & (args.kv_page - 1):
            raise ValueError(f"--kv_page must be a power of two in [16, 256], got {args.kv_page}")


def main(argv=None):
    args = get_test_args(argv)
    if args.no_kv_cache and (args.temperature != 0 or args.per_prompt_seed):
        raise ValueError("sampling (--temperature > 0, --per_prompt_seed) runs in the KV-cached decode step: drop "
                         "--no_kv_cache")
    if args.no_kv_cache and (args.logprobs or (args.repetition_penalty, args.presence_penalty,
                                               args.frequency_penalty) != (1.0, 0.0, 0.0)):
        raise ValueError("penalties and --logprobs run in the KV-cached decode step: drop --no_kv_cache")
    if args.decode_batch < 1 or (args.decode_batch > 1 and args.no_kv_cache):
        raise ValueError("--decode_batch must be >= 1, and > 1 batches the KV-cached decode step: drop --no_kv_cache")
    if args.prefill_chunk < 0 or (args.prefill_chunk > 0 and args.no_kv_cache):
        raise ValueError("--prefill_chunk must be >= 0, and > 0 chunks the KV-cached prefill: drop --no_kv_cache")
    if args.kv_cache_dtype != "act" and args.no_kv_cache:
        raise ValueError("--kv_cache_dtype chooses the storage of the KV cache: drop --no_kv_cache")
    check_kv_page_args(args)
    import torch.multiprocessing as mp
    os.environ.setdefault("MASTER_ADDR", args.master_addr)
    mp.spawn(test, args=(args,), nprocs=args.tp_size, join=True)


if __name__ == "__main__":
    main()
