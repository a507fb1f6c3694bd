"""KV-cached autoregressive decoding for the tensor-parallel Transformer.

The reference decodes greedily by re-running the whole prefix every token (``test.py:144-150``:
O(T²·L) work per token, no cache). This module keeps each layer's post-RoPE keys and values
for the local head shard:

* prefill: the prompt goes through the causal flash-attention kernel and fills cache rows
  ``[0, T0)``;
* prefill against a cache: T > 1 new tokens after what the cache holds (a prompt fed in pieces,
  ``prefill_chunk``; a multi-token continuation, also of a ragged cache) append their keys /
  values at every row's own length (``_kv_append_chunk``) and attend the cached prefix plus the
  causal part of the chunk (``_attn_extend``, csrc/kernels/attn_extend.hip);
* decode: one token per sequence per step.  The step is written against DEVICE state only —
  the cache length ``cache.len_t`` (int32) and the position ids ``pos`` live on the GPU, the
  new key/value rows are appended at ``len_t`` (``kv_append``), the single-query split-K
  attention kernel (``attn_decode``, csrc/kernels/decode.hip) reads ``len_t`` itself, and
  ``step_advance`` bumps ``len_t`` / ``pos`` at the end — so at TP = 1 the whole step (about
  20 kernels per layer) is captured once in a HIP graph and replayed per token, instead of being
  re-launched from Python.  With TP > 1 the same step runs eagerly (the row-parallel outputs
  are all-reduced and the vocab-sharded logits all-gathered, so every rank picks the same
  token).  ``DPFS_DECODE_GRAPH=0`` forces the eager step.

The token choice is ``argmax`` (greedy, the default) or, with ``temperature > 0``, one
``sample_logits`` launch (csrc/kernels/sample.hip: temperature, top-k, top-p, a stateless
Philox draw keyed on (seed, row, position)) inside the same captured step.  The four settings
may also be given per row (sequences of B values): the rows of a batch then mix greedy and
sampled requests of any settings, the values live in a device table of the session
(``SampleRows``) that the captured ``_sample_logits_rows`` launches read, and a call with new
settings or seeds is a copy into that table, never a new capture.  Repetition / presence /
frequency penalties and log-probabilities run a third form of the launch,
``_sample_logits_pen``, whose table (``SamplePen``) also holds the token history of every row:
the launch penalises the logits by it, counts the id it draws into it and writes the id's two
log-probabilities, all on the device, so penalised steps replay in the same 8-step graphs.

Ragged batches (``generate(..., prompt_lens=...)``): the prompts of a batch may differ in
length.  The prompt is right-padded; ``cache.len_t`` then holds one int32 per sequence and the
decode kernels read ``len_t[b]`` (their per-row forms), every row appends at its own length and
carries its own position, and the per-row step advance (``_step_advance_rows``) clamps a row
that fills the cache (it is frozen: appends nothing, reads only its cache rows) while shorter
rows go on.  The lengths are device data like the positions, so one captured graph serves every
mix of prompt lengths of the same ``(B, t_max)``.

fp8 KV cache (``kv_dtype="fp8"``; the default ``None`` keeps the activation dtype): keys and
values are stored as OCP e4m3 codes with one fp32 scale per cached (token, head) row
(``ops/reference.py:_kv_quant_rows`` is the format), ``(hd + 4) / (2 hd)`` of the bf16 cache.  The
cache is written by quantising appends (``_kv_append_chunk_q8``, ``_rope_append_q8``) and read
directly by the fp8 forms of the attention kernels (``_attn_decode_q8``, ``_attn_extend_q8``);
only storage is fp8, the math stays fp32 / bf16.  The whole-prompt prefill attends its own fresh,
unquantised q / k / v; everything that reads the cache later sees the quantised rows.

Paged KV cache (``kv_page=N``; the default 0 is the contiguous slab above): ``PagedKVCache`` keeps
per layer and side one pool ``(P, N, H_local, hd)`` and one block table ``tbl`` int32 ``(B, MP)``
for all layers (csrc/kernels/kv_page.h is the layout), always with per-row lengths.  The host maps
pages from a free list in front of every prefill piece, decode step or graph replay
(``reserve``); the kernels (the ``_paged`` ops: the PAGED forms of the same kernels) read the
table from device memory and are safe for any table content, so the mapping is device data like
the lengths and a session's graphs are captured once.

``generate(model, prompt, ...)`` returns the prompt followed by the generated ids.
``logits_step`` exposes the last-position logits (tests compare it against the full recompute).
"""
from __future__ import annotations

import math
import os
import weakref
from typing import List, Optional

import torch

# decode steps captured per HIP graph replay (the host reads the tokens / checks EOS once per
# replay; profiles/r2_decode_bench.jsonl)
_GRAPH_STEPS = 8
# captured graphs kept per session (greedy: 2; sampling: 2 per (temperature, top_k, top_p, seed);
# per-row sampling: 2 for every setting; the penalised form: 2 more for every setting)
_MAX_GRAPHS = 16

from ..ops import gemm_select as GS
from ..ops.dispatch import K, shadow
from ..parallel import comm_ops
from ..parallel import process_manager as pm
from ..parallel import tp_comm


class KVCache:
    """Per-layer key/value buffers ``(B, T_max, H_local, hd)`` in the activation dtype
    (``kv_dtype`` None), or with ``kv_dtype="fp8"`` as ``torch.float8_e4m3fn`` codes plus the fp32
    row scales ``ks`` / ``vs`` ``(B, T_max, H_local)`` (head_dim 32, 64 or 128)."""

    page = 0    # the page size of a ``PagedKVCache``; 0: this contiguous form

    def __init__(self, n_layers: int, B: int, t_max: int, h_local: int, hd: int, dtype, device,
                 ragged: bool = False, kv_dtype: Optional[str] = None):
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"KVCache: kv_dtype must be None (the activation dtype) or 'fp8', got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        if kv_dtype == "fp8":
            if hd not in (32, 64, 128):
                raise ValueError(f"KVCache: kv_dtype='fp8' needs head_dim 32, 64 or 128, got {hd}")
            dtype = torch.float8_e4m3fn
            self.ks = [torch.empty(B, t_max, h_local, dtype=torch.float32, device=device) for _ in range(n_layers)]
            self.vs = [torch.empty(B, t_max, h_local, dtype=torch.float32, device=device) for _ in range(n_layers)]
        self.k = [torch.empty(B, t_max, h_local, hd, dtype=dtype, device=device) for _ in range(n_layers)]
        self.v = [torch.empty(B, t_max, h_local, hd, dtype=dtype, device=device) for _ in range(n_layers)]
        self.len = 0                      # host view (prefill / multi-token steps); ragged: the longest row
        # device view (decode steps): one length for the batch, or with ``ragged`` one per row
        self.len_t = torch.zeros(B if ragged else 1, dtype=torch.int32, device=device)
        self.lens = [0] * B if ragged else None   # host view of the per-row lengths
        self.t_max = t_max
        self._sample_rows = None          # the per-row sampling settings (device), made on first use
        self._sample_pen = None           # the same plus penalties and token history, made on first use

    @property
    def ragged(self) -> bool:
        return self.lens is not None

    @property
    def fp8(self) -> bool:
        return self.kv_dtype == "fp8"

    def tensors(self):
        """Every device buffer of the cache (the fp8 form: codes and scales)."""
        return self.k + self.v + (self.ks + self.vs if self.fp8 else [])

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors())

    def sample_rows(self) -> "SampleRows":
        """The cache's table of per-row sampling settings: like ``len_t`` it is device state of
        the batch that the captured steps read, one per session."""
        if self._sample_rows is None:
            self._sample_rows = SampleRows(self.k[0].size(0), self.len_t.device)
        return self._sample_rows

    def sample_pen(self, vocab: int) -> "SamplePen":
        """The cache's table of the penalised form (settings, penalties, token history)."""
        if self._sample_pen is None or self._sample_pen.vocab != vocab:
            self._sample_pen = SamplePen(self.k[0].size(0), vocab, self.len_t.device)
        return self._sample_pen

    def reset(self):
        self.len = 0
        if self.ragged:
            self.lens = [0] * len(self.lens)

    def set_lens(self, lens):
        self.lens = [min(int(n), self.t_max) for n in lens]
        self.len = max(self.lens)

    def advance(self, n: int = 1):
        """Host bookkeeping of ``n`` decode steps (what ``step_advance`` did on the device)."""
        if self.ragged:
            self.set_lens(m + n for m in self.lens)
        else:
            self.len += n

    def sync_device_len(self):
        if self.ragged:
            self.len_t.copy_(torch.tensor(self.lens, dtype=torch.int32))
        else:
            self.len_t.fill_(self.len)

    def device_pos(self) -> torch.Tensor:
        """Position ids (B,) int64 of the next token of every row, from the device lengths (a
        full row of a ragged cache stays on the cache's last position)."""
        B = self.k[0].size(0)
        if self.ragged:
            return self.len_t.clamp(max=self.t_max - 1).long()
        return self.len_t.long().expand(B).contiguous()


def _check_kv_page(page: int, who: str = "generate") -> int:
    if not isinstance(page, int) or page < 16 or page > 256 or page & (page - 1):
        raise ValueError(f"{who}: kv_page must be a power of two in [16, 256] (0: no paging), got {page!r}")
    return page


class PagedKVCache(KVCache):
    """The paged form of ``KVCache`` (csrc/kernels/kv_page.h is the layout): per layer and side one
    pool ``(P, page, H_local, hd)`` of ``P = pool_pages`` pages (``kv_dtype="fp8"``: e4m3 codes plus
    fp32 scale pools ``(P, page, H_local)``), and one block table ``tbl`` int32 ``(B, MP)``,
    ``MP = ceil(t_max / page)``, for all layers: key t of row b lives in pool row
    ``tbl[b, t // page] * page + t % page``; -1 maps nothing.  Always per-row (``ragged``).

    The pages are handed out on the host: ``reserve(need)`` maps pages from the free list until
    row b can hold ``need[b]`` tokens and uploads the table when it changed; the kernels read the
    table from device memory, so captured graphs stay valid as the mapping changes.  The default
    ``pool_pages = B * MP`` can never run out; a smaller pool serves batches whose rows do not all
    reach ``t_max``, and ``reserve`` raises ``RuntimeError`` on the host when it cannot cover a
    request.  ``page_order`` (a permutation of ``range(P)``, or a callable ``P -> permutation``)
    is the order in which the free list hands pages out (tests: non-contiguous, interleaved)."""

    def __init__(self, n_layers: int, B: int, t_max: int, h_local: int, hd: int, dtype, device, page: int,
                 pool_pages: Optional[int] = None, kv_dtype: Optional[str] = None, page_order=None):
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"PagedKVCache: kv_dtype must be None (the activation dtype) or 'fp8', got {kv_dtype!r}")
        self.page = _check_kv_page(page, "PagedKVCache")
        device = torch.device(device)
        if hd not in (32, 64, 128) and (kv_dtype == "fp8" or device.type == "cuda"):
            raise ValueError(f"PagedKVCache: the paged kernels need head_dim 32, 64 or 128, got {hd}")
        self.kv_dtype = kv_dtype
        self.B = B
        self.t_max = t_max
        self.max_pages = -(-t_max // page)             # MP: table columns
        P = B * self.max_pages if pool_pages is None else int(pool_pages)
        if P < 1 or P * page >= 2 ** 31:
            raise ValueError(f"PagedKVCache: pool_pages must be >= 1 with pool_pages * page < 2^31, got {P}")
        self.pool_pages = P
        if kv_dtype == "fp8":
            dtype = torch.float8_e4m3fn
            self.ks = [torch.empty(P, page, h_local, dtype=torch.float32, device=device) for _ in range(n_layers)]
            self.vs = [torch.empty(P, page, h_local, dtype=torch.float32, device=device) for _ in range(n_layers)]
        self.k = [torch.empty(P, page, h_local, hd, dtype=dtype, device=device) for _ in range(n_layers)]
        self.v = [torch.empty(P, page, h_local, hd, dtype=dtype, device=device) for _ in range(n_layers)]
        order = list(page_order(P) if callable(page_order) else range(P) if page_order is None else page_order)
        if sorted(order) != list(range(P)):
            raise ValueError(f"PagedKVCache: page_order must be a permutation of range({P})")
        self._order = order
        self.tbl = torch.full((B, self.max_pages), -1, dtype=torch.int32, device=device)
        self.tbl_host = torch.full((B, self.max_pages), -1, dtype=torch.int32)     # the host mirror
        self.free = list(reversed(order))          # the free list: pages are popped from its end
        self.mapped = [0] * B                      # pages mapped per row
        self.uploads = 0                           # table uploads so far
        self.len = 0
        self.len_t = torch.zeros(B, dtype=torch.int32, device=device)
        self.lens = [0] * B
        self._sample_rows = None
        self._sample_pen = None

    def tensors(self):
        """Every device buffer of the cache: the pools (fp8: codes and scales) and the table."""
        return super().tensors() + [self.tbl]

    def scales(self, li: int):
        """The (ks, vs) scale pools of layer ``li``, (None, None) for bf16 pools: the two
        arguments by which the paged ops tell the two forms apart."""
        return (self.ks[li], self.vs[li]) if self.fp8 else (None, None)

    def sample_rows(self) -> "SampleRows":
        if self._sample_rows is None:
            self._sample_rows = SampleRows(self.B, self.len_t.device)
        return self._sample_rows

    def sample_pen(self, vocab: int) -> "SamplePen":
        if self._sample_pen is None or self._sample_pen.vocab != vocab:
            self._sample_pen = SamplePen(self.B, vocab, self.len_t.device)
        return self._sample_pen

    def _upload(self):
        self.tbl.copy_(self.tbl_host)
        self.uploads += 1

    def reserve(self, need) -> None:
        """Map pages until row b can hold ``need[b]`` tokens (clamped at ``t_max``); one table
        upload, and only if a page was mapped.  Raises ``RuntimeError`` before anything is mapped
        when the free list cannot cover the request."""
        want = [-(-min(max(int(n), 0), self.t_max) // self.page) for n in need]
        if len(want) != self.B:
            raise ValueError(f"PagedKVCache.reserve: need one token count per row ({self.B}), got {len(want)}")
        extra = sum(max(w - m, 0) for w, m in zip(want, self.mapped))
        if extra == 0:
            return
        if extra > len(self.free):
            raise RuntimeError(f"PagedKVCache.reserve: {extra} pages wanted, {len(self.free)} free (a pool of "
                               f"{self.pool_pages} pages of {self.page} tokens; rows hold {self.mapped} pages and "
                               f"need {want})")
        for b, w in enumerate(want):
            while self.mapped[b] < w:
                self.tbl_host[b, self.mapped[b]] = self.free.pop()
                self.mapped[b] += 1
        self._upload()

    def reset(self):
        """Return every page to the free list (in its original order) and unmap the table."""
        super().reset()
        if any(self.mapped):
            self.free = list(reversed(self._order))
            self.mapped = [0] * self.B
            self.tbl_host.fill_(-1)
            self._upload()


class SampleRows:
    """The sampling settings of every row of a batch as device data, (B,) each, in the layout
    ``_sample_logits_rows`` reads: ``inv_t`` fp32 = fp32(1 / temperature) with 0 for a greedy row,
    ``top_k`` int32, ``top_p`` fp64, ``seed`` int64 and the Philox row id ``rid`` int32."""

    def __init__(self, B: int, device):
        dts = (torch.float32, torch.int32, torch.float64, torch.int64, torch.int32)
        self.inv_t, self.top_k, self.top_p, self.seed, self.rid = (torch.zeros(B, dtype=dt, device=device)
                                                                   for dt in dts)

    def tensors(self):
        return self.inv_t, self.top_k, self.top_p, self.seed, self.rid

    def load(self, host) -> "SampleRows":
        """Copy the five host lists of ``_row_settings`` into the table."""
        for t, v in zip(self.tensors(), host):
            t.copy_(torch.tensor(v, dtype=t.dtype))
        return self


class SamplePen(SampleRows):
    """``SampleRows`` plus what ``_sample_logits_pen`` reads beside it: the penalties ``rep``,
    ``inv_rep`` = fp32(1 / rep), ``pres`` and ``freq``, fp32 (B,) each, and the token history
    ``hist`` int32 (B, ld_h), ld_h = vocab rounded up to 8 (whole 16-byte vectors of a bf16 row's
    layout: B * ld_h * 4 bytes, 201 KB per row of GPT-2's vocabulary).  Bit 31 of ``hist[b, i]``
    says that id i occurs in row b's prompt, bits 0..30 count the draws of i; the launch itself
    adds the id it draws, so the table follows the tokens inside a graph replay.  ``logp`` is the
    (B, 2) log-probability output of the latest launch through ``_draw``."""

    def __init__(self, B: int, vocab: int, device):
        super().__init__(B, device)
        self.rep, self.inv_rep, self.pres, self.freq = (torch.zeros(B, dtype=torch.float32, device=device)
                                                        for _ in range(4))
        self.vocab = vocab
        self.hist = torch.zeros(B, (vocab + 7) // 8 * 8, dtype=torch.int32, device=device)
        self.logp = None

    def pen_tensors(self):
        return self.tensors() + (self.rep, self.inv_rep, self.pres, self.freq, self.hist)

    def load(self, host) -> "SamplePen":
        """Copy the nine host lists (``_row_settings`` + ``_penalty_settings``) into the table."""
        for t, v in zip(self.pen_tensors()[:9], host):
            t.copy_(torch.tensor(v, dtype=t.dtype))      # (fp64 host values round to fp32 here)
        return self

    def load_history(self, prompt: torch.Tensor, lens=None) -> "SamplePen":
        """Zero the history and flag the ids of ``prompt`` (B, T), of ``prompt[b, :lens[b]]`` with
        ``lens``: once per generate() call, before its first draw."""
        idx = prompt.long()
        if lens is not None:    # the padding repeats the row's first id, which is flagged anyway
            real = torch.arange(idx.size(1), device=idx.device)[None, :] < torch.tensor(lens, device=idx.device)[:, None]
            idx = torch.where(real, idx, idx[:, :1])
        self.hist.zero_()
        self.hist.scatter_(1, idx, -2 ** 31)
        return self


def _penalty_settings(B: int, repetition_penalty, presence_penalty, frequency_penalty):
    """The penalties of the B rows as four host lists (rep, 1 / rep in fp64, pres, freq; the table
    rounds them to fp32), scalars broadcast and every value checked; None when every row is
    neutral (1, 0, 0)."""
    vals = [repetition_penalty, presence_penalty, frequency_penalty]
    names = ("repetition_penalty", "presence_penalty", "frequency_penalty")
    for i, name in enumerate(names):
        if isinstance(vals[i], (list, tuple, torch.Tensor)):
            vals[i] = vals[i].tolist() if isinstance(vals[i], torch.Tensor) else list(vals[i])
            if len(vals[i]) != B:
                raise ValueError(f"generate: {name} needs one value per sequence ({B}), got {len(vals[i])}")
        else:
            vals[i] = [vals[i]] * B
        vals[i] = [float(v) for v in vals[i]]
        # (the table holds fp32: a value that overflows it is not finite there)
        if not all(math.isfinite(v) for v in torch.tensor(vals[i], dtype=torch.float64).float().tolist()):
            raise ValueError(f"generate: {name} must be finite in fp32 in every row, got {vals[i]}")
    reps, pres, freq = vals
    if not all(r > 0 for r in reps):
        raise ValueError(f"generate: repetition_penalty must be > 0 in every row, got {reps}")
    inv = [1.0 / r for r in reps]
    inv32 = torch.tensor(inv, dtype=torch.float64).float().tolist()
    if not all(math.isfinite(v) and v != 0.0 for v in inv32):
        raise ValueError(f"generate: fp32(1 / repetition_penalty) must be finite and non-zero, got {reps}")
    if all(r == 1.0 for r in reps) and all(v == 0.0 for v in pres + freq):
        return None
    return reps, inv, pres, freq


def _row_settings(B: int, temperature, top_k, top_p, seed):
    """The per-row form of the sampling settings: None when all four are scalars (one setting
    for the batch), else the five host lists of a ``SampleRows`` table, every scalar broadcast
    to the B rows and every value checked by the rules of the scalar call.  With one ``seed``
    for the batch row b keeps the row id b, so equal settings given as lists draw what the
    scalar call draws; with a seed per row the row id is 0 and a request's stream depends on
    (its seed, position) alone, not on its slot."""
    vals = [temperature, top_k, top_p, seed]
    seq = [isinstance(v, (list, tuple, torch.Tensor)) for v in vals]
    if not any(seq):
        return None
    names = ("temperature", "top_k", "top_p", "seed")
    for i, name in enumerate(names):
        if seq[i]:
            vals[i] = vals[i].tolist() if isinstance(vals[i], torch.Tensor) else list(vals[i])
            if len(vals[i]) != B:
                raise ValueError(f"generate: {name} needs one value per sequence ({B}), got {len(vals[i])}")
        else:
            vals[i] = [vals[i]] * B
    temps, ks, ps, seeds = vals
    if not (all(t >= 0 for t in temps) and all(k >= 0 for k in ks) and all(0 < p <= 1 for p in ps)):
        raise ValueError("generate: need temperature >= 0, top_k >= 0 and 0 < top_p <= 1 in every row, got "
                         f"{temps}, {ks}, {ps}")
    if not all(-2 ** 63 <= int(sd) < 2 ** 63 for sd in seeds):
        raise ValueError(f"generate: every seed must fit 64 bits, got {seeds}")
    inv_t = [1.0 / float(t) if t > 0 else 0.0 for t in temps]      # rounded to fp32 by the table
    # the table marks a greedy row by fp32(1 / T) == 0: a sampled row must not round to it (or to inf)
    scale = torch.tensor(inv_t, dtype=torch.float64).float()
    if any(t > 0 and (s == 0.0 or s == float("inf")) for t, s in zip(temps, scale.tolist())):
        raise ValueError("generate: a temperature > 0 needs a finite, non-zero fp32(1 / temperature) (0 marks a "
                         f"greedy row), got {temps}")
    return (inv_t, [min(int(k), 2 ** 31 - 1) for k in ks], [float(p) for p in ps], [int(sd) for sd in seeds],
            [0] * B if seq[3] else list(range(B)))


def _draw(logits: torch.Tensor, vocab: int, sample, pos: torch.Tensor) -> torch.Tensor:
    """Ids (B,) sampled from ``logits`` with ``sample`` = (temperature, top_k, top_p, seed), one
    ``sample_logits`` launch, or a ``SampleRows`` table, one ``_sample_logits_rows`` launch, or a
    ``SamplePen`` table, one ``_sample_logits_pen`` launch, which also counts the ids into the
    table's history and leaves the two log-probabilities of every id in ``sample.logp``."""
    if isinstance(sample, SamplePen):
        out = K(logits)._sample_logits_pen(logits, vocab, *sample.pen_tensors(), pos)
        sample.logp = out[4]
        return out[0]
    if isinstance(sample, SampleRows):
        return K(logits)._sample_logits_rows(logits, vocab, *sample.tensors(), pos)[0]
    return K(logits).sample_logits(logits, vocab, *sample, pos)[0]


def _attention_step(layer, x2d, positions, tab, cache: KVCache, li: int, B: int, T: int, n_t=None):
    """Multi-token step (prefill, or T > 1 continuation) with host-side cache bookkeeping.  The
    continuation (``cache.len > 0``) reads the cache lengths from ``cache.len_t`` (the caller has
    run ``cache.sync_device_len()``); ``n_t`` (device int32 (B,), or None for T) gives the real
    new tokens of every right-padded row.

    fp8 cache: the whole-prompt prefill (``cache.len == 0``) still attends the fresh, unquantised
    q / k / v through ``attn_fwd``; it fills the cache through ``_kv_append_chunk_q8`` at device
    length 0 (``cache.len_t`` holds 0 there: the caller has synchronised it), the rows the slice
    copy writes.  A continuation appends and attends through the ``_q8`` kernels, so its queries
    see the quantised prefix and the quantised rows of their own chunk."""
    attn = layer.attn
    h, hd = attn.num_local_heads, attn.head_dim
    qkv = attn.wqkv(x2d)                                     # (B*T, 3*h*hd)
    k_ = K(qkv)
    k_.rope_(qkv, positions, tab, 2 * h, hd, False)
    scale = 1.0 / math.sqrt(hd)
    if cache.page:
        # paged cache: the appends and the extend attention go through the block table; the
        # whole-prompt prefill fills the pages at device length 0 (the real ids of every row:
        # ``n_t``) and still attends its fresh q / k / v
        pools = (cache.k[li], cache.v[li], *cache.scales(li), cache.tbl, cache.len_t)
        k_._kv_append_chunk_paged(qkv, *pools, n_t, cache.t_max, cache.page)
        if cache.len == 0:
            q = qkv[:, : h * hd].view(B, T, h, hd)
            kk = qkv[:, h * hd: 2 * h * hd].view(B, T, h, hd)
            v = qkv[:, 2 * h * hd:].view(B, T, h, hd)
            o, _ = k_.attn_fwd(q, kk, v, scale, True)
        else:
            o = k_._attn_extend_paged(qkv, *pools, n_t, cache.t_max, cache.page, scale)
    elif cache.len == 0:
        # prefill: causal flash attention over the prompt
        q = qkv[:, : h * hd].view(B, T, h, hd)
        kk = qkv[:, h * hd: 2 * h * hd].view(B, T, h, hd)
        v = qkv[:, 2 * h * hd:].view(B, T, h, hd)
        if cache.fp8:
            k_._kv_append_chunk_q8(qkv, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t, None)
        else:
            cache.k[li][:, :T] = kk
            cache.v[li][:, :T] = v
        o, _ = k_.attn_fwd(q, kk, v, scale, True)
    elif cache.fp8:
        k_._kv_append_chunk_q8(qkv, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t, n_t)
        o = k_._attn_extend_q8(qkv, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t, n_t, scale)
    else:
        # continuation chunk: every row appends its new keys / values at its own cache length,
        # then its T new queries attend the cached prefix plus the causal part of the chunk
        k_._kv_append_chunk(qkv, cache.k[li], cache.v[li], cache.len_t, n_t)
        o = k_._attn_extend(qkv, cache.k[li], cache.v[li], cache.len_t, n_t, scale)
    return attn.wo(o.reshape(B * T, h * hd))


def _prefill_piece(model, ids: torch.Tensor, cache: KVCache, n: Optional[List[int]]) -> torch.Tensor:
    """Feed ``ids`` (B, T) after what the cache holds and advance its host lengths; ``n`` gives
    the real ids of every right-padded row (0..T, ragged caches), None means T.  Returns the
    hidden states (B, T, D) in front of the final norm."""
    B, T = ids.shape
    dev = ids.device
    if cache.page:      # pages for what this piece appends, before anything is launched
        cache.reserve(c + m for c, m in zip(cache.lens, n if n is not None else [T] * B))
    dt = model.act_dtype(dev)
    model.embedding.out_dtype = dt
    x = model.embedding(ids).reshape(B * T, -1).to(dt)
    n_t = None
    if cache.len == 0:
        positions = torch.arange(T, device=dev).repeat(B)
        if cache.fp8 or cache.page:
            cache.sync_device_len()       # the quantising / paged append of the prefill reads len_t (0)
        if cache.page and n is not None:  # a paged prefill appends the real ids only (pages are per need)
            n_t = torch.tensor(n, dtype=torch.int32, device=dev)
    else:
        cache.sync_device_len()
        base = cache.lens if cache.ragged else [cache.len] * B
        # (the padding and rows past the capacity stay inside the RoPE table)
        positions = (torch.tensor(base, device=dev)[:, None] + torch.arange(T, device=dev)).clamp(
            max=cache.t_max - 1).reshape(-1)
        if n is not None:
            n_t = torch.tensor(n, dtype=torch.int32, device=dev)
    tab = model.rope_table(dev)
    for li, layer in enumerate(model.layers):
        x = x + _attention_step(layer, layer.norm1(x), positions, tab, cache, li, B, T, n_t)
        x = x + layer.ffn(layer.norm2(x))
    if cache.ragged:
        cache.set_lens(c + m for c, m in zip(cache.lens, n if n is not None else [T] * B))
    else:
        cache.len += T
    return x.view(B, T, -1)


def _check_lens(lens, B: int, T: int) -> List[int]:
    lens = [int(n) for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if len(lens) != B:
        raise ValueError(f"prompt_lens: need one length per sequence ({B}), got {len(lens)}")
    if any(n < 1 or n > T for n in lens):
        raise ValueError(f"prompt_lens: every length must be in [1, {T}], got {lens}")
    return lens


@torch.inference_mode()
def logits_step(model, ids: torch.Tensor, cache: KVCache, lens=None, prefill_chunk: int = 0) -> torch.Tensor:
    """Feed ``ids`` (B, T) at positions cache.len.., return (B, vocab) logits of the last one.

    ``lens`` (B ints in [1, T]) feeds a ragged cache right-padded rows: row b holds ``lens[b]``
    real ids, the logits are those of its last real id, and its cache length grows by
    ``lens[b]`` (the cache rows of a prefill's padding are overwritten by the appends before any
    read; a continuation appends the real ids only).  A multi-token continuation of a ragged
    cache needs ``lens``.  Later single-token steps on that cache advance every row at its own
    length.

    ``prefill_chunk`` > 0 feeds ``ids`` in pieces of at most that many tokens (the first piece of
    an empty cache through the flash prefill, the others through ``_attn_extend``), so the
    activations of a call scale with the piece and not with T; the logits are still those of
    every row's last real id."""
    B, T = ids.shape
    dev = ids.device
    if prefill_chunk < 0:
        raise ValueError(f"logits_step: prefill_chunk must be >= 0, got {prefill_chunk}")
    if lens is not None:
        if not cache.ragged:
            raise ValueError("logits_step: lens needs a KVCache(..., ragged=True)")
        lens = _check_lens(lens, B, T)
    if cache.ragged and T > 1 and cache.len > 0 and lens is None:
        raise ValueError("logits_step: a multi-token continuation of a ragged cache is not supported "
                         "without lens (the real new ids of every row)")
    if cache.ragged and cache.len > 0 and lens is not None:
        assert all(c + m <= cache.t_max for c, m in zip(cache.lens, lens)) and cache.t_max <= model.args.maxlen
    else:
        assert cache.len + T <= cache.t_max <= model.args.maxlen
    if T == 1 and cache.len > 0:
        if cache.page:
            cache.reserve(m + 1 for m in cache.lens)
        cache.sync_device_len()
        pos = cache.device_pos() if cache.ragged else torch.full((B,), cache.len, dtype=torch.int64, device=dev)
        _, logits = decode_step(model, ids, pos, cache)
        cache.advance()
        return logits
    step = prefill_chunk if 0 < prefill_chunk < T else T
    last = [m - 1 for m in (lens if lens is not None else [T] * B)]   # the last real id of every row
    h = None
    for s in range(0, T, step):
        e = min(s + step, T)
        n = [min(max(m + 1 - s, 0), e - s) for m in last] if cache.ragged else None
        x = _prefill_piece(model, ids[:, s:e].contiguous(), cache, n)
        rows = [b for b, m in enumerate(last) if s <= m < e]      # their last real id is in this piece
        if rows:
            h = x.new_empty(B, x.size(-1)) if h is None else h
            h[rows] = x[rows, [last[b] - s for b in rows]]
    h = model.norm(h)
    logits = model._lm_head_local(h)
    logits = comm_ops.Gather.apply(logits, model.lm_head.sizes)
    return logits[..., : model.vocab_size].float()


def _pick(model, logits: torch.Tensor, pos: torch.Tensor, sample):
    """Next ids (B,) and the fp32 (B, vocab) logits from the gathered (B, padded vocab) logits:
    ``argmax`` without ``sample``, else one ``sample_logits`` launch on the gathered rows with
    ``sample`` = (temperature, top_k, top_p, seed) and the step's device positions (every TP
    rank holds the same rows, seed and positions, so the ranks agree), or one
    ``_sample_logits_rows`` launch with ``sample`` a ``SampleRows`` table (every rank fills its
    table from the same host lists)."""
    if sample is None:
        logits = logits[..., : model.vocab_size].float()
        return logits.argmax(-1), logits
    nxt = _draw(logits, model.vocab_size, sample, pos)
    return nxt, logits[..., : model.vocab_size].float()


def decode_step(model, ids: torch.Tensor, pos: torch.Tensor, cache: KVCache, sample=None):
    """One token per sequence (``ids`` (B, 1), ``pos`` (B,) int64 = cache.len_t) against the
    cache; advances ``cache.len_t`` and ``pos`` on the device (a ragged cache: per row, clamped
    at the cache capacity).  Returns (next ids (B,),
    logits (B, vocab) fp32); the ids are the ``argmax``, or with ``sample`` = (temperature,
    top_k, top_p, seed) a draw keyed on (seed, row, ``pos``), or with a ``SampleRows`` table every
    row's own choice: ``argmax``, or a draw keyed on (its seed, its row id, ``pos``).  Touches no
    host state: graph-capturable."""
    from .engine_common import _Layer
    if model.args.norm != "rmsnorm":
        return _decode_step_modules(model, ids, pos, cache, sample)
    B = ids.size(0)
    dev = ids.device
    dt = model.act_dtype(dev)
    k = K(model.embedding.weight, dt)
    W = lambda w: shadow(w, dt) if w is not None else None
    model.embedding.out_dtype = dt
    x = model.embedding(ids).reshape(B, -1).to(dt)
    tab = model.rope_table(dev)
    pend = pend_bias = None
    small = B <= 16

    def proj(a, w, bias=None, swiglu=False):
        if small:   # MFMA GEMV-class kernel, SwiGLU fused into the down projection's operand
            return GS.small_nt(k, a, w, bias, swiglu)
        return GS.gemm_nt(k, k.swiglu_fwd(a) if swiglu else a, w, bias)
    # Per layer: [bias + residual +] RMSNorm (one kernel), QKV projection, RoPE + append of
    # k/v at len (one kernel), split-K decode attention, Wo projection, bias + residual +
    # RMSNorm, gate|up projection, SwiGLU + down projection (its bias + residual fold into the
    # next layer's norm).
    for li, layer in enumerate(model.layers):
        L = _Layer(layer)
        if pend is None:
            h1, _ = k.rmsnorm_fwd(x, L.s1, L.eps1)
        else:
            x, h1, _ = k.add_rmsnorm_fwd(pend, pend_bias, x, L.s1, L.eps1)
        qkv = proj(h1, W(L.wqkv), L.bqkv)
        if cache.page:  # through the block table; head_dim 32 / 64 / 128: always the fused kernel
            pools = (cache.k[li], cache.v[li], *cache.scales(li), cache.tbl, cache.len_t, cache.t_max, cache.page)
            k._rope_append_paged(qkv, pos, tab, *pools)
            o = k._attn_decode_paged(qkv, *pools, 1.0 / math.sqrt(L.hd))
        elif cache.fp8:   # head_dim 32 / 64 / 128: always the fused kernel
            k._rope_append_q8(qkv, pos, tab, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t)
            o = k._attn_decode_q8(qkv, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t,
                                  1.0 / math.sqrt(L.hd))
        else:
            if L.hd % 16 == 0:
                k.rope_append(qkv, pos, tab, cache.k[li], cache.v[li], cache.len_t)
            else:
                k.rope_(qkv, pos, tab, 2 * L.h, L.hd, False)
                k.kv_append(qkv, cache.k[li], cache.v[li], cache.len_t)
            o = k.attn_decode(qkv, cache.k[li], cache.v[li], cache.len_t, 1.0 / math.sqrt(L.hd))
        pout = proj(o, W(L.wo))
        tp_comm.all_reduce(pout, async_op=False)
        x, h2, _ = k.add_rmsnorm_fwd(pout, L.bo, x, L.s2, L.eps2)
        pend, pend_bias = proj(proj(h2, W(L.wgu), L.bgu), W(L.wd), swiglu=True), L.bd
        tp_comm.all_reduce(pend, async_op=False)
    _, hfin, _ = k.add_rmsnorm_fwd(pend, pend_bias, x, model.norm.scale, model.norm.eps)
    logits = proj(hfin, W(model.lm_head.weight), model.lm_head.bias)
    nxt, logits = _pick(model, comm_ops.Gather.apply(logits, model.lm_head.sizes), pos, sample)
    _advance(cache, pos)
    return nxt, logits


def _advance(cache: KVCache, pos: torch.Tensor) -> None:
    if cache.ragged:
        K(pos)._step_advance_rows(cache.len_t, pos, cache.t_max)
    else:
        K(pos).step_advance(cache.len_t, pos)


def _decode_step_modules(model, ids: torch.Tensor, pos: torch.Tensor, cache: KVCache, sample=None):
    """decode_step through the nn.Module layers (any norm type, e.g. the LayerNorm variant)."""
    B = ids.size(0)
    dev = ids.device
    dt = model.act_dtype(dev)
    model.embedding.out_dtype = dt
    x = model.embedding(ids).reshape(B, -1).to(dt)
    tab = model.rope_table(dev)
    for li, layer in enumerate(model.layers):
        attn = layer.attn
        h, hd = attn.num_local_heads, attn.head_dim
        qkv = attn.wqkv(layer.norm1(x))                      # (B, 3*h*hd)
        k_ = K(qkv)
        k_.rope_(qkv, pos, tab, 2 * h, hd, False)
        if cache.page:  # the un-fused single-token append: the paged chunk kernel at T = 1
            pools = (cache.k[li], cache.v[li], *cache.scales(li), cache.tbl, cache.len_t)
            k_._kv_append_chunk_paged(qkv, *pools, None, cache.t_max, cache.page)
            o = k_._attn_decode_paged(qkv, *pools, cache.t_max, cache.page, 1.0 / math.sqrt(hd))
        elif cache.fp8:   # the un-fused single-token append: the chunk kernel at T = 1
            k_._kv_append_chunk_q8(qkv, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t, None)
            o = k_._attn_decode_q8(qkv, cache.k[li], cache.v[li], cache.ks[li], cache.vs[li], cache.len_t,
                                   1.0 / math.sqrt(hd))
        else:
            k_.kv_append(qkv, cache.k[li], cache.v[li], cache.len_t)
            o = k_.attn_decode(qkv, cache.k[li], cache.v[li], cache.len_t, 1.0 / math.sqrt(hd))
        x = x + attn.wo(o)
        x = x + layer.ffn(layer.norm2(x))
    logits = model._lm_head_local(model.norm(x))
    nxt, logits = _pick(model, comm_ops.Gather.apply(logits, model.lm_head.sizes), pos, sample)
    _advance(cache, pos)
    return nxt, logits


class DecodeGraph:
    """``nsteps`` decode steps captured as one HIP graph (static ids / pos / output buffers):
    step s writes its next ids into ``outs[s]`` and feeds them to step s + 1 on the device, so
    the host reads the tokens back (and checks EOS) once per replay instead of once per token
    (that round trip, ~90 us, was idle GPU time in every step).  ``sample`` = (temperature,
    top_k, top_p, seed) captures sampling steps: the settings are launch arguments of the
    captured ``sample_logits`` nodes (a session keys its graphs on them), and the draw reads the
    device positions, so a replay at any position draws what the eager step draws there.
    ``sample`` = a ``SampleRows`` table captures ``_sample_logits_rows`` nodes that read the
    settings from the table at replay: one graph for every setting written there later.
    ``sample`` = a ``SamplePen`` table captures ``_sample_logits_pen`` nodes, which also read and
    update the table's token history; step s writes its log-probabilities into ``logps[s]``."""

    def __init__(self, model, cache: KVCache, B: int, nsteps: int = 1, sample=None):
        dev = cache.len_t.device
        self.cache = cache
        self.nsteps = nsteps
        self.ids = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int64, device=dev)
        self.outs = torch.zeros(nsteps, B, dtype=torch.int64, device=dev)
        pen = isinstance(sample, SamplePen)
        # the penalised form: the (model, drawn) log-probabilities of every captured step
        self.logps = torch.zeros(nsteps, B, 2, dtype=torch.float32, device=dev) if pen else None
        saved = cache.len_t.clone()
        saved_hist = sample.hist.clone() if pen else None     # the warm-up step counts its id
        # Warm-up off the capture (first-call GEMM choices, allocator pools).  It appends a row
        # at len_t, which the first real step rewrites before anything reads it.
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.pos.copy_(cache.device_pos())
            decode_step(model, self.ids, self.pos, cache, sample)
        torch.cuda.current_stream().wait_stream(s)
        cache.len_t.copy_(saved)
        if pen:
            sample.hist.copy_(saved_hist)
        _graph_rng_state_normal(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for i in range(nsteps):
                nxt, self.logits = decode_step(model, self.ids, self.pos, cache, sample)
                self.outs[i].copy_(nxt)
                if pen:
                    self.logps[i].copy_(sample.logp)
                if i + 1 < nsteps:
                    self.ids.copy_(nxt.view(-1, 1))
        self.out = self.outs[nsteps - 1]
        cache.len_t.copy_(saved)

    def step(self, ids: torch.Tensor) -> torch.Tensor:
        """Feed ids (B,) at the cache's device length; returns the next ids of every captured
        step (nsteps, B) (device); the cache advances by nsteps rows."""
        self.ids.copy_(ids.view(-1, 1))
        self.graph.replay()
        return self.outs


_RNG_GRAPH_STATE = {}


def _graph_rng_state_normal(dev) -> None:
    """The CUDA generator's graph-safe RNG state is allocated when the first graph registers with
    the generator (and freed when the last one is destroyed); allocated under inference mode
    (this module's decode paths) those tensors are inference tensors, and every later capture
    outside inference mode (engine.GraphTrainStep) fails on their in-place update.  So a
    one-op graph built with inference mode off is kept alive for the process: the state is
    allocated once, as normal tensors, before the first decode capture."""
    if dev.index in _RNG_GRAPH_STATE:
        return
    with torch.inference_mode(False):
        x = torch.zeros(1, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            x.add_(1)
    _RNG_GRAPH_STATE[dev.index] = (g, x)


def _use_graph(dev) -> bool:
    p = pm.pgm
    return (dev.type == "cuda" and os.environ.get("DPFS_DECODE_GRAPH", "1") != "0"
            and (p is None or p.tp_size == 1))


_SESSIONS = {}   # (id(model), B, t_max, device, kv_dtype, ragged[, kv_page, kv_pool_pages]) -> KV cache + decode graphs


def _session(model, B: int, t_max: int, dev, ragged: bool = False, kv_dtype: Optional[str] = None,
             kv_page: int = 0, kv_pool_pages: Optional[int] = None):
    """The KV cache and decode graphs for this (model, batch, length, cache dtype, uniform /
    ragged, page size, pool pages): reused
    by the next generate() call of the same shape, so serving pays the graph capture once (a
    ragged session serves every mix of prompt lengths: they are device data).  Reused only
    while it is the same live model object and no parameter changed since the capture (the
    graphs hold the bf16 weight copies of that version); otherwise rebuilt.  One kept shape
    per model (with a session per cache dtype of that shape), and only caches up to
    DPFS_DECODE_SESSION_MAX_GB (default 16; an fp8 cache counts codes and scales, a paged one its
    pools and table) are kept; ``clear_sessions()`` frees them.  A paged cache (``kv_page`` > 0) is
    a form of the cache like its dtype: its key is the unpaged key followed by (kv_page,
    kv_pool_pages), and the paged sessions of the kept shape stay beside the unpaged ones."""
    attn0 = model.layers[0].attn
    key = (id(model), B, t_max, str(dev), kv_dtype, ragged)
    if kv_page:
        key += (kv_page, kv_pool_pages)
    vers = tuple(p._version for p in model.parameters())
    ent = _SESSIONS.get(key)
    if ent is not None and ent["model"]() is model and ent["vers"] == vers:
        ent["cache"].reset()
        return ent["cache"], ent["graphs"]
    if kv_page:
        cache = PagedKVCache(len(model.layers), B, t_max, attn0.num_local_heads, attn0.head_dim, model.act_dtype(dev),
                             dev, kv_page, kv_pool_pages, kv_dtype)
    else:
        cache = KVCache(len(model.layers), B, t_max, attn0.num_local_heads, attn0.head_dim, model.act_dtype(dev), dev,
                        ragged, kv_dtype)
    graphs = {}
    kv_bytes = cache.nbytes()             # the fp8 form: codes and scales; the paged form: pools and table
    keep_gb = float(os.environ.get("DPFS_DECODE_SESSION_MAX_GB", "16"))
    if _use_graph(dev) and kv_bytes <= keep_gb * 2 ** 30:
        shape = lambda k: k[:4] + k[5:6]      # (what the cache holds, not how: dtype and paging aside)
        for k in [k for k, e in _SESSIONS.items()
                  if e["model"]() is None or (k[0] == id(model) and shape(k) != shape(key))]:
            del _SESSIONS[k]          # dead models, and other shapes of this one (its other cache dtype stays)
        _SESSIONS[key] = {"model": weakref.ref(model), "vers": vers, "cache": cache, "graphs": graphs}
    return cache, graphs


def _session_sample(cache: KVCache, sample, vocab: int = 0):
    """``sample`` as the decode steps take it, and what names it in a session's graph keys: the
    scalar settings (or None, greedy) themselves; per-row host lists (``_row_settings``) are
    copied into the cache's table and the key is "rows" whatever they hold; with the four
    penalty lists behind them (``_penalty_settings``) the table is the ``SamplePen`` one and the
    key is "pen"."""
    if sample is None or isinstance(sample[0], float):
        return sample, sample
    if len(sample) == 9:
        return cache.sample_pen(vocab).load(sample), "pen"
    return cache.sample_rows().load(sample), "rows"


def clear_sessions():
    """Drop every kept KV cache and decode graph (frees their device memory)."""
    _SESSIONS.clear()


@torch.inference_mode()
def generate(model, prompt: torch.Tensor, max_new_tokens: int, eos_id: Optional[int] = None,
             max_len: Optional[int] = None, temperature=0.0, top_k=0, top_p=1.0,
             seed=0, prompt_lens=None, prefill_chunk: int = 0,
             kv_dtype: Optional[str] = None, repetition_penalty=1.0, presence_penalty=0.0,
             frequency_penalty=0.0, return_logprobs: bool = False, kv_page: int = 0,
             kv_pool_pages: Optional[int] = None):
    """Decoding with a KV cache. ``prompt`` (B, T0) int64. Returns, per sequence, the
    prompt plus the generated ids. A sequence stops after emitting ``eos_id`` (kept in the
    output) or when the total length reaches ``max_len`` (default: model maxlen).

    ``prompt_lens`` (B ints in [1, T0], a sequence or a tensor) decodes a ragged batch: row b of
    the right-padded ``prompt`` holds ``prompt_lens[b]`` real ids (the padding values do not
    matter), and the result is ``prompt[b, :prompt_lens[b]]`` plus that row's generated ids.  A
    row stops after ``eos_id``, after ``max_new_tokens`` new ids or when its own total reaches
    ``max_len``; generation ends when every row has stopped.  This always runs the per-row decode
    kernels, also when all lengths are equal.

    ``temperature`` 0 decodes greedily.  ``temperature`` > 0 samples every token with
    ``sample_logits``: softmax(logits / temperature) cut to the ``top_k`` largest logits (0:
    off) and then to the ``top_p`` nucleus (1: off), ties at either cutoff kept whole.  The draw
    for the token that follows position t of row b depends only on (``seed``, b, t), so the same
    call returns the same tokens on the graph and the eager path and on every TP rank.

    Each of ``temperature``, ``top_k``, ``top_p`` and ``seed`` may also be a sequence of B values
    (a list, a tuple or a tensor), one per row; if any is, the call runs per row (scalars are
    broadcast, every value is checked by the same rules, a wrong length is a ``ValueError``).  Row
    b then decodes greedily where ``temperature[b]`` is 0 and samples with its own settings
    elsewhere (the table marks a greedy row by fp32(1 / temperature) == 0, so a positive
    temperature whose fp32 reciprocal is 0 or infinite, above about 1e45 or below about 3e-39,
    is a ``ValueError`` in this mode).  With a scalar ``seed`` the draw of row b is keyed on (``seed``, b, t) as above, so
    equal settings given as lists return what the scalar call returns; with a sequence the draw
    is keyed on (``seed[b]``, 0, t) alone: a request keeps its stream in whatever row of whatever
    batch it is decoded.  The settings are device data of the session (``SampleRows``): its two
    per-row graphs are captured once and serve every later setting and seed.

    ``repetition_penalty`` (> 0), ``presence_penalty`` and ``frequency_penalty`` (any finite
    value), each a scalar or a sequence of B values, penalise the logits before the token choice
    in the vLLM order (``ops/reference.py:penalised_logits``): a logit whose id occurs in the
    row's prompt or among its generated ids is divided by the repetition penalty when positive
    and multiplied by it otherwise; ``frequency_penalty`` times the number of times the id has
    been generated, and ``presence_penalty`` once if that number is not 0, are subtracted.  The
    first generated token is penalised (by the prompt) and counted too.  ``return_logprobs=True``
    returns ``(tokens, logprobs)``: ``logprobs[b]`` holds one ``(logp_model, logp_sampled)`` pair
    per generated id of row b, the id's log-probability under the model's own distribution (raw
    logits, temperature 1, no penalty, no filter) and under the distribution it was drawn from.
    A call with a penalty other than (1, 0, 0) in some row or with ``return_logprobs`` takes the
    ``_sample_logits_pen`` launch for every row and step: all settings go through the session's
    ``SamplePen`` table, whose token history the launch itself updates, so the 8-step replays
    hold; its two graphs, keyed "pen", are captured once for every later setting.  Every other
    call runs exactly the paths above.

    ``prefill_chunk`` > 0 prefills the prompt in pieces of at most that many tokens
    (``logits_step``): the peak activation memory of the call then scales with the piece, not
    with T0.  The decode steps, graphs and sessions are the same; 0 prefills the prompt whole.

    ``kv_dtype="fp8"`` keeps the KV cache as e4m3 codes with per-row fp32 scales (about half the
    bytes; head_dim 32, 64 or 128); ``None`` keeps it in the activation dtype.  A session is kept
    per cache dtype.

    ``kv_page`` > 0 (a power of two in [16, 256]; head_dim 32, 64 or 128 on the GPU) keeps the
    cache in pages of that many tokens (``PagedKVCache``): per layer and side one pool of
    ``kv_pool_pages`` pages (default: ``B * ceil(t_max / kv_page)``, which cannot run out) and one
    block table on the device, so a row occupies the pages its own length needs and not the
    longest length any row might reach.  A paged call always runs the per-row path, as
    ``prompt_lens`` does (without ``prompt_lens`` every row holds T0 ids), returns the tokens of
    the unpaged per-row call, and composes with ``kv_dtype``, ``prefill_chunk`` and every sampling
    form; pages are mapped on the host before each prefill piece, decode step or graph replay, and
    a pool too small for the request raises ``RuntimeError`` there, before anything is launched.
    0, the default, is the contiguous cache."""
    if kv_dtype not in (None, "fp8"):
        raise ValueError(f"generate: kv_dtype must be None (the activation dtype) or 'fp8', got {kv_dtype!r}")
    if prefill_chunk < 0:
        raise ValueError(f"generate: prefill_chunk must be >= 0, got {prefill_chunk}")
    if kv_page != 0:
        _check_kv_page(kv_page)
        if kv_pool_pages is not None and int(kv_pool_pages) < 1:
            raise ValueError(f"generate: kv_pool_pages must be >= 1 (None: B * ceil(t_max / kv_page)), got {kv_pool_pages}")
    elif kv_pool_pages is not None:
        raise ValueError("generate: kv_pool_pages needs kv_page > 0")
    B, T0 = prompt.shape
    dev = prompt.device
    pen = _penalty_settings(B, repetition_penalty, presence_penalty, frequency_penalty)
    if pen is not None or return_logprobs:
        # the penalised form is per row always: a scalar temperature is broadcast here, and a
        # scalar seed keeps the row ids 0 .. B - 1 of the scalar call
        if not isinstance(temperature, (list, tuple, torch.Tensor)):
            temperature = [temperature] * B
        sample = _row_settings(B, temperature, top_k, top_p, seed) + (pen or ([1.0] * B, [1.0] * B, [0.0] * B,
                                                                              [0.0] * B))
    else:
        sample = _row_settings(B, temperature, top_k, top_p, seed)     # host lists; a session's table below
    if sample is None:
        if temperature < 0 or top_k < 0 or not 0 < top_p <= 1:
            raise ValueError("generate: need temperature >= 0, top_k >= 0 and 0 < top_p <= 1, got "
                             f"{temperature}, {top_k}, {top_p}")
        sample = (float(temperature), int(top_k), float(top_p), int(seed)) if temperature > 0 else None
    if prompt_lens is not None or kv_page:
        lens = _check_lens(prompt_lens, B, T0) if prompt_lens is not None else [T0] * B
        return _generate_ragged(model, prompt, lens, max_new_tokens, eos_id, max_len,
                                sample, prefill_chunk, kv_dtype, return_logprobs, kv_page, kv_pool_pages)
    t_max = min(model.args.maxlen, max_len or model.args.maxlen, T0 + max_new_tokens)
    cache, graphs = _session(model, B, t_max, dev, kv_dtype=kv_dtype)
    out = [list(map(int, row)) for row in prompt.tolist()]
    lps = [[] for _ in range(B)]          # (logp_model, logp_sampled) per generated id (the "pen" form)
    result = lambda: (out, lps) if return_logprobs else out
    done = [False] * B
    if max_new_tokens <= 0 or T0 >= t_max:
        return result()
    sample, skey = _session_sample(cache, sample, model.vocab_size)
    pen = isinstance(sample, SamplePen)
    if pen:
        sample.load_history(prompt)
    logits = logits_step(model, prompt, cache, prefill_chunk=prefill_chunk)
    if sample is None:
        nxt = logits.argmax(-1)
    else:   # the first token follows position T0 - 1
        pos0 = torch.full((B,), T0 - 1, dtype=torch.int64, device=dev)
        nxt = _draw(logits, model.vocab_size, sample, pos0)
    cache.sync_device_len()
    pos = torch.full((B,), cache.len, dtype=torch.int64, device=dev)
    chunk = _GRAPH_STEPS
    n_gen = 0

    def emit(row, lp=None) -> bool:
        """Append one step's ids (and log-probabilities); True when generation is finished."""
        nonlocal n_gen
        n_gen += 1
        for b, t in enumerate(row):
            if not done[b]:
                out[b].append(int(t))
                if lp is not None:
                    lps[b].append(tuple(lp[b]))
                done[b] = eos_id is not None and int(t) == eos_id
        return all(done) or n_gen >= max_new_tokens or cache.len >= t_max

    if emit(nxt.tolist(), sample.logp.tolist() if pen else None):
        return result()
    while True:
        if _use_graph(dev):
            # S steps per replay while S more tokens are wanted and the cache has room for them
            S = chunk if (max_new_tokens - n_gen >= chunk and cache.len + chunk <= t_max) else 1
            gkey = S if sample is None else (S, skey)
            g = graphs.get(gkey)
            if g is None:
                if sample is not None and len(graphs) >= _MAX_GRAPHS:
                    for k in [k for k in graphs if isinstance(k, tuple) and k[1] != skey]:
                        del graphs[k]     # sampling graphs of earlier settings; greedy ones stay
                g = graphs[gkey] = DecodeGraph(model, cache, B, S, sample)
            g.pos.fill_(cache.len)
            outs = g.step(nxt)
            rows = outs.tolist()
            lrows = g.logps.tolist() if pen else [None] * S
            nxt = g.out
            for row, lp in zip(rows, lrows):
                cache.len += 1
                if emit(row, lp):
                    return result()
        else:
            nxt, _ = decode_step(model, nxt.view(B, 1), pos, cache, sample)
            cache.len += 1
            if emit(nxt.tolist(), sample.logp.tolist() if pen else None):
                return result()


def _generate_ragged(model, prompt: torch.Tensor, lens: List[int], max_new_tokens: int, eos_id, max_len, sample,
                     prefill_chunk: int = 0, kv_dtype: Optional[str] = None, return_logprobs: bool = False,
                     kv_page: int = 0, kv_pool_pages: Optional[int] = None):
    """generate() for per-row prompt lengths ``lens`` (see there).  Every row is fed to every
    step, finished or not; the host drops the ids of a finished row, and the device keeps a row
    that has filled the cache frozen inside it (``_step_advance_rows``).  With ``kv_page`` the
    cache is a ``PagedKVCache``: the pages of what a step (or a replay's steps) appends are
    reserved on the host in front of it."""
    B = prompt.size(0)
    dev = prompt.device
    cap = min(model.args.maxlen, max_len or model.args.maxlen)     # total length at which a row stops
    t_max = min(cap, max(lens) + max_new_tokens)
    cache, graphs = _session(model, B, t_max, dev, ragged=True, kv_dtype=kv_dtype, kv_page=kv_page,
                             kv_pool_pages=kv_pool_pages)
    rows = prompt.tolist()
    out = [list(map(int, rows[b][:lens[b]])) for b in range(B)]
    lps = [[] for _ in range(B)]
    result = lambda: (out, lps) if return_logprobs else out
    done = [n >= cap for n in lens]
    if max_new_tokens <= 0 or all(done):
        return result()
    sample, skey = _session_sample(cache, sample, model.vocab_size)
    pen = isinstance(sample, SamplePen)
    if pen:
        sample.load_history(prompt, lens)
    # The padded prompt up to the longest row that fits the cache; a row at or past the cache
    # capacity is done already and enters the cache full (frozen).
    T = min(max(lens), t_max)
    logits = logits_step(model, prompt[:, :T].contiguous(), cache, [min(n, T) for n in lens],
                         prefill_chunk)
    if sample is None:
        nxt = logits.argmax(-1)
    else:   # the first token of row b follows position lens[b] - 1
        pos0 = torch.tensor(cache.lens, dtype=torch.int64, device=dev) - 1
        nxt = _draw(logits, model.vocab_size, sample, pos0)
    cache.sync_device_len()
    pos = cache.device_pos()
    chunk = _GRAPH_STEPS
    n_gen = 0

    def emit(row, lp=None) -> bool:
        """Append one step's ids (and log-probabilities) to the live rows; True when every row is
        finished."""
        nonlocal n_gen
        n_gen += 1
        for b, t in enumerate(row):
            if not done[b]:
                out[b].append(int(t))
                if lp is not None:
                    lps[b].append(tuple(lp[b]))
                done[b] = (eos_id is not None and int(t) == eos_id) or len(out[b]) >= cap
        return all(done) or n_gen >= max_new_tokens

    if emit(nxt.tolist(), sample.logp.tolist() if pen else None):
        return result()
    while True:
        if _use_graph(dev):
            # S steps per replay while S more tokens are wanted and the longest live row has room
            # for them (a finished row may run past its end: the kernels keep it in bounds)
            longest = max(n for n, d in zip(cache.lens, done) if not d)
            S = chunk if (max_new_tokens - n_gen >= chunk and longest + chunk <= t_max) else 1
            if cache.page:   # the pages of the replay's S appends (the table is device data: no new capture)
                cache.reserve(n + S for n in cache.lens)
            gkey = S if sample is None else (S, skey)
            g = graphs.get(gkey)
            if g is None:
                if sample is not None and len(graphs) >= _MAX_GRAPHS:
                    for k in [k for k in graphs if isinstance(k, tuple) and k[1] != skey]:
                        del graphs[k]     # sampling graphs of earlier settings; greedy ones stay
                g = graphs[gkey] = DecodeGraph(model, cache, B, S, sample)
            g.pos.copy_(cache.device_pos())
            outs = g.step(nxt)
            steps = outs.tolist()
            lsteps = g.logps.tolist() if pen else [None] * S
            nxt = g.out
            for row, lp in zip(steps, lsteps):
                cache.advance()
                if emit(row, lp):
                    return result()
        else:
            if cache.page:
                cache.reserve(n + 1 for n in cache.lens)
            nxt, _ = decode_step(model, nxt.view(B, 1), pos, cache, sample)
            cache.advance()
            if emit(nxt.tolist(), sample.logp.tolist() if pen else None):
                return result()
