"""The fp8 KV cache on the MI355X (csrc/kernels/kv8.hip and the fp8 forms of decode.hip /
attn_extend.hip): the quantising appends against the independent quantiser of
tests/numerics_kv8.py bit for bit, the fp8 decode attention against its fp64 oracle and derived
unit, the fp8 extend attention against the bf16 kernel on the dequantised caches bit for bit, and
the model paths (``logits_step``, ``generate``, sessions) on gpt2-small (2 layers).

NaN codes (0x7f) and NaN scales in rows nobody may read are data: every index stays in bounds."""
import os

import pytest
import torch

import numerics as N
import numerics_kv8 as Q

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"
NAN = float("nan")
B, H = N.DEC_B, N.DEC_H
SENT = 0x55                      # byte sentinel of unwritten codes


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _u8(c):
    return c.view(torch.uint8)


def _blank_caches(Tmax, hd):
    k8 = torch.full((B, Tmax, H, hd), SENT, dtype=torch.uint8, device=DEV).view(Q.F8)
    ks = torch.full((B, Tmax, H), NAN, device=DEV)
    return k8, k8.clone(), ks, ks.clone()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _strided(x, pad=16, off=8):
    """x [M, n] as a column slice of a wider NaN tensor: row stride n + pad, 16-byte aligned."""
    w = torch.full((x.size(0), x.size(1) + pad), NAN, dtype=x.dtype, device=x.device)
    v = w[:, off:off + x.size(1)]
    v.copy_(x)
    assert v.stride(0) == x.size(1) + pad
    return v


def _qkv_rows(T, hd, seed):
    """Packed rows [B*T, 3 H hd]: randn, with a zero k row, the tie row and an outlier row."""
    g = torch.Generator().manual_seed(seed + 10 * hd + T)
    qkv = torch.randn(B * T, 3, H, hd, generator=g)
    qkv[0, 1, 0] = 0
    qkv[0, 2, 1] = Q.tie_row(hd)
    qkv[B * T - 1, 1, 2] = Q.outlier_row(hd, g)
    qkv[B * T - 1, 2, 0] = -Q.tie_row(hd)
    return qkv.view(B * T, 3 * H * hd).bfloat16()


# -------------------------------------------------------------------------- appends ----

APPEND_CASES = [                                   # (T, len, n)
    (1, [7], None), (1, [0, 39], None), (1, [3, 40], None),
    (5, [0], None), (5, [33, 37], None), (5, [2, 20], [0, 3]),
    (33, [0], None), (33, [7], [33, 10]), (33, [3, 20], [33, 33]),
]


@pytest.mark.parametrize("T,lens,n", APPEND_CASES)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_kv_append_chunk_q8_exact(C, hd, T, lens, n):
    """T 1 / 5 / 33 into T_max 40, uniform and per-row lengths, per-row n with a 0, rows cut off at
    len + t >= T_max (and a full row): the written codes and scales equal the helper quantiser's bit
    for bit, every other byte and scale keeps its sentinel.  qkv is a strided view (ld > row)."""
    Tmax = 40
    qkv = _qkv_rows(T, hd, 71)
    k8, v8, ks, vs = _blank_caches(Tmax, hd)
    C._kv_append_chunk_q8(_strided(qkv.to(DEV)), k8, v8, ks, vs, _i32(lens), None if n is None else _i32(n))
    rows = qkv.view(B, T, 3, H, hd)
    ll = lens * B if len(lens) == 1 else lens
    for c8, cs, part in ((k8, ks, 1), (v8, vs, 2)):
        want8 = torch.full((B, Tmax, H, hd), SENT, dtype=torch.uint8)
        wants = torch.full((B, Tmax, H), NAN)
        for b in range(B):
            m = max(0, min(T if n is None else n[b], T, Tmax - ll[b]))
            if m:
                cq, iq = Q.quant_rows(rows[b, :m, part])
                want8[b, ll[b]:ll[b] + m], wants[b, ll[b]:ll[b] + m] = _u8(cq), iq
        assert torch.equal(_u8(c8).cpu(), want8), (hd, T, lens, n, part)
        assert _same_bits(cs.cpu(), wants), (hd, T, lens, n, part)


@pytest.mark.parametrize("lens", [[0], [17], [39], [40], [45], [5, 38], [40, 12], [40, 40]])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_rope_append_q8_exact(C, hd, lens):
    """_rope_append_q8 leaves qkv as rope_append leaves it, and its codes and scales equal rope_
    followed by _kv_append_chunk_q8 at T 1 (which the test above ties to the helper): uniform and
    per-row lengths, one row full, and a full uniform cache, where nothing may be written."""
    Tmax = 40
    g = torch.Generator().manual_seed(73 + hd + sum(lens))
    qkv = _qkv_rows(1, hd, 74).to(DEV)
    pos = torch.randint(0, 512, (B,), generator=g).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    ln = _i32(lens)
    a = _strided(qkv)
    k8, v8, ks, vs = _blank_caches(Tmax, hd)
    C._rope_append_q8(a, pos, tab, k8, v8, ks, vs, ln)
    # rope_append on bf16 caches: the same rotation
    r = qkv.clone()
    kc = torch.zeros(B, Tmax, H, hd, dtype=torch.bfloat16, device=DEV)
    C.rope_append(r, pos, tab, kc, kc.clone(), ln)
    assert torch.equal(a, r)
    # rope_ + the chunk append at T 1
    b_ = qkv.clone()
    C.rope_(b_, pos, tab, 2 * H, hd, False)
    assert torch.equal(a, b_)
    k8b, v8b, ksb, vsb = _blank_caches(Tmax, hd)
    C._kv_append_chunk_q8(b_, k8b, v8b, ksb, vsb, ln, None)
    assert torch.equal(_u8(k8), _u8(k8b)) and torch.equal(_u8(v8), _u8(v8b))
    assert _same_bits(ks, ksb) and _same_bits(vs, vsb)
    ll = lens * B if len(lens) == 1 else lens
    for b in range(B):
        written = (_u8(k8)[b] != SENT).any(-1).any(-1).nonzero().view(-1).tolist()
        assert written == ([ll[b]] if ll[b] < Tmax else []), (hd, lens, b, written)


# ----------------------------------------------------------------- decode attention ----

@pytest.fixture(scope="module")
def dec_cases():
    """The quantised caches of numerics.dec_inputs, computed once on the CPU."""
    out = {}
    for hd in N.DEC_HD:
        for Tmax in N.DEC_TMAX:
            for fam in N.DEC_FAMILIES:
                qkv, kc, vc = N.dec_inputs(hd, Tmax, fam)
                (k8, ks), (v8, vs) = Q.quant_cache(kc), Q.quant_cache(vc)
                out[hd, Tmax, fam] = tuple(t.to(DEV) for t in (qkv, k8, v8, ks, vs))
    return out


@pytest.mark.parametrize("fam", N.DEC_FAMILIES)
@pytest.mark.parametrize("Tmax", N.DEC_TMAX)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_decode_q8_bounds(C, dec_cases, hd, Tmax, fam):
    """The cases of test_decode_bounds_gpu.test_attn_decode_bounds on quantised caches.  Rows past
    each length hold NaN codes and NaN scales: the output must be finite, equal to the run with
    zeros there and to the run with contiguous q, and within the oracle's unit."""
    qkv, k8, v8, ks, vs = dec_cases[hd, Tmax, fam]
    scale = hd ** -0.5
    qc = qkv[:, : H * hd].contiguous()
    lens = N.dec_lengths(Tmax)
    tiles = {1: (hd, 8)}
    for la, lb in zip(lens, reversed(lens)):
        for pair in ((la, lb), (la, la)):
            rows = pair[0] != pair[1]
            ln = _i32(list(pair)) if rows else _i32([la])
            (kn, ksn), (vn, vsn) = Q.blank_past(k8, ks, pair, True), Q.blank_past(v8, vs, pair, True)
            (kz, ksz), (vz, vsz) = Q.blank_past(k8, ks, pair, False), Q.blank_past(v8, vs, pair, False)
            o = C._attn_decode_q8(qkv, kn, vn, ksn, vsn, ln, scale)
            assert o.shape == (B, H * hd) and o.dtype == torch.bfloat16
            what = f"attn_decode_q8 hd {hd} Tmax {Tmax} {fam} len {pair} {'rows' if rows else 'uniform'}"
            assert bool(torch.isfinite(o.float()).all()), what + ": read past a length"
            assert torch.equal(o, C._attn_decode_q8(qkv, kz, vz, ksz, vsz, ln, scale)), what
            assert torch.equal(o, C._attn_decode_q8(qc, kn, vn, ksn, vsn, ln, scale)), what + ": contiguous q"
            ref, unit = Q.ref_attn_decode_q8(qkv, kn, vn, ksn, vsn, _i32(list(pair)), scale)
            N.assert_within(o, ref, unit, N.DERIVED, what, tiles)


@pytest.mark.parametrize("Tmax,length", [(16, 7), (300, 257), (300, 305), (512, 511), (512, 512)])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_decode_q8_selects_the_key_exactly(C, hd, Tmax, length):
    """One key per (b, h) carries all the probability: o[b, h] == bf16(f32(v8[b, t*, h]) *
    vs[b, t*, h]) bit for bit, for per-row and uniform len."""
    qkv, kc, vc, tstar, ln = N.dec_selection_inputs(hd, Tmax, length)
    (k8, ks), (v8, vs) = Q.quant_cache(kc), Q.quant_cache(vc)
    lens = [length] * B
    deq = Q.dequant_bf16(v8, vs)
    want = torch.stack([deq[b, int(tstar[b, h]), h] for b in range(B) for h in range(H)]).view(B, H * hd).to(DEV)
    (kn, ksn), (vn, vsn) = Q.blank_past(k8.to(DEV), ks.to(DEV), lens, True), Q.blank_past(v8.to(DEV), vs.to(DEV), lens, True)
    ln = ln.to(DEV)
    for l in (ln, ln[:1].contiguous()):
        o = C._attn_decode_q8(qkv.to(DEV), kn, vn, ksn, vsn, l, hd ** -0.5)
        assert torch.equal(o, want), (hd, Tmax, length, l.numel(), tstar.tolist())


# ----------------------------------------------------------------- extend attention ----

EXT_TMAX = 160


@pytest.mark.parametrize("length,T", [(1, 33), (95, 40), (127, 33), (150, 20)])
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_attn_extend_q8_equals_the_bf16_kernel_on_dequantised_caches(C, hd, length, T):
    """_attn_extend_q8 == _attn_extend on bf16_rn(f32(code) * scale) caches, bit for bit: uniform
    len, per-row len, and n with a 0 and a partial row; (150, 20) runs past the capacity.  Padded
    q rows, unattended cache rows and their scales are NaN."""
    g = torch.Generator().manual_seed(81 + hd + length)
    kc = torch.randn(B, EXT_TMAX, H, hd, generator=g).bfloat16()
    vc = torch.randn(B, EXT_TMAX, H, hd, generator=g).bfloat16()
    kc[0, :, 1] *= (1 + 6 * torch.arange(EXT_TMAX).float() / EXT_TMAX).view(-1, 1).bfloat16()
    (k8, ks), (v8, vs) = Q.quant_cache(kc), Q.quant_cache(vc)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16()
    scale = hd ** -0.5
    for lens, n in (([length], None), ([length, max(length - 30, 0)], None), ([length, max(length - 30, 0)], [T - 7, 0]),
                    ([max(length - 30, 0), length], [T, T - 7])):
        ll = lens * B if len(lens) == 1 else lens
        nn = [T] * B if n is None else n
        q = qkv.clone().view(B, T, -1)
        k8n, v8n, ksn, vsn = _u8(k8).clone(), _u8(v8).clone(), ks.clone(), vs.clone()
        for b in range(B):
            live = max(0, min(nn[b], EXT_TMAX - ll[b]))
            q[b, live:] = NAN                                  # padded / cut-off queries
            k8n[b, ll[b] + live:], v8n[b, ll[b] + live:] = Q.NAN_CODE, Q.NAN_CODE
            ksn[b, ll[b] + live:], vsn[b, ll[b] + live:] = NAN, NAN
        k8n, v8n = k8n.view(Q.F8).to(DEV), v8n.view(Q.F8).to(DEV)
        ksn, vsn = ksn.to(DEV), vsn.to(DEV)
        q = q.view(B * T, -1).to(DEV)
        ln, nt = _i32(lens), None if n is None else _i32(n)
        o8 = C._attn_extend_q8(q, k8n, v8n, ksn, vsn, ln, nt, scale)
        ob = C._attn_extend(q, Q.dequant_bf16(k8n, ksn), Q.dequant_bf16(v8n, vsn), ln, nt, scale)
        what = (hd, length, T, lens, n)
        assert o8.shape == (B * T, H * hd) and bool(torch.isfinite(o8.float()).all()), what
        assert torch.equal(o8, ob), what
        assert any(bool((o8.view(B, T, -1)[b, :1] != 0).any()) for b in range(B) if nn[b] > 0 and ll[b] < EXT_TMAX), what


# ---------------------------------------------------------------------------- model ----

@pytest.fixture(scope="module")
def dist1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    yield
    destroy_dist_env()


@pytest.fixture(scope="module")
def model(dist1):
    from distributed_pytorch_from_scratch_amd.models import get_preset, Transformer
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m = Transformer.from_args(get_preset("gpt2-small", num_layers=2)).cuda()
    m.reset_parameters()
    m.eval()
    yield m
    G.clear_sessions()


@pytest.fixture(scope="module")
def cpu_model(model):
    """An fp32 CPU copy of the model: the full recompute the GPU logits are compared against."""
    from distributed_pytorch_from_scratch_amd.models import Transformer
    m = Transformer.from_args(model.args)
    m.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    m.eval()
    return m


def _prompt(m, nb, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, m.args.vocab_size, (nb, T), generator=g).cuda()


def _cache(m, nb, t_max, ragged=False, kv_dtype="fp8"):
    from distributed_pytorch_from_scratch_amd.models.generation import KVCache
    attn = m.layers[0].attn
    return KVCache(len(m.layers), nb, t_max, attn.num_local_heads, attn.head_dim, torch.bfloat16, torch.device("cuda"),
                   ragged=ragged, kv_dtype=kv_dtype)


def _full_cpu(cm, seq):
    seq = seq.cpu()
    with torch.inference_mode():
        return cm(seq.view(1, -1), torch.arange(seq.numel()).view(1, -1))[0, -1].float()


LIMIT = Q.KV8_LOGITS_REL + 3e-2     # the quantised cache's own error + bf16 kernels against the fp32 recompute


def test_fp8_cache_logits_against_the_cpu_recompute(model, cpu_model):
    """Whole prefill, prefill_chunk, and three decode steps on both caches, teacher-forced:
    rel(GPU fp8-cache logits, CPU full recompute) <= KV8_LOGITS_REL + 3e-2."""
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    nb = 2
    prompt = _prompt(model, nb, 70, 21)
    cw, cc = _cache(model, nb, 96), _cache(model, nb, 96)
    assert cw.nbytes() == len(model.layers) * 2 * nb * 96 * 12 * (64 + 4)
    assert sum(t.numel() * t.element_size() for t in cw.tensors()) == cw.nbytes()
    lw, lc = logits_step(model, prompt, cw), logits_step(model, prompt, cc, prefill_chunk=32)
    seq = prompt
    for step in range(4):
        for b in range(nb):
            full = _full_cpu(cpu_model, seq[b])
            rw, rc = N.rel(lw[b].cpu(), full), N.rel(lc[b].cpu(), full)
            print("step", step, "row", b, "whole vs cpu", rw, "chunked vs cpu", rc, "limit", LIMIT)
            assert rw <= LIMIT and rc <= LIMIT, (step, b, rw, rc)
        if step == 3:
            break
        nxt = lw.argmax(-1, keepdim=True)
        seq = torch.cat([seq, nxt], 1)
        lw, lc = logits_step(model, nxt, cw), logits_step(model, nxt, cc)
    assert cw.len == cc.len == 73


def test_fp8_cache_ragged_continuation_against_the_cpu_recompute(model, cpu_model):
    """Rows of 60, 37 and 1 cached ids take 20, 5 and 20 more in one right-padded step, then a
    decode step; the padding ids change nothing, bit for bit."""
    from distributed_pytorch_from_scratch_amd.models.generation import logits_step
    lens, more = [60, 37, 1], [20, 5, 20]
    ids = _prompt(model, 3, 80, 22)
    new = torch.stack([ids[b, n:n + 20] for b, n in enumerate(lens)])
    zero_pad, rand_pad = new.clone(), new.clone()
    for b, n in enumerate(more):
        zero_pad[b, n:] = 0
        rand_pad[b, n:] = _prompt(model, 1, 20 - n, 27 + b)[0]
    outs = []
    for pad in (zero_pad, rand_pad):
        c = _cache(model, 3, 96, ragged=True)
        logits_step(model, ids[:, :60].contiguous(), c, lens)
        outs.append(logits_step(model, pad, c, lens=more))
        assert c.lens == [80, 42, 21]
        outs.append(logits_step(model, outs[-1].argmax(-1, keepdim=True), c))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    seqs = [ids[b, :n + k] for b, (n, k) in enumerate(zip(lens, more))]
    for b, seq in enumerate(seqs):
        rel = N.rel(outs[0][b].cpu(), _full_cpu(cpu_model, seq))
        rel1 = N.rel(outs[1][b].cpu(), _full_cpu(cpu_model, torch.cat([seq, outs[0][b].argmax(-1, keepdim=True)])))
        print("row", b, "rel", rel, "next step", rel1, "limit", LIMIT)
        assert rel <= LIMIT and rel1 <= LIMIT, (b, rel, rel1)


def test_generate_fp8_eager_equals_graph_and_sessions(model, monkeypatch):
    """generate(kv_dtype="fp8"): eager tokens == graph tokens, uniform and prompt_lens, greedy and
    sampled, with the requested lengths; a bf16 generate after an fp8 one (and the reverse) each
    reuse their own session; the kept cache's bytes are layers * 2 * B * T_max * H * (hd + 4)."""
    from distributed_pytorch_from_scratch_amd.models import generation as G
    prompt = _prompt(model, 3, 40, 23)
    G.clear_sessions()
    for kw in ({}, dict(prompt_lens=[40, 17, 1])):
        for samp in ({}, dict(temperature=0.8, top_k=50, top_p=0.9, seed=3)):
            monkeypatch.setenv("DPFS_DECODE_GRAPH", "0")
            eager = G.generate(model, prompt, max_new_tokens=20, kv_dtype="fp8", **kw, **samp)
            monkeypatch.setenv("DPFS_DECODE_GRAPH", "1")
            graph = G.generate(model, prompt, max_new_tokens=20, kv_dtype="fp8", **kw, **samp)
            assert eager == graph, (kw, samp)
            assert [len(o) for o in graph] == [n + 20 for n in kw.get("prompt_lens", [40] * 3)]
    # sessions: uniform (3, 60) fp8, then bf16, then both again
    G.clear_sessions()
    G.generate(model, prompt, max_new_tokens=20, kv_dtype="fp8")
    (k8,) = G._SESSIONS
    s8 = G._SESSIONS[k8]
    assert k8[4] == "fp8" and s8["cache"].fp8
    attn = model.layers[0].attn
    assert s8["cache"].nbytes() == len(model.layers) * 2 * 3 * 60 * attn.num_local_heads * (attn.head_dim + 4)
    G.generate(model, prompt, max_new_tokens=20)
    assert len(G._SESSIONS) == 2
    (kb,) = [k for k in G._SESSIONS if k != k8]
    sb = G._SESSIONS[kb]
    assert kb[4] is None and not sb["cache"].fp8 and sb["cache"].k[0].dtype == torch.bfloat16
    n8, nb_ = len(s8["graphs"]), len(sb["graphs"])
    assert n8 >= 1 and nb_ >= 1
    a = G.generate(model, prompt, max_new_tokens=20, kv_dtype="fp8")
    b_ = G.generate(model, prompt, max_new_tokens=20)
    assert G._SESSIONS[k8] is s8 and G._SESSIONS[kb] is sb and len(s8["graphs"]) == n8 and len(sb["graphs"]) == nb_
    assert [len(o) for o in a] == [len(o) for o in b_] == [60] * 3
    G.clear_sessions()
