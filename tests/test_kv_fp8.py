"""The fp8 KV cache on the CPU: the row format (quantiser properties, the oracle of
``ops/reference.py`` against the independent quantiser of tests/numerics_kv8.py), the fp32
emulation of the fp8 decode attention against its fp64 oracle (within the derived unit at every
case of the GPU test; three planted scale faults are not), the model plumbing on the oracle path
(``KVCache(kv_dtype="fp8")``, ``logits_step``, ``generate``) with the measured logits error of
the quantised cache, and the argument checks."""
import pytest
import torch

import numerics as N
import numerics_kv8 as Q

from dist_helpers import run_distributed


# ------------------------------------------------------------------------ quantiser ----

def _u8(c):
    return c.view(torch.uint8)


def test_every_positive_finite_bf16_amax():
    """Rows (amax, -amax, amax / 3, 0 ...) for every positive finite bf16 amax: scale and inv are
    finite and non-zero, no NaN code (0x7f / 0xff) appears, and the amax element is +-448 wherever
    the 1e-12 floor is not in force."""
    bits = torch.arange(1, 0x7F80, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    rows = torch.zeros(bits.numel(), 8)
    rows[:, 0], rows[:, 1], rows[:, 2] = bits.float(), -bits.float(), bits.float() / 3
    rows = rows.bfloat16()
    codes, inv = Q.quant_rows(rows)
    assert bool(torch.isfinite(inv).all()) and bool((inv > 0).all())
    scale = 448.0 / rows.float().abs().amax(-1).clamp_min(1e-12)
    assert bool(torch.isfinite(scale).all()) and bool((scale > 0).all())
    assert float((rows.float()[:, 0] * scale).max()) <= 448.0001      # reaches 448.00003: the clamp is needed
    u = _u8(codes)
    assert not bool(((u & 0x7F) == 0x7F).any())
    big = bits.float() >= 1e-12
    assert bool((codes.float()[big, 0] == 448).all()) and bool((codes.float()[big, 1] == -448).all())


def test_zero_row_tie_row_outlier_row():
    hd = 32
    g = torch.Generator().manual_seed(3)
    x = torch.stack([torch.zeros(hd), Q.tie_row(hd), Q.outlier_row(hd, g)]).bfloat16()
    codes, inv = Q.quant_rows(x)
    assert bool((_u8(codes)[0] == 0).all()) and float(inv[0]) == pytest.approx(1e-12 / 448, rel=1e-6)
    assert float(inv[1]) == 1.0 and tuple(codes.float()[1, :6].tolist()) == Q.TIE_WANT
    # the outlier takes the whole range: it is exact, the unit-variance rest sits in the subnormals
    assert float(codes.float()[2, hd // 2]) == 448.0 and float(inv[2]) == pytest.approx(1024 / 448, rel=1e-6)


def test_value_error_bound_per_element():
    """|value - x| <= 2^-4 |x| + 2^-10 inv: three mantissa bits, and half the subnormal step
    (2^-9 in code units) for elements far below the row's amax."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(64, 3, 128, generator=g)
    x[:8] *= torch.logspace(-20, 20, 8).view(8, 1, 1)
    x[8, 0, 5] = 2.0 ** 10
    x[9] = 0
    x = x.bfloat16()
    codes, inv = Q.quant_rows(x)
    err = (Q.dequant64(codes, inv) - x.double()).abs()
    bound = 2.0 ** -4 * x.double().abs() + 2.0 ** -10 * inv.double()[..., None]
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def test_reference_quantiser_equals_the_helper_bit_for_bit():
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 3, 64, generator=g)
    x[:10] *= torch.logspace(-30, 30, 10).view(10, 1, 1)
    x[10, 0] = 0
    x[11, 0] = Q.tie_row(64)
    x[12, 0] = Q.outlier_row(64, g)
    bits = torch.arange(1, 0x7F80, 7, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    sweep = torch.zeros(bits.numel(), 8)
    sweep[:, 0], sweep[:, 3] = bits.float(), -bits.float() / 3
    for t in (x.bfloat16(), sweep.bfloat16()):
        c, i = R._kv_quant_rows(t)
        cq, iq = Q.quant_rows(t)
        assert c.dtype == Q.F8 and i.dtype == torch.float32 and i.shape == t.shape[:-1]
        assert torch.equal(_u8(c), _u8(cq)) and torch.equal(i.view(torch.int32), iq.view(torch.int32))


def test_reference_appends_and_attention_ops():
    """The oracle ops on the CPU: the chunk append writes exactly the live rows (codes and scales
    of the helper), the fused append is rope_ + the append, and the attention ops are the bf16
    oracle's on the dequantised caches."""
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    B, T, H, hd, Tmax = 2, 5, 3, 32, 12
    g = torch.Generator().manual_seed(6)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16()
    (k8, ks), (v8, vs) = (Q.quant_rows(torch.randn(B, Tmax, H, hd, generator=g).bfloat16()) for _ in range(2))
    ln, n = torch.tensor([2, 9], dtype=torch.int32), torch.tensor([5, 4], dtype=torch.int32)
    for b_, L in enumerate(ln.tolist()):                         # sentinels past the cached prefix
        _u8(k8)[b_, L:], _u8(v8)[b_, L:] = 0x55, 0x55
        ks[b_, L:], vs[b_, L:] = float("nan"), float("nan")
    before = [t.clone() for t in (k8, v8, ks, vs)]
    R._kv_append_chunk_q8(qkv, k8, v8, ks, vs, ln, n)
    rows = qkv.view(B, T, 3, H, hd)
    for b_, (L, m) in enumerate([(2, 5), (9, 3)]):                # row 1 is cut off at T_max
        for c8, cs, c0, part in ((k8, ks, before[0], 1), (v8, vs, before[1], 2)):
            cq, iq = Q.quant_rows(rows[b_, :m, part])
            assert torch.equal(_u8(c8)[b_, L:L + m], _u8(cq)) and torch.equal(cs[b_, L:L + m], iq)
            assert torch.equal(_u8(c8)[b_, :L], _u8(c0)[b_, :L]) and bool((_u8(c8)[b_, L + m:] == 0x55).all())
            assert bool(torch.isfinite(cs[b_, :L]).all()) and bool(torch.isnan(cs[b_, L + m:]).all())
    o = R._attn_extend_q8(qkv, k8, v8, ks, vs, ln, n, hd ** -0.5)
    want = R._attn_extend(qkv, k8.float() * ks[..., None], v8.float() * vs[..., None], ln, n, hd ** -0.5)
    assert torch.equal(o, want) and bool(torch.isfinite(o.float()).all())
    # fused single-token append at per-row lengths 7 and 12 (full: nothing written), then decode
    tab = N.rope_table(16, hd)
    pos = torch.tensor([7, 11])
    q1 = torch.randn(B, 3 * H * hd, generator=g).bfloat16()
    ln1 = torch.tensor([7, 12], dtype=torch.int32)
    a, a2 = q1.clone(), q1.clone()
    before = _u8(k8).clone()
    R._rope_append_q8(a, pos, tab, k8, v8, ks, vs, ln1)
    R.rope_(a2, pos, tab, 2 * H, hd, False)
    assert torch.equal(a, a2)
    cq, iq = Q.quant_rows(a[0, H * hd: 2 * H * hd].view(H, hd))
    assert torch.equal(_u8(k8)[0, 7], _u8(cq)) and torch.equal(ks[0, 7], iq)
    assert torch.equal(_u8(k8)[1], before[1])
    od = R._attn_decode_q8(a, k8, v8, ks, vs, ln1, hd ** -0.5)
    kz, vz = torch.nan_to_num(k8.float() * ks[..., None]), torch.nan_to_num(v8.float() * vs[..., None])
    assert torch.equal(od, R.attn_decode(a, kz, vz, ln1, hd ** -0.5)) and bool(torch.isfinite(od.float()).all())


# ------------------------------------------------------------------------ emulation ----

@pytest.mark.parametrize("fam", N.DEC_FAMILIES)
@pytest.mark.parametrize("Tmax", N.DEC_TMAX)
@pytest.mark.parametrize("hd", N.DEC_HD)
def test_fp8_decode_emulation_within_its_unit(hd, Tmax, fam):
    """The cases of test_kv_fp8_gpu.test_attn_decode_q8_bounds: an fp32 evaluation of the kernel's
    scheme stays within the derived unit, so a correct kernel can."""
    qkv, kc, vc = N.dec_inputs(hd, Tmax, fam)
    (k8, ks), (v8, vs) = Q.quant_cache(kc), Q.quant_cache(vc)
    lens = N.dec_lengths(Tmax)
    for la, lb in zip(lens, reversed(lens)):
        for pair in ((la, lb), (la, la)):
            ln = torch.tensor(pair, dtype=torch.int32)
            kn, ksn = Q.blank_past(k8, ks, pair, True)
            vn, vsn = Q.blank_past(v8, vs, pair, True)
            ref, unit = Q.ref_attn_decode_q8(qkv, kn, vn, ksn, vsn, ln, hd ** -0.5)
            out = Q.emu_attn_decode_q8(qkv, kn, vn, ksn, vsn, ln, hd ** -0.5)
            N.assert_within(out, ref, unit, N.DERIVED, f"decode q8 hd {hd} Tmax {Tmax} {fam} len {pair}", {1: (hd, 8)})


@pytest.mark.parametrize("fault", Q.KV8_FAULTS)
def test_fp8_decode_scale_faults_are_caught(fault):
    """One (sequence, head) with a wrong scale: the K scale ignored, the V scale of the
    neighbouring key, both scales of the next head.  The per-element bound names the sequence."""
    hd, Tmax = 64, 300
    qkv, kc, vc = N.dec_inputs(hd, Tmax, "rising")
    (k8, ks), (v8, vs) = Q.quant_cache(kc), Q.quant_cache(vc)
    ln = torch.tensor([299, 257], dtype=torch.int32)
    ref, unit = Q.ref_attn_decode_q8(qkv, k8, v8, ks, vs, ln, hd ** -0.5)
    N.assert_within(Q.emu_attn_decode_q8(qkv, k8, v8, ks, vs, ln, hd ** -0.5), ref, unit, N.DERIVED, "no fault")
    for b, h in [(0, 0), (1, 2)]:
        bad = Q.emu_attn_decode_q8(qkv, k8, v8, ks, vs, ln, hd ** -0.5, fault=(fault, b, h))
        with pytest.raises(AssertionError, match=rf"at \({b}, "):
            N.assert_within(bad, ref, unit, N.DERIVED, fault, {1: (hd, 8)})


def test_fp8_decode_key_selection_is_exact_in_fp32():
    hd, Tmax, B, H = 64, 300, 2, 3
    qkv, kc, vc, tstar, ln = N.dec_selection_inputs(hd, Tmax, 299)
    (k8, ks), (v8, vs) = Q.quant_cache(kc), Q.quant_cache(vc)
    out = Q.emu_attn_decode_q8(qkv, k8, v8, ks, vs, ln, hd ** -0.5)
    deq = Q.dequant_bf16(v8, vs)
    want = torch.stack([deq[b, tstar[b, h], h] for b in range(B) for h in range(H)]).view(B, H * hd)
    assert torch.equal(out, want)


# ------------------------------------------------------------------- model plumbing ----

LENS = [7, 3]
MORE = [4, 2]


def _tiny_model():
    """The small model of tests/test_chunked_prefill.py with two heads, so head_dim is 32."""
    from distributed_pytorch_from_scratch_amd.models import ModelArgs, Transformer
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    args = ModelArgs(attn_dim=64, ffn_dim=128, num_heads=2, num_layers=2, vocab_size=96, maxlen=64, vocab_pad_to=1)
    m = Transformer.from_args(args)
    set_seed(0)
    m.reset_parameters()
    m.eval()
    g = torch.Generator().manual_seed(5)
    return m, torch.randint(3, 96, (2, 12), generator=g)


def _plumbing(rank, world):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, ids = _tiny_model()
    dev = torch.device("cpu")
    new = lambda kd, ragged=False: G.KVCache(2, 2, 24, 2, 32, torch.float32, dev, ragged=ragged, kv_dtype=kd)
    c8 = new("fp8")
    assert c8.fp8 and c8.k[0].dtype == torch.float8_e4m3fn and c8.ks[0].shape == (2, 24, 2) and len(c8.ks) == 2
    assert c8.nbytes() == 2 * 2 * 2 * 24 * 2 * (32 + 4)
    ca = new(None)
    assert not ca.fp8 and ca.k[0].dtype == torch.float32 and not hasattr(ca, "ks")
    e = {}

    def both(name, fn):
        """fn(cache dtype) -> list of logits; the relative error of every one against the exact cache."""
        exact, quant = fn(None), fn("fp8")
        for i, (a, b) in enumerate(zip(quant, exact)):
            e[f"{name}[{i}]"] = N.rel(a, b)

    def whole(kd):          # whole prefill (attends the fresh q / k / v), then two decode steps
        c = new(kd)
        out = [G.logits_step(m, ids, c)]
        for t in (5, 9):
            out.append(G.logits_step(m, torch.full((2, 1), t), c))
        assert c.len == 14
        return out

    def chunked(kd):        # pieces of 3: every piece after the first reads the quantised prefix
        c = new(kd)
        out = [G.logits_step(m, ids, c, prefill_chunk=3)]
        out.append(G.logits_step(m, torch.full((2, 1), 5), c))
        return out

    def ragged(kd):         # rows of 7 and 3 ids, then 4 and 2 more, then a decode step
        c = new(kd, True)
        out = [G.logits_step(m, ids[:, :7].contiguous(), c, LENS)]
        more = torch.stack([ids[0, 7:11], torch.cat([ids[1, 3:5], ids[1, :2]])])
        out.append(G.logits_step(m, more, c, lens=MORE))
        assert c.lens == [11, 5]
        out.append(G.logits_step(m, torch.full((2, 1), 9), c))
        return out

    both("whole", whole)
    both("chunked", chunked)
    both("ragged", ragged)
    e_whole0 = e.pop("whole[0]")
    e_ragged0 = e.pop("ragged[0]")
    # generate: its tokens are the argmax of logits_step on an fp8 cache along the same ids, and
    # the logits error along the generated sequence joins the maximum
    p = ids[:, :7].contiguous()
    gen = {}
    for name, kw in (("uniform", {}), ("ragged", dict(prompt_lens=LENS))):
        G.clear_sessions()
        toks = G.generate(m, p, 6, kv_dtype="fp8", **kw)
        lens = kw.get("prompt_lens", [7, 7])
        gen[name] = [len(t) for t in toks]
        assert all(t[:n] == p[b, :n].tolist() for b, (t, n) in enumerate(zip(toks, lens)))
        cq, cx = new("fp8", name == "ragged"), new(None, name == "ragged")
        lk = dict(lens=lens) if name == "ragged" else {}
        lq, lx = G.logits_step(m, p, cq, **lk), G.logits_step(m, p, cx, **lk)
        for s in range(6):
            nxt = torch.tensor([[toks[b][lens[b] + s]] for b in range(2)])
            assert lq.argmax(-1).view(-1).tolist() == nxt.view(-1).tolist(), (name, s)
            if s:
                e[f"gen_{name}[{s}]"] = N.rel(lq, lx)
            if s < 5:
                lq, lx = G.logits_step(m, nxt, cq), G.logits_step(m, nxt, cx)
    G.clear_sessions()
    errs = {}
    for bad in ("bf16", "int8", ""):
        try:
            new(bad)
        except ValueError as ex:
            errs[bad] = str(ex)
    try:
        G.KVCache(2, 2, 24, 4, 16, torch.float32, dev, kv_dtype="fp8")
    except ValueError as ex:
        errs["hd16"] = str(ex)
    try:
        G.generate(m, p, 2, kv_dtype="e5m2")
    except ValueError as ex:
        errs["generate"] = str(ex)
    return {"e": e, "e_whole0": e_whole0, "e_ragged0": e_ragged0, "gen": gen, "errs": errs}


@pytest.fixture(scope="module")
def plumbing():
    return run_distributed(_plumbing, 1)[0]


def test_model_logits_error_of_the_fp8_cache(plumbing):
    """fp8-cache logits against exact-cache logits (relative Frobenius error, fp32 CPU math) for
    a whole prefill + decode steps, a chunked prefill, a ragged continuation and along generated
    sequences, uniform and ragged.  The maximum is the recorded ``KV8_LOGITS_REL``."""
    e = plumbing["e"]
    for k, v in sorted(e.items()):
        print(f"e_q {k}: {v:.4g}")
    worst = max(e.values())
    print("max e_q", worst, "recorded", Q.KV8_LOGITS_REL)
    assert 0 < worst <= Q.KV8_LOGITS_REL
    # the whole-prompt prefill attends its own unquantised keys and values: no error at all
    assert plumbing["e_whole0"] == 0 and plumbing["e_ragged0"] == 0


def test_generate_lengths_and_value_errors(plumbing):
    assert plumbing["gen"] == {"uniform": [13, 13], "ragged": [13, 9]}
    errs = plumbing["errs"]
    assert set(errs) == {"bf16", "int8", "", "hd16", "generate"}
    assert all("kv_dtype" in v for v in errs.values()) and "head_dim" in errs["hd16"]


def test_kv_cache_dtype_cli_flag():
    from distributed_pytorch_from_scratch_amd.evaluate import get_test_args, main
    base = ["--data_path", "d", "--ckpt_dir", "c"]
    assert get_test_args(base).kv_cache_dtype == "act"
    assert get_test_args(base + ["--kv_cache_dtype", "fp8"]).kv_cache_dtype == "fp8"
    with pytest.raises(SystemExit):
        get_test_args(base + ["--kv_cache_dtype", "int4"])
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        main(base + ["--kv_cache_dtype", "fp8", "--no_kv_cache"])
