"""``_gemm_nt_w8a8`` (csrc/kernels/gemm_w8a8.hip) against fp64 on the same codes at the edges of its BM x 128 x 128
tile, every k position exact and in place, the fused SwiGLU quantiser's bytes, ``quantised_prefill="a8"`` on a model."""
import pytest
import torch

import numerics as N
import numerics_kv8 as Q
import numerics_w8 as W8

pytestmark = pytest.mark.gpu

from test_gemv_w8_gpu import C, DEV, _strided, model  # noqa: E402,F401  (the fp8 tests' fixtures and helper)
from distributed_pytorch_from_scratch_amd.ops import reference as R  # noqa: E402

BN, BK = 128, 128     # BM = 32 below 256 workgroups of 64 x 128 (the first five shapes), then 64 / 128 / 256
# Factor on the unit's accumulator term: 1 is the derived bound of an fp32 sum of K exact products in any order.  The
# fp8 MFMA's 128-product sum does not keep it: measured against fp64 over SHAPES, max (err - the other terms) / the term
# = 1.837 (M 2100 N 4000 K 128 with bias; <= 0.74 below 10^5 outputs); the factor is 2 x that measured worst excess.
ACC = 2 * 1.837

SHAPES = [
    (65, 100, 128),        # the first row count routed here: a ragged third row tile; N below one tile; one stage
    (33, 301, 384),        # M = BM + 1; three column tiles, the last ragged, odd N: the scalar stores; 3 stages = the ring
    (70, 256, 1152),       # whole column tiles; 9 stages: every slot three times
    (1, 136, 256),         # one row (every other row of the tile clamped); 2 stages: fewer than the ring's slots
    (17, 136, 128),        # 17 rows
    (1100, 1930, 128),     # 288 tiles of 64 rows, 144 of 128: the BM 64 launch, ragged both ways, N % 4 == 2
    (1990, 2100, 128),     # 272 tiles of 128 rows, 136 of 256: the BM 128 launch, ragged both ways, vector stores
    (2100, 4000, 128),     # 288 tiles of 256 rows: the BM 256 launch, ragged both ways
]


def ref_w8a8(xc, sa, codes, inv, bias):
    """(ref, unit) of y = bf16((xc codes^T) * sa * inv + bias), fp64 on the codes: the bf16 store, the fp32
    accumulator of K exact products scaled by sa inv, three fp32 roundings (two multiplies and the add)."""
    a64, c64, s64 = N.d(xc.view(Q.F8).float()), N.d(codes.view(Q.F8).float()), N.d(sa)[:, None] * N.d(inv)
    acc, mag = a64 @ c64.t(), a64.abs() @ c64.abs().t()
    b64 = N.d(bias) if bias is not None else torch.zeros_like(N.d(inv))
    ref = acc * s64 + b64
    return ref, N.U16 * ref.abs() + ACC * s64 * N.acc_term_gemm(mag, codes.size(1)) + \
        3 * N.U32 * ((acc * s64).abs() + b64.abs())


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,Nn,K", SHAPES)
def test_gemm_w8a8_bounds(C, M, Nn, K, bias):
    x, w, b = N.gemv_inputs(M, Nn, K)
    (xc, sa), (wc, inv) = R._quant_w8_rows(x), R._quant_w8_rows(w)
    ref, unit = ref_w8a8(xc, sa, wc, inv, b if bias else None)
    xc, sa, wc, inv, b = xc.to(DEV), sa.to(DEV), wc.to(DEV), inv.to(DEV), b.to(DEV) if bias else None
    y = C._gemm_nt_w8a8(xc, sa, wc, inv, b)
    what = f"gemm_w8a8 M {M} N {Nn} K {K} bias {bias}"
    print(what, "worst err/unit", N.worst_ratio(y.cpu(), ref, unit)[0])
    N.assert_within(y.cpu(), ref, unit, N.DERIVED, what, tiles={0: (256, 128, 64, 32, 16), 1: (BN, 64, 16)})
    assert torch.equal(C._gemm_nt_w8a8(xc, sa, wc, inv, b), y), what                      # run to run
    assert torch.equal(C._gemm_nt_w8a8(_strided(xc, 16), sa, _strided(wc, 16), inv, b), y), what


@pytest.mark.parametrize("M,Nn,K", [(144, 136, 256), (1100, 1930, 128), (1990, 2100, 128), (2100, 4000, 128)])
def test_every_k_exact_and_in_place(C, M, Nn, K):
    """One-hot A code rows (the code of 1.0, sa = 1) pick one k per row, in every row tile of the BM 32 / 64 /
    128 / 256 launches: y is that column of the dequantised weight, exactly (every byte of a stage row, every stage)."""
    ks = (torch.arange(M) * 37 + 5) % K
    assert {int(k) % BK for k in ks} == set(range(BK)) and {int(k) // BK for k in ks} == set(range(K // BK))
    xc = torch.zeros(M, K, dtype=torch.uint8)
    xc[torch.arange(M), ks] = 0x38
    table = torch.tensor([b for b in range(256) if b & 0x7F != Q.NAN_CODE], dtype=torch.uint8)
    codes = table[torch.arange(Nn * K) % 254].view(Nn, K)
    inv = torch.exp2((torch.arange(Nn) % 9 - 4).float())
    want = (codes.view(Q.F8).float() * inv[:, None]).bfloat16()       # (4 significant bits x 2^e: exact)
    y = C._gemm_nt_w8a8(xc.to(DEV), torch.ones(M, device=DEV), codes.to(DEV), inv.to(DEV), None)
    assert torch.equal(y.cpu(), want[:, ks].t())


@pytest.mark.parametrize("M,F", [(70, 256), (1, 128)])
def test_fused_swiglu_quantiser_bytes(C, M, F):
    gu = torch.randn(M, 2 * F, generator=torch.Generator().manual_seed(M + F)) * 3
    gu[M // 2] = 0                                                      # an all-zero row
    gu = gu.bfloat16().to(DEV)
    codes, inv = C._swiglu_quant_w8_rows(gu)
    want_c, want_i = C._quant_w8_rows(C.swiglu_fwd(gu))
    assert torch.equal(codes, want_c) and torch.equal(inv, want_i)


@pytest.mark.parametrize("B", [3, 70])
def test_model_a8_prefill(model, monkeypatch, B):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    p = W8.prompt(B).cuda()
    olds = [dict(), dict(weight_dtype="fp8", quantised_prefill=True)] + ([dict(weight_dtype="fp8")] if B <= 64 else [])
    before = [G.generate(model, p, 9, **kw) for kw in olds]
    cm = W8.tiny_model()       # the prompt, then one token, against the CPU oracle path on the same weight codes
    cm.load_state_dict({k: v.detach().bfloat16().float().cpu() for k, v in model.state_dict().items()})
    cg, cc = W8.cache(G, model, B, "cuda", torch.bfloat16), W8.cache(G, cm, B, "cpu", torch.float32)
    cg.wq_prefill = cc.wq_prefill = "a8"
    lg, lc = G.logits_step(model, p, cg), G.logits_step(cm, p.cpu(), cc)
    nxt = lg.argmax(-1, keepdim=True)                                    # (the CPU side is fed the GPU's id)
    rels = (N.rel(lg.cpu(), lc), N.rel(G.logits_step(model, nxt, cg).cpu(), G.logits_step(cm, nxt.cpu(), cc)))
    print("a8 batch", B, "rel(GPU logits, CPU oracle on the same codes): prefill, first step", rels)
    assert max(rels) <= 3e-2

    def refuse(*a, **k):
        raise AssertionError("a projection of an a8 session left its route")
    kw = dict(weight_dtype="fp8", quantised_prefill="a8", prefill_chunk=5, prompt_lens=[12 - b % 6 for b in range(B)])
    runs = {}
    with monkeypatch.context() as mp:
        for name in ("gemm_nt", "small_nt", "big_nt_w8"):
            mp.setattr(G.GS, name, refuse)
        for graph in ("1", "0"):
            mp.setenv("DPFS_DECODE_GRAPH", graph)
            runs[graph] = [G.generate(model, p, 9, **kw), G.generate(model, p, 9, kv_dtype="fp8", kv_page=16, **kw)]
    assert runs["1"] == runs["0"]
    assert [G.generate(model, p, 9, **kw) for kw in olds] == before     # the older sessions return what they did
