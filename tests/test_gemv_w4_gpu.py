"""MXFP4 projection weights on the MI355X (csrc/kernels/gemv_w4.hip): the quantiser bit for bit, every
code exact and in place, ``_gemv_nt_w4`` within its derived unit (tests/numerics_w4.py) on both launch
forms, every M tile count, full and shortened batches, and ``generate(..., weight_dtype="mxfp4")`` on a tiny
model."""
import pytest
import torch

import numerics as N
import numerics_w4 as W4
import numerics_w8 as W8

pytestmark = pytest.mark.gpu

from test_gemv_w8_gpu import C, DEV, _strided, model  # noqa: E402,F401  (the fp8 tests' fixtures and helper)
from distributed_pytorch_from_scratch_amd.ops import reference as R  # noqa: E402


@pytest.mark.parametrize("Nn,K,strided", [(100, 128, False), (37, 640, False), (48, 3072, True)])
def test_quantiser_bytes(C, Nn, K, strided):
    w = W4.quant_inputs(Nn, K)
    cq, sq = R._quant_w4_rows(w)
    codes, scales = C._quant_w4_rows(_strided(w.to(DEV), 64) if strided else w.to(DEV))
    assert codes.dtype == scales.dtype == torch.uint8 and codes.is_contiguous() and scales.is_contiguous()
    assert torch.equal(codes.cpu(), cq) and torch.equal(scales.cpu(), sq)


@pytest.mark.parametrize("M", [16, 64])
def test_every_code_exact_and_in_place(C, M):
    """One-hot A rows walk over every k, M at a time, so y is the whole dequantised weight: both nibbles,
    every word, all four lane groups, K-wave slices of 15 quads (the last: 8), full and shortened
    batches (8 + 7 at M 16; 4 + 4 + 4 + 3 at M 64).  Bytes cycle through all 256 values, scales 2^-8 .. 2^8."""
    Nn, K = 48, 113 * 128
    codes = (torch.arange(Nn * K // 2) * 37 % 256).to(torch.uint8).view(Nn, K // 2).to(DEV)
    scales = (119 + torch.arange(Nn * K // 32) % 17).to(torch.uint8).view(Nn, K // 32).to(DEV)
    rows = torch.arange(M, device=DEV)
    ys = []
    for k0 in range(0, K, M):
        x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        x[rows, k0 + rows] = 1.0
        ys.append(C._gemv_nt_w4(x, codes, scales))
    assert torch.equal(torch.cat(ys).double(), W4.dequant64(codes, scales).t())


# (100, 128): one block per lane, idle K-waves, ragged N; (37, 640): 5 quads over 4 K-waves, 2 / 2 / 1 / 0;
# (48, 3072): the 8 K-wave form, 3 quads each; (8200, 1024): more than 512 column tiles, the wide-N
# form, ragged N; (32, 7680): K-waves of 8 quads and one of 4, the full 8-quad batch of M <= 16; (49, 128): the
# ragged lm_head shard of a tensor-parallel rank (97 ids over 2 ranks): one row in the last column tile
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 64])
@pytest.mark.parametrize("Nn,K", [(100, 128), (37, 640), (48, 3072), (8200, 1024), (32, 7680), (49, 128)])
def test_gemv_w4_bounds(C, Nn, K, M, bias):
    for sw in (False, True) if (Nn, K) in ((37, 640), (48, 3072)) else (False,):
        x, w, b = N.gemv_inputs(M, Nn, K, sw)
        codes, scales = (t.to(DEV) for t in R._quant_w4_rows(w))
        x, b = x.to(DEV), b.to(DEV) if bias else None
        y = C._gemv_nt_w4(x, codes, scales, b, sw)
        ref, unit = W4.ref_w4(x, codes, scales, b, sw)
        what = f"gemv_w4 N {Nn} K {K} M {M} bias {bias} swiglu {sw}"
        print(what, "worst err/unit", N.worst_ratio(y, ref, unit)[0])
        N.assert_within(y, ref, unit, N.DERIVED, what, tiles={0: (16,), 1: (32, 16)})
        assert torch.equal(C._gemv_nt_w4(x, codes, scales, b, sw), y), what         # run to run
        assert torch.equal(C._gemv_nt_w4(_strided(x, 8), _strided(codes, 16), _strided(scales, 4), b, sw), y), what


@pytest.mark.parametrize("B", [3, 20])
def test_model_mxfp4_weights(model, monkeypatch, B):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    p = W8.prompt(B).cuda()
    # the first decode step's logits against the CPU oracle path on the same quantised weights
    cm = W8.tiny_model()
    cm.load_state_dict({k: v.detach().bfloat16().float().cpu() for k, v in model.state_dict().items()})
    cg, cc = W8.cache(G, model, B, "cuda", torch.bfloat16, False), W8.cache(G, cm, B, "cpu", torch.float32, False)
    cg.w4, cc.w4 = G.quantise_weights(model, "cuda", "mxfp4"), G.quantise_weights(cm, "cpu", "mxfp4")
    assert len(cg.w4) == 9 and all(torch.equal(a[j].cpu(), b[j]) for a, b in zip(cg.w4.values(), cc.w4.values())
                                   for j in (0, 1))
    nxt = G.logits_step(model, p, cg).argmax(-1, keepdim=True)          # (the CPU side is fed the GPU's id)
    G.logits_step(cm, p.cpu(), cc)
    rel = N.rel(G.logits_step(model, nxt, cg).cpu(), G.logits_step(cm, nxt.cpu(), cc))
    print("batch", B, "rel(GPU MXFP4-weight logits, CPU oracle on the same codes)", rel)
    assert rel <= 3e-2
    # graph and eager path: identical tokens, greedy, per-row sampling, and with the paged fp8 cache
    runs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("DPFS_DECODE_GRAPH", graph)
        none = G.generate(model, p, 9)
        runs[graph] = [G.generate(model, p, 9, weight_dtype="mxfp4", **kw) for kw in (
            {}, dict(temperature=[0.0, 0.7, 1.0] + [0.9] * (B - 3), top_k=20, seed=list(range(B))),
            dict(kv_dtype="fp8", kv_page=16))]
        assert graph == "0" or any(k[-1] == ("weights", "mxfp4") for k in G._SESSIONS)
        assert G.generate(model, p, 9) == none                  # sessions do not leak into the bf16 path
    assert runs["1"] == runs["0"]
