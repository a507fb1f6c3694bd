"""MXFP4 projection weights on the CPU oracle path: the oracle quantiser on the edge inputs, the
refusals, every projection routed through the codes, the measured logits error."""
import pytest
import torch

import numerics as N
import numerics_w4 as W4
import numerics_w8 as W8

from dist_helpers import run_distributed


def test_oracle_quantiser_on_the_edge_inputs():
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    w = W4.quant_inputs(37, 640)
    codes, scales = R._quant_w4_rows(w)
    assert codes.dtype == scales.dtype == torch.uint8 and codes.shape == (37, 320) and scales.shape == (37, 20)
    nib = torch.stack((codes & 15, codes >> 4), -1).flatten(1)
    for r0, blk in ((0, 0), (5, 19)):     # zeros, subnormals, bf16 maximum, amax 4, ties: scales, then the tie codes
        assert scales[r0:r0 + 5, blk].tolist() == [2, 2, 252, 127, 124]
        assert not nib[r0, 32 * blk:32 * blk + 32].any()
        assert nib[r0 + 4, 32 * blk:32 * blk + 18].tolist() == W4.TIE_CODES + [c | 8 for c in W4.TIE_CODES]
    # as near as the nearest e2m1 point of the scaled weight (randn rows), saturating; requantising is the identity
    wq = R._dequant_w4(codes, scales)
    assert torch.equal(wq.double(), W4.dequant64(codes, scales)) and torch.equal(wq, wq.bfloat16().float())
    q = (w.double() / torch.exp2(scales.double() - 127).repeat_interleave(32, 1))[10:]
    grid = torch.tensor(W4.E2M1, dtype=torch.float64)
    qc = q.abs().clamp_max(6)
    assert torch.equal((grid[(nib[10:] & 7).long()] - qc).abs(), (qc[..., None] - grid).abs().amin(-1))
    assert torch.equal(nib[10:] >> 3, (w[10:] < 0).to(torch.uint8))
    assert all(torch.equal(a, b) for a, b in zip(R._quant_w4_rows(wq), (codes, scales)))


def _plumbing(rank, world):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.models.engine_common import _Layer
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    m, md, p = W8.tiny_model(), W8.tiny_model(), W8.prompt(3)
    with torch.no_grad():                   # md: every coded projection weight replaced by its dequantised value
        ws = [w for L in map(_Layer, md.layers) for w in (L.wqkv, L.wo, L.wgu, L.wd)] + [md.lm_head.weight]
        for w in ws:                        # (a shard whose K is no multiple of 128, Wo at two ranks, has no codes)
            if w.size(1) % 128 == 0:
                w.copy_(R._dequant_w4(*R._quant_w4_rows(w)))
    # the first decode step after the exact-weight prefill of m: m on its codes, md and m on their weights
    step = {}
    for name, mm, fmt in (("w4", m, "mxfp4"), ("deq", md, None), ("act", m, None)):
        c = W8.cache(G, m, 3, "cpu", torch.float32, False)
        c.w4 = G.quantise_weights(m, "cpu", fmt) if fmt else None
        G.logits_step(m, p, c)
        step[name] = G.logits_step(mm, torch.full((3, 1), 5), c)
    kw = dict(prompt_lens=[12, 7, 9], kv_dtype="fp8", temperature=[0.0, 0.8, 1.0], seed=3)
    out = {"routed": torch.equal(step["w4"], step["deq"]), "rel": N.rel(step["w4"], step["act"]),
           "coded": len(G.quantise_weights(m, "cpu", "mxfp4")),
           # on md quantisation is the identity, prefill included: the same tokens with and without the codes
           "tokens": [G.generate(md, p, 6, weight_dtype=wd, **k) for wd in ("mxfp4", None) for k in ({}, kw)],
           "errs": {}}
    m.set_compute_dtype(torch.float32)
    for name, mm, B in (("batch", W8.tiny_model(), 65), ("norm", W8.tiny_model("layernorm"), 3), ("fp32", m, 3),
                        ("dtype", W8.tiny_model(), 3)):
        with pytest.raises(ValueError) as ex:
            G.generate(mm, W8.prompt(B), 2, weight_dtype="int4" if name == "dtype" else "mxfp4")
        out["errs"][name] = str(ex.value)
    return out


@pytest.fixture(scope="module")
def plumbing():
    return run_distributed(_plumbing, 1)[0]


@pytest.fixture(scope="module")
def plumbing_tp2():
    return run_distributed(_plumbing, 2)


def test_every_projection_runs_on_the_codes(plumbing):
    assert plumbing["coded"] == 9
    t = plumbing["tokens"]
    assert plumbing["routed"] and t[0] == t[2] and t[1] == t[3] and [len(r) for r in t[1]] == [18, 13, 15]
    print("rel(MXFP4-weight logits, exact-weight logits), first decode step:", plumbing["rel"])   # reported, no threshold
    assert 0 < plumbing["rel"] < 1


def test_two_ranks_agree(plumbing_tp2, plumbing):
    """One local head per rank: Wo (K 64) keeps its bf16 weights, the other seven projections run on their
    shard's codes, and both ranks return the same tokens."""
    a, b = plumbing_tp2[0], plumbing_tp2[1]
    assert a["coded"] == b["coded"] == 7 and a["routed"] and b["routed"]
    assert a["tokens"] == b["tokens"] and a["rel"] == b["rel"] and 0 < a["rel"] < 1
    t = a["tokens"]
    assert t[0] == t[2] and t[1] == t[3] and [len(r) for r in t[1]] == [18, 13, 15]
    assert a["errs"] == b["errs"] == plumbing["errs"]


def test_refusals(plumbing):
    e = plumbing["errs"]
    assert "64" in e["batch"] and "RMSNorm" in e["norm"] and "fp32" in e["fp32"] and "mxfp4" in e["dtype"]
