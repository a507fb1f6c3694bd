"""The serving path at TP 2 and 4 on the CPU oracle path (gloo, fp32): every cache and weight format of
``generate`` on the tiny model of tests/numerics_tp.py, whose local shapes land on and off the K multiples
of the quantised-weight kernels.  Every rank must return the same tokens (a rank that picks another token
desynchronises the collectives of a real node), the forms without weight codes must return the TP 1 tokens
(fp32: only the order of the row-parallel sums differs), ``quantise_weights`` must code exactly the
projections whose local K allows it, and a model whose coded shards hold their dequantised values must
decode the same tokens with and without the codes.

Inputs checked for near-ties that flip a token between TP 1 and TP k: model seed 0, prompt seed 5, sampling
seed 3, at heads 2 and 3 over two ranks and heads 6 over four: none flips."""
import pytest
import torch

import numerics_tp as TP

from dist_helpers import run_distributed

FORMATS = ("fp8", "mxfp4")
TWIN_KW = ({}, dict(kv_dtype="fp8", **TP.ROWS))


def _dequantised_twin(R, heads, weight_dtype):
    """The rank's model with every shard that ``weight_dtype`` codes replaced by its dequantised value (the
    other shards, a K 64 Wo under MXFP4 for one, keep the bf16 route and their exact weights)."""
    md = TP.tp_model(heads)
    names = TP.coded(md, weight_dtype)
    with torch.no_grad():
        for name, w in TP.projections(md):
            if name not in names:
                continue
            if weight_dtype == "mxfp4":
                w.copy_(R._dequant_w4(*R._quant_w4_rows(w)))
            else:
                codes, inv = R._quant_w8_rows(w)
                w.copy_(codes.view(torch.float8_e4m3fn).float() * inv[:, None])
    return md


def _serve(rank, world, heads):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    m, p = TP.tp_model(heads), TP.prompt()
    out = {"gen": {name: G.generate(m, p, TP.NEW, **kw) for name, kw in TP.MATRIX},
           "coded": {wd: (TP.coded_names(m, G.quantise_weights(m, "cpu", wd)), TP.coded(m, wd)) for wd in FORMATS},
           "local": (m.layers[0].attn.num_local_heads, m.lm_head.weight.size(0))}
    if world == 2:      # on the twin quantisation is the identity, prefill included
        out["twin"] = {wd: [G.generate(md, p, TP.NEW, weight_dtype=w, **kw) for w in (wd, None) for kw in TWIN_KW]
                       for wd in FORMATS for md in (_dequantised_twin(R, heads, wd),)}
    return out


@pytest.fixture(scope="module")
def single():
    return {heads: run_distributed(_serve, 1, heads)[0] for heads in sorted({h for _, h in TP.WORLD_HEADS})}


@pytest.fixture(scope="module", params=TP.WORLD_HEADS, ids=lambda wh: f"tp{wh[0]}-heads{wh[1]}")
def ranks(request):
    world, heads = request.param
    return world, heads, run_distributed(_serve, world, heads)


def test_every_rank_returns_the_same_tokens(ranks):
    world, heads, res = ranks
    assert sorted(res) == list(range(world))
    for name, _ in TP.MATRIX:
        for r in range(1, world):
            assert res[r]["gen"][name] == res[0]["gen"][name], (name, r)     # "pen": tokens and log-probs
    toks, lps = res[0]["gen"]["pen"]
    assert [len(t) for t in toks] == [TP.T + TP.NEW] * TP.B and [len(r) for r in lps] == [TP.NEW] * TP.B
    assert [len(t) for t in res[0]["gen"]["all"]] == [n + TP.NEW for n in TP.ROWS["prompt_lens"]]


def test_uncoded_forms_return_the_single_rank_tokens(ranks, single):
    world, heads, res = ranks
    for name, _ in TP.MATRIX:
        if name in TP.CODED:
            continue
        got, want = res[0]["gen"][name], single[heads]["gen"][name]
        if name == "pen":       # the ids exactly; the fp32 log-probabilities to the order of the sums
            assert got[0] == want[0]
            assert torch.allclose(torch.tensor(got[1]), torch.tensor(want[1]), rtol=0, atol=1e-4)
        else:
            assert got == want, name


def test_paged_and_contiguous_tokens_agree(ranks, single):
    world, heads, res = ranks
    for gen in [r["gen"] for r in res.values()] + [single[heads]["gen"]]:
        assert gen["paged"] == gen["plain"] and gen["kv8_paged"] == gen["kv8"]


def test_quantise_weights_codes_what_the_local_shapes_allow(ranks, single):
    world, heads, res = ranks
    for w, rs in ((world, res), (1, {0: single[heads]})):
        for wd in FORMATS:
            for r in range(w):
                got, want = rs[r]["coded"][wd]
                assert got == want, (wd, w, heads, r)
            assert [len(rs[r]["coded"][wd][0]) for r in range(w)] == TP.CODED_COUNTS[wd][(w, heads)], (wd, w, heads)
    if (world, heads) == (2, 3):    # the mixed step: rank 0's Wo on MXFP4 codes, rank 1's on bf16
        assert "0.wo" in res[0]["coded"]["mxfp4"][0] and "0.wo" not in res[1]["coded"]["mxfp4"][0]
        assert [res[r]["local"] for r in range(2)] == [(2, 48), (1, 49)]


def test_dequantised_twin_decodes_the_same_with_and_without_codes(ranks):
    world, heads, res = ranks
    if world != 2:
        return      # (the identity is per rank: two ranks show it at every local shape of the table)
    for wd in FORMATS:
        for r in range(world):
            t = res[r]["twin"][wd]
            assert t[0] == t[2] and t[1] == t[3], (wd, r)
            assert t == res[0]["twin"][wd], (wd, r)
            assert [len(x) for x in t[1]] == [n + TP.NEW for n in TP.ROWS["prompt_lens"]]
