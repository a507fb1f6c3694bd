"""fp8 projection weights on the CPU oracle path: the oracle quantiser against tests/numerics_kv8.py,
``generate``, the refusals, re-quantisation after a weight changes, the measured logits error."""
import pytest
import torch

import numerics as N
import numerics_kv8 as Q
import numerics_w8 as W8

from dist_helpers import run_distributed


def test_reference_quantiser_equals_the_helper_bit_for_bit():
    from distributed_pytorch_from_scratch_amd.ops import reference as R
    w = torch.randn(37, 576, generator=torch.Generator().manual_seed(1))
    w[0], w[1, 7] = 0, torch.finfo(torch.bfloat16).max
    codes, inv = R._quant_w8_rows(w.bfloat16())
    cq, iq = Q.quant_rows(w.bfloat16())
    assert codes.dtype == torch.uint8 and codes.shape == (37, 576) and inv.shape == (37,)
    assert torch.equal(codes, cq.view(torch.uint8)) and torch.equal(inv.view(torch.int32), iq.view(torch.int32))


def _plumbing(rank, world):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, p = W8.tiny_model(), W8.prompt(3)
    out = {"act": G.generate(m, p, 6), "fp8": G.generate(m, p, 6, weight_dtype="fp8", prompt_lens=[12, 7, 9],
                                                          kv_dtype="fp8", temperature=[0.0, 0.8, 1.0], seed=3)}
    # the first decode step's logits, teacher-forced, on both weight forms (the prefill keeps bf16 weights)
    step = {}
    for fp8 in (False, True):
        c = W8.cache(G, m, 3, "cpu", torch.float32, fp8)
        G.logits_step(m, p, c)
        step[fp8] = G.logits_step(m, torch.full((3, 1), 5), c)
    out["rel"] = N.rel(step[True], step[False])
    # a weight changed in place: the next call quantises it again and its log-probabilities follow
    lp = lambda: G.generate(m, p, 3, weight_dtype="fp8", return_logprobs=True)[1]
    before = lp()
    with torch.no_grad():
        m.lm_head.weight.mul_(3.0)
    c = W8.cache(G, m, 3, "cpu", torch.float32)
    G.logits_step(m, p, c)
    first = torch.tensor([r[12] for r in G.generate(m, p, 1)])
    want = torch.log_softmax(G.logits_step(m, first.view(3, 1), c), -1).max(-1).values
    out["requant"] = (before, lp(), want.tolist())
    errs = {}
    m.set_compute_dtype(torch.float32)
    for name, mm, B in (("batch", W8.tiny_model(), 65), ("norm", W8.tiny_model("layernorm"), 3), ("fp32", m, 3),
                        ("dtype", W8.tiny_model(), 3)):
        with pytest.raises(ValueError) as ex:
            G.generate(mm, W8.prompt(B), 2, weight_dtype="int4" if name == "dtype" else "fp8")
        errs[name] = str(ex.value)
    out["errs"] = errs
    return out


@pytest.fixture(scope="module")
def plumbing():
    return run_distributed(_plumbing, 1)[0]


def test_generate_runs_on_the_oracle_path(plumbing):
    assert [len(t) for t in plumbing["act"]] == [18] * 3 and [len(t) for t in plumbing["fp8"]] == [18, 13, 15]
    print("rel(fp8-weight logits, bf16-weight logits), first decode step:", plumbing["rel"])   # reported, no threshold
    assert 0 < plumbing["rel"] < 1


def test_a_changed_weight_is_quantised_again(plumbing):
    before, after, want = plumbing["requant"]
    got = [r[1][0] for r in after]                  # the second id is the first decode step's
    assert got != [r[1][0] for r in before] and got == pytest.approx(want, abs=1e-5)


def test_refusals(plumbing):
    e = plumbing["errs"]
    assert "64" in e["batch"] and "RMSNorm" in e["norm"] and "fp32" in e["fp32"] and "weight_dtype" in e["dtype"]
