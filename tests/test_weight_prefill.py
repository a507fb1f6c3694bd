"""``quantised_prefill`` on the fp32 CPU oracle path, TP 1 and 2: a quantised session is one model for the prompt
and the generated tokens, the default is unchanged, the refusals."""
import pytest
import torch

import numerics as N
import numerics_w8 as W8

from dist_helpers import run_distributed

T = 11


def _split(G, m, p, fmt, on):
    """rel(last-row logits of T ids prefilled + id T + 1 as a decode step, those of T + 1 ids prefilled)."""
    caches = []
    for _ in range(2):
        c = W8.cache(G, m, p.size(0), "cpu", torch.float32, False)
        if fmt:
            setattr(c, "w8" if fmt == "fp8" else "w4", G.quantise_weights(m, "cpu", fmt))
        c.wq_prefill = on
        caches.append(c)
    whole = G.logits_step(m, p[:, : T + 1], caches[0])
    G.logits_step(m, p[:, :T], caches[1])
    return N.rel(G.logits_step(m, p[:, T: T + 1], caches[1]), whole)


def _worker(rank, world):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, p = W8.tiny_model(), W8.prompt(3)
    out = {"r0": _split(G, m, p, None, False)}
    for fmt in ("fp8", "mxfp4"):
        out[fmt] = (_split(G, m, p, fmt, True), _split(G, m, p, fmt, False))
        out[fmt + " default"] = G.generate(m, p, 6, weight_dtype=fmt) == G.generate(m, p, 6, weight_dtype=fmt,
                                                                                     quantised_prefill=False)
    out["B65"] = [len(t) for t in G.generate(m, W8.prompt(65), 2, weight_dtype="fp8", quantised_prefill=True)]
    errs = {}
    m32 = W8.tiny_model()
    m32.set_compute_dtype(torch.float32)
    for name, mm, wd in (("none", m, None), ("norm", W8.tiny_model("layernorm"), "fp8"), ("fp32", m32, "mxfp4")):
        with pytest.raises(ValueError) as ex:
            G.generate(mm, p, 2, weight_dtype=wd, quantised_prefill=True)
        errs[name] = str(ex.value)
    out["errs"] = errs
    return out


@pytest.fixture(scope="module", params=[1, 2])
def ranks(request):
    return run_distributed(_worker, request.param)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_one_model_throughout(ranks, fmt):
    """Prefill and decode are the same fp32 operations in another order: with the option their difference on
    codes (r_q) is that of the bf16-weight session (r_0, factor 4 for the other weight values); without it
    it is the quantisation error, the gap the option closes."""
    for rank, out in ranks.items():
        r0, (rq, roff) = out["r0"], out[fmt]
        print(f"rank {rank} {fmt}: r_0 {r0:.3g}, r_q {rq:.3g}, r_q with the option off {roff:.3g}")
        assert rq <= 4 * r0 and roff >= 100 * r0


def test_default_unchanged_and_batch_above_64(ranks):
    for out in ranks.values():
        assert out["fp8 default"] and out["mxfp4 default"] and out["B65"] == [14] * 65


def test_refusals(ranks):
    for out in ranks.values():
        e = out["errs"]
        assert "quantised_prefill" in e["none"] and "RMSNorm" in e["norm"] and "fp32" in e["fp32"]
