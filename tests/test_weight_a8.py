"""``quantised_prefill="a8"`` on the fp32 CPU oracle path at TP 1: a session of its own whose projections above 64
rows round their activations to e4m3 per token (so its logits are not the ``True`` session's), and the refusals."""
import pytest
import torch

import numerics as N
import numerics_w8 as W8

from dist_helpers import run_distributed


def _worker(rank, world):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    m, p = W8.tiny_model(), W8.prompt(6)                       # 6 x 12 = 72 rows: above the 64 of the decode kernels
    out = {"ids": [len(t) for t in G.generate(m, p, 3, weight_dtype="fp8", quantised_prefill="a8")], "errs": {}}
    for qp in ("a8", True):
        cache, _ = G._session(m, 6, 24, torch.device("cpu"), weight_dtype="fp8", quantised_prefill=qp)
        out[qp] = (cache.wq_prefill, G.logits_step(m, p, cache))
    for wd in ("mxfp4", None):
        with pytest.raises(ValueError) as ex:
            G.generate(m, p, 2, weight_dtype=wd, quantised_prefill="a8")
        out["errs"][wd] = str(ex.value)
    return out


@pytest.fixture(scope="module")
def out():
    return run_distributed(_worker, 1)[0]


def test_a8_is_a_session_of_its_own(out):
    (flag8, l8), (flag, lt) = out["a8"], out[True]
    assert flag8 == "a8" and flag is True and out["ids"] == [15] * 6
    r = N.rel(l8, lt)       # (without the option's own value the string is merely truthy: r == 0)
    print("rel(a8 logits, weight-only quantised prefill logits)", r)
    assert 0 < r < 0.25     # e4m3 keeps 4 significant bits: the logits move, by far less than themselves


def test_a8_refusals(out):
    assert "'a8' needs weight_dtype='fp8'" in out["errs"]["mxfp4"] and "'a8' needs a weight_dtype" in out["errs"][None]
