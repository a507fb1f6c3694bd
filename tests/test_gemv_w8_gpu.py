"""fp8 projection weights on the MI355X (csrc/kernels/gemv_w8.hip): the quantiser bit for bit, every
code exact and in place, ``_gemv_nt_w8`` within its derived unit (tests/numerics_w8.py) on both
launch forms and every M tile count, and ``generate(..., weight_dtype="fp8")`` on a tiny model."""
import os

import pytest
import torch

import numerics as N
import numerics_kv8 as Q
import numerics_w8 as W8

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _strided(t, pad):      # t [R, n] as the leading columns of a wider tensor: row stride n + pad
    wide = torch.zeros(t.size(0), t.size(1) + pad, dtype=t.dtype, device=t.device)
    wide[:, : t.size(1)] = t
    return wide[:, : t.size(1)]


@pytest.mark.parametrize("Nn,K,strided", [(37, 576, False), (100, 64, False), (48, 3072, True)])
def test_quantiser_bytes(C, Nn, K, strided):
    w = torch.randn(Nn, K, generator=torch.Generator().manual_seed(Nn))
    w[3], w[5, K - 1] = 0, torch.finfo(torch.bfloat16).max      # an all-zero row, a row whose amax is the bf16 maximum
    w = w.bfloat16()
    wg = _strided(w.to(DEV), 64) if strided else w.to(DEV)
    codes, inv = C._quant_w8_rows(wg)
    cq, iq = Q.quant_rows(w)
    assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), cq.view(torch.uint8))
    assert torch.equal(inv.cpu().view(torch.int32), iq.view(torch.int32))


@pytest.mark.parametrize("M", [16, 64])
def test_every_code_exact_and_in_place(C, M):
    """One-hot A rows pick one k per row (both halves of a 16-code load, all four lane groups), inv
    powers of two, the codes cycle through the 254 non-NaN bytes: y == f32(code) * inv exactly."""
    Nn, K = 48, 1024
    table = torch.tensor([b for b in range(256) if b & 0x7F != Q.NAN_CODE], dtype=torch.uint8)
    codes = table[torch.arange(Nn * K) % 254].view(Nn, K)
    inv = torch.exp2((torch.arange(Nn) % 9 - 4).float())
    ks = (torch.arange(M) * 37 + 5) % K
    assert {int(k) % 16 // 8 for k in ks} == {0, 1} and {int(k) % 64 // 16 for k in ks} == {0, 1, 2, 3}
    x = torch.zeros(M, K)
    x[torch.arange(M), ks] = 1.0
    y = C._gemv_nt_w8(x.bfloat16().to(DEV), codes.to(DEV), inv.to(DEV))
    assert torch.equal(y.float().cpu(), (codes.view(Q.F8).float() * inv[:, None])[:, ks].t())


# (100, 64): one pair-step, idle K-waves, ragged N; (37, 576): 9 pair-steps over 4 K-waves; (48, 3072):
# the 8 K-wave form; (8200, 1024): more than 512 column tiles, the wide-N form, ragged N; the shards of a
# tensor-parallel rank: (49, 192): the ragged lm_head shard of 97 ids over 2 ranks, 3 pair-steps over 4 K-waves;
# (192, 64): the K 64 Wo shard of one local head, whole 32-column workgroups, one pair-step and idle K-waves
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 64])
@pytest.mark.parametrize("Nn,K", [(100, 64), (37, 576), (48, 3072), (8200, 1024), (49, 192), (192, 64)])
def test_gemv_w8_bounds(C, Nn, K, M, bias):
    for sw in (False, True) if (Nn, K) in ((37, 576), (48, 3072)) else (False,):
        x, w, b = N.gemv_inputs(M, Nn, K, sw)
        cq, inv = Q.quant_rows(w)
        x, codes, inv, b = x.to(DEV), cq.view(torch.uint8).to(DEV), inv.to(DEV), b.to(DEV) if bias else None
        y = C._gemv_nt_w8(x, codes, inv, b, sw)
        ref, unit = W8.ref_w8(x, codes, inv, b, sw)
        what = f"gemv_w8 N {Nn} K {K} M {M} bias {bias} swiglu {sw}"
        print(what, "worst err/unit", N.worst_ratio(y, ref, unit)[0])
        N.assert_within(y, ref, unit, N.DERIVED, what, tiles={0: (16,), 1: (32, 16)})
        assert torch.equal(C._gemv_nt_w8(x, codes, inv, b, sw), y), what            # run to run
        assert torch.equal(C._gemv_nt_w8(_strided(x, 8), _strided(codes, 16), inv, b, sw), y), what


@pytest.fixture(scope="module")
def model():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29579")
    from distributed_pytorch_from_scratch_amd.models import generation as G
    from distributed_pytorch_from_scratch_amd.utils.dist import init_dist_env, destroy_dist_env
    init_dist_env(rank=0, tp_size=1, world_size=1, backend="nccl")
    yield W8.tiny_model().cuda()
    G.clear_sessions()
    destroy_dist_env()


@pytest.mark.parametrize("B", [3, 20])
def test_model_fp8_weights(model, monkeypatch, B):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    p = W8.prompt(B).cuda()
    # the first decode step's logits against the CPU oracle path on the same quantised weights
    cm = W8.tiny_model()
    cm.load_state_dict({k: v.detach().bfloat16().float().cpu() for k, v in model.state_dict().items()})
    cg, cc = W8.cache(G, model, B, "cuda", torch.bfloat16), W8.cache(G, cm, B, "cpu", torch.float32)
    assert all(torch.equal(a[0].cpu(), b[0]) for a, b in zip(cg.w8.values(), cc.w8.values()))
    nxt = G.logits_step(model, p, cg).argmax(-1, keepdim=True)          # (the CPU side is fed the GPU's id)
    G.logits_step(cm, p.cpu(), cc)
    logits = [G.logits_step(model, nxt, cg).cpu(), G.logits_step(cm, nxt.cpu(), cc)]
    rel = N.rel(logits[0], logits[1])
    print("batch", B, "rel(GPU fp8-weight logits, CPU oracle on the same codes)", rel)
    assert rel <= 3e-2
    # graph and eager path: identical tokens, greedy, per-row sampling, and with the paged fp8 cache
    runs = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("DPFS_DECODE_GRAPH", graph)
        none = G.generate(model, p, 9)
        runs[graph] = [G.generate(model, p, 9, weight_dtype="fp8", **kw) for kw in (
            {}, dict(temperature=[0.0, 0.7, 1.0] + [0.9] * (B - 3), top_k=20, seed=list(range(B))),
            dict(kv_dtype="fp8", kv_page=16))]
        assert G.generate(model, p, 9) == none                  # sessions do not leak into the bf16 path
    assert runs["1"] == runs["0"]
