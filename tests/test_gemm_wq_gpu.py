"""The quantised-weight GEMM on the MI355X (csrc/kernels/gemm_wq.hip): ``_gemm_nt_w8`` / ``_gemm_nt_w4`` within
the derived units of the decode kernels' oracles at the edges of its BM x 128 x 64 tile, every code exact and
in place, and ``quantised_prefill=True`` on a tiny model: no projection of the session on a bf16 weight."""
import pytest
import torch

import numerics as N
import numerics_kv8 as Q
import numerics_w4 as W4
import numerics_w8 as W8

pytestmark = pytest.mark.gpu

from test_gemv_w8_gpu import C, DEV, _strided, model  # noqa: E402,F401  (the fp8 tests' fixtures and helper)
from distributed_pytorch_from_scratch_amd.ops import reference as R  # noqa: E402

BN, BK = 128, 64      # BM = 32 up to 255 workgroups of 128 x 128 (every shape below but the last two), then 64 / 128


def _operands(fmt, M, Nn, K, bias):
    x, w, b = N.gemv_inputs(M, Nn, K)
    if fmt == "fp8":
        cq, inv = Q.quant_rows(w)
        q = (cq.view(torch.uint8).to(DEV), inv.to(DEV))
    else:
        q = tuple(t.to(DEV) for t in R._quant_w4_rows(w))
    return x.to(DEV), q, b.to(DEV) if bias else None


def _run(C, fmt, x, q, b, strided=False):
    if strided:
        x, q = _strided(x, 8), (_strided(q[0], 16), _strided(q[1], 4) if fmt == "mxfp4" else q[1])
    return (C._gemm_nt_w8 if fmt == "fp8" else C._gemm_nt_w4)(x, *q, b)


# (M, N, K for fp8, K for MXFP4); a stage is 64 k, so K % 128 == 0 gives MXFP4 an even stage count always
SHAPES = [
    (65, 100, 64, 128),        # the first row count routed here: a ragged third row tile; N below one tile; the minimal K
    (32, 136, 192, 384),       # M = BM; one column tile + 8; 3 stages (fp8: the odd ring parity) / 6
    (33, 301, 640, 640),       # M = BM + 1; three column tiles, the last ragged, odd N: the scalar stores; 10 stages
    (70, 256, 1088, 1152),     # whole column tiles; a K past a thousand, 17 (odd) / 18 stages
    (1, 100, 192, 128),        # the kernel's own small-M correctness: one row
    (17, 136, 64, 256),        # and 17 rows
    (1100, 1930, 64, 128),     # 144 tiles of 128 rows, 288 of 64: the BM 64 launch, ragged both ways, N % 4 == 2
    (1990, 2100, 128, 128),    # 272 tiles of 128 x 128: the BM 128 launch, ragged both ways, vector stores
]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,Nn,K8,K4", SHAPES)
@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_gemm_wq_bounds(C, fmt, M, Nn, K8, K4, bias):
    K = K8 if fmt == "fp8" else K4
    x, q, b = _operands(fmt, M, Nn, K, bias)
    y = _run(C, fmt, x, q, b)
    ref, unit = (W8.ref_w8 if fmt == "fp8" else W4.ref_w4)(x, *q, b, False)
    what = f"gemm_wq {fmt} M {M} N {Nn} K {K} bias {bias}"
    print(what, "worst err/unit", N.worst_ratio(y, ref, unit)[0])
    N.assert_within(y, ref, unit, N.DERIVED, what, tiles={0: (128, 64, 32, 16), 1: (BN, 64, 16)})
    assert torch.equal(_run(C, fmt, x, q, b), y), what                      # run to run
    assert torch.equal(_run(C, fmt, x, q, b, strided=True), y), what


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_every_code_exact_and_in_place(C, fmt):
    """One-hot A rows pick one k per row over two row tiles of every BM: y is that column of the dequantised
    weight, exactly.  A wrong k order between the A and B images, nibble or neighbouring scale block shows."""
    M, Nn, K = 128 + 16, 136, 256
    ks = (torch.arange(M) * 37 + 5) % K
    # every position of a conversion group (16 codes of an fp8 load, 32 of an MXFP4 one) and of a stage
    # (both MFMA k-steps, all four lane groups), in every one of the K / 64 stages
    assert {int(k) % BK for k in ks} == set(range(BK)) and {int(k) // BK for k in ks} == set(range(K // BK))
    x = torch.zeros(M, K)
    x[torch.arange(M), ks] = 1.0
    if fmt == "fp8":
        table = torch.tensor([b for b in range(256) if b & 0x7F != Q.NAN_CODE], dtype=torch.uint8)
        codes = table[torch.arange(Nn * K) % 254].view(Nn, K)
        inv = torch.exp2((torch.arange(Nn) % 9 - 4).float())
        q, want = (codes.to(DEV), inv.to(DEV)), (codes.view(Q.F8).float() * inv[:, None]).double()
    else:
        codes = (torch.arange(Nn * K // 2) * 37 % 256).to(torch.uint8).view(Nn, K // 2)     # all 16 nibbles, both places
        scales = (119 + torch.arange(Nn * K // 32) % 17).to(torch.uint8).view(Nn, K // 32)
        q, want = (codes.to(DEV), scales.to(DEV)), W4.dequant64(codes, scales)
    y = _run(C, fmt, x.bfloat16().to(DEV), q, None)
    assert torch.equal(y.double().cpu(), want[:, ks].t())


@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_model_quantised_prefill(model, monkeypatch, fmt, B):
    from distributed_pytorch_from_scratch_amd.models import generation as G
    GS = G.GS
    p = W8.prompt(B).cuda()
    before = (G.generate(model, p, 9), G.generate(model, p, 9, weight_dtype=fmt) if B <= 64 else None)
    # the prompt, then one token, against the CPU oracle path on the same codes, every projection on them
    cm = W8.tiny_model()
    cm.load_state_dict({k: v.detach().bfloat16().float().cpu() for k, v in model.state_dict().items()})
    cg, cc = W8.cache(G, model, B, "cuda", torch.bfloat16, False), W8.cache(G, cm, B, "cpu", torch.float32, False)
    for c, m, dev in ((cg, model, "cuda"), (cc, cm, "cpu")):
        setattr(c, "w8" if fmt == "fp8" else "w4", G.quantise_weights(m, dev, fmt))
        c.wq_prefill = True
    lg, lc = G.logits_step(model, p, cg), G.logits_step(cm, p.cpu(), cc)
    nxt = lg.argmax(-1, keepdim=True)                                    # (the CPU side is fed the GPU's id)
    rels = (N.rel(lg.cpu(), lc), N.rel(G.logits_step(model, nxt, cg).cpu(), G.logits_step(cm, nxt.cpu(), cc)))
    print(fmt, "batch", B, "rel(GPU logits, CPU oracle on the same codes): prefill, first step", rels)
    assert max(rels) <= 3e-2

    def refuse(*a, **k):
        raise AssertionError("a projection of a quantised_prefill session ran on a bf16 weight")
    kw = dict(weight_dtype=fmt, quantised_prefill=True, prefill_chunk=5, prompt_lens=[12 - b % 6 for b in range(B)])
    runs = {}
    with monkeypatch.context() as mp:
        mp.setattr(GS, "gemm_nt", refuse)
        mp.setattr(GS, "small_nt", refuse)
        for graph in ("1", "0"):
            mp.setenv("DPFS_DECODE_GRAPH", graph)
            runs[graph] = [G.generate(model, p, 9, **kw), G.generate(model, p, 9, kv_dtype="fp8", kv_page=16, **kw)]
    assert runs["1"] == runs["0"]
    # sessions do not leak: the bf16 path and the plain weight_dtype path return what they did
    assert G.generate(model, p, 9) == before[0]
    assert B > 64 or G.generate(model, p, 9, weight_dtype=fmt) == before[1]
