"""Helpers of the MXFP4-weight tests (tests/test_weight_mxfp4.py, tests/test_gemv_w4_gpu.py): an fp64
decoder of the format written apart from the oracle's, the quantiser's edge inputs, and the fp64
oracle and derived unit of ``_gemv_nt_w4``."""
import torch

import numerics as N

E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, 7.5]      # times the block scale; the last two are above 6
TIE_CODES = [0, 2, 2, 4, 4, 6, 6, 7, 7]                       # ties go to the even code, above 6 saturates


def dequant64(codes, scales):
    # fp64 [N, K]: element k in bits 4 (k % 2) .. + 3 of byte k / 2, sign + e2m1, times 2^(s - 127)
    nib = torch.stack((codes & 15, codes >> 4), -1).flatten(1).long()
    v = torch.tensor(E2M1 + [-m for m in E2M1], dtype=torch.float64, device=codes.device)[nib]
    return v * torch.exp2(scales.double() - 127).repeat_interleave(32, 1)


def quant_inputs(Nn, K):
    """bf16 randn [Nn, K] with five edge blocks, the first of rows 0-4 and the last of rows 5-9: zeros; bf16
    subnormals; amax = the bf16 maximum; amax = 4, a power of two; the ties and above 6 (block scale 2^-3)."""
    g = torch.Generator().manual_seed(7 + Nn + K)
    w, edge = torch.randn(Nn, K, generator=g), torch.zeros(5, 32)
    edge[1] = torch.randint(-127, 128, (32,), generator=g) * 2.0 ** -133
    edge[2] = torch.randn(32, generator=g)
    edge[3] = torch.rand(32, generator=g) * 3.9
    edge[2, 9], edge[3, 5] = torch.finfo(torch.bfloat16).max, -4.0
    edge[4, :18] = torch.tensor(TIES + [-t for t in TIES]) / 8
    w[:5, :32], w[5:10, K - 32:] = edge, edge
    return w.bfloat16()


def ref_w4(x, codes, scales, bias=None, swiglu=False):
    """(ref, unit) of y = bf16(a wq^T + bias), fp64, the unit of ``numerics_w8.ref_w8`` without its scale
    term: the bf16 store, the fp32 accumulator, one fp32 rounding for the bias add, and under ``swiglu``
    the operand-flip term of ``numerics.ref_gemv``."""
    w64 = dequant64(codes, scales)
    flip = 0.0
    if swiglu:
        h, _, acc = N.ref_swiglu_fwd(x)
        a, ulp = N.bf16_round(h), N.bf16_ulp(h)
        flip = torch.where((ulp / 2 - (h - a).abs()) <= acc, ulp, torch.zeros_like(ulp)) @ w64.abs().t()
    else:
        a = N.d(x)
    acc_ref, mag = a @ w64.t(), a.abs() @ w64.abs().t()
    b64 = N.d(bias) if bias is not None else torch.zeros_like(w64[:, 0])
    ref = acc_ref + b64
    return ref, N.U16 * ref.abs() + N.acc_term_gemm(mag, w64.size(1)) + N.U32 * (acc_ref.abs() + b64.abs()) + flip
