"""Helpers of the fp8-weight projection tests (tests/test_weight_fp8.py, tests/test_gemv_w8_gpu.py):
the fp64 oracle and derived unit of ``_gemv_nt_w8``, and the tiny RMSNorm model of the model tests."""
import torch

import numerics as N
import numerics_kv8 as Q


def ref_w8(x, codes, inv, bias=None, swiglu=False):
    """(ref, unit) of y = bf16((a codes^T) * inv + bias), fp64: the bf16 store, the fp32 accumulator
    scaled by inv, two fp32 roundings (the scale multiply and the bias add; an FMA has one).
    ``swiglu``: a = bf16(silu(g) u), plus the operand-flip term of ``numerics.ref_gemv``."""
    c64, i64 = N.d(codes.view(Q.F8).float()), N.d(inv)
    K = c64.size(1)
    flip = 0.0
    if swiglu:
        h, _, acc = N.ref_swiglu_fwd(x)
        a, ulp = N.bf16_round(h), N.bf16_ulp(h)
        flip = torch.where((ulp / 2 - (h - a).abs()) <= acc, ulp, torch.zeros_like(ulp)) @ c64.abs().t() * i64
    else:
        a = N.d(x)
    acc_ref, mag = a @ c64.t(), a.abs() @ c64.abs().t()
    b64 = N.d(bias) if bias is not None else torch.zeros_like(i64)
    ref = acc_ref * i64 + b64
    return ref, N.U16 * ref.abs() + i64 * N.acc_term_gemm(mag, K) + 2 * N.U32 * ((acc_ref * i64).abs() + b64.abs()) + flip


def tiny_model(norm="rmsnorm"):
    """head_dim 64, 2 layers, d 128: every projection's K is a multiple of 64."""
    from distributed_pytorch_from_scratch_amd.models import ModelArgs, Transformer
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    m = Transformer.from_args(ModelArgs(attn_dim=128, ffn_dim=256, num_heads=2, num_layers=2, vocab_size=96, maxlen=64,
                                        vocab_pad_to=1, norm=norm))
    set_seed(0)
    m.reset_parameters()
    return m.eval()


def prompt(B, T=12, seed=5):
    return torch.randint(3, 96, (B, T), generator=torch.Generator().manual_seed(seed))


def cache(G, m, B, dev, dtype, fp8_weights=True):     # a KVCache of 24 rows with the fp8 weights attached
    a = m.layers[0].attn
    c = G.KVCache(len(m.layers), B, 24, a.num_local_heads, a.head_dim, dtype, torch.device(dev))
    c.w8 = G.quantise_weights(m, dev) if fp8_weights else None
    return c
