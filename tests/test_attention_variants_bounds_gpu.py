"""Per-element bounds of every attention `impl` besides the default, on MI355X.

DPFS_ATTN_IMPL switches whole trainings onto these kernels, and until now only a global Frobenius
ratio checked them.  Forward impls 1 (attn_fwd_k at head_dim 64 / 128), 6 (row sum by MFMA) and 8
(scale and max folded into the MFMAs); backward impls 2 (attn_bwd_dq_k + attn_bwd_dkdv2_k at
head_dim 64 / 128), 6 (the fused head_dim-64 kernel), 7 (dq3 + the 64-keys-per-wave dK/dV) and 9
(the v3 pair with K pre-scaled), with and without the inverse RoPE + QKV bias gradient, at the old
geometry, non-causal, and past eight heads; the 256-key-block kernels also past four blocks.

Units and keys (tests/numerics_attn.py): impls 1, 2 and the fused 6 round where the default
kernels do and keep the default units and keys; impl 6 forward (``rsm``), impl 8 (``mf``) and
impls 7 / 9 (``ksc``) add the first-order term of their extra rounding to the unit and have keys
of their own, measured on the CPU like every other limit.  The backward variants take o and lse
from the default forward, as the step would.
"""
import functools

import pytest
import torch

import numerics as N
import numerics_attn as A

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    return _ext.require()


@functools.lru_cache(maxsize=None)
def _case(case, fam, rope):
    """Inputs and the fp64 oracle (on the device) of one case, computed once and shared by every
    variant that runs it; nothing in it is modified."""
    B, H, hd, T, causal = case
    q, k, v, do, pos = A.attn_inputs_bh(hd, T, fam, B, H, DEV)
    tab = N.rope_table(512, hd).to(DEV) if rope else None
    ref = N.attn_refs(q, k, v, do, hd ** -0.5, causal, pos if rope else None, tab)
    return (q, k, v, do, pos if rope else None, tab), ref


def _reach_asserts(kernels, case):
    B, H, hd, T, causal = case
    for kern in kernels:
        r = A.reach(kern, B, H, T, causal)
        if B * H > 8:
            assert r["max_bh"] >= 8 and r["groups"] >= 2, "the past-eight case has bh >= 8"
            if A.KERNELS[kern][0] == "paired":
                assert r["empty_workgroups"] > 0
        if T == 641:
            assert A.KERNELS[kern][1] != 256 or (r["blocks"] == 3 and r["unpaired"] and r["max_p"] == 1)
            assert r["max_tiles"] == 11
        if not causal:
            assert r["max_tiles"] == A.cdiv(T, 64) and T % 64, "every block sweeps all of a ragged T"


@pytest.mark.parametrize("impl,variant,kernel,case,fam", A.fwd_variant_cases(), ids=A.pid)
def test_attention_fwd_variant_bounds(C, impl, variant, kernel, case, fam):
    B, H, hd, T, causal = case
    _reach_asserts((kernel,), case)
    (q, k, v, do, _, _), base = _case(case, fam, False)
    scale = hd ** -0.5
    ref = A.variant_units(base, q, k, v, do, scale, causal, variant)
    o, lse = C.attn_fwd(q, k, v, scale, causal, impl=impl)
    for name, out in (("o", o), ("lse", lse)):
        N.assert_within(out, ref[name], ref["unit_" + name], A.limit(A.key_for(name, hd, False, variant)),
                        f"attn fwd impl {impl} {name} B {B} H {H} hd {hd} T {T} causal={causal} {fam}",
                        N.ATTN_TILES[name], A.where_fn(kernel, name, B, H, T, causal))


@pytest.mark.parametrize("impl,variant,kq,kk,case,fam,rope", A.bwd_variant_cases(), ids=A.pid)
def test_attention_bwd_variant_bounds(C, impl, variant, kq, kk, case, fam, rope):
    B, H, hd, T, causal = case
    _reach_asserts((kq, kk), case)
    (q, k, v, do, pos, tab), base = _case(case, fam, rope)
    scale = hd ** -0.5
    ref = A.variant_units(base, q, k, v, do, scale, causal, variant, pos, tab)
    o, lse = C.attn_fwd(q, k, v, scale, causal)                 # the default forward, as the step would
    d = torch.full((B * T, 3 * H * hd), float("nan"), device=DEV, dtype=torch.bfloat16)   # unwritten elements show
    dq, dk, dv = N.packed_views(d, B, T, H, hd)
    out = {"dq": dq, "dk": dk, "dv": dv}
    if rope:
        db = torch.full((3 * H * hd,), float("nan"), device=DEV)
        flag = C.attn_bwd(do, q, k, v, o, lse, scale, causal, dq, dk, dv, pos, tab, dbias=db, impl=impl)
        assert flag is True, "the variant writes the QKV bias gradient"
        out["dbias"] = db
    else:
        flag = C.attn_bwd(do, q, k, v, o, lse, scale, causal, dq, dk, dv, impl=impl)
        assert flag is False, "no bias gradient was asked for"
    for name in out:
        kern = kq if name == "dq" else kk
        N.assert_within(out[name], ref[name], ref["unit_" + name], A.limit(A.key_for(name, hd, rope, variant)),
                        f"attn bwd impl {impl} {name} B {B} H {H} hd {hd} T {T} causal={causal} rope={rope} {fam}",
                        N.ATTN_TILES[name],
                        # (dbias has no owner; the fused backward's dq leaves through attn_dq_reduce_k's plain grid)
                        None if name == "dbias" or (kern == "fused" and name == "dq") else A.where_fn(kern, name, B, H, T, causal))
