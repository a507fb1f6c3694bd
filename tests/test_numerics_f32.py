"""The fp32 path's bounds themselves, on the CPU (tests/numerics_f32.py).

* The fp32 emulations of the attention kernels stay within ``numerics.DERIVED`` of the fp64
  oracle at every case tests/test_fp32_bounds_gpu.py runs; a plain fp32 matmul, its slabs summed
  in split order, does the same for the GEMM units, and reproduces integer products exactly.
* Seventeen planted faults each fail ``assert_within`` (``torch.equal`` in the integer form, the
  bias statistic for the chopped bf16 store).

For each fault the statistic of the older tests (test_kernels_gpu.py::test_gemm_f32: max |err| <
1e-4 sqrt(K); test_gemm_unaligned_bf16: max |err| < 1e-2 max |ref|; test_attention_f32: Frobenius
ratio of o < 1e-5, max lse error < 1e-4, ratio of the packed gradients and of dbias < 1e-4) is
evaluated on the same faulty output at that test's nearest shape, against the fp64 oracle.
``OLD_PASSES`` records which faults it lets through: the chopped bf16 store only.  Every other
fault here is gross enough for a global statistic at the old tests' shapes; what the older tests
lack for those is the cases (T 1, T below a tile, non-causal at head_dim 32 / 128, more than 256
partial rows, unaligned views, ragged and unlaunched splits), not the sensitivity.  (q chopped
to a 10-bit significand in the attention forward, which is not one of the seventeen, fails the
old statistic as well: a Frobenius ratio of 4e-4 against its 1e-5.)  Nothing more is claimed.
"""
import functools

import pytest
import torch

import numerics as N
import numerics_f32 as F


def _caught(fn):
    with pytest.raises(AssertionError):
        fn()


# the older tests' statistics ------------------------------------------------------------

def old_gemm_f32(out, ref, K):
    return float((out.double() - ref).abs().max()) < 1e-4 * max(1.0, K ** 0.5)


def old_gemm_bf16(out, ref):
    return float((out.double() - ref).abs().max()) < 1e-2 * float(ref.abs().max())


def old_attn_fwd(o, lse, ref):
    return N.rel(o, ref["o"]) < 1e-5 and float((lse.double() - ref["lse"]).abs().max()) < 1e-4


def old_attn_bwd(dq, dk, dv, db, ref):
    cat = lambda a, b, c: torch.cat([a.double(), b.double(), c.double()], -1)
    return (N.rel(cat(dq, dk, dv), cat(ref["dq"], ref["dk"], ref["dv"])) < 1e-4) and N.rel(db, ref["dbias"]) < 1e-4


# fault number -> does the older statistic pass the faulty output (True = the old suite misses it)
OLD_PASSES = {1: False, 2: False, 3: False, 4: False, 5: False, 6: False, 7: True, 8: False, 9: False, 10: False,
              11: False, 12: False, 13: False, 14: False, 15: False, 16: False, 17: False}


# ------------------------------------------------------------------------------ GEMM ----

def _gemm_ref(M, Nn, K, layout, with_bias, with_acc, integers=False, dtype=torch.float32):
    a, b, bias, acc = F.gemm_operands(M, Nn, K, layout, 200, integers, dtype)
    bias = bias if with_bias else None
    acc = acc if with_acc else None
    ref, mag = N.ref_gemm(a, b, layout, bias, acc)
    return a, b, bias, acc, ref, mag


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
@pytest.mark.parametrize("M,Nn,K", F.GEMM32_SHAPES)
def test_gemm_emulation_within_derived_and_integer_exact(M, Nn, K, layout):
    for with_bias, with_acc in ((layout == "nt", False), (False, True)):
        a, b, bias, acc, ref, mag = _gemm_ref(M, Nn, K, layout, with_bias, with_acc)
        unit = N.unit_gemm_f32(mag, K, F.gemm_splits_for_unit(K), acc)
        N.assert_within(F.emu_gemm32(a, b, layout, bias, acc), ref, unit, N.DERIVED, f"emulated gemm {layout}")
        a, b, bias, acc, ref, _ = _gemm_ref(M, Nn, K, layout, with_bias, with_acc, integers=True)
        assert float(ref.abs().max()) < 2 ** 24
        assert torch.equal(F.emu_gemm32(a, b, layout, bias, acc).long(), ref.long())


def test_gemm_plan_reaches_the_split_cases():
    assert F.gemm_plan(8, 12, 1024) == (2, 512, 2)
    assert F.gemm_plan(130, 8, 1089) == (2, 576, 2) and 1089 - 576 == 513
    assert F.gemm_plan(8, 8, 33000) == (64, 544, 61)
    assert F.gemm_plan(200, 136, 64)[0] == 1 and F.gemm_plan(8, 12, 1089)[2] == 2
    assert all(F.gemm_plan(M, Nn, K)[0] <= F.gemm_splits_for_unit(K) for M, Nn, K in F.GEMM32_SHAPES)


@pytest.mark.parametrize("M,Nn,K", F.GEMM32_BF16_SHAPES)
def test_gemm_bf16_storage_emulation_within_derived(M, Nn, K):
    bf = torch.bfloat16
    for layout in ("nt", "nn"):
        a, b, bias, _, ref, mag = _gemm_ref(M, Nn, K, layout, layout == "nt", False, dtype=bf)
        unit = N.unit_gemm_bf16(ref, mag, K + F.gemm_splits_for_unit(K))
        N.assert_within(F.emu_gemm32(a, b, layout, bias, out_bf16=True), ref, unit, N.DERIVED, f"emulated bf16 gemm {layout}")
        a, b, bias, _, ref, _ = _gemm_ref(M, Nn, K, layout, layout == "nt", False, integers=True, dtype=bf)
        assert torch.equal(F.emu_gemm32(a, b, layout, bias, out_bf16=True), ref.float().bfloat16())
    a, b, _, acc, ref, mag = _gemm_ref(M, Nn, K, "tn", False, True, dtype=bf)
    N.assert_within(F.emu_gemm32(a, b, "tn", None, acc), ref, N.unit_gemm_f32(mag, K, F.gemm_splits_for_unit(K), acc),
                    N.DERIVED, "emulated bf16-in gemm tn accumulate")


def _gemm_fault(num, M, Nn, K, layout, fault, with_acc=False, old=None):
    """The fault fails the new check at (M, Nn, K); the old statistic at ``old`` = its nearest shape."""
    with_bias = layout == "nt"
    a, b, bias, acc, ref, mag = _gemm_ref(M, Nn, K, layout, with_bias, with_acc)
    unit = N.unit_gemm_f32(mag, K, F.gemm_splits_for_unit(K), acc)
    N.assert_within(F.emu_gemm32(a, b, layout, bias, acc), ref, unit, N.DERIVED, "unfaulted")
    _caught(lambda: N.assert_within(F.emu_gemm32(a, b, layout, bias, acc, fault=fault), ref, unit, N.DERIVED, fault,
                                    F.GEMM32_TILES))
    if fault != "tf32":    # the integer form sees it too (chopping keeps small integers exact)
        a, b, bias, acc, ref, _ = _gemm_ref(M, Nn, K, layout, with_bias, with_acc, integers=True)
        assert not torch.equal(F.emu_gemm32(a, b, layout, bias, acc, fault=fault).long(), ref.long())
    M, Nn, K = old
    a, b, bias, acc, ref, _ = _gemm_ref(M, Nn, K, layout, with_bias, with_acc)
    assert old_gemm_f32(F.emu_gemm32(a, b, layout, bias, acc, fault=fault), ref, K) == OLD_PASSES[num]


def test_fault_01_operands_chopped_to_10_bits():
    _gemm_fault(1, 200, 136, 64, "nt", "tf32", old=(300, 200, 96))


def test_fault_02_last_k_element_dropped():
    _gemm_fault(2, 129, 130, 33, "tn", "k_tail", old=(96, 130, 33))


def test_fault_03_split_boundary_row_counted_twice():
    _gemm_fault(3, 130, 8, 1089, "tn", "split_overlap", old=(128, 128, 8192))


def test_fault_04_bias_added_once_per_split():
    _gemm_fault(4, 130, 8, 1089, "nt", "bias_per_split", old=(128, 128, 8192))


def test_fault_05_accumulate_overwrites():
    _gemm_fault(5, 130, 8, 1089, "tn", "overwrite", with_acc=True, old=(96, 130, 33))
    _gemm_fault(5, 129, 130, 33, "tn", "overwrite", with_acc=True, old=(96, 130, 33))


def test_fault_06_slab_sum_stops_one_split_early():
    _gemm_fault(6, 8, 8, 33000, "nn", "slab_short", old=(128, 128, 8192))


def test_fault_07_bf16_output_chopped():
    """Chopping stays within the per-element bound's order (2 U16 against U16): assert_within sees
    it at most elements, the bias statistic at the rounding-mode shape by its -0.5 ulp mean."""
    M, Nn, K = F.GEMM32_STAT_SHAPE
    a, b, bias, _, ref, mag = _gemm_ref(M, Nn, K, "nt", True, False, dtype=torch.bfloat16)
    unit, at = N.unit_gemm_bf16(ref, mag, K + 1), N.acc_term_gemm(mag, K + 1)
    good, bad = (F.emu_gemm32(a, b, "nt", bias, out_bf16=True, fault=f) for f in (None, "chopped"))
    N.assert_within(good, ref, unit, N.DERIVED, "rounded")
    assert N.bias_stat(good, ref, at, "rounded")[2] < 0.10
    _caught(lambda: N.bias_stat(bad, ref, at, "chopped"))
    _caught(lambda: N.assert_within(bad, ref, unit, N.DERIVED, "chopped"))
    a, b, bias, _, ref, _ = _gemm_ref(300, 500, 777, "nt", True, False, dtype=torch.bfloat16)   # the old test's shape
    assert old_gemm_bf16(F.emu_gemm32(a, b, "nt", bias, out_bf16=True, fault="chopped"), ref) == OLD_PASSES[7]


# ------------------------------------------------------------------------- attention ----

@functools.lru_cache(maxsize=4)
def _attn_ref(hd, T, causal, fam, rope=False, B=2, H=3):
    """Inputs, oracle, and the oracle's o / lse rounded to fp32 (the backward's known inputs)."""
    q, k, v, do, pos = F.attn32_inputs(hd, T, fam, B=B, H=H)
    tab = N.rope_table(512, hd) if rope else None
    scale = F.scale_f32(hd)
    ref = F.ref_attn32(q, k, v, do, scale, causal, pos if rope else None, tab)
    return (q, k, v, do, pos if rope else None, tab, scale), ref, ref["o"].float(), ref["lse"].float()


def _attn_emulated(hd, T, causal, fam, rope=False, fwd_fault=None, bwd_fault=None, **kw):
    (q, k, v, do, pos, tab, scale), ref, o_in, lse_in = _attn_ref(hd, T, causal, fam, rope, **kw)
    o, lse = F.emu_attn32_fwd(q, k, v, scale, causal, fwd_fault)
    dq, dk, dv, db = F.emu_attn32_bwd(do, q, k, v, o_in, lse_in, scale, causal, pos, tab, bwd_fault)
    return ref, {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "dbias": db}


def _assert_all(ref, out, names, what):
    for name in names:
        N.assert_within(out[name], ref[name], ref["unit_" + name], N.DERIVED, f"{what} {name}", F.ATTN32_TILES[name])


@pytest.mark.parametrize("fam", list(F.ATTN32_FAMILIES))
@pytest.mark.parametrize("hd,T,causal", F.ATTN32_CASES)
def test_attention_emulation_within_derived(hd, T, causal, fam):
    ref, out = _attn_emulated(hd, T, causal, fam)
    _assert_all(ref, out, ("o", "lse", "dq", "dk", "dv", "dbias"), "emulated")


@pytest.mark.parametrize("fam", list(F.ATTN32_FAMILIES))
@pytest.mark.parametrize("hd,T", F.ATTN32_ROPE_CASES)
def test_attention_rope_dbias_emulation_within_derived(hd, T, fam):
    ref, out = _attn_emulated(hd, T, True, fam, rope=True)
    _assert_all(ref, out, ("dq", "dk", "dv", "dbias"), "emulated (rope)")


def test_attention_many_partial_rows_emulation_within_derived():
    c = F.ATTN32_MANY_ROWS
    ref, out = _attn_emulated(c["hd"], c["T"], True, "randn", rope=True, B=c["B"], H=c["H"])
    _assert_all(ref, out, ("o", "lse", "dq", "dk", "dv", "dbias"), "emulated (B 65, T 1)")


def _attn_fault(num, case, names, fwd_fault=None, bwd_fault=None, old_case=None):
    """The fault fails ``names`` at ``case`` = (hd, T, causal, rope); the older statistic is
    evaluated at ``old_case``, the old test's nearest shape."""
    hd, T, causal, rope = case
    ref, good = _attn_emulated(hd, T, causal, "randn", rope)
    _, bad = _attn_emulated(hd, T, causal, "randn", rope, fwd_fault, bwd_fault)
    for name in names:
        args = (ref[name], ref["unit_" + name], N.DERIVED)
        N.assert_within(good[name], *args, f"unfaulted {name}")
        _caught(lambda: N.assert_within(bad[name], *args, f"fault {num} {name}", F.ATTN32_TILES[name]))
    hd, T, causal, rope = old_case or case
    ref, bad = _attn_emulated(hd, T, causal, "randn", rope, fwd_fault, bwd_fault)
    old = old_attn_fwd(bad["o"], bad["lse"], ref) if fwd_fault else old_attn_bwd(bad["dq"], bad["dk"], bad["dv"], bad["dbias"], ref)
    assert old == OLD_PASSES[num]


def test_fault_08_diagonal_key_masked_in_one_head():
    _attn_fault(8, (64, 129, True, False), ("o", "lse"), fwd_fault="diag", old_case=(64, 300, True, False))


def test_fault_09_keys_past_T_unmasked_when_not_causal():
    _attn_fault(9, (128, 65, False, False), ("o", "lse"), fwd_fault="tail", old_case=(64, 193, False, False))


def test_fault_10_o_not_rescaled_in_one_tile():
    _attn_fault(10, (32, 129, True, False), ("o",), fwd_fault="alpha", old_case=(32, 193, True, False))


def test_fault_11_lse_left_in_log2_units():
    _attn_fault(11, (64, 33, True, False), ("lse",), fwd_fault="log2", old_case=(64, 300, True, False))


def test_fault_12_delta_from_the_neighbouring_head():
    _attn_fault(12, (64, 65, True, False), ("dq", "dk"), bwd_fault="delta_head", old_case=(64, 300, True, True))


def test_fault_13_sin_sign_flipped_in_the_inverse_rope():
    _attn_fault(13, (128, 129, True, True), ("dq", "dk"), bwd_fault="sin_sign", old_case=(128, 129, True, True))


def test_fault_14_head_dim_32_with_the_pairing_of_64():
    _attn_fault(14, (32, 65, True, True), ("dq", "dk"), bwd_fault="pairing", old_case=(32, 193, True, True))


def test_fault_15_one_wave_missing_from_dbias():
    _attn_fault(15, (64, 300, True, True), ("dbias",), bwd_fault="dbias_wave")


def test_fault_16_row_past_T_included_in_dbias():
    _attn_fault(16, (32, 65, True, True), ("dbias",), bwd_fault="dbias_row", old_case=(32, 193, True, True))


def test_fault_17_dk_without_scale():
    _attn_fault(17, (128, 33, False, False), ("dk",), bwd_fault="dk_scale", old_case=(64, 193, False, True))


def test_chopped_operands_are_outside_the_attention_units():
    """Not one of the seventeen: q chopped to a 10-bit significand gives 11 x the unit or more."""
    (q, k, v, do, _, _, scale), ref, _, _ = _attn_ref(64, 129, True, "randn")
    o, lse = F.emu_attn32_fwd(F.tf32(q), k, v, scale, True)
    assert N.worst_ratio(o, ref["o"], ref["unit_o"])[0] > 11 and N.worst_ratio(lse, ref["lse"], ref["unit_lse"])[0] > 11


# ---------------------------------------------------- shared oracles at fp32 storage ----

def test_storage_keyword_defaults_are_unchanged_and_fp32_swaps_the_store_term():
    g = torch.Generator().manual_seed(5)
    gu, dh = torch.randn(9, 16, generator=g), torch.randn(9, 8, generator=g)
    h, u16, acc = N.ref_swiglu_fwd(gu)
    _, u32, _ = N.ref_swiglu_fwd(gu, bf16_out=False)
    assert torch.equal(u16, N.U16 * h.abs() + acc) and torch.equal(u32, N.U32 * h.abs() + acc)
    ref, b16, acc = N.ref_swiglu_bwd(dh.double(), gu)[:3]
    b32 = N.ref_swiglu_bwd(dh.double(), gu, bf16_out=False)[1]
    assert torch.equal(b16, N.U16 * ref.abs() + acc) and torch.equal(b32, N.U32 * ref.abs() + acc)
    y, res, b = torch.randn(5, 8, generator=g), torch.randn(5, 8, generator=g), torch.randn(8, generator=g)
    x, r16, acc = N.ref_bias_residual(y, b, res)
    assert torch.equal(r16, N.U16 * x.abs() + acc) and torch.equal(N.ref_bias_residual(y, b, res, False)[1], N.U32 * x.abs() + acc)
    # add_rmsnorm at fp32 storage: the norm of x rounded once to fp32
    w = torch.rand(8, generator=g) + 0.5
    out = N.ref_add_rmsnorm_fwd(y, b, res, w, 1e-5, bf16_out=False)
    hr, uh, rr, ur = N.ref_rmsnorm_fwd(x.float(), w, 1e-5, False)
    assert torch.equal(out[2], hr) and torch.equal(out[3], uh) and torch.equal(out[4], rr)
    # an fp32 evaluation attains the fp32-storage units
    N.assert_within(torch.nn.functional.silu(gu[:, :8]) * gu[:, 8:], h, u32, N.DERIVED, "swiglu fp32")
    N.assert_within(y + b + res, x, N.ref_bias_residual(y, b, res, False)[1], N.DERIVED, "bias_residual fp32")
