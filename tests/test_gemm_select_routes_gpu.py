"""Every route of every entry point of ops/gemm_select.py, per element, on MI355X.

The engines never call the bindings: they call the selector, whose route for a shape is chosen by
a stopwatch on the first call, so which kernel form a run exercises depends on the clock.  Here
nothing is timed.  Each test starts from an empty selector state, forces a route by seeding
``gemm_select._choice`` with the key the function under test builds (``_ms`` is replaced by a
function that fails the test, so a key that does not match cannot fall through to a timing), runs
the entry point with a recording proxy in place of the kernel set, asserts from the proxy's log
that the named route is the one that ran, and judges the result with ``numerics.assert_within``
against the fp64 oracle.  Every limit is ``numerics.DERIVED``.
"""

import pytest
import torch

import numerics as N
import numerics_f32 as F32
import numerics_items as I

pytestmark = pytest.mark.gpu

from distributed_pytorch_from_scratch_amd.ops import _ext  # noqa: E402
from distributed_pytorch_from_scratch_amd.ops import gemm_select as GS  # noqa: E402
from distributed_pytorch_from_scratch_amd.parallel.grad_sync import GradArena  # noqa: E402

DEV = "cuda:0"
IDX = 0
TILES = {0: (256, 128, 16), 1: (256, 192, 128, 96, 16)}
SENTINEL = -7.0
BF16_ROUTES = ["ours", "ours256", "ours192", "ours_nt", "ours256_nt", "ours192_nt"]


@pytest.fixture(scope="module")
def C():
    return _ext.require()


class Spy:
    """Forwards attribute access to the kernel set and logs every call (name, args, kwargs)."""

    def __init__(self, target, direct=False):
        self._target, self.calls = target, []
        if direct:
            self.DIRECT = True

    def __getattr__(self, name):
        attr = getattr(self._target, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            self.calls.append((name, a, kw))
            return attr(*a, **kw)
        return call

    def names(self):
        return [c[0] for c in self.calls]

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def _no_timing(*a, **kw):
    raise AssertionError("the selector timed a candidate: the seeded key does not match the one it builds")


@pytest.fixture
def k(monkeypatch, C):
    monkeypatch.setattr(GS, "_choice", {})
    monkeypatch.setattr(GS, "_times", {})
    monkeypatch.setattr(GS, "_ms", _no_timing)
    monkeypatch.setenv("DPFS_GEMM_BACKEND", "auto")
    monkeypatch.delenv("DPFS_GEMM_LIB", raising=False)
    return Spy(C)


def _randn(*shape, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def seed_nt(M, Nn, K, bias, route="ours"):
    GS._choice[("nt", M, Nn, K, bool(bias), IDX)] = route


def seed_nn(M, Nn, K, route="ours"):
    GS._choice[("nn", M, Nn, K, IDX)] = route


def seed_tn(M, Nn, K, acc, route="ours"):
    GS._choice[("tn", M, Nn, K, bool(acc), IDX)] = route


def _variant_seen(k, name, route):
    calls = k.of(name)
    assert len(calls) == 1 and calls[0][2].get("variant") == GS._VARIANT[route], (route, k.names(), calls[0][2])


def _in_slot(M, Nn, colslice):
    """(buffer, out): ``out`` [M, N] inside a sentinel-filled staging buffer -- a column slice of wider
    rows (the NT binding takes one), else contiguous rows between sentinel pads (the NN binding wants
    a contiguous output)."""
    if colslice:
        buf = torch.full((M, Nn + 24), SENTINEL, device=DEV, dtype=torch.bfloat16)
        return buf, buf[:, 8:8 + Nn]
    buf = torch.full((M + 2, Nn), SENTINEL, device=DEV, dtype=torch.bfloat16)
    return buf, buf[1:M + 1]


def _pads_intact(buf, out):
    probe = buf.clone()
    out_in_probe = probe.as_strided(out.shape, out.stride(), out.storage_offset() - buf.storage_offset())
    out_in_probe.fill_(SENTINEL)
    return bool((probe == SENTINEL).all())


# ------------------------------------------------------------------ gemm_nt / gemm_nn ----

@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_bf16_routes_bounds_and_bit_identical(k, layout):
    """The six width / store routes: each within the bound, each with ``out`` a slot of a
    sentinel-filled buffer, and all twelve results torch.equal -- the claim of ``_ours_variants``'
    docstring, on which leaving the choice to the clock rests."""
    M, Nn, K = 300, 392, 96
    a = _randn(M, K, seed=1)
    b = _randn(Nn, K, seed=2) if layout == "nt" else _randn(K, Nn, seed=2)
    bias = _randn(Nn, seed=3, dtype=torch.float32) if layout == "nt" else None
    ref, mag = N.ref_gemm(a, b, layout, bias)
    unit = N.unit_gemm_bf16(ref, mag, K)
    results = []
    for route in BF16_ROUTES:
        for slot in (False, True):
            k.calls.clear()
            seed_nt(M, Nn, K, True, route) if layout == "nt" else seed_nn(M, Nn, K, route)
            buf, out = _in_slot(M, Nn, layout == "nt") if slot else (None, None)
            y = GS.gemm_nt(k, a, b, bias, out=out) if layout == "nt" else GS.gemm_nn(k, a, b, out=out)
            _variant_seen(k, "gemm_" + layout, route)
            what = f"route {route} gemm_{layout} slot={slot}"
            if slot:
                assert y.data_ptr() == out.data_ptr() and _pads_intact(buf, out), what + ": sentinel overwritten"
            N.assert_within(y, ref, unit, N.DERIVED, what, TILES)
            results.append((what, y.clone()))
    for what, y in results[1:]:
        assert torch.equal(y, results[0][1]), f"{what} differs from {results[0][0]}"


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_bf16_direct_below_min_rows_and_selector_at_it(k, layout):
    """M = _MIN_ROWS - 1 takes the direct call (no variant, nothing recorded), M = _MIN_ROWS the selector."""
    Nn, K = 264, 64
    for M, route in ((GS._MIN_ROWS - 1, None), (GS._MIN_ROWS, "ours192_nt")):
        k.calls.clear()
        a = _randn(M, K, seed=4)
        b = _randn(Nn, K, seed=5) if layout == "nt" else _randn(K, Nn, seed=5)
        bias = _randn(Nn, seed=6, dtype=torch.float32) if layout == "nt" else None
        if route:
            seed_nt(M, Nn, K, True, route) if layout == "nt" else seed_nn(M, Nn, K, route)
        y = GS.gemm_nt(k, a, b, bias) if layout == "nt" else GS.gemm_nn(k, a, b)
        if route:
            _variant_seen(k, "gemm_" + layout, route)
        else:
            assert k.names() == ["gemm_" + layout] and "variant" not in k.calls[0][2] and not GS._choice
        ref, mag = N.ref_gemm(a, b, layout, bias)
        N.assert_within(y, ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, f"gemm_{layout} M {M} route {route}", TILES)


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_stream_k_routes(k, C, layout):
    """``ours_sk`` / ``ours_sk_nt`` at the shape the selector offers them for: tiles at 1.5 per CU,
    K = SK_MIN_K."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    (M, Nn), K = I.sk_shape(cus), GS.SK_MIN_K
    if not GS._sk_ok(k, M, Nn, K):
        pytest.skip(f"stream-K is not a candidate for {M}x{Nn}x{K} on {cus} CUs")
    items = I.sk_order(M, Nn, cus)
    a = _randn(M, K, seed=7, scale=K ** -0.25)
    b = (_randn(Nn, K, seed=8, scale=K ** -0.25) if layout == "nt" else _randn(K, Nn, seed=8, scale=K ** -0.25))
    bias = _randn(Nn, seed=9, dtype=torch.float32) if layout == "nt" else None
    ys = []
    C.gemm_sk_error(True)
    for route in ("ours_sk", "ours_sk_nt"):
        for slot in (False, True):
            k.calls.clear()
            seed_nt(M, Nn, K, True, route) if layout == "nt" else seed_nn(M, Nn, K, route)
            buf, out = _in_slot(M, Nn, layout == "nt") if slot else (None, None)
            ys.append(GS.gemm_nt(k, a, b, bias, out=out) if layout == "nt" else GS.gemm_nn(k, a, b, out=out))
            _variant_seen(k, "gemm_" + layout, route)
            if slot:
                assert ys[-1].data_ptr() == out.data_ptr() and _pads_intact(buf, out), f"{route}: sentinel overwritten"
    torch.cuda.synchronize()
    assert C.gemm_sk_error(False) == 0

    def slab(r0, r1):
        ref, mag = N.ref_gemm(a[r0:r1], b, layout, bias)
        return ref, I.unit_gemm_sk(ref, mag, K)
    I.assert_within_rows(ys[0], slab, N.DERIVED, f"route ours_sk gemm_{layout} {M}x{Nn}x{K}", TILES, items, 256)
    assert all(torch.equal(ys[0], y) for y in ys[1:]), "the stream-K routes (plain / non-temporal, fresh output / slot) differ"


# ---------------------------------------------------------------------- gemm_nt_rope ----

def _rope_case(M, H, hd, K, seed=10):
    Nn = 3 * H * hd
    x, w = _randn(M, K, seed=seed), _randn(Nn, K, seed=seed + 1, scale=K ** -0.5)
    bias = _randn(Nn, seed=seed + 2, dtype=torch.float32)
    pos = torch.randint(0, 512, (M,), generator=torch.Generator().manual_seed(seed + 3)).to(DEV)
    tab = N.rope_table(512, hd).to(DEV)
    lin, mag = N.ref_gemm(x, w, "nt", bias)
    return Nn, x, w, bias, pos, tab, lin, mag


def _seed_rope(M, Nn, K, hd, rot, split_ok, route):
    GS._choice[("nt_rope", M, Nn, K, hd, rot, split_ok, IDX)] = route


@pytest.mark.parametrize("route", ["ours", "ours_split"])
@pytest.mark.parametrize("H,hd", [(4, 64), (2, 128)])
def test_rope_routes(k, H, hd, route):
    M, K = 300, 64
    Nn, x, w, bias, pos, tab, lin, mag = _rope_case(M, H, hd, K)
    rot = 2 * H * hd
    _seed_rope(M, Nn, K, hd, rot, True, route)
    y = GS.gemm_nt_rope(k, x, w, bias, pos, tab, 2 * H, hd)
    calls = k.of("gemm_nt")
    if route == "ours":
        assert len(calls) == 1 and calls[0][2].get("variant") == 0 and calls[0][1][5] == 2 * H
    else:       # the rotated Q | K columns and the V columns as two launches into one output
        assert len(calls) == 2
        (a0, kw0), (a1, kw1) = (calls[0][1], calls[0][2]), (calls[1][1], calls[1][2])
        assert a0[1].data_ptr() == w.data_ptr() and tuple(a0[1].shape) == (rot, K)
        assert a1[1].data_ptr() == w.data_ptr() + rot * K * 2 and tuple(a1[1].shape) == (Nn - rot, K)
        assert a0[2].data_ptr() == bias.data_ptr() and a1[2].data_ptr() == bias.data_ptr() + rot * 4
        assert a0[5] == 2 * H and a0[6] == hd and len(a1) == 3
        o0, o1 = kw0["out"], kw1["out"]
        assert o0.data_ptr() == y.data_ptr() and tuple(o0.shape) == (M, rot) and o0.stride() == (Nn, 1)
        assert o1.data_ptr() == y.data_ptr() + rot * 2 and tuple(o1.shape) == (M, Nn - rot) and o1.stride() == (Nn, 1)
    ref, rmag = N.ref_rope(lin, pos, tab, 2 * H, hd)
    acc = N.ref_rope(lin, pos, tab, 2 * H, hd, mag=N.acc_term_gemm(mag, K))[1]
    N.assert_within(y, ref, N.U16 * ref.abs() + acc + 3 * N.U32 * rmag, N.DERIVED, f"route {route} gemm_nt_rope hd {hd}", TILES)


def test_rope_not_fusable_head_dim_is_a_second_pass(k):
    """hd 32: the epilogue does not rotate it, the binding runs rope_ over the stored output."""
    M, H, hd, K = 300, 8, 32, 64
    Nn, x, w, bias, pos, tab, lin, mag = _rope_case(M, H, hd, K, seed=20)
    _seed_rope(M, Nn, K, hd, 2 * H * hd, False, "ours")
    y = GS.gemm_nt_rope(k, x, w, bias, pos, tab, 2 * H, hd)
    assert k.names() == ["gemm_nt"]
    ref, unit = I.unit_rope_two_pass(lin, N.acc_term_gemm(mag, K), pos, tab, 2 * H, hd)
    N.assert_within(y, ref, unit, N.DERIVED, "gemm_nt_rope hd 32 (two passes)", TILES)


def test_rope_unaligned_k(k):
    """K = 100: ``_unaligned`` (the fp32-input kernel, bf16 storage) followed by ``rope_``."""
    M, H, hd, K = 300, 4, 64, 100
    Nn, x, w, bias, pos, tab, lin, mag = _rope_case(M, H, hd, K, seed=30)
    y = GS.gemm_nt_rope(k, x, w, bias, pos, tab, 2 * H, hd)
    assert k.names() == ["gemm_f32", "rope_"] and not GS._choice
    f32_term = N.acc_term_gemm(mag, K + F32.gemm_splits_for_unit(K))
    ref, unit = I.unit_rope_two_pass(lin, f32_term, pos, tab, 2 * H, hd)
    N.assert_within(y, ref, unit, N.DERIVED, "gemm_nt_rope K 100 (unaligned + rope_)", TILES)


# --------------------------------------------------------- gate_up, down_dgrad_swiglu ----

@pytest.mark.parametrize("perm,K,fused", [(True, 64, True), (True, 96, False), (False, 64, False)])
def test_gate_up_routes(k, perm, K, fused):
    """The fused kernel (accepts K 64), its fallback (declines K 96: interleaved copies, the plain
    GEMM, the interleaved SwiGLU pass) and the natural layout, all against the natural-layout oracle."""
    M, F_ = 300, 320
    x, w = _randn(M, K, seed=40, scale=0.25), _randn(2 * F_, K, seed=41, scale=0.25)
    b = _randn(2 * F_, seed=42, dtype=torch.float32)
    seed_nt(M, 2 * F_, K, True, "ours")
    gu, h = GS.gate_up(k, x, w, b, perm)
    if fused:
        assert k.names() == ["gemm_nt_swiglu"]
    elif perm:
        assert k.names() == ["gemm_nt_swiglu", "gemm_nt", "swiglu_fwd"] and k.of("swiglu_fwd")[0][1][1] is True
        assert k.of("gemm_nt")[0][1][1].data_ptr() != w.data_ptr()         # the interleaved copy
    else:
        assert k.names() == ["gemm_nt", "swiglu_fwd"] and k.of("gemm_nt")[0][1][1].data_ptr() == w.data_ptr()
    ref, mag = N.ref_gemm(x, w, "nt", b)
    what = f"gate_up perm={perm} K {K}"
    N.assert_within(torch.cat(N.gu_unperm64(gu, perm), 1), ref, N.unit_gemm_bf16(ref, mag, K), N.DERIVED, what + " gu", TILES)
    href, hunit, _ = N.ref_swiglu_fwd(gu, perm=perm)        # h against the SwiGLU of the kernel's own gu
    N.assert_within(h, href, hunit, N.DERIVED, what + " h")


@pytest.mark.parametrize("perm", [True, False])
@pytest.mark.parametrize("K,fused", [(64, True), (96, False)])
def test_down_dgrad_swiglu_routes(k, K, fused, perm):
    """The fused epilogue, and its fallback at a shape dpfs_gemm4_nn_swiglu_bwd declines (K % 64 != 0):
    gemm_nn + swiglu_bwd.  Both round dy w to bf16 before the derivative, so one unit holds both."""
    M, F_ = 300, 320
    dy, w = _randn(M, K, seed=50, scale=0.25), _randn(K, F_, seed=51, scale=0.25)
    gu = _randn(M, 2 * F_, seed=52)
    db = torch.full((2 * F_,), float("nan"), device=DEV)
    seed_nn(M, F_, K, "ours")
    dgu = GS.down_dgrad_swiglu(k, dy, w, gu, db, perm)
    want = ["gemm_nn_swiglu_bwd"] if fused else ["gemm_nn_swiglu_bwd", "gemm_nn", "swiglu_bwd"]
    assert k.names() == want
    ds, mag = N.ref_gemm(dy, w, "nn")
    ref, unit, _, dbr, dbu = N.ref_swiglu_bwd(ds, gu, perm, dh_unit=N.unit_gemm_bf16(ds, mag, K))
    what = f"down_dgrad_swiglu fused={fused} perm={perm}"
    N.assert_within(dgu, ref, unit, N.DERIVED, what + " dgu", TILES)
    N.assert_within(db, dbr, dbu, N.DERIVED, what + " dbias")


# --------------------------------------------------------------------------- gemm_tn ----

def _tn_operands(K, M, Nn, seed):
    return _randn(K, M, seed=seed), _randn(K, Nn, seed=seed + 1)


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("given,accumulate", [(False, False), (True, False), (True, True)])
def test_gemm_tn_routes(C, k, given, accumulate, direct):
    """``ours`` through the run() closure (out as a keyword-less third argument with its variant) and
    the ``_direct`` branch (a kernel set called as it is), with ``out`` given and not."""
    K, M, Nn = 320, 264, 200
    if direct:
        k = Spy(C, direct=True)
    a, b = _tn_operands(K, M, Nn, 60)
    init = _randn(M, Nn, seed=62, dtype=torch.float32) if accumulate else torch.full((M, Nn), float("nan"), device=DEV)
    out = init.clone() if given else None
    seed_tn(M, Nn, K, accumulate, "ours")
    y = GS.gemm_tn(k, a, b, out, accumulate)
    call = k.of("gemm_tn")
    assert k.names() == ["gemm_tn"] and (given == (len(call[0][1]) == 4)) and (direct == ("variant" not in call[0][2]))
    assert (y.data_ptr() == out.data_ptr()) if given else True
    ref, mag = N.ref_gemm(a, b, "tn", acc=init if accumulate else None)
    S = max(1, C.gemm_tn_splits(M, Nn, K))
    N.assert_within(y, ref, N.unit_gemm_f32(mag, K, S, init if accumulate else None), N.DERIVED,
                    f"gemm_tn given={given} accumulate={accumulate} direct={direct}", TILES)


def _pair_ref(a0, b0, a1, b1, init):
    r0, m0 = N.ref_gemm(a0, b0, "tn")
    r1, m1 = N.ref_gemm(a1, b1, "tn")
    K = a0.size(0) + a1.size(0)
    ref = r0 + r1 + (init.double() if init is not None else 0)
    return ref, N.unit_gemm_f32(m0 + m1, K, I.cdiv(K, 64), init)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("route", ["pair", "split"])
def test_gemm_tn_pair_routes(k, route, accumulate):
    K0 = K1 = 512
    M, Nn = 136, 200
    a0, b0 = _tn_operands(K0, M, Nn, 70)
    a1, b1 = _tn_operands(K1, M, Nn, 72)
    init = _randn(M, Nn, seed=74, dtype=torch.float32)
    out = init.clone() if accumulate else torch.full((M, Nn), float("nan"), device=DEV)
    GS._choice[("tn2", M, Nn, K0, K1, accumulate, IDX)] = route
    seed_tn(M, Nn, K0, False), seed_tn(M, Nn, K0, True)
    y = GS.gemm_tn_pair(k, a0, b0, a1, b1, out, accumulate)
    assert k.names() == (["gemm_tn2"] if route == "pair" else ["gemm_tn", "gemm_tn"]) and y.data_ptr() == out.data_ptr()
    ref, unit = _pair_ref(a0, b0, a1, b1, init if accumulate else None)
    N.assert_within(y, ref, unit, N.DERIVED, f"gemm_tn_pair route {route} accumulate={accumulate}", TILES)


def test_gemm_tn_pair_plan_does_not_fit(k):
    """K0 = 320: no split length of at least 512 rows divides it, gemm_tn2 returns None; the result
    must come out through ``split`` and the selector must remember that."""
    K0, K1, M, Nn = 320, 512, 136, 200
    a0, b0 = _tn_operands(K0, M, Nn, 80)
    a1, b1 = _tn_operands(K1, M, Nn, 82)
    out = torch.full((M, Nn), float("nan"), device=DEV)
    seed_tn(M, Nn, K0, False), seed_tn(M, Nn, K1, True)
    y = GS.gemm_tn_pair(k, a0, b0, a1, b1, out, False)
    assert k.names() == ["gemm_tn2", "gemm_tn", "gemm_tn"]
    assert GS._choice[("tn2", M, Nn, K0, K1, False, IDX)] == "split"
    ref, unit = _pair_ref(a0, b0, a1, b1, None)
    N.assert_within(y, ref, unit, N.DERIVED, "gemm_tn_pair where the plan does not fit", TILES)


# --------------------------------------------------------------------- gemm_tn_group ----

GROUP = [(136, 200), (264, 96), (200, 136)]
GROUP_ACC = [True, False, True]


def _arena(shapes):
    """The members' gradients as a GradArena gives them out: views of one flat fp32 buffer, packed
    back to back in completion order with each weight's bias slot between (no alignment beyond the
    element), everything sentinel-filled first."""
    params = []
    for i, (m, n) in enumerate(shapes):
        params += [(f"w{i}", torch.empty(m, n, device="meta")), (f"b{i}", torch.empty(m, device="meta"))]
    arena = GradArena([("layer", params)], DEV)
    arena.buf.fill_(SENTINEL)
    return arena, [arena.view("layer", f"w{i}") for i in range(len(shapes))]


def _group_case(two, K=512, K1=512, seed=90):
    A = [_randn(K, m, seed=seed + i) for i, (m, _) in enumerate(GROUP)]
    B = [_randn(K, n, seed=seed + 10 + i) for i, (_, n) in enumerate(GROUP)]
    A2 = [_randn(K1, m, seed=seed + 20 + i) for i, (m, _) in enumerate(GROUP)] if two else [None] * 3
    B2 = [_randn(K1, n, seed=seed + 30 + i) for i, (_, n) in enumerate(GROUP)] if two else [None] * 3
    inits = [_randn(m, n, seed=seed + 40 + i, dtype=torch.float32) if acc else None
             for i, ((m, n), acc) in enumerate(zip(GROUP, GROUP_ACC))]
    return A, B, A2, B2, inits


def _group_outs(inits):
    arena, outs = _arena(GROUP)
    for o, init in zip(outs, inits):
        o.copy_(init if init is not None else torch.full_like(o, float("nan")))
    return arena, outs


def _group_items(A, B, A2, B2, outs, two):
    return [(a, b, o, acc) + ((a2, b2) if two else ()) for a, b, a2, b2, o, acc in zip(A, B, A2, B2, outs, GROUP_ACC)]


def _seed_group_each(K, K1, two):
    for (m, n), acc in zip(GROUP, GROUP_ACC):
        if two:
            GS._choice[("tn2", m, n, K, K1, acc, IDX)] = "pair"
        else:
            seed_tn(m, n, K, acc)


def _group_check(outs, arena, A, B, A2, B2, inits, two, what):
    for i in range(3):
        if two:
            ref, unit = _pair_ref(A[i], B[i], A2[i], B2[i], inits[i])
        else:
            ref, mag = N.ref_gemm(A[i], B[i], "tn", acc=inits[i])
            unit = N.unit_gemm_f32(mag, A[i].size(0), I.cdiv(A[i].size(0), 64), inits[i])
        N.assert_within(outs[i], ref, unit, N.DERIVED, f"{what} member {i}", TILES)
    for i, (m, _) in enumerate(GROUP):      # the bias slots between the views
        assert bool((arena.view("layer", f"b{i}") == SENTINEL).all()), f"{what}: the slot after member {i} was written"


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("route", ["group", "each"])
def test_gemm_tn_group_routes(k, route, two):
    K, K1 = 512, (512 if two else 0)
    A, B, A2, B2, inits = _group_case(two)
    arena, outs = _group_outs(inits)
    GS._choice[("tng",) + tuple((m, n, acc) for (m, n), acc in zip(GROUP, GROUP_ACC)) + (K, K1, IDX)] = route
    _seed_group_each(K, K1, two)
    r = GS.gemm_tn_group(k, _group_items(A, B, A2, B2, outs, two))
    assert k.names() == (["gemm_tn_group"] if route == "group" else ["gemm_tn2" if two else "gemm_tn"] * 3)
    assert all(x.data_ptr() == o.data_ptr() for x, o in zip(r, outs))
    _group_check(outs, arena, A, B, A2, B2, inits, two, f"gemm_tn_group route {route} two={two}")


@pytest.mark.parametrize("case", ["one_item", "out_none", "short_k", "different_k", "mixed_buffers", "group_off"])
def test_gemm_tn_group_early_returns_give_each(C, k, monkeypatch, case):
    """Every early return of gemm_tn_group is taken once: none may launch the group or record a
    group choice, and each must give, bit for bit, what ``each`` gives -- the member's own entry
    point (gemm_tn, or gemm_tn2 for a member with second buffers) on the same operands."""
    K = 128 if case == "short_k" else 512
    A, B, A2, B2, inits = _group_case(case == "mixed_buffers", K=K)
    if case == "different_k":
        A[1], B[1] = _randn(384, GROUP[1][0], seed=190), _randn(384, GROUP[1][1], seed=191)
    if case == "mixed_buffers":         # member 1 has no second buffers
        A2[1] = B2[1] = None
    accs = [False] * 3 if case == "out_none" else GROUP_ACC
    for i, ((m, n), acc) in enumerate(zip(GROUP, accs)):
        seed_tn(m, n, A[i].size(0), acc)
        if A2[i] is not None:
            GS._choice[("tn2", m, n, K, A2[i].size(0), acc, IDX)] = "pair"
    arena, outs = _group_outs(inits)
    items, want = [], []
    for i in range(1 if case == "one_item" else 3):
        out = None if case == "out_none" else outs[i]
        items.append((A[i], B[i], out, accs[i]) + ((A2[i], B2[i]) if case == "mixed_buffers" and A2[i] is not None else ()))
        dst = None if out is None else out.clone()
        if A2[i] is not None:
            want.append(C.gemm_tn2(A[i], B[i], A2[i], B2[i], dst, accs[i]))
        else:
            want.append(C.gemm_tn(A[i], B[i]) if dst is None else C.gemm_tn(A[i], B[i], dst, accs[i]))
    if case == "group_off":
        monkeypatch.setattr(GS, "TN_GROUP", False)
    r = GS.gemm_tn_group(k, items)
    assert "gemm_tn_group" not in k.names() and not [key for key in GS._choice if key[0] == "tng"], k.names()
    assert k.names() == ["gemm_tn2" if len(it) == 6 else "gemm_tn" for it in items]
    assert len(r) == len(want)
    for i, (x, w) in enumerate(zip(r, want)):
        assert w is not None and torch.equal(x, w), f"early return {case}: member {i} differs from the each result"
    if case != "out_none":
        assert all(x.data_ptr() == o.data_ptr() for x, o in zip(r, outs))


# ------------------------------------------------------------------------ _unaligned ----

def _bf16_storage_unit(ref, mag, K):
    return N.unit_gemm_bf16(ref, mag, K + F32.gemm_splits_for_unit(K))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("layout,M,Nn,K", [("nt", 300, 260, 100), ("nt", 300, 264, 1089), ("nn", 300, 260, 96), ("nn", 257, 96, 100)])
def test_unaligned_bf16_routes(k, layout, M, Nn, K, strided):
    """N or K no multiple of 8 through the entry points: the fp32-input kernel with bf16 storage;
    with ``out`` of unit last stride (written by the kernel) and of last stride 2 (copied into)."""
    a = _randn(M, K, seed=200)
    b = _randn(Nn, K, seed=201) if layout == "nt" else _randn(K, Nn, seed=201)
    bias = _randn(Nn, seed=202, dtype=torch.float32) if layout == "nt" else None
    buf = torch.full((M, 2 * Nn + 8), SENTINEL, device=DEV, dtype=torch.bfloat16)
    out = buf[:, 0:2 * Nn:2] if strided else buf[:, 4:4 + Nn]
    y = GS.gemm_nt(k, a, b, bias, out=out) if layout == "nt" else GS.gemm_nn(k, a, b, out=out)
    call = k.of("gemm_f32")
    assert k.names() == ["gemm_f32"] and call[0][1][2] == (0 if layout == "nt" else 1) and not GS._choice
    assert (call[0][1][4] is None) == strided and y.data_ptr() == out.data_ptr() and _pads_intact(buf, out)
    ref, mag = N.ref_gemm(a, b, layout, bias)
    N.assert_within(y, ref, _bf16_storage_unit(ref, mag, K), N.DERIVED,      # (the copy of a bf16 value is exact)
                    f"_unaligned {layout} {M}x{Nn}x{K} strided={strided}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,Nn,K", [(260, 200, 300), (264, 100, 1089)])
def test_unaligned_tn_routes(k, M, Nn, K, accumulate, strided):
    """Layout 2 (fp32 out), accumulating in the kernel (unit last stride) and through ``out.add_(c)``
    (last stride 2: one more fp32 addition, inside unit_gemm_f32's slack of 2)."""
    a, b = _tn_operands(K, M, Nn, 210)
    init = _randn(M, Nn, seed=212, dtype=torch.float32)
    buf = torch.full((M, 2 * Nn + 8), SENTINEL, device=DEV)
    out = buf[:, 0:2 * Nn:2] if strided else buf[:, 4:4 + Nn]
    out.copy_(init if accumulate else torch.full_like(init, float("nan")))
    y = GS.gemm_tn(k, a, b, out, accumulate)
    call = k.of("gemm_f32")
    assert k.names() == ["gemm_f32"] and call[0][1][2] == 2 and not GS._choice
    assert (call[0][1][4] is None) == strided and call[0][1][5] == (accumulate and not strided)
    assert y.data_ptr() == out.data_ptr() and _pads_intact(buf, out)
    ref, mag = N.ref_gemm(a, b, "tn", acc=init if accumulate else None)
    unit = N.unit_gemm_f32(mag, K, F32.gemm_splits_for_unit(K), init if accumulate else None)
    N.assert_within(y, ref, unit, N.DERIVED, f"_unaligned tn {M}x{Nn}x{K} accumulate={accumulate} strided={strided}")
