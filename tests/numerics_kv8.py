"""Helpers of the fp8 KV cache tests (tests/test_kv_fp8.py on the CPU, tests/test_kv_fp8_gpu.py on
the MI355X): an independent quantiser written from the format's contract, the fp64 oracle and
derived unit of the fp8 decode attention, and an fp32 emulation of the kernel's scheme with
planted faults.

The contract (one row = the hd bf16 values of one (sequence, cache row, head)):

    amax  = max(max_j |f32(x_j)|, 1e-12f)
    scale = 448.f / amax                              IEEE fp32 division
    code_j = e4m3fn(clamp(f32(x_j) * scale, +-448))   fp32 product, round to nearest even
    inv   = 1.f / scale                               IEEE fp32 division; the stored scale
    value_j = f32(code_j) * inv

``quant_rows`` does not use the framework's fp8 conversion for the rounding: it rounds to the
e4m3 grid by arithmetic (the spacing of e4m3 at |y| is 2^(max(floor(log2 |y|), -6) - 3); y / spacing
is exact in fp32; torch.round is half-to-even) and only then stores the exactly representable
result as float8_e4m3fn.
"""
import torch

import numerics as N

# max over the CPU test's cases of the relative Frobenius error of fp8-cache logits against
# exact-cache logits on the oracle path (fp32 CPU math), recorded from tests/test_kv_fp8.py
# (test_model_logits_error_of_the_fp8_cache prints every case); the GPU model test allows this
# plus the project's 3e-2 for bf16 kernel paths against the fp32 recompute.
KV8_LOGITS_REL = 4.8e-3      # measured 4.741e-3 (the ragged batch's first generated step)

F8 = torch.float8_e4m3fn
NAN_CODE = 0x7F


def quant_rows(x):
    """x [..., hd] (bf16 or fp32 holding bf16 values) -> (codes [..., hd] float8_e4m3fn, inv [...]
    fp32), by the contract above."""
    xf = x.float()
    amax = torch.maximum(xf.abs().amax(-1, keepdim=True), torch.tensor(1e-12, dtype=torch.float32, device=x.device))
    scale = torch.tensor(448.0, dtype=torch.float32, device=x.device) / amax
    y = torch.clamp(xf * scale, -448.0, 448.0)
    _, e = torch.frexp(y)                                   # |y| in [2^(e-1), 2^e)
    step = torch.exp2((torch.clamp(e - 1, min=-6) - 3).float())
    grid = torch.round(y / step) * step                     # half to even on the e4m3 grid
    codes = grid.to(F8)
    assert torch.equal(codes.float(), grid), "the rounded values must be e4m3 numbers"
    return codes, (torch.tensor(1.0, dtype=torch.float32, device=x.device) / scale).squeeze(-1)


def dequant64(c8, inv):
    """The exact value of every cached element, fp64: d(code) * d(inv)."""
    return c8.float().double() * inv.double()[..., None]


def dequant_bf16(c8, inv):
    """bf16_rn(f32(code) * inv): what the extend kernel feeds its MFMAs."""
    return (c8.float() * inv[..., None]).bfloat16()


def quant_cache(c):
    """A bf16 cache (B, T, H, hd) -> (codes, inv (B, T, H))."""
    return quant_rows(c)


def blank_past(c8, cs, lens, nan):
    """Copies of (codes, scales) with every row past a sequence's attended keys set to NaN codes
    (0x7f) and NaN scales (``nan`` True) or to zeros."""
    c8, cs = c8.clone(), cs.clone()
    L = N.dec_attended(torch.tensor(lens), c8.size(1))
    for b in range(c8.size(0)):
        c8.view(torch.uint8)[b, int(L[b]):] = NAN_CODE if nan else 0
        cs[b, int(L[b]):] = float("nan") if nan else 0.0
    return c8, cs


def ref_attn_decode_q8(q, k8, v8, ks, vs, lens, scale):
    """fp64 oracle of ``_attn_decode_q8`` over the exactly dequantised caches d(code) d(inv), and
    its unit: the derivation of ``numerics.ref_attn_decode`` with one more fp32 rounding per side.
    The score is ks (sum of hd FMAs of the rounded q scale and the exact codes): (hd + 3) U32 in
    place of (hd + 2); the value's scale is folded into p by one fp32 product in front of the P V
    FMAs: one more U32 sum p |v| in the output term.  Rows past the attended keys are not read
    (NaN codes and scales there)."""
    B, Tmax, H, hd = k8.shape
    U32, U16, d = N.U32, N.U16, N.d
    L = N.dec_attended(lens, Tmax).to(k8.device)
    live = torch.arange(Tmax, device=k8.device)[None, :] < L[:, None]
    z = torch.zeros((), dtype=torch.float64, device=k8.device)
    k = torch.where(live[:, :, None, None], dequant64(k8, ks), z).permute(0, 2, 1, 3)    # [B, H, T, hd]
    v = torch.where(live[:, :, None, None], dequant64(v8, vs), z).permute(0, 2, 1, 3)
    qh = d(q)[:, : H * hd].reshape(B, H, 1, hd)
    s = (qh * k).sum(-1) * scale
    smag = (qh.abs() * k.abs()).sum(-1) * scale
    s = torch.where(live[:, None, :], s, torch.full_like(s, float("-inf")))
    p = torch.softmax(s, -1)
    A = torch.where(live[:, None, :], s.abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
    e = U32 * ((hd + 3) * smag + 6 * A + 3 * (3 + 2 * A) + 2)
    o = (p[..., None] * v).sum(2)
    pv = (p[..., None] * v.abs()).sum(2)
    err = ((p * e)[..., None] * v.abs()).sum(2) + pv * (p * e).sum(-1, keepdim=True)
    Lf = L.double().view(B, 1, 1)
    unit = U16 * o.abs() + err + (2 * (Lf + 1) + 3 + 1) * U32 * pv
    return o.reshape(B, H * hd), unit.reshape(B, H * hd)


KV8_FAULTS = ("k_scale_ignored", "v_scale_neighbour", "scale_head")


def emu_attn_decode_q8(q, k8, v8, ks, vs, lens, scale, fault=None):
    """fp32 evaluation of the fp8 decode kernels on the CPU: ``numerics.emu_attn_decode``'s
    splits, waves and merges, with the score ks[key] * sum_j q_j f32(code_j) and the value's scale
    folded into p (the row sum keeps the unscaled p).  ``fault`` = (name, b, h) plants on one
    (sequence, head): "k_scale_ignored" (the score without ks), "v_scale_neighbour" (vs of key
    t + 1), "scale_head" (both scales read from head h + 1)."""
    B, Tmax, H, hd = k8.shape
    L = N.dec_attended(lens, Tmax)
    Tp = (Tmax + 255) // 256 * 256
    ns = Tp // 256
    live = (torch.arange(Tp)[None, None, :] < L.view(B, 1, 1)).expand(B, H, Tp)
    pad = lambda c: torch.cat([c.float(), torch.zeros(B, Tp - Tmax, *c.shape[2:])], 1)
    k, v = torch.nan_to_num(pad(k8)).permute(0, 2, 1, 3), torch.nan_to_num(pad(v8)).permute(0, 2, 1, 3)
    ksp, vsp = torch.nan_to_num(pad(ks)).permute(0, 2, 1).clone(), torch.nan_to_num(pad(vs)).permute(0, 2, 1).clone()
    if fault:
        name, fb, fh = fault
        if name == "k_scale_ignored":
            ksp[fb, fh] = 1.0
        elif name == "v_scale_neighbour":
            vsp[fb, fh] = torch.roll(vsp[fb, fh], -1)
        elif name == "scale_head":
            ksp[fb, fh], vsp[fb, fh] = ksp[fb, (fh + 1) % H].clone(), vsp[fb, (fh + 1) % H].clone()
        else:
            raise ValueError(name)
    qf = q.float()[:, : H * hd].reshape(B, H, 1, hd) * torch.tensor(scale, dtype=torch.float32)
    s = torch.zeros(B, H, Tp)
    for i in range(hd):
        s += qf[..., i] * k[..., i]
    s = s * ksp
    s = torch.where(live, s, torch.full_like(s, float("-inf"))).view(B, H, ns, 4, 64)
    vw = v.reshape(B, H, ns, 4, 64, hd)
    m = s.max(-1).values
    fin = torch.isfinite(m)
    p = torch.where(fin[..., None], torch.exp(s - torch.where(fin, m, torch.zeros_like(m))[..., None]), torch.zeros_like(s))
    lsum = p.sum(-1)
    ow = ((p * vsp.view(B, H, ns, 4, 64))[..., None] * vw).sum(-2)
    Ms = m.max(-1).values
    sfin = torch.isfinite(Ms)
    f = torch.where(fin, torch.exp(m - torch.where(sfin, Ms, torch.zeros_like(Ms))[..., None]), torch.zeros_like(m))
    acc = (f[..., None] * ow).sum(-2)
    ls = (f * lsum).sum(-1)
    Mg = Ms.max(-1).values
    f2 = torch.where(sfin, torch.exp(Ms - Mg[..., None]), torch.zeros_like(Ms))
    num = (f2[..., None] * acc).sum(-2)
    den = (f2 * ls).sum(-1)
    return (num * (1.0 / den)[..., None]).reshape(B, H * hd).to(torch.bfloat16)


# ---- special rows of the append tests (values exact in bf16)

def tie_row(hd):
    """amax 448, so scale exactly 1: 17, 19, 34, 38, 272 sit halfway between e4m3 numbers and
    round to the even ones 16, 20, 32, 40, 256."""
    r = torch.zeros(hd)
    r[:6] = torch.tensor([448.0, 17.0, 19.0, 34.0, 38.0, 272.0])
    return r


TIE_WANT = (448.0, 16.0, 20.0, 32.0, 40.0, 256.0)


def outlier_row(hd, gen):
    r = torch.randn(hd, generator=gen)
    r[hd // 2] = 2.0 ** 10
    return r
