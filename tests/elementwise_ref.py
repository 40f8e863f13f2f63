"""References of the element-wise entries: csrc/optim.hip (fp64 with a propagated bound) and csrc/layout.hip (index expressions, equal as stored).

Same conventions as launch_ref.py: plain torch, tensors in, ``(ref, bnd)`` out for launch_ref.check_values; the layout references return the
result in the dtype the kernel stores and are compared with check_exact (the ``bnd == 0`` case: equal bit for bit, a NaN matching any NaN).
Everything runs on the device of its inputs, so the CPU tests and the GPU tests (which keep a 2^24-element case on the device) share it.
"""

from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32
RND = 1.01 * U            # the factor launch_ref.py puts on roundoff terms
DENORM = 2.0 ** -149      # absolute slack of one fp32 subnormal step

# Cost of sqrtf and of `/` in optim.hip, in unit roundoffs.  Finding (Makefile: -O3, no -ffast-math, hipcc's default
# -fhip-fp32-correctly-rounded-divide-sqrt; `tools/disasm.sh build/csrc/optim.o adam_kernel`): the division is the
# v_div_scale_f32 / v_rcp_f32 / v_fma_f32 chain / v_div_fmas_f32 / v_div_fixup_f32 sequence, i.e. IEEE division; sqrtf is
# v_sqrt_f32 followed by the two residual tests fma(-(s-1ulp), s, x) <= 0 and fma(-(s+1ulp), s, x) > 0 that move the result to the
# neighbour where needed (with the 2^32 pre-scale for tiny arguments), i.e. IEEE square root.  Both are correctly rounded: 1 u each.
SQRT_U = 1.0
DIV_U = 1.0


def _f32(x) -> float:
    return float(np.float32(x))


def adam_constants(lr, beta1, beta2, eps, wd, step, exact_constants=False):
    """the fp32 values yolo_adam_step* form on the host and in the kernel preamble, as Python floats:
    b1, b2, eps, wd (the float arguments), 1 - b1 and 1 - b2 (fp32 subtractions), step_size = (float)(lr / bc1), inv_bc2_sqrt = (float)(1 / sqrt(bc2))
    with bc = 1 - pow((double)beta, step) in double.  exact_constants: the derived four stay doubles (the formula itself, for a comparison with
    an fp64 torch.optim.Adam that was given the same fp32 hyper-parameters)"""
    b1, b2 = _f32(beta1), _f32(beta2)
    bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
    if exact_constants:
        return dict(b1=b1, b2=b2, eps=_f32(eps), wd=_f32(wd), omb1=1.0 - b1, omb2=1.0 - b2, step_size=_f32(lr) / bc1, inv_bc2_sqrt=1.0 / math.sqrt(bc2))
    return dict(b1=b1, b2=b2, eps=_f32(eps), wd=_f32(wd), omb1=_f32(np.float32(1.0) - np.float32(beta1)), omb2=_f32(np.float32(1.0) - np.float32(beta2)),
                step_size=_f32(_f32(lr) / bc1), inv_bc2_sqrt=_f32(1.0 / math.sqrt(bc2)))


def clip_ref(norm_sq, max_norm) -> float:
    """the clip coefficient of every optimizer kernel (clip_coefficient in csrc/multi_tensor.h; scale_by_clip_kernel: clip_ratio), bit for bit:
    total = (float)sqrt(double norm_sq); c = max_norm / (total + 1e-6f) in fp32; min(1, c).  norm_sq None (NULL): 1"""
    if norm_sq is None:
        return 1.0
    total = np.float32(np.sqrt(np.float64(norm_sq)))
    c = np.float32(max_norm) / (total + np.float32(1e-6))
    return float(c) if c < np.float32(1.0) else 1.0


def clip_raw(norm_sq, max_norm) -> float:
    """c before the min (scale_by_clip_kernel leaves g alone when c >= 1)"""
    total = np.float32(np.sqrt(np.float64(norm_sq)))
    return float(np.float32(max_norm) / (total + np.float32(1e-6)))


def _rnd(val, err, cost=1.0):
    """error of a computed fp32 result whose exact-arithmetic value is `val` when its operands carried `err`: the propagated error plus one
    rounding of the value actually formed (|val| + err at most)"""
    return err + cost * RND * (val.abs() + err)


def adam_ref(p, g, m, v, *, lr, beta1, beta2, eps, wd, step, norm_sq, max_norm, exact_constants=False):
    """fp64 (p', m', v') of one adam1 call of optim.hip on fp32 tensors, and a bound for each, from carrying (value, |error|) through adam1 as written:

        g = g * clip;  g = g + wd * p;  m = m + (g - m) * (1 - b1);  v = v * b2 + ((1 - b2) * g) * g;
        denom = sqrtf(v) * inv_bc2_sqrt + eps;  p = p - step_size * (m / denom)

    one unit roundoff 2^-24 (times 1.01) per fp32 operation, SQRT_U / DIV_U for sqrtf and `/` (both 1: see the constants above), the constants being
    the fp32 values of adam_constants / clip_ref, plus 2^-149 absolute.  optim.hip is built with FMA contraction allowed: a fused a * b + c rounds once
    where this model charges the product and the sum separately, so the unfused bound holds for either code generation (and for the three kernels,
    which need not contract alike).  Inputs must keep every intermediate in the normal range (|g| >= 1e-15 so that g * g is normal).
    -> (p', m', v'), (bound_p, bound_m, bound_v), all fp64 on the inputs' device."""
    k = adam_constants(lr, beta1, beta2, eps, wd, step, exact_constants)
    clip = clip_ref(norm_sq, max_norm)
    P, G, M, V = (t.double() for t in (p, g, m, v))
    zero = torch.zeros_like(P)
    g1 = G * clip
    e_g1 = _rnd(g1, zero)
    t = k["wd"] * P
    e_t = _rnd(t, zero)
    g2 = g1 + t
    e_g2 = _rnd(g2, e_g1 + e_t)
    d = g2 - M
    e_d = _rnd(d, e_g2)
    q = d * k["omb1"]
    e_q = _rnd(q, e_d * k["omb1"])
    m2 = M + q
    e_m = _rnd(m2, e_q)
    a = V * k["b2"]
    e_a = _rnd(a, zero)
    b = k["omb2"] * g2
    e_b = _rnd(b, k["omb2"] * e_g2)
    c = b * g2
    e_c = _rnd(c, e_b * g2.abs() + b.abs() * e_g2 + e_b * e_g2)
    v2 = a + c
    e_v = _rnd(v2, e_a + e_c)
    s = v2.clamp_min(0.0).sqrt()
    e_s = _rnd(s, s - (v2 - e_v).clamp_min(0.0).sqrt(), SQRT_U)       # sqrt is concave: the downward side is the larger one
    d1 = s * k["inv_bc2_sqrt"]
    e_d1 = _rnd(d1, e_s * k["inv_bc2_sqrt"])
    den = d1 + k["eps"]
    e_den = _rnd(den, e_d1)
    r = m2 / den
    e_r = _rnd(r, (e_m + r.abs() * e_den) / (den - e_den).clamp_min(DENORM), DIV_U)
    t2 = k["step_size"] * r
    e_t2 = _rnd(t2, k["step_size"] * e_r)
    p2 = P - t2
    e_p = _rnd(p2, e_t2)
    return (p2, m2, v2), (e_p + DENORM, e_m + DENORM, e_v + DENORM)


def adam1_fp32(p, g, m, v, *, lr, beta1, beta2, eps, wd, step, norm_sq, max_norm):
    """adam1 in torch fp32, one rounding per operation (no fused multiply-add): what a build without contraction computes -> (p', m', v') fp32"""
    k = adam_constants(lr, beta1, beta2, eps, wd, step)
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    g = g * f(clip_ref(norm_sq, max_norm))
    g = g + f(k["wd"]) * p
    m = m + (g - m) * f(k["omb1"])
    v = v * f(k["b2"]) + (f(k["omb2"]) * g) * g
    denom = v.sqrt() * f(k["inv_bc2_sqrt"]) + f(k["eps"])
    p = p - f(k["step_size"]) * (m / denom)
    return p, m, v


def sumsq_ref(g, acc0=0.0, n_total=None):
    """(ref, bnd) of *acc after yolo_sumsq_f32 / _multi added sum(g^2) onto acc0 (both kernels: float4 groups, s += (double)(x*x + y*y) +
    (double)(z*z + w*w), scalar tail s += (double)(g*g); wave shuffles, four partials and the atomics in double).

    Every square is one fp32 rounding and every pair sum one more: a pair carries (1 + u)^2 - 1 <= 2.02 u relative (a fused x*x + y*y rounds less).
    Everything after is an fp64 sum of non-negative terms: a term passes at most n roundings of 2^-53 whatever the order of the atomics (one per
    two-pair add and per loop trip of its thread, 6 shuffle steps, 3 partial adds, one atomic per workgroup -- never more than the elements that
    were added), each relative to a partial sum that is <= the total.  So |got - ref| <= 2.02 u sum(g^2) + n 2^-53 ref, ref = acc0 + sum(g^2)."""
    gs = [g] if isinstance(g, torch.Tensor) else list(g)
    s = sum(float((t.double() ** 2).sum()) for t in gs)
    n = n_total if n_total is not None else sum(t.numel() for t in gs)
    ref = float(acc0) + s
    return ref, 2.02 * U * s + n * 2.0 ** -53 * ref


# ---- layout.hip: index expressions, equal as stored -------------------------------------------------------------------------------------------------

BF = torch.bfloat16


def exact(ref):
    """(ref, bnd) with bnd == 0 for launch_ref.check_values (finite values; check_exact also tells -0 from 0 and accepts NaN for NaN)"""
    return ref.double(), torch.zeros(ref.shape, dtype=torch.float64, device=ref.device)


_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}


def check_exact(ref, got, tag, fails, what=""):
    """got == ref as stored (same dtype, same bits; a NaN matches any NaN).  Appends a message to `fails`; -> number of differing elements"""
    r, g = ref.reshape(-1).cpu(), got.reshape(-1).cpu()
    if r.dtype != g.dtype or r.numel() != g.numel():
        fails.append(f"{what}: {tag}: got {g.dtype}[{g.numel()}], reference {r.dtype}[{r.numel()}]")
        return g.numel()
    it = _INT[r.element_size()]
    bad = r.contiguous().view(it) != g.contiguous().view(it)
    if r.is_floating_point():
        bad &= ~(torch.isnan(r) & torch.isnan(g))
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad).flatten()[0])
        fails.append(f"{what}: {n} of {r.numel()} {tag} elements differ (first: element {i}: got {float(g[i])!r}, ref {float(r[i])!r})")
    return n


def nchw_to_nhwc_ref(x, Cpad, lo, hi, init):
    """yolo_nchw_f32_to_nhwc_bf16: x fp32 [N][C][H][W] -> init [N][H+lo+hi][W+lo+hi][Cpad] bf16 with the interior replaced (channels >= C zero)"""
    N, C, H, W = x.shape
    out = init.clone()
    out[:, lo:lo + H, lo:lo + W, :] = 0
    out[:, lo:lo + H, lo:lo + W, :C] = x.permute(0, 2, 3, 1).to(BF)
    return out


def nhwc_to_nchw_ref(x, halo, dtype):
    """yolo_nhwc_bf16_to_nchw_f32 / _bf16: x bf16 [N][H+2h][W+2h][C] -> [N][C][H][W]"""
    H, W = x.shape[1] - 2 * halo, x.shape[2] - 2 * halo
    return x[:, halo:halo + H, halo:halo + W].permute(0, 3, 1, 2).to(dtype).contiguous()


def pack_conv_fwd_ref(w, Cinp, KWp):
    """[Cout][KH][KWp][Cinp] bf16, padding zero"""
    Co, Ci, KH, KW = w.shape
    out = torch.zeros(Co, KH, KWp, Cinp, dtype=BF)
    out[:, :, :KW, :Ci] = w.permute(0, 2, 3, 1).to(BF)
    return out


def pack_conv_dgrad_ref(w):
    """[Cin][KH][KW][Cout] bf16 with the taps flipped"""
    return w.flip(2, 3).permute(1, 2, 3, 0).to(BF).contiguous()


def unpack_conv_wgrad_ref(dwp, Cin, KW, dw0, accumulate):
    """packed fp32 [Cout][KH][KWp][Cinp] -> OIHW; accumulate: one fp32 add onto dw0"""
    v = dwp[:, :, :KW, :Cin].permute(0, 3, 1, 2).contiguous()
    return dw0 + v if accumulate else v


def pack_fc_ref(w, C, HW):
    """w [O][C*HW] fp32 -> ([O][HW*C] bf16 with the K axis in (hw, c) order, its transpose [HW*C][O])"""
    O = w.shape[0]
    wf = w.view(O, C, HW).permute(0, 2, 1).reshape(O, HW * C).to(BF).contiguous()
    return wf, wf.t().contiguous()


def pack_fc_blocked_ref(w):
    """w [O][K] fp32 -> bf16 panels [ceil(O/128)][K/64][128][64], rows >= O zero"""
    O, K = w.shape
    nb = (O + 127) // 128
    full = torch.zeros(nb * 128, K, dtype=BF)
    full[:O] = w.to(BF)
    return full.view(nb, 128, K // 64, 64).permute(0, 2, 1, 3).contiguous()


def pack_fc_blocked_hwc_ref(w, C, HW):
    O = w.shape[0]
    return pack_fc_blocked_ref(w.view(O, C, HW).permute(0, 2, 1).reshape(O, HW * C).contiguous())


def transpose_f32_to_bf16_ref(x, ld, init):
    """x fp32 [R][Cc] -> init [Cc][ld] bf16 with columns < R replaced"""
    out = init.clone()
    out[:, : x.shape[0]] = x.t().to(BF)
    return out


def transpose_bf16_ref(x, Cc, init):
    """x bf16 [R][ldx] -> init [Cc][ldy] with columns < R replaced by the transpose of x[:, :Cc]"""
    out = init.clone()
    out[:, : x.shape[0]] = x[:, :Cc].t()
    return out


def im2col_rows_ref(x, img_stride, row_stride, px_stride, stride, KH, seg, N, Ho, Wo, ho, init):
    """xcol[n][oy+ho][ox+ho][ky*seg + j] = x[n*img + (oy*stride + ky)*row + ox*stride*px + j]; x flat bf16, init [N][Ho+2ho][Wo+2ho][KH*seg]"""
    src = x.as_strided((N, Ho, Wo, KH, seg), (img_stride, stride * row_stride, stride * px_stride, row_stride, 1), x.storage_offset())
    out = init.clone()
    out[:, ho:ho + Ho, ho:ho + Wo] = src.reshape(N, Ho, Wo, KH * seg)
    return out


def bias_lrelu_rows_ref(x, bias, slope):
    """x fp32 [slabs][R][Cc]: v = x[0] + x[1] + .. in index order, + bias[c] (NULL: + 0.0f), v > 0 ? v : v * slope, all fp32 -> (bf16, fp32).
    None of these operations can contract (no product feeds a sum), so torch fp32 on the CPU gives the same bits."""
    v = x[0].clone()
    for s in range(1, x.shape[0]):
        v = v + x[s]
    v = v + (bias if bias is not None else torch.zeros((), dtype=torch.float32))
    v = torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    return v.to(BF), v


def scale_rows_ref(x, mask, scale, act, slope, ld):
    """bf16( x * (mask ? scale : 0) * (act > 0 ? 1 : slope) ), [R][ld] with columns >= Cc zero"""
    R, Cc = x.shape
    one = torch.ones((), dtype=torch.float32)
    v = x.clone()
    if mask is not None:
        v = v * torch.where(mask != 0, torch.tensor(scale, dtype=torch.float32), 0.0 * one)
    if act is not None:
        v = v * torch.where(act.float() > 0, one, torch.tensor(slope, dtype=torch.float32))
    out = torch.zeros(R, ld, dtype=BF)
    out[:, :Cc] = v.to(BF)
    return out


def dropout_ref(x, mask, scale):
    """mask ? bf16(float(x) * scale) : +0"""
    return torch.where(mask != 0, (x.float() * torch.tensor(scale, dtype=torch.float32)).to(BF), torch.zeros((), dtype=BF))


def fc_dgrad_to_nhwc_ref(dxT, N, C, H, W, halo, yact, slope, init):
    """dxT fp32 [C*H*W][N] -> init [N][H+2h][W+2h][C] bf16 with the interior replaced by bf16(v * (yact > 0 ? 1 : slope)) (yact None: v)"""
    v = dxT.view(C, H, W, N).permute(3, 1, 2, 0)
    if yact is not None:
        ya = yact[:, halo:halo + H, halo:halo + W].float()
        v = torch.where(ya > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    out = init.clone()
    out[:, halo:halo + H, halo:halo + W] = v.to(BF)
    return out


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------------------

GUARD = 256                                                                                  # elements on either side (>= 512 B)
GUARD_PAT = {torch.float32: (torch.int32, 0x7FC00D1E), BF: (torch.int16, 0x7FC1), torch.uint8: (torch.uint8, 0xA5)}   # NaN payloads no result equals


class Guarded:
    """a copy of `src` (any shape, on its device) between two guard bands inside one allocation: .t is the view a kernel writes, .ptr its address
    (valid and 512-B aligned also for an empty tensor), guards_ok() whether both bands still hold their pattern"""

    def __init__(self, src, dtype=None):
        dtype = dtype or src.dtype
        it, pat = GUARD_PAT[dtype]
        self.n = src.numel()
        self.raw = torch.full((self.n + 2 * GUARD,), pat, dtype=it, device=src.device)
        self.t = self.raw.view(dtype)[GUARD: GUARD + self.n]
        self.t.copy_(src.reshape(-1))
        self.shape = tuple(src.shape)
        self.pat = pat

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.raw.element_size()

    def guards_ok(self):
        return bool((self.raw[:GUARD] == self.pat).all()) and bool((self.raw[GUARD + self.n:] == self.pat).all())
