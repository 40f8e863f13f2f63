"""Reference of the SGD entries of csrc/sgd.hip (yolo_sgd_step, yolo_sgd_step_multi, yolo_sgd_step_multi_bg) and of yolo.optim.SGD's CPU path:
torch.optim.SGD's recurrence (maximize=False) behind the folded clip_grad_norm_, in fp64 from the fp32 inputs, with a per-element bound carried
through every fp32 operation the way elementwise_ref.adam_ref carries it -- and the same recurrence restated in torch fp32.

    g = grad * clip ; g = g + wd * p (wd != 0) ; buf = first_step ? g : momentum * buf + (1 - dampening) * g ; g = nesterov ? g + momentum * buf : buf
    (momentum != 0) ; p = p - lr * g

Same conventions as elementwise_ref.py: tensors in, ``(ref, bnd)`` out for launch_ref.check_values, everything on the device of the inputs.
"""

from __future__ import annotations

import torch

from elementwise_ref import DENORM, _f32, _rnd, clip_ref


def sgd_constants(lr, momentum, dampening, wd):
    """the fp32 values the kernels work with, as Python floats: lr, momentum, wd are the float arguments of the C entries; omd is
    (float)(1.0 - (double)dampening) with dampening the float argument (sgd_args in sgd.hip).  torch.optim.SGD hands its kernels the
    Python floats, which they narrow to the tensors' fp32 -- the same values for lr / momentum / wd, and fp32(1 - dampening) for omd,
    which differs from the entry's only when 1 - fp32(dampening) lies within 2^-30 or so of a rounding boundary (not for 0 or 0.1)."""
    return dict(lr=_f32(lr), momentum=_f32(momentum), wd=_f32(wd), omd=_f32(1.0 - _f32(dampening)))


def sgd_ref(p, g, buf, *, lr, momentum, dampening, wd, nesterov, first_step, norm_sq, max_norm, clip=None):
    """fp64 (p', buf') of one sgd1 call of sgd.hip on fp32 tensors and a bound for each, from carrying (value, |error|) through the recurrence:
    one unit roundoff 2^-24 (times 1.01) per fp32 operation, products and the sums they feed charged separately, plus 2^-149 absolute.  The kernels
    fuse every a * b + c (one rounding where this model charges two) and stock torch may or may not: the unfused bound holds for both.  The constants
    are the fp32 values of sgd_constants / elementwise_ref.clip_ref.  `buf` is not read when first_step or momentum == 0 (may be None); buf' and its
    bound are None when momentum == 0.  Inputs must keep every intermediate in the normal range.  `clip`: the fp32 coefficient a caller's own clipping
    applied, in place of clip_ref(norm_sq, max_norm) (torch's clip_grad_norm_ forms reciprocal(total + 1e-6) * max_norm, two roundings where the
    kernels divide once: the two coefficients differ in the last bit for some totals).
    -> (p', buf'), (bound_p, bound_buf), fp64 on the inputs' device."""
    k = sgd_constants(lr, momentum, dampening, wd)
    clip = clip_ref(norm_sq, max_norm) if clip is None else float(clip)
    P, G = p.double(), g.double()
    zero = torch.zeros_like(P)
    g2 = G * clip
    e_g2 = _rnd(g2, zero)
    if k["wd"] != 0.0:
        t = k["wd"] * P
        e_t = _rnd(t, zero)
        g2, e_g1 = g2 + t, e_g2
        e_g2 = _rnd(g2, e_g1 + e_t)
    b2 = e_b = None
    g3, e_g3 = g2, e_g2
    if k["momentum"] != 0.0:
        if first_step:
            b2, e_b = g2, e_g2                       # the stored copy of the computed g
        else:
            a = k["momentum"] * buf.double()
            e_a = _rnd(a, zero)
            q = k["omd"] * g2
            e_q = _rnd(q, k["omd"] * e_g2)
            b2 = a + q
            e_b = _rnd(b2, e_a + e_q)
        g3, e_g3 = b2, e_b
        if nesterov:
            r = k["momentum"] * b2
            e_r = _rnd(r, k["momentum"] * e_b)
            g3 = g2 + r
            e_g3 = _rnd(g3, e_g2 + e_r)
    s = k["lr"] * g3
    e_s = _rnd(s, k["lr"] * e_g3)
    p2 = P - s
    e_p = _rnd(p2, e_s)
    return (p2, b2), (e_p + DENORM, e_b + DENORM if e_b is not None else None)


def sgd1_fp32(p, g, buf, *, lr, momentum, dampening, wd, nesterov, first_step, norm_sq, max_norm):
    """the recurrence in torch fp32, one rounding per operation (no fused multiply-add) -> (p', buf' or None) fp32"""
    k = sgd_constants(lr, momentum, dampening, wd)
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    g = g * f(clip_ref(norm_sq, max_norm))
    if k["wd"] != 0.0:
        g = g + f(k["wd"]) * p
    if k["momentum"] != 0.0:
        buf = g.clone() if first_step else f(k["momentum"]) * buf + f(k["omd"]) * g
        g = g + f(k["momentum"]) * buf if nesterov else buf
    else:
        buf = None
    return p - f(k["lr"]) * g, buf


def bf16_bits(x):
    """x fp32 -> the bits of bf16(x), round to nearest even, as int16 (what the kernels store into a shadow)"""
    return x.to(torch.bfloat16).view(torch.int16)


# the hyper-parameter combinations both test files run: momentum 0 / 0.9, dampening 0 / 0.1, nesterov on / off (only legal with momentum and no
# dampening), weight decay 0 / 5e-4
HYPERS = [dict(momentum=m, dampening=d, nesterov=n, wd=wd)
          for m in (0.0, 0.9) for d in (0.0, 0.1) for n in (False, True) for wd in (0.0, 5e-4)
          if not (n and (m == 0.0 or d != 0.0))]


def hyper_id(h):
    return f"m{h['momentum']}-d{h['dampening']}-{'nesterov' if h['nesterov'] else 'plain'}-wd{h['wd']}"

