"""Reference of the LARS entries of csrc/lars.hip (yolo_lars_norms_multi; yolo_lars_step, yolo_lars_step_multi, yolo_lars_step_multi_bg) and of
yolo.optim.LARS's CPU path, in the manner of sgd_ref.py:

* ``norm_order_ref``: the per-tensor sum of squares restated in numpy in the kernels' own order -- lars.hip is built without FMA contraction, so a
  float4 is fp32(fp32(x*x) + fp32(y*y)) and fp32(fp32(z*z) + fp32(w*w)), widened and added in double; a lane adds its groups in rising order; the
  wave shuffles (offsets 32 .. 1), part[0] + part[1] + part[2] + part[3], one slot per 65536-element slice; the finish kernel's thread-strided, then
  rising order over a tensor's slots.  Bit for bit what the device stores.
* ``trust_ref``: the trust ratio in float64 narrowed to float32, as lars_trust states it.
* ``lars_ref``: the step in fp64 from the fp32 inputs with a per-element bound carried through every fp32 operation (one unit roundoff each, products
  and the sums they feed charged separately: holds for the fused kernels and for unfused stock torch), the trust ratio carrying 2 fp32 ulps.
* ``lars1_fp32``: the recurrence in torch fp32, one rounding per operation.

    g = grad * clip ; g = g + wd * p (wd != 0) ; g = g * trust ; buf = first_step ? g : momentum * buf + g (momentum != 0) ; p = p - lr * buf
"""

from __future__ import annotations

import math

import numpy as np
import torch

from elementwise_ref import DENORM, _f32, _rnd, clip_ref

SQ_CHUNK = 65536          # elements per workgroup of the norm pass (multi_tensor.h)
TRUST_ULPS = 2.0          # fp32 ulps the bound grants the device's trust ratio (fp64 sqrt, division and the narrowing)


# ---- the norm pass, in its own order ------------------------------------------------------------------------------------------------------------------

def _wg_sumsq(x: np.ndarray) -> np.float64:
    """one 256-thread workgroup over a slice of <= SQ_CHUNK fp32 elements (wg_sumsq in multi_tensor.h with i0 = 4 * thread, stride 1024)"""
    n = x.size
    sq = x * x                                                    # fp32, one rounding each
    nfull, rem = n // 4, n % 4
    q = sq[:4 * nfull].reshape(nfull, 4)
    d = (q[:, 0] + q[:, 1]).astype(np.float64) + (q[:, 2] + q[:, 3]).astype(np.float64)      # fp32 pair sums, widened, added in double
    trips = -(-(nfull + (1 if rem else 0)) // 256) if n else 0
    grid = np.zeros((max(trips, 1), 256), dtype=np.float64)
    grid.reshape(-1)[:nfull] = d                                  # group k belongs to lane k % 256, trip k // 256
    s = np.zeros(256, dtype=np.float64)
    for j in range(trips):
        s = s + grid[j]                                           # (+ 0.0 where the lane has no group in this trip: exact)
    if rem:                                                       # the scalar tail: the lane that owns group nfull, behind its full groups
        lane = nfull % 256
        for k in range(4 * nfull, n):
            s[lane] = s[lane] + np.float64(sq[k])
    w = s.reshape(4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):                              # s += __shfl_down(s, off, 64): lane 0 ends with this tree
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def norm_order_ref(x) -> float:
    """norms[k] of one tensor: the slices' workgroup sums, then lars_norm_finish_kernel's order (thread t: slots t, t + 256, .. rising; the 256
    thread sums rising)"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
    slots = [_wg_sumsq(x[b:b + SQ_CHUNK]) for b in range(0, x.size, SQ_CHUNK)]
    red = np.zeros(256, dtype=np.float64)
    for i, v in enumerate(slots):
        red[i % 256] = red[i % 256] + v
    t = red[0]
    for k in range(1, 256):
        t = t + red[k]
    return float(t)


def g_total_ref(norms) -> float:
    """*g_total: norms[1] + norms[3] + .. in rising tensor order, from 0.0"""
    t = np.float64(0.0)
    for v in list(norms)[1::2]:
        t = t + np.float64(v)
    return float(t)


def exact_sumsq(x) -> float:
    """math.fsum of the exact squares (an fp32 square is exact in double)"""
    v = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    return math.fsum(v * v)


# ---- the step -----------------------------------------------------------------------------------------------------------------------------------------

def trust_ref(sum_p, sum_g, *, clip, eta, wd, eps, adapt=True) -> float:
    """lars_trust in lars.hip: float64 from the two stored sums and the fp32 scalars, narrowed once to float32"""
    if not adapt:
        return 1.0
    wn = np.sqrt(np.float64(sum_p))
    gn = np.float64(_f32(clip)) * np.sqrt(np.float64(sum_g))
    if not (wn > 0.0 and gn > 0.0):
        return 1.0
    den = (gn + np.float64(_f32(wd)) * wn) + np.float64(_f32(eps))
    return float(np.float32(np.float64(_f32(eta)) * wn / den))


def lars_constants(lr, momentum, wd):
    return dict(lr=_f32(lr), momentum=_f32(momentum), wd=_f32(wd))


def lars_ref(p, g, buf, *, lr, momentum, wd, eta, eps, first_step, norm_sq, max_norm, norms, adapt=True, clip=None):
    """fp64 (p', buf') of one lars1 call of lars.hip on fp32 tensors and a bound for each: (value, |error|) carried through the recurrence as in
    sgd_ref.sgd_ref, the trust ratio entering as trust_ref's fp32 value with TRUST_ULPS of its spacing as error.  ``norms``: (sum p^2, sum g^2) as
    handed to the entry (None with adapt False).  `buf` is not read when first_step or momentum == 0; buf' and its bound are None when momentum == 0.
    -> (p', buf'), (bound_p, bound_buf), fp64 on the inputs' device."""
    k = lars_constants(lr, momentum, wd)
    clip = clip_ref(norm_sq, max_norm) if clip is None else float(clip)
    trust = trust_ref(norms[0], norms[1], clip=clip, eta=eta, wd=wd, eps=eps, adapt=adapt) if adapt else 1.0
    e_trust = TRUST_ULPS * float(np.spacing(np.float32(trust))) if trust != 1.0 else 0.0
    P, G = p.double(), g.double()
    zero = torch.zeros_like(P)
    g2 = G * clip
    e_g2 = _rnd(g2, zero)
    if k["wd"] != 0.0:
        t = k["wd"] * P
        e_t = _rnd(t, zero)
        g2, e_g1 = g2 + t, e_g2
        e_g2 = _rnd(g2, e_g1 + e_t)
    g3 = g2 * trust
    e_g3 = _rnd(g3, trust * e_g2 + g2.abs() * e_trust + e_g2 * e_trust)
    b2 = e_b = None
    s_in, e_in = g3, e_g3
    if k["momentum"] != 0.0:
        if first_step:
            b2, e_b = g3, e_g3
        else:
            a = k["momentum"] * buf.double()
            e_a = _rnd(a, zero)
            b2 = a + g3
            e_b = _rnd(b2, e_a + e_g3)
        s_in, e_in = b2, e_b
    s = k["lr"] * s_in
    e_s = _rnd(s, k["lr"] * e_in)
    p2 = P - s
    e_p = _rnd(p2, e_s)
    return (p2, b2), (e_p + DENORM, e_b + DENORM if e_b is not None else None)


def lars1_fp32(p, g, buf, *, lr, momentum, wd, eta, eps, first_step, norm_sq, max_norm, norms, adapt=True):
    """the recurrence in torch fp32, one rounding per operation (no fused multiply-add) -> (p', buf' or None) fp32"""
    k = lars_constants(lr, momentum, wd)
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    clip = clip_ref(norm_sq, max_norm)
    g = g * f(clip)
    if k["wd"] != 0.0:
        g = g + f(k["wd"]) * p
    if adapt:
        g = g * f(trust_ref(norms[0], norms[1], clip=clip, eta=eta, wd=wd, eps=eps))
    if k["momentum"] != 0.0:
        buf = g.clone() if first_step else f(k["momentum"]) * buf + g
        g = buf
    else:
        buf = None
    return p - f(k["lr"]) * g, buf


def bf16_bits(x):
    """x fp32 -> the bits of bf16(x), round to nearest even, as int16 (what the kernels store into a shadow)"""
    return x.to(torch.bfloat16).view(torch.int16)


# the hyper-parameter combinations both test files run: momentum 0 / 0.9, weight decay 0 / 5e-4, adapt on / off
HYPERS = [dict(momentum=m, wd=wd, adapt=ad) for m in (0.0, 0.9) for wd in (0.0, 5e-4) for ad in (True, False)]


def hyper_id(h):
    return f"m{h['momentum']}-wd{h['wd']}-{'adapt' if h['adapt'] else 'plain'}"
