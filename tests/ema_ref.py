"""Reference of the EMA entries of csrc/ema.hip (yolo_ema_update, yolo_ema_update_multi, yolo_ema_update_multi_bg) and of yolo.optim.ModelEMA:

    e' = e + w * (p - e)                w = fp32(1 - decay)

in fp64 from the fp32 inputs, with a bound for what the kernels store, e_hat = fmaf(w, fl(p - e), e).  With u = 2^-24, d = p - e:

    fl(p - e) = d (1 + a)                                  |a| <= u      (one rounding of the difference)
    e_hat     = (e + w d (1 + a)) (1 + b)                  |b| <= u      (one rounding of the fused multiply-add; w * fl(d) is not rounded)
              = e' + w d a + (e' + w d a) b
    |e_hat - e'| <= u w |d| + u |e'| + u^2 w |d|  <=  1.01 u (w |p - e| + |e'|)

(the u^2 term is 6e-8 of the first and disappears in the 1.01).  Valid while fl(p - e) and the result stay in the normal range -- the test inputs
do.  An unfused w * fl(d) + e, which torch.lerp may compute on a CPU, rounds the product as well: u w |d| (1 + u) more, so twice the first term;
``ema_ref(..., fused=False)`` charges it.  w = 0 gives e' = e and the kernels fmaf(0, d, e) = e exactly (the bound is then one rounding of e, loose
but never wrong); w = 1 gives e' = p with the two roundings above.

Same conventions as elementwise_ref.py / sgd_ref.py: tensors in, ``(ref, bnd)`` fp64 out for launch_ref.check_values, on the device of the inputs.
"""

from __future__ import annotations

import math

import torch

from elementwise_ref import RND, _f32


def ema_weight(decay: float, updates: int | None = None, tau: float = 0.0) -> float:
    """the fp32 weight the launches work with, as a Python float: (float)(1.0 - d) formed in double, d = decay * (1 - exp(-updates / tau)) for tau > 0"""
    d = decay * (1.0 - math.exp(-updates / tau)) if tau > 0 else decay
    return _f32(1.0 - d)


def ema_ref(e, p, w: float, fused: bool = True):
    """fp64 e' of one update of the fp32 tensors e, p with the fp32 weight w (a Python float that is an fp32 value) and its bound -> (ref, bnd)"""
    assert _f32(w) == w, "w must be the fp32-rounded weight"
    E, P = e.double(), p.double()
    d = P - E
    ref = E + w * d
    bnd = RND * ((w if fused else 2.0 * w) * d.abs() + ref.abs())
    return ref, bnd


def ema_chain_ref(e0, snapshots, weights):
    """the recurrence over several updates, fed back in fp64: e_k = e_{k-1} + w_k (p_k - e_{k-1}) from e0 (fp32) over the fp32 snapshots p_k.
    The stored fp32 chain differs from it by its own roundings and by the error it carried in: an error c in e_{k-1} arrives as (1 - w_k) c (plus
    its share of the difference's rounding, u w c, inside the 1.01), so
        c_k = (1 - w_k) c_{k-1} + 1.01 u (w_k (|p_k - e_{k-1}| + c_{k-1}) + |e_k| + c_{k-1})
    -> (ref, bnd) after the last update"""
    ref = e0.double()
    c = torch.zeros_like(ref)
    for p, w in zip(snapshots, weights):
        assert _f32(w) == w
        d = p.double() - ref
        nxt = ref + w * d
        c = (1.0 - w) * c + RND * (w * (d.abs() + c) + nxt.abs() + c)
        ref = nxt
    return ref, c
