"""Reference of the gradient-accumulation entries of csrc/accum.hip (yolo_grad_accum, yolo_grad_accum_multi) and of yolo.optim.GradAccumulator:

    dst = alpha * x + y        (y given)
    dst = alpha * x            (no y)                alpha = fp32(1 / K)

in fp64 from the fp32 inputs, with a bound for what the kernels store, fmaf(alpha, x, y) or fl(alpha * x).  alpha and x are fp32 values, so
their product has at most 48 significant bits and is exact in fp64 -- and exact inside the fused multiply-add, which rounds once, at the end.
With u = 2^-24 and ref the fp64 value:

    stored = ref (1 + b)           |b| <= u          (the one rounding of the fma, or of the plain product)
    |stored - ref| <= u |ref|  <=  1.01 u |ref|

(the 1.01 is launch_ref.py's factor on roundoff terms; the fp64 reference's own rounding, 2^-53 relative, disappears in it).  Valid while the
result stays in the normal range, which the test inputs do; an exact cancellation gives ref = 0, bound 0, and the fma gives 0 exactly.

The chain of a K-step group, fed back in fp64:  ref_1 = alpha g_1,  ref_k = alpha g_k + ref_{k-1}.  The stored fp32 chain a_k = fmaf(alpha, g_k,
a_{k-1}) starts each link from a_{k-1} = ref_{k-1} + e with |e| <= c_{k-1}: the exact value of the link is ref_k + e (the error passes through
the addition unchanged) and its rounding is at most u (|ref_k| + c_{k-1}), so

    c_1 = 1.01 u |ref_1|,      c_k = c_{k-1} + 1.01 u (|ref_k| + c_{k-1})

Which of the three buffers a link is stored to (the accumulator, or -- the fold -- the gradient memory) does not enter the arithmetic.

Same conventions as ema_ref.py: tensors in, ``(ref, bnd)`` fp64 out for launch_ref.check_values, on the device of the inputs.
"""

from __future__ import annotations

import torch

from elementwise_ref import RND, _f32


def accum_alpha(K: int) -> float:
    """the fp32 weight the launches work with, as a Python float: (float)(1.0 / K), the quotient formed in double"""
    return _f32(1.0 / K)


def accum_ref(x, y, alpha: float):
    """fp64 alpha * x + y (y None: alpha * x) of the fp32 tensors with the fp32 weight alpha (a Python float that is an fp32 value) -> (ref, bnd)"""
    assert _f32(alpha) == alpha, "alpha must be the fp32-rounded weight"
    ref = alpha * x.double()
    if y is not None:
        ref = ref + y.double()
    return ref, RND * ref.abs()


def accum_chain_ref(micro_grads, K: int):
    """the K-step recurrence over the fp32 micro-gradients (K of them), fed back in fp64 -> (ref, bnd) after the last link"""
    assert len(micro_grads) == K >= 1
    alpha = accum_alpha(K)
    ref = alpha * micro_grads[0].double()
    c = RND * ref.abs()
    for g in micro_grads[1:]:
        ref = alpha * g.double() + ref
        c = c + RND * (ref.abs() + c)
    return ref, c


def accum_ranks_ref(chains):
    """the mean over the ranks' chains [(ref, bnd)], as a SUM all-reduce followed by one multiplication with 1 / world stores it: the errors
    carried in add up, the cross-rank additions are charged one rounding of the sum (two ranks: one addition), the multiplication one more
    -> (ref, bnd)"""
    world = len(chains)
    tot = sum(r for r, _ in chains)
    c = sum(b for _, b in chains)
    c = c + (world - 1) * RND * (tot.abs() + c)
    ref = tot / world
    return ref, c / world + RND * (ref.abs() + c / world)
