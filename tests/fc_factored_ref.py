"""fp64 reference of the factored Linear gradient (csrc/fc_factored.hip, include/yolo_hip.h: yolo_fc_factors): G = scale * dy^T x from the
two bf16 batch factors, the absolute-value product the element bounds are stated in, and the Gram matrices behind |G|^2.

Same conventions as launch_ref.py / elementwise_ref.py: plain torch, tensors in, fp64 out on the device of the inputs.  ``scale`` is the fp32
value the C entries receive (``f32(scale)``); bf16 -> fp64 is exact.
"""

from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32
RND = 1.01 * U            # the factor launch_ref.py puts on roundoff terms
BF = torch.bfloat16

SHAPES = [(1, 136, 200), (5, 136, 200), (64, 136, 200), (80, 136, 200), (128, 264, 392)]       # (rows, O, I)
SCALES = [1.0, 0.5, 1.0 / 3.0]


def f32(x) -> float:
    return float(np.float32(x))


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def factors(rows, O, I, seed, device="cpu", ld_dy=None, ld_x=None, pad_value=float("nan")):
    """dy bf16 [rows][ld_dy] and x bf16 [rows][ld_x] of N(0, 1) values; the padding columns O .. ld_dy - 1 and I .. ld_x - 1 hold ``pad_value``
    (a NaN: nothing may read them into a result).  ld_dy defaults to round_up(O, 32) as the plan lays the gradient rows out."""
    gen = torch.Generator().manual_seed(seed)
    ld_dy = round_up(O, 32) if ld_dy is None else ld_dy
    ld_x = I if ld_x is None else ld_x
    dy = torch.full((rows, ld_dy), pad_value, dtype=torch.float32)
    x = torch.full((rows, ld_x), pad_value, dtype=torch.float32)
    dy[:, :O] = torch.randn((rows, O), generator=gen)
    x[:, :I] = torch.randn((rows, I), generator=gen)
    return dy.to(BF).to(device), x.to(BF).to(device)


def grad_ref(dy, x, O, I, scale):
    """-> (G64, Gabs): G64 = scale * dy^T x and Gabs = |dy|^T |x|, fp64 [O][I]"""
    d, xx = dy[:, :O].double(), x[:, :I].double()
    return f32(scale) * (d.t() @ xx), d.abs().t() @ xx.abs()


def scale_is_pow2(scale) -> bool:
    m, _ = math.frexp(f32(scale))
    return m == 0.5


def grad_bound(Gabs, rows, scale):
    """Products of bf16 values are exact in fp32, so only the fp32 additions round: no term passes more than rows - 1 of them, plus one
    rounding for a scale that is not a power of two:  |G - G64| <= (rows - 1 + [scale not in 2^Z]) * 1.01 u * scale * Gabs"""
    n = rows - 1 + (0 if scale_is_pow2(scale) else 1)
    return n * RND * f32(scale) * Gabs


def gram_ref(dy, x, O, I):
    """-> (A, B, Aabs, Babs): the rows x rows Gram matrices A = dy dy^T (over the O columns), B = x x^T (over the I columns) and the same of the
    absolute values, fp64"""
    d, xx = dy[:, :O].double(), x[:, :I].double()
    return d @ d.t(), xx @ xx.t(), d.abs() @ d.abs().t(), xx.abs() @ xx.abs().t()


def sumsq_ref(dy, x, O, I, scale, chain):
    """-> (sum G64^2 by the Gram identity, bound): |G|^2 = scale^2 sum_{n,m} A[n][m] B[n][m].  With ``chain`` the longest fp32 accumulation chain of
    a Gram entry (YOLO_FC_GRAM_CHAIN), every computed Gram entry errs by at most chain * 1.01 u times its absolute-value entry, so
        |got - ref| <= scale^2 (2.02 chain u + 1e-12) sum Aabs o Babs
    (the 1e-12 covers the fp64 sums of the chunk partials, the products and the slots)"""
    A, B, Aa, Ba = gram_ref(dy, x, O, I)
    s2 = f32(scale) ** 2
    return s2 * float((A * B).sum()), s2 * (2.02 * chain * U + 1e-12) * float((Aa * Ba).sum())


def grad_fp32_sequential(dy, x, O, I, scale):
    """a restatement in torch fp32, the rows added one after the other (one rounding per addition), then one multiply by scale"""
    d, xx = dy[:, :O].float(), x[:, :I].float()
    g = torch.zeros((O, I), dtype=torch.float32, device=dy.device)
    for n in range(d.shape[0]):
        g = g + d[n][:, None] * xx[n][None, :]
    return g * torch.tensor(f32(scale), dtype=torch.float32, device=dy.device)


def sumsq_fp32_chunked(dy, x, O, I, scale, chain):
    """a restatement of the Gram form: every Gram entry from fp32 chunk sums of ``chain`` columns (torch's fp32 matmul), the chunks added in fp64"""
    def gram(m, cols):
        acc = torch.zeros((m.shape[0], m.shape[0]), dtype=torch.float64, device=m.device)
        for c0 in range(0, cols, chain):
            blk = m[:, c0: min(cols, c0 + chain)].float()
            acc += (blk @ blk.t()).double()
        return acc
    return f32(scale) ** 2 * float((gram(dy, O) * gram(x, I)).sum())
