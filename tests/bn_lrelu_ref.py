"""fp64 references of yolo_batchnorm_train_fwd_lrelu / yolo_batchnorm_bwd_lrelu (bn.hip), on top of launch_ref's BatchNorm references, with bounds
propagated the same way.  What LeakyReLU adds to them: y = t for t > 0, slope * t otherwise -- the multiply is one more fp32 rounding, and
|slope| <= 1 scales the incoming bound.  What the fused pool adds: nothing to the arithmetic (a maximum of stored values is exact), only a selection.

Decisions are made on ROUNDED values by the kernels (the mask on fp32 t, the arg-max on the bf16 y), so a caller that checks a device passes the
decisions the device made -- `mask` = stored bf16 y > 0 and `sel` = first_argmax of the stored bf16 y of an unfused forward launch -- and the references
compute everything else from them.  Without them (the CPU test against stock torch) the references decide on their own fp64 values."""
from types import SimpleNamespace

import torch

import launch_ref as lr
from launch_ref import TINY, U


def windows(x):
    """[N][H][W][C] (H, W even) -> [N][H/2][W/2][4][C], window position 2*dy + dx: scan order"""
    N, H, W, C = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def unwindows(w):
    """inverse of windows"""
    N, Hq, Wq, _, C = w.shape
    return w.reshape(N, Hq, Wq, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Hq, 2 * Wq, C)


def first_argmax(y):
    """window position of the FIRST maximum in scan order (0,0), (0,1), (1,0), (1,1) -- the rule of yolo_maxpool2_bwd_lrelu and of aten:
    y [N][H][W][C] -> int64 [N][H/2][W/2][C]"""
    w = windows(y)
    best = torch.zeros(w.shape[:3] + w.shape[4:], dtype=torch.int64, device=y.device)
    m = w[:, :, :, 0]
    for j in range(1, 4):
        gt = w[:, :, :, j] > m
        best = torch.where(gt, torch.full_like(best, j), best)
        m = torch.where(gt, w[:, :, :, j], m)
    return best


def select(x, sel):
    """x [N][H][W][C] at the window positions sel -> [N][H/2][W/2][C]"""
    return windows(x).gather(3, sel.unsqueeze(3)).squeeze(3)


def scatter(v, sel):
    """v [N][H/2][W/2][C] placed at the window positions sel, zeros elsewhere -> [N][H][W][C]"""
    w = torch.zeros(v.shape[:3] + (4,) + v.shape[3:], dtype=v.dtype, device=v.device)
    return unwindows(w.scatter_(3, sel.unsqueeze(3), v.unsqueeze(3)))


def fwd_ref(z, mean, var, dm, dv, gamma, beta, eps, slope, mask=None, sel=None, pool=False):
    """z fp64 [N][H][W][C]; statistics (mean, var) with the kernel's within (dm, dv), as lr.bn_fwd_ref takes them.
    -> namespace: y, bnd [N][H][W][C] (pool: [N][H/2][W/2][C], the y at the selected position), save, save_bnd [4][C], mask, sel"""
    N, H, W, C = z.shape
    B = lr.bn_fwd_ref(z.reshape(-1, C), mean, var, dm, dv, gamma, beta, eps)          # t = z scale + shift; its save / save_bnd are what we need
    scale, shift = B.save[2], B.save[3]
    inv = B.save[1]
    v = var.clamp_min(0.0)
    dinv = torch.maximum(((v - dv).clamp_min(0.0) + eps).rsqrt() - inv, inv - (v + dv + eps).rsqrt())
    dscale = gamma.double().abs() * dinv
    t = z * scale + shift
    err = (z - mean).abs() * dscale + dm * (scale.abs() + dscale) + U * (z.abs() * scale.abs() + shift.abs() + t.abs())          # as lr.bn_fwd_ref
    if mask is None:
        mask = t > 0
    y = torch.where(mask, t, slope * t)
    err = torch.where(mask, err, abs(slope) * err + U * y.abs())          # one more fp32 rounding; |slope| <= 1 scales the bound
    bnd = (1 + 2.0 ** -8) * 1.01 * err + 2.0 ** -8 * y.abs() + TINY
    R = SimpleNamespace(save=B.save, save_bnd=B.save_bnd, mask=mask, sel=None)
    if pool:
        if sel is None:
            sel = first_argmax(y)
        R.sel = sel
        y, bnd = select(y, sel), select(bnd, sel)
    R.y, R.bnd = y, bnd
    return R


def bwd_ref(dy, z, gamma, save, L, slope, mask, sel=None, frozen=False):
    """dy fp64: [N][H][W][C], or with sel the gradient of the POOLED map [N][H/2][W/2][C]; z fp64 [N][H][W][C]; save the forward's [4][C]
    (mean, invstd, scale, shift); mask bool [N][H][W][C] (t > 0); L pixels of dy per lane (lr.bn_lane_pixels of dy's pixel count: the three
    zeros a pooled lane adds per window are exact).  dy' = dy (mask ? 1 : slope), at the selected position only; then lr.bn_bwd_ref.
    -> namespace: g, dz, bnd [N][H][W][C]; dgamma, dbeta and their bounds [C]"""
    N, H, W, C = z.shape
    mult = torch.where(mask, torch.ones_like(z), torch.full_like(z, slope))
    g = scatter(dy * select(mult, sel), sel) if sel is not None else dy * mult
    eg = torch.where(mask, torch.zeros_like(g), U * g.abs())          # the fp32 rounding of dy * slope
    P = N * H * W
    zz, gg = z.reshape(P, C), g.reshape(P, C)
    B = lr.bn_bwd_ref(gg, zz, gamma, save, L, None, frozen)
    xh = (zz - save[0].double()) * save[1].double()
    eg = eg.reshape(P, C)
    e1, e2 = 1.01 * eg.sum(0), 1.01 * (eg * xh.abs()).sum(0)
    c0 = (gamma.double() * save[1].double()).abs()
    extra = c0 * (eg if frozen else eg + e1 / P + xh.abs() * e2 / P)
    R = SimpleNamespace(g=g, dz=B.dz.reshape(N, H, W, C), bnd=(B.bnd + (1 + 2.0 ** -8) * 1.01 * extra).reshape(N, H, W, C))
    R.dbeta, R.dbeta_bnd = B.dbeta, B.dbeta_bnd + e1
    R.dgamma, R.dgamma_bnd = B.dgamma, B.dgamma_bnd + e2
    return R
