#!/usr/bin/env python3
"""micro-benchmark: yolo_batchnorm_train_fwd_lrelu and yolo_batchnorm_bwd_lrelu at the 24 layer shapes of the BatchNorm YOLOv1 network at batch 64 /
448 x 448 -- with the pool fused (pool2 = 1) and unfused (pool2 = 0 + yolo_maxpool2_fwd / yolo_maxpool2_bwd_lrelu) on the four pooled layers, and the
ReLU entries (yolo_batchnorm_train_fwd / yolo_batchnorm_bwd with relu_from_z) at the same shapes for comparison: ms (median of --reps samples of 10
launches, configurations alternating, min - max behind it) and the effective HBM rate from the bytes the passes must move, in passes over the
un-pooled bf16 map: forward 3 (statistics 1, apply 2), + 1.25 for a separate pool, 2.25 fused; backward 5 (reduce 2, apply 3), + 2.25 for a
separate pool backward, 3.5 fused.

    python tools/time_bn_lrelu.py [--batch 64] [--reps 3]"""
import argparse, ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))
import torch
import torch.nn as nn
from yolo import YOLOv1Backbone
from yolo._hip import BN_ACC_REPLICAS, PoolDesc, check, lib, ptr, stream
from yolo.engine import Act

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
N, dev, L = a.batch, torch.device("cuda"), lib()

# (H, C, pooled) of every conv output, from the module list itself
layers, hw, mods = [], 448, list(YOLOv1Backbone(batch_norm=True).features)
for i, m in enumerate(mods):
    if isinstance(m, nn.Conv2d):
        hw = (hw + 2 * m.padding[0] - m.kernel_size[0]) // m.stride[0] + 1
        layers.append((hw, m.out_channels, isinstance(mods[i + 3] if i + 3 < len(mods) else None, nn.MaxPool2d)))
    elif isinstance(m, nn.MaxPool2d):
        hw //= 2
assert len(layers) == 24
shapes = sorted(set(layers), key=lambda s: -s[0] * s[0] * s[1])


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 10


totals = {}
for H, C, pool in shapes:
    count = layers.count((H, C, pool))
    z, y, dy, dz, gy = (Act(N, H, H, C, 1, dev) for _ in range(5))
    yp, dp = Act(N, H // 2, H // 2, C, 1, dev), Act(N, H // 2, H // 2, C, 1, dev)
    for t in (z, dy, dp):
        t.interior().normal_()
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    acc = torch.zeros(BN_ACC_REPLICAS * 2 * C, dtype=torch.float64, device=dev)
    ss, save, coef = torch.empty(2 * C, device=dev), torch.empty(4 * C, device=dev), torch.empty(3 * C, device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    pd = PoolDesc(N, H, H, C, 1, 1)
    st = (dz.img_stride, dz.row_stride, dz.px_stride, dz.interior_off())

    def fwd(p2, out):
        check(L.yolo_batchnorm_train_fwd_lrelu(z.p, N, H, H, C, 1, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm), ptr(rv), 0.1, p2, ptr(acc), ptr(ss), out.p, 1,
                                               ptr(save), 0, stream()))

    def bwd(p2, g):
        check(L.yolo_batchnorm_bwd_lrelu(g.p, 1, z.p, 1, N, H, H, C, ptr(gamma), ptr(save), 0.1, p2, dz.p, *st, 0, ptr(dg), ptr(db), ptr(acc), ptr(coef), stream()))

    def fwd_unfused():
        fwd(0, y)
        check(L.yolo_maxpool2_fwd(ctypes.byref(pd), y.p, yp.p, stream()))

    def bwd_unfused():
        check(L.yolo_maxpool2_bwd_lrelu(ctypes.byref(pd), y.p, dp.p, 1.0, gy.p, stream()))
        bwd(0, gy)

    def fwd_relu():
        check(L.yolo_batchnorm_train_fwd(z.p, N, H, H, C, 1, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm), ptr(rv), None, 0, 1, ptr(acc), ptr(ss), y.p, 1, ptr(save), 0,
                                         stream()))

    def bwd_relu():
        check(L.yolo_batchnorm_bwd(dy.p, 1, None, 1, z.p, 1, N, H, H, C, ptr(gamma), ptr(save), dz.p, *st, 0, 1, ptr(dg), ptr(db), ptr(acc), ptr(coef), stream()))

    el = N * H * H * C * 2
    cfgs = [("fwd lrelu", lambda: fwd(0, y), 3.0), ("fwd relu ", fwd_relu, 3.0), ("bwd lrelu", lambda: bwd(0, dy), 5.0), ("bwd relu ", bwd_relu, 5.0)]
    if pool:
        cfgs += [("fwd lrelu + pool, unfused", fwd_unfused, 4.25), ("fwd lrelu + pool, fused  ", lambda: fwd(1, yp), 2.25),
                 ("bwd pool + lrelu, unfused", bwd_unfused, 7.25), ("bwd pool + lrelu, fused  ", lambda: bwd(1, dp), 3.5)]
    fwd(0, y)          # save / y hold a real forward for the backward launches
    samples = {name: [] for name, _, _ in cfgs}
    for _ in range(a.reps):          # alternating: every configuration once per round
        for name, fn, _ in cfgs:
            samples[name].append(timed(fn))
    print(f"{H:4d} x {H:4d} x {C:5d}  ({count} layer{'s' if count > 1 else ''}{', pooled' if pool else ''}; {el / 1e6:.0f} MB per pass)")
    for name, _, passes in cfgs:
        ms = statistics.median(samples[name])
        print(f"    {name:27s} {ms:7.3f} ms ({min(samples[name]):.3f} - {max(samples[name]):.3f})  {passes * el / ms / 1e9:5.2f} TB/s effective ({passes} passes)")
        totals[name.strip()] = totals.get(name.strip(), 0.0) + count * ms
    del z, y, dy, dz, gy, yp, dp
pooled_un = totals.get("fwd lrelu + pool, unfused", 0) + totals.get("bwd pool + lrelu, unfused", 0)
pooled_fu = totals.get("fwd lrelu + pool, fused", 0) + totals.get("bwd pool + lrelu, fused", 0)
print("per training step, all 24 layers (ms):", {k: round(v, 3) for k, v in totals.items()})
print(f"the four pooled layers, forward + backward: unfused {pooled_un:.3f} ms, fused {pooled_fu:.3f} ms")
