"""Executor of conv -> BatchNorm -> LeakyReLU(0.1) [-> MaxPool2d(2,2)] chains: the BatchNorm variant of the YOLOv1 network in training
(``YOLOv1Backbone(batch_norm=True)``; Darknet's yolov1.cfg has batch_normalize=1 on every convolution).  One autograd node for the whole chain
(``BNTrainFunction``), modelled on the trainable ResNet trunk: every unit keeps its conv output z, the activation mask and the pool's arg-max are
recomputed from z in the backward pass (bn.hip: yolo_batchnorm_train_fwd_lrelu / yolo_batchnorm_bwd_lrelu).  Inference does not come here: in eval()
without gradients the BatchNorm layers fold into the convolutions and the ordinary ``executor.Plan`` runs (models.py)."""

from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _hip
from ._hip import EPI_NONE, PoolDesc, check, ptr
from .autograd import BNTrainFunction
from .config import CONFIG as CFG
from .conv_bn import Unit, _ConvBNBase, _TrainBackward
from .plans import igemm_call
from .runtime import RT, _igemm, _timed, f32, is_stem, require_pool2

SLOPE = 0.1
NO_INPUT_GRAD = "the BatchNorm chain (BNPlan) computes no gradient with respect to its input image: detach the input"
BN_LRELU_NOT_DETERMINISTIC = ("EngineConfig.DETERMINISTIC does not cover a BatchNorm backbone in training mode: its batch statistics and the sums of its "
                              "backward pass are fp64 atomics (bn.hip).  Train without --deterministic, or without --batch-norm")


class BNPlan(_ConvBNBase):
    """``from_modules`` takes a flat list of ``[Conv2d(bias=False), BatchNorm2d, LeakyReLU(0.1)] [MaxPool2d(2, 2)]`` groups.
    ``forward_train(x, frozen)`` -> (NCHW fp32 output, saved); ``backward_train(saved, gout)`` -> {parameter: fp32 gradient}.
    Per unit, forward: conv (no epilogue) into z, kept -> yolo_batchnorm_train_fwd_lrelu -> y, or the pooled y where the map is even and
    ``EngineConfig.BN_POOL_FUSED`` (otherwise y, then yolo_maxpool2_fwd).  Backward: [yolo_maxpool2_bwd_lrelu with slope 1 ->]
    yolo_batchnorm_bwd_lrelu -> dz -> yolo_wgrad on the side stream + the data-gradient yolo_igemm, as ResNetPlan.backward_train does it.
    The statistics always come from the separate pass (stats_ready = 0): ``BN_STATS_IN_CONV`` is the ResNet trunk's switch and is not read here.
    frozen: eval() mode with gradients -- running statistics, nothing updated, no batch terms in the backward pass."""

    WHAT = "a BatchNorm chain"
    NO_INPUT_GRAD = NO_INPUT_GRAD

    def __init__(self, units: list):
        super().__init__()
        self.units = units           # [(conv, bn, pool, first)]

    @staticmethod
    def from_modules(mods) -> "BNPlan":
        mods, units, i = list(mods), [], 0
        while i < len(mods):
            conv, bn, act = (mods[i + j] if i + j < len(mods) else None for j in range(3))
            if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d) and isinstance(act, nn.LeakyReLU)):
                raise ValueError(f"BNPlan: expected Conv2d, BatchNorm2d, LeakyReLU at module {i}, got {conv}, {bn}, {act}")
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            if conv.kernel_size[0] != conv.kernel_size[1] or conv.groups != 1 or conv.dilation != (1, 1) or conv.bias is not None:
                raise ValueError(f"BNPlan: unsupported conv {conv} (square, dense, bias=False: BatchNorm's shift is the bias)")
            if abs(act.negative_slope - SLOPE) > 1e-12:
                raise ValueError("BNPlan: only LeakyReLU(0.1)")
            if bn.num_features != conv.out_channels or bn.weight is None or not bn.track_running_stats or bn.num_features > 2048:
                raise ValueError(f"BNPlan: {bn} must be affine with running statistics, at most 2048 channels, behind a conv of as many output channels")
            first = is_stem(conv)
            if first and (i != 0 or conv.out_channels != 64):
                raise ValueError("BNPlan: the 7x7/s2 stem has 64 output channels and comes first")
            if not first and (not ((k == 3 and p == 1) or (k == 1 and p == 0)) or s not in (1, 2) or conv.in_channels % 64 or conv.out_channels % 64):
                raise ValueError(f"BNPlan: unsupported conv geometry {conv} (1x1, 3x3/p1, stride 1 or 2, channels in multiples of 64)")
            i += 3
            pool = i < len(mods) and isinstance(mods[i], nn.MaxPool2d)
            if pool:
                require_pool2(mods[i], "BNPlan: ")
                i += 1
            units.append((conv, bn, pool, first))
        if not units:
            raise ValueError("BNPlan: no units")
        return BNPlan(units)

    @property
    def params(self) -> list:
        """conv weight, BatchNorm weight and bias of every unit, in module order"""
        return [p for (conv, bn, _, _) in self.units for p in (conv.weight, bn.weight, bn.bias)]

    # ------------------------------------------------------------------ forward
    @_hip.device_guard
    def forward_train(self, x: torch.Tensor, frozen: bool = False):
        """Returns (out, saved).  One forward may be in flight per plan (the buffers are reused step to step)."""
        _hip.require_cuda(x)
        L_, st = RT.lib(), RT.stream()
        packable = [(i, conv, bn, first) for i, (conv, bn, _, first) in enumerate(self.units)]
        self._train_pk = self._pack(packable, self._train_pk, dgrad=True)
        pk = self._train_pk[1]
        N, dev = x.shape[0], x.device
        acc, ss = self._scratch(dev)
        stat = self._stat_arena(packable, dev)
        if self.units[0][3]:
            cur = self._stem_input(x, st)
        else:
            C0 = self.units[0][0].in_channels
            if x.shape[1] != C0:
                raise RuntimeError(f"BNPlan: the input has {x.shape[1]} channels, the first conv expects {C0}")
            cur = self._act("in", N, x.shape[2], x.shape[3], C0, 1, dev)
            check(L_.yolo_nchw_f32_to_nhwc_bf16(ptr(f32(x)), N, C0, x.shape[2], x.shape[3], cur.p, C0, 1, 1, st), "nchw->nhwc")
        recs = []
        for i, (conv, bn, pool, first) in enumerate(self.units):
            wf, wd, _, _ = pk[i]
            C = conv.out_channels
            k, s, p, Ho, Wo = self._geom(cur, conv)
            z = self._act((i, "z"), N, Ho, Wo, C, 1, dev)
            if first:
                with _timed(str(i), "igemm", 2.0 * N * Ho * Wo * 64 * 147):
                    _igemm(L_, self._stem_desc(cur, z, EPI_NONE, 1.0), cur.p, ptr(wf), None, None, z.p, st, "igemm stem")
            else:
                d = self._desc(cur, p, s, k, z, EPI_NONE, 1.0)
                with _timed(str(i), "igemm", 2.0 * N * Ho * Wo * C * conv.in_channels * k * k):
                    igemm_call(d, cur.p, ptr(wf), None, None, z.p, st, f"igemm {i}")
            stats = stat(C)
            fused = pool and CFG.BN_POOL_FUSED and Ho % 2 == 0 and Wo % 2 == 0
            y = self._act((i, "y"), N, Ho // 2 if fused else Ho, Wo // 2 if fused else Wo, C, 1, dev)
            mom = 0.1 if bn.momentum is None else bn.momentum
            check(L_.yolo_batchnorm_train_fwd_lrelu(z.p, N, Ho, Wo, C, z.halo, ptr(bn.weight.detach()), ptr(bn.bias.detach()), float(bn.eps), float(mom),
                                                         ptr(bn.running_mean), ptr(bn.running_var), SLOPE, 1 if fused else 0, ptr(acc), ptr(ss), y.p, y.halo,
                                                         ptr(stats), 2 if frozen else 0, st), f"batchnorm_train_fwd_lrelu {i}")
            if not frozen:
                bn.num_batches_tracked += 1
            out = y
            if pool and not fused:
                out = self._act((i, "yp"), N, Ho // 2, Wo // 2, C, 1, dev)
                pd = PoolDesc(N, Ho, Wo, C, y.halo, out.halo)
                check(L_.yolo_maxpool2_fwd(ctypes.byref(pd), y.p, out.p, st), f"maxpool2_fwd {i}")
            recs.append(Unit(i, conv, bn, cur, z, y, stats, wd, k, s, p, first, pool=pool, fused=fused, out=out))
            cur = out
        res = self._to_nchw(cur, dev, st)
        self._train_gen += 1
        return res, {"N": N, "dev": dev, "units": recs, "out": cur, "gen": self._train_gen, "frozen": frozen}

    # ------------------------------------------------------------------ backward
    def backward_train(self, saved, gout: torch.Tensor) -> dict:
        """gradients of every parameter of the chain for the forward recorded in `saved`: {parameter: fp32 gradient}."""
        L_, st = RT.lib(), RT.stream()
        recs = saved["units"]
        B = _TrainBackward(self, saved, [u.conv for u in recs if not u.first], st)
        N, dev = B.N, B.dev
        g = B.seed(saved["out"], gout)
        for u in reversed(recs):
            i, z, y, bn = u.tag, u.z, u.y, u.bn
            C = z.C
            B.note(i, "gout", g)
            if u.pool and not u.fused:
                gy = self._act((i, "gy"), N, z.H, z.W, C, 1, dev)          # an odd last row / column is never written: it stays zero
                pd = PoolDesc(N, z.H, z.W, C, y.halo, g.halo)
                check(L_.yolo_maxpool2_bwd_lrelu(ctypes.byref(pd), y.p, g.p, 1.0, gy.p, st), f"maxpool2_bwd {i}")
                g = gy
            dz, strides, dg, db = B.bn_outputs(u)
            check(L_.yolo_batchnorm_bwd_lrelu(g.p, g.halo, z.p, z.halo, N, z.H, z.W, C, ptr(bn.weight.detach()), ptr(u.stats), SLOPE, 1 if u.fused else 0,
                                                   dz.p, *strides, 1 if saved["frozen"] else 0, ptr(dg), ptr(db), ptr(B.acc), ptr(self._coef), st),
                  f"batchnorm_bwd_lrelu {i}")
            if u.first:
                B.flush()
                B.stem_wgrad(u, dz)
                break
            B.wgrad(u, dz)
            if i > 0:
                g = B.dgrad(u, dz, None)
                B.note(i, "gx", g)
            B.flush(24)
        B.flush()
        return B.finish()


def run_bn_plan(plan: BNPlan, x, training: bool) -> torch.Tensor:
    """the chain with gradients: batch statistics in training mode, running statistics (frozen) in eval() mode.  x: NCHW fp32 on the device, or a
    ``yolo.augment.U8Batch`` (its fp32 tensor is taken)"""
    if not isinstance(x, torch.Tensor):
        x = x.to_tensor()
    if training and CFG.DETERMINISTIC:
        raise NotImplementedError(BN_LRELU_NOT_DETERMINISTIC)
    if x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(NO_INPUT_GRAD)
    return BNTrainFunction.apply(plan, not training, x, *plan.params)
