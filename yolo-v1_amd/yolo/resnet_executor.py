"""Executor of the ResNet-50 trunk (``yolo.resnet.resnet50_trunk``; reference src/yolo/models.py:131-176) on the same kernels: inference with
BatchNorm folded, the frozen trunk in training mode (batch statistics), and the trainable trunk's forward / backward."""

from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _hip
from ._hip import EPI_BIAS, EPI_BIAS_LRELU, EPI_NONE, PoolDesc, check, ptr
from .config import CONFIG as CFG
from .conv_bn import Unit, _ConvBNBase, _TrainBackward
from .plans import igemm_call
from .runtime import RT, Act, _igemm, _timed, desc_aux, stem_tiles_ok


# ====================================================================================================
# ResNet-50 trunk: inference (BatchNorm folded into the conv that precedes it), batch statistics, training
# ====================================================================================================
class ResNetPlan(_ConvBNBase):
    """Inference executor for ``yolo.resnet.resnet50_trunk`` on the same kernels: every conv+BN(+ReLU) is
    one yolo_igemm (BN folded into the bf16 weights and an fp32 bias at pack time), the residual add + ReLU
    of a bottleneck is the epilogue of its last 1x1 conv (YOLO_EPI_BIAS_ADD_LRELU with slope 0), the stem's
    MaxPool2d(3,2,1) is yolo_maxpool3s2_fwd.  ``forward_batch_stats`` runs the same trunk with BatchNorm in training mode
    (batch statistics: conv with the raw weights, then yolo_batchnorm_train_fwd) for the FROZEN backbone of a training run;
    ``forward_train`` / ``backward_train`` are the trainable trunk of the reference's default run (src/train.py:144)."""

    WHAT = "a ResNet trunk"

    def __init__(self, trunk: nn.Sequential):
        super().__init__()
        self.trunk = trunk
        self._packed = None          # (versions, operands) of the folded weights: inference
        self._raw = None             # .. of the raw weights, forward only: forward_batch_stats (forward_train: _train_pk)
        self._units = [("stem", trunk[0], trunk[1], True)]          # (tag, conv, bn, first) in the order the packers take them
        for li in range(4, 8):
            for bi, blk in enumerate(trunk[li]):
                self._units += [((li, bi, 1), blk.conv1, blk.bn1, False), ((li, bi, 2), blk.conv2, blk.bn2, False), ((li, bi, 3), blk.conv3, blk.bn3, False)]
                if blk.downsample is not None:
                    self._units.append(((li, bi, "d"), blk.downsample[0], blk.downsample[1], False))

    def _walk(self, cur: Act, step, act=lambda r: r):
        """the bottlenecks behind the stem's pool: step(tag, input, relu, residual) runs one unit, act(its result) is the unit's output
        -> (the trunk's output, [(li, bi, result of conv1, conv2, conv3, downsample or None)])"""
        blocks = []
        for li in range(4, 8):
            for bi, blk in enumerate(self.trunk[li]):
                rd = None if blk.downsample is None else step((li, bi, "d"), cur, False, None)
                r1 = step((li, bi, 1), cur, True, None)
                r2 = step((li, bi, 2), act(r1), True, None)
                r3 = step((li, bi, 3), act(r2), True, cur if rd is None else act(rd))
                blocks.append((li, bi, r1, r2, r3, rd))
                cur = act(r3)
        return cur, blocks

    def _bn_train(self, a: Act, bn: nn.BatchNorm2d, relu: bool, residual: Act | None, dev, st, out: Act | None = None, save: torch.Tensor | None = None,
                  stats_ready: bool = False, frozen: bool = False):
        """BatchNorm with batch statistics (+ residual, + ReLU) in place on the conv output, running statistics updated.
        frozen: eval() mode with gradients -- normalise with the running statistics as they are, update nothing."""
        C = a.C
        acc, ss = self._scratch(dev)
        if C > 2048 or bn.weight is None or not bn.track_running_stats:
            raise NotImplementedError("batch-statistics BatchNorm: affine layers with running statistics and C <= 2048")
        mom = 0.1 if bn.momentum is None else bn.momentum
        check(RT.lib().yolo_batchnorm_train_fwd(a.p, a.N, a.H, a.W, C, a.halo, ptr(bn.weight.detach()), ptr(bn.bias.detach()), float(bn.eps), float(mom),
                                             ptr(bn.running_mean), ptr(bn.running_var), residual.p if residual is not None else None,
                                             residual.halo if residual is not None else 0, 1 if relu else 0, ptr(acc), ptr(ss),
                                             out.p if out is not None else None, out.halo if out is not None else 0,
                                             ptr(save) if save is not None else None, 2 if frozen else (1 if stats_ready else 0), st), "batchnorm_train_fwd")
        if not frozen:
            bn.num_batches_tracked += 1

    def _unit(self, tag, a_in: Act, packed, N, relu: bool, residual: Act | None, dev, st, stat=None, frozen: bool = False, first: bool = False):
        """conv -> z -> BatchNorm(batch statistics; frozen: running statistics) [+ residual] [ReLU].  Without stat (forward_batch_stats) in place, in the
        one buffer that is returned.  stat (forward_train): the statistics arena's take -- z is kept, the result goes to y, the batch mean / invstd to
        the arena, and the record the backward needs is returned."""
        wf, wd, conv, bn = packed
        k, s, p, Ho, Wo = self._geom(a_in, conv)
        keep = stat is not None
        z = self._act((tag, "z") if keep else tag, N, Ho, Wo, conv.out_channels, 1, dev)
        y = self._act((tag, "y"), N, Ho, Wo, conv.out_channels, 1, dev) if keep else None
        stats = stat(conv.out_channels) if keep else None
        in_conv = CFG.BN_STATS_IN_CONV and not frozen and not first
        if first:
            _igemm(RT.lib(), self._stem_desc(a_in, z, EPI_NONE, 1.0), a_in.p, ptr(wf), None, None, z.p, st, "igemm stem")
        else:
            d = self._desc(a_in, p, s, k, z, EPI_NONE, 1.0)
            d.bn_stats = self._scratch(dev)[0].data_ptr() if in_conv else None      # the conv's epilogue accumulates BatchNorm's sums
            with _timed(str(tag), "igemm", 2.0 * N * Ho * Wo * conv.out_channels * conv.in_channels * k * k):
                igemm_call(d, a_in.p, ptr(wf), None, None, z.p, st, f"igemm {tag}")
        self._bn_train(z, bn, relu, residual, dev, st, out=y, save=stats, stats_ready=in_conv, frozen=frozen)
        return Unit(tag, conv, bn, a_in, z, y, stats, wd, k, s, p, first, relu, residual is not None) if keep else z

    @_hip.device_guard
    def forward_batch_stats(self, x: torch.Tensor) -> torch.Tensor:
        """the trunk with its BatchNorm layers in TRAINING mode (batch statistics, running statistics updated) -- the frozen
        backbone of the reference's default training run (trainer.py:49).  Forward only: no gradient flows into the trunk."""
        _hip.require_cuda(x)
        st = RT.stream()
        self._raw = self._pack(self._units, self._raw)
        pk = self._raw[1]
        N, dev = x.shape[0], x.device

        def unit(tag, a_in, relu, res, first=False):
            return self._unit(tag, a_in, pk[tag], N, relu, res, dev, st, first=first)

        s1 = unit("stem", self._stem_input(x, st), True, None, first=True)
        cur, _ = self._walk(self._stem_pool(s1, dev, st), unit)
        return self._to_nchw(cur, dev, st)

    # ------------------------------------------------------------------ trainable trunk (forward keeps z, backward)
    @_hip.device_guard
    def forward_train(self, x: torch.Tensor, frozen: bool = False):
        """Training-mode forward of a TRAINABLE trunk (the reference's default run, src/train.py:144: ResNetBackbone(freeze=False)):
        as forward_batch_stats, but every unit keeps its conv output z, its activation y and the batch mean / invstd.
        frozen: the trunk is in eval() mode and gradients are wanted -- every BatchNorm normalises with its running statistics
        (aten batch_norm(training=False)) and updates nothing; the backward pass then has no batch terms.
        Returns (out, saved).  One forward may be in flight per plan (the buffers are reused step to step)."""
        _hip.require_cuda(x)
        st = RT.stream()
        self._train_pk = self._pack(self._units, self._train_pk, dgrad=True)
        pk = self._train_pk[1]
        N, dev = x.shape[0], x.device
        stat = self._stat_arena(self._units, dev)

        def unit(tag, a_in, relu, res, first=False):
            return self._unit(tag, a_in, pk[tag], N, relu, res, dev, st, stat, frozen, first)

        stem = unit("stem", self._stem_input(x, st), True, None, first=True)
        cur, blocks = self._walk(self._stem_pool(stem.y, dev, st), unit, lambda u: u.y)
        out = self._to_nchw(cur, dev, st)
        self._train_gen += 1
        return out, {"N": N, "dev": dev, "stem": stem, "blocks": blocks, "out": cur, "gen": self._train_gen, "frozen": frozen}

    def backward_train(self, saved, gout: torch.Tensor) -> dict:
        """gradients of every trunk parameter for the forward recorded in `saved`: {parameter: fp32 gradient}."""
        L_, st = RT.lib(), RT.stream()
        B = _TrainBackward(self, saved, [u.conv for b in saved["blocks"] for u in b[2:] if u is not None], st)
        N, dev = B.N, B.dev
        wgrad, dgrad = B.wgrad, B.dgrad
        frozen = 2 if saved["frozen"] else 0

        def bn_bwd(u: Unit, dy: Act, store_masked: bool) -> Act:
            """dz of unit u from the gradient dy wrt its output"""
            z, y, bn = u.z, u.y, u.bn
            dz, strides, dg, db = B.bn_outputs(u)
            from_z = u.relu and not u.res        # conv -> BN -> ReLU: the mask is recomputed from z, y is not read
            check(L_.yolo_batchnorm_bwd(dy.p, dy.halo, y.p if (u.relu and not from_z) else None, y.halo, z.p, z.halo, N, z.H, z.W, z.C,
                                        ptr(bn.weight.detach()), ptr(u.stats), dz.p, *strides, 1 if store_masked else 0, (1 if from_z else 0) | frozen,
                                        ptr(dg), ptr(db), ptr(B.acc), ptr(self._coef), st), f"batchnorm_bwd {u.tag}")
            return dz

        cur_g = B.seed(saved["out"], gout)
        for (li, bi, u1, u2, u3, ud) in reversed(saved["blocks"]):
            B.note((li, bi), "gout", cur_g)
            dz3 = bn_bwd(u3, cur_g, True)                 # cur_g becomes g * [out > 0]: what the identity branch receives
            wgrad(u3, dz3)
            g_t2 = dgrad(u3, dz3, None)
            dz2 = bn_bwd(u2, g_t2, False)
            wgrad(u2, dz2)
            g_t1 = dgrad(u2, dz2, None)
            dz1 = bn_bwd(u1, g_t1, False)
            wgrad(u1, dz1)
            if ud is not None:
                dzd = bn_bwd(ud, cur_g, False)
                wgrad(ud, dzd)
                g_idn = dgrad(ud, dzd, None)
            else:
                g_idn = cur_g
            cur_g = dgrad(u1, dz1, g_idn)
            B.note((li, bi), "gx", cur_g)
            B.flush(24)
        B.flush()
        # stem: MaxPool2d(3,2,1) backward -> BatchNorm/ReLU backward -> the direct 7x7 weight-gradient kernel
        stem = saved["stem"]
        y0 = stem.y
        g_y0 = self._act(("stem", "gy"), N, y0.H, y0.W, 64, 1, dev)
        pd = PoolDesc(N, y0.H, y0.W, 64, y0.halo, cur_g.halo)
        check(L_.yolo_maxpool3s2_bwd(ctypes.byref(pd), y0.p, cur_g.p, g_y0.p, g_y0.halo, st), "maxpool3s2_bwd")
        B.stem_wgrad(stem, bn_bwd(stem, g_y0, False))
        return B.finish()

    def _stem_pool(self, y: Act, dev, st) -> Act:
        """MaxPool2d(3,2,1) behind the stem"""
        cur = self._act("pool", y.N, (y.H - 1) // 2 + 1, (y.W - 1) // 2 + 1, 64, 1, dev)
        pd = PoolDesc(y.N, y.H, y.W, 64, 1, 1)
        check(RT.lib().yolo_maxpool3s2_fwd(ctypes.byref(pd), y.p, cur.p, st), "maxpool3s2")
        return cur

    def _conv(self, tag, a_in: Act, packed, N, relu: bool, residual: Act | None, dev, st):
        wf, b, conv, _ = packed
        k, s, p, Ho, Wo = self._geom(a_in, conv)
        a_out = self._act(tag, N, Ho, Wo, conv.out_channels, 1, dev)
        d = self._desc(a_in, p, s, k, a_out, EPI_BIAS_LRELU if relu else EPI_BIAS, 0.0 if relu else 1.0)
        aux = None
        if residual is not None:
            d.epilogue = _hip.EPI_BIAS_ADD_LRELU
            desc_aux(d, residual)
            aux = residual.p
        with _timed(str(tag), "igemm", 2.0 * N * Ho * Wo * conv.out_channels * conv.in_channels * k * k):
            igemm_call(d, a_in.p, ptr(wf), ptr(b), aux, a_out.p, st, f"igemm {tag}")
        return a_out

    @_hip.device_guard
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(N,3,H,W) fp32 on the device -> (N,2048,H/32,W/32) fp32."""
        _hip.require_cuda(x)
        st = RT.stream()
        self._packed = self._pack(self._units, self._packed, fold=True)
        pk = self._packed[1]
        N, dev = x.shape[0], x.device
        a = self._stem_input(x, st)
        # stem: 7x7/s2 (+BN+ReLU) through its dedicated kernel or as the row-segment implicit GEMM, then MaxPool2d(3,2,1)
        wf, b, conv, _ = pk["stem"]
        _, _, _, Ho, Wo = self._geom(a, conv)
        s1 = self._act("stem", N, Ho, Wo, 64, 1, dev)
        if CFG.STEM_KERNEL and stem_tiles_ok(64, Ho, Wo):
            with _timed("stem", "stem", 2.0 * N * Ho * Wo * 64 * 147):
                check(RT.lib().yolo_conv_stem7_fwd(a.p, ptr(wf), ptr(b), N, Ho, Wo, a.img_stride, a.row_stride, 0.0, 0, s1.p, s1.img_stride, s1.row_stride,
                                                s1.interior_off(), None, 0, 0, 0, st), "conv_stem7_fwd")
        else:
            with _timed("stem", "igemm", 2.0 * N * Ho * Wo * 64 * 147):
                _igemm(RT.lib(), self._stem_desc(a, s1, EPI_BIAS_LRELU, 0.0), a.p, ptr(wf), ptr(b), None, s1.p, st, "igemm stem")
        cur, _ = self._walk(self._stem_pool(s1, dev, st), lambda tag, a_in, relu, res: self._conv(tag, a_in, pk[tag], N, relu, res, dev, st))
        return self._to_nchw(cur, dev, st)
