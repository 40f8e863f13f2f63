"""What the conv -> BatchNorm executors share (``resnet_executor.ResNetPlan``, ``bn_executor.BNPlan``): the buffers and caches of a plan, the
per-pass record of a unit, the weight packer, the stem, and the steps of a backward pass that do not depend on which BatchNorm kernel a plan runs."""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _hip
from ._hip import EPI_NONE, ConvPackItem, ConvUnpackItem, IgemmDesc, WgradDesc, check, ptr
from .config import CONFIG as CFG
from .plans import igemm_call
from .runtime import RT, Act, _on_side_stream, _round_up, _timed, desc_aux, f32, igemm_desc, side_stream, stem_tiles_ok


@dataclass(slots=True)
class Unit:
    """one conv -> BatchNorm unit of one training forward, as the backward pass needs it"""
    tag: object                    # the plan's name of the unit: keys its buffers, labels its launches
    conv: nn.Conv2d
    bn: nn.BatchNorm2d
    x: Act                         # the conv's input
    z: Act                         # the conv's output, kept
    y: Act                         # BatchNorm [+ residual] + activation of z
    stats: torch.Tensor            # the unit's 4 * C floats of the statistics arena (batch mean, invstd, ...)
    wd: torch.Tensor | None        # data-gradient operand of the conv (the stem has none)
    k: int
    s: int
    p: int
    first: bool = False            # the 7x7/s2/p3 stem: NHWC4 input, its own weight-gradient kernel, no data gradient
    relu: bool = True              # ResNetPlan: ReLU behind the BatchNorm
    res: bool = False              # ResNetPlan: a residual is added before the ReLU
    pool: bool = False             # BNPlan: MaxPool2d(2,2) behind the unit ..
    fused: bool = False            # .. inside the BatchNorm + LeakyReLU passes (y is the pooled map)
    out: Act | None = None         # BNPlan: what the next unit reads (y, or the pooled y of an unfused pool)


class _ConvBNBase:
    WHAT = ""                      # "a ResNet trunk": how messages of the autograd bridge name the plan
    NO_INPUT_GRAD = None           # the message a plan that computes no input gradient refuses one with

    def __init__(self):
        self._bufs: dict = {}        # activation buffers, by (key, geometry, device)
        self._bn_scratch = None      # (fp64 accumulators, fp32 scale / shift) of the BatchNorm kernels
        self._coef = self._zero_bias = None              # backward: BatchNorm-backward coefficients; the bias of a data gradient that adds a residual
        self._stats = None           # the statistics arena of a training forward
        self._stem_part = self._stem_db = None           # partial sums / bias gradient of yolo_wgrad_stem7
        self._train_pk = None        # (versions, {tag: (forward operand, data-gradient operand, conv, bn)}) of the raw weights
        self._train_gen = 0          # counts training forwards: the buffers hold the latest one only
        self.trace = None            # tests: a list that backward_train fills with (where, "gout" | "gx", NCHW fp32 gradient)

    # -- BN folding: y = gamma * (conv(x) - mean) / sqrt(var + eps) + beta
    @staticmethod
    def _fold(conv: nn.Conv2d, bn: nn.BatchNorm2d):
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        w = conv.weight.detach().float() * scale.view(-1, 1, 1, 1)
        b = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
        if conv.bias is not None:
            b = b + conv.bias.detach().float() * scale
        return w.contiguous(), b.contiguous()

    def _scratch(self, dev):
        if self._bn_scratch is None or self._bn_scratch[0].device != dev:
            self._bn_scratch = (torch.zeros(_hip.BN_ACC_REPLICAS * 2 * 2048, dtype=torch.float64, device=dev), torch.empty(2 * 2048, dtype=torch.float32, device=dev))
        return self._bn_scratch

    def _bwd_scratch(self, dev):
        if self._coef is None or self._coef.device != dev:
            self._coef = torch.empty(3 * 2048, dtype=torch.float32, device=dev)
            self._zero_bias = torch.zeros(2048, dtype=torch.float32, device=dev)

    def _act(self, key, N, H, W, C, halo, dev):
        k = (key, N, H, W, C, halo, str(dev))
        a = self._bufs.get(k)
        if a is None:
            a = Act(N, H, W, C, halo, dev)
            self._bufs[k] = a
        return a

    def _stat_arena(self, units, dev):
        """-> take(C): the next 4 * C floats of the plan's statistics arena, which holds 4 floats per BatchNorm channel of ``units``"""
        n = 4 * sum(bn.num_features for (_, _, bn, _) in units)
        if self._stats is None or self._stats.numel() < n or self._stats.device != dev:
            self._stats = torch.empty(n, dtype=torch.float32, device=dev)
        cursor = 0

        def take(C):
            nonlocal cursor
            cursor += 4 * C
            return self._stats[cursor - 4 * C: cursor]
        return take

    @staticmethod
    def _geom(a_in: Act, conv: nn.Conv2d):
        """(k, stride, pad, Ho, Wo) of conv over a_in"""
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        return k, s, p, (a_in.H + 2 * p - k) // s + 1, (a_in.W + 2 * p - k) // s + 1

    @staticmethod
    def _desc(a_in: Act, shift: int, stride: int, k: int, a_out: Act, epilogue: int, slope: float) -> IgemmDesc:
        """a k x k conv that reads a_in from `shift` pixels up / left of its interior and fills a_out's interior, channels as the buffers have them"""
        d = igemm_desc(a_out.N, a_out.H, a_out.W, stride, k, k, a_in.C, a_out.C, a_in, a_in.interior_off(shift), a_out)
        d.epilogue, d.slope = epilogue, slope
        return d

    def _stem_input(self, x: torch.Tensor, st) -> Act:
        """the batch as the stem reads it: an NHWC4 bf16 copy with a halo of 3"""
        N, _, H, W = x.shape
        x = f32(x)
        a = self._act("in", N, H, W, 4, 3, x.device)
        check(RT.lib().yolo_nchw_f32_to_nhwc_bf16(ptr(x), N, 3, H, W, a.p, 4, 3, 3, st), "nchw->nhwc4")
        return a

    @staticmethod
    def _stem_desc(a: Act, out: Act, epilogue: int, slope: float) -> IgemmDesc:
        """the stem as a row-segment implicit GEMM: 7 taps of 8 pixels x 4 channels per output pixel"""
        d = igemm_desc(a.N, out.H, out.W, 2, 7, 1, 32, 64, a, 0, out)
        d.epilogue, d.slope = epilogue, slope
        return d

    @staticmethod
    def _to_nchw(cur: Act, dev, st) -> torch.Tensor:
        out = torch.empty((cur.N, cur.C, cur.H, cur.W), dtype=torch.float32, device=dev)
        check(RT.lib().yolo_nhwc_bf16_to_nchw_f32(cur.p, cur.N, cur.C, cur.H, cur.W, cur.halo, ptr(out), st), "nhwc->nchw")
        return out

    def _pack(self, units, cached, fold: bool = False, dgrad: bool = False):
        """bf16 operands of ``units`` ((tag, conv, bn, first) in forward order) -> (versions, {tag: (forward operand, second, conv, bn)}), to be kept
        by the caller and handed back as ``cached``: nothing is launched while the versions stand.
        fold (inference): BatchNorm folded into the weights, second = the folded fp32 bias; stale when any parameter or buffer changed.
        Otherwise the raw conv weights, stale when one of them changed; second = the data-gradient operand if ``dgrad`` (the stem has none), else None.
        One yolo_pack_conv_weight per conv into fresh operands; with dgrad, yolo_pack_conv_weights_multi, 32 layers per launch, for every conv it takes,
        and the operands are refilled in place."""
        if fold:
            ver = tuple(int(t._version) for (_, conv, bn, _) in units for m in (conv, bn) for t in (*m.parameters(), *m.buffers()))
        else:
            ver = tuple(int(conv.weight._version) for (_, conv, _, _) in units)
        if cached is not None and cached[0] == ver:
            return cached
        L_, st = RT.lib(), RT.stream()
        out = cached[1] if cached is not None else {}
        items = []
        for (tag, conv, bn, first) in units:
            w, b = self._fold(conv, bn) if fold else (f32(conv.weight), None)
            co, ci, k, _ = w.shape
            old = out.get(tag) if dgrad else None
            if old is not None and old[0].device == w.device:
                wf, wd = old[0], old[1]
            else:
                wf = torch.empty((co, 7, 8, 4) if first else (co, k, k, ci), dtype=torch.bfloat16, device=w.device)
                wd = torch.empty((ci, k, k, co), dtype=torch.bfloat16, device=w.device) if dgrad and not first else None
            if first:
                check(L_.yolo_pack_conv_weight(ptr(w), co, 3, 7, 7, 4, 8, ptr(wf), None, st), "pack stem")
            elif dgrad and co % 64 == 0 and ci % 64 == 0:
                items.append((ConvPackItem(w.data_ptr(), wf.data_ptr(), wd.data_ptr(), co, ci, k, k), w))
            else:
                check(L_.yolo_pack_conv_weight(ptr(w), co, ci, k, k, ci, k, ptr(wf), ptr(wd) if dgrad else None, st), "pack")
            out[tag] = (wf, b if fold else wd, conv, bn)
        for i in range(0, len(items), 32):
            tab = (ConvPackItem * len(items[i: i + 32]))(*[it[0] for it in items[i: i + 32]])
            check(L_.yolo_pack_conv_weights_multi(tab, len(items[i: i + 32]), st), "pack_conv_weights_multi")
        return ver, out

    def _stem_wgrad(self, xin: Act, dz0: Act, conv: nn.Conv2d, N, Ho, Wo, dev, st) -> torch.Tensor:
        """fp32 weight gradient of the 7x7/s2 stem from its NHWC4 input and dz0 (Ho x Wo, 64 channels): the direct kernel, or the row-unfolded fallback"""
        L_ = RT.lib()
        dw = torch.empty_like(conv.weight, dtype=torch.float32)
        if self._stem_part is None or self._stem_part.device != dev:
            self._stem_part = torch.empty((768 * 14400,), dtype=torch.float32, device=dev)
            self._stem_db = torch.empty(64, dtype=torch.float32, device=dev)
        part = self._stem_part
        if stem_tiles_ok(64, Ho, Wo):
            check(L_.yolo_wgrad_stem7(xin.p, dz0.p, N, Ho, Wo, xin.img_stride, xin.row_stride, dz0.img_stride, dz0.row_stride, dz0.interior_off(),
                                      ptr(dw), ptr(self._stem_db), ptr(part), part.numel(), st), "wgrad_stem7")
        else:
            # stem maps that the direct kernel's 8 x 16-pixel tiles do not cover (inputs that are not (16k) x (32k) pixels): the generic weight-gradient
            # kernel over a row-unfolded copy of the input (7 kernel rows x 8 columns x 4 channels per output pixel), as Plan.backward does
            xcol = self._act(("stem", "xcol"), N, Ho, Wo, 7 * 32, 1, dev)
            check(L_.yolo_im2col_rows(xin.p, xin.img_stride, xin.row_stride, xin.px_stride, 2, 7, 32, N, Ho, Wo, 1, xcol.p, st), "im2col_rows")
            dwp = torch.zeros(64 * 7 * 8 * 4, dtype=torch.float32, device=dev)
            wd = WgradDesc(dz0.slots, dz0.px_stride, xcol.px_stride, 64, 7 * 32, 1, 1, 0, xcol.row_stride, max(1, min(1024, dz0.slots // 4096)), 0)
            check(L_.yolo_wgrad(ctypes.byref(wd), xcol.p, dz0.p, ptr(dwp), None, st), "wgrad stem")
            check(L_.yolo_unpack_conv_wgrad(ptr(dwp), 64, 3, 7, 7, 4, 8, ptr(dw), 0, st), "unpack stem")
        return dw


class _TrainBackward:
    """one backward pass over conv -> BatchNorm units: the weight gradients (and their unpack passes) on the low-priority second stream, beside the
    BatchNorm-backward / data-gradient chain (Plan.backward does the same): the chain's HBM-bound BatchNorm passes and the MFMA-bound weight gradients
    mix well.  ``grads`` collects {parameter: fp32 gradient}.  A plan's backward_train keeps the wiring of its units and its own BatchNorm-backward
    kernel; the steps around that kernel are here."""

    def __init__(self, plan: _ConvBNBase, saved, convs, st):
        """saved: what the plan's forward_train returned; convs: the convs whose weight gradient goes through ``wgrad`` (all but the stem)"""
        if saved["gen"] != plan._train_gen:
            raise RuntimeError(f"{type(plan).__name__}: a later training forward has reused this forward's activation buffers -- call backward() "
                               "before the next forward of the same backbone (one forward in flight per plan)")
        self.plan, self.N, self.dev, self.st = plan, saved["N"], saved["dev"], st
        N, dev = self.N, self.dev
        self.L_ = RT.lib()
        self.acc = plan._scratch(dev)[0]
        plan._bwd_scratch(dev)
        self.grads: dict = {}
        self.offs, tot = {}, 0
        for c in convs:
            self.offs[id(c)] = tot
            tot += _round_up(c.weight.numel(), 64)
        self.scratch = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.pending: list = []
        self.main_t = RT.STREAMS.current(dev)
        self.side_t = side_stream(dev) if CFG.WGRAD_STREAM else None

    def seed(self, out: Act, gout: torch.Tensor) -> Act:
        """the gradient of the forward's NCHW fp32 output as an NHWC bf16 buffer shaped like ``out``"""
        gout = f32(gout)
        g = self.plan._act(("g", "out"), self.N, out.H, out.W, out.C, 1, self.dev)
        check(self.L_.yolo_nchw_f32_to_nhwc_bf16(ptr(gout), self.N, out.C, out.H, out.W, g.p, out.C, 1, 1, self.st), "gout nchw->nhwc")
        return g

    def note(self, where, what: str, g: Act):
        if self.plan.trace is not None:
            self.plan.trace.append((where, what, g.interior().float().permute(0, 3, 1, 2).contiguous()))

    def bn_outputs(self, u: Unit):
        """what the BatchNorm-backward kernel of unit u writes -> (dz, its image / row / pixel strides and interior offset, dg, db).  dz has the form
        yolo_wgrad and the data gradient read: on the conv's output grid, or, behind a strided conv, zero-stuffed on its INPUT grid.  dg and db are
        entered into ``grads``."""
        z, bn = u.z, u.bn
        grid, m = (z, 1) if u.first or u.s == 1 else (u.x, u.s)
        dz = self.plan._act((u.tag, "dz"), self.N, grid.H, grid.W, z.C, 1, self.dev)
        dg, db = torch.empty_like(bn.weight, dtype=torch.float32), torch.empty_like(bn.bias, dtype=torch.float32)
        self.grads[bn.weight], self.grads[bn.bias] = dg, db
        return dz, (dz.img_stride, m * dz.row_stride, m * dz.px_stride, dz.interior_off()), dg, db

    def flush(self, at_least: int = 0):
        """the packed -> OIHW conversion of the pending weight gradients, 32 per launch, on the second stream; not yet with fewer than ``at_least``"""
        if len(self.pending) < at_least:
            return
        with _on_side_stream(self.main_t, self.side_t):
            pending = self.pending
            for i in range(0, len(pending), 32):
                items = [ConvUnpackItem(dwp.data_ptr(), dw.data_ptr(), c.out_channels, c.in_channels, c.kernel_size[0], c.kernel_size[1])
                         for (c, dwp, dw) in pending[i: i + 32]]
                check(self.L_.yolo_unpack_conv_wgrads_multi((ConvUnpackItem * len(items))(*items), len(items), RT.stream()), "unpack_conv_wgrads_multi")
            pending.clear()

    def wgrad(self, u: Unit, dz: Act):
        N = self.N
        conv, xin, k, s, p = u.conv, u.x, u.k, u.s, u.p
        Hout, Wout = u.z.H, u.z.W
        o = self.offs[id(conv)]
        dwp = self.scratch[o: o + conv.weight.numel()]
        if Hout >= 2 and Wout >= 2 and (s > 1 or dz.Hp * dz.Wp >= 1.12 * Hout * Wout):
            wd = WgradDesc(N * Hout * Wout, dz.px_stride, xin.px_stride, conv.out_channels, conv.in_channels, k, k, p, xin.row_stride, 0, 0, 0,
                           Wout, Hout, dz.Hp * dz.Wp, dz.Wp * s, s, dz.halo * dz.Wp + dz.halo)
        else:
            wd = WgradDesc(dz.slots, dz.px_stride, xin.px_stride, conv.out_channels, conv.in_channels, k, k, p, xin.row_stride, 0, 0)
        dw = torch.empty_like(conv.weight, dtype=torch.float32)
        with _on_side_stream(self.main_t, self.side_t) as wst:
            with _timed(f"{u.tag}.wgrad", "wgrad", 2.0 * N * Hout * Wout * conv.out_channels * conv.in_channels * k * k):
                check(self.L_.yolo_wgrad(ctypes.byref(wd), xin.p, dz.p, ptr(dwp), None, wst), f"wgrad {u.tag}")
        self.grads[conv.weight] = dw
        self.pending.append((conv, dwp, dw))

    def dgrad(self, u: Unit, dz: Act, add: Act | None) -> Act:
        N, plan = self.N, self.plan
        conv, xin, k, p = u.conv, u.x, u.k, u.p
        g = plan._act((u.tag, "gx"), N, xin.H, xin.W, conv.in_channels, 1, self.dev)
        d = plan._desc(dz, k - 1 - p, 1, k, g, EPI_NONE, 1.0)         # over the conv's input grid, with the flipped panel
        d.split_k = 1
        aux, bias = None, None
        if add is not None:
            d.epilogue = _hip.EPI_BIAS_ADD_LRELU          # slope 1: out = conv + 0 + aux
            desc_aux(d, add)
            aux, bias = add.p, ptr(plan._zero_bias)
        with _timed(f"{u.tag}.dgrad", "igemm", 2.0 * N * xin.H * xin.W * conv.out_channels * conv.in_channels * k * k):
            igemm_call(d, dz.p, ptr(u.wd), bias, aux, g.p, self.st, f"dgrad {u.tag}")
        return g

    def stem_wgrad(self, u: Unit, dz: Act):
        self.grads[u.conv.weight] = self.plan._stem_wgrad(u.x, dz, u.conv, self.N, u.z.H, u.z.W, self.dev, self.st)

    def finish(self) -> dict:
        """every weight gradient is final before the pass returns"""
        if self.side_t is not None:
            self.main_t.wait_stream(self.side_t)
        return self.grads
