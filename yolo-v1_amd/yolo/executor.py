"""Layer-plan executor of the YOLOv1 networks: runs a conv / pool / FC stack of the reference's models on the HIP kernels.

A *plan* is built once from the PyTorch-layout modules (``nn.Conv2d``/``nn.LeakyReLU``/``nn.MaxPool2d`` inside ``backbone.features`` / ``head`` -- those
modules stay the owners of the fp32 parameters so that ``state_dict`` keys and shapes are the reference's).  On a device tensor the
modules' ``forward`` is bypassed and the plan drives libyolo_hip.so:

  * activations: zero-haloed NHWC bf16 buffers with a guard band (``runtime.Act``), allocated once per (batch, mode) and reused; producers only ever
    write the interior, so halos stay zero;
  * weights: bf16 panels re-packed from the fp32 masters only when a parameter's version changes;
  * forward = one yolo_igemm per conv / Linear (+ pool / flatten helpers), launched with the problem's plan (``plans.igemm_call``); ``Plan.forward`` is a
    loop over the layers that hands each to the ``_fwd_*`` step of its kind;
  * backward = per conv one yolo_wgrad (on a second stream) + one yolo_igemm data-gradient whose epilogue applies the previous LeakyReLU's
    derivative (or a pool backward): ``Plan.backward`` walks the layers the other way through the ``_bwd_*`` steps, which share a ``_Backward`` state;
  * descriptors are filled by the builders of ``runtime`` (``igemm_desc``, ``desc_aux``, ``rows_desc``), nowhere else.

Everything is enqueued on the current PyTorch stream (and the plan's side stream); there is no host synchronisation.  Switches: ``plan.cfg`` (an
``EngineConfig``) if set, else the process-wide ``config.CONFIG``."""

from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _hip
from ._hip import (EPI_BIAS, EPI_BIAS_LRELU, EPI_MUL_DLRELU, EPI_NONE, ConvPackItem, ConvUnpackItem, IgemmDesc, PoolDesc, WgradDesc, check, ptr)
from .config import CONFIG as CFG
from .plans import igemm_call
from .runtime import (RT, Act, _attach_wgrad_slabs, _EventSlot, _igemm, _on_side_stream, _round_up, _timed, desc_aux, f32, igemm_desc, is_stem,
                      require_pool2, rows_desc, side_stream, stem_tiles_ok)


@dataclass
class Layer:
    kind: str                      # conv | pool | flatten | fc
    name: str = ""
    Cout: int = 0
    Cin: int = 0
    K: int = 1
    stride: int = 1
    pad: int = 0
    lrelu: bool = False
    dropout: float = 0.0
    drop_mod: object = None     # the nn.Dropout behind a Linear: its p is read at every forward, as stock torch does (a plan outlives `model.head[3].p = 0.0`)
    weight: nn.Parameter | None = None
    bias: nn.Parameter | None = None
    first: bool = False            # the 3-channel 7x7/s2 stem (NHWC4 input, row-segment taps)
    # geometry of the workspace in use: Plan._workspace computes it, Plan._apply_geom puts it back
    Hin: int = 0
    Win: int = 0
    Hout: int = 0
    Wout: int = 0


class FcFactors:
    """The pending weight gradient of one Linear layer as its two batch factors (EngineConfig.FC_FACTORED): G = scale * dy[:, :O]^T x, with
    ``dy`` bf16 [rows][ld_dy] (the gradient wrt the layer's output, through its dropout + LeakyReLU) and ``x`` bf16 [rows][ld_x] (the layer's
    input).  The record OWNS both tensors: ``x`` is a copy of the workspace's flatten buffer, which the next forward rewrites while a
    background optimizer pass may still read the factors.  ``parallel.gather_fc_factors`` replaces it by the ranks' concatenation with
    ``scale = 1 / world``."""

    __slots__ = ("dy", "x", "rows", "scale")

    def __init__(self, dy: torch.Tensor, x: torch.Tensor, rows: int, scale: float = 1.0):
        self.dy, self.x, self.rows, self.scale = dy, x, int(rows), float(scale)

    def desc(self, weight) -> "_hip.FcFactors":
        """struct yolo_fc_factors for the [O][I] parameter ``weight``"""
        O, I = weight.shape
        return _hip.FcFactors(self.dy.data_ptr(), self.x.data_ptr(), self.rows, O, I, self.dy.stride(0), self.x.stride(0), self.scale)

    def nbytes(self) -> int:
        return self.dy.numel() * self.dy.element_size() + self.x.numel() * self.x.element_size()


def fc_factors_of(p):
    """the pending FcFactors record of parameter ``p`` (None: it has an ordinary gradient or none) and the plan that holds it"""
    ref = getattr(p, "_fc_factored_plan", None)
    plan = ref() if ref is not None else None
    rec = plan.fc_factors.get(id(p)) if plan is not None else None
    return (rec, plan) if rec is not None else (None, None)


class Plan:
    """Executable plan for [conv|pool]* [flatten fc*]? (with no conv / pool in front, the input is the feature map that nn.Flatten flattens)."""

    SLOPE = 0.1

    def __init__(self, layers: list[Layer], in_channels: int, input_is_image: bool, S: int | None = None):
        self.layers = layers
        self.in_channels = in_channels
        self.input_is_image = input_is_image
        self.params: list[nn.Parameter] = []
        for L in layers:
            if L.kind in ("conv", "fc"):
                self.params += [L.weight, L.bias]
        self._pf: dict[int, tuple] = {}
        self._pd: dict[int, tuple] = {}
        self._pfb: dict[int, tuple] = {}
        self._pd2: dict[int, tuple] = {}
        self._ws: dict[tuple, list] = {}
        self.grad_norm_sq: dict = {}   # id(weight) -> ((data_ptr, shape) of the gradient, its version, device double |g|^2) left by the last backward pass
        self.fc_factors: dict = {}     # id(weight) -> FcFactors left by the last backward pass (EngineConfig.FC_FACTORED); the optimizer step that consumes a record removes it
        self.debug_keep = False      # tests: True = keep the last workspace (activations + gradients) for inspection AND store the
                                     # un-pooled activations; "codes" = keep the workspace of the product path (pooled maps + arg-max codes)
        self.last = None
        # optional persistent gradient arena (data-parallel training): one flat fp32 buffer holding every
        # parameter gradient in the order backward PRODUCES them (last layer first), so that finished
        # gradients form a growing contiguous prefix that can be all-reduced while backward continues
        self.arena = None
        self.arena_views: dict[int, tuple] = {}
        self.on_grad_ready = None    # callback(lo, hi): arena[lo:hi] (elements) is final -- called with the PRODUCING stream current
        self.on_backward_done = None # callback(): every gradient is final and the current stream has waited for all of them
        self.on_stream_wait = None   # callback(waiter, waited): hipStream_t handles; `waiter` now waits for everything queued on `waited`
        self.cfg = None              # an EngineConfig of this plan's own (None: the process-wide config.CONFIG)
        self.params_ready = _EventSlot()      # event behind a background update of the Linear layers (forward waits in front of them)
        self.owner = None            # weakref to the nn.Module whose layers this plan runs (models.*.hip_plan sets it)

    @property
    def c(self):
        """the switches this plan runs with"""
        return self.cfg if self.cfg is not None else CFG

    def attach_grad_arena(self, device) -> torch.Tensor:
        """Allocate the gradient arena; backward then writes gradients into it, assigns ``p.grad`` views and
        returns no gradients to autograd (gradients are OVERWRITTEN each backward; yolo.optim.GradAccumulator keeps the sum of several
        backward passes beside the arena and folds it back into it)."""
        order = [li for li in reversed(range(len(self.layers))) if self.layers[li].kind in ("conv", "fc")]
        off = 0
        wv, bv = {}, {}
        for li in order:                          # every view starts on a 256-B boundary (float4 kernels)
            n = 0 if self._fc_factored(self.layers[li]) else self.layers[li].weight.numel()      # a factored layer has no dw: its factors are gathered instead
            wv[li] = (off, off + n, _round_up(off + n, 64))
            off = _round_up(off + n, 64)
        self._arena_w_end = off
        for li in order:
            n = self.layers[li].bias.numel()
            bv[li] = (off, off + n)
            off = _round_up(off + n, 64)
        self.arena = torch.zeros(off, dtype=torch.float32, device=device)
        self.arena_views = {li: (self.arena[wv[li][0]:wv[li][1]].view_as(self.layers[li].weight) if wv[li][1] > wv[li][0] else None,
                                 self.arena[bv[li][0]:bv[li][1]].view_as(self.layers[li].bias), wv[li][0], wv[li][2])
                            for li in order}
        return self.arena

    def _fc_factored(self, L: Layer) -> bool:
        """this Linear layer's weight gradient stays factored (EngineConfig.FC_FACTORED; I % 8 == 0 is what the kernels' 16-B operand loads need)"""
        return bool(self.c.FC_FACTORED) and L.kind == "fc" and L.Cout * L.Cin >= self.c.FC_FACTORED_MIN and L.Cin % 8 == 0

    @_hip.device_guard
    def fc_weight_grad(self, weight: torch.Tensor) -> torch.Tensor:
        """the gradient of a factored Linear weight on request (yolo_fc_factored_grad), fp32 in the weight's shape: what ``weight.grad`` would hold.
        The record stays pending: the optimizer step forms the same bits tile by tile."""
        rec = self.fc_factors.get(id(weight))
        if rec is None:
            raise RuntimeError("Plan.fc_weight_grad: this parameter has no pending factored gradient (EngineConfig.FC_FACTORED off, no backward pass "
                               "since the last optimizer step, or not a qualifying Linear weight)")
        g = torch.empty(tuple(weight.shape), dtype=torch.float32, device=rec.dy.device)
        d = rec.desc(weight)
        check(RT.lib().yolo_fc_factored_grad(ctypes.byref(d), ptr(g), RT.stream()), "yolo_fc_factored_grad")
        return g

    def _layer_done(self, li: int):
        if self.arena is not None and self.on_grad_ready is not None:
            _, _, a, b = self.arena_views[li]
            self.on_grad_ready(a, b)

    # ------------------------------------------------------------------ construction helpers
    @staticmethod
    def from_modules(mods, in_channels: int, input_is_image: bool) -> "Plan":
        """mods: flat list of nn.Module (Conv2d, LeakyReLU, MaxPool2d, Flatten, Linear, Dropout)."""
        layers: list[Layer] = []
        i = 0
        mods = list(mods)
        while i < len(mods):
            m = mods[i]
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(m, nn.Conv2d):
                k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
                if m.kernel_size[0] != m.kernel_size[1] or m.groups != 1 or m.dilation != (1, 1) or m.bias is None:
                    raise ValueError(f"unsupported conv {m}")
                act = isinstance(nxt, nn.LeakyReLU)
                if act and abs(nxt.negative_slope - Plan.SLOPE) > 1e-12:
                    raise ValueError("only LeakyReLU(0.1) is fused")
                first = is_stem(m)
                if not first and not ((k == 3 and p == 1) or (k == 1 and p == 0)) or (not first and s not in (1, 2)):
                    raise ValueError(f"unsupported conv geometry {m}")
                if not first and (m.in_channels % 32 or m.out_channels % 8):
                    raise ValueError(f"unsupported channel counts {m}")
                layers.append(Layer("conv", Cout=m.out_channels, Cin=m.in_channels, K=k, stride=s, pad=p, lrelu=act,
                                    weight=m.weight, bias=m.bias, first=first))
                i += 2 if act else 1
            elif isinstance(m, nn.MaxPool2d):
                require_pool2(m)
                layers.append(Layer("pool"))
                i += 1
            elif isinstance(m, nn.Flatten):
                layers.append(Layer("flatten"))
                i += 1
            elif isinstance(m, nn.Linear):
                if m.in_features % 64 or m.bias is None:
                    raise ValueError(f"unsupported Linear {m}: in_features must be a multiple of 64")
                act = isinstance(nxt, nn.LeakyReLU)
                j = i + (2 if act else 1)
                drop, drop_mod = 0.0, None
                if j < len(mods) and isinstance(mods[j], nn.Dropout):
                    drop, drop_mod = mods[j].p, mods[j]
                    j += 1
                layers.append(Layer("fc", Cout=m.out_features, Cin=m.in_features, lrelu=act, dropout=drop, drop_mod=drop_mod, weight=m.weight, bias=m.bias))
                i = j
            else:
                raise ValueError(f"unsupported module in plan: {m}")
        return Plan(layers, in_channels, input_is_image)

    # ------------------------------------------------------------------ weights
    # bf16 operand copies of the fp32 masters, cached per layer and keyed on (tensor version, storage):
    #   _pf[li] = (key, forward operand)        conv: [Cout][KH][KW][Cin]      Linear: [O][K] (the master's layout)
    #   _pd[li] = (key, data-gradient operand)  conv: [Cin][KH][KW][Cout] flipped   Linear: [K][ld(O)] (only the
    #             small Linear layers; the big one in front of nn.Flatten uses the forward copy, see backward)
    @staticmethod
    def _wkey(w):
        return (w._version, w.data_ptr())

    def _multi_ok(self, L: Layer) -> bool:
        return L.kind == "conv" and not L.first and L.Cout % 64 == 0 and L.Cin % 64 == 0 and L.K * L.K <= 9

    def _src(self, L: Layer):
        return f32(L.weight)

    def _pack_all(self, need_dgrad: bool):
        """Refresh every stale conv operand of the plan in ONE launch (yolo_pack_conv_weights_multi)."""
        items, keep, done = [], [], []
        for li, L in enumerate(self.layers):
            if not self._multi_ok(L):
                continue
            key = self._wkey(L.weight)
            f, d = self._pf.get(li), self._pd.get(li)
            want_f = f is None or f[0] != key
            want_d = need_dgrad and li > 0 and (d is None or d[0] != key)
            if not (want_f or want_d):
                continue
            dev = L.weight.device
            wsrc = self._src(L)
            keep.append(wsrc)
            wf = wd = None
            if want_f:
                wf = f[1] if f is not None else torch.empty((L.Cout, L.K, L.K, L.Cin), dtype=torch.bfloat16, device=dev)
            if want_d:
                wd = d[1] if d is not None else torch.empty((L.Cin, L.K, L.K, L.Cout), dtype=torch.bfloat16, device=dev)
            items.append(ConvPackItem(wsrc.data_ptr(), wf.data_ptr() if wf is not None else None, wd.data_ptr() if wd is not None else None,
                                      L.Cout, L.Cin, L.K, L.K))
            done.append((li, key, wf, wd))
        if items:
            tab = (ConvPackItem * len(items))(*items)
            check(RT.lib().yolo_pack_conv_weights_multi(tab, len(items), RT.stream()), "pack_conv_weights_multi")
            for li, key, wf, wd in done:
                if wf is not None:
                    self._pf[li] = (key, wf)
                if wd is not None:
                    self._pd[li] = (key, wd)

    def _pack(self, li: int, need_dgrad: bool):
        """(forward operand, data-gradient operand | None) of layer li, refreshed if the master changed."""
        L = self.layers[li]
        key = self._wkey(L.weight)
        f, d = self._pf.get(li), self._pd.get(li)
        ok_f = f is not None and f[0] == key
        ok_d = d is not None and d[0] == key
        if ok_f and (ok_d or not need_dgrad):
            return f[1], (d[1] if ok_d else None)
        dev = L.weight.device
        wsrc = self._src(L)
        wf = f[1] if f is not None else None
        wd = d[1] if d is not None else None
        if L.kind == "conv":
            if L.first:
                if wf is None:
                    wf = torch.empty((L.Cout, 7, 8, 4), dtype=torch.bfloat16, device=dev)
                check(RT.lib().yolo_pack_conv_weight(ptr(wsrc), L.Cout, 3, 7, 7, 4, 8, ptr(wf), None, RT.stream()), "pack_conv_weight")
                self._pf[li] = (key, wf)
                return wf, None
            if wf is None:
                wf = torch.empty((L.Cout, L.K, L.K, L.Cin), dtype=torch.bfloat16, device=dev)
            if need_dgrad and wd is None:
                wd = torch.empty((L.Cin, L.K, L.K, L.Cout), dtype=torch.bfloat16, device=dev)
            check(RT.lib().yolo_pack_conv_weight(ptr(wsrc), L.Cout, L.Cin, L.K, L.K, L.Cin, L.K, None if ok_f else ptr(wf),
                                              ptr(wd) if (need_dgrad and not ok_d) else None, RT.stream()), "pack_conv_weight")
        else:
            if not ok_f:
                if wf is None:
                    wf = torch.empty((L.Cout, L.Cin), dtype=torch.bfloat16, device=dev)
                check(RT.lib().yolo_cast_f32_to_bf16(ptr(wsrc), wsrc.numel(), ptr(wf), RT.stream()), "cast fc weight")
            if need_dgrad and not ok_d:
                ld = _round_up(L.Cout, 32)
                if wd is None:
                    wd = torch.zeros((L.Cin, ld), dtype=torch.bfloat16, device=dev)
                check(RT.lib().yolo_transpose_f32_to_bf16(ptr(wsrc), L.Cout, L.Cin, ptr(wd), ld, RT.stream()), "transpose")
        self._pf[li] = (key, wf)
        if need_dgrad:
            self._pd[li] = (key, wd)
            return wf, wd
        return wf, (wd if ok_d else None)

    def _stride2_panels(self, li: int, wdg: torch.Tensor) -> dict:
        """data-gradient operands of a stride-2 3x3 conv by input-pixel parity: slices of the flipped panel
        wd[ci][ky'][kx'][co] (ky' = 2 - ky): parity 0 uses ky' = 1, parity 1 uses ky' = 0 (tap offset 0) and 2 (offset 1)."""
        L = self.layers[li]
        key = self._wkey(L.weight)
        hit = self._pd2.get(li)
        if hit is not None and hit[0] == key:
            return hit[1]
        sel = {0: slice(1, 2), 1: slice(0, 3, 2)}      # basic slices: one strided copy per class, no gather kernels
        panels = {}
        for py in (0, 1):
            for px in (0, 1):
                panels[(py, px)] = wdg[:, sel[py], sel[px], :].contiguous()
        self._pd2[li] = (key, panels)
        return panels

    def _pack_fc_blocked(self, li: int, hwc=None):
        """inference operand of a Linear layer: bf16 [O/128][K/64][128][64] panels (contiguous 16-KB stage reads; the
        plain [O][K] copy that training shares with the optimizer streams ~15 % slower).  ``hwc = (C, HW)``: K axis permuted from
        nn.Flatten's (c, hw) order to (hw, c) -- the layer then reads the dense NHWC conv output directly (self.c.FLATTEN_FREE)."""
        L = self.layers[li]
        key = (self._wkey(L.weight), hwc)
        hit = self._pfb.get(li)
        if hit is not None and hit[0] == key:
            return hit[1]
        wsrc = self._src(L)
        wb = hit[1] if hit is not None else torch.empty((_round_up(L.Cout, 128) * L.Cin,), dtype=torch.bfloat16, device=L.weight.device)
        if hwc is not None:
            check(RT.lib().yolo_pack_fc_weight_blocked_hwc(ptr(wsrc), L.Cout, hwc[0], hwc[1], ptr(wb), RT.stream()), "pack_fc_blocked_hwc")
        else:
            check(RT.lib().yolo_pack_fc_weight_blocked(ptr(wsrc), L.Cout, L.Cin, ptr(wb), RT.stream()), "pack_fc_blocked")
        self._pfb[li] = (key, wb)
        return wb

    def fc_biases(self):
        """bias parameters of the Linear layers on the device (updated together with their weights, yolo.optim.Adam.attach_plan)"""
        return [L.bias for L in self.layers if L.kind == "fc" and L.bias is not None and L.bias.is_cuda]

    def bf16_shadows(self):
        """[(param, bf16 forward operand with the master's layout, callback)] for the Linear layers: an optimizer
        that writes bf16(p) into the operand while it updates p calls ``callback(p)`` afterwards
        (yolo.optim.Adam.attach_plan), which saves the 822 MB + 411 MB re-cast of the big Linear per step."""
        out = []
        for li, L in enumerate(self.layers):
            if L.kind != "fc" or not L.weight.is_cuda:
                continue
            wf, _ = self._pack(li, False)

            def fresh(p, li=li, wf=wf):
                self._pf[li] = (self._wkey(p), wf)
            out.append((L.weight, wf, fresh))
        return out

    # ------------------------------------------------------------------ workspace
    def _workspace(self, N: int, x_shape, device, train: bool):
        key = (N, tuple(x_shape[1:]), str(device), train)
        pool = self._ws.setdefault(key, [])
        if pool:
            ws = pool.pop()
            self._apply_geom(ws)
            return key, ws
        ws = {"acts": [], "grads": {}, "misc": {}, "geom": {}}
        C, H, W = x_shape[1], x_shape[2], x_shape[3]
        if self.layers and self.layers[0].kind == "conv" and self.layers[0].first:
            a = Act(N, H, W, 4, 3, device)
        else:
            a = Act(N, H, W, C, 1, device)
        ws["in"] = a
        cur = a
        flat = None
        for li, L in enumerate(self.layers):
            if L.kind == "conv":
                L.Hin, L.Win = cur.H, cur.W
                L.Hout = (cur.H + 2 * L.pad - L.K) // L.stride + 1
                L.Wout = (cur.W + 2 * L.pad - L.K) // L.stride + 1
                # inference, conv -> nn.Flatten -> Linear: the conv writes a dense NHWC map (no halo) that the Linear layer reads as it
                # lies, through weight panels with a permuted K axis -- no flatten pass (self.c.FLATTEN_FREE)
                dense = (not train and self.c.FLATTEN_FREE and li + 2 < len(self.layers) and self.layers[li + 1].kind == "flatten"
                         and self.layers[li + 2].kind == "fc" and L.Cout % 8 == 0 and (L.Cout * L.Hout * L.Wout) % 64 == 0)
                cur = Act(N, L.Hout, L.Wout, L.Cout, 0 if dense else 1, device)
            elif L.kind == "pool":
                L.Hin, L.Win = cur.H, cur.W
                cur = Act(N, cur.H // 2, cur.W // 2, cur.C, 1, device)
            elif L.kind == "flatten":
                flat = torch.empty((N, cur.C * cur.H * cur.W), dtype=torch.bfloat16, device=device)
                cur = flat
            elif L.kind == "fc":
                feat = flat.shape[1] if (flat is not None and cur is flat) else None
                if feat is not None and feat != L.Cin:
                    # the reference raises here too (stock nn.Linear): e.g. a 224x224 batch into the 448x448 head
                    raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({N}x{feat} and {L.Cin}x{L.Cout}): input of "
                                       f"{tuple(x_shape[2:])} pixels does not match the Linear layer behind nn.Flatten")
                cur = None  # allocated per call (tiny)
            ws["acts"].append(cur)
            ws["geom"][li] = (L.Hin, L.Win, L.Hout, L.Wout)
        return key, ws

    def _apply_geom(self, ws):
        """the layer geometry (Hin, Win, Hout, Wout) belongs to a workspace, not to the plan: a plan may serve several input
        sizes, and a forward at another size may run between a training forward and its backward.  Every entry point that
        reads ``L.Hin`` .. ``L.Wout`` calls this first with the workspace it is about to use."""
        for li, g in ws["geom"].items():
            L = self.layers[li]
            L.Hin, L.Win, L.Hout, L.Wout = g

    def _release(self, key, ws):
        self._ws.setdefault(key, []).append(ws)

    # ------------------------------------------------------------------ descriptors
    def _conv_desc(self, L: Layer, a_in: Act, a_out: Act) -> IgemmDesc:
        if L.first:          # row-segment taps: 7 rows of 8 pixels x 4 channels, read from the buffer's first slot (the halo of 3 is the padding)
            d = igemm_desc(a_in.N, L.Hout, L.Wout, L.stride, 7, 1, 32, L.Cout, a_in, 0, a_out)
        else:
            d = igemm_desc(a_in.N, L.Hout, L.Wout, L.stride, L.K, L.K, L.Cin, L.Cout, a_in, a_in.interior_off(L.pad), a_out)
        c = self.c
        d.epilogue, d.slope, d.split_k = (EPI_BIAS_LRELU if L.lrelu else EPI_BIAS), self.SLOPE, 1
        d.tile_hint, d.tile_px = c.TILE_HINT, c.TILE_PX
        return d

    def _dgrad_desc(self, L: Layer, g: Act, N: int, gp: Act, out_mul: int = 1) -> IgemmDesc:
        """data gradient of conv layer L into gp: a stride-1 conv of its (zero-stuffed, for stride 2) output gradient g with the flipped panel, over L's input grid"""
        d = igemm_desc(N, L.Hin, L.Win, 1, L.K, L.K, L.Cout, L.Cin, g, g.interior_off(L.K - 1 - L.pad), gp, out_mul=out_mul)
        d.slope, d.split_k = self.SLOPE, 1
        return d

    @staticmethod
    def _stem_ok(L: Layer) -> bool:
        """the dedicated stem kernels apply to this layer (each site adds what else it needs)"""
        return L.kind == "conv" and L.first and stem_tiles_ok(L.Cout, L.Hout, L.Wout)

    def _stem_fwd_ok(self, L: Layer, y: Act) -> bool:
        return self.c.STEM_KERNEL and self._stem_ok(L) and y.C == 64 and L.bias.dtype == torch.float32

    @staticmethod
    def _pool_fusable(L: Layer) -> bool:
        """conv -> LeakyReLU -> MaxPool2d(2,2) as one launch: the library's 8 x 16-patch pooled epilogue (224^2 and 112^2
        maps), or the pipelined kernels' 224-pixel tiles of whole row pairs (rows of 112, 56 or 28 pixels)"""
        if L.Cout % 8:
            return False
        if L.Hout % 8 == 0 and L.Wout % 16 == 0:
            return True
        nk = L.K * L.K * L.Cin // 32
        return (not L.first and L.Cin % 32 == 0 and nk % 2 == 0 and nk >= 4 and L.Wout in (112, 56, 28) and L.Hout % 2 == 0
                and (L.Hout * L.Wout) % 112 == 0)

    def _few_tiles(self, L: Layer, N: int) -> bool:
        """small batches: a deep-K conv in front of a pool whose pooled kernel would have work for less than a quarter of the chip (batch 1: conv18 = 4
        pixel tiles x 4 channel tiles under K = 4608, 83 us) runs un-fused -- K ranges as slabs over the whole chip (plans._default_plan / the tuner's
        slab candidates; the pooled epilogue has no split form) and the pool as its own small pass (config.SMALL_SPLIT)"""
        tiles = ((N * L.Hout * L.Wout + 223) // 224) * ((L.Cout + 255) // 256)
        return bool(self.c.SMALL_SPLIT and not L.first and tiles < 64 and L.K * L.K * L.Cin >= 2304 and L.Cin % 64 == 0)

    # ------------------------------------------------------------------ forward
    def _bind_input(self, x, train: bool, u8_size):
        """the workspace of this call with every conv operand fresh and the input in ws["in"] -> (key, ws, x, stem_f32); stem_f32: nothing was
        converted, the stem kernel reads the fp32 batch x itself"""
        from .augment import U8Batch
        N, dev = x.shape[0], x.device
        batch = isinstance(x, U8Batch)
        u8 = batch or u8_size is not None
        if not u8:
            if x.dim() != 4 or x.shape[1] != self.in_channels:
                raise RuntimeError(f"expected input of shape (N, {self.in_channels}, H, W), got {tuple(x.shape)}")
            x = f32(x)
        elif not batch:
            x = x.detach()
        key, ws = self._workspace(N, x.shape if (batch or not u8) else (N, 3, u8_size[0], u8_size[1]), dev, train)
        self._pack_all(train)
        a = ws["in"]
        nhwc4 = a.C == 4 and a.halo == 3
        if u8 and not nhwc4:
            raise ValueError("uint8 input needs a plan that starts with the 7x7/s2 stem")
        if batch:
            x.into_act(a)
        elif u8:
            from . import preprocess as _pp
            _pp.preprocess_u8_into(x, u8_size, a)
        else:
            # inference: the stem kernel reads the caller's NCHW fp32 batch itself (the patch is converted on its way into LDS); training
            # keeps the NHWC4 copy, which the stem's weight gradient reads
            L0 = self.layers[0]
            if (not train and self.c.STEM_F32_INPUT and nhwc4 and self._stem_fwd_ok(L0, ws["acts"][0])
                    and 2 * L0.Hout == x.shape[2] and 2 * L0.Wout == x.shape[3]):
                return key, ws, x, True
            check(RT.lib().yolo_nchw_f32_to_nhwc_bf16(ptr(x), N, x.shape[1], x.shape[2], x.shape[3], a.p, a.C, a.halo, a.halo, RT.stream()), "nchw->nhwc")
        return key, ws, x, False

    @_hip.device_guard
    def forward(self, x: torch.Tensor, train: bool, drop_training: bool, u8_size=None):
        """x: NCHW fp32 device tensor -- or, with ``u8_size = (H, W)``, decoded uint8 images [N][h][w][3] that
        yolo_preprocess_u8 resizes + normalises straight into the stem's NHWC4 input buffer (no fp32 NCHW round trip).
        ``x`` may also be a ``yolo.augment.U8Batch`` (decoded images of different sizes + their crop / colour parameters, in training too: the
        stem's weight gradient reads the same NHWC4 buffer): yolo_augment_u8 fills the stem's input buffer.
        Returns (out, saved) -- out is (N, O) fp32 if the plan ends with an fc layer, else NCHW fp32 features."""
        N, dev = x.shape[0], x.device
        key, ws, x, stem_f32 = self._bind_input(x, train, u8_size)
        # training, conv -> LeakyReLU -> MaxPool2d(2,2): the fused epilogue stores the pooled map and, per pooled element, the 2-bit
        # window position of the maximum; the backward pass needs nothing else of the un-pooled activation (debug_keep: the tests'
        # teacher-forced checks read that activation, so it is written instead; debug_keep = "codes": keep the workspace of the product path)
        f = _Pass(ws=ws, acts=ws["acts"], c=self.c, N=N, dev=dev, lib=RT.lib(), st=RT.stream(), train=train, drop_training=drop_training, x32=x if stem_f32 else None,
                  codes_mode=train and self.c.POOL_CODES and self.debug_keep is not True, cur=ws["in"], hwc=None, fc_saved={}, out=None)
        self.grad_norm_sq.clear()
        ws["codes"] = set()
        step = {"conv": self._fwd_conv, "pool": self._fwd_pool, "flatten": self._fwd_flatten, "fc": self._fwd_fc}
        li = 0
        while li < len(self.layers):
            li += step[self.layers[li].kind](f, li)       # (a conv that pools consumes the MaxPool2d behind it)
        out, cur = f.out, f.cur
        if out is None:
            out = torch.empty((N, cur.C, cur.H, cur.W), dtype=torch.float32, device=dev)
            check(f.lib.yolo_nhwc_bf16_to_nchw_f32(cur.p, N, cur.C, cur.H, cur.W, cur.halo, ptr(out), f.st), "nhwc->nchw")
        if train:
            return out, (key, ws, f.fc_saved, N, dev)
        self._release(key, ws)
        return out, None

    def _fwd_conv(self, f, li: int) -> int:
        """conv (+ LeakyReLU), with the MaxPool2d(2,2) behind it where it fuses -> layers consumed.  Inference folds the pool into the epilogue
        (``fuse``, pool2 = 1: the conv output tiles into 8 x 16 pixel patches or whole row pairs); training does too (``dual``) and keeps what the
        backward pass needs: arg-max codes (pool2 = 3), or the un-pooled activation next to the pooled one (pool2 = 2)"""
        L, N, train, acts, cur = self.layers[li], f.N, f.train, f.acts, f.cur
        wf, _ = self._pack(li, train)
        pool_next = f.c.FUSE_POOL and li + 1 < len(self.layers) and self.layers[li + 1].kind == "pool"
        fuse = not train and pool_next and self._pool_fusable(L) and not self._few_tiles(L, N)
        b = L.bias.detach()
        full = acts[li]
        if L.first and self._stem_fwd_ok(L, full):
            return self._fwd_stem(f, li, wf, b, fuse, train and pool_next)
        dual = train and pool_next and self._pool_fusable(L) and not L.first
        dst = acts[li + 1] if (fuse or dual) else full
        d = self._conv_desc(L, cur, dst)
        d.pool2, aux = (1 if fuse else 0), None
        if dual:
            codes = self._codes(f.ws, li, dst) if f.codes_mode else None
            if codes is not None:
                d.pool2, aux = 3, ptr(codes)
            else:
                d.pool2, aux = 2, full.p
                desc_aux(d, full)
        with _timed(f"conv{li}" + ("+pool" if (fuse or dual) else ""), "igemm", 2.0 * N * L.Hout * L.Wout * L.Cout * L.Cin * L.K * L.K):
            igemm_call(d, cur.p, ptr(wf), ptr(b), aux, dst.p, f.st, f"igemm conv{li}")
        f.cur = dst
        return 2 if (fuse or dual) else 1

    def _fwd_stem(self, f, li: int, wf, b, fuse: bool, dual: bool) -> int:
        """dedicated stem kernel: input patch staged once per 8x16 tile, weights in registers.  Second output: the pool's arg-max codes (the 411 MB
        un-pooled activation of batch 64 is never written), or that activation next to the pooled one (training without codes), or none"""
        L, N, cur = self.layers[li], f.N, f.cur
        full = f.ws["acts"][li]
        dst = f.ws["acts"][li + 1] if (fuse or dual) else full
        codes = self._codes(f.ws, li, dst) if (dual and f.codes_mode) else None
        slope = self.SLOPE if L.lrelu else 1.0
        if codes is not None:
            pool2, second = 3, (ptr(codes), 0, 0, 0)
        elif dual:
            pool2, second = 1, (full.p, full.img_stride, full.row_stride, full.interior_off())
        else:
            pool2, second = (1 if fuse else 0), (None, 0, 0, 0)
        out = (dst.p, dst.img_stride, dst.row_stride, dst.interior_off())
        with _timed(f"conv{li}" + ("+pool" if (fuse or dual) else ""), "stem", 2.0 * N * L.Hout * L.Wout * L.Cout * L.Cin * L.K * L.K):
            if f.x32 is not None and li == 0:
                x = f.x32
                check(f.lib.yolo_conv_stem7_fwd_f32(ptr(x), ptr(wf), ptr(b), N, x.shape[2], x.shape[3], slope, pool2, *out, *second, f.st), "conv_stem7_fwd_f32")
            else:
                check(f.lib.yolo_conv_stem7_fwd(cur.p, ptr(wf), ptr(b), N, L.Hout, L.Wout, cur.img_stride, cur.row_stride, slope, pool2, *out, *second, f.st),
                      "conv_stem7_fwd")
        f.cur = dst
        return 2 if (fuse or dual) else 1

    def _fwd_pool(self, f, li: int) -> int:
        cur, nxt = f.cur, f.ws["acts"][li]
        pd = PoolDesc(f.N, cur.H, cur.W, cur.C, cur.halo, nxt.halo)
        with _timed(f"pool{li}", "maxpool2_fwd"):
            check(f.lib.yolo_maxpool2_fwd(ctypes.byref(pd), cur.p, nxt.p, f.st), "maxpool")
        f.cur = nxt
        return 1

    def _fwd_flatten(self, f, li: int) -> int:
        cur = f.cur
        if not f.train and isinstance(cur, Act) and cur.halo == 0 and cur.halo_hi == 0 and self.c.FLATTEN_FREE:
            f.hwc = (cur.C, cur.H * cur.W)            # the next Linear layer takes (hw, c)-ordered panels
            f.cur = cur.t.view(f.N, -1)
            return 1
        nxt = f.ws["acts"][li]
        check(f.lib.yolo_nhwc_bf16_to_nchw_bf16(cur.p, f.N, cur.C, cur.H, cur.W, cur.halo, ptr(nxt), f.st), "flatten")
        f.cur = nxt
        return 1

    def _fwd_fc(self, f, li: int) -> int:
        L, N, dev, L_, st = self.layers[li], f.N, f.dev, f.lib, f.st
        self.params_ready.wait(dev)      # yolo.optim.Adam(overlap): the Linear layers' update of the last step runs on a second stream
        if f.train:
            wf, _ = self._pack(li, False)
        else:
            wf = self._pack_fc_blocked(li, f.hwc)
            f.hwc = None
        xin = f.cur  # (N, K) bf16
        K = L.Cin
        d = rows_desc(N, xin.shape[1], K, L.Cout)
        d.slope, d.out_fp32 = self.SLOPE, 1
        d.w_blocked = 0 if f.train else 1
        last = (li == len(self.layers) - 1)
        nk = K // 64
        # blocked panels (inference) run the 3-stage weight-stream kernel: 32 co-tiles x 32 splits = two full rounds of 512 slots
        splits = max(1, min(32 if d.w_blocked else 48, nk // 16)) if K >= 4096 else 1
        b = L.bias.detach()
        if splits > 1:
            # every K split STORES its partial [N][Cout] result as a slab; the finishing pass adds the slabs in fixed
            # order -> the forward is bit-reproducible (fp32 atomics of 32 splits were not) and needs no zero fill
            acc = RT._splitk_scratch(splits * N * L.Cout, zero=False)
            d.epilogue, d.split_k, d.split_slabs = EPI_NONE, splits, 1
            with _timed(f"fc{li}", "igemm", 2.0 * N * L.Cout * L.Cin):
                _igemm(L_, d, ptr(xin), ptr(wf), None, None, ptr(acc), st, f"igemm fc{li}")
            yb = torch.empty((N, L.Cout), dtype=torch.bfloat16, device=dev) if not last else None
            yf = torch.empty((N, L.Cout), dtype=torch.float32, device=dev) if last else None
            check(L_.yolo_bias_lrelu_rows_slabs(ptr(acc), splits, ptr(b), N, L.Cout, self.SLOPE if L.lrelu else 1.0, ptr(yb), ptr(yf), st),
                  "bias_lrelu_rows")
        else:
            yf = torch.empty((N, L.Cout), dtype=torch.float32, device=dev)
            d.epilogue, d.split_k = (EPI_BIAS_LRELU if L.lrelu else EPI_BIAS), 1
            with _timed(f"fc{li}", "igemm", 2.0 * N * L.Cout * L.Cin):
                _igemm(L_, d, ptr(xin), ptr(wf), ptr(b), None, ptr(yf), st, f"igemm fc{li}")
            yb = None
            if not last:
                yb = torch.empty((N, L.Cout), dtype=torch.bfloat16, device=dev)
                check(L_.yolo_cast_f32_to_bf16(ptr(yf), yf.numel(), ptr(yb), st), "cast")
        mask = None
        if L.drop_mod is not None:
            L.dropout = float(L.drop_mod.p)          # (the backward of this forward reads L.dropout)
        f.cur = yb
        if not last and L.dropout > 0 and f.drop_training:
            mask = (torch.rand((N, L.Cout), device=dev) >= L.dropout).to(torch.uint8)
            f.cur = torch.empty_like(yb)
            check(L_.yolo_dropout_bf16(ptr(yb), ptr(mask), 1.0 / max(1.0 - L.dropout, 1e-12) if L.dropout < 1.0 else 0.0, yb.numel(), ptr(f.cur), st), "dropout")
        f.fc_saved[li] = (xin, yb, mask)
        if last:
            f.out = yf
        return 1

    # ------------------------------------------------------------------ backward
    @staticmethod
    def _codes(ws, li: int, pooled: Act) -> torch.Tensor:
        """arg-max codes of the pool behind conv layer li: uint16 per (pooled pixel, 8 channels), indexed like the pooled map / 8"""
        c = ws["misc"].get(("codes", li))
        if c is None:
            c = torch.empty(pooled.t.numel() // 8, dtype=torch.int16, device=pooled.t.device)
            ws["misc"][("codes", li)] = c
        ws["codes"].add(li)
        return c

    @staticmethod
    def _misc(ws, key, make):
        """a buffer of the workspace that the first pass needing it allocates"""
        buf = ws["misc"].get(key)
        if buf is None:
            buf = ws["misc"][key] = make()
        return buf

    def _grad_buf(self, ws, li: int, N, dev) -> Act:
        """gradient wrt the (post-activation-derivative) output of conv layer li, in the geometry
        yolo_wgrad's flat indexing needs (= the layer's INPUT geometry; zero-stuffed for stride 2)."""
        g = ws["grads"].get(li)
        if g is None:
            L = self.layers[li]
            if L.stride == 1 or L.first:
                g = Act(N, L.Hout, L.Wout, L.Cout, 1, dev)
            else:
                g = Act(N, L.Hin, L.Win, L.Cout, 1, dev)
            ws["grads"][li] = g
        return g

    @staticmethod
    def _wgrad_desc(L: Layer, g: Act, xin: Act, N: int) -> WgradDesc:
        """yolo_wgrad problem of conv layer L over N images of the gradient buffer g / the input buffer xin"""
        # kernel variant: the 256 x 256 pipelined kernel (5) on the big deep layers, where the in-process A/B measured it 10-19 %
        # faster (56x56 256 -> 512, 28x28 512 -> 1024, 14x14 1024 -> 1024: tools/time_wgrad.py); the 128 x 128 kernel (0) elsewhere
        px = N * L.Hout * L.Wout
        deep = (L.Cout >= 512 and L.Cin >= 256 and px >= 40000) or (L.Cout >= 1024 and L.Cin >= 1024 and px >= 12000)
        variant = 5 if (CFG.WGRAD_PIPE and L.K == 3 and L.stride == 1 and deep) else 0
        flat = False
        if CFG.WGRAD_PIPE and CFG.WGRAD_WIDE and L.K == 3 and L.stride == 1:
            # variant 6 (tools/time_wgrad.py, each launch alone, same box): 56x56 256 -> 512 0.542 -> 0.484 ms, 28x28 512 -> 1024 0.499 -> 0.488,
            # 112x112 64 -> 192 (four taps per 256-column tile) 0.360 (128 x 128 kernel) -> 0.303; NOT on 14x14 1024 -> 1024 (0.297 vs 0.287).
            # From 56x56 up it reduces over every slot of the zero-haloed buffer (<= 7 % more pixels) and saves the pixel -> slot arithmetic.
            if (deep and L.Cin < 1024) or (L.Cin == 64 and L.Cout >= 192 and px >= 500000):
                variant = 6
                flat = L.Hout >= 56 and L.Wout >= 56
        geo_ok = L.Hout >= 2 and L.Wout >= 2
        geo = variant >= 5 or (geo_ok and (L.stride > 1 or g.Hp * g.Wp >= 1.12 * L.Hout * L.Wout))
        choice = CFG.WGRAD_CHOICE.get((N, L.Hout, L.Wout, L.Cout, L.Cin, L.K, L.stride)) if CFG.WGRAD_CHOICE else None
        if choice is not None and L.K == 3 and L.stride == 1 and CFG.WGRAD_PIPE and (int(choice[0]) != 6 or CFG.WGRAD_WIDE):
            # a choice measured inside the training step (tools/search_wgrad.py): which kernel, and whether it walks every slot of the zero-haloed buffer
            variant, flat = int(choice[0]), bool(choice[1])
            geo = geo_ok and not flat
        if not flat and geo:
            return WgradDesc(N * L.Hout * L.Wout, g.px_stride, xin.px_stride, L.Cout, L.Cin, L.K, L.K, L.pad, xin.row_stride, 0, 0, variant,
                             L.Wout, L.Hout, g.Hp * g.Wp, g.Wp * L.stride, L.stride, g.halo * g.Wp + g.halo)
        return WgradDesc(N * g.Hp * g.Wp, g.px_stride, xin.px_stride, L.Cout, L.Cin, L.K, L.K, L.pad, xin.row_stride, 0, 0, variant)

    def backward(self, saved, gout: torch.Tensor, need_gx: bool):
        """gout: gradient of the plan output (same shape as forward's out).  Returns (gx or None, [param grads])."""
        b = _Backward(self, saved, need_gx)
        gout = f32(gout)
        with b.on_side():
            b.scratch.zero_()
        li = len(self.layers) - 1
        self._bwd_seed(b, li, gout)
        step = {"fc": self._bwd_fc, "pool": self._bwd_pool, "conv": self._bwd_conv}
        while li >= 0:
            if li == 0 and self.layers[0].kind == "flatten":
                break             # a plan that starts with nn.Flatten (a pooled 1 x 1 map into a Linear layer): b.g_flat is the input's gradient already
            assert self.layers[li].kind != "flatten", "nn.Flatten is handled together with the Linear layer behind it"
            li -= step[self.layers[li].kind](b, li)       # (the Linear behind nn.Flatten consumes both)
        return self._finish_backward(b)

    def _bwd_seed(self, b, li: int, gout: torch.Tensor):
        """the gradient flowing into the last layer li: b.g_flat, fp32 (N, K) rows wrt an fc layer's output, or b.g_act, an Act wrt a conv / pool
        output (already through LeakyReLU')"""
        L, N, dev = self.layers[li], b.N, b.dev
        if L.kind == "fc":
            b.g_flat = gout.reshape(N, -1)
            return
        # plan ends with feature maps (NCHW fp32 gradient): last layer is a conv(+lrelu) or a pool
        y = b.ws["acts"][li]
        graw = Act(N, y.H, y.W, y.C, 1, dev)
        check(b.lib.yolo_nchw_f32_to_nhwc_bf16(ptr(gout), N, y.C, y.H, y.W, graw.p, y.C, 1, 1, b.st), "gout->nhwc")
        if L.kind == "conv":
            b.g_act = self._grad_buf(b.ws, li, N, dev)
            self._apply_dlrelu_into(graw, y, L, b.g_act, b.st)
        else:
            assert L.kind == "pool", "plans end with fc, conv or pool"
            b.g_act = graw

    def _bwd_fc(self, b, li: int) -> int:
        L, N, dev, L_, st, det = self.layers[li], b.N, b.dev, b.lib, b.st, b.det
        xin, y_act, mask = b.fc_saved[li]
        last = (li == len(self.layers) - 1)
        ldg = _round_up(L.Cout, 32)
        gb = torch.empty((N, ldg), dtype=torch.bfloat16, device=dev)
        # through dropout + LeakyReLU of THIS layer's output (none for the last layer)
        check(L_.yolo_scale_rows_to_bf16(ptr(b.g_flat), ptr(mask), ((1.0 / (1.0 - L.dropout)) if L.dropout < 1.0 else 0.0) if mask is not None else 1.0,
                                         ptr(y_act) if (L.lrelu and not last) else None, self.SLOPE, N, L.Cout, ldg, ptr(gb), st), "scale_rows")
        # weight / bias gradient, native [O][K] layout
        fact = self._fc_factored(L)
        dw, db = b.grad_tensors(li, want_dw=not fact)
        wd = WgradDesc(N, ldg, L.Cin, L.Cout, L.Cin, 1, 1, 0, 0, 1, 0)
        nsq = None
        if fact:
            # no dw: the optimizer rebuilds it from (gb, xin) inside its update kernel.  The bias gradient still runs (dw == NULL: a column sum of gb).
            if N > _hip.FC_MAX_ROWS:
                raise _hip.HipUnsupported(f"EngineConfig.FC_FACTORED: batch {N} exceeds the {_hip.FC_MAX_ROWS} factor rows the update kernels take")
            nch = (L.Cout + 7) // 8
            if det and N // ((256 // min(nch, 256)) * 32) > 2:
                raise NotImplementedError(f"EngineConfig.DETERMINISTIC with EngineConfig.FC_FACTORED at batch {N}: the bias-only yolo_wgrad launch adds more "
                                          "than two row ranges with atomics there")
            # the record owns its factors: xin is the workspace's flatten buffer, rewritten by the next forward while a background update may still read it
            self.fc_factors[id(L.weight)] = FcFactors(gb, xin.clone(), N, 1.0)
            L.weight._fc_factored_plan = weakref.ref(self)
        elif det:
            pass      # the norm hint ends in one fp64 atomic per workgroup: the optimizer's order-fixed pass reads this gradient instead
        elif L.Cout * L.Cin >= self.c.FC_NORM_IN_WGRAD and L.Cin % 4 == 0:
            # the kernel that stores this gradient also sums its squares: the optimizer's global-norm pass (clip_grad_norm_) then
            # need not read the 822 MB of the Linear behind nn.Flatten again (yolo.optim.grad_norm_sq, `known`)
            nsq = torch.zeros((), dtype=torch.float64, device=dev)
            wd.dw_sumsq = nsq.data_ptr()
        # HBM-bound both: the weight gradient of the Linear behind nn.Flatten STORES 822 MB (4.1 TB/s alone), its data gradient READS
        # the 411 MB of weights (2.7 TB/s alone); side by side they share the memory system instead of taking turns
        side = self.c.FC_WGRAD_SIDE and b.side_t is not None
        if side:
            b.fc_keep.append(gb)          # (a temporary of the main stream's allocator that the second stream reads: alive until the streams join)
        with b.on_side(side) as wst:
            if det and not fact:
                _attach_wgrad_slabs(L_, wd, dev, wst)
            with _timed(f"fc{li}.wgrad", "wgrad", 2.0 * N * L.Cout * (1 if fact else L.Cin)):
                check(L_.yolo_wgrad(ctypes.byref(wd), ptr(xin), ptr(gb), ptr(dw), ptr(db), wst), f"wgrad fc{li}")
            self._layer_done(li)
        if nsq is not None:
            # (no reference to dw itself: autograd takes the gradient over without a copy only while nobody else holds it)
            self.grad_norm_sq[id(L.weight)] = ((dw.data_ptr(), tuple(dw.shape)), dw._version, nsq)
        b.grads[li] = (dw, db)
        # data gradient
        if li == 0 and not b.need_gx:
            return 1
        if li >= 2 and self.layers[li - 1].kind == "flatten" and self.layers[li - 2].kind in ("conv", "pool"):
            # the Linear behind nn.Flatten (205 M weights): reduce over the OUTPUT features with the
            # weight-gradient kernel -- both operands are strided along the reduction axis there, which
            # is exactly how W[o][k] and g^T[o][n] lie in memory -- and read the forward bf16 copy of W:
            #   dxT[k][n] = sum_o W[o][k] * gT[o][n]
            Lc = self.layers[li - 2]
            y = b.ws["acts"][li - 2]
            wf, _ = self._pack(li, False)
            ldn = _round_up(N, 8)
            gT = torch.zeros((L.Cout, ldn), dtype=torch.bfloat16, device=dev)
            check(L_.yolo_transpose_bf16(ptr(gb), N, L.Cout, ldg, ptr(gT), ldn, st), "transpose g")
            dxT = torch.zeros((L.Cin, N), dtype=torch.float32, device=dev)
            wd = WgradDesc(L.Cout, L.Cin, ldn, L.Cin, N, 1, 1, 0, 0, 0, 1)   # split 0: library's schedule (0.095 vs 0.135 ms with 3 ranges)
            if det:
                wd.accumulate = 0       # (dxT is zero: the same value) the pixel ranges of a tile as slabs, on this stream's own scratch
                _attach_wgrad_slabs(L_, wd, dev, st)
            with _timed(f"fc{li}.dgrad", "wgrad", 2.0 * N * L.Cout * L.Cin):
                check(L_.yolo_wgrad(ctypes.byref(wd), ptr(gT), ptr(wf), ptr(dxT), None, st), f"dgrad fc{li}")
            if Lc.kind == "conv":
                assert Lc.stride == 1, "nn.Flatten is expected after a stride-1 conv or a pool"
                g = self._grad_buf(b.ws, li - 2, N, dev)
                yact = y.p if Lc.lrelu else None
            else:
                g = self._misc(b.ws, "graw_flat", lambda: Act(N, y.H, y.W, y.C, 1, dev))
                yact = None
            check(L_.yolo_fc_dgrad_to_nhwc(ptr(dxT), N, y.C, y.H, y.W, 1, yact, self.SLOPE, g.p, st), "fc_dgrad_to_nhwc")
            b.g_act, b.g_flat = g, None
            return 2          # nn.Flatten is done as well
        _, wt = self._pack(li, True)
        d = rows_desc(N, ldg, ldg, L.Cin)
        d.epilogue, d.slope, d.out_fp32, d.split_k = EPI_NONE, self.SLOPE, 1, 1
        b.g_flat = torch.empty((N, L.Cin), dtype=torch.float32, device=dev)
        with _timed(f"fc{li}.dgrad", "igemm", 2.0 * N * L.Cout * L.Cin):
            _igemm(L_, d, ptr(gb), ptr(wt), None, None, ptr(b.g_flat), st, f"dgrad fc{li}")
        return 1

    def _bwd_pool(self, b, li: int) -> int:
        """b.g_act = gradient wrt the pooled output -> gradient wrt the conv in front (through its LeakyReLU)"""
        lc, ws, g_act = li - 1, b.ws, b.g_act
        Lc = self.layers[lc]
        assert Lc.kind == "conv" and Lc.lrelu, "MaxPool2d is expected right after conv+LeakyReLU"
        if lc == 0 and self.c.STEM_POOL_BWD_FUSED and self._stem_ok(Lc) and g_act.halo == 1 and not b.need_gx:
            # the stem's weight-gradient kernel rebuilds this pool's (+ LeakyReLU's) backward per tile from the activation and the pooled
            # gradient: the 224x224x64 gradient buffer is never written or read (a gradient wrt the input image needs it as a tensor)
            b.stem_dpool = g_act
            return 1
        yfull = ws["acts"][lc]
        g = self._grad_buf(ws, lc, b.N, b.dev)
        pd = PoolDesc(b.N, yfull.H, yfull.W, yfull.C, 1, 1)
        with _timed(f"pool{li}.bwd", "maxpool2_bwd"):
            if lc in ws.get("codes", ()):
                ypool = ws["acts"][li]
                assert (ypool.Hp, ypool.Wp, ypool.C, ypool.halo) == (g_act.Hp, g_act.Wp, g_act.C, g_act.halo)
                check(b.lib.yolo_maxpool2_bwd_codes(ctypes.byref(pd), ypool.p, ptr(ws["misc"][("codes", lc)]), g_act.p, self.SLOPE, g.p, b.st), "maxpool_bwd_codes")
            else:
                check(b.lib.yolo_maxpool2_bwd_lrelu(ctypes.byref(pd), yfull.p, g_act.p, self.SLOPE, g.p, b.st), "maxpool_bwd")
        b.g_act = g
        return 1

    def _bwd_conv(self, b, li: int) -> int:
        # The data gradients form the chain every later layer waits for; a layer's weight gradient only needs that layer's output
        # gradient and is first read by the optimizer.  The conv weight gradients (and their unpack passes / gradient-ready
        # callbacks) therefore go to a second stream: their atomic epilogues, partial last rounds and prologues -- phases in which a
        # kernel leaves the matrix cores idle -- overlap with the data-gradient kernels of the layers below, workgroup by workgroup.
        g = b.g_act        # dZ of this layer, flat-geometry buffer
        self._bwd_conv_wgrad(b, li, g)
        if li > 0:
            self._bwd_conv_dgrad(b, li, g)
        return 1

    def _bwd_conv_wgrad(self, b, li: int, g: Act):
        """weight + bias gradient of conv layer li on the second stream: the stem's direct kernels, its im2col fallback, or yolo_wgrad into the packed
        scratch (unpacked to OIHW later, several layers per launch: b.flush)"""
        L, N, dev, ws, L_ = self.layers[li], b.N, b.dev, b.ws, b.lib
        xin = ws["in"] if li == 0 else ws["acts"][li - 1]
        dw, db = b.grads[li] = b.grad_tensors(li)
        o = b.offs[("w", li)]
        with b.on_side() as wst:
            if self._stem_ok(L):
                self._bwd_stem_wgrad(b, L, g, xin, dw, db, wst)
                b.flush()
                self._layer_done(li)
                return
            if L.first:
                xcol = self._misc(ws, "xcol", lambda: Act(N, L.Hout, L.Wout, 7 * 32, 1, dev))
                check(L_.yolo_im2col_rows(xin.p, xin.img_stride, xin.row_stride, xin.px_stride, 2, 7, 32, N, L.Hout, L.Wout, 1, xcol.p, wst), "im2col_rows")
                dwp = b.scratch[o: o + L.Cout * 7 * 8 * 4]
                wd = WgradDesc(g.slots, g.px_stride, xcol.px_stride, L.Cout, 7 * 32, 1, 1, 0, xcol.row_stride, max(1, min(1024, g.slots // 4096)), 0)
                slabs, xp, macs = b.det, xcol.p, 147
            else:
                dwp = b.scratch[o: o + L.Cout * L.K * L.K * L.Cin]
                # reduce over the layer's OUTPUT pixels only (not over every slot of the zero-haloed -- for stride 2
                # zero-stuffed -- gradient buffer, whose geometry the input buffer shares slot for slot)
                # (measured: worth it from 28x28 down and for stride 2; at 56x56 and above the halo is < 8 % of the slots
                # and the per-row coordinate arithmetic costs more than it saves)
                wd = self._wgrad_desc(L, g, xin, N)
                slabs, xp, macs = b.det or (self.c.WGRAD_SLABS and wd.variant >= 5), xin.p, L.Cin * L.K * L.K
            if slabs:
                _attach_wgrad_slabs(L_, wd, dev, wst)
            with _timed(f"conv{li}.wgrad", "wgrad", 2.0 * N * L.Hout * L.Wout * L.Cout * macs):
                check(L_.yolo_wgrad(ctypes.byref(wd), xp, g.p, ptr(dwp), ptr(db), wst), f"wgrad conv{li}")
            b.pending.append((li, L, dwp, dw))
            if li == 0 or sum(t[2].numel() for t in b.pending) >= (16 << 20):
                b.flush()

    def _bwd_stem_wgrad(self, b, L: Layer, g: Act, xin: Act, dw, db, wst):
        """the stem's direct weight-gradient kernel; with b.stem_dpool (the pooled gradient) it rebuilds the pool's and LeakyReLU's backward per tile,
        from the arg-max codes or from the un-pooled activation"""
        N, ws, L_, dp = b.N, b.ws, b.lib, b.stem_dpool
        part = self._misc(ws, "stem_part", lambda: torch.empty((768 * 14400,), dtype=torch.float32, device=b.dev))
        slope = self.SLOPE if L.lrelu else 1.0
        with _timed("conv0.wgrad", "wgrad", 2.0 * N * L.Hout * L.Wout * L.Cout * 147):
            if dp is not None and 0 in ws.get("codes", ()):
                yp = ws["acts"][1]
                assert (yp.Hp, yp.Wp, yp.C, yp.halo) == (dp.Hp, dp.Wp, dp.C, dp.halo)
                check(L_.yolo_wgrad_stem7_codes(xin.p, yp.p, ptr(ws["misc"][("codes", 0)]), N, L.Hout, L.Wout, xin.img_stride, xin.row_stride,
                                                dp.p, dp.img_stride, dp.row_stride, dp.interior_off(), slope, ptr(dw), ptr(db), ptr(part), part.numel(), wst),
                      "wgrad_stem7_codes")
            elif dp is not None:
                yf = ws["acts"][0]
                check(L_.yolo_wgrad_stem7_pooled(xin.p, yf.p, N, L.Hout, L.Wout, xin.img_stride, xin.row_stride, yf.img_stride, yf.row_stride,
                                                 yf.interior_off(), dp.p, dp.img_stride, dp.row_stride, dp.interior_off(), slope, ptr(dw), ptr(db), ptr(part),
                                                 part.numel(), wst), "wgrad_stem7_pooled")
            else:
                check(L_.yolo_wgrad_stem7(xin.p, g.p, N, L.Hout, L.Wout, xin.img_stride, xin.row_stride, g.img_stride, g.row_stride,
                                          g.interior_off(), ptr(dw), ptr(db), ptr(part), part.numel(), wst), "wgrad_stem7")

    def _bwd_conv_dgrad(self, b, li: int, g: Act):
        """gradient wrt the output of layer li - 1 (through its LeakyReLU), or wrt the pooled map if a MaxPool2d is in front"""
        L, prev, N, dev, ws, st = self.layers[li], self.layers[li - 1], b.N, b.dev, b.ws, b.st
        _, wdg = self._pack(li, True)
        flops = 2.0 * N * L.Hout * L.Wout * L.Cout * L.Cin * L.K * L.K
        if prev.kind == "pool":
            gp = self._misc(ws, ("gpool", li), lambda: Act(N, L.Hin, L.Win, L.Cin, 1, dev))
            yprev = None
        elif prev.kind == "conv":
            gp = self._grad_buf(ws, li - 1, N, dev)
            yprev = ws["acts"][li - 1] if prev.lrelu else None
        else:
            raise AssertionError("conv after flatten/fc")
        if (prev.kind == "conv" and self.c.STRIDE2_CLASSES and L.stride == 2 and L.K == 3 and L.pad == 1 and prev.stride == 1
                and L.Hin % 2 == 0 and L.Win % 2 == 0):
            # stride-2 3x3 conv: the gradient buffer g holds dy zero-stuffed to the input grid, and the plain data gradient
            # spends 3/4 of its MACs on those zeros.  By input-pixel parity (py, px) only the taps ky = 1 (py even) or
            # ky = 2, 0 (py odd; likewise kx) contribute: four small convs over the NON-ZERO slots (doubled input strides)
            # with 1, 2, 2 and 4 taps -- 9 taps per 2x2 input pixels instead of 36 -- each writing its parity class of the
            # previous layer's gradient (doubled output strides).
            with _timed(f"conv{li}.dgrad", "igemm", flops):
                for (py, px), wc in self._stride2_panels(li, wdg).items():
                    dc = igemm_desc(N, L.Hin // 2, L.Win // 2, 1, 1 + py, 1 + px, L.Cout, L.Cin, g, g.interior_off(), gp, 2, 2, py, px)
                    dc.slope, dc.split_k, dc.tile_hint = self.SLOPE, 1, self.c.TILE_HINT
                    dc.epilogue = EPI_NONE
                    if yprev is not None:
                        dc.epilogue = EPI_MUL_DLRELU
                        desc_aux(dc, yprev, 2, py, px)
                    igemm_call(dc, g.p, ptr(wc), None, yprev.p if yprev is not None else None, gp.p, st, f"dgrad conv{li} class {py}{px}")
        else:
            # the previous layer's gradient buffer has ITS input geometry: zero-stuffed if that layer has stride 2
            d = self._dgrad_desc(L, g, N, gp, 2 if (prev.kind == "conv" and prev.stride != 1 and not prev.first) else 1)
            d.tile_hint = self.c.TILE_HINT
            d.epilogue = EPI_NONE
            if yprev is not None:
                d.epilogue = EPI_MUL_DLRELU
                desc_aux(d, yprev)
            with _timed(f"conv{li}.dgrad", "igemm", flops):
                igemm_call(d, g.p, ptr(wdg), None, yprev.p if yprev is not None else None, gp.p, st, f"dgrad conv{li}")
        b.g_act = gp

    def _finish_backward(self, b):
        """join the streams, the gradient wrt the plan's input if asked for, the workspace back to its pool, gradients to the arena's owner or to autograd"""
        L = self.layers[0]
        assert L.kind in ("conv", "flatten"), "plans start with a conv layer or with nn.Flatten"
        if b.side_t is not None:
            b.main_t.wait_stream(b.side_t)       # every weight gradient is final before anything that follows the backward pass
            if self.arena is not None and self.on_stream_wait is not None:
                self.on_stream_wait(b.main_t.cuda_stream, b.side_t.cuda_stream)
        gx = None
        if b.need_gx and L.kind == "flatten":
            a = b.ws["in"]            # nn.Flatten keeps the NCHW order of the plan's fp32 input: the rows of the Linear layer's data gradient are that tensor
            gx = b.g_flat.view(b.N, a.C, a.H, a.W)
        elif b.need_gx:
            gx = (self._stem_dgrad if L.first else self._dgrad_to_input)(0, b.g_act, b.N, b.dev, b.st)
        if self.debug_keep:
            self.last = (b.ws, b.fc_saved)
        else:
            self._release(b.key, b.ws)
        grads = b.grads
        if self.arena is None:
            return gx, [grads[i][j] for i in sorted(grads) for j in (0, 1)]
        if self.on_backward_done is not None:
            self.on_backward_done()
        for i in grads:          # hand the views to the optimizer without going through autograd
            L2 = self.layers[i]
            if L2.weight.grad is not grads[i][0]:
                L2.weight.grad = grads[i][0]
            if L2.bias.grad is not grads[i][1]:
                L2.bias.grad = grads[i][1]
        return gx, [None] * (2 * len(grads))

    def _apply_dlrelu_into(self, graw: Act, y: Act, L: Layer, g: Act, st):
        """g(interior, possibly zero-stuffed) = graw * lrelu'(y) -- used only at plan ends (rare path)."""
        gi = graw.interior().float()
        if L.lrelu:
            gi = gi * torch.where(y.interior().float() > 0, 1.0, self.SLOPE)
        gi = gi.to(torch.bfloat16)
        if L.stride == 1 or L.first:
            g.interior().copy_(gi)
        else:
            g.interior()[:, 0::2, 0::2, :][:, : gi.shape[1], : gi.shape[2], :].copy_(gi)

    def _stem_dgrad(self, li, g: Act, N, dev, st):
        """gradient wrt the input IMAGE through the 7x7 / stride-2 / pad-3 stem (the reference back-propagates to x in
        tests/test_backbone.py:187-196; training never asks for it, so the step's FLOP count skips this product).  By the parity
        (py, px) of the image pixel (y, x) = (2a + py, 2b + px) only the taps ky = py + 5 - 2 ty (ty = 0 .. 2 + py; likewise kx) meet an
        output pixel, (a + ty - 1, b + tx - 1): four stride-1 correlations over the stem's output gradient g with 3x3, 3x4, 4x3 and 4x4
        taps of 64 channels, each writing its parity class of the image (doubled output strides) -- the scheme of the stride-2 3x3
        layers' data gradient.  The three image channels ride in an 8-channel fp32 NHWC scratch; rows / columns a + 2 past the map fall
        on the zero halo of the next row / image (or the guard band)."""
        L = self.layers[li]
        assert L.first and L.K == 7 and L.stride == 2 and L.pad == 3 and g.halo == 1 and g.C == L.Cout and L.Cout % 64 == 0
        H, W = 2 * L.Hout, 2 * L.Wout
        w = L.weight.detach().float()                                   # [Cout][3][7][7]
        buf = torch.empty((N, H, W, 8), dtype=torch.float32, device=dev)
        L_ = RT.lib()
        for py in (0, 1):
            for px in (0, 1):
                kys = [py + 5 - 2 * t for t in range(3 + py)]
                kxs = [px + 5 - 2 * t for t in range(3 + px)]
                panel = torch.zeros((8, len(kys), len(kxs), L.Cout), dtype=torch.bfloat16, device=dev)
                panel[:3] = w[:, :, kys][:, :, :, kxs].permute(1, 2, 3, 0).to(torch.bfloat16)      # [c][ty][tx][co]
                d = igemm_desc(N, L.Hout, L.Wout, 1, len(kys), len(kxs), L.Cout, 8, g, g.interior_off(1))
                d.out_img_stride, d.out_row_stride, d.out_px_stride, d.out_off = H * W * 8, 2 * W * 8, 16, (py * W + px) * 8     # (a plain tensor, not an Act)
                d.epilogue, d.slope, d.out_fp32, d.split_k, d.tile_hint = EPI_NONE, self.SLOPE, 1, 1, 4      # 64 x 128 tiles: 8 "channels"
                _igemm(L_, d, g.p, ptr(panel), None, None, ptr(buf), st, f"stem dgrad class {py}{px}")
        return buf[..., :3].permute(0, 3, 1, 2).contiguous()

    def _dgrad_to_input(self, li, g: Act, N, dev, st):
        """data gradient of the first conv of a plan whose input is a feature map (DetectionHead)."""
        L = self.layers[li]
        _, wdg = self._pack(li, True)
        gi = Act(N, L.Hin, L.Win, L.Cin, 1, dev)
        d = self._dgrad_desc(L, g, N, gi)
        d.epilogue = EPI_NONE
        _igemm(RT.lib(), d, g.p, ptr(wdg), None, None, gi.p, st, "dgrad input")
        gx = torch.empty((N, L.Cin, L.Hin, L.Win), dtype=torch.float32, device=dev)
        check(RT.lib().yolo_nhwc_bf16_to_nchw_f32(gi.p, N, L.Cin, L.Hin, L.Win, 1, ptr(gx), st), "gx nhwc->nchw")
        return gx


class _Pass:
    """what the steps of one forward pass share: the workspace, the batch, the stream, and the activation flowing from layer to layer (``cur``)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Backward:
    """State of one backward pass: the workspace and batch of its forward, both streams, the scratch areas of the weight gradients, the gradients
    made so far, and the gradient flowing from layer to layer -- ``g_flat``, fp32 (N, K) rows in front of an fc layer, or ``g_act``, an Act wrt a
    conv / pool output (already through LeakyReLU')."""

    def __init__(self, plan: Plan, saved, need_gx: bool):
        self.plan, self.need_gx = plan, need_gx
        self.lib, self.st = RT.lib(), RT.stream()
        self.key, self.ws, self.fc_saved, self.N, self.dev = saved
        dev = self.dev
        plan._apply_geom(self.ws)
        if plan.arena is not None:
            plan.arena[plan._arena_w_end:].zero_()      # bias gradients are accumulated with atomics
        # two zero-filled fp32 scratch areas for the whole pass: the packed conv weight gradients (targets of yolo_wgrad's atomics; a buffer
        # of the workspace, cleared ON THE SIDE STREAM, where its first user runs: 80 MB of fill off the data-gradient chain) and,
        # without an arena, the bias gradients (fresh every pass: they are handed to autograd) -- two fills instead of ~50
        self.offs, tot, btot = {}, 0, 0
        for i, L in enumerate(plan.layers):
            if L.kind == "conv":
                self.offs[("w", i)] = tot
                tot += _round_up(L.Cout * 7 * 8 * 4 if L.first else L.Cout * L.K * L.K * L.Cin, 64)
            if L.kind in ("conv", "fc") and plan.arena is None:
                self.offs[("b", i)] = btot
                btot += _round_up(L.Cout, 64)
        self.scratch = self.ws["misc"].get("wgrad_scratch")
        if self.scratch is None or self.scratch.numel() < tot:
            self.scratch = self.ws["misc"]["wgrad_scratch"] = torch.empty(max(tot, 1), dtype=torch.float32, device=dev)
        self.bscratch = torch.zeros(max(btot, 1), dtype=torch.float32, device=dev)
        self.main_t = RT.STREAMS.current(dev)
        self.side_t = side_stream(dev) if plan.c.WGRAD_STREAM else None
        self.det = bool(plan.c.DETERMINISTIC)     # every yolo_wgrad launch with slabs (scratch per stream), no norm hint (EngineConfig.DETERMINISTIC)
        self.grads: dict[int, tuple] = {}
        self.pending: list[tuple] = []     # conv gradients waiting for their packed -> OIHW conversion
        self.fc_keep: list = []
        self.stem_dpool = None             # pooled gradient handed straight to the stem's weight-gradient kernel (pool backward fused there)
        self.g_flat = self.g_act = None

    def on_side(self, side: bool = True):
        """``with b.on_side() as st:`` -- the second stream, behind everything queued on the main one (the main stream itself without one / if not side)"""
        return _on_side_stream(self.main_t, self.side_t if side else None, self.plan.on_stream_wait if self.plan.arena is not None else None)

    def grad_tensors(self, i: int, want_dw: bool = True):
        """(dw, db) of layer i: the arena's views, or a fresh weight gradient and a slice of the zeroed bias scratch (dw None: a factored Linear layer)"""
        if self.plan.arena is not None:
            dw, db, _, _ = self.plan.arena_views[i]
            if want_dw != (dw is not None):
                raise RuntimeError("the gradient arena was attached with another EngineConfig.FC_FACTORED / FC_FACTORED_MIN than this backward pass runs with")
            return dw, db
        L = self.plan.layers[i]
        o = self.offs[("b", i)]
        return (torch.empty_like(L.weight, dtype=torch.float32) if want_dw else None), self.bscratch[o: o + L.Cout]

    def flush(self):
        """packed -> OIHW conversion of the finished conv gradients, several layers per launch (yolo_unpack_conv_wgrads_multi) on the current
        stream; the gradients are final (and announced) here"""
        plan, L_ = self.plan, self.lib
        items = [ConvUnpackItem(dwp.data_ptr(), dw.data_ptr(), L.Cout, L.Cin, L.K, L.K) for (i, L, dwp, dw) in self.pending if plan._multi_ok(L)]
        if items:
            check(L_.yolo_unpack_conv_wgrads_multi((ConvUnpackItem * len(items))(*items), len(items), RT.stream()), "unpack_conv_wgrads_multi")
        for (i, L, dwp, dw) in self.pending:
            if not plan._multi_ok(L):
                shape = (3, 7, 7, 4, 8) if L.first else (L.Cin, L.K, L.K, L.Cin, L.K)          # (the stem's panel: rows of 8 taps x 4 channels)
                check(L_.yolo_unpack_conv_wgrad(ptr(dwp), L.Cout, *shape, ptr(dw), 0, RT.stream()), "unpack")
            plan._layer_done(i)
        self.pending.clear()
