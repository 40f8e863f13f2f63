"""Optimizer step on the HIP kernels (optim.hip, sgd.hip): Adam or SGD with momentum + global-norm gradient clipping in one HBM pass.

``Adam`` takes the constructor arguments of ``torch.optim.Adam`` (the reference builds
``optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)``, src/train.py:177-179) and keeps the
same per-parameter state (``step``, ``exp_avg``, ``exp_avg_sq``), so optimizer ``state_dict``s are
interchangeable with the reference's checkpoints.  ``max_grad_norm`` folds
``clip_grad_norm_(params, max_norm)`` (trainer.py:79,93) into the same pass: the global norm is
reduced on the device and read by the update kernel, no host sync.

``SGD`` is ``torch.optim.SGD`` (the YOLOv1 paper's recipe: momentum 0.9, weight decay 5e-4) in the same slot, with the same
``max_grad_norm``, ``skip_if``, ``attach_plan`` and second-stream pass; what the two share lives in ``_Fused``.

``LARS`` (lars.hip) scales every tensor's regularised gradient by its trust ratio and hands it to SGD with momentum, for large effective
batches; its one norms pass per step also yields the clip norm.  ``lars_param_groups`` builds its two param groups.
"""

from __future__ import annotations

import torch

import ctypes
import os
import weakref

from . import _hip
from ._hip import MT_MAX, AccumTensor, AdamTensor, EmaTensor, SgdTensor, check, lib, ptr, stream
from .config import CONFIG as CFG
from .executor import fc_factors_of


BG_CUS = 128       # CUs the background update of the Linear layers holds (yolo_adam_step_multi_bg): a CU streams ~42 GB/s whatever it keeps in flight,
                   # so the pass runs at ~4.5 TB/s there -- under the conv stack of the next forward, whose persistent kernels draw their tiles from a
                   # queue and so lose only the share of the chip the pass holds.  Step at batch 64 (tools/ab_train.py, one process): 32 CUs 12.16 ms,
                   # 48: 11.20, 64: 11.02-11.10, 96: 10.92, 128: 10.89-10.99, 160: 11.06, 192: 11.17, 256: 11.37.  (Round 2, statically scheduled conv
                   # kernels: 64 was the optimum and 96 no better.)
EMA_BACKGROUND = True   # ModelEMA averages the parameters of a background update in the background too ("Weight EMA", has the step times)
OVERLAP = os.environ.get("YOLO_ADAM_OVERLAP", "1") != "0"     # attach_plan(overlap=True) takes effect (switch for A/B runs)


def _wait_before_state_io(waiter, module) -> None:
    """``module.state_dict()`` and ``module.load_state_dict()`` first make the current stream wait for ``waiter``'s background launch
    (``waiter.synchronize()``).  Once per module (``waiter._hooked``); the hooks hold the waiter weakly."""
    if id(module) in waiter._hooked:
        return
    waiter._hooked.add(id(module))
    me = weakref.ref(waiter)

    def wait(*_a, **_k):
        w = me()
        if w is not None:
            w.synchronize()
    module.register_state_dict_pre_hook(wait)
    module.register_load_state_dict_pre_hook(wait)


def _f32c(g: torch.Tensor) -> torch.Tensor:
    return g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()


def grad_norm_sq(params, known=None) -> torch.Tensor:
    """device double holding sum over all gradients of g^2 (enqueued, not synchronised): one launch
    for the whole list (yolo_sumsq_f32_multi).

    ``known``: {id(param): ((data_ptr, shape) of the gradient, its version counter, device double)} -- squared norms the producer of a gradient
    already has (engine.Plan.backward: yolo_wgrad sums the squares of the 205 M-element gradient of the Linear behind
    nn.Flatten while it stores it, yolo_wgrad_desc.dw_sumsq: 822 MB less to read).  An entry is used only while the parameter's
    .grad is still that very memory, unmodified (autograd hands over a detached alias that shares the version counter; accumulation,
    an all-reduce or clipping in place bump it)."""
    grads, extra = _split_known(params, known)
    dev = (grads[0] if grads else extra[0]).device
    if dev.type != "cuda":          # CPU parameters: stock torch ops (an explicit device choice, like the models' CPU path)
        acc = torch.zeros((), dtype=torch.float64)
        for g in grads:
            acc += g.double().pow(2).sum()
        for e in extra:
            acc += e
        return acc
    _hip.require_cuda(*grads)
    with torch.cuda.device(dev):
        acc = torch.zeros((), dtype=torch.float64, device=dev)
        if grads:
            gp = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
            gn = (ctypes.c_long * len(grads))(*[g.numel() for g in grads])
            if CFG.DETERMINISTIC:
                # workgroup partials into scratch slots + a fixed-order last stage: the double, and with it the clip coefficient of every
                # parameter, no longer depends on the order in which fp64 atomics arrived
                slots = ctypes.c_long(0)
                check(lib().yolo_sumsq_fixed_slots(gn, len(grads), ctypes.byref(slots)), "yolo_sumsq_fixed_slots")
                st = stream()
                scratch = _scratch("sumsq", dev, st, slots.value)
                check(lib().yolo_sumsq_f32_multi_fixed(gp, gn, len(grads), ptr(scratch), scratch.numel(), ptr(acc), st), "yolo_sumsq_f32_multi_fixed")
            else:
                check(lib().yolo_sumsq_f32_multi(gp, gn, len(grads), ptr(acc), stream()), "yolo_sumsq_f32_multi")
        for e in extra:
            acc += e
    return acc


_SCRATCH: dict = {}


def _scratch(what: str, dev, st, numel: int) -> torch.Tensor:
    """fp64 scratch ``what`` ("sumsq": the slots of the order-fixed norms; "lars": the 2 x count doubles yolo_lars_norms_multi stores), one per
    device and stream (launches of one stream use it one after the other), grown on demand"""
    key = (what, dev.index, st.value or 0)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < numel:
        if buf is not None:
            buf.record_stream(torch.cuda.current_stream(dev))
        buf = _SCRATCH[key] = torch.empty(max(numel, 1), dtype=torch.float64, device=dev)
    return buf


def _split_known(params, known):
    """(gradients whose squares must be summed, squared norms taken over from ``known``): an entry of ``known`` counts only while
    the parameter's .grad is still the very memory it was computed from, at the same version"""
    grads, extra = [], []
    for p in params:
        if p.grad is None:
            continue
        k = known.get(id(p)) if known else None
        if k is not None and k[0] == (p.grad.data_ptr(), tuple(p.grad.shape)) and k[1] == p.grad._version:
            extra.append(k[2])
        else:
            grads.append(_f32c(p.grad))
    return grads, extra


FC_FACTORED_REFUSED = ("EngineConfig.FC_FACTORED (--factored-fc) is not supported with {what}: the factored gradient of the big Linear layer is consumed by "
                       "the update kernels of yolo.optim.Adam / yolo.optim.SGD only")


def _plan_factored(plan) -> bool:
    cfg = getattr(plan, "c", None)          # (None: not an executor.Plan)
    return cfg is not None and bool(cfg.FC_FACTORED)


def fc_factored_sumsq(weight, rec, acc: torch.Tensor) -> None:
    """*acc += |G|^2 of the factored gradient ``rec`` of ``weight`` (yolo_fc_factored_sumsq: two Gram matrices, order-fixed, G is not formed),
    enqueued on the current stream"""
    d = rec.desc(weight)
    need = ctypes.c_long(0)
    check(lib().yolo_fc_factored_sumsq_slots(ctypes.byref(d), ctypes.byref(need)), "yolo_fc_factored_sumsq_slots")
    st = stream()
    scratch = _scratch("sumsq", acc.device, st, need.value)
    check(lib().yolo_fc_factored_sumsq(ctypes.byref(d), ptr(scratch), scratch.numel(), ptr(acc), st), "yolo_fc_factored_sumsq")


def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """HIP version of torch.nn.utils.clip_grad_norm_ (L2): returns the total norm as a device tensor."""
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.zeros(())
    acc = grad_norm_sq(params)
    with torch.cuda.device(acc.device):
        st = stream()
        for p in params:
            check(lib().yolo_clip_scale_f32(ptr(p.grad), p.grad.numel(), ptr(acc), float(max_norm), st), "yolo_clip_scale_f32")
    return acc.sqrt().float()


class _Fused(torch.optim.Optimizer):
    """What the fused optimizers share: the folded clip_grad_norm_ (``max_grad_norm``, with the attached plans' squared-norm hints), the
    device-side skip flag (``skip_if``), the bf16 shadows of the Linear layers and their background pass on a second stream
    (``attach_plan``, ``synchronize``), one multi-tensor launch per group of parameters.  A subclass supplies its state and table entry
    (``_entry``), its two launches (``_launch``) and the same step in stock torch ops for CPU parameters (``_step_on_cpu``)."""

    def __init__(self, params, defaults, max_grad_norm: float | None = None):
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.bf16_shadow: dict[int, tuple] = {}   # id(param) -> (bf16 tensor refreshed in the same pass, callback(param) | None)
        self.plans: list = []                     # attached engine plans: their backward passes leave squared gradient norms (grad_norm_sq)
        # attach_plan(plan, overlap=True): id(param) -> plan.  The update of these parameters (the Linear layers: 76 % of the model's
        # optimizer bytes, first used at the END of the next forward) runs as a background pass on BG_CUS CUs of a second stream
        # (yolo_adam_step_multi_bg / yolo_sgd_step_multi_bg) beside the next forward's conv stack; the plan's forward waits for it in front of its first
        # Linear layer.
        self.deferred: dict[int, object] = {}
        self._side = None
        self._pending = None                      # event behind the last background launch
        # device float (or None), consumed by the next step(): non-zero = the producer of the gradients found its input invalid and
        # the step must update nothing.  The training loop hands over YOLOLoss's error word (LossParts.device_flag), which the host
        # reads only after the step was enqueued -- the reference raises inside the loss forward, before any update
        self.skip_if = None
        self.last_skip = None                     # the skip_if the last step() consumed (None: it had none): ModelEMA.update hands it to its own launches
        self._hooked: set = set()                 # ids of the modules that carry this optimizer's state_dict / load_state_dict hooks

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        all_params = [p for g in self.param_groups for p in g["params"] if p.grad is not None or fc_factors_of(p)[0] is not None]
        if not all_params:
            return loss
        if all(not p.is_cuda for p in all_params):
            if CFG.FC_FACTORED:
                raise RuntimeError(FC_FACTORED_REFUSED.format(what="CPU parameters"))
            self._step_on_cpu(all_params)
            return loss
        _hip.require_cuda(*all_params)
        with torch.cuda.device(all_params[0].device):
            return self._step_on_device(all_params, loss)

    def _known_norms(self) -> dict:
        """squared gradient norms the attached plans' backward passes left (grad_norm_sq): one backward pass, one use"""
        known = {}
        for plan in self.plans:
            known.update(plan.grad_norm_sq)
            plan.grad_norm_sq.clear()
        return known

    def _begin_cpu_step(self, all_params, norm_sq=None):
        """the head of every ``_step_on_cpu``: drains the plans' norm hints, forms the global gradient norm (from ``norm_sq`` where the caller
        has the squared one already, else from the gradients and the hints) and consumes ``skip_if`` into ``last_skip``
        -> (the norm as a double tensor, None without ``max_grad_norm``; does the flag cancel the step?)"""
        known = self._known_norms()
        total = None
        if self.max_grad_norm is not None:
            total = (grad_norm_sq(all_params, known) if norm_sq is None else norm_sq).sqrt()
        skip, self.skip_if = self.skip_if, None
        self.last_skip = skip
        return total, skip is not None and float(skip) != 0.0

    def _sgd_step_on_cpu(self, total, trust=None):
        """SGD with momentum in stock torch ops, for SGD and LARS: the clip coefficient formed in fp32 as the kernels form it (clip_coefficient in
        csrc/multi_tensor.h, which is clip_grad_norm_'s), then torch.optim.SGD's own sequence of operations.  ``trust(group, p, g, clip)``: LARS's
        scaling of the clipped, regularised gradient ``g``"""
        clip = None
        if total is not None:
            clip = (torch.tensor(self.max_grad_norm, dtype=torch.float32) / (total.float() + torch.tensor(1e-6, dtype=torch.float32))).clamp(max=1.0)
        for group in self.param_groups:
            momentum, wd = group["momentum"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad.float()
                if clip is not None:
                    g = g * clip
                if wd != 0:
                    g = g.add(p, alpha=wd)
                if trust is not None:
                    g = trust(group, p, g, clip)
                if momentum != 0:
                    state = self.state[p]
                    buf = state.get("momentum_buffer")
                    if buf is None:
                        buf = state["momentum_buffer"] = g.clone()
                    else:
                        buf.mul_(momentum).add_(g, alpha=1 - group.get("dampening", 0))
                    g = g.add(buf, alpha=momentum) if group.get("nesterov", False) else buf
                p.add_(g, alpha=-group["lr"])

    def _momentum_buffer(self, group, p):
        """(momentum buffer or None, is this the parameter's first step?)"""
        buf, first = None, False
        if group["momentum"] != 0:
            state = self.state[p]
            buf = state.get("momentum_buffer")
            first = buf is None
            if first:
                buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()):
                raise RuntimeError(f"yolo.optim.{type(self).__name__} needs contiguous fp32 momentum buffers on the device")
        return buf, first

    def _clip_norm_sq(self, all_params):
        """device double with the global squared gradient norm the step launches clip by (None: no clipping), enqueued on the current stream in
        front of the first step launch"""
        if self.max_grad_norm is None:
            return None
        known = self._known_norms()
        dense = [p for p in all_params if p.grad is not None]
        acc = grad_norm_sq(dense, known) if dense else torch.zeros((), dtype=torch.float64, device=all_params[0].device)
        for p in all_params:
            # a factored gradient adds its |G|^2 from the Gram matrices of its factors: order-fixed with and without DETERMINISTIC
            rec, _ = fc_factors_of(p) if p.grad is None else (None, None)
            if rec is not None:
                fc_factored_sumsq(p, rec, acc)
        return acc

    def _enter_side(self, main_t, norm, skip, side_used: bool):
        """the second stream, behind the gradients, the norm and the last forward's / backward's reads (once per step)"""
        side = self._side_stream()
        if not side_used:
            side.wait_stream(main_t)
            if norm is not None:
                norm.record_stream(side)
            if skip is not None:
                skip.record_stream(side)
        return side

    def _factored_state(self, group, p):
        """the state of a parameter whose gradient is factored, created (and counted up) on the current stream before any launch of the step"""
        raise RuntimeError(FC_FACTORED_REFUSED.format(what=f"yolo.optim.{type(self).__name__}"))

    def _launch_factored(self, group, p, rec, shadow, fstate, norm, skip, side):
        raise RuntimeError(FC_FACTORED_REFUSED.format(what=f"yolo.optim.{type(self).__name__}"))

    def _step_on_device(self, all_params, loss):
        norm = self._clip_norm_sq(all_params)
        skip, self.skip_if = self.skip_if, None
        self.last_skip = skip
        if skip is not None:
            if not (skip.is_cuda and skip.dtype == torch.float32 and skip.numel() == 1):
                raise ValueError("skip_if must be one float32 on the device")
            _hip.require_cuda(all_params[0], skip)
        main_t = torch.cuda.current_stream()
        side_used = False
        for group in self.param_groups:
            # one launch per (group, key of the subclass, foreground / background): normally one for the conv stack and one for the Linear layers
            by_key: dict[tuple, list] = {}
            keep = []                      # temporaries the launch reads must outlive the enqueue
            factored = []                  # (p, record, its plan, shadow hook, background?, state) of the parameters whose gradient is a pair of factors
            for p in group["params"]:
                if p.grad is None:
                    rec, rplan = fc_factors_of(p)
                    if rec is not None:
                        if p.dtype != torch.float32 or not p.is_contiguous():
                            raise RuntimeError(f"yolo.optim.{type(self).__name__} needs contiguous fp32 parameters")
                        # (the state is created here, on the current stream and in front of the second stream's wait for it: the zero fill of a
                        # new state tensor must not run beside the background launch that writes it)
                        factored.append((p, rec, rplan, self.bf16_shadow.get(id(p)), OVERLAP and id(p) in self.deferred, self._factored_state(group, p)))
                    continue
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError(f"yolo.optim.{type(self).__name__} needs contiguous fp32 parameters")
                g = _f32c(p.grad)
                keep.append(g)
                hook = self.bf16_shadow.get(id(p))
                late = OVERLAP and id(p) in self.deferred
                if late:
                    g.record_stream(self._side_stream())     # read on the second stream after the caller may have dropped it
                key, entry = self._entry(group, p, g, hook[0] if hook is not None else None)
                by_key.setdefault((key, late), []).append((p, entry, hook))
            for (key, late), items in sorted(by_key.items(), key=lambda kv: kv[0][1]):      # the foreground launch first
                tab = (type(items[0][1]) * len(items))(*[it[1] for it in items])
                side = None
                if late and len(items) <= MT_MAX:
                    side = self._enter_side(main_t, norm, skip, side_used)
                    side_used = True
                self._launch(group, key, tab, len(items), norm, skip, side)
                for p, _, hook in items:
                    # the kernel updated p through a raw pointer: bump the autograd version so that the
                    # engine's packed bf16 copies notice (no memory traffic) ...
                    torch.autograd.graph.increment_version(p)
                    if hook is not None and hook[1] is not None:
                        hook[1](p)         # ... and tell the owner of a shadow that it is already current
            for p, rec, rplan, hook, late, fstate in factored:
                # one launch per factored parameter (yolo_*_step_factored), in the place of its row in the tables above: in the background on
                # BG_CUS persistent workgroups of the second stream where the parameter is deferred, else on the current stream
                side = None
                if late:
                    side = self._enter_side(main_t, norm, skip, side_used)
                    side_used = True
                    rec.dy.record_stream(side)               # the record's own tensors, dropped below: read on the second stream
                    rec.x.record_stream(side)
                self._launch_factored(group, p, rec, hook[0] if hook is not None else None, fstate, norm, skip, side)
                rplan.fc_factors.pop(id(p), None)            # one backward pass feeds one step
                torch.autograd.graph.increment_version(p)
                if hook is not None and hook[1] is not None:
                    hook[1](p)
        if side_used:
            ev = torch.cuda.Event()
            ev.record(self._side)
            self._pending = ev
            for plan in {id(pl): pl for pl in self.deferred.values()}.values():
                plan.params_ready.event = ev            # Plan.forward waits for it in front of its first Linear layer
        return loss

    def _side_stream(self):
        if self._side is None:
            self._side = _hip.side_stream(torch.device("cuda", torch.cuda.current_device()), low=False)
        return self._side

    def synchronize(self) -> None:
        """Make the CURRENT stream wait for a background update still running on the second stream (attach_plan(overlap=True)).
        The attached plan's forward does this by itself in front of its Linear layers; call it before reading those layers'
        parameters or the optimizer state in any other way.  Waiting by themselves: this optimizer's state_dict() / load_state_dict() /
        zero_grad(set_to_none=False), and the owning model's state_dict() / load_state_dict() / copy.deepcopy (hooks set by attach_plan)."""
        if self._pending is not None:
            torch.cuda.current_stream().wait_event(self._pending)
            self._pending = None
            for plan in self.deferred.values():
                plan.params_ready.event = None

    def _hook_owner(self, plan) -> None:
        """the module that owns ``plan`` waits for a background update by itself wherever torch reads or writes its parameters in
        bulk: ``state_dict()`` (checkpoints, ``torch.save(model.state_dict())``), ``load_state_dict()`` (resume) and
        ``copy.deepcopy`` (EMA copies; models.YOLOv1.__deepcopy__ asks the plan) -- no caller has to know about the second stream."""
        owner = plan.owner() if getattr(plan, "owner", None) is not None else None
        if owner is not None:
            _wait_before_state_io(self, owner)

    def state_dict(self):
        self.synchronize()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self.synchronize()
        return super().load_state_dict(state_dict)

    def zero_grad(self, set_to_none: bool = True):
        if not set_to_none:
            self.synchronize()             # zeroing in place would race with the background pass, which still reads the gradients
        return super().zero_grad(set_to_none=set_to_none)

    def attach_plan(self, plan, overlap: bool = False) -> None:
        """Let this optimizer refresh the engine's bf16 forward operands of Linear layers in the same
        pass that updates their fp32 masters (``plan``: ``model.hip_plan()``).

        ``overlap``: update the Linear layers as a background pass on a second stream, beside the next forward's conv stack (same
        floats; see ``synchronize`` for what then has to wait).  Worth 0.15 ms of the 11.9-ms YOLOv1 step (train.py, bench.py); behind the HBM-heavy ResNet trunk it loses."""
        for p, shadow, fresh in plan.bf16_shadows():
            self.bf16_shadow[id(p)] = (shadow, fresh)
            if overlap:
                self.deferred[id(p)] = plan
        if overlap:
            for b in plan.fc_biases():
                self.deferred[id(b)] = plan
            self._hook_owner(plan)
        if all(pl is not plan for pl in self.plans):
            self.plans.append(plan)


class Adam(_Fused):
    """torch.optim.Adam semantics (amsgrad=False, L2 weight decay) on yolo_adam_step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm: float | None = None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm)

    def _step_on_cpu(self, all_params):
        """CPU parameters (the reference's ``--device cpu`` runs, the gloo tests of the data-parallel path): the same step in stock
        torch ops -- clip coefficient min(1, max_norm / (|g| + 1e-6)) from the squared norms (incl. the plans' hints), then the
        arithmetic of adam1 in optim.hip, which is torch.optim.Adam's."""
        total, skipped = self._begin_cpu_step(all_params)
        if skipped:
            return
        clip = 1.0 if total is None else min(1.0, self.max_grad_norm / (float(total) + 1e-6))
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state, t = self._next_step(p)
                g = p.grad.float() * clip + group["weight_decay"] * p
                state["exp_avg"].lerp_(g, 1.0 - b1)
                state["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                denom = state["exp_avg_sq"].sqrt() / ((1.0 - b2 ** t) ** 0.5) + group["eps"]
                p.addcdiv_(state["exp_avg"], denom, value=-group["lr"] / (1.0 - b1 ** t))

    def _next_step(self, p):
        """the parameter's state, created at its first step, with ``step`` counted up -> (state, step)"""
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state["step"] += 1
        return state, int(state["step"].item())

    def _entry(self, group, p, g, shadow):
        state, step = self._next_step(p)
        return step, AdamTensor(p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(),
                                shadow.data_ptr() if shadow is not None else None, p.numel())

    def _factored_state(self, group, p):
        return self._next_step(p)

    def _launch_factored(self, group, p, rec, shadow, fstate, norm, skip, side):
        state, step = fstate
        b1, b2 = group["betas"]
        d = rec.desc(p)
        check(lib().yolo_adam_step_factored(ctypes.byref(d), ptr(p), ptr(state["exp_avg"]), ptr(state["exp_avg_sq"]), ptr(shadow), float(group["lr"]), float(b1),
                                            float(b2), float(group["eps"]), float(group["weight_decay"]), step, ptr(norm), float(self.max_grad_norm or 0.0),
                                            ptr(skip), BG_CUS if side is not None else 0,
                                            ctypes.c_void_p(side.cuda_stream) if side is not None else stream()), "yolo_adam_step_factored")

    def _launch(self, group, step, tab, count, norm, skip, side):
        b1, b2 = group["betas"]
        h = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), step, ptr(norm),
             float(self.max_grad_norm or 0.0), ptr(skip))
        if side is not None:
            check(lib().yolo_adam_step_multi_bg(tab, count, *h, BG_CUS, ctypes.c_void_p(side.cuda_stream)), "yolo_adam_step_multi_bg")
        else:
            check(lib().yolo_adam_step_multi(tab, count, *h, stream()), "yolo_adam_step_multi")


class SGD(_Fused):
    """torch.optim.SGD semantics (momentum, dampening, L2 weight decay, Nesterov; maximize=False) on yolo_sgd_step_multi: the state is
    ``momentum_buffer`` per parameter, created on the first step, and the param groups carry torch's keys, so ``state_dict()`` loads into
    ``torch.optim.SGD`` and the other way round.

    One edge: a step that ``skip_if`` cancels on the device while it is a parameter's very first one leaves the new momentum buffer at
    zero, and the host has already counted it as created -- the next step then takes ``momentum * 0 + (1 - dampening) * g`` where torch
    would copy ``g`` (the same unless dampening != 0).  The reference raises inside the loss forward in that situation and training ends;
    so it does here, when the training loop reads the loss ``parts`` of the flagged step."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm: float | None = None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None), max_grad_norm)

    def _step_on_cpu(self, all_params):
        """CPU parameters: the same step in stock torch ops (``_Fused._sgd_step_on_cpu``)"""
        total, skipped = self._begin_cpu_step(all_params)
        if not skipped:
            self._sgd_step_on_cpu(total)

    def _factored_state(self, group, p):
        return self._momentum_buffer(group, p)

    def _launch_factored(self, group, p, rec, shadow, fstate, norm, skip, side):
        buf, first = fstate
        d = rec.desc(p)
        check(lib().yolo_sgd_step_factored(ctypes.byref(d), ptr(p), ptr(buf), ptr(shadow), float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                                           float(group["weight_decay"]), int(bool(group["nesterov"])), int(first), ptr(norm), float(self.max_grad_norm or 0.0),
                                           ptr(skip), BG_CUS if side is not None else 0,
                                           ctypes.c_void_p(side.cuda_stream) if side is not None else stream()), "yolo_sgd_step_factored")

    def _entry(self, group, p, g, shadow):
        buf, first = self._momentum_buffer(group, p)
        return first, SgdTensor(p.data_ptr(), g.data_ptr(), buf.data_ptr() if buf is not None else None,
                                shadow.data_ptr() if shadow is not None else None, p.numel())

    def _launch(self, group, first, tab, count, norm, skip, side):
        h = (float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]), int(bool(group["nesterov"])),
             int(first), ptr(norm), float(self.max_grad_norm or 0.0), ptr(skip))
        if side is not None:
            check(lib().yolo_sgd_step_multi_bg(tab, count, *h, BG_CUS, ctypes.c_void_p(side.cuda_stream)), "yolo_sgd_step_multi_bg")
        else:
            check(lib().yolo_sgd_step_multi(tab, count, *h, stream()), "yolo_sgd_step_multi")


class LARS(_Fused):
    """Layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) on yolo_lars_step_multi, for the large effective batches of
    ``--accum-steps`` x ranks: the regularised gradient of every tensor is scaled by its trust ratio

        trust = eta * |p| / (clip * |g| + weight_decay * |p| + eps)          (1 when |p| or |g| is 0, or the group carries ``adapt=False``)

    and handed to SGD with momentum (no dampening, no Nesterov; the form of the common PyTorch LARS wrappers around ``torch.optim.SGD``).
    Per step ONE yolo_lars_norms_multi call reads every parameter and gradient once and leaves |p|^2, |g|^2 per tensor and the global
    squared gradient norm on the device (order-fixed, no atomics: the same entries serve ``EngineConfig.DETERMINISTIC``); the step launches
    read them there, so ``max_grad_norm``, ``skip_if``, ``attach_plan`` (bf16 shadows, the background pass of the Linear layers) and
    ``synchronize`` are ``_Fused``'s, unchanged.  The attached plans' squared-norm hints are dropped unused.  State per parameter:
    ``momentum_buffer``.  Use ``lars_param_groups`` to keep biases and BatchNorm gamma / beta out of the adaptation and the decay."""

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0, eta=1e-3, eps=1e-8, max_grad_norm: float | None = None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if eta < 0.0:
            raise ValueError(f"Invalid eta value: {eta}")
        if eps < 0.0:
            raise ValueError(f"Invalid eps value: {eps}")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, eta=eta, eps=eps, adapt=True), max_grad_norm)
        self._norms = None                        # this step's norms buffer
        self._norm_index: dict[int, int] = {}     # id(param) -> its tensor index in it

    @torch.no_grad()
    def step(self, closure=None):
        if CFG.FC_FACTORED or any(_plan_factored(pl) for pl in self.plans) or \
                any(p.grad is None and fc_factors_of(p)[0] is not None for g in self.param_groups for p in g["params"]):
            raise RuntimeError(FC_FACTORED_REFUSED.format(what="yolo.optim.LARS (its trust ratio needs the per-tensor norm of the gradient)"))
        return super().step(closure)

    def _step_on_cpu(self, all_params):
        """CPU parameters: the same step in stock torch ops -- per-tensor sums of squares in double, the clip coefficient formed in fp32 as the
        kernels form it, the trust ratio in double narrowed to fp32, then SGD (``_Fused._sgd_step_on_cpu``: with ``adapt=False`` it is
        yolo.optim.SGD's CPU step).  The plans' hints are drained unused."""
        sums = {id(p): (p.detach().double().pow(2).sum(), p.grad.double().pow(2).sum()) for p in all_params}
        acc = torch.zeros((), dtype=torch.float64)
        for p in all_params:
            acc += sums[id(p)][1]
        total, skipped = self._begin_cpu_step(all_params, acc)
        if skipped:
            return
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))

        def trust(group, p, g, clip):
            if group.get("adapt", True):
                wn = float(sums[id(p)][0].sqrt())
                gn = (float(clip) if clip is not None else 1.0) * float(sums[id(p)][1].sqrt())
                if wn > 0.0 and gn > 0.0:
                    g = g * torch.tensor(f32(group["eta"]) * wn / (gn + f32(group["weight_decay"]) * wn + f32(group["eps"])), dtype=torch.float32)
            return g
        self._sgd_step_on_cpu(total, trust)

    def _clip_norm_sq(self, all_params):
        """one norms call for all parameters with gradients, in the foreground; -> its g_total (None without max_grad_norm)"""
        self._known_norms()                       # cleared, not used (FC1's own tensor could take its hint: a follow-up)
        dev = all_params[0].device
        grads = []
        for p in all_params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("yolo.optim.LARS needs contiguous fp32 parameters")
            grads.append(_f32c(p.grad))
        _hip.require_cuda(*grads)
        count = len(all_params)
        if self._pending is not None:
            torch.cuda.current_stream().wait_event(self._pending)    # the last background launch read the norms buffer this call overwrites
        st = stream()
        pp = (ctypes.c_void_p * count)(*[p.data_ptr() for p in all_params])
        gp = (ctypes.c_void_p * count)(*[g.data_ptr() for g in grads])
        gn = (ctypes.c_long * count)(*[p.numel() for p in all_params])
        slots = ctypes.c_long(0)
        check(lib().yolo_lars_norm_slots(gn, count, ctypes.byref(slots)), "yolo_lars_norm_slots")
        scratch = _scratch("sumsq", dev, st, slots.value)
        self._norms = _scratch("lars", dev, st, 2 * count)
        self._norm_index = {id(p): i for i, p in enumerate(all_params)}
        total = torch.empty((), dtype=torch.float64, device=dev) if self.max_grad_norm is not None else None
        check(lib().yolo_lars_norms_multi(pp, gp, gn, count, ptr(scratch), scratch.numel(), ptr(self._norms), ptr(total), st), "yolo_lars_norms_multi")
        return total

    def _entry(self, group, p, g, shadow):
        buf, first = self._momentum_buffer(group, p)
        adapt = bool(group.get("adapt", True))
        norms = self._norms.data_ptr() + 16 * self._norm_index[id(p)] if adapt else None
        return first, _hip.LarsTensor(p.data_ptr(), g.data_ptr(), buf.data_ptr() if buf is not None else None,
                                      shadow.data_ptr() if shadow is not None else None, norms, p.numel(), int(adapt))

    def _launch(self, group, first, tab, count, norm, skip, side):
        h = (float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]), float(group["eta"]), float(group["eps"]), int(first),
             ptr(norm), float(self.max_grad_norm or 0.0), ptr(skip))
        if side is not None:
            self._norms.record_stream(side)
            check(lib().yolo_lars_step_multi_bg(tab, count, *h, BG_CUS, ctypes.c_void_p(side.cuda_stream)), "yolo_lars_step_multi_bg")
        else:
            check(lib().yolo_lars_step_multi(tab, count, *h, stream()), "yolo_lars_step_multi")


def lars_param_groups(model, weight_decay: float) -> list:
    """the two param groups of a LARS run: tensors with ``ndim > 1`` (convolution and Linear weights: adapted, decayed) and tensors with
    ``ndim <= 1`` (biases, BatchNorm gamma / beta: ``adapt=False``, ``weight_decay=0`` -- the plain clipped SGD step)"""
    params = [p for p in model.parameters() if p.requires_grad]
    return [{"params": [p for p in params if p.ndim > 1], "weight_decay": weight_decay},
            {"params": [p for p in params if p.ndim <= 1], "weight_decay": 0.0, "adapt": False}]


def _state_tensors(module):
    """(name, tensor) of every entry ``module.state_dict()`` would hold, in its order (per module: parameters, persistent buffers, then the
    children) -- read off the modules themselves, because ``state_dict()`` runs the hooks that wait for a background update (_Fused._hook_owner)
    and ModelEMA.update must not wait"""
    for prefix, m in module.named_modules(remove_duplicate=False):
        dot = prefix + "." if prefix else ""
        for k, v in m._parameters.items():
            if v is not None:
                yield dot + k, v
        for k, v in m._buffers.items():
            if v is not None and k not in m._non_persistent_buffers_set:
                yield dot + k, v


class ModelEMA:
    """Exponential moving average of a model's weights, the copy a detector validates and ships (torch.optim.swa_utils.AveragedModel with
    get_ema_multi_avg_fn): ``module`` is a deep copy of ``model`` in eval() mode, and every ``update()`` -- one per optimizer step -- moves it
    towards the model,

        e = fmaf(w, p - e, e)          w = fp32(1 - d),  d = decay * (1 - exp(-updates / tau)) if tau > 0 else decay

    for floating-point parameters and buffers (BatchNorm running statistics); other buffers (num_batches_tracked) are copied.  CPU tensors
    take ``torch._foreach_lerp_``, device tensors yolo_ema_update_multi (ema.hip) on the current stream.

    ``optimizer``: the ``yolo.optim`` optimizer that steps ``model``.  The parameters it updates in the background
    (``attach_plan(plan, overlap=True)``: the Linear layers, three quarters of the bytes) are averaged in the background too:
    yolo_ema_update_multi_bg on the optimizer's own second stream, behind its launch, on BG_CUS CUs beside the next forward's conv stack.
    A step the optimizer skipped on the device (``skip_if``) is no EMA step: its flag goes to the EMA launches as well.

    Nobody who reads ``module`` has to know about that stream: ``state_dict()`` / ``load_state_dict()`` here and on ``module``,
    ``copy.deepcopy(module)`` and a forward of ``module`` make the current stream wait for the background launch by themselves (the hooks and
    the plan's ``params_ready`` slot that ``attach_plan`` uses on the model's side); ``synchronize()`` does it for any other reader.
    ``background=False`` keeps every launch on the current stream, which then waits for the optimizer's background launch first (default:
    EMA_BACKGROUND).  Without ``optimizer`` nothing is known about a second stream: give it whenever the optimizer has one."""

    def __init__(self, model, decay: float = 0.9999, tau: float = 0.0, optimizer=None, background: bool | None = None):
        import copy
        if not (0.0 <= decay <= 1.0) or tau < 0.0:
            raise ValueError("ModelEMA needs 0 <= decay <= 1 and tau >= 0")
        self.decay, self.tau, self.updates = float(decay), float(tau), 0
        self.optimizer = optimizer
        self.background = EMA_BACKGROUND if background is None else bool(background)
        self.module = copy.deepcopy(model).eval()       # waits for a background update of ``model`` (models._PlanOwner.__deepcopy__)
        self.module.requires_grad_(False)
        self._model = weakref.ref(model)
        self._event, self._event_device = None, None    # behind the last background launch
        self._hooked: set = set()
        _wait_before_state_io(self, self.module)

    def effective_decay(self, updates: int | None = None) -> float:
        """the decay of update number ``updates`` (default: the last one made): the warm-up of ``tau`` lets the first updates follow the model"""
        import math
        n = self.updates if updates is None else updates
        return self.decay * (1.0 - math.exp(-n / self.tau)) if self.tau > 0 else self.decay

    def synchronize(self) -> None:
        """make the CURRENT stream wait for a background update of ``module`` still running on the optimizer's second stream"""
        if self._event is not None:
            torch.cuda.current_stream(self._event_device).wait_event(self._event)
            self._event = None

    @torch.no_grad()
    def update(self, model=None) -> None:
        """one EMA step from ``model`` (default: the model the constructor copied), to be called after ``optimizer.step()``.  The host counts
        it in ``updates`` even when the device-side flag then cancels it: the training loop ends at such a step, where the loss raises."""
        model = self._model() if model is None else model
        if model is None:
            raise ValueError("ModelEMA.update: the model the average was built from is gone, pass the one being trained")
        opt = self.optimizer
        skip = getattr(opt, "last_skip", None)
        dst, src = list(_state_tensors(self.module)), list(_state_tensors(model))
        if [n for n, _ in dst] != [n for n, _ in src]:
            raise RuntimeError("ModelEMA.update: the model's state_dict entries are not those of the averaged copy")
        if skip is not None and not skip.is_cuda and float(skip) != 0.0:
            return                                      # CPU run: the optimizer read the flag on the host and skipped; so does the EMA
        self.updates += 1
        w = 1.0 - self.effective_decay()                # in double; the launches narrow it to fp32, the value tests/ema_ref.py works with
        cpu_e, cpu_p, fore, back = [], [], [], []
        deferred = opt.deferred if (self.background and opt is not None and OVERLAP and getattr(opt, "_side", None) is not None) else {}
        for (name, e), (_, p) in zip(dst, src):
            if e.shape != p.shape or e.device != p.device:
                raise RuntimeError(f"ModelEMA.update: {name}: {tuple(p.shape)} on {p.device} does not match the averaged copy")
            if not e.is_floating_point():
                if skip is None or not e.is_cuda:
                    e.copy_(p)
                else:
                    e.copy_(torch.where(skip != 0, e, p))      # a skipped step is no EMA step: the counter stays, too
            elif e.numel() == 0:
                continue
            elif not e.is_cuda:
                cpu_e.append(e)
                cpu_p.append(p.detach().to(e.dtype))
            else:
                if e.dtype != torch.float32 or p.dtype != torch.float32 or not (e.is_contiguous() and p.is_contiguous()):
                    raise RuntimeError(f"yolo.optim.ModelEMA needs contiguous fp32 tensors on the device ({name})")
                (back if id(p) in deferred else fore).append((e, p))
        if cpu_e:
            torch._foreach_lerp_(cpu_e, cpu_p, w)
        if not (fore or back):
            return
        if len(back) > MT_MAX:                            # more than one background table: the optimizer took the foreground as well
            fore, back = fore + back, []
        if not back and hasattr(opt, "synchronize"):
            opt.synchronize()                           # everything in the foreground: the optimizer's background launch writes p, wait for it
        dev = (fore or back)[0][0].device
        _hip.require_cuda(skip, *[t for pair in fore + back for t in pair])
        with torch.cuda.device(dev):
            if fore:
                self.synchronize()                      # these may include tensors an earlier update left to the second stream (long done by now)
                tab = (EmaTensor * len(fore))(*[EmaTensor(e.data_ptr(), p.data_ptr(), e.numel()) for e, p in fore])
                check(lib().yolo_ema_update_multi(tab, len(fore), w, ptr(skip), stream()), "yolo_ema_update_multi")   # one launch per MT_MAX tensors
            if back:
                # The second stream runs its launches in order.  The optimizer's background launch of this step is already on it, so the
                # EMA reads the updated p; the NEXT step's background launch -- the only writer of these p -- will be enqueued on the same
                # stream behind this read.  What the main stream did to the averaged tensors (a forward of ``module`` during validation,
                # load_state_dict) comes first through wait_stream; later readers there wait for the event recorded below.
                side = opt._side
                side.wait_stream(torch.cuda.current_stream())
                for e, _ in back:
                    e.record_stream(side)
                if skip is not None:
                    skip.record_stream(side)
                tab = (EmaTensor * len(back))(*[EmaTensor(e.data_ptr(), p.data_ptr(), e.numel()) for e, p in back])
                check(lib().yolo_ema_update_multi_bg(tab, len(back), w, ptr(skip), BG_CUS, ctypes.c_void_p(side.cuda_stream)),
                      "yolo_ema_update_multi_bg")
                ev = torch.cuda.Event()
                ev.record(side)
                self._event, self._event_device = ev, dev
                self._publish(model, ev)
            for e, _ in fore + back:
                # the kernels wrote through raw pointers: bump the version so that ``module``'s engine plan repacks its bf16 operands
                torch.autograd.graph.increment_version(e)

    def _publish(self, model, ev) -> None:
        """hand the event to the averaged copy's own plans (the twins of the plans whose Linear layers the optimizer defers): their forward
        waits for it in front of the first Linear layer, and a deep copy of their owner waits too"""
        names = {id(m): n for n, m in model.named_modules()}
        for plan in {id(pl): pl for pl in self.optimizer.deferred.values()}.values():
            owner = plan.owner() if getattr(plan, "owner", None) is not None else None
            if owner is None or id(owner) not in names:
                continue
            twin = self.module.get_submodule(names[id(owner)])
            _wait_before_state_io(self, twin)
            twin_plan = twin.__dict__.get("_plan")
            if twin_plan is not None and hasattr(twin_plan, "params_ready"):
                twin_plan.params_ready.event = ev

    def state_dict(self) -> dict:
        return {"module": self.module.state_dict(), "updates": self.updates, "decay": self.decay, "tau": self.tau}

    def load_state_dict(self, state: dict) -> None:
        self.module.load_state_dict(state["module"])
        self.updates = int(state["updates"])
        self.decay, self.tau = float(state.get("decay", self.decay)), float(state.get("tau", self.tau))


def accum_alpha(steps: int) -> float:
    """the fp32 weight of one micro-batch in a group of ``steps``, as a Python float: (float)(1.0 / steps), the quotient formed in double"""
    return float(torch.tensor(1.0 / int(steps), dtype=torch.float64).float())


def _reducers(reducer) -> list:
    """the reducers behind ``reducer`` (parallel._Both holds several)"""
    if reducer is None:
        return []
    if hasattr(reducer, "reducers"):
        return [r for sub in reducer.reducers for r in _reducers(sub)]
    return [reducer]


class GradAccumulator:
    """Gradient accumulation: ``steps`` = K micro-batches per optimizer step, and per all-reduce (DDP's ``no_sync``, Darknet's subdivisions).
    After the K-th backward ``p.grad`` holds

        g = (g_1 + ... + g_K) / K          as the chain  a = alpha g_1;  a = fmaf(alpha, g_k, a);  g = fmaf(alpha, g_K, a),   alpha = fp32(1 / K)

    -- the gradient of the concatenated batch, because YOLOLoss divides by the local N and the micro-batches are equal (and so does
    ``yolo.classify.SoftmaxCrossEntropy``, the mean over its batch: with equal micro-batches and equal shards the folded, rank-averaged
    gradient of the classifier is the concatenated batch's too).  The last link
    folds the accumulator INTO THE GRADIENT MEMORY, not the other way round: ``p.grad`` stays the arena view (or autograd's tensor), so the
    optimizers, the clip norm, the bf16 shadows, the background update of the Linear layers and the reducers read what they read without
    accumulation, and none of them changes.

        acc = GradAccumulator(model, K, reducer)          # reducer: parallel.make_grad_reducer(model, device), or None
        for images, targets in loader:
            optimizer.zero_grad(set_to_none=True)
            acc.before_backward()
            loss, parts = criterion(model(images), targets)
            loss.backward()
            if acc.after_backward(getattr(parts, "device_flag", None)):
                optimizer.skip_if = acc.skip_if
                optimizer.step()

    On a GPU, a fused YOLOv1 (``model._fusable()``) or a ``DetectionHead`` with ``hip_plan`` gets the plan's gradient arena attached if it has
    none (the plan's ``on_*`` callbacks stay None without a reducer) and ONE flat accumulator of the arena's size: the whole network is one
    yolo_grad_accum call per micro-batch (accum.hip; 8 B per element for the first, 12 B for the others).  A model that runs several plans and
    lists them as ``hip_plans()`` (``YOLOv1Classifier``: trunk, head) gets an arena and an accumulator per plan, and the arenas go through
    yolo_grad_accum_multi as one launch.  Parameters outside a plan (a ResNet
    trunk, custom modules) get an accumulator each and go through yolo_grad_accum_multi.  CPU tensors take stock torch ops
    (``torch._foreach_mul_`` / ``torch._foreach_add_`` with alpha).  ``steps == 1`` allocates nothing and launches nothing.

    ``skip_if``: the maximum of the micro-batches' ``LossParts.device_flag`` (a torch op on the device, nothing waits): one flagged micro-batch
    cancels the group's optimizer step, and through ``optimizer.last_skip`` the EMA step.

    With a reducer, ``before_backward`` mutes it for the micro-batches 1 .. K-1 (no range announced, no collective enqueued, ``all_reduce_mean``
    not called), so the ranks exchange one gradient per K backward passes.  For a ``parallel.OverlappedGradAllReduce`` the fold of the K-th
    pass is its ``pre_reduce(lo, hi)`` hook: ``arena[lo:hi]`` is folded immediately in front of the collective that carries it, on the stream
    that enqueues the collective, so the all-reduce still overlaps the backward pass.  Why that is ordered:

    * the ranges ``_reduce`` sees partition [0, arena.numel()) exactly once per backward, so every element is folded once;
    * every range starts on a 256-B boundary (``attach_grad_arena`` rounds to 64 elements), which the kernel's 16-B rule needs;
    * ``_check_ordered`` has verified that the enqueuing stream holds every piece of the range, so the fold reads a finished micro-gradient;
    * the accumulator itself was written by the launches of the micro-batches 1 .. K-1 on the MAIN stream, each behind its own backward (whose
      end joins the side stream into the main one).  The K-th backward enters the side stream through ``_on_side_stream``, which makes it
      wait for everything queued on the main stream -- those launches included -- so a fold on either stream reads the finished sum.  The next
      group's first launch overwrites the accumulator on the main stream behind the K-th backward's join, i.e. behind every fold.

    After the fold the plans' ``grad_norm_sq`` hints are dropped and the arena's version is bumped (as ``OverlappedGradAllReduce.finish``
    does): the hint is the last micro-gradient's norm, so the clip pass reads the folded gradient instead.  The pass is elementwise, so
    ``EngineConfig.DETERMINISTIC`` keeps its promise with accumulation on."""

    def __init__(self, model, steps: int, reducer=None):
        if int(steps) != steps or steps < 1:
            raise ValueError("GradAccumulator needs steps >= 1")
        self.steps, self.reducer, self.micro = int(steps), reducer, 0
        self.alpha = accum_alpha(self.steps)
        self.skip_if = None                  # device float: the group's flag so far (None: no micro-batch brought one)
        self._overlapped = [r for r in _reducers(reducer) if hasattr(r, "pre_reduce")]
        self._arenas: list[tuple] = []       # (plan, accumulator of the arena's size, folded by a reducer's hook?)
        self._rest: list = []                # parameters outside every plan
        self._acc: dict[int, torch.Tensor] = {}      # id(param) -> accumulator, allocated at the parameter's first gradient
        self._have: set = set()              # ids whose accumulator holds something in this group
        if self.steps == 1:
            return
        if CFG.FC_FACTORED or any(_plan_factored(r.plan) for r in self._overlapped):
            raise RuntimeError(FC_FACTORED_REFUSED.format(what=f"yolo.optim.GradAccumulator(steps={self.steps}) (the sum of K factored gradients is "
                                                               "not a product of two factors of one micro-batch)"))
        params = [p for p in model.parameters() if p.requires_grad]
        plans = {id(r.plan): (r.plan, r) for r in self._overlapped}
        on_gpu = bool(params) and params[0].is_cuda
        if on_gpu:
            head = getattr(model, "head", None)
            plan = model.hip_plan() if (hasattr(model, "_fusable") and model._fusable()) else \
                head.hip_plan() if (head is not None and hasattr(head, "hip_plan")) else None
            own = [plan] if plan is not None else list(model.hip_plans()) if hasattr(model, "hip_plans") else []
            for plan in own:
                if plan.arena is None:
                    plan.attach_grad_arena(params[0].device)
                plans.setdefault(id(plan), (plan, None))
        covered = set()
        for plan, red in plans.values():
            if _plan_factored(plan):
                raise RuntimeError(FC_FACTORED_REFUSED.format(what=f"yolo.optim.GradAccumulator(steps={self.steps})"))
            self._arenas.append((plan, torch.empty_like(plan.arena), red is not None))
            covered |= {id(p) for p in plan.params}
            if red is not None:
                red.pre_reduce = self._hook(len(self._arenas) - 1)
        self._rest = [p for p in params if id(p) not in covered]

    # ------------------------------------------------------------------ the one operation, by device
    def _run(self, items) -> None:
        """items: (dst, x, y | None) tensors of one device, dst being x, y or neither -- dst = alpha * x (+ y)"""
        if not items:
            return
        if not items[0][0].is_cuda:
            store = [(d, x) for d, x, y in items if y is None and d is not x]
            scale = [d for d, x, y in items if d is x]                                # the fold (and a fold without a sum: alpha * g)
            if store:
                torch._foreach_copy_([d for d, _ in store], [x for _, x in store])
                scale += [d for d, _ in store]
            if scale:
                torch._foreach_mul_(scale, self.alpha)
            fold = [(d, y) for d, x, y in items if d is x and y is not None]
            if fold:
                torch._foreach_add_([d for d, _ in fold], [y for _, y in fold])
            add = [(d, x) for d, x, y in items if d is y]
            if add:
                torch._foreach_add_([d for d, _ in add], [x for _, x in add], alpha=self.alpha)
            return
        for t in items:
            for v in t:
                if v is not None and not (v.dtype == torch.float32 and v.is_contiguous()):
                    raise RuntimeError("yolo.optim.GradAccumulator needs contiguous fp32 gradients on the device")
        _hip.require_cuda(*[v for t in items for v in t if v is not None])
        with torch.cuda.device(items[0][0].device):
            if len(items) == 1:
                dst, x, y = items[0]
                check(lib().yolo_grad_accum(ptr(dst), ptr(x), ptr(y), dst.numel(), self.alpha, None, stream()), "yolo_grad_accum")
            else:
                tab = (AccumTensor * len(items))(*[AccumTensor(d.data_ptr(), x.data_ptr(), y.data_ptr() if y is not None else None, d.numel())
                                                   for d, x, y in items])
                check(lib().yolo_grad_accum_multi(tab, len(items), self.alpha, None, stream()), "yolo_grad_accum_multi")   # one launch per MT_MAX tensors

    def _hook(self, k: int):
        def fold(lo: int, hi: int):
            plan, acc, _ = self._arenas[k]
            if self.micro == self.steps - 1:             # armed: the K-th backward of the group is running
                g = plan.arena[lo:hi]
                self._run([(g, g, acc[lo:hi])])
        return fold

    # ------------------------------------------------------------------ the two calls around loss.backward()
    def before_backward(self) -> None:
        """in front of every ``loss.backward()``: mutes the reducer on the micro-batches 1 .. K-1, arms the fold on the K-th"""
        if self.micro == 0:
            self.skip_if = None
        last = self.micro == self.steps - 1
        for r in self._overlapped:
            r.muted = not last

    @torch.no_grad()
    def after_backward(self, device_flag=None) -> bool:
        """behind every ``loss.backward()``: accumulates, and on the K-th call of a group folds (and averages across ranks) and returns True --
        the optimizer's turn.  ``device_flag``: the loss's ``LossParts.device_flag`` (None: none)"""
        if device_flag is not None:
            self.skip_if = device_flag if self.skip_if is None else torch.maximum(self.skip_if, device_flag)
        first, last = self.micro == 0, self.micro == self.steps - 1
        self.micro = 0 if last else self.micro + 1
        if self.steps == 1:
            if self.reducer is not None:
                self.reducer.all_reduce_mean()
            return True
        items = []
        for plan, acc, hooked in self._arenas:
            if not last:
                items.append((acc, plan.arena, None if first else acc))
            elif not hooked:
                items.append((plan.arena, plan.arena, acc))
        if first:
            self._have.clear()
        for p in self._rest:
            g, a = p.grad, self._acc.get(id(p))
            if g is None:
                if last and id(p) in self._have:
                    p.grad = a.clone()                   # no gradient in the last micro-batch: the sum so far is the group's
                continue
            if a is None and not last:
                a = self._acc[id(p)] = torch.empty_like(g, memory_format=torch.contiguous_format)
            have = id(p) in self._have
            if not last:
                items.append((a, g, a if have else None))
                self._have.add(id(p))
            else:
                items.append((g, g, a if have else None))
        by_dev: dict = {}
        for it in items:
            by_dev.setdefault(it[0].device, []).append(it)
        for group in by_dev.values():
            self._run(group)
        if not last:
            return False
        if self.reducer is not None:
            self.reducer.all_reduce_mean()           # an overlapped reducer folded range by range in front of its collectives
        for plan, _, _ in self._arenas:
            plan.grad_norm_sq.clear()                # the last micro-gradient's norm, not the group's
            torch.autograd.graph.increment_version(plan.arena)
        return True
