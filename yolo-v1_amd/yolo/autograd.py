"""autograd bridges: a whole plan (or the whole trainable ResNet trunk, or BatchNorm chain) is ONE autograd node -- no per-layer graph."""

from __future__ import annotations

import torch

from . import _hip
from .executor import Plan

class PlanFunction(torch.autograd.Function):
    """autograd bridge: forward/backward of a whole plan as ONE node (no per-layer autograd graph)."""

    @staticmethod
    def forward(ctx, plan: Plan, drop_training: bool, need_grad: bool, x: torch.Tensor, *params):
        out, saved = plan.forward(x, need_grad, drop_training)
        ctx.plan = plan
        ctx.saved = saved
        ctx.x_needs = x.requires_grad
        return out

    @staticmethod
    @_hip.device_guard
    def backward(ctx, gout):
        if ctx.saved is None:
            raise RuntimeError("backward through a plan that ran without grad")
        gx, pg = ctx.plan.backward(ctx.saved, gout, ctx.x_needs)
        ctx.saved = None
        return (None, None, None, gx, *pg)


class ConvBNTrainFunction(torch.autograd.Function):
    """autograd bridge of the conv -> BatchNorm executors: one node for the whole trainable ResNet trunk or BatchNorm chain
    (``plan.forward_train`` / ``plan.backward_train`` of a ResNetPlan or a BNPlan)."""

    @staticmethod
    def forward(ctx, plan, frozen: bool, x: torch.Tensor, *params):
        out, saved = plan.forward_train(x, frozen)
        ctx.plan, ctx.saved, ctx.params = plan, saved, params
        return out

    @staticmethod
    @_hip.device_guard
    def backward(ctx, gout):
        if ctx.saved is None:
            raise RuntimeError(f"backward through {ctx.plan.WHAT} forward that was already consumed")
        if ctx.needs_input_grad[2] and ctx.plan.NO_INPUT_GRAD is not None:
            raise NotImplementedError(ctx.plan.NO_INPUT_GRAD)
        grads = ctx.plan.backward_train(ctx.saved, gout)
        ctx.saved = None
        return (None, None, None) + tuple(grads.get(p) if p.requires_grad else None for p in ctx.params)


ResNetTrainFunction = BNTrainFunction = ConvBNTrainFunction          # the names the two executors were given their bridges under


def run_plan(plan: Plan, x, drop_training: bool) -> torch.Tensor:
    """x: NCHW fp32 device tensor, or a ``yolo.augment.U8Batch`` on the device (which never asks for an input gradient)"""
    if not isinstance(x, torch.Tensor):
        with torch.cuda.device(x.device):          # device_guard looks at tensor arguments only
            return _run_plan(plan, x, drop_training)
    return _run_plan(plan, x, drop_training)


@_hip.device_guard
def _run_plan(plan: Plan, x, drop_training: bool) -> torch.Tensor:
    _hip.require_cuda(x)
    # grad mode must be sampled here: inside Function.forward it is always off
    need = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in plan.params))
    return PlanFunction.apply(plan, drop_training, need, x, *plan.params)

