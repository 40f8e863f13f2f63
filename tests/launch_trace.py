"""Launch traces of the executors on the CPU: the real ``Plan`` / ``ResNetPlan`` / ``BNPlan`` code drives a stand-in library and recording streams (the ``RT``
hooks, as tests/test_parallel_cpu.py does), and every library call and every ``wait_stream`` becomes one normalised line:

    entry | scalar arguments | full bytes of every descriptor / array argument | pointers as null / (buffer name, element offset) / tmp

Pointer-typed descriptor fields are taken out of the bytes and normalised like pointer arguments.  Names are resolved after the pass against the
buffers reachable from the plan (workspaces, operand caches, parameters, arena), so no raw address enters a trace and a trace is stable run to run.
A refactor of the host code that moves no launch leaves every trace as it is: tests/test_launch_trace_cpu.py compares digests recorded at the
commit BEFORE such a refactor (``python tests/launch_trace.py --root <checkout of that commit> --write tests/launch_trace_cpu.json``)."""

from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import hashlib
import json
import os
import sys

import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

MAIN, SIDE = 0x1000, 0x2000
_STREAM_NAMES = {MAIN: "main", SIDE: "side"}
SLAB_FLOATS = 4096          # what the stand-in yolo_wgrad_slab_floats answers: every launch that asks gets slabs attached


class _KeepAlive(TorchDispatchMode):
    """keeps every tensor made during a recorded pass alive until the names are resolved: an address of a freed temporary that a later
    buffer of the plan reuses would otherwise resolve to that buffer"""

    def __init__(self):
        super().__init__()
        self.keep = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.keep.append(out)
        return out


class _Stream:
    def __init__(self, rec, handle):
        self.rec, self.cuda_stream = rec, handle

    def wait_stream(self, other):
        self.rec.log("wait_stream", [("p", self.cuda_stream), ("p", other.cuda_stream)])

    def wait_event(self, ev):
        pass


class _Lib:
    def __init__(self, rec):
        self.rec = rec

    def __getattr__(self, name):
        def call(*args):
            if name == "yolo_wgrad_slab_floats":
                args[1]._obj.value = SLAB_FLOATS
            self.rec.log(name, [p for a in args for p in _parts(a)])
            return 0
        return call


def _parts(a):
    """one argument -> [("s", text) | ("p", address)]"""
    if a is None:
        return [("s", "null")]
    if isinstance(a, ctypes.c_void_p):
        return [("p", a.value or 0)]
    if isinstance(a, (bool, int, float, str)):
        return [("s", repr(a))]
    if hasattr(a, "_obj"):                        # ctypes.byref(x)
        return _parts(a._obj)
    if isinstance(a, ctypes.Structure):
        raw = type(a).from_buffer_copy(a)
        out = []
        for f in a._fields_:
            if f[1] is ctypes.c_void_p:
                out.append(("p", getattr(a, f[0]) or 0))
                setattr(raw, f[0], None)
        return [("s", type(a).__name__ + ":" + bytes(raw).hex())] + out
    if isinstance(a, ctypes.Array):
        if issubclass(a._type_, ctypes.Structure):
            return [("s", f"[{len(a)}]")] + [p for item in a for p in _parts(item)]
        return [("s", type(a).__name__ + ":" + bytes(a).hex())]
    if isinstance(a, ctypes._SimpleCData):
        return [("s", repr(a.value))]
    raise TypeError(f"launch trace: argument of type {type(a)}")


_SKIP = {"grad_norm_sq", "layers", "owner", "cfg", "trace", "params_ready", "last"}     # (keyed by id(), or nothing that a launch points into)


def _named(obj, path, out):
    """(first byte, end, first element, item size, name) of every buffer reachable from obj"""
    from yolo.runtime import Act
    if isinstance(obj, Act):
        s = obj.store
        out.append((s.data_ptr(), s.data_ptr() + s.numel() * s.element_size(), obj.t.data_ptr(), s.element_size(), path))
    elif isinstance(obj, torch.Tensor):
        if obj.numel():
            out.append((obj.data_ptr(), obj.data_ptr() + obj.numel() * obj.element_size(), obj.data_ptr(), obj.element_size(), path))
    elif isinstance(obj, nn.Module):
        for n, t in list(obj.named_parameters()) + list(obj.named_buffers()):
            _named(t, f"{path}.{n}", out)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _named(v, f"{path}[{k!r}]", out)
    elif isinstance(obj, (list, tuple, set)):
        for i, v in enumerate(obj):
            _named(v, f"{path}[{i}]", out)
    elif hasattr(obj, "__dict__") and type(obj).__module__.startswith("yolo"):
        for k in sorted(vars(obj)):
            if k not in _SKIP:
                _named(getattr(obj, k), f"{path}.{k}", out)


class Recorder:
    """``with rec.recording(): ...`` runs executor code against the stand-ins; ``rec.lines(plan, x=x, ...)`` resolves the pointers and returns the trace"""

    def __init__(self):
        self.calls = []
        self.main, self.side_s = _Stream(self, MAIN), _Stream(self, SIDE)
        self.cur = self.main
        self.keep = _KeepAlive()

    def log(self, entry, parts):
        """one line: the entry, the stream that is current while it is called, its arguments"""
        self.calls.append((f"{entry} @{_STREAM_NAMES[self.cur.cuda_stream]}", parts))

    def callbacks(self, plan):
        """the gradient reducer's callbacks of a plan with an arena, as trace lines"""
        plan.on_grad_ready = lambda lo, hi: self.log("on_grad_ready", [("s", f"{lo} {hi}")])
        plan.on_backward_done = lambda: self.log("on_backward_done", [])
        plan.on_stream_wait = lambda a, b: self.log("on_stream_wait", [("p", a), ("p", b)])

    # -- the RT.STREAMS interface
    def current(self, dev):
        return self.cur

    def side(self, dev, low):
        return self.side_s

    def use(self, s):
        @contextlib.contextmanager
        def ctx():
            prev, self.cur = self.cur, s
            try:
                yield
            finally:
                self.cur = prev
        return ctx()

    @contextlib.contextmanager
    def recording(self):
        from yolo import _hip, preprocess
        from yolo.runtime import RT
        lib = _Lib(self)

        def u8_into(images, size, act, *a):       # yolo.preprocess launches through _hip directly (no RT hook): the executor's side of it only
            self.log("preprocess_u8_into", [("s", repr(tuple(size))), ("p", act.t.data_ptr())])

        patches = [(RT, "lib", lambda: lib), (RT, "stream", lambda: ctypes.c_void_p(self.cur.cuda_stream)), (RT, "STREAMS", self),
                   (RT, "_SIDE_STREAMS", {}), (RT, "_splitk_scratch", lambda n, zero: torch.zeros(n)),
                   (_hip, "require_cuda", lambda *t: None), (preprocess, "preprocess_u8_into", u8_into),
                   (torch.cuda, "current_stream", lambda dev=None: self.cur)]      # (the conv -> BatchNorm executors of a recorded commit may ask torch for the main stream)
        old = [(o, n, getattr(o, n)) for o, n, _ in patches]
        for o, n, v in patches:
            setattr(o, n, v)
        try:
            with self.keep:
                yield self
        finally:
            for o, n, v in old:
                setattr(o, n, v)

    def lines(self, plan, **extra):
        bufs = []
        for k, v in extra.items():
            _named(v, k, bufs)
        _named(plan, "plan", bufs)

        def name(addr):
            if addr == 0:
                return "null"
            if addr in _STREAM_NAMES:
                return "stream:" + _STREAM_NAMES[addr]
            for lo, hi, base, size, path in bufs:
                if lo <= addr < hi:
                    return f"{path}+{(addr - base) // size}"
            return "tmp"

        return [entry + " | " + " ".join(v if kind == "s" else name(v) for kind, v in parts) for entry, parts in self.calls]


# --------------------------------------------------------------------------------------------------------------------------- scenarios
_MODELS: dict = {}


def _model(kind):
    """one module per kind for the whole process (the 205 M-weight Linear takes seconds to initialise); every scenario builds its own plan from it"""
    if kind not in _MODELS:
        from yolo import models
        from yolo.resnet import resnet50_trunk
        torch.manual_seed(0)
        _MODELS[kind] = {"yolo": models.YOLOv1, "backbone": models.YOLOv1Backbone, "head": lambda: models.DetectionHead(2048),
                         "resnet": resnet50_trunk, "bn_backbone": lambda: models.YOLOv1Backbone(batch_norm=True)}[kind]()
    return _MODELS[kind]


def _plan(kind, cfg):
    from yolo.config import CONFIG
    from yolo.executor import Plan
    m = _model(kind)
    if kind == "yolo":
        plan = Plan.from_modules(list(m.backbone.features) + list(m.head), 3, True)
    elif kind == "backbone":
        plan = Plan.from_modules(m.features, 3, True)
    else:
        plan = Plan.from_modules(list(m.conv_layers) + list(m.fc_layers), 2048, False)
    if cfg:
        plan.cfg = dataclasses.replace(CONFIG, **cfg)
    for p in plan.params:
        p.grad = None
    return plan


def _train(kind="yolo", shape=(2, 3, 448, 448), need_gx=False, arena=False, det=False, **cfg):
    def run():
        from yolo.config import CONFIG
        rec, plan = Recorder(), _plan(kind, cfg)
        x = torch.zeros(shape)
        was = CONFIG.DETERMINISTIC
        CONFIG.DETERMINISTIC = det         # (plans.igemm_call reads the process-wide switch, the executor the plan's)
        try:
            with rec.recording():
                if arena:
                    plan.attach_grad_arena(x.device)
                    rec.callbacks(plan)
                out, saved = plan.forward(x, True, True)
                gout = torch.zeros_like(out)
                plan.backward(saved, gout, need_gx)
        finally:
            CONFIG.DETERMINISTIC = was
            for p in plan.params:
                p.grad = None
        return rec.lines(plan, x=x, out=out, gout=gout)
    return run


def _infer(N=2, u8=False, **cfg):
    def run():
        rec, plan = Recorder(), _plan("yolo", cfg)
        x = torch.zeros((N, 300, 400, 3), dtype=torch.uint8) if u8 else torch.zeros((N, 3, 448, 448))
        with rec.recording():
            out, _ = plan.forward(x, False, False, u8_size=(448, 448) if u8 else None)
        return rec.lines(plan, x=x, out=out)
    return run


@contextlib.contextmanager
def _switches(sw):
    """process-wide switches for one scenario (the conv -> BatchNorm executors read ``CONFIG``, not a plan's own copy)"""
    from yolo.config import CONFIG
    was = {k: getattr(CONFIG, k) for k in sw}
    for k, v in sw.items():
        setattr(CONFIG, k, v)
    try:
        yield
    finally:
        for k, v in was.items():
            setattr(CONFIG, k, v)


def _resnet(mode, size=64, **sw):
    def run():
        from yolo.resnet_executor import ResNetPlan
        trunk = _model("resnet")
        state = {k: v.clone() for k, v in trunk.state_dict().items()}      # (batch-statistics passes count num_batches_tracked up)
        rec, plan = Recorder(), ResNetPlan(trunk)
        x = torch.zeros((2, 3, size, size))
        extra = {"x": x}
        try:
            with _switches(sw), rec.recording():
                if mode == "forward":
                    extra["out"] = plan.forward(x)
                elif mode == "forward_twice":
                    extra["out"] = [plan.forward(x), plan.forward(x)]
                elif mode == "batch_stats":
                    extra["out"] = plan.forward_batch_stats(x)
                else:
                    out, saved = plan.forward_train(x, frozen=(mode == "frozen"))
                    gout = torch.zeros_like(out)
                    plan.backward_train(saved, gout)
                    extra.update(out=out, gout=gout)
        finally:
            trunk.load_state_dict(state)
        return rec.lines(plan, **extra)
    return run


def _bn(size=448, frozen=False, repack=False, **sw):
    def run():
        from yolo.bn_executor import BNPlan
        feats = _model("bn_backbone").features
        state = {k: v.clone() for k, v in feats.state_dict().items()}
        rec, plan = Recorder(), BNPlan.from_modules(feats)
        x = torch.zeros((2, 3, size, size))
        extra = {"x": x}
        try:
            with _switches(sw), rec.recording():
                if repack:          # the pack cache: the second forward packs nothing, the third repacks after a weight's version moved
                    outs = [plan.forward_train(x)[0], plan.forward_train(x)[0]]
                    with torch.no_grad():
                        plan.units[3][0].weight.add_(0)
                    extra["out"] = outs + [plan.forward_train(x)[0]]
                else:
                    out, saved = plan.forward_train(x, frozen=frozen)
                    gout = torch.zeros_like(out)
                    plan.backward_train(saved, gout)
                    extra.update(out=out, gout=gout)
        finally:
            feats.load_state_dict(state)
        return rec.lines(plan, **extra)
    return run


SCENARIOS = {
    "yolo_train": _train(),
    "yolo_train_arena": _train(arena=True),
    "yolo_train_need_gx": _train(need_gx=True),
    "yolo_train_deterministic": _train(det=True, DETERMINISTIC=True),
    "yolo_infer_b1": _infer(1),
    "yolo_infer_b2": _infer(2),
    "yolo_infer_u8": _infer(2, u8=True),
    **{f"yolo_train_no_{s}": _train(**{s: False}) for s in ("STEM_KERNEL", "FUSE_POOL", "POOL_CODES", "STEM_POOL_BWD_FUSED", "WGRAD_STREAM",
                                                          "FC_WGRAD_SIDE", "STRIDE2_CLASSES")},
    "yolo_infer_no_FLATTEN_FREE": _infer(2, FLATTEN_FREE=False),
    "yolo_infer_no_STEM_F32_INPUT": _infer(2, STEM_F32_INPUT=False),
    "backbone_train_448": _train("backbone"),
    "backbone_train_224": _train("backbone", (2, 3, 224, 224)),
    "backbone_train_240": _train("backbone", (2, 3, 240, 240)),      # 120 x 120 stem map: im2col weight gradient; odd maps: the stride-2 layer without classes
    "head_train_need_gx": _train("head", (2, 2048, 14, 14), need_gx=True),
    "resnet_forward": _resnet("forward"),
    "resnet_forward_generic_stem": _resnet("forward", 48),            # a stem map the dedicated kernel's 8 x 16 tiles do not cover
    "resnet_batch_stats": _resnet("batch_stats"),
    "resnet_train": _resnet("train"),
    "resnet_train_generic_stem": _resnet("train", 48),
    "resnet_train_frozen": _resnet("frozen"),
    "resnet_forward_twice": _resnet("forward_twice"),                 # the second pass packs nothing
    "resnet_train_no_BN_STATS_IN_CONV": _resnet("train", BN_STATS_IN_CONV=False),
    "resnet_batch_stats_no_BN_STATS_IN_CONV": _resnet("batch_stats", BN_STATS_IN_CONV=False),
    "resnet_train_no_WGRAD_STREAM": _resnet("train", WGRAD_STREAM=False),
    "bn_train_448": _bn(),
    "bn_train_240": _bn(240),               # 120 x 120 stem map: im2col stem weight gradient; an odd map: unfused pool forward and backward
    "bn_train_frozen": _bn(frozen=True),
    "bn_train_no_BN_POOL_FUSED": _bn(224, BN_POOL_FUSED=False),
    "bn_train_no_WGRAD_STREAM": _bn(224, WGRAD_STREAM=False),
    "bn_train_repack": _bn(224, repack=True),
}


def digest(lines):
    """call count, digest of the whole trace, and six hex digits per line (enough to name the first line that differs)"""
    return {"calls": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(),
            "lines": "".join(hashlib.sha256(ln.encode()).hexdigest()[:6] for ln in lines)}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose yolo package is traced")
    ap.add_argument("--write", help="JSON file for {scenario: {calls, sha256}}")
    ap.add_argument("--dump", help="directory for the full traces")
    ap.add_argument("only", nargs="*")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "yolo-v1_amd"))
    res = {}
    for name_ in a.only or SCENARIOS:
        tr = SCENARIOS[name_]()
        res[name_] = digest(tr)
        print(name_, res[name_]["calls"], res[name_]["sha256"], flush=True)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, name_ + ".txt"), "w") as f:
                f.write("\n".join(tr) + "\n")
    if a.write:
        with open(a.write, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
