"""Workspaces and streams of the engine: zero-haloed activation buffers (``Act``), scratch pools, the second stream of the backward pass and the
event slot of a background optimizer pass, the per-launch timers -- and ``RT``, the one place the executors get the library, the current stream and the
stream factory from (tests of the stream schedule put recording stand-ins there: ``engine.lib = fake`` forwards to ``RT.lib``)."""

from __future__ import annotations

import ctypes

import torch

from . import _hip
from ._hip import IgemmDesc, WgradDesc, check
from .config import CONFIG as CFG


def _round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def _igemm(L_, d, inp, w, bias, aux, out, st, what):
    CFG.IGEMM_LAUNCHES += 1
    check(L_.yolo_igemm(ctypes.byref(d), inp, w, bias, aux, out, st), what)


# ---- yolo_igemm descriptors: the one place that knows how an ``Act`` (defined below) maps onto the in / out / aux sides of an ``IgemmDesc``.  Each builder
# sets exactly the fields named here; everything else (epilogue, slope, tile hints, split_k ..) stays zero until the call site sets it.
def igemm_desc(N, Ho, Wo, stride, KH, KW, tap_len, Cout, a_in: "Act", in_off: int, a_out: "Act | None" = None, in_mul: int = 1, out_mul: int = 1,
               py: int = 0, px: int = 0) -> IgemmDesc:
    """Problem geometry (an N x Ho x Wo output grid, KH x KW taps of tap_len channels at the given stride, Cout output channels), input side (a_in's
    strides, the first tap at element in_off) and, with a_out, output side (its interior).  in_mul = 2 reads every other slot (the non-zero slots of a
    zero-stuffed gradient); out_mul = 2 writes every other slot, from pixel (py, px) on: a parity class, or zero-stuffing.  One constructor call: these
    are the struct's leading fields, in its order (a forward at batch 1 is bound by this host code)."""
    if a_out is None:
        return IgemmDesc(N, Ho, Wo, a_in.img_stride, in_mul * a_in.row_stride, in_mul * a_in.px_stride, in_off, stride, KH, KW, tap_len, Cout)
    return IgemmDesc(N, Ho, Wo, a_in.img_stride, in_mul * a_in.row_stride, in_mul * a_in.px_stride, in_off, stride, KH, KW, tap_len, Cout,
                     a_out.img_stride, out_mul * a_out.row_stride, out_mul * a_out.px_stride, a_out.interior_off() + py * a_out.row_stride + px * a_out.px_stride)


def rows_desc(N, ld_in, K, Cout) -> IgemmDesc:
    """a Linear layer: N rows of K inputs (leading dimension ld_in) -> N dense rows of Cout outputs, as a 1 x 1 conv over a 1 x 1 grid"""
    return IgemmDesc(N, 1, 1, ld_in, 0, ld_in, 0, 1, 1, 1, K, Cout, Cout, 0, Cout, 0)


def desc_aux(d: IgemmDesc, a: "Act", mul: int = 1, py: int = 0, px: int = 0) -> None:
    """aux side (second input or second output of an epilogue), addressed like the output side of igemm_desc"""
    d.aux_img_stride, d.aux_row_stride, d.aux_px_stride = a.img_stride, mul * a.row_stride, mul * a.px_stride
    d.aux_off = a.interior_off() + py * a.row_stride + px * a.px_stride


def f32(t: torch.Tensor) -> torch.Tensor:
    """t detached, as contiguous fp32: t's own storage where it is that already"""
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def is_stem(conv) -> bool:
    """the 7x7/s2/p3 conv over an RGB image: the layer that reads the NHWC4 input and has the dedicated stem kernels"""
    return conv.in_channels == 3 and conv.kernel_size[0] == 7 and conv.stride[0] == 2 and conv.padding[0] == 3


def require_pool2(m, who: str = "") -> None:
    """the only pool the YOLOv1 executors run: MaxPool2d(2,2)"""
    ks = m.kernel_size if isinstance(m.kernel_size, int) else m.kernel_size[0]
    st = m.stride if isinstance(m.stride, int) else m.stride[0]
    if ks != 2 or st != 2:
        raise ValueError(who + "only MaxPool2d(2,2)")


def stem_tiles_ok(Cout: int, Hout: int, Wout: int) -> bool:
    """the dedicated 7x7/s2 stem kernels (forward, weight gradient, fused pool backward) cover this output map: 64 channels in 8 x 16-pixel tiles"""
    return Cout == 64 and Hout % 8 == 0 and Wout % 16 == 0


class _Streams:
    """where the executors get their streams from (tests of the stream schedule put recording stand-ins here)"""

    @staticmethod
    def current(dev):
        return torch.cuda.current_stream(dev)

    @staticmethod
    def side(dev, low):
        return _hip.side_stream(torch.device(dev), low=low)

    @staticmethod
    def use(s):
        return torch.cuda.stream(s)


def side_stream(dev) -> "torch.cuda.Stream":
    """the second stream of a backward pass (weight gradients): one per device, shared by all plans (kept outside the plan
    objects, which are deep-copied with their modules)"""
    key = torch.device(dev).index
    if key not in RT._SIDE_STREAMS:
        RT._SIDE_STREAMS[key] = RT.STREAMS.side(dev, CFG.SIDE_LOW)
    return RT._SIDE_STREAMS[key]


class _on_side_stream:
    """``with _on_side_stream(main, side) as st:`` -- work issued inside goes to ``side`` (None: stays on ``main``), behind everything
    queued on ``main`` so far; ``st`` is the hipStream_t to launch on.  The caller joins with ``main.wait_stream(side)``.
    ``note(waiter, waited)``: told about the wait (the gradient reducer keeps track of which stream has seen which)."""

    def __init__(self, main_t, side_t, note=None):
        self.main_t, self.side_t, self.note = main_t, side_t, note

    def __enter__(self):
        if self.side_t is None:
            return ctypes.c_void_p(self.main_t.cuda_stream)
        self.side_t.wait_stream(self.main_t)
        if self.note is not None:
            self.note(self.side_t.cuda_stream, self.main_t.cuda_stream)
        self.ctx = RT.STREAMS.use(self.side_t)
        self.ctx.__enter__()
        return ctypes.c_void_p(self.side_t.cuda_stream)

    def __exit__(self, *exc):
        if self.side_t is not None:
            self.ctx.__exit__(*exc)
        return False


class _timed:
    def __init__(self, tag: str, kernel: str, flops: float = 0.0):
        self.tag, self.kernel, self.flops = tag, kernel, flops

    def __enter__(self):
        if CFG.TIMERS is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if CFG.TIMERS is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            CFG.TIMERS.append((self.tag, self.kernel, self.flops, self.e0, e1))
        return False


_SPLITK_SCRATCH: dict = {}


def _splitk_scratch(n: int, zero: bool) -> torch.Tensor:
    """fp32 scratch of n elements on the current device for a split-K launch (allocated once per device and grown on
    demand; the atomics form needs it zero-filled, the slab form does not)"""
    dev = torch.cuda.current_device()
    buf = _SPLITK_SCRATCH.get(dev)
    if buf is None or buf.numel() < n:
        buf = _SPLITK_SCRATCH[dev] = torch.empty(n, dtype=torch.float32, device=torch.device("cuda", dev))
    v = buf[:n]
    if zero:
        v.zero_()
    return v


_WGRAD_SLAB_BUF: dict = {}
_WGRAD_SLAB_OLD: list = []


def _attach_wgrad_slabs(L_, wd: WgradDesc, dev, st=None) -> None:
    """slab mode of the weight-gradient kernels (yolo_wgrad_desc.slabs): partial tiles as plain stores + a fixed-order sum
    instead of fp32 atomics.  One scratch per device AND per stream ``st`` (the hipStream_t the launch goes to; None: the current one), grown on
    demand: the launches of one stream use it one after the other, launches of two streams (the data-gradient chain and the weight-gradient
    stream of the backward pass) may be in flight together and never share it."""
    need = ctypes.c_long(0)
    check(L_.yolo_wgrad_slab_floats(ctypes.byref(wd), ctypes.byref(need)), "wgrad_slab_floats")
    if need.value <= 0:
        return
    if st is None:
        st = RT.stream()
    key = (torch.device(dev).index, getattr(st, "value", st) or 0)
    buf = _WGRAD_SLAB_BUF.get(key)
    if buf is None or buf.numel() < need.value:
        old = buf
        buf = _WGRAD_SLAB_BUF[key] = torch.empty(need.value, dtype=torch.float32, device=dev)
        if old is not None:
            # the smaller buffer may still be read by a launch in flight on ``st``, which is not necessarily torch's current stream:
            # keep it alive instead of handing it back to the allocator of another stream
            _WGRAD_SLAB_OLD.append(old)
    wd.slabs, wd.slab_floats = buf.data_ptr(), buf.numel()


class _EventSlot:
    """holder of the event behind a background optimizer launch (yolo.optim.Adam.attach_plan(overlap=True)).  It lives on the plan
    object (not in a table keyed by id(plan), which outlives garbage collection); a deep copy of a plan starts with an empty slot --
    events do not copy, and the copy's parameters are new tensors nobody updates in the background."""

    def __init__(self):
        self.event = None

    def __deepcopy__(self, memo):
        return _EventSlot()

    def __reduce__(self):
        return (_EventSlot, ())

    def wait(self, dev=None, keep: bool = False):
        """the current stream waits for the pending update; ``keep``: leave the event in place for later readers on other streams"""
        ev = self.event
        if not keep:
            self.event = None
        if ev is not None:
            torch.cuda.current_stream(dev).wait_event(ev)


class Act:
    """Zero-haloed NHWC bf16 activation: [N][H+2h][W+2h][C] plus guard bands of zeros."""

    def __init__(self, N, H, W, C, halo, device, halo_hi=None):
        self.N, self.H, self.W, self.C = N, H, W, C
        self.halo = halo
        self.halo_hi = halo if halo_hi is None else halo_hi
        self.Hp = H + self.halo + self.halo_hi
        self.Wp = W + self.halo + self.halo_hi
        self.px_stride = C
        self.row_stride = self.Wp * C
        self.img_stride = self.Hp * self.Wp * C
        self.slots = N * self.Hp * self.Wp
        guard = _round_up((self.Wp + 2) * C + 64 * 8, 128)
        self.store = torch.zeros(guard + self.slots * C + guard, dtype=torch.bfloat16, device=device)
        self.t = self.store[guard: guard + self.slots * C]

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def interior_off(self, shift=0):
        """element offset of logical pixel (-shift, -shift) inside an image"""
        h = self.halo - shift
        return (h * self.Wp + h) * self.C

    def view(self):
        return self.t.view(self.N, self.Hp, self.Wp, self.C)

    def interior(self):
        h = self.halo
        return self.view()[:, h: h + self.H, h: h + self.W, :]




class _Runtime:
    """patchable hooks: the library, the current HIP stream, the stream factory, the split-K scratch pool, the side streams per device"""

    def __init__(self):
        self.lib = _hip.lib
        self.stream = _hip.stream
        self.STREAMS = _Streams()
        self._SIDE_STREAMS: dict = {}
        self._splitk_scratch = _splitk_scratch


RT = _Runtime()
HOOKS = frozenset(("lib", "stream", "STREAMS", "_SIDE_STREAMS", "_splitk_scratch"))
