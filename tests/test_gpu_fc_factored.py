"""The factored Linear gradient (EngineConfig.FC_FACTORED) on the device: the five entries of csrc/fc_factored.hip / optim.hip / sgd.hip through the C
ABI against tests/fc_factored_ref.py (fp64), then the plan, the optimizers, determinism across processes and two ranks over gloo.

Bounds (fc_factored_ref.py has the reasoning): products of bf16 values are exact in fp32, so G = scale * dy^T x errs by at most
(rows - 1 + [scale not a power of two]) * 1.01 u * scale * |dy|^T |x| per element; |G|^2 from the Gram matrices by at most
scale^2 (2.02 c u + 1e-12) sum |A| o |B| with c = YOLO_FC_GRAM_CHAIN.  The step entries are fed the G the gradient entry stored -- the same bits by
construction (one device function, one multiply) -- through elementwise_ref.adam_ref / sgd_ref.sgd_ref: Adam is sign(g)-like near zero at step 1,
so no bound exists against a gradient from another summation order.  Every output lies between guard bands of a NaN pattern and starts as NaN
where the entry must store every element."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import elementwise_ref as er
import fc_factored_ref as fr
import launch_ref as lr
import sgd_ref as sr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
Guarded = er.Guarded
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MAX_NORM = 1e-3, 10.0
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=5e-4)
PAPER = dict(momentum=0.9, dampening=0.0, nesterov=False, wd=5e-4)
NORMS = {"null": None, "inactive": 1.0, "active": (10.0 / 0.37) ** 2}
E_ARG, E_UNSUPPORTED = -1, -2


def _lib():
    from yolo._hip import lib
    return lib()


def _stream():
    from yolo._hip import stream
    return stream()


def _last_error():
    return _lib().yolo_hip_last_error().decode(errors="replace")


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Case:
    """the factors of one shape on the device between guard bands, their descriptor, and the fp64 reference (computed once per shape and scale)"""

    _cache: dict = {}

    def __init__(self, rows, O, I, scale, seed=0):
        from yolo._hip import FcFactors
        self.rows, self.O, self.I, self.scale = rows, O, I, fr.f32(scale)
        dy, x = fr.factors(rows, O, I, seed + rows * 7 + O, device="cuda")
        self.DY, self.X = Guarded(dy), Guarded(x)
        self.dy, self.x = self.DY.t.view(dy.shape), self.X.t.view(x.shape)
        self.desc = FcFactors(self.DY.ptr, self.X.ptr, rows, O, I, dy.shape[1], x.shape[1], self.scale)
        self.G64, self.Gabs = fr.grad_ref(self.dy, self.x, O, I, scale)
        self.bound = fr.grad_bound(self.Gabs, rows, scale)

    @classmethod
    def get(cls, rows, O, I, scale):
        key = (rows, O, I, fr.f32(scale))
        if key not in cls._cache:
            cls._cache[key] = cls(rows, O, I, scale)
        return cls._cache[key]

    def grad(self):
        """G as yolo_fc_factored_grad stores it (a Guarded fp32 buffer that started as NaN)"""
        out = Guarded(torch.full((self.O * self.I,), float("nan"), dtype=torch.float32, device="cuda"))
        rc = _lib().yolo_fc_factored_grad(ctypes.byref(self.desc), ctypes.c_void_p(out.ptr), _stream())
        assert rc == 0, _last_error()
        torch.cuda.synchronize()
        return out

    def inputs_intact(self):
        return self.DY.guards_ok() and self.X.guards_ok()


def _scale_id(s):
    return {1.0: "s1", 0.5: "s0.5"}.get(s, "s1/3")


# ---- 1. the gradient entry ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", fr.SCALES, ids=_scale_id)
@pytest.mark.parametrize("rows,O,I", fr.SHAPES)
def test_grad_entry_against_fp64(rows, O, I, scale):
    c = Case.get(rows, O, I, scale)
    a, b = c.grad(), c.grad()
    fails = []
    worst = lr.check_values(c.G64, c.bound, a.t, "G", fails, f"rows {rows} O {O} I {I} scale {scale:.4g}")
    print(f"rows {rows} O {O} I {I} scale {scale:.4g}: worst |err| / bound {worst:.3f}")
    if not (a.guards_ok() and b.guards_ok() and c.inputs_intact()):
        fails.append("a guard band was overwritten")
    if not torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)):
        fails.append("two launches differ in some bits")
    assert not fails, "\n".join(fails)


# ---- 2. the squared norm --------------------------------------------------------------------------------------------------------------------------

def _sumsq(c, acc0=3.25, short=0):
    need = ctypes.c_long(0)
    rc = _lib().yolo_fc_factored_sumsq_slots(ctypes.byref(c.desc), ctypes.byref(need))
    assert rc == 0 and need.value > 0, _last_error()
    scratch = Guarded(torch.full((need.value - short,), -7.0, dtype=torch.float64, device="cuda").view(torch.float32))
    acc = torch.full((1,), acc0, dtype=torch.float64, device="cuda")
    rc = _lib().yolo_fc_factored_sumsq(ctypes.byref(c.desc), ctypes.c_void_p(scratch.ptr), need.value - short, _vp(acc), _stream())
    torch.cuda.synchronize()
    return rc, acc, scratch


@pytest.mark.parametrize("scale", fr.SCALES, ids=_scale_id)
@pytest.mark.parametrize("rows,O,I", fr.SHAPES)
def test_sumsq_entry_against_fp64(rows, O, I, scale):
    from yolo._hip import FC_GRAM_CHAIN
    c = Case.get(rows, O, I, scale)
    ref, bnd = fr.sumsq_ref(c.dy, c.x, O, I, scale, FC_GRAM_CHAIN)
    direct = float((c.G64 ** 2).sum())
    assert abs(direct - ref) <= 1e-11 * abs(ref)                       # the identity itself, in fp64
    rc, acc, scratch = _sumsq(c)
    assert rc == 0, _last_error()
    rc2, acc2, _ = _sumsq(c)
    assert rc2 == 0, _last_error()
    got = float(acc) - 3.25
    print(f"rows {rows} O {O} I {I} scale {scale:.4g}: |err| / bound {abs(got - ref) / bnd:.4f} (|G|^2 = {ref:.6g})")
    assert abs(got - ref) <= bnd + 3.25 * 2.0 ** -52, (got, ref, bnd)
    assert torch.equal(acc.view(torch.int64), acc2.view(torch.int64)), "two launches differ as doubles"
    assert scratch.guards_ok() and c.inputs_intact()


def test_sumsq_refuses_a_short_scratch():
    c = Case.get(64, 136, 200, 1.0)
    rc, acc, scratch = _sumsq(c, short=1)
    assert rc == E_ARG and "yolo_fc_factored_sumsq" in _last_error()
    assert float(acc) == 3.25
    assert bool((scratch.t.view(torch.float64) == -7.0).all()) and scratch.guards_ok()


# ---- 3. the step entries --------------------------------------------------------------------------------------------------------------------------

def _state(c, seed, with_buf):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = c.O * c.I
    p = torch.randn(n, generator=gen, dtype=torch.float32, device="cuda")
    z = torch.zeros(n, dtype=torch.float32, device="cuda")
    return (p, z.clone()) if with_buf else (p, z.clone(), z.clone())


def _adam_call(c, P, M, V, PB, step, norm, skip, wg):
    rc = _lib().yolo_adam_step_factored(ctypes.byref(c.desc), ctypes.c_void_p(P.ptr), ctypes.c_void_p(M.ptr), ctypes.c_void_p(V.ptr),
                                        ctypes.c_void_p(PB.ptr) if PB is not None else None, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"],
                                        ADAM["wd"], step, _vp(norm), MAX_NORM, _vp(skip), wg, _stream())
    assert rc == 0, _last_error()


def _sgd_call(c, P, B, PB, first, norm, skip, wg, h=PAPER):
    rc = _lib().yolo_sgd_step_factored(ctypes.byref(c.desc), ctypes.c_void_p(P.ptr), ctypes.c_void_p(B.ptr) if B is not None else None,
                                       ctypes.c_void_p(PB.ptr) if PB is not None else None, LR, h["momentum"], h["dampening"], h["wd"],
                                       int(h["nesterov"]), int(first), _vp(norm), MAX_NORM, _vp(skip), wg, _stream())
    assert rc == 0, _last_error()


def _bits(*gs):
    return torch.cat([g.t.view(torch.int32) for g in gs])


@pytest.mark.parametrize("norm_id", list(NORMS))
@pytest.mark.parametrize("k,shape", list(enumerate(fr.SHAPES)), ids=[f"{r}x{o}x{i}" for r, o, i in fr.SHAPES])
def test_adam_step_entry(k, shape, norm_id):
    rows, O, I = shape
    scale = fr.SCALES[k % 3]
    c = Case.get(rows, O, I, scale)
    G = c.grad().t.clone()
    norm_sq = NORMS[norm_id]
    norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda") if norm_sq is not None else None
    p0, m0, v0 = _state(c, 11 + k, False)
    fails, results = [], {}
    for wg in (0, 8, 1):
        P, M, V = Guarded(p0), Guarded(m0), Guarded(v0)
        PB = Guarded(torch.zeros(p0.numel(), dtype=BF, device="cuda"), BF)
        for step in (1, 2, 3):                                   # state carried: every step judged from the state the kernel left before it
            pb, mb, vb = P.t.clone(), M.t.clone(), V.t.clone()
            _adam_call(c, P, M, V, PB, step, norm, None, wg)
            torch.cuda.synchronize()
            (rp, rm, rv), (bp, bm, bv) = er.adam_ref(pb, G, mb, vb, step=step, norm_sq=norm_sq, max_norm=MAX_NORM, **ADAM)
            tag = f"wg {wg} step {step}"
            worst = max(lr.check_values(rp, bp, P.t, "p", fails, tag), lr.check_values(rm, bm, M.t, "exp_avg", fails, tag),
                        lr.check_values(rv, bv, V.t, "exp_avg_sq", fails, tag))
            if not torch.equal(PB.t.view(torch.int16), sr.bf16_bits(P.t)):
                fails.append(f"{tag}: bf16 shadow != bf16(p)")
            if wg == 0:
                print(f"{shape} {norm_id} {tag}: worst |err| / bound {worst:.3f}")
        if not all(X.guards_ok() for X in (P, M, V, PB)):
            fails.append(f"wg {wg}: a guard band was overwritten")
        results[wg] = torch.cat([_bits(P, M, V), PB.t.view(torch.int16).int()])
    for wg in (8, 1):
        if not torch.equal(results[0], results[wg]):
            fails.append(f"workgroups {wg} and 0 differ in some bits")
    if not c.inputs_intact():
        fails.append("a factor was written")
    assert not fails, "\n".join(fails[:12])


@pytest.mark.parametrize("norm_id", list(NORMS))
@pytest.mark.parametrize("k,shape", list(enumerate(fr.SHAPES)), ids=[f"{r}x{o}x{i}" for r, o, i in fr.SHAPES])
def test_sgd_step_entry(k, shape, norm_id):
    rows, O, I = shape
    scale = fr.SCALES[(k + 1) % 3]
    c = Case.get(rows, O, I, scale)
    G = c.grad().t.clone()
    norm_sq = NORMS[norm_id]
    norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda") if norm_sq is not None else None
    p0, b0 = _state(c, 23 + k, True)
    fails, results = [], {}
    for wg in (0, 8, 1):
        P, B = Guarded(p0), Guarded(b0)
        PB = Guarded(torch.zeros(p0.numel(), dtype=BF, device="cuda"), BF)
        for step in (1, 2, 3):
            pb, bb = P.t.clone(), B.t.clone()
            _sgd_call(c, P, B, PB, step == 1, norm, None, wg)
            torch.cuda.synchronize()
            (rp, rb), (bp, bbuf) = sr.sgd_ref(pb, G, bb, lr=LR, first_step=step == 1, norm_sq=norm_sq, max_norm=MAX_NORM, **PAPER)
            tag = f"wg {wg} step {step}"
            worst = max(lr.check_values(rp, bp, P.t, "p", fails, tag), lr.check_values(rb, bbuf, B.t, "momentum_buffer", fails, tag))
            if not torch.equal(PB.t.view(torch.int16), sr.bf16_bits(P.t)):
                fails.append(f"{tag}: bf16 shadow != bf16(p)")
            if wg == 0:
                print(f"{shape} {norm_id} {tag}: worst |err| / bound {worst:.3f}")
        if not all(X.guards_ok() for X in (P, B, PB)):
            fails.append(f"wg {wg}: a guard band was overwritten")
        results[wg] = torch.cat([_bits(P, B), PB.t.view(torch.int16).int()])
    for wg in (8, 1):
        if not torch.equal(results[0], results[wg]):
            fails.append(f"workgroups {wg} and 0 differ in some bits")
    assert not fails, "\n".join(fails[:12])


def test_sgd_step_entry_without_momentum_leaves_buf_alone():
    c = Case.get(5, 136, 200, 1.0)
    G = c.grad().t.clone()
    p0, b0 = _state(c, 5, True)
    b0.fill_(0.25)
    h = dict(momentum=0.0, dampening=0.0, nesterov=False, wd=0.0)
    P, B = Guarded(p0), Guarded(b0)
    _sgd_call(c, P, B, None, 0, None, None, 0, h)
    torch.cuda.synchronize()
    (rp, _), (bp, _) = sr.sgd_ref(p0, G, None, lr=LR, first_step=False, norm_sq=None, max_norm=MAX_NORM, **h)
    fails = []
    lr.check_values(rp, bp, P.t, "p", fails, "no momentum")
    assert not fails, fails
    assert torch.equal(B.t, b0) and P.guards_ok() and B.guards_ok()


@pytest.mark.parametrize("entry", ["adam", "sgd"])
def test_skip_flag_writes_nothing(entry):
    c = Case.get(80, 136, 200, 0.5)
    skip = torch.ones(1, dtype=torch.float32, device="cuda")
    PB0 = torch.full((c.O * c.I,), 1.5, dtype=BF, device="cuda")
    if entry == "adam":
        p0, m0, v0 = _state(c, 3, False)
        bufs = [Guarded(p0), Guarded(m0), Guarded(v0)]
        PB = Guarded(PB0, BF)
        for wg in (0, 8):
            _adam_call(c, *bufs, PB, 1, None, skip, wg)
        starts = [p0, m0, v0]
    else:
        p0, b0 = _state(c, 3, True)
        bufs = [Guarded(p0), Guarded(b0)]
        PB = Guarded(PB0, BF)
        for wg in (0, 8):
            _sgd_call(c, *bufs, PB, 1, None, skip, wg)
        starts = [p0, b0]
    torch.cuda.synchronize()
    for X, s in zip(bufs, starts):
        assert torch.equal(X.t.view(torch.int32), s.view(torch.int32)) and X.guards_ok()
    assert torch.equal(PB.t.view(torch.int16), PB0.view(torch.int16)) and PB.guards_ok()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------

def refusal_descs(dy_ptr, x_ptr, rows=64, O=136, I=200):
    """(name, descriptor, expected code) of every refusal of section 1 of the descriptor alone"""
    from yolo._hip import FC_MAX_ROWS, FcFactors
    ld = fr.round_up(O, 32)
    return [("I % 8", FcFactors(dy_ptr, x_ptr, rows, O, 196, ld, 200, 1.0), E_UNSUPPORTED),
            ("ld_dy % 8", FcFactors(dy_ptr, x_ptr, rows, O, I, O + 4, I, 1.0), E_UNSUPPORTED),
            ("ld_x % 8", FcFactors(dy_ptr, x_ptr, rows, O, I, ld, I + 4, 1.0), E_UNSUPPORTED),
            ("dy misaligned", FcFactors(dy_ptr + 2, x_ptr, rows, O, I, ld, I, 1.0), E_UNSUPPORTED),
            ("x misaligned", FcFactors(dy_ptr, x_ptr + 8, rows, O, I, ld, I, 1.0), E_UNSUPPORTED),
            ("rows > max", FcFactors(dy_ptr, x_ptr, FC_MAX_ROWS + 1, O, I, ld, I, 1.0), E_UNSUPPORTED),
            ("rows 0", FcFactors(dy_ptr, x_ptr, 0, O, I, ld, I, 1.0), E_ARG),
            ("ld_dy < O", FcFactors(dy_ptr, x_ptr, rows, O, I, 128, I, 1.0), E_ARG),
            ("null x", FcFactors(dy_ptr, None, rows, O, I, ld, I, 1.0), E_ARG)]


def refused_calls(L, d, out_ptr, scratch_ptr, acc_ptr, stream):
    """every entry called with descriptor d -> [(entry name, return code)]; out_ptr: >= 3 * O * I floats (p / m / v or g_out), 16-B aligned"""
    n = d.O * d.I * 4 if d.O > 0 and d.I > 0 else 0
    p, m, v = out_ptr, out_ptr + n, out_ptr + 2 * n
    c = ctypes.c_void_p
    need = ctypes.c_long(-5)
    return [("yolo_fc_factored_grad", L.yolo_fc_factored_grad(ctypes.byref(d), c(p), stream)),
            ("yolo_fc_factored_sumsq_slots", L.yolo_fc_factored_sumsq_slots(ctypes.byref(d), ctypes.byref(need))),
            ("yolo_fc_factored_sumsq", L.yolo_fc_factored_sumsq(ctypes.byref(d), c(scratch_ptr), 1 << 20, c(acc_ptr), stream)),
            ("yolo_adam_step_factored", L.yolo_adam_step_factored(ctypes.byref(d), c(p), c(m), c(v), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 10.0, None, 0,
                                                                  stream)),
            ("yolo_sgd_step_factored", L.yolo_sgd_step_factored(ctypes.byref(d), c(p), c(m), None, 1e-3, 0.9, 0.0, 0.0, 0, 1, None, 10.0, None, 0, stream))]


def test_refusals_launch_nothing():
    L = _lib()
    c = Case.get(64, 136, 200, 1.0)
    n = 136 * 200
    out = Guarded(torch.full((3 * n,), float("nan"), dtype=torch.float32, device="cuda"))
    scratch = torch.full((1 << 20,), -7.0, dtype=torch.float64, device="cuda")
    acc = torch.full((1,), 3.25, dtype=torch.float64, device="cuda")
    fails = []
    for name, d, code in refusal_descs(c.DY.ptr, c.X.ptr):
        for entry, rc in refused_calls(L, d, out.ptr, scratch.data_ptr(), acc.data_ptr(), _stream()):
            # (a call is checked right behind itself: yolo_hip_last_error is the calling thread's last message)
            if rc != code:
                fails.append(f"{name}: {entry} returned {rc}, expected {code}")
    # the message names the entry: one call at a time
    for name, d, code in refusal_descs(c.DY.ptr, c.X.ptr)[:2]:
        assert L.yolo_fc_factored_grad(ctypes.byref(d), ctypes.c_void_p(out.ptr), _stream()) == code and "yolo_fc_factored_grad" in _last_error()
        assert L.yolo_adam_step_factored(ctypes.byref(d), ctypes.c_void_p(out.ptr), ctypes.c_void_p(out.ptr + 4 * n), ctypes.c_void_p(out.ptr + 8 * n), None, 1e-3,
                                         0.9, 0.999, 1e-8, 0.0, 1, None, 10.0, None, 0, _stream()) == code and "yolo_adam_step_factored" in _last_error()
        assert L.yolo_sgd_step_factored(ctypes.byref(d), ctypes.c_void_p(out.ptr), ctypes.c_void_p(out.ptr + 4 * n), None, 1e-3, 0.9, 0.0, 0.0, 0, 1, None, 10.0,
                                        None, 0, _stream()) == code and "yolo_sgd_step_factored" in _last_error()
        assert L.yolo_fc_factored_sumsq(ctypes.byref(d), _vp(scratch), 1 << 20, _vp(acc), _stream()) == code and "yolo_fc_factored_sumsq" in _last_error()
    # misaligned outputs and state, a negative grid, a bad step
    good = c.desc
    vp = ctypes.c_void_p
    more = [("g_out misaligned", L.yolo_fc_factored_grad(ctypes.byref(good), vp(out.ptr + 4), _stream()), E_UNSUPPORTED),
            ("p misaligned", L.yolo_adam_step_factored(ctypes.byref(good), vp(out.ptr + 4), vp(out.ptr + 4 * n), vp(out.ptr + 8 * n), None, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                                       1, None, 10.0, None, 0, _stream()), E_UNSUPPORTED),
            ("shadow misaligned", L.yolo_sgd_step_factored(ctypes.byref(good), vp(out.ptr), vp(out.ptr + 4 * n), vp(out.ptr + 8 * n + 2), 1e-3, 0.9, 0.0, 0.0, 0, 1,
                                                           None, 10.0, None, 0, _stream()), E_UNSUPPORTED),
            ("workgroups < 0", L.yolo_adam_step_factored(ctypes.byref(good), vp(out.ptr), vp(out.ptr + 4 * n), vp(out.ptr + 8 * n), None, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                                         1, None, 10.0, None, -1, _stream()), E_ARG),
            ("step 0", L.yolo_adam_step_factored(ctypes.byref(good), vp(out.ptr), vp(out.ptr + 4 * n), vp(out.ptr + 8 * n), None, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                                 0, None, 10.0, None, 0, _stream()), E_ARG),
            ("null acc", L.yolo_fc_factored_sumsq(ctypes.byref(good), _vp(scratch), 1 << 20, None, _stream()), E_ARG)]
    fails += [f"{name}: returned {rc}, expected {code}" for name, rc, code in more if rc != code]
    torch.cuda.synchronize()
    assert not fails, "\n".join(fails)
    assert bool(torch.isnan(out.t).all()) and out.guards_ok(), "a refused call wrote its output"
    assert bool((scratch == -7.0).all()) and float(acc) == 3.25


def test_rows_at_the_documented_maximum():
    """rows = YOLO_FC_MAX_ROWS: the K panels take 133 KB of LDS, beyond the default limit of a launch -- the path that raises it, for every kernel"""
    from yolo._hip import FC_GRAM_CHAIN, FC_MAX_ROWS
    c = Case.get(FC_MAX_ROWS, 72, 136, 0.5)
    g = c.grad()
    fails = []
    worst = lr.check_values(c.G64, c.bound, g.t, "G", fails, "rows 512")
    ref, bnd = fr.sumsq_ref(c.dy, c.x, c.O, c.I, c.scale, FC_GRAM_CHAIN)
    rc, acc, _ = _sumsq(c)
    assert rc == 0, _last_error()
    print(f"rows {FC_MAX_ROWS}: G worst |err| / bound {worst:.3f}, |G|^2 |err| / bound {abs(float(acc) - 3.25 - ref) / bnd:.4f}")
    assert abs(float(acc) - 3.25 - ref) <= bnd + 3.25 * 2.0 ** -52
    G = g.t.clone()
    p0, m0, v0 = _state(c, 1, False)
    P, M, V = Guarded(p0), Guarded(m0), Guarded(v0)
    _adam_call(c, P, M, V, None, 1, None, None, 8)
    P2, B2 = Guarded(p0), Guarded(m0)
    _sgd_call(c, P2, B2, None, 1, None, None, 0)
    torch.cuda.synchronize()
    (rp, rm, rv), (bp, bm, bv) = er.adam_ref(p0, G, m0, v0, step=1, norm_sq=None, max_norm=MAX_NORM, **ADAM)
    lr.check_values(rp, bp, P.t, "p", fails, "adam rows 512")
    lr.check_values(rv, bv, V.t, "exp_avg_sq", fails, "adam rows 512")
    (rp, rb), (bp, bb) = sr.sgd_ref(p0, G, m0, lr=LR, first_step=True, norm_sq=None, max_norm=MAX_NORM, **PAPER)
    lr.check_values(rp, bp, P2.t, "p", fails, "sgd rows 512")
    lr.check_values(rb, bb, B2.t, "momentum_buffer", fails, "sgd rows 512")
    assert not fails, "\n".join(fails)
    assert all(X.guards_ok() for X in (g, P, M, V, P2, B2))


# ---- 5. the plan and the optimizers -----------------------------------------------------------------------------------------------------------------

import factored_child as fch  # noqa: E402


@pytest.fixture
def factored(monkeypatch):
    """EngineConfig.FC_FACTORED on with the threshold of the small model: Linear(1024, 256) qualifies, Linear(256, 24) does not"""
    from yolo.config import CONFIG
    monkeypatch.setattr(CONFIG, "FC_FACTORED", True)
    monkeypatch.setattr(CONFIG, "FC_FACTORED_MIN", fch.FC_MIN)
    return CONFIG


def _backward(mods, plan, x, gy):
    for p in mods.parameters():
        p.grad = None
    fch.loss_of(plan, x, gy).backward()


def _pair_bound(rec, w, rows):
    """(G64, bound of the factored gradient + bound of the dense yolo_wgrad launch) from the plan's own factors.  Dense: launch_ref.wgrad_bound's
    gamma(P + R - 1) S with P = rows pixel slots and R = 1 range (the Linear layers' descriptor has split = 1)"""
    O, I = w.shape
    G64, Gabs = fr.grad_ref(rec.dy, rec.x, O, I, rec.scale)
    return G64, Gabs, fr.grad_bound(Gabs, rec.rows, rec.scale) + lr.gamma(rows) * rec.scale * Gabs


def test_plan_records_factors_and_materialises_the_gradient(factored):
    mods = fch.small_model(0)
    plan = fch.make_plan(mods)
    x, gy = fch.small_batch()
    _backward(mods, plan, x, gy)
    w1, w2 = mods[3].weight, mods[6].weight
    assert w1.grad is None and w2.grad is not None and mods[3].bias.grad is not None
    rec = plan.fc_factors[id(w1)]
    assert list(plan.fc_factors) == [id(w1)] and rec.rows == fch.BATCH and rec.scale == 1.0
    assert rec.dy.shape == (fch.BATCH, 256) and rec.x.shape == (fch.BATCH, 1024) and id(w1) not in plan.grad_norm_sq
    g = plan.fc_weight_grad(w1)
    G64, Gabs = fr.grad_ref(rec.dy, rec.x, 256, 1024, 1.0)
    fails = []
    worst = lr.check_values(G64, fr.grad_bound(Gabs, rec.rows, 1.0), g, "fc_weight_grad", fails, "plan")
    print(f"plan.fc_weight_grad: worst |err| / bound {worst:.3f}")
    assert not fails, fails
    assert torch.equal(g, plan.fc_weight_grad(w1)) and id(w1) in plan.fc_factors           # on request, as often as asked
    # the bias gradient of the factored layer is the dense path's: the column sum of the same dy
    db64 = rec.dy[:, :256].double().sum(0)
    assert float((mods[3].bias.grad.double() - db64).abs().max()) <= lr.gamma(fch.BATCH) * float(rec.dy[:, :256].double().abs().sum(0).max())
    with pytest.raises(RuntimeError, match="no pending factored gradient"):
        plan.fc_weight_grad(w2)


def _one_step(kind, switch_on, monkeypatch, overlap=False, between=None):
    """one step of the small model from seed 0 -> (modules, optimizer, plan, the factors' record or None)"""
    from yolo.config import CONFIG
    from yolo.optim import SGD, Adam
    monkeypatch.setattr(CONFIG, "FC_FACTORED", switch_on)
    monkeypatch.setattr(CONFIG, "FC_FACTORED_MIN", fch.FC_MIN)
    mods = fch.small_model(0)
    plan = fch.make_plan(mods)
    if kind == "sgd":
        opt = SGD(mods.parameters(), lr=0.5, momentum=0.9, max_grad_norm=1e6)        # the clip is computed and inactive (c = 1): SGD stays linear in g
    else:
        opt = Adam(mods.parameters(), lr=1e-3, max_grad_norm=1e6)
    opt.attach_plan(plan, overlap=overlap)
    x, gy = fch.small_batch()
    _backward(mods, plan, x, gy)
    rec = plan.fc_factors.get(id(mods[3].weight))
    if between is not None:
        between(plan)
    opt.step()
    if between is not None:
        between(plan)                    # ... and beside a background pass
    opt.synchronize()
    torch.cuda.synchronize()
    return mods, opt, plan, rec


def test_sgd_step_factored_against_dense(monkeypatch):
    """SGD with momentum, first step, clip inactive, no weight decay: buf = g and p' = fma(-lr, g, p).  SGD is linear in g, so the two runs differ by
    |buf_f - buf_d| <= bound(factored) + bound(dense wgrad) and |p_f - p_d| <= lr * that + the one rounding each run gives its own p'
    (2 * 1.01 u |p'|: without it a difference far below an ulp of p could never flip a rounding).  Every other tensor is bit-equal."""
    md, od, _, _ = _one_step("sgd", False, monkeypatch)
    mf, of, plan, rec = _one_step("sgd", True, monkeypatch)
    assert rec is not None and not plan.fc_factors, "the step consumes the record"
    wd_, wf = md[3].weight, mf[3].weight
    assert wf.grad is None and wd_.grad is not None
    G64, Gabs, bnd = _pair_bound(rec, wf, fch.BATCH)
    db = (of.state[wf]["momentum_buffer"].double() - od.state[wd_]["momentum_buffer"].double()).abs()
    dp = (wf.detach().double() - wd_.detach().double()).abs()
    bp = 0.5 * bnd + 2 * er.RND * wf.detach().double().abs()
    print(f"sgd factored vs dense: buf worst {float((db / bnd.clamp_min(1e-300)).max()):.3f}, p worst {float((dp / bp).max()):.3f} of the bound; "
          f"{int((dp > 0).sum())} of {dp.numel()} weights differ")
    assert bool((db <= bnd).all()) and bool((dp <= bp).all())
    for (n, a), (_, b) in zip(md.named_parameters(), mf.named_parameters()):
        if a is not wd_:
            assert torch.equal(a, b), n
            assert torch.equal(od.state[a]["momentum_buffer"], of.state[b]["momentum_buffer"]), n


def test_adam_step_factored_against_dense(monkeypatch):
    """first Adam step: exp_avg = (1 - beta1) g, linear in g -> within (1 - beta1) times the bound of the SGD test; every other tensor bit-equal"""
    md, od, _, _ = _one_step("adam", False, monkeypatch)
    mf, of, plan, rec = _one_step("adam", True, monkeypatch)
    wd_, wf = md[3].weight, mf[3].weight
    _, _, bnd = _pair_bound(rec, wf, fch.BATCH)
    dm = (of.state[wf]["exp_avg"].double() - od.state[wd_]["exp_avg"].double()).abs()
    omb1 = er.adam_constants(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)["omb1"]
    print(f"adam factored vs dense: exp_avg worst {float((dm / (omb1 * bnd).clamp_min(1e-300)).max()):.3f} of the bound")
    assert bool((dm <= omb1 * bnd).all())
    assert int(of.state[wf]["step"]) == 1 and bool(torch.isfinite(wf).all())
    for (n, a), (_, b) in zip(md.named_parameters(), mf.named_parameters()):
        if a is not wd_:
            assert torch.equal(a, b), n
            assert torch.equal(od.state[a]["exp_avg_sq"], of.state[b]["exp_avg_sq"]), n


@pytest.mark.parametrize("overlap", [False, True], ids=["foreground", "background"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_factors_outlive_the_next_forward(monkeypatch, kind, overlap):
    """Lifetime: the record owns its factors.  Training forwards at another batch size and at the same one (which rewrites the very flatten buffer
    the factors were copied from) between backward() and step(), and again right behind a step whose Linear update may still run on the second
    stream, leave the updated weights bit-equal to the run without them."""
    from yolo import engine, optim
    monkeypatch.setattr(optim, "OVERLAP", overlap)

    def other_forwards(plan):
        for n, seed in ((4, 91), (fch.BATCH, 92)):
            xo, _ = fch.small_batch(n, seed)
            with torch.enable_grad():
                engine.run_plan(plan, xo * 3.0, True)

    ma, oa, _, _ = _one_step(kind, True, monkeypatch, overlap=overlap)
    mb, ob, _, _ = _one_step(kind, True, monkeypatch, overlap=overlap, between=other_forwards)
    assert bool(oa.deferred) == overlap
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), n
        for k, v in oa.state[a].items():
            if torch.is_tensor(v):
                assert torch.equal(v, ob.state[b][k]), (n, k)


def test_what_refuses_the_switch(factored):
    from yolo.optim import LARS, Adam, GradAccumulator
    mods = fch.small_model(0)
    plan = fch.make_plan(mods)
    x, gy = fch.small_batch()
    _backward(mods, plan, x, gy)
    with pytest.raises(RuntimeError, match=r"FC_FACTORED.*LARS"):
        LARS(mods.parameters(), lr=1e-3).step()
    with pytest.raises(RuntimeError, match=r"FC_FACTORED.*GradAccumulator"):
        GradAccumulator(mods, 2)
    GradAccumulator(mods, 1)                       # steps == 1 allocates and launches nothing: fine
    cpu = fch.small_model(0, device="cpu")
    for p in cpu.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match=r"FC_FACTORED.*CPU parameters"):
        Adam(cpu.parameters(), lr=1e-3).step()


def test_arena_leaves_the_factored_gradient_out(factored):
    mods = fch.small_model(0)
    plan = fch.make_plan(mods)
    arena = plan.attach_grad_arena(torch.device("cuda"))
    n_other = sum(p.numel() for p in mods.parameters()) - mods[3].weight.numel()
    assert n_other <= arena.numel() < n_other + 64 * 8, (arena.numel(), n_other)        # every view rounded up to 64 elements, FC1's dw absent
    x, gy = fch.small_batch()
    _backward(mods, plan, x, gy)
    assert mods[3].weight.grad is None and mods[6].weight.grad is not None and id(mods[3].weight) in plan.fc_factors


# ---- 6. determinism across processes ----------------------------------------------------------------------------------------------------------------

def _child(args, timeout=300, **extra_env):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra_env)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


CHILD = os.path.join(ROOT, "tests", "factored_child.py")


def test_two_fresh_processes_print_the_same_hashes(tmp_path):
    outs = []
    for k in range(2):
        f = tmp_path / f"h{k}.txt"
        _child([CHILD, "det", str(f)], YOLO_AMD_DETERMINISTIC="1", YOLO_AMD_FC_FACTORED="1", YOLO_AMD_FC_FACTORED_MIN=str(fch.FC_MIN))
        outs.append(f.read_text().split())
    assert len(outs[0]) == 3 and len(set(outs[0])) == 3 and outs[0] == outs[1], outs


# ---- 7. two ranks on one GPU over gloo ----------------------------------------------------------------------------------------------------------------

def test_two_ranks_factored_against_dense(tmp_path):
    res = {}
    for k, on in enumerate(("0", "1")):
        out = tmp_path / f"two{on}.pt"
        port = 29300 + os.getpid() % 300 + 300 * k
        _child(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port), CHILD, "gloo2",
                str(out)], timeout=600, YOLO_AMD_FC_FACTORED=on, YOLO_AMD_FC_FACTORED_MIN=str(fch.FC_MIN))
        res[on] = [torch.load(f"{out}.r{r}", weights_only=True) for r in (0, 1)]
    d0, d1 = res["0"]
    f0, f1 = res["1"]
    assert f0["factored"] and not d0["factored"] and f0["w1_grad_is_none"] and not d0["w1_grad_is_none"]
    for a, b in ((d0, d1), (f0, f1)):                          # replicas are bit-identical to each other
        for n in a["params"]:
            assert torch.equal(a["params"][n], b["params"][n]) and torch.equal(a["buf"][n], b["buf"][n]), n
    # the reducer's arena does not contain FC1's dw; the wire carries the gathered factors instead
    assert d0["arena_numel"] - f0["arena_numel"] == f0["w1_numel"] and d0["payload_bytes"] == 4 * d0["arena_numel"]
    assert f0["payload_bytes"] == 4 * f0["arena_numel"] + 2 * fch.BATCH * (256 + 1024)
    print(f"bytes on the wire per step, two ranks, small model: dense {d0['payload_bytes']}, factored {f0['payload_bytes']}")
    assert f0["rows"] == fch.BATCH and f0["local_rows"] == fch.BATCH // 2 and f0["scale"] == 0.5
    assert torch.equal(f0["dy"].view(torch.int16), f1["dy"].view(torch.int16)) and torch.equal(f0["x"].view(torch.int16), f1["x"].view(torch.int16))
    # factored vs dense: the averaged gradient and FC1's weights within the bound of section 5
    G64, Gabs = fr.grad_ref(f0["dy"], f0["x"], 256, 1024, 0.5)
    bnd = fr.grad_bound(Gabs, fch.BATCH, 0.5) + lr.gamma(fch.BATCH) * 0.5 * Gabs
    fails = []
    lr.check_values(G64, fr.grad_bound(Gabs, fch.BATCH, 0.5), f0["g"], "gathered gradient", fails, "two ranks")
    lr.check_values(G64, lr.gamma(fch.BATCH) * 0.5 * Gabs, d0["g"], "dense averaged gradient", fails, "two ranks")
    assert not fails, fails
    n = "3.weight"
    db = (f0["buf"][n].double() - d0["buf"][n].double()).abs()
    dp = (f0["params"][n].double() - d0["params"][n].double()).abs()
    assert bool((db <= bnd).all()) and bool((dp <= 0.5 * bnd + 2 * er.RND * f0["params"][n].double().abs()).all())
    for k in d0["params"]:
        if k != n:
            assert torch.equal(d0["params"][k], f0["params"][k]), k
