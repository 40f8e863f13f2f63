"""The LARS entries of csrc/lars.hip through the C ABI, against tests/lars_ref.py, and yolo.optim.LARS on the device.

Norms (yolo_lars_norm_slots, yolo_lars_norms_multi): every stored double BIT-EQUAL to the numpy restatement of the kernels' summation order and within
2^-22 relative of math.fsum of the exact squares (one fp32 rounding per square and one per pair sum, all terms positive; the fp64 accumulation adds
below 2^-40 at these sizes); g_total bit-equal to the rising-order sum; guard bands around norms, scratch and inputs; two calls the same bits.
Step (yolo_lars_step, yolo_lars_step_multi, yolo_lars_step_multi_bg): the norms are handed in by the test; every element within lars_ref's bound,
the shadow equal to bf16(p), buf untouched without momentum, the three forms (background on 1, 2 and 256 workgroups) the same bits, skip_flag.
Then: exact scale invariance, the optimizer against its CPU step, no yolo_sumsq* entry during a step, YOLOv1 at batch 2 with and without the
background pass, and two deterministic runs in a child process."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import elementwise_ref as er
import lars_ref as lf
import launch_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "lars_child.py")
BF = torch.bfloat16
LR, MAX_NORM, ETA, EPS = 1e-2, 10.0, 1e-3, 1e-8
Guarded = er.Guarded
NORM_SIZES = [0, 1, 3, 4, 65535, 65536, 65537, 2 * 65536 + 5]
STEP_SIZES = [0, 1, 3, 8191, 8192, 8193, 3 * 8192 + 17]
ENTRIES = [("single", 0), ("multi", 0), ("bg", 1), ("bg", 2), ("bg", 256)]
F64_PAT = 0x7FF80D1E0D1E0D1E          # a NaN payload no result equals
F64_GUARD = 64


def _lib():
    from yolo._hip import lib
    return lib()


def _stream():
    from yolo._hip import stream
    return stream()


def _last_error():
    return _lib().yolo_hip_last_error().decode(errors="replace")


class GuardedF64:
    """n doubles of a NaN pattern between two guard bands of it: .t the view a kernel writes, .ptr its address, guards_ok()"""

    def __init__(self, n):
        self.n = n
        self.raw = torch.full((n + 2 * F64_GUARD,), F64_PAT, dtype=torch.int64, device="cuda")
        self.t = self.raw.view(torch.float64)[F64_GUARD: F64_GUARD + n]

    @property
    def ptr(self):
        return self.raw.data_ptr() + 8 * F64_GUARD

    def guards_ok(self):
        return bool((self.raw[:F64_GUARD] == F64_PAT).all()) and bool((self.raw[F64_GUARD + self.n:] == F64_PAT).all())


def _values(n, gen):
    """fp32 with 1e-3 <= |x| <= 1e3 (no fp32 square underflows) and random sign"""
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64, device="cuda")
    mag = torch.exp(r() * (np.log(1e3) - np.log(1e-3)) + np.log(1e-3)).clamp(1e-3, 1e3)
    return (mag * torch.where(r() < 0.5, -1.0, 1.0)).float()


def _bits(x: float) -> int:
    return int(np.float64(x).view(np.int64))


# ---- norms ---------------------------------------------------------------------------------------------------------------------------------------------

def _norms_run(ps, gs, with_total=True):
    """one yolo_lars_norms_multi call on Guarded inputs -> (norms as a list of python floats, g_total); asserts the guard bands and that the scratch
    beyond what yolo_lars_norm_slots asked for is untouched"""
    L, st = _lib(), _stream()
    count = len(ps)
    ns = (ctypes.c_long * count)(*[P.n for P in ps])
    slots = ctypes.c_long(-1)
    assert L.yolo_lars_norm_slots(ns, count, ctypes.byref(slots)) == 0, _last_error()
    assert slots.value == 2 * sum((P.n + 65535) // 65536 for P in ps)
    scratch, norms, total = GuardedF64(slots.value), GuardedF64(2 * count), GuardedF64(1)
    pp = (ctypes.c_void_p * count)(*[P.ptr for P in ps])
    gp = (ctypes.c_void_p * count)(*[G.ptr for G in gs])
    rc = L.yolo_lars_norms_multi(pp, gp, ns, count, scratch.ptr, slots.value, norms.ptr, total.ptr if with_total else None, st)
    assert rc == 0, _last_error()
    torch.cuda.synchronize()
    assert scratch.guards_ok() and norms.guards_ok() and total.guards_ok(), "a guard band of scratch / norms / g_total was written"
    assert all(X.guards_ok() for X in ps + gs), "a guard band of an input was written"
    if not with_total:
        assert int(total.raw[F64_GUARD]) == F64_PAT, "g_total == NULL and something was stored"
    return norms.t.cpu().tolist(), (float(total.t.cpu()[0]) if with_total else None)


def _check_norms(sizes, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    p0 = [_values(n, gen) for n in sizes]
    g0 = [_values(n, gen) for n in sizes]
    ps, gs = [Guarded(x) for x in p0], [Guarded(x) for x in g0]
    got, total = _norms_run(ps, gs)
    again, total2 = _norms_run(ps, gs)
    assert [_bits(v) for v in got] == [_bits(v) for v in again] and _bits(total) == _bits(total2), "two calls differ in some bits"
    for P, x in zip(ps + gs, p0 + g0):
        assert torch.equal(P.t, x), "an input was written"
    fails = []
    for i, n in enumerate(sizes):
        for k, x in ((0, p0[i]), (1, g0[i])):
            v = got[2 * i + k]
            xs = x.cpu().numpy()
            want, exact = lf.norm_order_ref(xs), lf.exact_sumsq(xs)
            if _bits(v) != _bits(want):
                fails.append(f"tensor {i} (n={n}) norms[{2 * i + k}] = {v!r}, the order restatement gives {want!r}")
            if abs(v - exact) > 2.0 ** -22 * exact:
                fails.append(f"tensor {i} (n={n}) norms[{2 * i + k}] = {v!r}, exact {exact!r}: off by {abs(v - exact) / exact:.3g} relative")
    if _bits(total) != _bits(lf.g_total_ref(got)):
        fails.append(f"g_total = {total!r}, the rising-order sum gives {lf.g_total_ref(got)!r}")
    assert not fails, "\n".join(fails[:10])
    return got


def test_norms_all_sizes_in_one_table():
    got = _check_norms(NORM_SIZES, 1)
    assert got[0] == 0.0 and got[1] == 0.0, "an empty tensor gives 0, 0"


@pytest.mark.parametrize("n", NORM_SIZES)
def test_norms_single_tensors(n):
    _check_norms([n], 10 + n % 97)


def test_norms_hundred_tensors_three_launches():
    pool = [5, 65537, 1, 1027, 0, 4, 65536, 2 * 65536 + 5, 3, 8193]
    _check_norms([pool[(7 * i) % len(pool)] for i in range(100)], 3)


def test_norms_without_g_total_and_all_empty():
    gen = torch.Generator(device="cuda").manual_seed(4)
    ps, gs = [Guarded(_values(n, gen)) for n in (5, 0)], [Guarded(_values(n, gen)) for n in (5, 0)]
    got, total = _norms_run(ps, gs, with_total=False)
    assert total is None and got[2] == 0.0 and got[3] == 0.0 and got[0] > 0.0
    empty = [Guarded(torch.zeros(0, device="cuda")) for _ in range(3)]
    got, total = _norms_run(empty, empty)
    assert got == [0.0] * 6 and total == 0.0, "empty tensors are legal and give 0, 0 (stored, not left)"


def test_norms_reject_bad_arguments_and_launch_nothing():
    from yolo._hip import E_ARG, E_UNSUPPORTED
    L, st = _lib(), _stream()
    x = torch.ones(64, device="cuda")
    nrm, sc = GuardedF64(4), GuardedF64(4)
    V = lambda *v: (ctypes.c_void_p * len(v))(*v)
    N = lambda *v: (ctypes.c_long * len(v))(*v)
    a = x.data_ptr()
    call = lambda p=V(a, a), g=V(a, a), n=N(8, 8), count=2, scratch=sc.ptr, slots=4, out=nrm.ptr: \
        L.yolo_lars_norms_multi(p, g, n, count, scratch, slots, out, None, st)
    assert call(p=V(a, None)) == E_ARG and "tensor 1" in _last_error() and call(n=N(8, -1)) == E_ARG
    assert call(g=V(a + 4, a)) == E_UNSUPPORTED and "tensor 0" in _last_error()
    assert call(slots=3) == E_ARG and "scratch" in _last_error() and call(out=None) == E_ARG and call(count=-1) == E_ARG
    torch.cuda.synchronize()
    assert bool((nrm.raw == F64_PAT).all()) and bool((sc.raw == F64_PAT).all()), "a rejected call must not launch"


# ---- the step ------------------------------------------------------------------------------------------------------------------------------------------

def _inputs(sizes, seed, zero=None):
    """per tensor p, g, buf fp32 on the device: 1e-3 <= |g| <= 1e3, buf a previous state at the scale of a trust-scaled gradient; zero = 'p' / 'g':
    that array is all zeros"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for n in sizes:
        g = _values(n, gen)
        buf = g * (torch.rand(n, generator=gen, device="cuda") * 2 - 1) * 1e-3
        p = torch.randn(n, generator=gen, dtype=torch.float32, device="cuda")
        if zero == "p":
            p = torch.zeros_like(p)
        if zero == "g":
            g = torch.zeros_like(g)
        out.append((p, g, buf))
    return out


def _sums(ins):
    """(sum p^2, sum g^2) per tensor in fp64 (torch), and the device table the entries read"""
    pairs = [(float(p.double().pow(2).sum()), float(g.double().pow(2).sum())) for p, g, _ in ins]
    return pairs, torch.tensor([v for pr in pairs for v in pr] or [0.0], dtype=torch.float64, device="cuda")


def _run(entry, wg, bufs, h, first, norm, skip, table):
    """one pass over bufs = [(P, G, B, PB or None)] (Guarded) through one entry; the return code must be 0"""
    from yolo._hip import LarsTensor
    L, st = _lib(), _stream()
    nptr = ctypes.c_void_p(norm.data_ptr()) if norm is not None else None
    sptr = ctypes.c_void_p(skip.data_ptr()) if skip is not None else None
    adapt = int(h["adapt"])
    hy = (LR, h["momentum"], h["wd"], h.get("eta", ETA), h.get("eps", EPS), int(first), nptr, MAX_NORM)
    nr = lambda i: (table.data_ptr() + 16 * i) if adapt else None
    if entry == "single":
        for i, (P, G, B, PB) in enumerate(bufs):
            rc = L.yolo_lars_step(P.ptr, G.ptr, B.ptr, P.n, nr(i), adapt, *hy, PB.ptr if PB else None, sptr, st)
            assert rc == 0, _last_error()
        return
    tab = (LarsTensor * len(bufs))(*[LarsTensor(P.ptr, G.ptr, B.ptr, PB.ptr if PB else None, nr(i), P.n, adapt) for i, (P, G, B, PB) in enumerate(bufs)])
    if entry == "multi":
        rc = L.yolo_lars_step_multi(tab, len(bufs), *hy, sptr, st)
    else:
        rc = L.yolo_lars_step_multi_bg(tab, len(bufs), *hy, sptr, wg, st)
    assert rc == 0, _last_error()


def _judge(tag, bufs, starts, pairs, h, first, norm_sq, fails):
    worst = 0.0
    for i, ((P, G, B, PB), (p0, g0, b0)) in enumerate(zip(bufs, starts)):
        where = f"{tag}: tensor {i} (n={P.n})"
        for X, name in ((P, "p"), (G, "g"), (B, "buf"), (PB, "shadow")):
            if X is not None and not X.guards_ok():
                fails.append(f"{where}: guard band of {name} overwritten")
        if not torch.equal(G.t, g0):
            fails.append(f"{where}: the gradient was written")
        if not P.n:
            continue
        (rp, rb), (bp, bb) = lf.lars_ref(p0, g0, b0, lr=LR, momentum=h["momentum"], wd=h["wd"], eta=h.get("eta", ETA), eps=h.get("eps", EPS),
                                         first_step=first, norm_sq=norm_sq, max_norm=MAX_NORM, norms=pairs[i], adapt=h["adapt"])
        worst = max(worst, lr.check_values(rp, bp, P.t, "p", fails, where))
        if rb is not None:
            worst = max(worst, lr.check_values(rb, bb, B.t, "momentum_buffer", fails, where))
        elif not torch.equal(B.t.view(torch.int32), b0.view(torch.int32)):
            fails.append(f"{where}: momentum == 0 but buf was written")
        if PB is not None and not torch.equal(PB.t.view(torch.int16), lf.bf16_bits(P.t)):
            fails.append(f"{where}: bf16 shadow != bf16(p)")
    return worst


def _check_case(sizes, shadow, h, first, norm_sq, seed, entries=ENTRIES, zero=None, what=""):
    """all entries on the same inputs: each within the reference's bound on its own, and all of them the same bits -> the first entry's (p, buf) bits"""
    ins = _inputs(sizes, seed, zero)
    pairs, table = _sums(ins)
    norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda") if norm_sq is not None else None
    fails, results = [], {}
    for entry, wg in entries:
        tag = f"{what} {entry}" + (f"[{wg}]" if entry == "bg" else "")
        bufs = [(Guarded(p), Guarded(g), Guarded(b), Guarded(torch.zeros(p.numel(), dtype=BF, device="cuda"), BF) if sh else None)
                for (p, g, b), sh in zip(ins, shadow)]
        _run(entry, wg, bufs, h, first, norm, None, table)
        torch.cuda.synchronize()
        worst = _judge(tag, bufs, ins, pairs, h, first, norm_sq, fails)
        results[(entry, wg)] = [torch.cat([b[0].t, b[2].t]).view(torch.int32) for b in bufs]
        print(f"{tag}: worst |err| / bound {worst:.3f}")
    keys = list(results)
    for k in keys[1:]:
        if not all(torch.equal(a, b) for a, b in zip(results[keys[0]], results[k])):
            fails.append(f"{what}: {k} and {keys[0]} differ in some bits")
    assert not fails, "\n".join(fails[:12])
    return results[keys[0]]


_GRID = [(h, first, clip) for h in lf.HYPERS for first in (0, 1) for clip in (None, (10.0 / 0.37) ** 2)]


@pytest.mark.parametrize("idx", range(len(_GRID)), ids=[f"{lf.hyper_id(h)}-first{f}-{'clip' if c else 'noclip'}" for h, f, c in _GRID])
def test_step_every_combination(idx):
    """first_step 0 / 1, momentum 0 / 0.9, wd 0 / 5e-4, with norm_sq (a clip of 0.37) and without, adapt 0 / 1, every size in one table, the shadow on
    every second tensor"""
    h, first, norm_sq = _GRID[idx]
    _check_case(STEP_SIZES, [i % 2 == 1 for i in range(len(STEP_SIZES))], h, first, norm_sq, 200 + idx, what=f"{lf.hyper_id(h)} first={first}")


def test_step_norm_present_but_not_clipping():
    """norm_sq = 1: the coefficient is 1, the gradient norm enters the trust ratio unscaled"""
    _check_case(STEP_SIZES, [True] * len(STEP_SIZES), dict(momentum=0.9, wd=5e-4, adapt=True), 0, 1.0, 300, what="norm 1.0")


@pytest.mark.parametrize("n", STEP_SIZES[1:])
def test_step_single_tensors(n):
    _check_case([n], [True], dict(momentum=0.9, wd=5e-4, adapt=True), 0, (10.0 / 0.37) ** 2, 400 + n % 89, what=f"n={n}")


@pytest.mark.parametrize("zero", ["p", "g"])
def test_zero_norm_gives_trust_one(zero):
    """sum p^2 = 0 or sum g^2 = 0: the trust ratio is 1 -- the bits of the same step with adapt off"""
    h = dict(momentum=0.9, wd=5e-4, adapt=True, eta=0.5)
    sizes, shadow = [8193, 5], [True, False]
    a = _check_case(sizes, shadow, h, 0, None, 500, zero=zero, what=f"zero {zero}")
    b = _check_case(sizes, shadow, dict(h, adapt=False), 0, None, 500, zero=zero, entries=ENTRIES[1:2], what=f"zero {zero} plain")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("norm_sq", [None, (10.0 / 0.37) ** 2], ids=["noclip", "clip0.37"])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_trust_ratio_against_the_restatement(wd, norm_sq):
    """the trust ratio read off the device: p = 0, g = 1, lr = 1, no momentum, the norms handed in -> p' = fma(-1, (1 * clip + wd * 0) * trust, 0), and
    with clip = 1 exactly -trust.  96 pairs of sums between 1e-6 and 1e6: within TRUST_ULPS fp32 ulps of trust_ref (with the clip: one more rounding,
    of clip * trust, half an ulp); prints how many are bit-equal"""
    from yolo._hip import LarsTensor
    L, st = _lib(), _stream()
    rng = np.random.default_rng(5)
    sums = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), (96, 2)))
    table = torch.tensor(sums.reshape(-1), dtype=torch.float64, device="cuda")
    p = torch.zeros(96 * 4, device="cuda")
    g = torch.ones(96 * 4, device="cuda")
    tab = (LarsTensor * 96)(*[LarsTensor(p.data_ptr() + 16 * i, g.data_ptr() + 16 * i, None, None, table.data_ptr() + 16 * i, 1, 1) for i in range(96)])
    norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda") if norm_sq is not None else None
    rc = L.yolo_lars_step_multi(tab, 96, 1.0, 0.0, wd, ETA, EPS, 0, ctypes.c_void_p(norm.data_ptr()) if norm is not None else None, MAX_NORM, None, st)
    assert rc == 0, _last_error()
    torch.cuda.synchronize()
    got = (-p.view(96, 4)[:, 0]).cpu().numpy()
    assert not bool(p.view(96, 4)[:, 1:].any()), "elements behind a one-element tensor were written"
    clip = er.clip_ref(norm_sq, MAX_NORM)
    ref = np.array([lf.trust_ref(a, b, clip=clip, eta=ETA, wd=wd, eps=EPS) for a, b in sums], dtype=np.float32)
    want = (np.float32(clip) * ref).astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = lf.TRUST_ULPS * np.spacing(ref).astype(np.float64) * clip + (0.5 * np.spacing(want).astype(np.float64) if clip != 1.0 else 0.0)
    print(f"trust ratio wd={wd} clip={clip!r}: {int((got == want).sum())} of 96 bit-equal to the restatement, worst |err| / bound {(err / bound).max():.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("entry,wg", ENTRIES)
@pytest.mark.parametrize("first", [0, 1])
def test_skip_flag(entry, wg, first):
    """*skip_flag != 0: p, buf and the shadow keep their bytes; == 0: updated"""
    sizes = [8193, 5, 0, 3 * 8192 + 17]
    ins = _inputs(sizes, 600)
    pairs, table = _sums(ins)
    norm = torch.tensor([(10.0 / 0.37) ** 2], dtype=torch.float64, device="cuda")
    h = dict(momentum=0.9, wd=5e-4, adapt=True)
    for flag in (1.0, -0.5, float("nan"), 0.0):
        bufs = [(Guarded(p), Guarded(g), Guarded(b), Guarded(torch.full((p.numel(),), 3.0, dtype=BF, device="cuda"), BF)) for p, g, b in ins]
        raw = [[X.raw.clone() for X in (P, B, PB)] for P, _, B, PB in bufs]
        _run(entry, wg, bufs, h, first, norm, torch.tensor([flag], device="cuda"), table)
        torch.cuda.synchronize()
        for (P, G, B, PB), r0, (p, _, b) in zip(bufs, raw, ins):
            kept = all(torch.equal(X.raw, r) for X, r in zip((P, B, PB), r0))                  # the whole allocations, guard bands included
            if not P.n:
                assert kept
                continue
            moved = not torch.equal(P.t, p) and not torch.equal(B.t, b) and torch.equal(PB.t.view(torch.int16), lf.bf16_bits(P.t))
            assert (kept if flag != 0.0 else moved), f"skip_flag {flag}: tensor of {P.n}"
            assert all(X.guards_ok() for X in (P, B, PB))


def test_step_entries_reject_bad_arguments():
    from yolo._hip import E_ARG, E_UNSUPPORTED, LarsTensor
    L, st = _lib(), _stream()
    x = [torch.ones(64, device="cuda") for _ in range(3)]
    nrm = torch.ones(2, dtype=torch.float64, device="cuda")
    p, g, b = (t.data_ptr() for t in x)
    hy = lambda **kw: (kw.get("lr", LR), kw.get("momentum", 0.9), kw.get("wd", 5e-4), kw.get("eta", ETA), kw.get("eps", EPS), 0, None, MAX_NORM)
    one = lambda **kw: L.yolo_lars_step(kw.get("p", p), kw.get("g", g), kw.get("b", b), kw.get("n", 16), kw.get("nr", nrm.data_ptr()), kw.get("adapt", 1),
                                        *hy(**kw), None, None, st)
    assert one(eta=-1.0) == E_ARG and "yolo_lars_step" in _last_error() and one(eps=-1.0) == E_ARG and one(lr=-1.0) == E_ARG
    assert one(nr=None) == E_ARG and one(b=None) == E_ARG and one(n=-1) == E_ARG and one(p=p + 4) == E_UNSUPPORTED
    T = lambda **kw: LarsTensor(kw.get("p", p), kw.get("g", g), kw.get("b", b), None, kw.get("nr", nrm.data_ptr()), kw.get("n", 16), kw.get("adapt", 1))
    for fn, extra in ((L.yolo_lars_step_multi, ()), (L.yolo_lars_step_multi_bg, (4,))):
        call = lambda tab, count, **kw: fn(tab, count, *hy(**kw), None, *extra, st)
        assert call((LarsTensor * 2)(T(), T(nr=None)), 2) == E_ARG and "tensor 1" in _last_error()
        assert call((LarsTensor * 2)(T(g=g + 4), T()), 2) == E_UNSUPPORTED and "tensor 0" in _last_error()
        assert call((LarsTensor * 2)(T(), T()), 2, eta=-1.0) == E_ARG
    many = (LarsTensor * 49)(*([T()] * 48 + [T(g=g + 4)]))
    assert L.yolo_lars_step_multi(many, 49, *hy(), None, st) == E_UNSUPPORTED and "tensor 48" in _last_error()
    assert L.yolo_lars_step_multi_bg((LarsTensor * 49)(*[T()] * 49), 49, *hy(), None, 4, st) == E_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in x), "a rejected call must not launch"


# ---- scale invariance, exact ---------------------------------------------------------------------------------------------------------------------------

def test_scaling_the_gradient_by_1024_changes_no_bit():
    """eps = 0, wd = 0, no clip: the step from g and the step from 1024 g, the norms recomputed on the device for each, give bit-equal p and buf --
    powers of two commute with every rounding in the chain (squares, sums, sqrt, the division, the narrowing, g * trust)"""
    from yolo._hip import LarsTensor
    L, st = _lib(), _stream()
    sizes = [8193, 5, 65537, 3 * 8192 + 17]
    ins = _inputs(sizes, 700)
    out = []
    for scale in (1.0, 1024.0):
        ps, gs = [Guarded(p) for p, _, _ in ins], [Guarded(g * scale) for _, g, _ in ins]
        bs = [Guarded(b) for _, _, b in ins]
        ns = (ctypes.c_long * len(sizes))(*sizes)
        slots = ctypes.c_long(0)
        assert L.yolo_lars_norm_slots(ns, len(sizes), ctypes.byref(slots)) == 0
        scratch, norms = GuardedF64(slots.value), GuardedF64(2 * len(sizes))
        pp = (ctypes.c_void_p * len(sizes))(*[P.ptr for P in ps])
        gp = (ctypes.c_void_p * len(sizes))(*[G.ptr for G in gs])
        assert L.yolo_lars_norms_multi(pp, gp, ns, len(sizes), scratch.ptr, slots.value, norms.ptr, None, st) == 0, _last_error()
        tab = (LarsTensor * len(sizes))(*[LarsTensor(P.ptr, G.ptr, B.ptr, None, norms.ptr + 16 * i, P.n, 1) for i, (P, G, B) in enumerate(zip(ps, gs, bs))])
        assert L.yolo_lars_step_multi(tab, len(sizes), LR, 0.9, 0.0, ETA, 0.0, 0, None, MAX_NORM, None, st) == 0, _last_error()
        torch.cuda.synchronize()
        assert all(X.guards_ok() for X in ps + gs + bs) and norms.guards_ok() and scratch.guards_ok()
        out.append(([P.t.clone() for P in ps], [B.t.clone() for B in bs], norms.t.clone()))
    assert torch.equal(out[1][2][1::2], out[0][2][1::2] * 1024.0 ** 2) and torch.equal(out[1][2][0::2], out[0][2][0::2])
    for i in range(len(sizes)):
        assert not torch.equal(out[0][0][i], ins[i][0]), "the step must move the parameter"
        assert torch.equal(out[0][0][i].view(torch.int32), out[1][0][i].view(torch.int32)), f"tensor {i}: p differs"
        assert torch.equal(out[0][1][i].view(torch.int32), out[1][1][i].view(torch.int32)), f"tensor {i}: buf differs"


# ---- the optimizer -------------------------------------------------------------------------------------------------------------------------------------

def test_lars_on_the_classifier_against_its_cpu_step(monkeypatch):
    """yolo.optim.LARS on the parameters of YOLOv1Classifier(4, batch_norm=True) with random gradients, three steps on the device, against _step_on_cpu
    on copies; no yolo_sumsq* entry is called.

    The bound.  Each side lies within lars_ref's bound (bp, bb) of the exact step from its own state (the device's norms are within 2^-22 of the
    exact sums, the CPU's within 2^-50: both trust ratios within TRUST_ULPS of trust_ref).  The states differ by (Dp, Db) after the last step, and the
    exact step maps a difference in p and buf to  Db' = momentum Db + trust wd Dp,  Dp' = Dp + lr Db'.  So per step
        Db <- momentum Db + trust wd Dp + 2 bb + c ;   Dp <- Dp + lr Db + 2 bp
    (2: one bound per side; the CPU side's bound, taken at a state Dp away, equals the device's to second order -- 1 % is added for it).
    c: the two sides clip by different doubles -- the device by its order-fixed g_total (which the reference is given: the optimizer's own
    _clip_norm_sq is wrapped to keep it), the CPU by torch's fp64 sum, 2^-22 apart at most, so their fp32 totals are neighbours at worst and the
    quotients max_norm / (total + 1e-6) at most 3 fp32 ulps apart; the coefficient enters once directly and once through the trust ratio's
    gn: c = 6 * 2^-23 * |trust * (clip * g + wd * p)|."""
    import copy
    import yolo.optim as yo
    from yolo import YOLOv1Classifier
    from yolo.optim import LARS, lars_param_groups
    calls = []
    real = yo.lib()

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(yo, "lib", lambda: Spy())
    torch.manual_seed(3)
    dev_m = YOLOv1Classifier(4, batch_norm=True).cuda()
    cpu_m = copy.deepcopy(dev_m).cpu()
    kw = dict(lr=LR, momentum=0.9, eta=ETA, eps=EPS, max_grad_norm=MAX_NORM)
    od, oc = LARS(lars_param_groups(dev_m, 5e-4), **kw), LARS(lars_param_groups(cpu_m, 5e-4), **kw)
    totals, inner = [], od._clip_norm_sq
    od._clip_norm_sq = lambda ps: totals.append(inner(ps)) or totals[-1]
    dps, cps = list(dev_m.parameters()), list(cpu_m.parameters())
    adapt = {id(p): g.get("adapt", True) for g in od.param_groups for p in g["params"]}
    wd = {id(p): g["weight_decay"] for g in od.param_groups for p in g["params"]}
    Dp = [torch.zeros(p.shape, dtype=torch.float64, device="cuda") for p in dps]
    Db = [torch.zeros(p.shape, dtype=torch.float64, device="cuda") for p in dps]
    gen = torch.Generator(device="cuda").manual_seed(9)
    fails = []
    for step in range(3):
        for p, q in zip(dps, cps):
            p.grad = torch.randn(p.shape, generator=gen, device="cuda") * 0.3          # |g| = 0.3 sqrt(60 M): the clip is active
            q.grad = p.grad.cpu()
        before = [(p.detach().clone(), od.state[p]["momentum_buffer"].clone() if step else None) for p in dps]
        od.step()
        oc.step()
        torch.cuda.synchronize()
        norm_sq, exact = float(totals[-1]), float(sum(p.grad.double().pow(2).sum() for p in dps))
        assert abs(norm_sq - exact) <= 2.0 ** -22 * exact and er.clip_ref(norm_sq, MAX_NORM) < 1.0
        for i, (p, (p0, b0)) in enumerate(zip(dps, before)):
            sums = (float(p0.double().pow(2).sum()), float(p.grad.double().pow(2).sum()))
            (rp, rb), (bp, bb) = lf.lars_ref(p0, p.grad, b0, lr=LR, momentum=0.9, wd=wd[id(p)], eta=ETA, eps=EPS, first_step=step == 0, norm_sq=norm_sq,
                                             max_norm=MAX_NORM, norms=sums, adapt=adapt[id(p)])
            lr.check_values(rp, bp, p.detach(), "p", fails, f"step {step} tensor {i}")
            lr.check_values(rb, bb, od.state[p]["momentum_buffer"], "momentum_buffer", fails, f"step {step} tensor {i}")
            trust = lf.trust_ref(*sums, clip=er.clip_ref(norm_sq, MAX_NORM), eta=ETA, wd=wd[id(p)], eps=EPS, adapt=adapt[id(p)])
            c = 6 * 2.0 ** -23 * trust * (er.clip_ref(norm_sq, MAX_NORM) * p.grad.double() + wd[id(p)] * p0.double()).abs()
            Db[i] = 0.9 * Db[i] + trust * wd[id(p)] * Dp[i] + 2.02 * bb + c
            Dp[i] = Dp[i] + LR * Db[i] + 2.02 * bp
    assert not fails, "\n".join(fails[:10])
    for i, (p, q) in enumerate(zip(dps, cps)):
        dp = (p.detach().double() - q.detach().double().cuda()).abs()
        db = (od.state[p]["momentum_buffer"].double() - oc.state[q]["momentum_buffer"].double().cuda()).abs()
        assert bool((dp <= Dp[i]).all()) and bool((db <= Db[i]).all()), f"tensor {i}: device and CPU step differ by more than the summed bound"
    assert "yolo_lars_norms_multi" in calls and "yolo_lars_step_multi" in calls
    assert not [c for c in calls if c.startswith("yolo_sumsq")], calls


def test_lars_on_yolov1_with_and_without_the_background_pass():
    """yolo.optim.LARS on YOLOv1 at batch 2, two training steps with attach_plan(plan, overlap=True) and two with the overlap off, from the same weights
    and inputs: parameters and momentum buffers BIT-EQUAL (the second optimizer is handed the first model's gradient tensors, as
    tests/test_gpu_sgd.py does: the conv weight gradients are summed with atomics and differ from run to run; the norms are order-fixed and the plans'
    hints are not used, so nothing else can differ)"""
    import copy
    import synth
    from yolo import YOLOLoss, YOLOv1
    from yolo.optim import LARS, lars_param_groups
    torch.manual_seed(6)
    mA = YOLOv1().cuda().train()
    mB = copy.deepcopy(mA)
    start = [p.detach().clone() for p in mA.parameters()]
    kw = dict(lr=LR, momentum=0.9, eta=ETA, max_grad_norm=10.0)
    oA, oB = LARS(lars_param_groups(mA, 5e-4), **kw), LARS(lars_param_groups(mB, 5e-4), **kw)
    planA, planB = mA.hip_plan(), mB.hip_plan()
    oA.attach_plan(planA, overlap=True)
    oB.attach_plan(planB, overlap=False)
    assert oA.deferred and not oB.deferred and len(oA.bf16_shadow) == len(oB.bf16_shadow) >= 2
    x = torch.from_numpy(synth.synth_images(2, 3)).cuda()
    tgt = torch.from_numpy(synth.synth_targets(2, 4)).cuda()
    crit = YOLOLoss()
    for step in range(2):
        oA.zero_grad(set_to_none=True)
        loss, parts = crit(mA(x), tgt)
        loss.backward()
        for p, q in zip(mA.parameters(), mB.parameters()):
            q.grad = p.grad
        oA.skip_if = oB.skip_if = parts.device_flag
        oB.step()
        oA.step()
        assert oA._pending is not None and oB._pending is None
        assert not planA.grad_norm_sq and not planB.grad_norm_sq, "the plans' hints are cleared"
        assert float(parts["total"]) > 0
    oA.synchronize()
    torch.cuda.synchronize()
    for o, plan in ((oA, planA), (oB, planB)):
        for li in [li for li, L in enumerate(plan.layers) if L.kind == "fc"]:
            L = plan.layers[li]
            shadow = o.bf16_shadow[id(L.weight)][0]
            assert torch.equal(shadow.view(-1).view(torch.int16), lf.bf16_bits(L.weight.detach().view(-1))), "bf16 operand != bf16(master)"
    n = 0
    for p, q, p0 in zip(mA.parameters(), mB.parameters(), start):
        # (a bias is neither adapted nor decayed: behind the default initialisation its gradient can lie below half an ulp of lr^-1 |p| and leave it)
        assert p.ndim <= 1 or not torch.equal(p.detach(), p0), "two steps must move every adapted parameter"
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), "background and foreground updates differ"
        bA, bB = oA.state[p]["momentum_buffer"], oB.state[q]["momentum_buffer"]
        assert torch.equal(bA.view(torch.int32), bB.view(torch.int32)) and bool(torch.isfinite(bA).all())
        n += 1
    assert n == 52


def test_two_deterministic_runs_are_bit_equal(tmp_path):
    """YOLO_AMD_DETERMINISTIC=1 (read at import: a child process): two models from one seed, two LARS steps each at batch 2 with the background pass,
    stay bit-equal in every parameter, gradient and momentum buffer; the norm entries are the same in both modes"""
    out = tmp_path / "h.txt"
    env = dict(os.environ, YOLO_AMD_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, CHILD, "det", str(out), "2", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    assert len(out.read_text().split()) == 2
