"""Every form of yolo_wgrad, element by element against the fp64 reference of tests/launch_ref.py (wgrad_bound).

The matrix is tests/wgrad_cases.py: (shape, mode) pairs over the six kernel variants in four families (A = 0 / 1, A8 = 4, B = 2 / 3, C = 5 / 6),
flat and pixel-geometry indexing, uniform and two-segment pixel splits, atomics, slabs and accumulate, tap pairing and tap grouping, the fused bias
gradient and sum of squares, and the bias-only launch.  Every case runs with the exact operand set (bound 0: dw and db equal fp64 bit for bit, whatever
the order of the atomics) and, up to 2048 pixels, with the random set (|err| <= gamma(n) (S + |previous|), n = P + ranges - 1 + accumulate).

Per launch: dw, db and the slab scratch arrive as NaN where the launch stores, as the previous contents (multiples of 1/4) where it adds onto them, as
zeros where split tiles meet in atomics; NaN guard bands behind dw, db, the scratch and the sum-of-squares accumulator must survive; x and dy must be
bit-unchanged; a form without atomics (one range per tile without accumulate, every slab form) must give the same bits twice.  A case either runs
and is checked or stands in wgrad_cases.EXPECT_REFUSED with its return code -- then dw, db, the scratch and the accumulator must be untouched.

The fused sum of squares (yolo_wgrad_desc.dw_sumsq) is compared with the fp64 sum of squares of the dw the launch stored, plus the accumulator's
previous value.  A thread of wgrad_kernel squares and adds k = 64 values in fp32 before the fp64 part -- two row blocks of eight quads:
        for (int h = 0; h < 2; ++h) { ... for (int it = 0; it < 8; ++it) { ...
                    ssq += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        double s = (double)ssq;          (shuffles, LDS and one atomicAdd per workgroup in fp64 from here)
so |got - ref| <= gamma(k + 1) * sum of squares, k + 1 = 65 covering the roundings of the squares themselves.

Worst |err| / bound of the random set on an MI355X (the exact set is 0 everywhere: bit-equal), per family and mode; 1719 launches checked, 1141 of
them repeated for their bits, 192 refusals:
                 one range   atomics   accumulate   slabs
    A  (0 / 1)     0.288      0.012      0.012      0.013       with dw_sumsq: dw 0.349, the sum of squares itself 0.0007
    A8 (4)         0.288      0.012      0.012      0.013
    B  (2 / 3)     0.222      0.008      0.006      (refused)
    C  (5 / 6)     0.288      0.012      0.012      0.013
    bias-only                 0.006
(one range: a few pixels, so gamma(n) is a few u and one rounding is a good part of it; the split forms have P >= 129 and a bound of 512+ roundings.)
Variants 5 / 6 group 256 / Cin taps per tile for Cin in {8, 16, 32, 64, 128}: all five pass, flat and over the interior, with atomics and with slabs.
Cin = 4 (3x3) runs with one tap per tile since the host code asks for Cin % 8 == 0 before it groups taps (it divided by Cin / 8 = 0 chunks per tap).
"""

import ctypes
import math
from collections import defaultdict

import pytest
import torch

import launch_ref as lr
import wgrad_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096                 # floats of NaN behind dw, db and the slab scratch
SUMSQ0 = 3.25                # the accumulator's value before the launch
SUMSQ_K = 64                 # values a thread squares and adds in fp32 (quoted above)
REPORT = defaultdict(float)  # (family, mode kind) -> worst |err| / bound of the random set
COUNTS = defaultdict(int)

_CACHE = {}


def _problem(shape, opset):
    """operands of a shape on the device, pristine copies of x / dy, and the fp64 sums (signed and absolute), computed once per shape"""
    key = (shape.name, opset)
    if key not in _CACHE:
        ops = wc.operands(shape, opset, DEV)
        ops.x_keep, ops.dy_keep = ops.x.clone(), ops.dy.clone()
        d = wc.Case("ref", shape, wc.Mode(0)).desc()
        ops.refs = lr.wgrad_ref(d, ops.x, ops.x_base, ops.dy, ops.dy_base, device=DEV, absolute=True)
        _CACHE[key] = ops
    return _CACHE[key]


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _guarded(n, arrives, prev=None):
    t = torch.full((n + GUARD,), math.nan, device=DEV)
    if arrives == "zero":
        t[:n] = 0.0
    elif arrives != "nan":
        t[:n] = prev
    return t


def _last_error():
    from yolo._hip import lib
    return lib().yolo_hip_last_error().decode(errors="replace")


class Launch:
    """one yolo_wgrad call on fresh buffers"""

    def __init__(self, case, ops):
        from yolo._hip import WgradDesc, lib, stream
        s, m = case.shape, case.mode
        self.d = d = case.desc(WgradDesc)
        self.n_dw = s.n_dw()
        self.dw = _guarded(self.n_dw, wc.dw_arrives(case), ops.dw0)
        self.db = _guarded(s.Cout, wc.db_arrives(case), ops.db0) if m.db else None
        self.need = 0
        if m.slabs:
            need = ctypes.c_long(0)
            lib().yolo_wgrad_slab_floats(ctypes.byref(d), ctypes.byref(need))        # (0 where the form is refused or no tile is split)
            self.need = need.value
        self.slabs = _guarded(max(self.need, 1024) if m.slabs else 0, "nan")
        self.sq = torch.full((1 + 16,), math.nan, dtype=torch.float64, device=DEV)
        self.sq[0] = SUMSQ0
        if m.slabs:
            d.slabs, d.slab_floats = self.slabs.data_ptr(), self.slabs.numel() - GUARD
        if m.sumsq:
            d.dw_sumsq = self.sq.data_ptr()
        self.bufs = [t for t in (self.dw, self.db, self.slabs, self.sq) if t is not None]
        before = [t.clone() for t in self.bufs]
        torch.cuda.synchronize()
        self.rc = lib().yolo_wgrad(ctypes.byref(d), ctypes.c_void_p(ops.x.data_ptr() + 2 * ops.x_base), ctypes.c_void_p(ops.dy.data_ptr() + 2 * ops.dy_base),
                                   ctypes.c_void_p(self.dw.data_ptr()), ctypes.c_void_p(self.db.data_ptr()) if m.db else None, stream())
        torch.cuda.synchronize()
        self.untouched = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(self.bufs, before))

    def guards_ok(self, case):
        ok = bool(torch.isnan(self.dw[self.n_dw:]).all()) and bool(torch.isnan(self.sq[1:]).all())
        if self.db is not None:
            ok = ok and bool(torch.isnan(self.db[case.shape.Cout:]).all())
        used = self.need if case.mode.slabs else 0
        return ok and bool(torch.isnan(self.slabs[used:]).all())         # (a launch that needs no slabs leaves the whole scratch alone)


def _kind(case):
    m = case.mode
    return ("slabs" if m.slabs else "accumulate" if m.accumulate else "one range" if wc.max_ranges(case.desc()) == 1 else "atomics") + (" +sumsq" if m.sumsq else "")


def run_case(case, opset, fails):
    ops = _problem(case.shape, opset)
    tag = f"{case.id} [{opset}]"
    a = Launch(case, ops)
    if case.id in wc.EXPECT_REFUSED:
        code, why = wc.EXPECT_REFUSED[case.id]
        if a.rc != code:
            fails.append(f"{tag}: returned {a.rc}, expected the refusal {code} ({why})")
        if not a.untouched:
            fails.append(f"{tag}: a refused launch wrote")
        COUNTS["refused"] += 1
        return
    if a.rc != 0:
        fails.append(f"{tag}: refused with {a.rc} ({_last_error()}) but is not in EXPECT_REFUSED")
        return
    COUNTS["ran"] += 1
    s, m, d = case.shape, case.mode, case.desc()
    if not a.guards_ok(case):
        fails.append(f"{tag}: a guard band behind dw / db / the scratch / the accumulator was written")
    if not (torch.equal(ops.x.view(torch.int16), ops.x_keep.view(torch.int16)) and torch.equal(ops.dy.view(torch.int16), ops.dy_keep.view(torch.int16))):
        fails.append(f"{tag}: an operand changed")
    b = lr.wgrad_bound(d, ops.x, ops.x_base, ops.dy, ops.dy_base, dw0=ops.dw0 if wc.dw_arrives(case) == "dw0" else None,
                       db0=ops.db0 if (m.db and wc.db_arrives(case) == "db0") else None, ranges=wc.max_ranges(d), exact=opset == "exact", refs=ops.refs)
    worst = lr.check_values(b.dw, b.dw_bnd, a.dw[: a.n_dw], "dw", fails, tag)
    if m.db:
        worst = max(worst, lr.check_values(b.db, b.db_bnd, a.db[: s.Cout], "db", fails, tag))
    if m.sumsq:
        sq = float((a.dw[: a.n_dw].double() ** 2).sum())
        err, bnd = abs(float(a.sq[0]) - (SUMSQ0 + sq)), lr.gamma(SUMSQ_K + 1) * sq
        print(f"{tag}: dw_sumsq |err| / bound {err / bnd:.4f}")
        if not err <= bnd:
            fails.append(f"{tag}: dw_sumsq {float(a.sq[0])!r}, fp64 of the stored dw {SUMSQ0 + sq!r}, bound {bnd:.3g}")
        worst = max(worst, err / bnd)
    elif float(a.sq[0]) != SUMSQ0:
        fails.append(f"{tag}: the sum-of-squares accumulator changed without dw_sumsq")
    if opset == "random":
        key = (case.family, _kind(case))
        REPORT[key] = max(REPORT[key], worst)
    if wc.repeatable(case):
        a2 = Launch(case, ops)
        same = a2.rc == 0 and torch.equal(_bits(a.dw[: a.n_dw]), _bits(a2.dw[: a.n_dw])) and (not m.db or torch.equal(_bits(a.db[: s.Cout]), _bits(a2.db[: s.Cout])))
        if not same:
            fails.append(f"{tag}: a second launch gives other bits")
        COUNTS["repeated"] += 1


def _print_report(title):
    rows = "  ".join(f"{f}/{k} {v:.4f}" for (f, k), v in sorted(REPORT.items()))
    print(f"\n{title}: {dict(COUNTS)}\n  worst |err| / bound, random set, so far: {rows}", flush=True)


GROUPS = sorted({(c.group, c.family) for c in wc.MATRIX})


@pytest.mark.parametrize("group,family", GROUPS, ids=[f"{g}-{f}" for g, f in GROUPS])
def test_wgrad_matrix(group, family):
    cases = [c for c in wc.MATRIX if c.group == group and c.family == family]
    assert cases
    fails = []
    for c in cases:
        for opset in c.opsets:
            run_case(c, opset, fails)
        if len(fails) > 20:
            break
    for key in [k for k in _CACHE if _CACHE[k].x.numel() > (1 << 22)]:      # the two schedule shapes: free them with their test
        del _CACHE[key]
    _print_report(f"{group} {family}")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("P,Cout", wc.BIAS_ONLY)
def test_bias_only_launch(P, Cout):
    """dw == NULL: colsum_kernel adds the column sums of dy onto db (at most 2048 / 32 = 64 workgroups meet in atomics on a channel here)"""
    from yolo._hip import WgradDesc, lib, stream
    shape = wc.Shape(Cout, 8, P=P)
    case = wc.Case("bias", shape, wc.Mode(0))
    for opset in wc.OPSETS:
        ops = _problem(shape, opset)
        d = case.desc(WgradDesc)
        db = _guarded(Cout, "db0", ops.db0)
        rc = lib().yolo_wgrad(ctypes.byref(d), ctypes.c_void_p(ops.x.data_ptr()), ctypes.c_void_p(ops.dy.data_ptr()), None, ctypes.c_void_p(db.data_ptr()), stream())
        torch.cuda.synchronize()
        assert rc == 0, _last_error()
        assert bool(torch.isnan(db[Cout:]).all()), "guard band behind db was written"
        assert torch.equal(ops.dy.view(torch.int16), ops.dy_keep.view(torch.int16)) and torch.equal(ops.x.view(torch.int16), ops.x_keep.view(torch.int16))
        b = lr.wgrad_bound(case.desc(), ops.x, ops.x_base, ops.dy, ops.dy_base, db0=ops.db0, ranges=64, exact=opset == "exact", refs=ops.refs)
        fails = []
        w = lr.check_values(b.db, b.db_bnd, db[:Cout], "db", fails, f"bias-only P {P} Cout {Cout} [{opset}]")
        if opset == "random":
            REPORT[("bias-only", "atomics")] = max(REPORT[("bias-only", "atomics")], w)
        assert not fails, fails
    _print_report(f"bias-only P {P} Cout {Cout}")


def test_bias_only_launch_refuses_a_pixel_geometry():
    """colsum_kernel walks slots 0 .. P - 1, so dw == NULL with geo_W != 0 is refused (as the header says) and db stays as it was"""
    from yolo._hip import WgradDesc, lib, stream
    case = wc.Case("bias", wc.Shape(30, 8, 3, nhw=(2, 7, 7), geo="interior"), wc.Mode(0))
    ops = _problem(case.shape, "exact")
    d = case.desc(WgradDesc)
    db = _guarded(30, "db0", ops.db0)
    before = db.clone()
    rc = lib().yolo_wgrad(ctypes.byref(d), ctypes.c_void_p(ops.x.data_ptr() + 2 * ops.x_base), ctypes.c_void_p(ops.dy.data_ptr() + 2 * ops.dy_base), None,
                          ctypes.c_void_p(db.data_ptr()), stream())
    torch.cuda.synchronize()
    assert rc == wc.E_UNSUPPORTED and "bias-only" in _last_error()
    assert torch.equal(_bits(db), _bits(before))


def test_no_case_is_skipped():
    """the table of refusals holds forms of the matrix only, and together with the cases that run it is the matrix"""
    ids = {c.id for c in wc.MATRIX}
    assert set(wc.EXPECT_REFUSED) <= ids and all(code == wc.E_UNSUPPORTED for code, _ in wc.EXPECT_REFUSED.values())
    assert {(c.group, c.family) for c in wc.MATRIX} == set(GROUPS)
