"""What tests/test_gpu_wgrad.py relies on, checked without a GPU: the exact operand set really is exact (the fp64 reference of every case is an fp32
number with room to spare), launch_ref.wgrad_bound holds a brute-force fp32 accumulation in random orders, the schedule mirror of tests/wgrad_cases.py
sizes every case as the library does (yolo_wgrad_slab_floats: host arithmetic only), the cases named after a split really split, and the host code
refuses exactly the forms of EXPECT_REFUSED (a refusal returns before anything is launched, so it can be asked for here)."""

import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

import launch_ref as lr
import wgrad_cases as wc

# (N, H, Cout, Cin, split) -> floats of slab scratch of variants 5 / 6 on the network's own 3x3 layers, as tests/test_deterministic_cpu.py records them
RECORDED_56 = {(8, 56, 512, 256, 0): 16515072, (8, 56, 512, 256, 3): 3538944, (8, 14, 1024, 1024, 0): 9437184, (8, 14, 1024, 1024, 3): 28311552,
               (8, 112, 192, 64, 0): 16711680, (8, 112, 192, 64, 3): 589824, (64, 14, 1024, 1024, 0): 33554432, (1, 28, 1024, 512, 0): 14155776,
               (64, 28, 1024, 512, 0): 33554432, (64, 7, 1024, 1024, 3): 28311552}


def _lib():
    from yolo import _hip
    if not _hip.available():
        pytest.fail("libyolo_hip.so is not built")
    L = ctypes.CDLL(_hip.LIB_PATH)
    L.yolo_wgrad_slab_floats.argtypes = [ctypes.POINTER(_hip.WgradDesc), ctypes.POINTER(ctypes.c_long)]
    return L


def _need(L, d):
    n = ctypes.c_long(-1)
    assert L.yolo_wgrad_slab_floats(ctypes.byref(d), ctypes.byref(n)) == 0
    return n.value


def _schedule(P, Cout, Cin, K, variant=0):
    tiles, slots = wc.wgrad_tiles(Cout, Cin, K * K, variant)
    return wc.wgrad_schedule(P, tiles, slots)


def _shapes():
    seen = {}
    for c in wc.MATRIX:
        seen.setdefault(c.shape.name, c)
    return list(seen.values())


def _bound(case, opset, ops=None, **kw):
    ops = ops or wc.operands(case.shape, opset)
    return lr.wgrad_bound(case.desc(), ops.x, ops.x_base, ops.dy, ops.dy_base, **kw), ops


@pytest.mark.parametrize("case", _shapes(), ids=lambda c: c.shape.name)
def test_exact_set_reference_is_representable(case):
    """the zero bound rests on this: the reference, without and with the previous contents, is an fp32 number and 4 |ref| < 2^24 (a multiple of 1/4
    below 2^22); the operands hold what the module docstring says, halo and guard bands zero"""
    ops = wc.operands(case.shape, "exact")
    s = case.shape
    for t, C, ld, base, lim in ((ops.x, s.Cin, s.x_stride, ops.x_base, 3.0), (ops.dy, s.Cout, s.dy_stride, ops.dy_base, 0.5)):
        body = t[base:] if s.nhw is None else t[base: base + s.nhw[0] * s.Hp * s.Wp * ld]
        cols = body.view(-1, ld).double()
        assert float(cols[:, :C].abs().max()) <= lim and bool(((cols[:, :C] * 4) % 1 == 0).all())
        if s.nhw is not None:
            assert not bool(t[:base].any()) and not bool(t[base + body.numel():].any()), "guard bands are zeros"
            halo = body.view(s.nhw[0], s.Hp, s.Wp, ld).clone()
            halo[:, 1:-1, 1:-1] = 0
            assert not bool(halo.any()), "the halo is zero in every column"
            lo, hi = lr.wgrad_extent(case.desc(), "x")
            assert -lo <= ops.x_base and hi <= ops.x.numel() - ops.x_base, "the guard band covers every tap offset"
        if s.poison:
            assert float(cols[:, C:].abs().max()) == wc.POISON
    for prev in (False, True):
        b, _ = _bound(case, "exact", ops, exact=True, dw0=ops.dw0 if prev else None, db0=ops.db0 if prev else None)
        for ref, bnd in ((b.dw, b.dw_bnd), (b.db, b.db_bnd)):
            assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) * 4 < 2.0 ** 24
            assert bool(((ref * 4) % 1 == 0).all()) and not bool(bnd.any())


def _brute_force(case, ops, rng, ranges, prev):
    """dw, db of the launch added up in fp32, pixel by pixel in a random order inside `ranges` random pixel ranges, the ranges' partial sums added in a
    random order onto the previous contents"""
    d = case.desc()
    dims, slots, slot0 = lr._wgrad_pixels(d)
    Co, K = d.Cout, d.KH * d.KW * d.Cin
    G = ops.dy.as_strided(dims + (Co,), tuple(st * d.dy_px_stride for st in slots) + (1,), ops.dy_base + slot0 * d.dy_px_stride)
    X = ops.x.as_strided(dims + (d.KH, d.KW, d.Cin), tuple(st * d.x_px_stride for st in slots) + (d.x_row_stride, d.x_px_stride, 1),
                         ops.x_base + slot0 * d.x_px_stride - d.pad * d.x_row_stride - d.pad * d.x_px_stride)
    G = G.float().reshape(-1, Co).numpy()
    X = X.float().reshape(-1, K).numpy()
    order = rng.permutation(G.shape[0])
    parts_w, parts_b = [], []
    for chunk in np.array_split(order, ranges):
        w, b = np.zeros((Co, K), np.float32), np.zeros(Co, np.float32)
        for p in chunk:
            w += np.outer(G[p], X[p])          # bf16 x bf16: the product is exact in fp32, the addition rounds
            b += G[p]
        parts_w.append(w)
        parts_b.append(b)
    dw = ops.dw0.numpy().reshape(Co, K).copy() if prev else np.zeros((Co, K), np.float32)
    db = ops.db0.numpy().copy() if prev else np.zeros(Co, np.float32)
    for i in rng.permutation(ranges):
        dw += parts_w[i]
        db += parts_b[i]
    return torch.from_numpy(dw.reshape(-1)), torch.from_numpy(db)


SMALL = [wc.Case("small", wc.Shape(6, 5, P=37), wc.Mode(0)), wc.Case("small", wc.Shape(5, 8, 3, nhw=(2, 3, 4), geo="interior"), wc.Mode(0)),
         wc.Case("small", wc.Shape(4, 3, 3, nhw=(1, 5, 6), geo="stride2", x_stride=8), wc.Mode(0)),
         wc.Case("small", wc.Shape(7, 6, 3, nhw=(1, 4, 3), geo="flat", dy_stride=16, poison=True), wc.Mode(0))]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.shape.name)
@pytest.mark.parametrize("opset", wc.OPSETS)
def test_bound_holds_a_brute_force_fp32_sum_in_random_orders(case, opset):
    ops = wc.operands(case.shape, opset)
    rng = np.random.default_rng(5)
    for ranges, prev in ((1, False), (3, False), (4, True), (1, True)):
        b, _ = _bound(case, opset, ops, exact=opset == "exact", ranges=ranges, dw0=ops.dw0 if prev else None, db0=ops.db0 if prev else None)
        assert b.n == case.shape.P + ranges - 1
        for _ in range(3):
            dw, db = _brute_force(case, ops, rng, ranges, prev)
            fails = []
            w = max(lr.check_values(b.dw, b.dw_bnd, dw, "dw", fails, opset), lr.check_values(b.db, b.db_bnd, db, "db", fails, opset))
            assert not fails, fails
            assert w == 0.0 if opset == "exact" else w < 1.0
    # gamma, not 1.01 n u: the two part ways once n u is no longer small
    assert lr.gamma(1) == lr.U / (1 - lr.U) and lr.gamma(1 << 10) < 1.01 * (1 << 10) * lr.U and lr.gamma(1 << 20) > 1.01 * (1 << 20) * lr.U


# ---- the schedule mirror against the library -----------------------------------------------------------------------------------------------------------

def _slab_floats_mirror(d):
    """yolo_wgrad_slab_floats restated over the mirror (variants 0 / 1 / 4: split segments only, plus [co][range] bias partials; 5 / 6: every part)"""
    ntaps = d.KH * d.KW
    tiles, slots = wc.wgrad_tiles(d.Cout, d.Cin, ntaps, d.variant, d.x_px_stride)
    pipe = d.variant in (5, 6)
    if d.split > 0:
        r = wc.ranges_of(d)[0]
        if pipe:
            return tiles * r * 65536
        return tiles * r * 16384 + -(-d.Cout // 128) * 128 * r if r > 1 else 0
    mt, ms, tt, ts = wc.wgrad_schedule(d.P, tiles, slots)
    if pipe:
        return (mt * ms + tt * ts) * 65536
    nparts = (mt * ms if ms > 1 else 0) + (tt * ts if ts > 1 else 0)
    return nparts * 16384 + -(-d.Cout // 128) * 128 * max(ms if mt else 1, ts if tt else 1) if nparts else 0


def _wdesc(case):
    from yolo._hip import WgradDesc
    return case.desc(WgradDesc)


def test_mirror_sizes_every_case_as_the_library_does():
    L = _lib()
    n = 0
    for c in wc.MATRIX:
        if c.family == "B" or (c.id in wc.EXPECT_REFUSED and not (c.mode.slabs or c.mode.sumsq)):
            continue
        d = _wdesc(c)
        assert _need(L, d) == _slab_floats_mirror(d), c.id
        n += 1
    assert n > 300
    for (N, H, Cout, Cin, split), want in RECORDED_56.items():       # ... and the recorded sizes of the network's own layers
        from yolo._hip import WgradDesc
        Hp = H + 2
        d = WgradDesc(N * H * H, Cout, Cin, Cout, Cin, 3, 3, 1, Hp * Cin, split, 0, 5, H, H, Hp * Hp, Hp, 1, Hp + 1)
        assert _slab_floats_mirror(d) == want, (N, H, Cout, Cin, split)
    assert _schedule(6400, 2176, 2048, 1) == (256, 2, 16, 25) and _schedule(6400, 4352, 2048, 1, variant=5) == (128, 2, 8, 25)
    assert wc.wgrad_tiles(136, 4, 9, 5) == (9, 256) and wc.wgrad_tiles(136, 8, 9, 6) == (1, 256) and wc.wgrad_tiles(136, 128, 9, 5) == (5, 256)


def test_cases_named_after_a_split_really_split():
    L = _lib()
    seen = Counter()
    for c in wc.MATRIX:
        d, m = c.desc(), c.mode
        if c.group == "both-segments":
            tiles, slots = wc.wgrad_tiles(d.Cout, d.Cin, 1, d.variant)
            mt, ms, tt, ts = wc.wgrad_schedule(d.P, tiles, slots)
            assert mt > 0 and ms > 1 and tt > 0 and ts > ms, (c.id, mt, ms, tt, ts)
            assert wc.ranges_of(d) == (ms, ts), "every range of both segments holds pixels"
            assert _need(L, _wdesc(c)) > 0
            assert c.opsets == ("exact",)
            seen["both"] += 1
        elif c.group == "schedule":
            tiles, slots = wc.wgrad_tiles(d.Cout, d.Cin, 1, d.variant)
            mt, ms, tt, ts = wc.wgrad_schedule(d.P, tiles, slots)
            assert mt == 0 and ts > 1 and 1 < wc.ranges_of(d)[1] < ts, (c.id, tt, ts, wc.ranges_of(d))
            seen["empty " + c.family] += 1
        elif m.split in (2, 3):
            assert 1 < wc.ranges_of(d)[0] <= m.split, (c.id, wc.ranges_of(d))
            if c.group == "modes" and c.shape.nhw is None:
                assert wc.ranges_of(d)[0] == m.split
            if c.family != "B" and not m.accumulate:
                assert _need(L, _wdesc(c)) > 0, c.id
            seen["uniform"] += 1
        assert c.opsets[0] == "exact" and (len(c.opsets) == 2) == (d.P <= 2048)
        if c.group not in ("both-segments",):
            assert d.P <= 2048 and c.shape.n_dw() <= 1 << 20, c.id
    assert seen["both"] == 15 and all(seen["empty " + f] == 3 * len(v) for f, v in wc.FAMILIES.items()) and seen["uniform"] > 100
    for fam in wc.FAMILIES:       # split = 0 with a split tile, and with atomics on it, in every family
        assert any(c.family == fam and c.mode.split == 0 and wc.dw_arrives(c) == "zero" for c in wc.MATRIX), fam


def test_the_host_code_refuses_exactly_the_documented_forms():
    from yolo._hip import WgradDesc, lib
    L = lib()
    L.yolo_wgrad.restype = ctypes.c_int
    host = torch.zeros(64)                         # 16-B aligned host memory: a refusal returns before any pointer is used
    q = _lib()
    rules = Counter()
    for c in wc.MATRIX:
        d = _wdesc(c)
        need = ctypes.c_long(-1)
        rc = q.yolo_wgrad_slab_floats(ctypes.byref(d), ctypes.byref(need))
        if c.id not in wc.EXPECT_REFUSED:
            assert rc == 0 and wc.documented_refusal(c) is None, c.id
            continue
        code, why = wc.EXPECT_REFUSED[c.id]
        rules[why] += 1
        if c.mode.slabs:
            d.slabs, d.slab_floats = host.data_ptr(), max(need.value, 1 << 40)
        if c.mode.sumsq:
            d.dw_sumsq = host.data_ptr()
        p = ctypes.c_void_p(host.data_ptr())
        got = L.yolo_wgrad(ctypes.byref(d), p, p, p, p if c.mode.db else None, None)
        assert got == code == wc.E_UNSUPPORTED, (c.id, got, L.yolo_hip_last_error().decode(errors="replace"))
    # outside the matrix: the bias-only launch (dw == NULL) walks slots 0 .. P - 1 and refuses a pixel geometry
    d = wc.Case("bias", wc.Shape(30, 8, 3, nhw=(2, 7, 7), geo="interior"), wc.Mode(0)).desc(WgradDesc)
    p = ctypes.c_void_p(host.data_ptr())
    assert L.yolo_wgrad(ctypes.byref(d), p, p, None, p, None) == wc.E_UNSUPPORTED and "bias-only" in L.yolo_hip_last_error().decode(errors="replace")
    assert not bool(host.any())
    # the table holds nothing but the header's rules, each of them reached
    assert set(rules) == {"geometry with variants 2 and 3", "variants 5 and 6, pad 0: P % 32 == 0",
                          "slabs: variant 0 / 1 / 4 / 5 / 6, accumulate = 0, Cin % 4 == 0", "dw_sumsq: split 1, accumulate 0, variant 0 / 1, Cin % 4 == 0"}, rules
    print(dict(rules), len(wc.MATRIX))
