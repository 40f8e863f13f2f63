"""Every ABI entry of csrc/optim.hip, called directly, against tests/elementwise_ref.py: each element of p, exp_avg and exp_avg_sq within the bound
propagated through adam1's fp32 operations (about 0.6-4 e-7 relative), the bf16 shadow equal to bf16 of the stored p, the clip coefficient and the
stand-alone clip bit for bit, the sum of squares within its derived bound.  Every buffer a kernel writes lies between guard bands of a NaN pattern
that must survive.  Gradients have 1e-6 <= |g| <= 1e3 (well above the 1e-15 below which g * g would leave the normal range: the bound models no
subnormal intermediate).  Rejected-argument cases are those the C entries test on the host before any launch.

The three Adam entries share adam1 but are three kernels compiled with FMA contraction allowed, so nothing makes them contract alike: each is held
to the bound on its own and their bitwise agreement is only reported (`-s` shows it; on the gfx950 build of this commit yolo_adam_step and
yolo_adam_step_multi agree bit for bit and the background kernel differs from them in the last bit of some elements)."""

import ctypes

import numpy as np
import pytest
import torch

import elementwise_ref as er
import launch_ref as lr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=5e-4)
MAX_NORM = 10.0
Guarded = er.Guarded
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1027, 8191, 8192, 8193, 16384 + 1, 3 * 8192 + 4232, 65535, 65536, 65537]
ENTRIES = [("single", 0), ("multi", 0), ("bg", 1), ("bg", 3), ("bg", 128), ("bg", 256)]

_BELOW = float(np.nextafter(np.float32(10.0), np.float32(0.0)))                   # total + 1e-6f rounds to 10: c == 1 exactly
_BELOW2 = float(np.nextafter(np.float32(_BELOW), np.float32(0.0)))                # c just above 1
NORMS = {"null": None, "small": 1.0, "at": 100.0, "at+3ulp": float(np.nextafter(np.nextafter(np.nextafter(100.0, 200.0), 200.0), 200.0)),
         "at-3ulp": float(np.nextafter(np.nextafter(np.nextafter(100.0, 0.0), 0.0), 0.0)), "c==1": _BELOW ** 2, "c>1": _BELOW2 ** 2,
         "0.37": (10.0 / 0.37) ** 2}


def _lib():
    from yolo._hip import lib
    return lib()


def _stream():
    from yolo._hip import stream
    return stream()


def _last_error():
    return _lib().yolo_hip_last_error().decode(errors="replace")


def _inputs(sizes, seed):
    """per tensor p, g, m, v fp32 on the device: |g| log-uniform in [1e-6, 1e3] with random sign, m and v a previous state of that scale"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for n in sizes:
        r = lambda: torch.rand(n, generator=gen, dtype=torch.float64, device="cuda")
        mag = torch.exp(r() * (np.log(1e3) - np.log(1e-6)) + np.log(1e-6))
        g = (mag * torch.where(r() < 0.5, -1.0, 1.0)).float()
        m = (mag * (r() * 2 - 1)).float()
        v = (mag * (0.1 + 0.9 * r())).float() ** 2
        p = torch.randn(n, generator=gen, dtype=torch.float32, device="cuda")
        out.append((p, g, m, v))
    return out


def _run(entry, wg, bufs, hyper, step, norm, skip):
    """one optimizer pass over bufs = [(P, g, M, V, PB or None)] (Guarded, g a tensor) through one entry -> return code(s) all zero"""
    from yolo._hip import AdamTensor
    L, st = _lib(), _stream()
    nptr = ctypes.c_void_p(norm.data_ptr()) if norm is not None else None
    sptr = ctypes.c_void_p(skip.data_ptr()) if skip is not None else None
    h = (hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["wd"])
    gp = lambda g: g._base_ptr
    if entry == "single":
        for P, g, M, V, PB in bufs:
            rc = L.yolo_adam_step(P.ptr, gp(g), M.ptr, V.ptr, P.n, *h, step, nptr, MAX_NORM, PB.ptr if PB else None, st)
            assert rc == 0, _last_error()
        return
    tab = (AdamTensor * len(bufs))(*[AdamTensor(P.ptr, gp(g), M.ptr, V.ptr, PB.ptr if PB else None, P.n) for P, g, M, V, PB in bufs])
    if entry == "multi":
        rc = L.yolo_adam_step_multi(tab, len(bufs), *h, step, nptr, MAX_NORM, sptr, st)
    else:
        rc = L.yolo_adam_step_multi_bg(tab, len(bufs), *h, step, nptr, MAX_NORM, sptr, wg, st)
    assert rc == 0, _last_error()


def _gbuf(g):
    """gradient (read only) with a valid pointer even when empty"""
    G = Guarded(g)
    t = G.t
    t._base_ptr = G.ptr
    t._keep = G
    return t


def _check_case(sizes, shadow, hyper, step, norm_sq, seed, entries=ENTRIES, skip_zero=False, what=""):
    """all entries on the same inputs: p, m, v of every tensor within the reference's bound, shadow == bf16(p), guard bands and g untouched.
    -> {entry: [p tensors]} for the comparison between entries"""
    ins = _inputs(sizes, seed)
    norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda") if norm_sq is not None else None
    refs = [er.adam_ref(p, g, m, v, step=step, norm_sq=norm_sq, max_norm=MAX_NORM, **hyper) if p.numel() else None for p, g, m, v in ins]
    gs = [_gbuf(g) for _, g, _, _ in ins]
    skip = torch.zeros(1, device="cuda") if skip_zero else None
    fails, results = [], {}
    for entry, wg in entries:
        if entry == "bg" and len(sizes) > 48:
            continue
        tag = f"{what} {entry}" + (f"[{wg}]" if entry == "bg" else "")
        bufs = [(Guarded(p), g, Guarded(m), Guarded(v), Guarded(torch.zeros(p.numel(), dtype=BF, device="cuda"), BF) if sh else None)
                for (p, _, m, v), g, sh in zip(ins, gs, shadow)]
        _run(entry, wg, bufs, hyper, step, norm, None if entry == "single" else skip)
        torch.cuda.synchronize()
        worst = 0.0
        for i, ((P, g, M, V, PB), ref) in enumerate(zip(bufs, refs)):
            for B, name in ((P, "p"), (M, "m"), (V, "v"), (PB, "shadow")):
                if B is not None and not B.guards_ok():
                    fails.append(f"{tag}: tensor {i} (n={P.n}): guard band of {name} overwritten")
            if ref is not None:
                for j, (B, name) in enumerate(((P, "p"), (M, "exp_avg"), (V, "exp_avg_sq"))):
                    worst = max(worst, lr.check_values(ref[0][j], ref[1][j], B.t, name, fails, f"{tag}: tensor {i} (n={P.n})"))
                if PB is not None and not torch.equal(PB.t.view(torch.int16), P.t.to(BF).view(torch.int16)):
                    fails.append(f"{tag}: tensor {i} (n={P.n}): bf16 shadow != bf16(p)")
        results[(entry, wg)] = [torch.cat([b[0].t, b[2].t, b[3].t]) for b in bufs]
        print(f"{tag}: worst |err| / bound {worst:.3f}")
    for (_, g, _, _), G in zip(ins, gs):
        if not torch.equal(g, G) or not G._keep.guards_ok():
            fails.append(f"{what}: a gradient was written")
    keys = list(results)
    same = all(all(torch.equal(a, b) for a, b in zip(results[keys[0]], results[k])) for k in keys[1:])
    print(f"{what}: entries {'agree bit for bit' if same else 'differ in some bits (each within the bound)'}")
    assert not fails, "\n".join(fails[:12])
    return results


def test_all_sizes_one_table():
    """every edge size in one table (the empty tensor first), shadow on every second tensor, clipped; single / multi / background at 1, 3, 128, 256
    workgroups: chunk boundaries +-1, a partial chunk at beg > 0 (16385, 3*8192+4232), float4 bodies with tails of 1-3, SQ_CHUNK +-1"""
    _check_case(SIZES, [i % 2 == 1 for i in range(len(SIZES))], HYPER, 1, NORMS["0.37"], 11, what="sizes")


def test_single_tensors():
    """each size as a table of its own (chunk count below / above the workgroup count), shadow on the scalar tails"""
    for n in SIZES[1:]:
        _check_case([n], [True], HYPER, 2, NORMS["0.37"], 100 + n, entries=[("single", 0), ("multi", 0), ("bg", 3), ("bg", 256)], what=f"n={n}")


def test_large_tensor():
    """2^24 + 3 elements: 2049 chunks for every workgroup count, a 3-element tail behind the last full chunk; reference in fp64 on the device"""
    _check_case([(1 << 24) + 3], [True], HYPER, 10, NORMS["0.37"], 12, what="2^24+3")


@pytest.mark.parametrize("where", ["first", "middle", "last", "all-but-one"])
def test_empty_tensors_in_a_table(where):
    sizes = {"first": [0, 0, 8193, 5], "middle": [5, 0, 8193, 0, 0, 100], "last": [8192, 1027, 0, 0], "all-but-one": [0, 0, 3, 0]}[where]
    _check_case(sizes, [True] * len(sizes), HYPER, 1, NORMS["0.37"], 13, what=f"empty {where}")


@pytest.mark.parametrize("count", [1, 47, 48, 49, 100])
def test_table_lengths(count):
    """the multi entry splits at YOLO_MT_MAX = 48 tensors per launch; the background entry takes at most 48 and must reject more"""
    from yolo._hip import AdamTensor
    pool = [5, 8193, 1, 1027, 0, 4, 8192, 3 * 8192 + 4232, 3]
    sizes = [pool[i % len(pool)] for i in range(count)]
    _check_case(sizes, [i % 3 == 0 for i in range(count)], HYPER, 1, NORMS["0.37"], 14 + count, what=f"{count} tensors")
    if count > 48:
        x = torch.zeros(64, device="cuda")
        tab = (AdamTensor * count)(*[AdamTensor(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 4) for _ in range(count)])
        rc = _lib().yolo_adam_step_multi_bg(tab, count, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, MAX_NORM, None, 4, _stream())
        assert rc != 0 and "yolo_adam_step_multi_bg" in _last_error()
        torch.cuda.synchronize()
        assert not bool(x.any()), "a rejected call must not launch"


_HYPER_GRID = [(s, wd, b) for s in (1, 2, 10, 1000, 10 ** 6) for wd in (0.0, 5e-4) for b in ((0.9, 0.999), (0.0, 0.5))]


@pytest.mark.parametrize("idx", range(len(_HYPER_GRID)))
def test_hyper_parameters(idx):
    """step 1 .. 10^6 (bias corrections from 0.1 / 0.001 to 1), weight decay off / on, two beta pairs; the norm cases rotate through the grid and
    every second case passes a zero skip_flag"""
    step, wd, (b1, b2) = _HYPER_GRID[idx]
    name = list(NORMS)[idx % len(NORMS)]
    sizes = [8193, 4, 1027, 3 * 8192 + 4232]
    _check_case(sizes, [True, False, True, False], dict(HYPER, wd=wd, beta1=b1, beta2=b2), step, NORMS[name], 200 + idx, skip_zero=bool(idx % 2),
                what=f"step={step} wd={wd} betas=({b1}, {b2}) norm={name}")


@pytest.mark.parametrize("name", list(NORMS))
def test_clip_coefficient_cases(name):
    """norm_sq NULL, clip > 1 (no scaling), max_norm^2 +- 3 fp64 ulps (total rounds to 10.0f, 1e-6f makes c < 1 on both sides), the fp32 totals for
    which c is exactly 1 and just above (the `c < 1 ? c : 1` branch on both sides), and a real clip of 0.37"""
    if NORMS[name] is not None:
        c = er.clip_raw(NORMS[name], MAX_NORM)
        assert {"small": c > 1, "at": c < 1, "at+3ulp": c < 1, "at-3ulp": c < 1, "c==1": c == 1.0, "c>1": c > 1, "0.37": abs(c - 0.37) < 1e-6}[name]
    _check_case([8193, 5, 1024], [True, True, False], HYPER, 3, NORMS[name], 300, what=f"norm {name}")


def test_three_steps_fed_back():
    """steps 1-3 on the kernel's own outputs, each checked against the reference of that step's stored inputs (no accumulated error in the bound)"""
    sizes = [8193, 3, 3 * 8192 + 4232, 0, 1027]
    for entry, wg in ENTRIES:
        ins = _inputs(sizes, 400)
        bufs = [(Guarded(p), _gbuf(g), Guarded(m), Guarded(v), Guarded(torch.zeros(p.numel(), dtype=BF, device="cuda"), BF)) for p, g, m, v in ins]
        norm = torch.tensor([NORMS["0.37"]], dtype=torch.float64, device="cuda")
        fails = []
        for step in (1, 2, 3):
            before = [(P.t.clone(), g.clone(), M.t.clone(), V.t.clone()) for P, g, M, V, _ in bufs]
            _run(entry, wg, bufs, HYPER, step, norm, None)
            torch.cuda.synchronize()
            for i, ((P, g, M, V, PB), (p0, g0, m0, v0)) in enumerate(zip(bufs, before)):
                if not p0.numel():
                    continue
                ref, bnd = er.adam_ref(p0, g0, m0, v0, step=step, norm_sq=NORMS["0.37"], max_norm=MAX_NORM, **HYPER)
                for j, (B, nm) in enumerate(((P, "p"), (M, "exp_avg"), (V, "exp_avg_sq"))):
                    lr.check_values(ref[j], bnd[j], B.t, nm, fails, f"{entry}[{wg}] step {step} tensor {i}")
                    assert B.guards_ok()
                assert torch.equal(PB.t.view(torch.int16), P.t.to(BF).view(torch.int16)) and PB.guards_ok()
                assert not torch.equal(P.t, p0), "the step must move the parameter"
        assert not fails, "\n".join(fails)


@pytest.mark.parametrize("entry,wg", [("multi", 0), ("bg", 1), ("bg", 128)])
def test_skip_flag(entry, wg):
    """*skip_flag != 0: p, m, v and the shadow keep their bits; == 0: updated (test_hyper_parameters checks those values)"""
    sizes = [8193, 5, 0, 3 * 8192 + 4232]
    ins = _inputs(sizes, 500)
    norm = torch.tensor([NORMS["0.37"]], dtype=torch.float64, device="cuda")
    for flag in (1.0, -0.5, float("nan"), 0.0):
        bufs = [(Guarded(p), _gbuf(g), Guarded(m), Guarded(v), Guarded(torch.full((p.numel(),), 3.0, dtype=BF, device="cuda"), BF)) for p, g, m, v in ins]
        _run(entry, wg, bufs, HYPER, 1, norm, torch.tensor([flag], device="cuda"))
        torch.cuda.synchronize()
        for (P, g, M, V, PB), (p, _, m, v) in zip(bufs, ins):
            if not P.n:
                continue
            kept = torch.equal(P.t, p) and torch.equal(M.t, m) and torch.equal(V.t, v) and bool((PB.t == 3.0).all())
            moved = not torch.equal(P.t, p) and not torch.equal(M.t, m) and not torch.equal(V.t, v) and torch.equal(PB.t, P.t.to(BF))
            assert (kept if flag != 0.0 else moved), f"skip_flag {flag}: tensor of {P.n}"
            assert all(B.guards_ok() for B in (P, M, V, PB))


# ---- sum of squares, stand-alone clip --------------------------------------------------------------------------------------------------------------

def test_sumsq_single_entry():
    """yolo_sumsq_f32 onto a non-zero accumulator at every edge size and 2^24 + 3"""
    L, st = _lib(), _stream()
    gen = torch.Generator(device="cuda").manual_seed(21)
    for n in SIZES + [(1 << 24) + 3]:
        g = _gbuf(torch.randn(n, generator=gen, device="cuda") * 3)
        acc = Guarded(torch.tensor([3.25], dtype=torch.float64, device="cuda").view(torch.float32))
        assert L.yolo_sumsq_f32(g._base_ptr, n, acc.ptr, st) == 0, _last_error()
        torch.cuda.synchronize()
        got = float(acc.t.view(torch.float64)[0])
        ref, bnd = er.sumsq_ref(g, 3.25)
        print(f"sumsq n={n}: |err| / bound {abs(got - ref) / bnd if bnd else 0.0:.3f}")
        assert abs(got - ref) <= bnd, f"n={n}: got {got!r}, ref {ref!r}, bound {bnd:.3g}"
        assert acc.guards_ok() and g._keep.guards_ok()


@pytest.mark.parametrize("count", [1, 16, 48, 49, 100])
def test_sumsq_multi_entry(count):
    L, st = _lib(), _stream()
    gen = torch.Generator(device="cuda").manual_seed(22)
    sizes = SIZES[:count] if count <= len(SIZES) else [SIZES[(7 * i) % len(SIZES)] for i in range(count)]
    if count == 1:
        sizes = [3 * 65536 + 1027]
    gs = [_gbuf(torch.randn(n, generator=gen, device="cuda") * 3) for n in sizes]
    acc = Guarded(torch.tensor([3.25], dtype=torch.float64, device="cuda").view(torch.float32))
    ptrs = (ctypes.c_void_p * count)(*[g._base_ptr for g in gs])
    ns = (ctypes.c_long * count)(*sizes)
    assert L.yolo_sumsq_f32_multi(ptrs, ns, count, acc.ptr, st) == 0, _last_error()
    torch.cuda.synchronize()
    got = float(acc.t.view(torch.float64)[0])
    ref, bnd = er.sumsq_ref(gs, 3.25)
    assert abs(got - ref) <= bnd, f"{count} tensors: got {got!r}, ref {ref!r}, bound {bnd:.3g}"
    assert acc.guards_ok()


def test_sumsq_rejects_what_it_cannot_run():
    from yolo._hip import E_ARG, E_UNSUPPORTED
    L, st = _lib(), _stream()
    g = torch.ones(64, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    assert L.yolo_sumsq_f32(g.data_ptr() + 4, 8, acc.data_ptr(), st) == E_UNSUPPORTED and "16-B" in _last_error()
    assert L.yolo_sumsq_f32(None, 8, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32(g.data_ptr(), 8, None, st) == E_ARG
    assert L.yolo_sumsq_f32(g.data_ptr(), -1, acc.data_ptr(), st) == E_ARG
    ptrs, ns = (ctypes.c_void_p * 2)(g.data_ptr(), g.data_ptr() + 4), (ctypes.c_long * 2)(8, 8)
    assert L.yolo_sumsq_f32_multi(ptrs, ns, 2, acc.data_ptr(), st) == E_UNSUPPORTED and "tensor 1" in _last_error()
    ns = (ctypes.c_long * 2)(8, -8)
    assert L.yolo_sumsq_f32_multi(ptrs, ns, 2, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_multi(None, ns, 2, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_multi(ptrs, ns, -1, acc.data_ptr(), st) == E_ARG
    torch.cuda.synchronize()
    assert float(acc) == 0.0, "a rejected call must not launch"


@pytest.mark.parametrize("name", [k for k in NORMS if k != "null"])
def test_clip_scale(name):
    """g *= c where c < 1 (one fp32 product: bit-equal to g * clip_ref), untouched where c >= 1"""
    L, st = _lib(), _stream()
    norm = torch.tensor([NORMS[name]], dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(23)
    for n in (0, 1, 5, 1023, 1024, 65537, (1 << 20) + 3):
        g0 = torch.randn(n, generator=gen, device="cuda") * 100
        G = Guarded(g0)
        assert L.yolo_clip_scale_f32(G.ptr, n, norm.data_ptr(), MAX_NORM, st) == 0, _last_error()
        torch.cuda.synchronize()
        c = er.clip_raw(NORMS[name], MAX_NORM)
        want = g0 * torch.tensor(er.clip_ref(NORMS[name], MAX_NORM), dtype=torch.float32, device="cuda") if c < 1.0 else g0
        assert torch.equal(G.t.view(torch.int32), want.view(torch.int32)), f"n={n}"
        assert G.guards_ok()
    assert L.yolo_clip_scale_f32(G.ptr, 4, None, MAX_NORM, st) == -1 and L.yolo_clip_scale_f32(None, 4, norm.data_ptr(), MAX_NORM, st) == -1
    assert L.yolo_clip_scale_f32(G.ptr, -4, norm.data_ptr(), MAX_NORM, st) == -1


def test_adam_entries_reject_bad_arguments():
    """the documented codes, each checked on the host before any launch: nothing may change"""
    from yolo._hip import AdamTensor, E_ARG, E_UNSUPPORTED
    L, st = _lib(), _stream()
    x = [torch.ones(64, device="cuda") for _ in range(4)]
    sh = torch.zeros(64, dtype=BF, device="cuda")
    p, g, m, v = (t.data_ptr() for t in x)
    h = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    one = lambda **kw: L.yolo_adam_step(kw.get("p", p), kw.get("g", g), m, v, kw.get("n", 16), *h, kw.get("step", 1), None, MAX_NORM, kw.get("pb"), st)
    assert one(step=0) == E_ARG and "yolo_adam_step" in _last_error()
    assert one(n=-1) == E_ARG and one(p=None) == E_ARG and one(g=None) == E_ARG
    assert one(p=p + 4) == E_UNSUPPORTED and one(g=g + 8) == E_UNSUPPORTED
    assert one(pb=sh.data_ptr() + 2) == E_UNSUPPORTED and "8-B" in _last_error()
    T = lambda **kw: AdamTensor(kw.get("p", p), kw.get("g", g), m, v, kw.get("pb"), kw.get("n", 16))
    for fn, extra in ((L.yolo_adam_step_multi, ()), (L.yolo_adam_step_multi_bg, (4,))):
        call = lambda tab, count, step=1: fn(tab, count, *h, step, None, MAX_NORM, None, *extra, st)
        ok = (AdamTensor * 2)(T(), T())
        assert call(None, 2) == E_ARG and call(ok, -1) == E_ARG and call(ok, 2, step=0) == E_ARG
        assert call((AdamTensor * 2)(T(), T(p=None)), 2) == E_ARG and "tensor 1" in _last_error()
        assert call((AdamTensor * 2)(T(), T(n=-3)), 2) == E_ARG
        assert call((AdamTensor * 2)(T(g=g + 4), T()), 2) == E_UNSUPPORTED and "tensor 0" in _last_error()
        assert call((AdamTensor * 2)(T(), T(pb=sh.data_ptr() + 2)), 2) == E_UNSUPPORTED and "shadow 1" in _last_error()
    ok = (AdamTensor * 2)(T(), T())
    for wg in (0, -1, 257):
        assert L.yolo_adam_step_multi_bg(ok, 2, *h, 1, None, MAX_NORM, None, wg, st) == E_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in x) and not bool(sh.any())


def _table49_with_misaligned_entry_48():
    """49 tensors, one more than a launch takes -> sizes, inputs and, for the last one, a gradient that starts 4 bytes behind a 16-B boundary"""
    pool = [5, 8193, 1, 1027, 0, 4, 8192]
    sizes = [pool[i % len(pool)] for i in range(49)]
    ins = _inputs(sizes, 600)
    g48 = torch.cat([ins[48][1].new_zeros(1), ins[48][1]])[1:]
    assert g48.data_ptr() % 16 == 4 and g48.numel() == sizes[48] == 8192
    return sizes, ins, g48


def test_adam_multi_checks_every_tensor_before_the_first_launch():
    """tensor 48 is refused: the 48 tensors of the first launch keep the bits of p, exp_avg and exp_avg_sq"""
    from yolo._hip import AdamTensor, E_UNSUPPORTED
    sizes, ins, g48 = _table49_with_misaligned_entry_48()
    bufs = [(Guarded(p), Guarded(m), Guarded(v)) for p, _, m, v in ins]
    gs = [_gbuf(g) for _, g, _, _ in ins[:48]]
    gptr = [g._base_ptr for g in gs] + [g48.data_ptr()]
    tab = (AdamTensor * 49)(*[AdamTensor(P.ptr, gp, M.ptr, V.ptr, None, P.n) for (P, M, V), gp in zip(bufs, gptr)])
    h = (HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"])
    rc = _lib().yolo_adam_step_multi(tab, 49, *h, 1, None, MAX_NORM, None, _stream())
    assert rc == E_UNSUPPORTED and "tensor 48" in _last_error(), (rc, _last_error())
    torch.cuda.synchronize()
    for i, ((P, M, V), (p, _, m, v)) in enumerate(zip(bufs, ins)):
        for B, src in ((P, p), (M, m), (V, v)):
            assert torch.equal(B.t.view(torch.int32), src.view(torch.int32)) and B.guards_ok(), f"tensor {i} (n={P.n}) was written by a refused call"


def test_sumsq_multi_checks_every_tensor_before_the_first_launch():
    """the same table: the accumulator keeps its 3.25"""
    from yolo._hip import E_UNSUPPORTED
    sizes, ins, g48 = _table49_with_misaligned_entry_48()
    gs = [_gbuf(g) for _, g, _, _ in ins[:48]]
    ptrs = (ctypes.c_void_p * 49)(*[g._base_ptr for g in gs], g48.data_ptr())
    ns = (ctypes.c_long * 49)(*sizes)
    acc = Guarded(torch.tensor([3.25], dtype=torch.float64, device="cuda").view(torch.float32))
    rc = _lib().yolo_sumsq_f32_multi(ptrs, ns, 49, acc.ptr, _stream())
    assert rc == E_UNSUPPORTED and "tensor 48" in _last_error(), (rc, _last_error())
    torch.cuda.synchronize()
    assert float(acc.t.view(torch.float64)[0]) == 3.25 and acc.guards_ok(), "a refused call added the first launch's tensors"
