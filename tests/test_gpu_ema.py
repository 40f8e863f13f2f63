"""The three EMA entries of csrc/ema.hip, called through the C ABI as tests/test_gpu_sgd.py calls the SGD entries, against tests/ema_ref.py:
every element of the average within the bound of the two fp32 roundings, every average between guard bands of a NaN pattern (4096 floats behind
it), p untouched.  The kernels write the update as one subtraction and one explicit fused multiply-add, so the single, multi-tensor and background
forms must agree BIT FOR BIT, and so must a repeated launch.  The last test runs yolo.optim.ModelEMA on the YOLOv1 model, with the Linear layers
averaged on the optimizer's second stream, in a child process."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

import ema_ref as emr
import launch_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 3, 255, 256, 257, 65536 + 5, (1 << 20) + 3]
POOL = [5, 8193, 1, 1027, 0, 4, 8192, 3 * 8192 + 4232, 3, 0]
TABLE50 = [POOL[i % len(POOL)] for i in range(50)]            # crosses YOLO_MT_MAX = 48; empty tensors inside and at the end of a launch
WEIGHTS = [0.0, 1.0, 1e-4, 0.5]
BAND = 4096                                                   # floats of NaN pattern behind (and in front of) every average
PAT = 0x7FC00D1E


def _lib():
    from yolo._hip import lib
    return lib()


def _stream():
    from yolo._hip import stream
    return stream()


def _last_error():
    return _lib().yolo_hip_last_error().decode(errors="replace")


class Banded:
    """a copy of `src` between two 4096-float bands of a NaN pattern inside one allocation (16-B aligned, valid pointer for an empty tensor)"""

    def __init__(self, src):
        self.n = src.numel()
        self.raw = torch.full((self.n + 2 * BAND,), PAT, dtype=torch.int32, device=src.device)
        self.t = self.raw.view(torch.float32)[BAND: BAND + self.n]
        self.t.copy_(src)
        self.ptr = self.raw.data_ptr() + 4 * BAND

    def bands_ok(self):
        return bool((self.raw[:BAND] == PAT).all()) and bool((self.raw[BAND + self.n:] == PAT).all())


@pytest.fixture(scope="module")
def inputs():
    """{table name: [(e, p)]} fp32 on the device, and a cache of the references per (table, w): computed once, never written"""
    gen = torch.Generator(device="cuda").manual_seed(17)
    out = {}
    for name, sizes in (("sizes", SIZES), ("table50", TABLE50)):
        tab = []
        for i, n in enumerate(sizes):
            e = torch.randn(n, generator=gen, device="cuda")
            p = e + torch.randn(n, generator=gen, device="cuda") * (1e-3 if i % 2 else 1.0)      # a trained weight near its average, and one far from it
            tab.append((e, p))
        out[name] = tab
    return out, {}


def _refs(inputs, name, w):
    tabs, cache = inputs
    if (name, w) not in cache:
        cache[(name, w)] = [emr.ema_ref(e, p, w) for e, p in tabs[name]]
    return cache[(name, w)]


def _run(form, wg, E, P, w, skip=None):
    """one pass over the Banded lists E (written) and P (read) through one launch form; the return code must be 0"""
    from yolo._hip import EmaTensor
    L, st = _lib(), _stream()
    sptr = ctypes.c_void_p(skip.data_ptr()) if skip is not None else None
    if form == "single":
        for e, p in zip(E, P):
            assert L.yolo_ema_update(e.ptr, p.ptr, e.n, w, sptr, st) == 0, _last_error()
        return
    tab = (EmaTensor * len(E))(*[EmaTensor(e.ptr, p.ptr, e.n) for e, p in zip(E, P)])
    if form == "multi":
        rc = L.yolo_ema_update_multi(tab, len(E), w, sptr, st)
    else:
        rc = L.yolo_ema_update_multi_bg(tab, len(E), w, sptr, wg, st)
    assert rc == 0, _last_error()


def _forms(count):
    """the launch forms a table of `count` tensors can take: the background form holds at most 48 (refused above, see the argument test)"""
    return [("single", 0), ("multi", 0)] + ([("bg", 1), ("bg", 128), ("bg", 256)] if count <= 48 else [])


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("name", ["sizes", "table50", "table48"])
def test_all_forms_within_the_bound_and_bit_equal(inputs, name, w):
    """every launch form on the same inputs: within the reference's bound, guard bands intact, p untouched; all forms and a repeated launch
    the same bits.  table48: the first 48 tensors of the 50, so that the background form runs a full table with empty tensors in it"""
    w = emr._f32(w)
    src = "table50" if name == "table48" else name
    count = 48 if name == "table48" else len(inputs[0][src])
    data, refs = inputs[0][src][:count], _refs(inputs, src, w)[:count]
    fails, results = [], {}
    for form, wg in _forms(count) + [("multi", 0)]:                       # the multi form twice: the repeat launch
        tag = f"{name} w={w} {form}" + (f"[{wg}]" if form == "bg" else "")
        E, P = [Banded(e) for e, _ in data], [Banded(p) for _, p in data]
        _run(form, wg, E, P, w)
        torch.cuda.synchronize()
        worst = 0.0
        for i, (e, p, (ref, bnd), (e0, p0)) in enumerate(zip(E, P, refs, data)):
            where = f"{tag}: tensor {i} (n={e.n})"
            if not (e.bands_ok() and p.bands_ok()):
                fails.append(f"{where}: a guard band was overwritten")
            if not torch.equal(p.t.view(torch.int32), p0.view(torch.int32)):
                fails.append(f"{where}: p was written")
            if e.n:
                worst = max(worst, lr.check_values(ref, bnd, e.t, "ema", fails, where))
                if w == 0.0 and not torch.equal(e.t.view(torch.int32), e0.view(torch.int32)):
                    fails.append(f"{where}: w = 0 must leave the average as it is")
        print(f"{tag}: worst |err| / bound {worst:.3f}")
        results.setdefault((form, wg), []).append([e.t.view(torch.int32).clone() for e in E])
    first = results[("single", 0)][0]
    for key, runs in results.items():
        for r in runs:
            if not all(torch.equal(a, b) for a, b in zip(first, r)):
                fails.append(f"{name} w={w}: {key} and the single form differ in some bits")
    assert len(results[("multi", 0)]) == 2
    assert not fails, "\n".join(fails[:12])


@pytest.mark.parametrize("form,wg", [("single", 0), ("multi", 0), ("bg", 1), ("bg", 128)])
def test_skip_flag(inputs, form, wg):
    """*skip_flag != 0: the averages keep their bytes, guard bands included; == 0: updated"""
    data = inputs[0]["sizes"]
    for flag in (1.0, -0.5, float("nan"), 0.0):
        E, P = [Banded(e) for e, _ in data], [Banded(p) for _, p in data]
        raw = [e.raw.clone() for e in E]
        _run(form, wg, E, P, 0.5, torch.tensor([flag], device="cuda"))
        torch.cuda.synchronize()
        for e, r0 in zip(E, raw):
            kept = torch.equal(e.raw, r0)
            assert kept if (flag != 0.0 or not e.n) else (not kept and e.bands_ok()), f"skip_flag {flag}: tensor of {e.n}"


def test_ema_entries_reject_bad_arguments():
    """the documented codes, each checked on the host before any launch: nothing may change"""
    from yolo._hip import E_ARG, E_UNSUPPORTED, EmaTensor as T
    L, st = _lib(), _stream()
    a, b = torch.ones(256, device="cuda"), torch.full((256,), 2.0, device="cuda")
    e, p = a.data_ptr(), b.data_ptr()
    one = lambda **k: L.yolo_ema_update(k.get("e", e), k.get("p", p), k.get("n", 16), k.get("w", 0.5), None, st)
    assert one(e=None) == E_ARG and one(p=None) == E_ARG and one(n=-1) == E_ARG and "yolo_ema_update" in _last_error()
    for w in (-1e-6, 1.0001, float("nan"), float("inf")):
        assert one(w=w) == E_ARG, w
    assert one(e=e + 4) == E_UNSUPPORTED and one(p=p + 4) == E_UNSUPPORTED and "16-B" in _last_error()
    assert one(p=e) == E_UNSUPPORTED and one(p=e + 48) == E_UNSUPPORTED and one(e=e + 48, p=e) == E_UNSUPPORTED and "overlaps" in _last_error()
    ok = (T * 2)(T(e, p, 16), T(e + 512, p + 512, 16))
    for fn, extra in ((L.yolo_ema_update_multi, ()), (L.yolo_ema_update_multi_bg, (4,))):
        call = lambda tab, count, w=0.5: fn(tab, count, w, None, *extra, st)
        assert call(None, 2) == E_ARG and call(ok, -1) == E_ARG and call(ok, 2, w=2.0) == E_ARG and call(ok, 2, w=float("nan")) == E_ARG
        assert call((T * 2)(T(e, p, 16), T(None, p, 16)), 2) == E_ARG and "tensor 1" in _last_error()
        assert call((T * 2)(T(e, p, 16), T(e, None, 16)), 2) == E_ARG and call((T * 2)(T(e, p, 16), T(e + 512, p + 512, -2)), 2) == E_ARG
        # the refused tensor is the LAST of the table: the valid one in front of it must not have been launched either
        assert call((T * 2)(T(e, p, 16), T(e + 512, p + 516, 16)), 2) == E_UNSUPPORTED and "tensor 1" in _last_error()
        assert call((T * 2)(T(e, p, 16), T(e + 512, e + 512 + 16, 16)), 2) == E_UNSUPPORTED and "overlaps" in _last_error()
    for wg in (0, -1, 257):
        assert L.yolo_ema_update_multi_bg(ok, 2, 0.5, None, wg, st) == E_ARG
    many = (T * 49)(*[T(e + 16 * i, p + 16 * i, 4) for i in range(49)])
    assert L.yolo_ema_update_multi_bg(many, 49, 0.5, None, 4, st) == E_ARG and "yolo_ema_update_multi_bg" in _last_error()
    # 49 tensors through the multi entry, the 49th refused: the first launch (48 tensors) must not have happened
    many[48] = T(e + 16 * 48, p + 16 * 48 + 4, 4)
    assert L.yolo_ema_update_multi(many, 49, 0.5, None, st) == E_UNSUPPORTED and "tensor 48" in _last_error()
    torch.cuda.synchronize()
    assert bool((a == 1).all()) and bool((b == 2).all()), "a refused call must not launch"


def test_model_ema_follows_the_background_update(tmp_path):
    """tests/ema_child.py in a fresh process: ModelEMA beside yolo.optim.Adam with the Linear layers on the second stream, three steps with nothing
    waiting in between -- within the propagated bound of the fp64 recurrence over the parameter snapshots, ema.module's plan repacks its operands,
    and under EngineConfig.DETERMINISTIC the averages are bit-equal to a run that synchronises after every call and to a second run.  A child that
    exceeds its time limit is killed (subprocess.run does that before it raises) and the test fails there."""
    out = tmp_path / "ema.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ema_child.py"), "steps", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    lines = out.read_text().splitlines()
    assert len(lines) == 7 and lines[-2:] == ["det-sync: bit-equal to det", "det-again: bit-equal to det"], lines
