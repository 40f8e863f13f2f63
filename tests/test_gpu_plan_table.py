"""Every launch plan of yolo/plans/gfx950.json, launch by launch, against the fp64 reference of tests/launch_ref.py.

The four runs of tools/tune_plans.py (YOLOv1 inference, a YOLOv1 training step, ResNet-50 variant inference, a training step of that variant with the
trunk trainable) at every measured batch size, on synthetic images with Dropout p = 0.  plans._run_plan_igemm and the library's yolo_wgrad are wrapped;
for each launch the wrapper synchronises, computes the reference from the operands BEFORE the launch (so it stays right where out aliases an
operand), snapshots the whole output region [out, out + N * out_img_stride) -- halo, channel padding and other parity classes included -- and the
BatchNorm statistics accumulator, fills the addressed output elements with NaN (where out overlaps no operand), runs the real launch and checks:

  * every addressed element is finite and within its element bound (launch_ref.igemm_ref), arg-max codes included;
  * every element the descriptor does not address is bit-unchanged;
  * with bn_stats, the 16 replicas' deltas add up to the fp64 per-channel sum and sum of squares of the stored outputs;
  * a second run of the same launch gives the same bits (every shipped form is deterministic: the table has no atomic "splitk" entry);
  * each yolo_wgrad launch (both WGRAD_CHOICE entries of batch 64 among them): dw and db within 1e-3 relative L2 of fp64, and every element of
    both within launch_ref.wgrad_bound: gamma(P + ranges - 1 + accumulate) (sum |dy| |x| + |previous contents|), the absolute sums from the same
    chunk loop as the signed ones.  Worst |err| / bound over all runs: 0.992 (variant 0 flat, from batch 2 on: the Linear layers reduce over P = batch
    pixels, so their bound is two or three roundings), db 0.33, every other form below 0.01.  Wall time per batch size on one MI355X, relative-L2 check alone -> with the element check:
    batch 1: 4.9 -> 4.0 s, 2: 2.9 -> 3.0, 4: 3.1 -> 3.3, 8: 3.2 -> 3.5, 16: 3.6 -> 4.0, 32: 4.5 -> 5.2, 64: 6.2 -> 7.2 (+16 %, under the quarter
    that would have confined the element check to n <= 16), 13: 3.4 -> 3.9, 3: 2.8 -> 3.1.

Coverage: every shipped key runs with exactly its shipped plan (a pool2 = 3 launch counts for its pool2 = 1 key, and each such key also runs once with
pool2 = 1).  The wrapper synchronises around every launch, so it cannot see races between the two streams of the backward pass."""

from __future__ import annotations

import json
import math
import time
from collections import defaultdict

import pytest
import torch

import launch_ref as lr
import synth

pytestmark = pytest.mark.gpu

MEASURED = (1, 2, 4, 8, 16, 32, 64)
UNREACHABLE: dict = {}            # shipped key -> why no run reaches it (none expected)
# pooled keys (pool2 = 1) that only the training step reaches, with pool2 = 3: at these batch sizes the inference forward runs the conv and the
# MaxPool2d as two launches (Plan._few_tiles), so no run launches them with pool2 = 1
_FEW_TILES = "inference runs conv and pool unfused at this batch size (Plan._few_tiles)"
CODES_ONLY = {(1, 28, 28, 3, 3, 512, 1024, 1, 2, 1, 1024, 512): _FEW_TILES, (1, 56, 56, 3, 3, 256, 512, 1, 2, 1, 512, 256): _FEW_TILES,
              (2, 28, 28, 3, 3, 512, 1024, 1, 2, 1, 1024, 512): _FEW_TILES, (2, 56, 56, 3, 3, 256, 512, 1, 2, 1, 512, 256): _FEW_TILES,
              (4, 28, 28, 3, 3, 512, 1024, 1, 2, 1, 1024, 512): _FEW_TILES}
VALUE_IMAGES: dict = {}           # batch -> images whose values are checked (a time budget's way out; unused: every image of every launch is checked)
STATS_REL = 256 * 1.01 * 2.0 ** -24      # the statistics epilogue sums a tile's <= 256 pixels in fp32 before its fp64 atomics
WGRAD_REL_L2 = 1e-3
ELEMENT_CHECK_MAX_BATCH = 64      # yolo_wgrad launches are also checked element by element up to this batch size (timings in the docstring)
REPORT = {"igemm": defaultdict(float), "bn_stats": 0.0, "wgrad": defaultdict(float), "wgrad_elem": defaultdict(float), "launches": 0, "wgrad_launches": 0}


class _Raw:
    def __init__(self, p, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(p), False), "version": 2}


def _addr(p) -> int:
    if p is None:
        return 0
    return int(p.value or 0) if hasattr(p, "value") else int(p)


def _raw(p, lo, hi, typestr="<i2"):
    """device elements [p + lo, p + hi) as a tensor (lo <= 0), and the index of p inside it"""
    size = {"<i2": 2, "<f4": 4, "<f8": 8}[typestr]
    t = torch.as_tensor(_Raw(p + lo * size, hi - lo, typestr), device="cuda")
    return t, -lo


def _bf(t):
    return t.view(torch.bfloat16)


def _form(plan) -> str:
    if isinstance(plan[0], str):
        return f"{plan[0]}/{plan[1]}" + (f"/S{plan[2]}" if plan[0] == "slabs" else "")
    return f"single/{plan[0]}" if len(plan) == 2 else f"cut/{plan[0]}+{plan[3]}"


class Checker:
    def __init__(self, shipped, batch):
        self.shipped, self.batch = shipped, batch
        self.ran = defaultdict(set)          # shipped key -> pool2 values it ran with under its shipped plan
        self.fails = []
        self.wgrads = []                      # (variant, geo, Cout, Cin, P)

    def fail(self, msg):
        if len(self.fails) < 40:
            self.fails.append(msg)

    # ---- yolo_igemm through a launch plan ----
    def igemm(self, real_run, L_, d, plan, inp, w, bias, aux, out, st, what):
        from yolo import _hip, plans
        torch.cuda.synchronize()
        dd = _hip.IgemmDesc.from_buffer_copy(d)
        key = plans._tune_key(dd)
        if self.shipped.get(key) == tuple(plan):
            self.ran[key].add(dd.pool2)
        tag = f"{what} key {plans._key_str(key)} plan {tuple(plan)}"
        p_in, p_w, p_b, p_aux, p_out = _addr(inp), _addr(w), _addr(bias), _addr(aux), _addr(out)
        esz = 4 if dd.out_fp32 else 2
        ilo, ihi = lr.igemm_extent(dd, "in")
        x_t, x_base = _raw(p_in, ilo, ihi)
        w_t, _ = _raw(p_w, *lr.igemm_extent(dd, "w"))
        b_t = _raw(p_b, 0, dd.Cout, "<f4")[0] if p_b else None
        reads_aux = dd.epilogue in (lr.EPI_MUL_DLRELU, lr.EPI_BIAS_ADD_LRELU) and not dd.pool2
        alo, ahi = lr.igemm_extent(dd, "aux")
        a_t, a_base = _raw(p_aux, alo, ahi) if (reads_aux and p_aux) else (None, 0)
        images = VALUE_IMAGES.get(dd.N) if self.batch in VALUE_IMAGES else None
        R = lr.igemm_ref(dd, _bf(x_t), x_base, _bf(w_t), b_t, _bf(a_t) if a_t is not None else None, a_base, images=images, device="cuda")
        nreg = lr.igemm_extent(dd, "out")[1]
        region = _raw(p_out, 0, nreg, "<f4" if dd.out_fp32 else "<i2")[0]
        before = region.clone()
        full = codes = None
        if dd.pool2 == 2:
            full = _raw(p_aux, 0, ahi)[0]
        elif dd.pool2 == 3:
            codes = _raw(p_aux, *lr.igemm_extent(dd, "codes"))[0]
        full_before = full.clone() if full is not None else None
        codes_before = codes.clone() if codes is not None else None
        stats = _raw(dd.bn_stats, 0, 16 * 2 * dd.Cout, "<f8")[0] if dd.bn_stats else None
        stats_before = stats.clone() if stats is not None else None
        o0, o1 = p_out, p_out + nreg * esz
        alias = (o0 < p_in + 2 * ihi and p_in + 2 * ilo < o1) or (reads_aux and p_aux and o0 < p_aux + 2 * ahi and p_aux + 2 * alo < o1)
        vals = region if dd.out_fp32 else _bf(region)
        if not alias:
            vals[R.addressed] = math.nan
            if full is not None:
                _bf(full)[R.aux_addressed] = math.nan
        torch.cuda.synchronize()
        try:
            real_run(L_, d, plan, inp, w, bias, aux, out, st, what)
        except _hip.HipUnsupported:
            region.copy_(before)            # nothing was launched: put back what the NaN fill overwrote
            if full is not None:
                full.copy_(full_before)
            torch.cuda.synchronize()
            raise
        torch.cuda.synchronize()
        REPORT["launches"] += 1
        worst, fails = R.check(vals, _bf(full) if full is not None else None, codes, what=tag)
        form = _form(plan)
        REPORT["igemm"][form] = max(REPORT["igemm"][form], worst)
        for f in fails:
            self.fail(f)
        untouched = ~R.addressed
        if not torch.equal(region[untouched], before[untouched]):
            n = int((region[untouched] != before[untouched]).sum())
            self.fail(f"{tag}: {n} elements outside the addressed set changed")
        if full is not None and not torch.equal(full[: R.aux_addressed.numel()][~R.aux_addressed], full_before[: R.aux_addressed.numel()][~R.aux_addressed]):
            self.fail(f"{tag}: un-pooled activation written outside its addressed set")
        if codes is not None:
            words = torch.zeros(codes.numel(), dtype=torch.bool, device="cuda")
            words[torch.nonzero(R.addressed).flatten() // 8] = True
            if not torch.equal(codes[~words], codes_before[~words]):
                self.fail(f"{tag}: arg-max code words written outside the pooled map's")
        if stats is not None:
            y = lr._out_view(_bf(region), dd).double()
            want = torch.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))])
            scale = torch.stack([y.abs().sum((0, 1, 2)), (y * y).sum((0, 1, 2))]).clamp_min(1e-300)
            got = (stats - stats_before).view(16, 2, dd.Cout).sum(0)
            rel = float(((got - want).abs() / scale).max())
            REPORT["bn_stats"] = max(REPORT["bn_stats"], rel)
            if not rel <= STATS_REL:
                self.fail(f"{tag}: BatchNorm statistics off by {rel:.3g} of the sum of |values| (bound {STATS_REL:.3g})")
        if not alias:
            after = region.clone()
            stats_after = stats.clone() if stats is not None else None
            codes_after = codes.clone() if codes is not None else None
            real_run(L_, d, plan, inp, w, bias, aux, out, st, what)
            torch.cuda.synchronize()
            if not torch.equal(region, after) or (codes is not None and not torch.equal(codes, codes_after)):
                n = int((region != after).sum())
                self.fail(f"{tag}: a second run differs in {n} elements (not deterministic)")
            if stats is not None:
                stats.copy_(stats_after)
                torch.cuda.synchronize()

    # ---- yolo_wgrad ----
    def wgrad(self, real, wd_ref, x, dy, dw, db, st):
        from yolo import _hip
        torch.cuda.synchronize()
        d = _hip.WgradDesc.from_buffer_copy(wd_ref._obj if hasattr(wd_ref, "_obj") else wd_ref)
        tag = f"yolo_wgrad P {d.P} Cout {d.Cout} Cin {d.Cin} K {d.KH}x{d.KW} variant {d.variant} geo_W {d.geo_W} split {d.split}"
        x_t, x_base = _raw(_addr(x), *lr.wgrad_extent(d, "x"))
        dy_lo, dy_hi = lr.wgrad_extent(d, "dy")
        dy_t, dy_base = _raw(_addr(dy), min(0, dy_lo), dy_hi)
        elem = self.batch <= ELEMENT_CHECK_MAX_BATCH
        refs = lr.wgrad_ref(d, _bf(x_t), x_base, _bf(dy_t), dy_base, device="cuda", absolute=elem)
        ref_dw, ref_db = refs[:2]
        dw_t = _raw(_addr(dw), *lr.wgrad_extent(d, "dw"), "<f4")[0]
        db_t = _raw(_addr(db), 0, d.Cout, "<f4")[0] if _addr(db) else None
        dw0 = dw_t.double().clone()
        db0 = db_t.double().clone() if db_t is not None else None
        torch.cuda.synchronize()
        rc = real(wd_ref, x, dy, dw, db, st)
        if rc != 0:
            return rc
        torch.cuda.synchronize()
        REPORT["wgrad_launches"] += 1
        self.wgrads.append((d.variant, bool(d.geo_W), d.Cout, d.Cin, d.P))
        if d.accumulate:
            want = dw0 + ref_dw.reshape(-1)
        else:
            if not d.slabs and d.split != 1 and bool((dw0 != 0).any()):
                self.fail(f"{tag}: dw was not zero-filled before a launch that accumulates into it")
            want = ref_dw.reshape(-1)
        form = f"variant {d.variant} {'geo' if d.geo_W else 'flat'}"
        e = lr.rel_l2(dw_t, want)
        REPORT["wgrad"][form] = max(REPORT["wgrad"][form], e)
        if not e <= WGRAD_REL_L2:
            self.fail(f"{tag}: dw off by {e:.3g} relative L2")
        if db_t is not None:
            e = lr.rel_l2(db_t, db0 + ref_db)
            REPORT["wgrad"]["db"] = max(REPORT["wgrad"]["db"], e)
            if not e <= WGRAD_REL_L2:
                self.fail(f"{tag}: db off by {e:.3g} relative L2")
        if elem:
            # element by element: |err| <= gamma(P + ranges - 1 + a) (sum |dy| |x| + |previous|), ranges = split or the 512 workgroup slots.  In slab
            # mode (not part of these runs) db may be stored instead of added to, so only dw is checked there.
            b = lr.wgrad_bound(d, None, 0, None, 0, dw0=dw0 if d.accumulate else None, db0=db0 if (db_t is not None and not d.slabs) else None, refs=refs,
                               device="cuda")
            fails = []
            w = lr.check_values(b.dw, b.dw_bnd, dw_t, "dw", fails, tag)
            REPORT["wgrad_elem"][form] = max(REPORT["wgrad_elem"][form], w)
            if db_t is not None and not d.slabs:
                w = lr.check_values(b.db, b.db_bnd, db_t, "db", fails, tag)
                REPORT["wgrad_elem"]["db"] = max(REPORT["wgrad_elem"]["db"], w)
            for f in fails:
                self.fail(f)
        return rc


class _LibProxy:
    """the library with yolo_wgrad wrapped; everything else forwarded"""

    def __init__(self, real_lib, chk):
        self._real, self._chk = real_lib, chk

    def __getattr__(self, name):
        return getattr(self._real, name)

    def yolo_wgrad(self, *args):
        return self._chk.wgrad(self._real.yolo_wgrad, *args)


@pytest.fixture
def shipped_table(monkeypatch):
    """the shipped table, loaded fresh (earlier tests add default entries to the process-wide one), restored afterwards"""
    from yolo import engine, plans
    saved, saved_borrowed, saved_choice = dict(plans._TUNED), set(plans._BORROWED), engine.WGRAD_CHOICE
    plans._TUNED.clear()
    plans._BORROWED.clear()
    plans.load_plans(plans.PLAN_FILE)
    with open(plans.PLAN_FILE) as f:
        shipped = {tuple(int(t) for t in k.split(",")): tuple(v) for k, v in json.load(f)["plans"].items()}
    assert engine.SMALL_SPLIT and engine.PLAN_TABLE and not engine.AUTOTUNE
    try:
        yield shipped
    finally:
        plans._TUNED.clear()
        plans._TUNED.update(saved)
        plans._BORROWED.clear()
        plans._BORROWED.update(saved_borrowed)
        engine.WGRAD_CHOICE = saved_choice


def _drive(n, chk, monkeypatch):
    """the four runs of tools/tune_plans.py at batch n under the checking wrappers"""
    from yolo import ResNetBackbone, YOLOLoss, YOLOv1, engine, plans
    real_run, real_lib = plans._run_plan_igemm, engine.lib
    proxy = _LibProxy(real_lib(), chk)
    monkeypatch.setattr(plans, "_run_plan_igemm", lambda *a: chk.igemm(real_run, *a))
    monkeypatch.setattr(engine, "lib", lambda: proxy)
    dev = torch.device("cuda")
    torch.manual_seed(n)
    x = torch.from_numpy(synth.synth_images(n, 23)).to(dev)
    tgt = torch.from_numpy(synth.synth_targets(n, 1)).to(dev)
    crit = YOLOLoss()

    def run(model, train):
        for mod in model.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        if train:
            model.train()
            loss, _ = crit(model(x), tgt)
            loss.backward()
        else:
            model.eval()
            with torch.no_grad():
                model(x)
        torch.cuda.synchronize()

    try:
        m = YOLOv1().to(dev)
        run(m, False)
        run(m, True)
        del m
        r = YOLOv1(backbone=ResNetBackbone(pretrained=False, freeze=True)).to(dev)
        run(r, False)
        del r
        t = YOLOv1(backbone=ResNetBackbone(pretrained=False, freeze=False)).to(dev)
        run(t, True)
        del t
    finally:
        monkeypatch.setattr(plans, "_run_plan_igemm", real_run)
        monkeypatch.setattr(engine, "lib", real_lib)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _report(n, t0):
    ig = "  ".join(f"{k} {v:.3f}" for k, v in sorted(REPORT["igemm"].items()))
    wg = "  ".join(f"{k} {v:.2e}" for k, v in sorted(REPORT["wgrad"].items()))
    we = "  ".join(f"{k} {v:.3f}" for k, v in sorted(REPORT["wgrad_elem"].items()))
    print(f"\nbatch {n}: {time.time() - t0:.1f} s; {REPORT['launches']} igemm launches, {REPORT['wgrad_launches']} wgrad launches so far\n"
          f"  worst |err| / bound per plan form: {ig}\n  BatchNorm statistics: {REPORT['bn_stats']:.3g} of sum |v|\n  wgrad relative L2: {wg}\n  wgrad worst |err| / element bound: {we}", flush=True)


@pytest.mark.parametrize("n", MEASURED)
def test_every_shipped_plan_of_a_batch_size_computes_its_launch(n, shipped_table, monkeypatch):
    t0 = time.time()
    chk = Checker(shipped_table, n)
    _drive(n, chk, monkeypatch)
    _report(n, t0)
    assert not chk.fails, "\n".join(chk.fails)
    mine = {k for k in shipped_table if k[0] == n}
    ran = set(chk.ran)
    missing = sorted(mine - ran - set(UNREACHABLE))
    assert not missing, f"{len(missing)} of {len(mine)} shipped keys of batch {n} never ran with their shipped plan: {missing[:10]}"
    no_pool1 = sorted(k for k in ran if k[9] == 1 and 1 not in chk.ran[k] and k not in CODES_ONLY)
    assert not no_pool1, f"pooled keys that ran only with pool2 = 3: {no_pool1}"
    assert len(ran & mine) + len(set(UNREACHABLE) & mine) == len(mine)
    print(f"  coverage: {len(ran & mine)} / {len(mine)} shipped keys of batch {n}", flush=True)
    if n == 64:
        # the weight-gradient table choices (variant 6; 14x14 1024 <- 512 over the interior pixels, 28x28 512 <- 256 over every slot)
        assert any(v == 6 and geo and co == 1024 and ci == 512 for v, geo, co, ci, _ in chk.wgrads), chk.wgrads
        assert any(v == 6 and not geo and co == 512 and ci == 256 for v, geo, co, ci, _ in chk.wgrads), chk.wgrads
    assert chk.wgrads


@pytest.mark.parametrize("n", [13, 3])
def test_borrowed_and_default_plans_compute_their_launches(n, shipped_table, monkeypatch):
    """batch sizes without measured plans: 13 borrows the plans of the nearest measured batch size, 3 takes the default rules"""
    t0 = time.time()
    chk = Checker(shipped_table, n)
    _drive(n, chk, monkeypatch)
    _report(n, t0)
    assert not chk.fails, "\n".join(chk.fails)
    assert REPORT["launches"] > 0 and chk.wgrads
