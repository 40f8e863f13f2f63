"""EngineConfig.DETERMINISTIC on the GPU, launch by launch and as whole training steps.

Per launch: the slab mode of the 128 x 128 weight-gradient kernels (yolo_wgrad variants 0 / 1 / 4 with yolo_wgrad_desc.slabs), the order-fixed bias
gradient of every slab-mode kernel (variants 5 / 6 included), and the order-fixed sum of squares (yolo_sumsq_f32_fixed / yolo_sumsq_f32_multi_fixed,
sized by yolo_sumsq_fixed_slots).  Whole step: children of tests/det_child.py, a fresh process per case.

The bound of a slab-mode weight gradient.  tests/launch_ref.py gives the fp64 value of a launch (wgrad_ref); the operands are bf16, so every product
dy * x is exact in fp32 (8 + 8 significand bits) and the only roundings are the fp32 additions: an output element is the sum of P products, added in some
tree inside the MFMA accumulation of a pixel range, plus (ranges - 1) additions of the slab sum.  No term passes more than P + ranges - 1 additions
whatever the tree, each relative to a partial sum of magnitude <= sum |dy * x|, so
    |dw - ref| <= (P + ranges - 1) * 1.01 u * sum_p |dy| |x|,           u = 2^-24 (launch_ref.U; 1.01 covers the second-order terms for P < 2^16)
and the same for db with x = 1 (bf16 -> fp32 conversion is exact).  sum |dy| |x| is wgrad_ref of the absolute values."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

import elementwise_ref as er
import launch_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "det_child.py")
GUARD = 4096          # floats of NaN behind dw, db and the slab scratch


def _last_error():
    from yolo._hip import lib
    return lib().yolo_hip_last_error().decode(errors="replace")


def wgrad_case(geo, Cin, K, Cout=256):
    """-> (x Act, dy Act, descriptor arguments without split / variant) of one weight-gradient problem; ragged pixel counts (not multiples of 64)"""
    from yolo.engine import Act
    dev = torch.device("cuda")
    N, H, W = (8, 14, 18) if geo == "stride2" else (4, 13, 17)
    pad = K // 2
    x, dy = Act(N, H, W, Cin, 1, dev), Act(N, H, W, Cout, 1, dev)
    g = torch.Generator(device="cuda").manual_seed(1000 * Cin + 10 * K + len(geo))
    x.interior().copy_(torch.randn(N, H, W, Cin, device="cuda", generator=g).to(torch.bfloat16))
    v = (torch.randn(N, H, W, Cout, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    if geo == "stride2":      # the zero-stuffed gradient of a stride-2 conv: values on the even pixels of the input's geometry
        m = torch.zeros(N, H, W, 1, device="cuda", dtype=torch.bfloat16)
        m[:, ::2, ::2] = 1
        v = v * m
    dy.interior().copy_(v)
    if geo == "flat":
        args = dict(P=dy.slots)
    elif geo == "interior":
        args = dict(P=N * H * W, geo_W=W, geo_H=H, geo_img_slots=dy.Hp * dy.Wp, geo_row_slots=dy.Wp, geo_px_slots=1, geo_slot0=dy.halo * dy.Wp + dy.halo)
    else:
        args = dict(P=N * (H // 2) * (W // 2), geo_W=W // 2, geo_H=H // 2, geo_img_slots=dy.Hp * dy.Wp, geo_row_slots=2 * dy.Wp, geo_px_slots=2,
                    geo_slot0=dy.halo * dy.Wp + dy.halo)
    args.update(dy_px_stride=dy.px_stride, x_px_stride=x.px_stride, Cout=Cout, Cin=Cin, KH=K, KW=K, pad=pad, x_row_stride=x.row_stride)
    return x, dy, args


def _desc(args, split, variant):
    from yolo._hip import WgradDesc
    d = WgradDesc()
    for k, v in args.items():
        setattr(d, k, v)
    d.split, d.accumulate, d.variant = split, 0, variant
    return d


def _ranges(d):
    """upper bound of the pixel ranges a tile of this launch is split into: the library never uses more than 512 (its workgroup slots), a uniform
    split exactly `split`"""
    return d.split if d.split > 0 else 512


def _guarded(n, fill=float("nan")):
    t = torch.full((n + GUARD,), float("nan"), device="cuda")      # the band behind the n floats is always NaN, whatever the buffer starts as
    t[:n] = fill
    return t, t[:n]


def _launch(d, x, dy, slabs_n, db_fill=float("nan")):
    from yolo._hip import check, lib, ptr, stream
    n_dw = d.Cout * d.KH * d.KW * d.Cin
    dw_all, dw = _guarded(n_dw)
    db_all, db = _guarded(d.Cout, db_fill)
    sl_all, sl = _guarded(slabs_n)
    d.slabs, d.slab_floats = (sl.data_ptr(), slabs_n) if slabs_n else (None, 0)
    check(lib().yolo_wgrad(ctypes.byref(d), x.p, dy.p, ptr(dw), ptr(db), stream()), "yolo_wgrad")
    torch.cuda.synchronize()
    for name, full, n in (("dw", dw_all, n_dw), ("db", db_all, d.Cout), ("slabs", sl_all, slabs_n)):
        assert bool(torch.isnan(full[n:]).all()), f"guard band behind {name} was written"
    return dw, db


def _need(d):
    from yolo._hip import check, lib
    need = ctypes.c_long(-1)
    check(lib().yolo_wgrad_slab_floats(ctypes.byref(d), ctypes.byref(need)), "yolo_wgrad_slab_floats")
    return need.value


@pytest.mark.parametrize("variant", [1, 4])
@pytest.mark.parametrize("split", [0, 3])
@pytest.mark.parametrize("geo", ["flat", "interior", "stride2"])
@pytest.mark.parametrize("Cin,K", [(64, 3), (128, 1), (192, 3), (512, 1), (128, 3)])
def test_wgrad_128_slab_mode(variant, split, geo, Cin, K):
    """variants 0 / 1 / 4 with slabs: dw, db and the scratch arrive as NaN; two launches bit-equal in dw and db; both within the derived bound of the
    fp64 reference; guard bands untouched; a scratch one float short refused"""
    from yolo._hip import lib, ptr, stream
    x, dy, args = wgrad_case(geo, Cin, K)
    d = _desc(args, split, variant)
    need = _need(d)
    assert need > 0 and need % 4 == 0, f"need {need}: the case must split a tile"
    runs = [_launch(d, x, dy, need) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]), "dw differs between two launches"
    assert torch.equal(runs[0][1], runs[1][1]), "db differs between two launches"
    dref = _desc(args, split, variant)
    ref_dw, ref_db = lr.wgrad_ref(dref, x.store, x.t.storage_offset(), dy.store, dy.t.storage_offset(), device="cuda")
    abs_dw, abs_db = lr.wgrad_ref(dref, x.store.abs(), x.t.storage_offset(), dy.store.abs(), dy.t.storage_offset(), device="cuda")
    n_add = d.P + _ranges(d) - 1
    fails = []
    w_dw = lr.check_values(ref_dw.reshape(-1), (n_add * 1.01 * lr.U * abs_dw).reshape(-1), runs[0][0], "dw", fails, f"variant {variant} split {split} {geo}")
    w_db = lr.check_values(ref_db, n_add * 1.01 * lr.U * abs_db, runs[0][1], "db", fails, f"variant {variant} split {split} {geo}")
    print(f"variant {variant} split {split} {geo} Cin {Cin} K {K}: need {need}, worst |err| / bound dw {w_dw:.4f} db {w_db:.4f}")
    assert not fails, fails
    d.slab_floats = need - 1
    dw = torch.zeros(d.Cout * K * K * Cin, device="cuda")
    db = torch.zeros(d.Cout, device="cuda")
    assert lib().yolo_wgrad(ctypes.byref(d), x.p, dy.p, ptr(dw), ptr(db), stream()) != 0 and "slabs hold" in _last_error()
    torch.cuda.synchronize()
    assert not bool(dw.any()) and not bool(db.any()), "a refused launch wrote"


@pytest.mark.parametrize("variant", [1, 4])
def test_wgrad_128_unsplit_tiles_keep_their_direct_store(variant):
    """a launch the library's schedule does not split needs no slabs and is bit-equal to the plain split = 1 launch; variants 2 / 3 and accumulate
    stay refused"""
    from yolo._hip import E_UNSUPPORTED, lib, ptr, stream
    from yolo.engine import Act
    dev = torch.device("cuda")
    N, H, W, Cin, Cout = 1, 5, 6, 128, 256         # 56 slots: one K step, nothing to split
    x, dy = Act(N, H, W, Cin, 1, dev), Act(N, H, W, Cout, 1, dev)
    x.interior().copy_(torch.randn(N, H, W, Cin, device="cuda").to(torch.bfloat16))
    dy.interior().copy_(torch.randn(N, H, W, Cout, device="cuda").to(torch.bfloat16))
    args = dict(P=dy.slots, dy_px_stride=dy.px_stride, x_px_stride=x.px_stride, Cout=Cout, Cin=Cin, KH=3, KW=3, pad=1, x_row_stride=x.row_stride)
    d0 = _desc(args, 0, variant)
    assert _need(d0) == 0
    a = _launch(_desc(args, 1, variant), x, dy, 0, db_fill=0.0)
    scratch = torch.full((1024,), float("nan"), device="cuda")
    d0.slabs, d0.slab_floats = scratch.data_ptr(), scratch.numel()
    dw = torch.full((Cout * 9 * Cin,), float("nan"), device="cuda")
    db = torch.zeros(Cout, device="cuda")
    assert lib().yolo_wgrad(ctypes.byref(d0), x.p, dy.p, ptr(dw), ptr(db), stream()) == 0, _last_error()
    torch.cuda.synchronize()
    assert torch.equal(dw, a[0]) and torch.equal(db, a[1]) and bool(torch.isnan(scratch).all())
    for bad in (_desc(args, 3, 2), _desc(args, 3, 3)):
        bad.slabs, bad.slab_floats = scratch.data_ptr(), scratch.numel()
        assert lib().yolo_wgrad(ctypes.byref(bad), x.p, dy.p, ptr(dw), ptr(db), stream()) == E_UNSUPPORTED
    acc = _desc(args, 3, variant)
    acc.accumulate = 1
    acc.slabs, acc.slab_floats = scratch.data_ptr(), scratch.numel()
    assert lib().yolo_wgrad(ctypes.byref(acc), x.p, dy.p, ptr(dw), ptr(db), stream()) == E_UNSUPPORTED


@pytest.mark.parametrize("variant", [5, 6])
@pytest.mark.parametrize("split", [0, 3])
def test_wgrad_pipelined_slab_mode_bias_is_order_fixed(variant, split):
    """variants 5 / 6 with slabs: db (NaN before the launch: it is stored, not accumulated) bit-equal across two launches and within the bound"""
    x, dy, args = wgrad_case("interior", 512, 3, Cout=512)
    d = _desc(args, split, variant)
    need = _need(d)
    assert need > 0 and need % (256 * 256) == 0
    runs = [_launch(d, x, dy, need) for _ in range(2)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])
    dref = _desc(args, split, variant)
    ref_dw, ref_db = lr.wgrad_ref(dref, x.store, x.t.storage_offset(), dy.store, dy.t.storage_offset(), device="cuda")
    _, abs_db = lr.wgrad_ref(dref, x.store.abs(), x.t.storage_offset(), dy.store.abs(), dy.t.storage_offset(), device="cuda")
    fails = []
    lr.check_values(ref_db, (d.P + (split if split else 256) - 1) * 1.01 * lr.U * abs_db, runs[0][1], "db", fails, f"variant {variant} split {split}")
    assert not fails, fails
    assert lr.rel_l2(runs[0][0], ref_dw.reshape(-1)) < 1e-3


# ---- order-fixed sum of squares -----------------------------------------------------------------------------------------------------------------------

SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1027, 8191, 8192, 8193, 16384 + 1, 3 * 8192 + 4232, 65535, 65536, 65537]      # those of tests/test_gpu_optim.py


def _gbuf(g):
    G = er.Guarded(g)
    t = G.t
    t._base_ptr = G.ptr
    t._keep = G
    return t


def _slots(sizes):
    from yolo._hip import check, lib
    ns = (ctypes.c_long * max(len(sizes), 1))(*sizes)
    out = ctypes.c_long(-1)
    check(lib().yolo_sumsq_fixed_slots(ns, len(sizes), ctypes.byref(out)), "yolo_sumsq_fixed_slots")
    assert out.value == sum((n + 65535) // 65536 for n in sizes)
    return out.value


def _fixed_run(gs, sizes, single):
    from yolo._hip import lib, stream
    L, st = lib(), stream()
    slots = _slots(sizes)
    scratch = er.Guarded(torch.full((2 * max(slots, 1),), float("nan"), device="cuda"))         # doubles as pairs of floats
    acc = er.Guarded(torch.tensor([3.25], dtype=torch.float64, device="cuda").view(torch.float32))
    if single:
        rc = L.yolo_sumsq_f32_fixed(gs[0]._base_ptr, sizes[0], scratch.ptr, slots, acc.ptr, st)
    else:
        ptrs = (ctypes.c_void_p * len(gs))(*[g._base_ptr for g in gs])
        ns = (ctypes.c_long * len(gs))(*sizes)
        rc = L.yolo_sumsq_f32_multi_fixed(ptrs, ns, len(gs), scratch.ptr, slots, acc.ptr, st)
    assert rc == 0, _last_error()
    torch.cuda.synchronize()
    assert acc.guards_ok() and scratch.guards_ok() and all(g._keep.guards_ok() for g in gs)
    return acc.t.view(torch.float64)[0].clone()


def test_sumsq_fixed_single_entry():
    gen = torch.Generator(device="cuda").manual_seed(21)
    for n in SIZES + [(1 << 24) + 3]:
        g = _gbuf(torch.randn(n, generator=gen, device="cuda") * 3)
        a, b = _fixed_run([g], [n], True), _fixed_run([g], [n], True)
        assert a.view(torch.int64) == b.view(torch.int64), f"n={n}: two launches differ as doubles"
        ref, bnd = er.sumsq_ref(g, 3.25)
        print(f"sumsq_fixed n={n}: |err| / bound {abs(float(a) - ref) / bnd if bnd else 0.0:.3f}")
        assert abs(float(a) - ref) <= bnd, f"n={n}: got {float(a)!r}, ref {ref!r}, bound {bnd:.3g}"


@pytest.mark.parametrize("count", [1, 16, 48, 49, 100])
def test_sumsq_fixed_multi_entry(count):
    gen = torch.Generator(device="cuda").manual_seed(22)
    sizes = SIZES[:count] if count <= len(SIZES) else [SIZES[(7 * i) % len(SIZES)] for i in range(count)]
    if count == 1:
        sizes = [3 * 65536 + 1027]
    gs = [_gbuf(torch.randn(n, generator=gen, device="cuda") * 3) for n in sizes]
    a, b = _fixed_run(gs, sizes, False), _fixed_run(gs, sizes, False)
    assert a.view(torch.int64) == b.view(torch.int64), "two launches differ as doubles"
    ref, bnd = er.sumsq_ref(gs, 3.25)
    assert abs(float(a) - ref) <= bnd, f"{count} tensors: got {float(a)!r}, ref {ref!r}, bound {bnd:.3g}"


def test_sumsq_fixed_rejects_what_it_cannot_run():
    from yolo._hip import E_ARG, E_UNSUPPORTED, lib, stream
    L, st = lib(), stream()
    g = torch.ones(64, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    sc = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert L.yolo_sumsq_f32_fixed(g.data_ptr() + 4, 8, sc.data_ptr(), 8, acc.data_ptr(), st) == E_UNSUPPORTED and "16-B" in _last_error()
    assert L.yolo_sumsq_f32_fixed(None, 8, sc.data_ptr(), 8, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_fixed(g.data_ptr(), 8, sc.data_ptr(), 8, None, st) == E_ARG
    assert L.yolo_sumsq_f32_fixed(g.data_ptr(), -1, sc.data_ptr(), 8, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_fixed(g.data_ptr(), 8, None, 8, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_fixed(g.data_ptr(), 8, sc.data_ptr(), 0, acc.data_ptr(), st) == E_ARG and "scratch holds" in _last_error()
    ptrs, ns = (ctypes.c_void_p * 2)(g.data_ptr(), g.data_ptr() + 4), (ctypes.c_long * 2)(8, 8)
    assert L.yolo_sumsq_f32_multi_fixed(ptrs, ns, 2, sc.data_ptr(), 8, acc.data_ptr(), st) == E_UNSUPPORTED and "tensor 1" in _last_error()
    ns = (ctypes.c_long * 2)(8, -8)
    assert L.yolo_sumsq_f32_multi_fixed(ptrs, ns, 2, sc.data_ptr(), 8, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_multi_fixed(None, ns, 2, sc.data_ptr(), 8, acc.data_ptr(), st) == E_ARG
    assert L.yolo_sumsq_f32_multi_fixed(ptrs, ns, -1, sc.data_ptr(), 8, acc.data_ptr(), st) == E_ARG
    out = ctypes.c_long(0)
    assert L.yolo_sumsq_fixed_slots(ns, 2, ctypes.byref(out)) == E_ARG and L.yolo_sumsq_fixed_slots(None, 2, ctypes.byref(out)) == E_ARG
    torch.cuda.synchronize()
    assert float(acc) == 0.0 and not bool(sc.any()), "a rejected call must not launch"


# ---- whole training steps, a fresh process per case ---------------------------------------------------------------------------------------------------

def _run(args, timeout=900, **extra_env):
    env = dict(os.environ)
    env.update(extra_env)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


@pytest.mark.parametrize("kind,batch", [("adam", 8), ("sgd", 8), ("adam", 64)])
def test_training_steps_repeat_bit_for_bit_in_and_across_processes(tmp_path, kind, batch):
    """EngineConfig.DETERMINISTIC: two models from one seed stay bit-equal in every parameter, gradient and optimizer-state tensor over three steps at
    448 x 448 (the child exits non-zero at the first difference), and two separate processes print the same hashes"""
    hashes = []
    for k in range(2):
        f = tmp_path / f"h{k}.txt"
        _run([CHILD, "repeat", str(f), kind, str(batch), "3"])
        hashes.append(f.read_text().split())
    assert len(hashes[0]) == 3 and hashes[0] == hashes[1], hashes


def test_deterministic_step_agrees_with_the_default_path(tmp_path):
    """one step with the switch off and one with it on: the forward is the same launches (equal loss); per-tensor gradients within the relative RMS
    tests/test_gpu_model.py allows between a gate-forced run and its reference (0.03)"""
    f = tmp_path / "cmp.pt"
    _run([CHILD, "compare", str(f), "8"])
    r = torch.load(f, weights_only=True)
    assert torch.equal(r["off"]["loss"], r["on"]["loss"]), (r["off"]["loss"], r["on"]["loss"])
    for n, g in r["off"].items():
        if n == "loss":
            continue
        rel = float(((r["on"][n] - g).pow(2).mean().sqrt() / g.pow(2).mean().sqrt().clamp_min(1e-30)))
        assert rel < 0.03, (n, rel)


def test_resume_continues_the_run_that_wrote_the_checkpoint(tmp_path):
    """train.py --deterministic --seed: 2 epochs at once vs 1 epoch + --resume for the second -- model and optimizer state bit-equal.  Nothing but
    `seed` / `deterministic` is added to the checkpoint: every epoch reseeds its generators from (seed, epoch)"""
    train = os.path.join(ROOT, "yolo-v1_amd", "train.py")
    common = ["--deterministic", "--seed", "11", "--synthetic", "16", "--batch-size", "8", "--num-workers", "0", "--backbone", "yolov1", "--device", "cuda"]
    a, b = tmp_path / "a", tmp_path / "b"
    _run([train, *common, "--epochs", "2", "--checkpoint-dir", str(a)])
    _run([train, *common, "--epochs", "1", "--checkpoint-dir", str(b)])
    _run([train, *common, "--epochs", "2", "--checkpoint-dir", str(b), "--resume", str(b / "yolo_latest.pth")])
    ca = torch.load(a / "yolo_latest.pth", map_location="cpu", weights_only=True)
    cb = torch.load(b / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert ca["epoch"] == cb["epoch"] == 2 and ca["seed"] == cb["seed"] == 11 and ca["deterministic"] is True
    for k, v in ca["model_state_dict"].items():
        assert torch.equal(v, cb["model_state_dict"][k]), k
    sa, sb = ca["optimizer_state_dict"]["state"], cb["optimizer_state_dict"]["state"]
    assert sa.keys() == sb.keys()
    for i in sa:
        for k, v in sa[i].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb[i][k])), (i, k)
