"""Weight EMA without a GPU: tests/ema_ref.py against torch.lerp, yolo.optim.ModelEMA on CPU tensors against the fp64 recurrence (five steps fed
back), the tau warm-up, integer buffers copied and float buffers averaged, the state_dict round trip, the skip flag, the ABI surface of ema.hip
with its host-side argument checks, and train.py --ema-decay / evaluate.py --use-ema on the CPU."""

import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import ema_ref as emr
import launch_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
WEIGHTS = (0.0, 1.0, 1e-4, 0.5)


def _small_model(seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.LeakyReLU(0.1), nn.Flatten(), nn.Linear(8 * 6 * 6, 37))


@pytest.mark.parametrize("w", WEIGHTS)
def test_reference_against_torch_lerp(w):
    """torch.lerp(e, p, w) in fp32 lies within the reference's bound of the fp64 value, for every weight the GPU test uses; the bound itself is
    a few unit roundoffs of the value"""
    gen = torch.Generator().manual_seed(3)
    e = torch.randn(1 << 16, generator=gen)
    p = e + torch.randn(1 << 16, generator=gen) * torch.tensor([1e-3, 1.0]).repeat(1 << 15)      # near the average, and far from it
    wf = emr._f32(w)
    ref, bnd = emr.ema_ref(e, p, wf)
    fails = []
    worst = lr.check_values(ref, bnd, torch.lerp(e, p, wf), "ema", fails, f"w={w}")
    print(f"w={w}: worst |err| / bound {worst:.3f}")
    assert not fails, fails
    assert float((bnd / ref.abs().clamp_min(1e-30)).median()) < 3 * 2.0 ** -24
    if w == 0.0:
        assert torch.equal(ref, e.double())
    if w == 1.0:
        assert torch.equal(ref, p.double())


def test_weight_is_formed_in_double_and_narrowed_once():
    assert emr.ema_weight(0.9999) == float(torch.tensor(1.0 - 0.9999, dtype=torch.float64).float())
    assert emr.ema_weight(0.9999) != float(torch.tensor(1.0) - torch.tensor(0.9999))      # an fp32 subtraction is another number
    assert emr.ema_weight(1.0) == 0.0 and emr.ema_weight(0.0) == 1.0


def test_model_ema_five_steps_against_the_fp64_recurrence():
    """ModelEMA on a small CPU model: every float tensor of the average within the propagated bound of the fp64 recurrence over the five
    snapshots; the copy is in eval mode, needs no gradients and shares no memory with the model"""
    from yolo import ModelEMA
    model = _small_model(0).train()
    ema = ModelEMA(model, decay=0.9)
    assert not ema.module.training and all(not p.requires_grad for p in ema.module.parameters())
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(ema.module.state_dict().values(), model.state_dict().values()))
    start = {k: v.clone() for k, v in ema.module.state_dict().items()}
    snaps = []
    gen = torch.Generator().manual_seed(1)
    for step in range(5):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=gen) * 0.05)
            model(torch.randn(4, 3, 8, 8, generator=gen))            # moves the BatchNorm running statistics and num_batches_tracked
        ema.update(model)
        snaps.append({k: v.clone() for k, v in model.state_dict().items()})
    assert ema.updates == 5
    fails = []
    w = emr.ema_weight(0.9)
    for k, v in ema.module.state_dict().items():
        if v.is_floating_point():
            ref, bnd = emr.ema_chain_ref(start[k], [s[k] for s in snaps], [w] * 5)
            lr.check_values(ref, bnd, v, k, fails, "five steps")
            assert not torch.equal(v, start[k]) and not torch.equal(v, snaps[-1][k])
        else:
            assert torch.equal(v, snaps[-1][k]) and int(v) == 5, "integer buffers are copied"
    assert not fails, "\n".join(fails)


def test_tau_warm_up_values():
    from yolo import ModelEMA
    model = _small_model(1)
    ema = ModelEMA(model, decay=0.9999, tau=2000.0)
    for n in (1, 2, 3):
        ema.update(model)
        assert ema.updates == n and ema.effective_decay() == 0.9999 * (1.0 - math.exp(-n / 2000.0))
    assert ema.effective_decay(10 ** 9) == 0.9999 and ModelEMA(model, decay=0.5).effective_decay(1) == 0.5
    # the first update of a warmed-up average follows the model almost entirely: w = 1 - 0.9999 * (1 - exp(-1 / 2000))
    m2 = _small_model(2)
    e2 = ModelEMA(m2, decay=0.9999, tau=2000.0)
    e0 = e2.module[4].weight.clone()
    with torch.no_grad():
        m2[4].weight.add_(1.0)
    e2.update(m2)
    w1 = emr.ema_weight(0.9999, 1, 2000.0)
    assert w1 > 0.9995
    ref, bnd = emr.ema_ref(e0, m2[4].weight.detach(), w1)
    fails = []
    lr.check_values(ref, bnd, e2.module[4].weight, "weight", fails, "tau")
    assert not fails, fails
    with pytest.raises(ValueError):
        ModelEMA(model, decay=1.5)


def test_state_dict_round_trip_and_name_check():
    from yolo import ModelEMA
    model = _small_model(3)
    ema = ModelEMA(model, decay=0.99, tau=10.0)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)
    ema.update()                                   # the model the constructor copied
    ema.update(model)
    sd = ema.state_dict()
    assert set(sd) == {"module", "updates", "decay", "tau"} and sd["updates"] == 2 and sd["decay"] == 0.99 and sd["tau"] == 10.0
    other = ModelEMA(_small_model(4), decay=0.5)
    other.load_state_dict(sd)
    assert other.updates == 2 and other.decay == 0.99 and other.tau == 10.0
    for (k, a), (_, b) in zip(other.module.state_dict().items(), ema.module.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(RuntimeError, match="state_dict entries"):
        ema.update(nn.Sequential(nn.Linear(3, 3)))


def test_a_skipped_step_is_no_ema_step():
    """the optimizer keeps the skip_if its last step consumed in last_skip; a non-zero flag there leaves the average and its counter alone"""
    from yolo import ModelEMA
    from yolo.optim import SGD
    model = nn.Linear(5, 3)
    opt = SGD(model.parameters(), lr=0.1)
    ema = ModelEMA(model, decay=0.5, optimizer=opt)
    before = ema.module.weight.clone()
    assert opt.last_skip is None
    for flag, moved in ((1.0, False), (0.0, True)):
        model.weight.grad, model.bias.grad = torch.ones(3, 5), torch.ones(3)
        opt.skip_if = torch.tensor([flag])
        opt.step()
        assert opt.skip_if is None and float(opt.last_skip) == flag
        with torch.no_grad():
            model.weight.add_(1.0)
        ema.update(model)
        assert (not torch.equal(ema.module.weight, before)) == moved and ema.updates == int(moved)
    model.weight.grad = torch.ones(3, 5)
    opt.step()
    assert opt.last_skip is None, "a step without a flag clears the record"


def test_every_ema_entry_is_declared_bound_and_called_by_the_gpu_test():
    """every YOLO_API entry ema.hip defines is in the header (which names what it replaces), in the binding, and named by tests/test_gpu_ema.py;
    the struct mirrors the C layout; the ABI version stays 2"""
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "ema.hip")) as f:
        src = f.read()
    entries = set(re.findall(r"YOLO_API int (yolo_\w+)", src))
    assert entries == {"yolo_ema_update", "yolo_ema_update_multi", "yolo_ema_update_multi_bg"}
    assert "fmaf(w, p - e, e)" in src[:src.index("#include")], "the header comment states the formula"
    with open(os.path.join(ROOT, "include", "yolo_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tests", "test_gpu_ema.py")) as f:
        called = set(re.findall(r"\.(yolo_\w+)\b", f.read()))
    for name in entries:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
    doc = header[:header.index("typedef struct yolo_ema_tensor")].rsplit("/*", 1)[1]
    assert "get_ema_multi_avg_fn" in doc and "_foreach_lerp_" in doc and "fmaf(w, p - e, e)" in doc
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header) and _hip.ABI_VERSION == 2
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(yolo_ema_tensor), ' \
            'offsetof(yolo_ema_tensor, ema), offsetof(yolo_ema_tensor, p), offsetof(yolo_ema_tensor, n));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src_c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src_c, "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src_c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = _hip.EmaTensor
    assert got == [ctypes.sizeof(T), T.ema.offset, T.p.offset, T.n.offset]


def test_ema_entries_refuse_bad_arguments_on_the_host():
    """the argument checks run before any HIP call, so they can be exercised without a device (as tests/test_abi.py does for yolo_decode); the
    pointers are never dereferenced"""
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    L = _hip.lib()
    E_ARG, E_UNS, T = _hip.E_ARG, _hip.E_UNSUPPORTED, _hip.EmaTensor
    e, p = 0x10000, 0x20000                        # 16-B aligned, 64 KB apart
    one = lambda **k: L.yolo_ema_update(k.get("e", e), k.get("p", p), k.get("n", 16), k.get("w", 0.1), None, None)
    assert one(e=None) == E_ARG and one(p=None) == E_ARG and one(n=-1) == E_ARG
    assert b"yolo_ema_update" in L.yolo_hip_last_error()
    for w in (-1e-6, 1.0001, float("nan"), float("inf")):
        assert one(w=w) == E_ARG, w
    assert one(e=e + 4) == E_UNS and one(p=p + 4) == E_UNS and b"16-B" in L.yolo_hip_last_error()
    assert one(p=e) == E_UNS and one(p=e + 48) == E_UNS and one(e=p + 48) == E_UNS and b"overlaps" in L.yolo_hip_last_error()
    ok = (T * 2)(T(e, p, 16), T(e + 4096, p + 4096, 16))
    for fn, extra in ((L.yolo_ema_update_multi, ()), (L.yolo_ema_update_multi_bg, (4,))):
        call = lambda tab, count, w=0.1: fn(tab, count, w, None, *extra, None)
        assert call(None, 2) == E_ARG and call(ok, -1) == E_ARG and call(ok, 2, w=2.0) == E_ARG and call(ok, 2, w=float("nan")) == E_ARG
        assert call((T * 2)(T(e, p, 16), T(None, p, 16)), 2) == E_ARG and b"tensor 1" in L.yolo_hip_last_error()
        assert call((T * 2)(T(e, p, 16), T(e, p, -2)), 2) == E_ARG
        assert call((T * 2)(T(e, p + 8, 16), T(e, p, 16)), 2) == E_UNS and b"tensor 0" in L.yolo_hip_last_error()
        assert call((T * 2)(T(e, p, 16), T(e, e + 16, 16)), 2) == E_UNS and b"tensor 1" in L.yolo_hip_last_error()
    for wg in (0, -1, 257):
        assert L.yolo_ema_update_multi_bg(ok, 2, 0.1, None, wg, None) == E_ARG
    many = (T * 49)(*[T(e + 64 * i, p + 64 * i, 16) for i in range(49)])
    assert L.yolo_ema_update_multi_bg(many, 49, 0.1, None, 4, None) == E_ARG


def _run(args, **kw):
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, **kw)


def test_train_and_evaluate_with_ema_on_the_cpu(tmp_path):
    """train.py --ema-decay on the CPU: two steps -> a checkpoint with ema_state_dict / ema_updates == 2 that loads with weights_only=True, raw and
    averaged weights differ, evaluate.py --use-ema accepts it; a checkpoint without the key is refused with the stated error; --resume restores it"""
    ck = tmp_path / "ck"
    base = [os.path.join(PKG, "train.py"), "--synthetic", "8", "--batch-size", "4", "--backbone", "yolov1", "--device", "cpu", "--num-workers", "0"]
    r = _run(base + ["--ema-decay", "0.9", "--epochs", "1", "--checkpoint-dir", str(ck)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in ("yolo_latest.pth", "yolo_best.pth"):
        d = torch.load(ck / name, map_location="cpu", weights_only=True)
        assert d["ema_updates"] == 2 and list(d["ema_state_dict"]) == list(d["model_state_dict"])
        differ = [k for k in d["model_state_dict"] if not torch.equal(d["model_state_dict"][k], d["ema_state_dict"][k])]
        assert len(differ) == len(d["model_state_dict"]), "two Adam steps move every tensor away from its average"
    out = tmp_path / "eval.txt"
    ev = [os.path.join(PKG, "evaluate.py"), "--synthetic", "4", "--device", "cpu", "--backbone", "yolov1", "--batch-size", "4", "--output", str(out)]
    r = _run(ev + ["--use-ema", "--checkpoint", str(ck / "yolo_latest.pth")])
    assert r.returncode == 0 and out.exists(), r.stdout[-2000:] + r.stderr[-3000:]
    # a second epoch resumed from the file: the average continues (4 updates), it does not restart from the raw weights
    r = _run(base + ["--ema-decay", "0.9", "--epochs", "2", "--checkpoint-dir", str(ck), "--resume", str(ck / "yolo_latest.pth")])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)["ema_updates"] == 4
    # without --ema-decay the file has the reference's keys only, and --use-ema says so
    plain = tmp_path / "plain"
    r = _run(base + ["--epochs", "1", "--checkpoint-dir", str(plain)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = torch.load(plain / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert not [k for k in d if k.startswith("ema")]
    r = _run(ev + ["--use-ema", "--checkpoint", str(plain / "yolo_latest.pth")])
    assert r.returncode != 0 and "has no 'ema_state_dict'" in r.stderr and "--ema-decay" in r.stderr, r.stderr[-2000:]
    sys.path.insert(0, PKG)
    try:
        import predict
        with pytest.raises(SystemExit, match="has no 'ema_state_dict'"):
            predict.load_model(str(plain / "yolo_latest.pth"), "cpu", backbone="yolov1", use_ema=True)
        m = predict.load_model(str(ck / "yolo_latest.pth"), "cpu", backbone="yolov1", use_ema=True)
        want = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)["ema_state_dict"]
        assert all(torch.equal(v, want[k]) for k, v in m.state_dict().items())
    finally:
        sys.path.remove(PKG)
