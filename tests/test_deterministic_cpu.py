"""EngineConfig.DETERMINISTIC without a GPU: the switch, train.py's flags, the ResNet rejection, the new ABI entries, what the switch relies on in the
shipped plan table, and yolo_wgrad_slab_floats (host arithmetic only) over the YOLOv1 conv layers."""

import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import wgrad_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")


def test_switch_exists_defaults_off_and_reads_the_environment():
    from yolo.config import CONFIG, SWITCHES, EngineConfig
    assert EngineConfig().DETERMINISTIC is False and CONFIG.DETERMINISTIC is False and "DETERMINISTIC" in SWITCHES
    code = f"import sys; sys.path.insert(0, {PKG!r}); from yolo.config import CONFIG; print(CONFIG.DETERMINISTIC)"
    for val, want in (("1", "True"), ("0", "False")):
        out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, YOLO_AMD_DETERMINISTIC=val), text=True)
        assert out.strip() == want


def test_train_py_deterministic_seeded_epoch_on_the_cpu(tmp_path):
    args = [sys.executable, os.path.join(PKG, "train.py"), "--deterministic", "--seed", "3", "--synthetic", "8", "--batch-size", "4", "--epochs", "1",
            "--num-workers", "0", "--backbone", "yolov1", "--device", "cpu", "--checkpoint-dir", str(tmp_path)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(tmp_path / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert ck["seed"] == 3 and ck["deterministic"] is True and ck["epoch"] == 1
    assert {"model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "train_loss", "val_loss"} <= set(ck)      # the reference's keys


def test_resnet_trunk_with_batch_statistics_is_rejected():
    from yolo.models import BN_STATS_NOT_DETERMINISTIC
    assert "BatchNorm" in BN_STATS_NOT_DETERMINISTIC and "statistics" in BN_STATS_NOT_DETERMINISTIC
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--deterministic", "--backbone", "resnet50", "--device", "cpu", "--synthetic", "8"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "BatchNorm batch statistics" in r.stderr
    src = open(os.path.join(PKG, "yolo", "models.py")).read()
    assert "if self.training and CONFIG.DETERMINISTIC:\n                raise NotImplementedError(BN_STATS_NOT_DETERMINISTIC)" in src


def test_every_new_entry_is_declared_bound_and_called_by_the_gpu_test():
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "norm_fixed.hip")) as f:
        entries = set(re.findall(r"YOLO_API int (yolo_\w+)", f.read()))
    assert entries == {"yolo_sumsq_fixed_slots", "yolo_sumsq_f32_fixed", "yolo_sumsq_f32_multi_fixed"}
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    called = set(re.findall(r"\.(yolo_\w+)\b", open(os.path.join(ROOT, "tests", "test_gpu_deterministic.py")).read()))
    for name in entries:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
    doc = header[:header.index("int yolo_sumsq_fixed_slots(")].rsplit("/*", 1)[1]
    assert "yolo_sumsq_f32_multi" in doc and "atomicAdd" in doc, "the declaration cites what it replaces"
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header)


def test_no_shipped_plan_is_a_splitk_plan():
    """the switch turns a ("splitk", ..) plan into its ("slabs", ..) form; the shipped table holds none, so the forward is the default path's launches"""
    text = open(os.path.join(PKG, "yolo", "plans", "gfx950.json")).read()
    assert '"splitk"' not in text and text.count('"slabs"') > 100


# ---- yolo_wgrad_slab_floats ---------------------------------------------------------------------------------------------------------------------------

def _conv_layers():
    """(Cin, Cout, K, stride, Hout) of the 24 conv layers of YOLOv1 at 448 x 448, from the model itself (meta tensors: shapes only)"""
    from yolo import YOLOv1
    with torch.device("meta"):
        m = YOLOv1()
    out = []

    def hook(mod, inp, res):
        out.append((mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0], res.shape[2]))
    hs = [c.register_forward_hook(hook) for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
    y = m.backbone.features(torch.empty(1, 3, 448, 448, device="meta"))
    for h in m.head:
        if isinstance(h, torch.nn.Flatten):
            break
        y = h(y)
    for h in hs:
        h.remove()
    return out


def _schedule(P, Cout, Cin, K, variant=0, x_px_stride=None):
    """the two-segment schedule of yolo_wgrad (split = 0) restated -> (main_tiles, main_split, tail_tiles, tail_split): 128 x 128 tiles on 512
    workgroup slots for variants 0 / 1 / 4, 256 x 256 tiles (tile_taps taps each) on 256 slots for variants 5 / 6 (tests/wgrad_cases.py)"""
    tiles, slots = wc.wgrad_tiles(Cout, Cin, K * K, variant, x_px_stride)
    return wc.wgrad_schedule(P, tiles, slots)


def _some_tile_is_split(P, Cout, Cin, K):
    """does the main or the tail segment of the 128 x 128 kernels' schedule use more than one pixel range?"""
    main_tiles, main_split, tail_tiles, tail_split = _schedule(P, Cout, Cin, K)
    return (main_tiles > 0 and main_split > 1) or (tail_tiles > 0 and tail_split > 1)


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


def test_slab_floats_of_the_128_kernels_is_nonzero_exactly_when_a_tile_is_split():
    from yolo._hip import WgradDesc
    L = _lib()
    layers = _conv_layers()
    assert len(layers) == 24
    seen = set()
    for N in (1, 8, 64):
        for (Cin, Cout, K, stride, H) in layers[1:]:             # (the stem has its own kernel)
            Hp = H * stride + 2
            for variant in (0, 1, 4):
                for flat in (True, False):
                    if flat:
                        d = WgradDesc(N * Hp * Hp, Cout, Cin, Cout, Cin, K, K, K // 2, Hp * Cin, 0, 0, variant)
                    else:
                        d = WgradDesc(N * H * H, Cout, Cin, Cout, Cin, K, K, K // 2, Hp * Cin, 0, 0, variant, H, H, Hp * Hp, Hp * stride, stride, Hp + 1)
                    need = _need(L, d)
                    split = _some_tile_is_split(d.P, Cout, Cin, K)
                    assert (need > 0) == split, (N, Cin, Cout, K, stride, H, variant, flat, need)
                    assert need % 4 == 0
                    seen.add(split)
                    d.split = 1
                    assert _need(L, d) == 0
                    d.split = 3
                    per = -(-(-(-d.P // 3)) // 64) * 64                  # a uniform split's ranges are whole 64-pixel steps
                    assert (_need(L, d) > 0) == (-(-d.P // per) > 1)
    assert seen == {True, False}
    for variant in (2, 3):
        assert _need(L, WgradDesc(4096, 256, 128, 256, 128, 3, 3, 1, 66 * 128, 3, 0, variant)) == 0


# (N, H, Cout, Cin, split) -> floats for variants 5 and 6, recorded from the build of the parent commit: their slab mode sizes its scratch as before
RECORDED_56 = {(8, 56, 512, 256, 0): 16515072, (8, 56, 512, 256, 3): 3538944, (8, 14, 1024, 1024, 0): 9437184, (8, 14, 1024, 1024, 3): 28311552,
               (8, 112, 192, 64, 0): 16711680, (8, 112, 192, 64, 3): 589824, (64, 56, 512, 256, 0): 16515072, (64, 56, 512, 256, 3): 3538944,
               (64, 14, 1024, 1024, 0): 33554432, (64, 14, 1024, 1024, 3): 28311552, (64, 112, 192, 64, 0): 16711680, (64, 112, 192, 64, 3): 589824,
               (1, 28, 1024, 512, 0): 14155776, (64, 28, 1024, 512, 0): 33554432, (64, 7, 1024, 1024, 3): 28311552}


def test_slab_floats_of_the_pipelined_kernels_is_unchanged():
    from yolo._hip import WgradDesc
    L = _lib()
    for (N, H, Cout, Cin, split), want in RECORDED_56.items():
        Hp = H + 2
        for variant in (5, 6):
            d = WgradDesc(N * H * H, Cout, Cin, Cout, Cin, 3, 3, 1, Hp * Cin, split, 0, variant, H, H, Hp * Hp, Hp, 1, Hp + 1)
            assert _need(L, d) == want and want % (256 * 256) == 0, (N, H, Cout, Cin, variant, split)


def test_gpu_cases_of_the_slab_test_all_split_a_tile():
    """the cases of tests/test_gpu_deterministic.py::test_wgrad_128_slab_mode, sized here without a GPU: every one must exercise the slab path"""
    from yolo._hip import WgradDesc
    L = _lib()
    for geo in ("flat", "interior", "stride2"):
        N, H, W = (8, 14, 18) if geo == "stride2" else (4, 13, 17)
        Hp, Wp = H + 2, W + 2
        for Cin, K in [(64, 3), (128, 1), (192, 3), (512, 1), (128, 3)]:
            for split in (0, 3):
                for variant in (1, 4):
                    if geo == "flat":
                        d = WgradDesc(N * Hp * Wp, 256, Cin, 256, Cin, K, K, K // 2, Wp * Cin, split, 0, variant)
                    elif geo == "interior":
                        d = WgradDesc(N * H * W, 256, Cin, 256, Cin, K, K, K // 2, Wp * Cin, split, 0, variant, W, H, Hp * Wp, Wp, 1, Wp + 1)
                    else:
                        d = WgradDesc(N * (H // 2) * (W // 2), 256, Cin, 256, Cin, K, K, K // 2, Wp * Cin, split, 0, variant, W // 2, H // 2, Hp * Wp, 2 * Wp, 2,
                                      Wp + 1)
                    assert _need(L, d) > 0, (geo, Cin, K, split, variant)
