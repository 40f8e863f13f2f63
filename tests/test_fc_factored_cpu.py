"""CPU side of the factored Linear gradient (EngineConfig.FC_FACTORED): the switch, the C ABI's refusals (argument checks come before any HIP call), the
fp64 reference's own identity and the fp32 restatements the GPU bounds were sized with, the CLI refusals, and the gather step of the data-parallel path
on two gloo ranks."""

import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fc_factored_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
ENTRIES = {"yolo_fc_factored_grad", "yolo_fc_factored_sumsq_slots", "yolo_fc_factored_sumsq", "yolo_adam_step_factored", "yolo_sgd_step_factored"}


def _lib():
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    return _hip.lib()


def test_switch_exists_defaults_off_and_reads_the_environment():
    from yolo.config import CONFIG, SWITCHES, EngineConfig
    assert EngineConfig().FC_FACTORED is False and CONFIG.FC_FACTORED is False and {"FC_FACTORED", "FC_FACTORED_MIN"} <= SWITCHES
    assert EngineConfig().FC_FACTORED_MIN == 1 << 26 == EngineConfig().FC_NORM_IN_WGRAD
    code = f"import sys; sys.path.insert(0, {PKG!r}); from yolo.config import CONFIG; print(CONFIG.FC_FACTORED, CONFIG.FC_FACTORED_MIN)"
    env = dict(os.environ, YOLO_AMD_FC_FACTORED="1", YOLO_AMD_FC_FACTORED_MIN="4096")
    assert subprocess.check_output([sys.executable, "-c", code], env=env, text=True).split() == ["True", "4096"]


def test_every_new_entry_is_declared_bound_and_called_by_the_gpu_test():
    from yolo import _hip
    found = set(re.findall(r"YOLO_API int (yolo_\w+)", open(os.path.join(PKG, "csrc", "fc_factored.hip")).read()))
    assert found == ENTRIES
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    called = set(re.findall(r"\.(yolo_\w+)\b", open(os.path.join(ROOT, "tests", "test_gpu_fc_factored.py")).read()))
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
    define = lambda name: int(re.search(rf"^#define {name} (\d+)$", header, flags=re.M).group(1))
    assert _hip.FC_MAX_ROWS == define("YOLO_FC_MAX_ROWS") >= 512 and _hip.FC_GRAM_CHAIN == define("YOLO_FC_GRAM_CHAIN")
    assert define("YOLO_HIP_ABI_VERSION") == 2


def test_descriptor_layout_matches_the_header(tmp_path):
    from yolo import _hip
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(yolo_fc_factors), '
                   'offsetof(yolo_fc_factors, rows), offsetof(yolo_fc_factors, scale));return 0;}\n')
    exe = tmp_path / "p"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(_hip.FcFactors), _hip.FcFactors.rows.offset, _hip.FcFactors.scale.offset]


def test_refusals_come_before_any_hip_call():
    """the argument checks of every entry, on host memory and without a GPU: a refused call returns its code and names itself"""
    from test_gpu_fc_factored import E_ARG, E_UNSUPPORTED, refusal_descs, refused_calls
    L = _lib()
    O, I = 136, 200
    host = (ctypes.c_float * (3 * O * I + 64))()
    fac = (ctypes.c_uint16 * (64 * 256 + 64))()
    scratch = (ctypes.c_double * 16)()
    acc = (ctypes.c_double * 1)(3.25)
    align = lambda a: (ctypes.addressof(a) + 63) // 64 * 64
    fails = []
    for name, d, code in refusal_descs(align(fac), align(fac)):
        for entry, rc in refused_calls(L, d, align(host), ctypes.addressof(scratch), ctypes.addressof(acc), None):
            msg = L.yolo_hip_last_error().decode()
            if rc != code:
                fails.append(f"{name}: {entry} returned {rc}, expected {code}")
    assert not fails, "\n".join(fails)
    # each message names its entry
    from yolo._hip import FcFactors
    bad = FcFactors(align(fac), align(fac), 64, O, 196, 160, 200, 1.0)
    c = ctypes.c_void_p
    assert L.yolo_fc_factored_grad(ctypes.byref(bad), c(align(host)), None) == E_UNSUPPORTED and b"yolo_fc_factored_grad" in L.yolo_hip_last_error()
    assert L.yolo_fc_factored_sumsq(ctypes.byref(bad), c(ctypes.addressof(scratch)), 16, c(ctypes.addressof(acc)), None) == E_UNSUPPORTED
    assert b"yolo_fc_factored_sumsq" in L.yolo_hip_last_error()
    assert L.yolo_adam_step_factored(ctypes.byref(bad), c(align(host)), c(align(host)), c(align(host)), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 10.0, None, 0,
                                     None) == E_UNSUPPORTED and b"yolo_adam_step_factored" in L.yolo_hip_last_error()
    assert L.yolo_sgd_step_factored(ctypes.byref(bad), c(align(host)), c(align(host)), None, 1e-3, 0.9, 0.0, 0.0, 0, 1, None, 10.0, None, 0,
                                    None) == E_UNSUPPORTED and b"yolo_sgd_step_factored" in L.yolo_hip_last_error()
    # a scratch one slot short: refused with the size it needs, nothing written
    good = FcFactors(align(fac), align(fac), 64, O, I, 160, 200, 1.0)
    need = ctypes.c_long(0)
    assert L.yolo_fc_factored_sumsq_slots(ctypes.byref(good), ctypes.byref(need)) == 0 and need.value > 16
    assert L.yolo_fc_factored_sumsq(ctypes.byref(good), c(ctypes.addressof(scratch)), need.value - 1, c(ctypes.addressof(acc)), None) == E_ARG
    assert str(need.value).encode() in L.yolo_hip_last_error() and acc[0] == 3.25 and not any(scratch)
    # the SGD entry keeps torch.optim.SGD's constructor checks
    assert L.yolo_sgd_step_factored(ctypes.byref(good), c(align(host)), c(align(host)), None, 1e-3, 0.0, 0.0, 0.0, 1, 1, None, 10.0, None, 0, None) == E_ARG


@pytest.mark.parametrize("rows,O,I", fr.SHAPES)
def test_reference_identity_and_restatements(rows, O, I):
    """sum G64^2 == scale^2 sum (dy dy^T) o (x x^T) in fp64; a sequential fp32 restatement of G stays at <= 0.44 of the element bound for rows >= 5
    (measured: 0.44 at 5 rows, 0.03 at 64, 0.02 at 80 and 128; the single rounding of rows = 1 with scale 1/3 reaches 0.82 of its one-rounding bound)
    and a chunked fp32 restatement of the Gram form (c = 256) stays below 0.003 of its bound: the references are well inside what the GPU tests assert"""
    dy, x = fr.factors(rows, O, I, rows * 7 + O)
    for scale in fr.SCALES:
        G64, Gabs = fr.grad_ref(dy, x, O, I, scale)
        ref, bnd = fr.sumsq_ref(dy, x, O, I, scale, 256)
        direct = float((G64 ** 2).sum())
        assert abs(direct - ref) <= 1e-12 * abs(ref)
        g32 = fr.grad_fp32_sequential(dy, x, O, I, scale).double()
        b = fr.grad_bound(Gabs, rows, scale)
        err = (g32 - G64).abs()
        if rows == 1 and fr.scale_is_pow2(scale):
            assert float(err.max()) == 0.0 and float(b.max()) == 0.0            # one exact product, an exact scale: bit equality
        else:
            assert float((err / b).max()) <= (0.5 if rows > 1 else 1.0)
        s32 = fr.sumsq_fp32_chunked(dy, x, O, I, scale, 256)
        assert abs(s32 - ref) <= 0.02 * bnd


@pytest.mark.parametrize("script", ["train.py", "pretrain.py"])
@pytest.mark.parametrize("extra,names", [(["--optimizer", "lars"], ("--factored-fc", "--optimizer lars")),
                                         (["--accum-steps", "2"], ("--factored-fc", "--accum-steps")),
                                         (["--device", "cpu"], ("--factored-fc", "--device cpu"))])
def test_cli_refusals(script, extra, names):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--factored-fc", "--synthetic", "8"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, r.stderr[-2000:]
    assert all(n in r.stderr for n in names), r.stderr[-2000:]


def test_optimizers_refuse_the_switch_on_cpu(monkeypatch):
    import torch.nn as nn
    from yolo.config import CONFIG
    from yolo.optim import LARS, Adam, GradAccumulator
    monkeypatch.setattr(CONFIG, "FC_FACTORED", True)
    m = nn.Linear(8, 4)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match=r"FC_FACTORED.*CPU parameters"):
        Adam(m.parameters(), lr=1e-3).step()
    with pytest.raises(RuntimeError, match=r"FC_FACTORED.*LARS"):
        LARS(m.parameters(), lr=1e-3).step()
    with pytest.raises(RuntimeError, match=r"FC_FACTORED.*GradAccumulator"):
        GradAccumulator(m, 2)
    monkeypatch.setattr(CONFIG, "FC_FACTORED", False)
    Adam(m.parameters(), lr=1e-3).step()
    GradAccumulator(m, 2)


def _gather_worker(rank, world, port, rows, q):
    for p in (ROOT, os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from yolo.executor import FcFactors
    from yolo.parallel import gather_fc_factors
    O, I = 40, 72
    dy, x = fr.factors(rows[rank], O, I, 100 + rank, pad_value=0.0)
    try:
        rec = gather_fc_factors(FcFactors(dy, x, rows[rank], 1.0))
        q.put((rank, rec.rows, rec.scale, rec.dy.float().numpy(), rec.x.float().numpy(), dy.float().numpy(), x.float().numpy()))
    except RuntimeError as e:
        q.put((rank, str(e)))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(rows, port_base):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = port_base + os.getpid() % 2000
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, rows, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def test_gather_step_two_ranks_gloo():
    """rank order, scale = 1 / 2, and G(gathered) == the mean of the ranks' dense gradients, in fp64"""
    r0, r1 = _two_ranks((4, 4), 37500)
    O, I = 40, 72
    for r in (r0, r1):
        assert r[1] == 8 and r[2] == 0.5
        assert (r[3][:4] == r0[5]).all() and (r[3][4:] == r1[5]).all() and (r[4][:4] == r0[6]).all() and (r[4][4:] == r1[6]).all()      # rank order
    assert (r0[3] == r1[3]).all() and (r0[4] == r1[4]).all()
    t = lambda a: torch.from_numpy(a)
    G, _ = fr.grad_ref(t(r0[3]), t(r0[4]), O, I, r0[2])
    dense = 0.5 * (fr.grad_ref(t(r0[5]), t(r0[6]), O, I, 1.0)[0] + fr.grad_ref(t(r1[5]), t(r1[6]), O, I, 1.0)[0])
    assert float((G - dense).abs().max()) <= 1e-13 * float(dense.abs().max())


def test_gather_step_refuses_unequal_rows():
    r0, r1 = _two_ranks((4, 3), 39500)
    for r in (r0, r1):
        assert len(r) == 2 and "equal shards" in r[1] and "FC_FACTORED" in r[1], r
