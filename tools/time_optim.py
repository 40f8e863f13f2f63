#!/usr/bin/env python3
"""micro-benchmark: yolo_adam_step_multi against yolo_sgd_step_multi over the YOLOv1 model's real parameter table (52 tensors, the Linear behind
nn.Flatten 205 M of the 271.7 M elements), clip coefficient read from the device, bf16 shadow on the Linear weights as in training.

    python tools/time_optim.py [--rounds 5] [--reps 10] [--json out/time_optim.json]

ms per pass and achieved TB/s = the bytes the pass must move / time: per element 28 B for Adam (read p, g, m, v; write p, m, v), 20 B for SGD with
momentum (read p, g, buf; write p, buf), 16 B on SGD's first step (buf is only written), + 2 B where a shadow is written.  The table (6-8 GB)
is far larger than the 256-MB Infinity Cache, so every pass streams from HBM.  Device events around `reps` back-to-back passes, `rounds` such
windows per kernel, the kernels alternating round by round so that clock or neighbour drift hits both alike; a warm-up pass of each first.
The median window is reported, with the spread of the windows.  Needs the GPU: there is no fallback.

adam_fc1_dense / adam_fc1_factored: the Linear(50176, 4096) behind nn.Flatten alone -- yolo_adam_step_multi on that one tensor (30 B per element with the
shadow) against yolo_adam_step_factored, which rebuilds the gradient from its two batch factors (--fc-rows rows, default 64) on the matrix cores and
moves 26 B per element + the factors; adam_fc1_factored_bg is the same launch on optim.BG_CUS persistent workgroups.  sgd_fc1_* likewise (22 / 18 B)."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))
import torch
from yolo import YOLOv1
from yolo._hip import AdamTensor, FcFactors, SgdTensor, check, lib, ptr, stream

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--json", default=None, help="also write the result there")
ap.add_argument("--fc-rows", type=int, default=64, help="rows of the two factors of the factored launches (the batch; x ranks under data parallelism)")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_optim.py measures on the GPU"
dev = torch.device("cuda")
torch.manual_seed(0)

model = YOLOv1().to(dev)
params = [p.detach() for p in model.parameters()]
assert len(params) == 52
elems = sum(p.numel() for p in params)
g = [torch.randn_like(p) * 1e-2 for p in params]
m, v, buf = ([torch.zeros_like(p) for p in params] for _ in range(3))
shadow = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) if p.dim() == 2 else None for p in params]      # the Linear weights
sh_elems = sum(p.numel() for p, s in zip(params, shadow) if s is not None)
norm = torch.tensor([sum(float(x.double().pow(2).sum()) for x in g)], dtype=torch.float64, device=dev)          # |g| ~ 165: the clip is active
adam_tab = (AdamTensor * 52)(*[AdamTensor(p.data_ptr(), x.data_ptr(), mm.data_ptr(), vv.data_ptr(), s.data_ptr() if s is not None else None, p.numel())
                               for p, x, mm, vv, s in zip(params, g, m, v, shadow)])
sgd_tab = (SgdTensor * 52)(*[SgdTensor(p.data_ptr(), x.data_ptr(), b.data_ptr(), s.data_ptr() if s is not None else None, p.numel())
                             for p, x, b, s in zip(params, g, buf, shadow)])
step = [0]


def adam():
    step[0] += 1
    check(lib().yolo_adam_step_multi(adam_tab, 52, 1e-4, 0.9, 0.999, 1e-8, 5e-4, step[0], ptr(norm), 10.0, None, stream()), "yolo_adam_step_multi")


def sgd(first=0):
    check(lib().yolo_sgd_step_multi(sgd_tab, 52, 1e-4, 0.9, 0.0, 5e-4, 0, first, ptr(norm), 10.0, None, stream()), "yolo_sgd_step_multi")


# the Linear behind nn.Flatten alone: the dense launch on its one tensor against the factored launch (EngineConfig.FC_FACTORED)
fc1 = max(range(52), key=lambda i: params[i].numel())
O, I = params[fc1].shape
fc_n = O * I
ldg = (O + 31) // 32 * 32
fdy = (torch.randn((a.fc_rows, ldg), device=dev) * 1e-2).to(torch.bfloat16)
fx = torch.randn((a.fc_rows, I), device=dev).to(torch.bfloat16)
fac = FcFactors(fdy.data_ptr(), fx.data_ptr(), a.fc_rows, O, I, ldg, I, 1.0)
fac_bytes = 2 * (fdy.numel() + fx.numel())
adam_fc1 = (AdamTensor * 1)(adam_tab[fc1])
sgd_fc1 = (SgdTensor * 1)(sgd_tab[fc1])
fstep = [0]


def adam_fc1_dense():
    fstep[0] += 1
    check(lib().yolo_adam_step_multi(adam_fc1, 1, 1e-4, 0.9, 0.999, 1e-8, 5e-4, fstep[0], ptr(norm), 10.0, None, stream()), "yolo_adam_step_multi")


def adam_fc1_factored(wg=0):
    fstep[0] += 1
    check(lib().yolo_adam_step_factored(ctypes.byref(fac), ptr(params[fc1]), ptr(m[fc1]), ptr(v[fc1]), ptr(shadow[fc1]), 1e-4, 0.9, 0.999, 1e-8, 5e-4, fstep[0],
                                        ptr(norm), 10.0, None, wg, stream()), "yolo_adam_step_factored")


def sgd_fc1_dense():
    check(lib().yolo_sgd_step_multi(sgd_fc1, 1, 1e-4, 0.9, 0.0, 5e-4, 0, 0, ptr(norm), 10.0, None, stream()), "yolo_sgd_step_multi")


def sgd_fc1_factored():
    check(lib().yolo_sgd_step_factored(ctypes.byref(fac), ptr(params[fc1]), ptr(buf[fc1]), ptr(shadow[fc1]), 1e-4, 0.9, 0.0, 5e-4, 0, 0, ptr(norm), 10.0, None, 0,
                                       stream()), "yolo_sgd_step_factored")


def fc1_sumsq():
    check(lib().yolo_fc_factored_sumsq(ctypes.byref(fac), ptr(gram), gram.numel(), ptr(gram_acc), stream()), "yolo_fc_factored_sumsq")


need = ctypes.c_long(0)
check(lib().yolo_fc_factored_sumsq_slots(ctypes.byref(fac), ctypes.byref(need)), "yolo_fc_factored_sumsq_slots")
gram, gram_acc = torch.empty(need.value, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
from yolo.optim import BG_CUS

runs = {"adam_fc1_dense": (adam_fc1_dense, 30 * fc_n), "adam_fc1_factored": (adam_fc1_factored, 26 * fc_n + fac_bytes),
        "adam_fc1_factored_bg": (lambda: adam_fc1_factored(BG_CUS), 26 * fc_n + fac_bytes),
        "sgd_fc1_dense": (sgd_fc1_dense, 22 * fc_n), "sgd_fc1_factored": (sgd_fc1_factored, 18 * fc_n + fac_bytes),
        "fc1_factored_sumsq": (fc1_sumsq, fac_bytes),
        "adam": (adam, 28 * elems + 2 * sh_elems), "sgd": (sgd, 20 * elems + 2 * sh_elems), "sgd_first_step": (lambda: sgd(1), 16 * elems + 2 * sh_elems)}
for fn, _ in runs.values():
    fn()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(a.rounds):
    for k, (fn, _) in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / a.reps)
assert all(bool(torch.isfinite(p).all()) for p in params[-4:])
out = {"elements": elems, "shadow_elements": sh_elems, "rounds": a.rounds, "reps": a.reps}
for k, (_, byts) in runs.items():
    ms = statistics.median(times[k])
    out[k] = {"ms": round(ms, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "bytes": byts, "TBps": round(byts / ms / 1e9, 3)}
    print(f"{k:21s} {ms:7.3f} ms (windows {min(times[k]):.3f} .. {max(times[k]):.3f})  {byts / 1e9:6.3f} GB  {byts / ms / 1e9:5.2f} TB/s")
out["fc_rows"] = a.fc_rows
out["adam_fc1_factored_over_dense"] = round(out["adam_fc1_factored"]["ms"] / out["adam_fc1_dense"]["ms"], 4)
print(f"FC1 alone, rows {a.fc_rows}: factored / dense Adam time {out['adam_fc1_factored_over_dense']:.3f} (bytes {26 / 30:.3f})")
out["sgd_over_adam"] = round(out["sgd"]["ms"] / out["adam"]["ms"], 4)
print(f"sgd / adam time {out['sgd_over_adam']:.3f} (bytes {out['sgd']['bytes'] / out['adam']['bytes']:.3f})")
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f)
