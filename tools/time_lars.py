#!/usr/bin/env python3
"""micro-benchmark: the LARS passes of csrc/lars.hip against yolo.optim.SGD's over the YOLOv1 model's real parameter table (52 tensors, the Linear
behind nn.Flatten 205 M of the 271.7 M elements), clip coefficient read from the device, bf16 shadow on the Linear weights as in training.

    python tools/time_lars.py [--rounds 5] [--reps 10] [--train-steps 20] [--json out/time_lars.json]

Foreground, all 52 tensors: the norms pass (yolo_lars_norms_multi: read p and g, 8 B per element), the LARS step (yolo_lars_step_multi: 20 B per
element + 2 B where a shadow is written), SGD's global-norm pass (yolo_sumsq_f32_multi: read g, 4 B) and SGD's step (yolo_sgd_step_multi: 20 B +
2 B); "sgd" and "lars" are the two launches of each back to back, what one optimizer step enqueues.  Background, the four tensors of the Linear
layers on BG_CUS persistent workgroups (yolo_sgd_step_multi_bg, yolo_lars_step_multi_bg), alone on the device.  The tables are far larger than the
256-MB Infinity Cache, so every pass streams from HBM.  Device events around `reps` back-to-back passes, `rounds` such windows per case, the cases
alternating round by round so that clock or neighbour drift hits all alike; a warm-up pass of each first.  The median window is reported, with the
spread of the windows.

--train-steps K > 0: also the batch-64 YOLOv1 training step (forward, loss, backward, optimizer with the background pass attached) with
yolo.optim.SGD against yolo.optim.LARS on one model in one process, three alternating windows of K steps each.  Needs the GPU: there is no fallback."""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
from yolo import YOLOv1
from yolo._hip import LarsTensor, SgdTensor, check, lib, ptr, stream
from yolo.optim import BG_CUS

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--train-steps", type=int, default=0, help="also time the batch-64 training step, sgd against lars, in windows of this many steps")
ap.add_argument("--json", default=None, help="also write the result there")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_lars.py measures on the GPU"
dev = torch.device("cuda")
torch.manual_seed(0)

model = YOLOv1().to(dev)
params = [p.detach() for p in model.parameters()]
assert len(params) == 52
elems = sum(p.numel() for p in params)
g = [torch.randn_like(p) * 1e-2 for p in params]
buf = [torch.zeros_like(p) for p in params]
shadow = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) if p.dim() == 2 else None for p in params]      # the Linear weights
sh_elems = sum(p.numel() for p, s in zip(params, shadow) if s is not None)
fc = [i for i, p in enumerate(params) if p.dim() == 2] + [i + 1 for i, p in enumerate(params) if p.dim() == 2]     # the Linear weights and their biases
fc_elems = sum(params[i].numel() for i in fc)
acc = torch.zeros(1, dtype=torch.float64, device=dev)
total = torch.zeros(1, dtype=torch.float64, device=dev)
norms = torch.zeros(2 * 52, dtype=torch.float64, device=dev)
n_arr = (ctypes.c_long * 52)(*[p.numel() for p in params])
p_arr = (ctypes.c_void_p * 52)(*[p.data_ptr() for p in params])
g_arr = (ctypes.c_void_p * 52)(*[x.data_ptr() for x in g])
slots = ctypes.c_long(0)
check(lib().yolo_lars_norm_slots(n_arr, 52, ctypes.byref(slots)), "yolo_lars_norm_slots")
scratch = torch.empty(max(slots.value, 1), dtype=torch.float64, device=dev)


def tables(idx):
    s = (SgdTensor * len(idx))(*[SgdTensor(params[i].data_ptr(), g[i].data_ptr(), buf[i].data_ptr(), shadow[i].data_ptr() if shadow[i] is not None else None,
                                           params[i].numel()) for i in idx])
    l = (LarsTensor * len(idx))(*[LarsTensor(params[i].data_ptr(), g[i].data_ptr(), buf[i].data_ptr(), shadow[i].data_ptr() if shadow[i] is not None else None,
                                             norms.data_ptr() + 16 * i, params[i].numel(), int(params[i].dim() > 1)) for i in idx])
    return s, l


sgd_all, lars_all = tables(range(52))
sgd_fc, lars_fc = tables(fc)
H_SGD = (1e-4, 0.9, 0.0, 5e-4, 0, 0)
H_LARS = (1e-4, 0.9, 5e-4, 1e-3, 1e-8, 0)


def sumsq():
    acc.zero_()
    check(lib().yolo_sumsq_f32_multi(g_arr, n_arr, 52, ptr(acc), stream()), "yolo_sumsq_f32_multi")


def sgd_step():
    check(lib().yolo_sgd_step_multi(sgd_all, 52, *H_SGD, ptr(acc), 10.0, None, stream()), "yolo_sgd_step_multi")


def lars_norms():
    check(lib().yolo_lars_norms_multi(p_arr, g_arr, n_arr, 52, ptr(scratch), scratch.numel(), ptr(norms), ptr(total), stream()), "yolo_lars_norms_multi")


def lars_step():
    check(lib().yolo_lars_step_multi(lars_all, 52, *H_LARS, ptr(total), 10.0, None, stream()), "yolo_lars_step_multi")


def sgd_bg():
    check(lib().yolo_sgd_step_multi_bg(sgd_fc, len(fc), *H_SGD, ptr(acc), 10.0, None, BG_CUS, stream()), "yolo_sgd_step_multi_bg")


def lars_bg():
    check(lib().yolo_lars_step_multi_bg(lars_fc, len(fc), *H_LARS, ptr(total), 10.0, None, BG_CUS, stream()), "yolo_lars_step_multi_bg")


runs = {"sgd_norm": (sumsq, 4 * elems), "sgd_step": (sgd_step, 20 * elems + 2 * sh_elems), "sgd": (lambda: (sumsq(), sgd_step()), 24 * elems + 2 * sh_elems),
        "lars_norms": (lars_norms, 8 * elems), "lars_step": (lars_step, 20 * elems + 2 * sh_elems),
        "lars": (lambda: (lars_norms(), lars_step()), 28 * elems + 2 * sh_elems),
        "sgd_fc_bg": (sgd_bg, 20 * fc_elems + 2 * sh_elems), "lars_fc_bg": (lars_bg, 20 * fc_elems + 2 * sh_elems)}
sumsq()
lars_norms()
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
out = {"elements": elems, "shadow_elements": sh_elems, "fc_elements": fc_elems, "bg_workgroups": BG_CUS, "rounds": a.rounds, "reps": a.reps}
for k, (_, byts) in runs.items():
    ms = statistics.median(times[k])
    out[k] = {"ms": round(ms, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "bytes": byts, "TBps": round(byts / ms / 1e9, 3)}
    print(f"{k:12s} {ms:7.3f} ms (windows {min(times[k]):.3f} .. {max(times[k]):.3f})  {byts / 1e9:6.3f} GB  {byts / ms / 1e9:5.2f} TB/s")
out["lars_over_sgd"] = round(out["lars"]["ms"] / out["sgd"]["ms"], 4)
print(f"lars / sgd time {out['lars_over_sgd']:.3f} (bytes {out['lars']['bytes'] / out['sgd']['bytes']:.3f})")

if a.train_steps > 0:
    import synth
    from yolo import YOLOLoss
    from yolo.optim import LARS, SGD, lars_param_groups
    del g, buf, shadow, sgd_all, lars_all, sgd_fc, lars_fc
    torch.cuda.empty_cache()
    model.train()
    x = torch.randn(64, 3, 448, 448, device=dev)
    tgt = torch.from_numpy(synth.synth_targets(64, seed=1)).to(dev)
    crit = YOLOLoss()
    opts = {"sgd": SGD(model.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0),
            "lars": LARS(lars_param_groups(model, 5e-4), lr=1e-4, momentum=0.9, max_grad_norm=10.0)}
    # one second stream for both: a process has few hardware queues, and a stream beyond them shares a queue with another one, in order with it
    # (with a stream each, the optimizer created second ran its background pass in line with the forward: 13.96 ms per step instead of 11.06)
    opts["lars"]._side = opts["sgd"]._side_stream()
    for o in opts.values():
        o.attach_plan(model.hip_plan(), overlap=True)

    def train_step(opt):
        opt.zero_grad(set_to_none=True)
        loss, _ = crit(model(x), tgt)
        loss.backward()
        opt.step()

    res = {k: [] for k in opts}
    for k, o in opts.items():
        for _ in range(3):
            train_step(o)
        o.synchronize()
    for rnd in range(3):
        for k, o in opts.items():
            for _ in range(2):
                train_step(o)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.train_steps):
                train_step(o)
            o.synchronize()
            torch.cuda.synchronize()
            res[k].append(1e3 * (time.perf_counter() - t0) / a.train_steps)
    for k, v in res.items():
        out["train_step_" + k] = {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
        print(f"batch-64 step, {k:4s}: " + " ".join(f"{t:.3f}" for t in v) + f"  ms/step (median {statistics.median(v):.3f})")
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f)
