#!/usr/bin/env python3
"""micro-benchmark of gradient accumulation (csrc/accum.hip, yolo.optim.GradAccumulator), in two parts.

    python tools/time_accum.py [--rounds 5] [--reps 10] [--groups 8] [--json out/time_accum.json]

1. The pass alone, on the YOLOv1 gradient arena (271.7 M elements, one yolo_grad_accum call as GradAccumulator issues it): the three uses of a
   K-step group -- store (acc = alpha g, 8 B per element), accumulate (acc = fmaf(alpha, g, acc), 12 B) and fold (g = fmaf(alpha, g, acc), 12 B) --
   next to yolo_ema_update_multi on the same element count in the same run (12 B per element as well: the yardstick of an elementwise
   two-reads-one-write pass).  The EMA pass is in the rotation TWICE, so that the table shows what a repeated measurement of one kernel spreads
   by; the 12-byte uses should reach its bytes/s within that spread.  Device events around `reps` back-to-back passes, `rounds` windows per
   kernel, the kernels alternating round by round; the median window is reported with the spread.  The buffers (1.09 GB each) are far larger
   than the 256-MB Infinity Cache, so every pass streams from HBM.
2. The training step at batch 64 (the step sequence of training.train_epoch: forward, loss, backward, accumulate or fold, and per group the fused
   clip + Adam), K = 1 against K = 4 as train.py sets them up (the Linear layers' update on the second stream at K = 1, in the foreground at
   K = 4), and for the record K = 4 with the background update, K = 1 with a gradient arena and the background update, and forward + backward with
   three of four steps left out, in ms per image: host clock around `groups` groups of 4 batches behind a warm-up, the window ending in a device
   synchronise; the setups alternate over `rounds` windows.

Needs the GPU: there is no fallback."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
from yolo import GradAccumulator, YOLOLoss, YOLOv1
from yolo._hip import EmaTensor, check, lib, ptr, stream
from yolo.optim import Adam, accum_alpha

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--groups", type=int, default=8)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=None, help="also write the result there")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_accum.py measures on the GPU"
dev = torch.device("cuda")
torch.manual_seed(0)
out = {"rounds": a.rounds, "reps": a.reps, "groups": a.groups, "batch": a.batch}


def median_of(times):
    return {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}


# ---- 1. the pass alone -------------------------------------------------------------------------------------------------------------------------
model = YOLOv1().to(dev)
n = model.hip_plan().attach_grad_arena(dev).numel()
del model
g = torch.randn(n, device=dev) * 1e-2
acc = torch.zeros(n, device=dev)
e = torch.zeros(n, device=dev)
ALPHA = accum_alpha(4)
ema_tab = (EmaTensor * 1)(EmaTensor(e.data_ptr(), g.data_ptr(), n))


def accum(dst, x, y):
    return lambda: check(lib().yolo_grad_accum(ptr(dst), ptr(x), ptr(y), n, ALPHA, None, stream()), "yolo_grad_accum")


def ema():
    check(lib().yolo_ema_update_multi(ema_tab, 1, 1e-4, None, stream()), "yolo_ema_update_multi")


runs = {
    "ema_multi": (ema, 12 * n),
    "accum_store": (accum(acc, g, None), 8 * n),
    "accum_accumulate": (accum(acc, g, acc), 12 * n),
    "accum_fold": (accum(g, g, acc), 12 * n),          # (g shrinks towards acc / (1 - alpha) pass by pass: the values do not matter to the rate)
    "ema_multi_again": (ema, 12 * n),
}
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
out["elements"] = n
for k, r in median_of(times).items():
    byts = runs[k][1]
    out[k] = dict(r, bytes=byts, GBps=round(byts / r["ms"] / 1e6, 1), GBps_min=round(byts / r["ms_max"] / 1e6, 1), GBps_max=round(byts / r["ms_min"] / 1e6, 1))
    print(f"{k:17s} {r['ms']:7.3f} ms (windows {r['ms_min']:.3f} .. {r['ms_max']:.3f})  {byts / 1e9:6.3f} GB  {out[k]['GBps']:7.1f} GB/s", flush=True)
ema_rates = [out[k][f] for k in ("ema_multi", "ema_multi_again") for f in ("GBps_min", "GBps_max")]
out["ema_GBps_spread"] = [min(ema_rates), max(ema_rates)]
print(f"the EMA pass, measured twice: {min(ema_rates):.1f} .. {max(ema_rates):.1f} GB/s over all windows", flush=True)
del g, acc, e, ema_tab
torch.cuda.empty_cache()

# ---- 2. inside the training step ---------------------------------------------------------------------------------------------------------------
import synth

x = torch.from_numpy(synth.synth_images(a.batch, 0)).to(dev)
t = torch.from_numpy(synth.synth_targets(a.batch, 1)).to(dev)
crit = YOLOLoss()
setups = {}
for name, K, overlap, arena, every in (("K1", 1, True, False, 1), ("K4", 4, False, True, 1), ("K4_background", 4, True, True, 1),
                                       ("K1_arena_background", 1, True, True, 1), ("no_accum_step_every_4th", 1, True, False, 4)):
    # K1, K4: train.py's choices -- the Linear layers' update in the background at K = 1, in the foreground under accumulation.  The others are
    # for the record: the background update under accumulation; the background update beside a gradient arena WITHOUT an accumulator; and what
    # forward + backward cost when three of four optimizer steps are simply left out (no accumulation: not a training recipe)
    torch.manual_seed(0)
    m = YOLOv1().to(dev).train()
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(m.hip_plan(), overlap=overlap)
    if arena and K == 1:
        m.hip_plan().attach_grad_arena(dev)
    setups[name] = (m, opt, GradAccumulator(m, K) if K > 1 else None, every)


def batches(name, count):
    m, opt, ga, every = setups[name]
    for i in range(count):
        opt.zero_grad(set_to_none=True)
        if ga is not None:
            ga.before_backward()
        loss, parts = crit(m(x), t)
        loss.backward()
        if ga is None:
            if i % every != every - 1:
                continue
            opt.skip_if = parts.device_flag
        elif ga.after_backward(parts.device_flag):
            opt.skip_if = ga.skip_if
        else:
            continue
        opt.step()


for K in setups:
    batches(K, 8)
torch.cuda.synchronize()
times = {K: [] for K in setups}
count = 4 * a.groups
for _ in range(a.rounds):
    for K in setups:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batches(K, count)
        torch.cuda.synchronize()
        times[K].append((time.perf_counter() - t0) * 1e3 / (count * a.batch))
for K, r in median_of(times).items():
    out[f"ms_per_image_{K}"] = r
    print(f"{K:24s} {r['ms']:.4f} ms per image (windows {r['ms_min']:.4f} .. {r['ms_max']:.4f}), {r['ms'] * a.batch:.3f} ms per batch of {a.batch}", flush=True)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f)
