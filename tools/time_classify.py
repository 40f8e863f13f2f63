#!/usr/bin/env python3
"""micro-benchmark of the classification kernels (csrc/classify.hip) and of one pretraining step, in two parts.

    python tools/time_classify.py [--rounds 5] [--reps 20] [--steps 10] [--json out/time_classify.json]

1. The three kernels alone at the shapes of a batch-64 pretraining step at 224 x 224 -- yolo_gap_fwd / yolo_gap_bwd at N = 64, C = 1024, HW = 49
   (12.8 MB each way) and yolo_softmax_xent_fwd_bwd at N = 64, K = 1000 (256 KB each way) -- next to yolo_ema_update_multi on 64 M elements
   (12 B per element, far beyond the 256-MB Infinity Cache: the streaming rate of an elementwise pass, the yardstick of tools/time_accum.py) in
   the same process.  Device events around `reps` back-to-back calls, `rounds` windows per kernel, the kernels alternating round by round; the
   median window is reported with the spread.  The new kernels' buffers fit in the cache, and back-to-back calls find them there: their GB/s are
   cache-resident rates, and what bounds kernels this small is the launch (the time column), not the memory system.
2. One pretraining step (YOLOv1Classifier(1000), batch 64, 224 x 224, SoftmaxCrossEntropy, the fused clip + SGD of yolo.optim) split by device
   events into trunk, head (pool + Linear) and loss, forward and backward, and the optimizer; and the share of the step spent in the three new
   kernels (their times of part 1 over the step's device time).

Needs the GPU: there is no fallback."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
from yolo import SoftmaxCrossEntropy, YOLOv1Classifier, engine
from yolo._hip import EmaTensor, check, lib, ptr, stream
from yolo.optim import SGD

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=None, help="also write the result there")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_classify.py measures on the GPU"
dev = torch.device("cuda")
torch.manual_seed(0)
out = {"rounds": a.rounds, "reps": a.reps, "steps": a.steps, "batch": a.batch}


def median_of(times):
    return {k: {"ms": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)} for k, v in times.items()}


def ev():
    return torch.cuda.Event(enable_timing=True)


# ---- 1. the kernels alone -----------------------------------------------------------------------------------------------------------------------
N, C, HW, K = a.batch, 1024, 49, 1000
x = torch.randn(N, C, HW, device=dev)
y = torch.empty(N, C, device=dev)
dy = torch.randn(N, C, device=dev)
dx = torch.empty(N, C, HW, device=dev)
logits = torch.randn(N, K, device=dev) * 5
labels = torch.randint(0, K, (N,), device=dev)
res, dl, hits, work = torch.empty(2, device=dev), torch.empty(N, K, device=dev), torch.empty(N, 2, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float64, device=dev)
n_ema = 64 << 20
e, p = torch.zeros(n_ema, device=dev), torch.randn(n_ema, device=dev)
ema_tab = (EmaTensor * 1)(EmaTensor(e.data_ptr(), p.data_ptr(), n_ema))


def ema():
    check(lib().yolo_ema_update_multi(ema_tab, 1, 1e-4, None, stream()), "yolo_ema_update_multi")


runs = {
    "ema_multi": (ema, 12 * n_ema),
    "gap_fwd": (lambda: check(lib().yolo_gap_fwd(ptr(x), N, C, HW, ptr(y), stream()), "yolo_gap_fwd"), 4 * (N * C * HW + N * C)),
    "gap_bwd": (lambda: check(lib().yolo_gap_bwd(ptr(dy), N, C, HW, ptr(dx), stream()), "yolo_gap_bwd"), 4 * (N * C * HW + N * C)),
    "softmax_xent": (lambda: check(lib().yolo_softmax_xent_fwd_bwd(ptr(logits), ptr(labels), N, K, 0.1, ptr(res), ptr(dl), ptr(hits), ptr(work), stream()),
                                   "yolo_softmax_xent_fwd_bwd"), 4 * 2 * N * K + 28 * N),
    "softmax_xent_fwd_only": (lambda: check(lib().yolo_softmax_xent_fwd_bwd(ptr(logits), ptr(labels), N, K, 0.1, ptr(res), None, ptr(hits), ptr(work), stream()),
                                            "yolo_softmax_xent_fwd_bwd"), 4 * N * K + 28 * N),
    "ema_multi_again": (ema, 12 * n_ema),
}
for fn, _ in runs.values():
    fn()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(a.rounds):
    for k, (fn, _) in runs.items():
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / a.reps)
for k, r in median_of(times).items():
    byts = runs[k][1]
    out[k] = dict(r, bytes=byts, GBps=round(byts / r["ms"] / 1e6, 1))
    print(f"{k:22s} {r['ms'] * 1e3:9.2f} us (windows {r['ms_min'] * 1e3:.2f} .. {r['ms_max'] * 1e3:.2f})  {byts / 1e6:9.3f} MB  {out[k]['GBps']:8.1f} GB/s", flush=True)
new_ms = out["gap_fwd"]["ms"] + out["gap_bwd"]["ms"] + out["softmax_xent"]["ms"]
del e, p, ema_tab
torch.cuda.empty_cache()

# ---- 2. one pretraining step --------------------------------------------------------------------------------------------------------------------
import synth

m = YOLOv1Classifier(K).to(dev).train()
opt = SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
opt.attach_plan(m.head_plan())
crit = SoftmaxCrossEntropy(0.1)
img = torch.from_numpy(synth.synth_images(a.batch, 0, hw=224)).to(dev)
PHASES = ("trunk_fwd", "head_fwd", "loss", "loss_bwd", "head_bwd", "trunk_bwd", "optimizer")


def step(timed):
    marks = [ev() for _ in range(8)] if timed else None

    def mark(i):
        if timed:
            marks[i].record()
    opt.zero_grad(set_to_none=True)
    mark(0)
    f = engine.run_plan(m.trunk_plan(), img, True)
    mark(1)
    lg = engine.run_plan(m.head_plan(), m.pool(f), True)
    mark(2)
    loss, parts = crit(lg, labels)
    mark(3)
    if timed:
        lg.register_hook(lambda g: marks[4].record())        # the gradient of the logits exists: the loss's backward is enqueued
        f.register_hook(lambda g: marks[5].record())         # ... of the trunk's features: Linear + pool backward are enqueued
    loss.backward()
    mark(6)
    opt.skip_if = parts.device_flag
    opt.step()
    mark(7)
    return marks


for _ in range(3):
    step(False)
torch.cuda.synchronize()
times = {k: [] for k in PHASES + ("step",)}
for _ in range(a.steps):
    marks = step(True)
    torch.cuda.synchronize()
    for i, k in enumerate(PHASES):
        times[k].append(marks[i].elapsed_time(marks[i + 1]))
    times["step"].append(marks[0].elapsed_time(marks[7]))
for k, r in median_of(times).items():
    out[f"step_{k}"] = r
    print(f"{k:10s} {r['ms']:8.3f} ms (steps {r['ms_min']:.3f} .. {r['ms_max']:.3f})", flush=True)
out["new_kernels_ms"] = round(new_ms, 5)
out["new_kernels_share"] = round(new_ms / out["step_step"]["ms"], 5)
print(f"the three new kernels: {new_ms * 1e3:.1f} us of a {out['step_step']['ms']:.3f}-ms step = {100 * out['new_kernels_share']:.2f} %", flush=True)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f)
