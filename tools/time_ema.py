#!/usr/bin/env python3
"""micro-benchmark of the weight EMA (csrc/ema.hip, yolo.optim.ModelEMA), in two parts.

    python tools/time_ema.py [--rounds 5] [--reps 10] [--steps 30] [--json out/time_ema.json]

1. The pass alone, over the YOLOv1 model's real tensor list (52 tensors, the Linear behind nn.Flatten 205 M of the 271.7 M elements): the single
   form (52 launches), the multi-tensor form (2 launches) and the background form on the tensors it is used for (the Linear layers, 76 % of the
   bytes) with BG_CUS and with 256 workgroups, next to yolo_sgd_step_multi on the same list in the same run -- both are plain streaming passes.
   Bytes a pass must move: 12 B per element for the EMA (read e, p; write e), 20 B for SGD with momentum (+ 2 B per shadowed element).  Device
   events around `reps` back-to-back passes, `rounds` windows per kernel, the kernels alternating round by round; the median window is reported
   with the spread.  The lists (3-5 GB) are far larger than the 256-MB Infinity Cache, so every pass streams from HBM.
2. The training step at batch 64 (forward, loss, backward, fused clip + Adam with the Linear layers on the second stream), `steps` steps behind
   a warm-up, host clock around a window that ends in a device synchronise: EMA off, EMA on with every launch in the foreground
   (ModelEMA(background=False)), EMA on with the Linear layers in the background.  The three alternate over `rounds` windows.

Needs the GPU: there is no fallback."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
from yolo import ModelEMA, YOLOLoss, YOLOv1
from yolo._hip import EmaTensor, SgdTensor, check, lib, ptr, stream
from yolo.optim import BG_CUS, Adam

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=None, help="also write the result there")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_ema.py measures on the GPU"
dev = torch.device("cuda")
torch.manual_seed(0)
out = {"rounds": a.rounds, "reps": a.reps, "steps": a.steps, "batch": a.batch}


def median_of(times):
    return {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}


# ---- 1. the pass alone -------------------------------------------------------------------------------------------------------------------------
model = YOLOv1().to(dev)
params = [p.detach() for p in model.parameters()]
assert len(params) == 52
elems = sum(p.numel() for p in params)
avg = [p.clone() for p in params]
g = [torch.randn_like(p) * 1e-2 for p in params]
buf = [torch.zeros_like(p) for p in params]
shadow = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) if p.dim() == 2 else None for p in params]
sh_elems = sum(p.numel() for p, s in zip(params, shadow) if s is not None)
norm = torch.tensor([sum(float(x.double().pow(2).sum()) for x in g)], dtype=torch.float64, device=dev)
ema_tab = (EmaTensor * 52)(*[EmaTensor(e.data_ptr(), p.data_ptr(), p.numel()) for e, p in zip(avg, params)])
fc = [i for i, p in enumerate(model.named_parameters()) if p[0].startswith("head.")]        # the Linear layers' weights and biases
fc_elems = sum(params[i].numel() for i in fc)
fc_tab = (EmaTensor * len(fc))(*[ema_tab[i] for i in fc])
sgd_tab = (SgdTensor * 52)(*[SgdTensor(p.data_ptr(), x.data_ptr(), b.data_ptr(), s.data_ptr() if s is not None else None, p.numel())
                             for p, x, b, s in zip(params, g, buf, shadow)])
W = 1e-4


def ema_single():
    for t in ema_tab:
        check(lib().yolo_ema_update(t.ema, t.p, t.n, W, None, stream()), "yolo_ema_update")


runs = {
    "ema_single": (ema_single, 12 * elems),
    "ema_multi": (lambda: check(lib().yolo_ema_update_multi(ema_tab, 52, W, None, stream()), "yolo_ema_update_multi"), 12 * elems),
    f"ema_bg_fc_{BG_CUS}": (lambda: check(lib().yolo_ema_update_multi_bg(fc_tab, len(fc), W, None, BG_CUS, stream()), "yolo_ema_update_multi_bg"), 12 * fc_elems),
    "ema_bg_fc_256": (lambda: check(lib().yolo_ema_update_multi_bg(fc_tab, len(fc), W, None, 256, stream()), "yolo_ema_update_multi_bg"), 12 * fc_elems),
    "sgd_multi": (lambda: check(lib().yolo_sgd_step_multi(sgd_tab, 52, 1e-4, 0.9, 0.0, 5e-4, 0, 0, ptr(norm), 10.0, None, stream()), "yolo_sgd_step_multi"),
                  20 * elems + 2 * sh_elems),
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
out["elements"], out["fc_elements"] = elems, fc_elems
for k, r in median_of(times).items():
    byts = runs[k][1]
    out[k] = dict(r, bytes=byts, GBps=round(byts / r["ms"] / 1e6, 1))
    print(f"{k:15s} {r['ms']:7.3f} ms (windows {r['ms_min']:.3f} .. {r['ms_max']:.3f})  {byts / 1e9:6.3f} GB  {out[k]['GBps']:7.1f} GB/s", flush=True)
out["ema_multi_over_sgd_rate"] = round(out["ema_multi"]["GBps"] / out["sgd_multi"]["GBps"], 4)
print(f"ema_multi bytes/s over sgd_multi bytes/s: {out['ema_multi_over_sgd_rate']:.3f}", flush=True)
del model, params, avg, g, buf, shadow, ema_tab, fc_tab, sgd_tab
torch.cuda.empty_cache()

# ---- 2. inside the training step ---------------------------------------------------------------------------------------------------------------
import synth

x = torch.from_numpy(synth.synth_images(a.batch, 0)).to(dev)
t = torch.from_numpy(synth.synth_targets(a.batch, 1)).to(dev)
crit = YOLOLoss()
setups = {}
for name, background in (("ema_off", None), ("ema_foreground", False), ("ema_background", True)):
    torch.manual_seed(0)
    m = YOLOv1().to(dev).train()
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(m.hip_plan(), overlap=True)
    ema = ModelEMA(m, decay=0.9999, optimizer=opt, background=background) if background is not None else None
    setups[name] = (m, opt, ema)


def steps(name, n):
    m, opt, ema = setups[name]
    for _ in range(n):
        opt.zero_grad(set_to_none=True)
        loss, parts = crit(m(x), t)
        loss.backward()
        opt.skip_if = parts.device_flag
        opt.step()
        if ema is not None:
            ema.update(m)


for name in setups:
    steps(name, 5)
torch.cuda.synchronize()
times = {k: [] for k in setups}
for _ in range(a.rounds):
    for name in setups:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(name, a.steps)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
for k, r in median_of(times).items():
    out["step_" + k] = r
    print(f"step {k:15s} {r['ms']:7.3f} ms (windows {r['ms_min']:.3f} .. {r['ms_max']:.3f})", flush=True)
print(f"step + stand-alone multi pass would be {out['step_ema_off']['ms'] + out['ema_multi']['ms']:.3f} ms", flush=True)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f)
