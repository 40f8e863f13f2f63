"""Child process of tests/test_gpu_ema.py (fresh process state, started like tests/det_child.py).

    ema_child.py steps <out.txt>

YOLOv1 at batch 4 with yolo.optim.Adam(max_grad_norm=10), the Linear layers' update on the second stream (attach_plan(overlap=True)) and a
ModelEMA(decay=0.9) that follows it there.  Three training steps, four times from the same initial weights:

  default      nothing waits between opt.step(), ema.update() and the next forward; after each step opt.synchronize() and a snapshot of the
               parameters.  The averaged tensors must lie within the propagated bound of the fp64 recurrence over the snapshots
               (tests/ema_ref.py), and ema.module(x) in eval mode must equal, bit for bit, a fresh YOLOv1 loaded from
               ema.state_dict()["module"] -- ema.module ran a forward after the first step, so its plan holds bf16 operands packed from older
               averages and has to notice the later updates.
  det          the same with EngineConfig.DETERMINISTIC on (the gradients, and with them the parameters, then repeat bit for bit)
  det-sync     ... with a torch.cuda.synchronize() after every call: two orderings of the same work, the averages must be bit-equal to `det`
  det-again    `det` once more: two runs from one seed, bit-equal averages

Exit status 1 at the first violation, with a message; <out.txt> receives one line per run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import ema_ref as emr  # noqa: E402
import launch_ref as lr  # noqa: E402
import synth  # noqa: E402
from yolo import ModelEMA, YOLOLoss, YOLOv1  # noqa: E402
from yolo.config import CONFIG  # noqa: E402
from yolo.optim import Adam  # noqa: E402

DECAY, STEPS, BATCH = 0.9, 3, 4


def run(init, x, t, sync: bool):
    """-> (ema, [initial weights], [snapshot of the parameters after each step]); `sync`: the host waits for the device after every call"""
    wait = torch.cuda.synchronize if sync else (lambda: None)
    model = YOLOv1().cuda().train()
    model.load_state_dict(init)
    opt = Adam(model.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(model.hip_plan(), overlap=True)
    ema = ModelEMA(model, decay=DECAY, optimizer=opt)
    crit = YOLOLoss()
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    snaps = []
    for s in range(STEPS):
        torch.manual_seed(100 + s)            # the dropout mask
        out = model(x)
        wait()
        loss, parts = crit(out, t)
        wait()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        wait()
        opt.skip_if = parts.device_flag       # zero for these targets: the flag travels to both streams and cancels nothing
        opt.step()
        wait()
        ema.update(model)
        wait()
        assert opt._pending is not None and ema._event is not None, "the Linear layers must have gone to the second stream"
        opt.synchronize()
        snaps.append({k: v.detach().clone() for k, v in model.named_parameters()})
        wait()
        if s == 0:
            with torch.no_grad():
                ema.module(x)                 # packs the plan's bf16 operands from the first average
            wait()
    assert ema.updates == STEPS and float(parts["total"]) > 0
    return ema, start, snaps


def bits(ema):
    """the averaged tensors as stored (state_dict() makes the current stream wait for the background launch)"""
    return {k: v.detach().clone().view(torch.int32) for k, v in ema.state_dict()["module"].items()}


def main(out_path):
    torch.manual_seed(5)
    init = {k: v.clone() for k, v in YOLOv1().state_dict().items()}
    x = torch.from_numpy(synth.synth_images(BATCH, 0)).cuda()
    t = torch.from_numpy(synth.synth_targets(BATCH, 1)).cuda()
    lines, got = [], {}
    for name, det, sync in (("default", False, False), ("det", True, False), ("det-sync", True, True), ("det-again", True, False)):
        CONFIG.DETERMINISTIC = det
        ema, start, snaps = run(init, x, t, sync)
        avg = ema.state_dict()["module"]
        assert list(avg) == list(start) and len(avg) == 52
        fails, worst = [], 0.0
        w = emr.ema_weight(DECAY)
        for k, v in avg.items():
            ref, bnd = emr.ema_chain_ref(start[k], [s[k] for s in snaps], [w] * STEPS)
            worst = max(worst, lr.check_values(ref, bnd, v, k, fails, name))
            if torch.equal(v, start[k]) or torch.equal(v, snaps[-1][k]):
                fails.append(f"{name}: {k}: the average did not move, or is the model")
        lines.append(f"{name}: worst |err| / bound {worst:.3f} over {len(avg)} tensors")
        print(lines[-1], flush=True)
        if fails:
            print("\n".join(fails[:12]))
            sys.exit(1)
        got[name] = bits(ema)
        if name == "default":
            fresh = YOLOv1().cuda().eval()
            fresh.load_state_dict(avg)
            with torch.no_grad():
                ya, yb = ema.module(x), fresh(x)
            torch.cuda.synchronize()
            if not torch.equal(ya.view(torch.int32), yb.view(torch.int32)):
                print(f"ema.module(x) differs from a fresh model with the same weights in {int((ya != yb).sum())} of {ya.numel()} outputs: "
                      "its plan kept operands packed from an older average")
                sys.exit(1)
            lines.append("default: ema.module(x) == fresh model from ema.state_dict(), bit for bit")
            del fresh
        del ema, start, snaps, avg
    for other in ("det-sync", "det-again"):
        diff = [k for k in got["det"] if not torch.equal(got["det"][k], got[other][k])]
        if diff:
            print(f"{other}: {len(diff)} of {len(got['det'])} averaged tensors differ from the unsynchronised deterministic run: {diff[:12]}")
            sys.exit(1)
        lines.append(f"{other}: bit-equal to det")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "steps":
        main(sys.argv[2])
    else:
        raise SystemExit(f"usage: {sys.argv[0]} steps <out.txt>")
