"""Child process of tests/test_gpu_lars.py (EngineConfig.DETERMINISTIC is read from YOLO_AMD_DETERMINISTIC at import, so the parent sets it).

    lars_child.py det <out.txt> <batch> <steps>    two YOLOv1 models from one seed, yolo.optim.LARS on lars_param_groups with the background Linear update
                                                   attached, `steps` training steps each: every parameter, gradient and momentum buffer must be bit-equal
                                                   between the two after every step (exit 1 otherwise); writes one hash per step
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import synth  # noqa: E402
from yolo import YOLOLoss, YOLOv1  # noqa: E402
from yolo.config import CONFIG  # noqa: E402
from yolo.optim import LARS, lars_param_groups  # noqa: E402


def _make(seed):
    torch.manual_seed(seed)
    model = YOLOv1().cuda().train()
    opt = LARS(lars_param_groups(model, 5e-4), lr=1e-2, momentum=0.9, eta=1e-3, max_grad_norm=10.0)
    opt.attach_plan(model.hip_plan(), overlap=True)
    return model, opt


def _step(model, opt, crit, x, t, seed):
    torch.manual_seed(seed)            # the dropout mask
    loss, _ = crit(model(x), t)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    opt.step()
    opt.synchronize()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone()}
    for n, p in model.named_parameters():
        out["p." + n] = p.detach().clone()
        out["g." + n] = grads[n]
        out["b." + n] = opt.state[p]["momentum_buffer"].detach().clone()
    return out


def _hash(tensors):
    h = hashlib.sha256()
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(tensors[k].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def det(out, batch, steps):
    assert CONFIG.DETERMINISTIC, "the parent sets YOLO_AMD_DETERMINISTIC=1"
    crit = YOLOLoss()
    x = torch.from_numpy(synth.synth_images(batch, 0)).cuda()
    t = torch.from_numpy(synth.synth_targets(batch, 1)).cuda()
    a, oa = _make(5)
    b, ob = _make(5)
    lines = []
    for s in range(steps):
        ra = _step(a, oa, crit, x, t, 100 + s)
        rb = _step(b, ob, crit, x, t, 100 + s)
        diff = [k for k in ra if not torch.equal(ra[k], rb[k])]
        if diff:
            print(f"step {s}: {len(diff)} of {len(ra)} tensors differ between the two models: {diff[:12]}")
            sys.exit(1)
        assert all(bool(torch.isfinite(v).all()) for v in ra.values()), f"step {s}: non-finite tensor"
        lines.append(_hash(ra))
        del ra, rb
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "det":
        det(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]}")
