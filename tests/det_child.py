"""Child process of tests/test_gpu_deterministic.py (fresh process state per case, started like tests/dist_child.py).

    det_child.py repeat <out.txt> <adam|sgd> <batch> <steps>    two models from one seed, EngineConfig.DETERMINISTIC on, `steps` training steps each with the
                                                             background Linear update attached: every parameter, gradient and optimizer-state tensor must be
                                                             bit-equal between the two after every step (exit 1 otherwise); writes one hash per step
    det_child.py compare <out.pt> <batch>                    one step with the switch off and one with it on, from the same weights and batch: losses and
                                                             per-tensor gradients
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
from yolo.optim import SGD, Adam  # noqa: E402


def _batch(n):
    x = torch.from_numpy(synth.synth_images(n, 0)).cuda()
    t = torch.from_numpy(synth.synth_targets(n, 1)).cuda()
    return x, t


def _make(kind, seed):
    torch.manual_seed(seed)
    model = YOLOv1().cuda().train()
    params = list(model.parameters())
    if kind == "sgd":
        opt = SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
    else:
        opt = Adam(params, lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(model.hip_plan(), overlap=True)
    return model, opt


def _step(model, opt, crit, x, t, seed):
    """one training step; -> (loss, {name: tensor} of every parameter, gradient and optimizer-state tensor afterwards)"""
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
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                out[f"s.{k}.{n}"] = v.detach().clone()
    return out


def _hash(tensors):
    h = hashlib.sha256()
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(tensors[k].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def repeat(out, kind, batch, steps):
    CONFIG.DETERMINISTIC = True
    crit = YOLOLoss()
    x, t = _batch(batch)
    a, oa = _make(kind, 5)
    b, ob = _make(kind, 5)
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


def compare(out, batch):
    crit = YOLOLoss()
    x, t = _batch(batch)
    res = {}
    for flag in (False, True):
        CONFIG.DETERMINISTIC = flag
        m, o = _make("adam", 9)
        r = _step(m, o, crit, x, t, 77)
        res[flag] = {k: v.cpu() for k, v in r.items() if k == "loss" or k.startswith("g.")}
        del m, o, r
    torch.save({"off": res[False], "on": res[True]}, out)


if __name__ == "__main__":
    if sys.argv[1] == "repeat":
        repeat(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    elif sys.argv[1] == "compare":
        compare(sys.argv[2], int(sys.argv[3]))
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]}")
