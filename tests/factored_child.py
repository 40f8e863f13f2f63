"""Child process of tests/test_gpu_fc_factored.py (not a test module; started like tests/det_child.py and tests/dist_child.py), and the small model
both share: a 64-channel 4 x 4 map through Conv2d(64, 64, 1) + LeakyReLU -> Flatten -> Linear(1024, 256) -> LeakyReLU -> Dropout(p = 0) -> Linear(256, 24)
at batch 8, one engine plan.  The parent sets the switches in the environment (YOLO_AMD_FC_FACTORED, YOLO_AMD_FC_FACTORED_MIN, YOLO_AMD_DETERMINISTIC).

    factored_child.py det <out.txt>          three Adam steps with the background update of the Linear layers attached; writes one hash of all
                                             parameters and optimizer state per step
    factored_child.py gloo2 <out.pt>         (under torch.distributed.run, two ranks on one GPU over gloo) one SGD-with-momentum step through
                                             OverlappedGradAllReduce, each rank on its half of the batch; writes <out.pt>.r<rank>
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

FC_MIN = 100000        # FC_FACTORED_MIN of the small model: Linear(1024, 256) qualifies (262144 weights), Linear(256, 24) does not
BATCH = 8


def small_model(seed=0, device="cuda"):
    torch.manual_seed(seed)
    mods = nn.Sequential(nn.Conv2d(64, 64, 1), nn.LeakyReLU(0.1), nn.Flatten(), nn.Linear(64 * 4 * 4, 256), nn.LeakyReLU(0.1), nn.Dropout(0.0),
                         nn.Linear(256, 24))
    return mods.to(device)


def small_batch(n=BATCH, seed=1, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((n, 64, 4, 4), generator=gen).to(device), torch.randn((n, 24), generator=gen).to(device)


def make_plan(mods):
    from yolo import engine
    return engine.Plan.from_modules(list(mods), 64, False)


def loss_of(plan, x, gy):
    """a loss whose gradient wrt the plan's output is gy / rows: the mean over the batch of <y, gy>, as YOLOLoss divides by the local N"""
    from yolo import engine
    return (engine.run_plan(plan, x, True) * gy).sum() / x.shape[0]


def _hash(tensors):
    h = hashlib.sha256()
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(tensors[k].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def det(out):
    from yolo.config import CONFIG
    from yolo.optim import Adam
    assert CONFIG.DETERMINISTIC and CONFIG.FC_FACTORED and CONFIG.FC_FACTORED_MIN == FC_MIN, "the parent sets the switches in the environment"
    mods = small_model(5)
    plan = make_plan(mods)
    opt = Adam(mods.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=1.0)
    opt.attach_plan(plan, overlap=True)
    w1 = mods[3].weight
    lines = []
    for s in range(3):
        x, gy = small_batch(seed=10 + s)
        opt.zero_grad(set_to_none=True)
        loss_of(plan, x, gy).backward()
        assert w1.grad is None and id(w1) in plan.fc_factors
        opt.step()
        opt.synchronize()
        torch.cuda.synchronize()
        t = {"p." + n: p for n, p in mods.named_parameters()}
        for n, p in mods.named_parameters():
            for k, v in opt.state[p].items():
                if torch.is_tensor(v):
                    t[f"s.{k}.{n}"] = v
        assert all(bool(torch.isfinite(v).all()) for v in t.values())
        lines.append(_hash(t))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def gloo2(out):
    import torch.distributed as dist
    from yolo.config import CONFIG
    from yolo.optim import SGD
    from yolo.parallel import OverlappedGradAllReduce, broadcast_parameters, shard_batch
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mods = small_model(7)
    broadcast_parameters(mods)
    plan = make_plan(mods)
    opt = SGD(mods.parameters(), lr=0.5, momentum=0.9, max_grad_norm=1e6)      # the clip is computed and inactive: SGD stays linear in g
    opt.attach_plan(plan)
    red = OverlappedGradAllReduce(plan, "cuda")
    x, gy = small_batch(seed=3)
    sl = shard_batch(BATCH, rank, world)
    opt.zero_grad(set_to_none=True)
    loss_of(plan, x[sl].contiguous(), gy[sl].contiguous()).backward()
    w1 = mods[3].weight
    local = plan.fc_factors.get(id(w1))
    red.all_reduce_mean()
    rec = plan.fc_factors.get(id(w1))
    res = {"factored": bool(CONFIG.FC_FACTORED), "arena_numel": int(red.arena.numel()), "payload_bytes": int(red.payload_bytes),
           "w1_numel": int(w1.numel()), "w1_grad_is_none": w1.grad is None}
    if rec is not None:
        res.update(rows=rec.rows, scale=rec.scale, local_rows=local.rows, dy=rec.dy.cpu(), x=rec.x.cpu(), g=plan.fc_weight_grad(w1).cpu())
    else:
        res["g"] = w1.grad.detach().cpu().clone()
    opt.step()
    opt.synchronize()
    torch.cuda.synchronize()
    res["params"] = {n: p.detach().cpu().clone() for n, p in mods.named_parameters()}
    res["buf"] = {n: opt.state[p]["momentum_buffer"].cpu().clone() for n, p in mods.named_parameters()}
    torch.save(res, f"{out}.r{rank}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if sys.argv[1] == "det":
        det(sys.argv[2])
    elif sys.argv[1] == "gloo2":
        gloo2(sys.argv[2])
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]}")
