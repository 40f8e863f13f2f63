"""Child process of tests/test_gpu_accum.py (not a test module; fresh process state, started like tests/dist_child.py and tests/ema_child.py).

    accum_child.py det <out.txt>
        EngineConfig.DETERMINISTIC (the parent sets YOLO_AMD_DETERMINISTIC=1): K = 3 micro-batches of 2 images through yolo.optim.GradAccumulator
        on YOLOv1, then Adam(max_grad_norm=10).step() -- twice from the same weights.  The folded gradients and the stepped parameters of the two
        runs must be bit-equal.

    python -m torch.distributed.run --nproc-per-node 2 ... accum_child.py ranks <out.pt>
        two ranks on ONE GPU over gloo (RCCL refuses to use a device twice, gloo stages through the host), deterministic mode, K = 2, 2 images per
        micro-batch per rank.  Each rank first takes its two raw micro-gradients from a second model instance with the same weights and no
        gradient arena, then runs the shipped path: make_grad_reducer + GradAccumulator + Adam.step.  Writes <out.pt>.r<rank> with what the
        parent compares.

Exit status 1 at the first violation, with a message."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import synth  # noqa: E402
from yolo import GradAccumulator, YOLOLoss, YOLOv1  # noqa: E402
from yolo.config import CONFIG  # noqa: E402
from yolo.optim import Adam  # noqa: E402


def build():
    m = YOLOv1()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.yolov1_state_dict().items()}, strict=True)
    return m.cuda().eval()                      # eval: no dropout, so that every pass sees the same network


def small(named):
    """what dist_child.py saves: the biases and the tensors under 2^20 elements"""
    return {n: v.detach().float().cpu().clone() for n, v in named if v.dim() == 1 or v.numel() < (1 << 20)}


def group(m, opt, acc, x, t, K, red=None):
    """one K-step group as training.train_epoch runs it -> (buckets the reducer had enqueued after the first micro-step, the group's flag)"""
    crit = YOLOLoss()
    after_first = None
    for k in range(K):
        opt.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, parts = crit(m(x[2 * k: 2 * k + 2]), t[2 * k: 2 * k + 2])
        loss.backward()
        done = acc.after_backward(parts.device_flag)
        if k == 0 and red is not None:
            after_first = len(red.log)
        assert done is (k == K - 1)
        assert float(parts["total"]) > 0
    return after_first, acc.skip_if


def det(out_path):
    assert CONFIG.DETERMINISTIC, "the parent sets YOLO_AMD_DETERMINISTIC=1"
    K = 3
    x = torch.from_numpy(synth.synth_images(2 * K, 23)).cuda()
    t = torch.from_numpy(synth.synth_targets(2 * K, 41, max_obj=3)).cuda()
    got = []
    for run in range(2):
        m = build()
        opt = Adam(m.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
        opt.attach_plan(m.hip_plan(), overlap=True)
        acc = GradAccumulator(m, K)
        _, skip = group(m, opt, acc, x, t, K)
        grads = {n: p.grad.detach().clone().view(torch.int32) for n, p in m.named_parameters()}
        opt.skip_if = skip
        opt.step()
        opt.synchronize()
        torch.cuda.synchronize()
        got.append((grads, {n: p.detach().clone().view(torch.int32) for n, p in m.named_parameters()}))
        del m, opt, acc
    for what, a, b in (("folded gradients", got[0][0], got[1][0]), ("stepped parameters", got[0][1], got[1][1])):
        diff = [n for n in a if not torch.equal(a[n], b[n])]
        if diff:
            print(f"det: {len(diff)} of {len(a)} {what} differ between two runs from the same weights: {diff[:12]}")
            sys.exit(1)
    with open(out_path, "w") as f:
        f.write(f"det: folded gradients and stepped parameters bit-equal over {len(got[0][0])} tensors\n")


def ranks(out_path):
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2 and CONFIG.DETERMINISTIC
    from yolo.parallel import broadcast_parameters, make_grad_reducer
    K = 2
    xs = torch.from_numpy(synth.synth_images(2 * K * world, 23)).cuda()
    ts = torch.from_numpy(synth.synth_targets(2 * K * world, 41, max_obj=3)).cuda()
    lo = rank * 2 * K
    x, t = xs[lo: lo + 2 * K].contiguous(), ts[lo: lo + 2 * K].contiguous()
    # the raw micro-gradients: a second instance, no arena, no accumulator
    plain = build()
    broadcast_parameters(plain)
    raw = []
    for k in range(K):
        plain.zero_grad(set_to_none=True)
        loss, _ = YOLOLoss()(plain(x[2 * k: 2 * k + 2]), t[2 * k: 2 * k + 2])
        loss.backward()
        raw.append(small((n, p.grad) for n, p in plain.named_parameters()))
    assert plain.hip_plan().arena is None
    del plain
    # the shipped path
    m = build()
    broadcast_parameters(m)
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(m.hip_plan())
    red = make_grad_reducer(m, "cuda")
    red.log = []
    acc = GradAccumulator(m, K, red)
    after_first, skip = group(m, opt, acc, x, t, K, red)
    grads = small((n, p.grad) for n, p in m.named_parameters())
    opt.skip_if = skip
    opt.step()
    torch.cuda.synchronize()
    params = {n: p.detach().float().cpu().clone() for n, p in m.named_parameters() if p.dim() == 1}
    torch.save({"raw": raw, "grads": grads, "params": params, "reducer": type(red).__name__, "deterministic": bool(CONFIG.DETERMINISTIC),
                "buckets_after_micro_1": after_first, "buckets": len(red.log), "skip": float(skip)}, f"{out_path}.r{rank}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "det":
        det(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "ranks":
        ranks(sys.argv[2])
    else:
        raise SystemExit(f"usage: {sys.argv[0]} det <out.txt> | ranks <out.pt>")
