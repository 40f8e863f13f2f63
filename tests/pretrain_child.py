"""Child process of tests/test_pretrain_scale_cpu.py and tests/test_gpu_pretrain_scale.py (not a test module; fresh process state, started like
tests/accum_child.py and tests/dist_child.py).

    python -m torch.distributed.run --nproc-per-node 2 ... pretrain_child.py cpu_ranks <out.pt>
        two ranks over gloo on the CPU: the He-initialised YOLOv1Classifier(4), rank r seeded differently and then given rank 0's parameters,
        4 of the 8 learning-set images each; the reducer make_grad_reducer picks (GradAllReduce), one plain SGD step.  Writes <out.pt>.r<rank>:
        the averaged gradients and the stepped parameters.

    python -m torch.distributed.run --nproc-per-node 2 ... pretrain_child.py ranks <out.pt>
        two ranks on ONE GPU over gloo (RCCL refuses to use a device twice, gloo stages through the host), deterministic mode, K = 2, 2 images per
        micro-batch per rank -- the harness of accum_child.py ranks on the classifier's two plans.  Each rank first takes its two raw
        micro-gradients from a second model instance with the same weights and no gradient arena, then runs the shipped path: make_grad_reducer
        (one overlapped reducer per plan) + GradAccumulator + SGD.step.  Writes <out.pt>.r<rank> with what the parent compares.

    python -m torch.distributed.run --nproc-per-node 2 ... pretrain_child.py cli <pretrain.py arguments>
        pretrain.py's main() as two ranks on ONE GPU: the process group the script asks for ("nccl" on cuda) is opened over gloo and every rank
        stays on device 0, for the reason above; everything else -- sampler, broadcast, reducers, accumulator, rank 0's checkpoints, barriers --
        is the script's own.

Exit status 1 at the first violation, with a message."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import pretrain_scale_ref as ps  # noqa: E402


def small(named):
    """what accum_child.py saves: the biases and the tensors under 2^20 elements"""
    return {n: v.detach().float().cpu().clone() for n, v in named if v.dim() == 1 or v.numel() < (1 << 20)}


def cpu_ranks(out_path):
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from yolo import SoftmaxCrossEntropy
    from yolo.parallel import broadcast_parameters, make_grad_reducer, shard_batch
    m = ps.classifier(4, "kaiming", seed=100 + rank).train()          # different per rank: the broadcast must fix it
    broadcast_parameters(m)
    x, y = ps.learn_set()
    sl = shard_batch(8, rank, world)
    red = make_grad_reducer(m, "cpu")
    assert type(red).__name__ == "GradAllReduce", type(red).__name__
    opt = torch.optim.SGD(m.parameters(), lr=ps.LEARN_LR)
    loss, _ = SoftmaxCrossEntropy()(m(x[sl]), y[sl])
    loss.backward()
    red.all_reduce_mean()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    opt.step()
    torch.save({"grads": grads, "params": {n: p.detach().clone() for n, p in m.named_parameters()}}, f"{out_path}.r{rank}")
    dist.barrier()
    dist.destroy_process_group()


def ranks(out_path):
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from yolo import GradAccumulator, SoftmaxCrossEntropy
    from yolo.config import CONFIG
    from yolo.optim import SGD
    from yolo.parallel import broadcast_parameters, make_grad_reducer
    assert world == 2 and CONFIG.DETERMINISTIC, "the parent sets YOLO_AMD_DETERMINISTIC=1"
    K = 2
    xs, ys = ps.learn_set("cuda")                                      # 8 images = 2 ranks x K x 2
    lo = rank * 2 * K
    x, y = xs[lo: lo + 2 * K].contiguous(), ys[lo: lo + 2 * K].contiguous()
    crit = SoftmaxCrossEntropy()
    # the raw micro-gradients: a second instance, no arena, no accumulator
    plain = ps.classifier(4, "kaiming").cuda().train()
    broadcast_parameters(plain)
    raw = []
    for k in range(K):
        plain.zero_grad(set_to_none=True)
        loss, _ = crit(plain(x[2 * k: 2 * k + 2]), y[2 * k: 2 * k + 2])
        loss.backward()
        raw.append(small((n, p.grad) for n, p in plain.named_parameters()))
    assert all(plan.arena is None for plan in plain.hip_plans())
    del plain
    # the shipped path
    m = ps.classifier(4, "kaiming").cuda().train()
    broadcast_parameters(m)
    opt = SGD(m.parameters(), lr=ps.LEARN_LR, max_grad_norm=ps.CLIP)
    opt.attach_plan(m.head_plan())
    red = make_grad_reducer(m, "cuda")
    kinds = [type(r).__name__ for r in red.reducers]
    plans = [r.plan for r in red.reducers]
    assert plans[0] is m.head_plan() and plans[1] is m.trunk_plan(), "the order backward runs the plans in: head first"
    for r in red.reducers:
        r.log = []
    acc = GradAccumulator(m, K, red)
    after_first = None
    for k in range(K):
        opt.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, parts = crit(m(x[2 * k: 2 * k + 2]), y[2 * k: 2 * k + 2])
        loss.backward()
        done = acc.after_backward(parts.device_flag)
        if k == 0:
            after_first = [len(r.log) for r in red.reducers]
        assert done is (k == K - 1)
        assert float(parts["total"]) > 0
    grads = small((n, p.grad) for n, p in m.named_parameters())
    opt.skip_if = acc.skip_if
    opt.step()
    torch.cuda.synchronize()
    params = {n: p.detach().float().cpu().clone() for n, p in m.named_parameters() if p.dim() == 1}
    torch.save({"raw": raw, "grads": grads, "params": params, "reducers": kinds, "deterministic": bool(CONFIG.DETERMINISTIC),
                "buckets_after_micro_1": after_first, "buckets": [len(r.log) for r in red.reducers], "skip": float(acc.skip_if)}, f"{out_path}.r{rank}")
    dist.barrier()
    dist.destroy_process_group()


def cli(argv):
    import runpy
    torch.cuda.set_device(0)
    torch.cuda.set_device = lambda _index: None                       # LOCAL_RANK 1 stays on the one device
    opened = dist.init_process_group
    asked = []

    def over_gloo(backend=None, *a, **k):
        asked.append(backend)
        return opened("gloo", *a, **k)
    dist.init_process_group = over_gloo
    sys.argv = [os.path.join(ROOT, "yolo-v1_amd", "pretrain.py")] + list(argv)
    runpy.run_path(sys.argv[0], run_name="__main__")
    assert asked == ["nccl"], f"pretrain.py --device cuda asks for RCCL: {asked}"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] in ("cpu_ranks", "ranks"):
        {"cpu_ranks": cpu_ranks, "ranks": ranks}[sys.argv[1]](sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "cli":
        cli(sys.argv[2:])
    else:
        raise SystemExit(f"usage: {sys.argv[0]} cpu_ranks <out.pt> | ranks <out.pt> | cli <pretrain.py arguments>")
