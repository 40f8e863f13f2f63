"""Numpy fp64 restatements of what csrc/classify.hip computes: the global average pool, the softmax cross-entropy row loss with label smoothing,
its gradient and the top-k hit rule -- plus the input cases the loss tests share and the measurement their tolerance comes from.

    python tests/classify_ref.py        prints the error of stock torch's fp32 CPU cross_entropy (forward, backward) against these fp64 formulas on
                                        xent_cases(): the figure DESIGN.md and tests/test_gpu_classify.py cite
"""

import numpy as np

XENT_SHAPES = [(1, 1), (3, 4), (5, 7), (4, 1000), (2, 1001), (3, 4099)]        # (N, K)
XENT_EPS = [0.0, 0.1]
KINDS = ("normal", "equal", "big", "label_max", "label_min", "ties")


def gap(x):
    """x [N][C][HW] -> [N][C] fp64 mean over HW"""
    return np.asarray(x, dtype=np.float64).mean(-1)


def gap_bound(x):
    """|err| allowed per output of an fp32 sum of HW terms plus one multiply: (HW + 2) * 2^-24 * sum|x| / HW"""
    x = np.asarray(x, dtype=np.float64)
    HW = x.shape[-1]
    return (HW + 2) * 2.0 ** -24 * np.abs(x).sum(-1) / HW


def gap_bwd(dy, HW):
    """dy [N][C] fp32 -> [N][C][HW] fp32: one fp32 multiply per element by (float)(1.0 / HW)"""
    dy = np.asarray(dy, dtype=np.float32)
    return np.repeat((dy * np.float32(1.0 / HW))[..., None], HW, axis=-1)


def xent(logits, labels, eps):
    """logits [N][K], labels [N] -> (mean loss, row losses [N], dlogits [N][K], hits [N][2] int32, flag), all fp64 arithmetic.
    Row loss = (1 - eps) (lse - x_y) + eps (lse - mean x); dlogits = (softmax - ((1 - eps) onehot + eps / K)) / N.
    A label outside [0, K): zero loss, zero gradient row, no hits, flag = 1.  The mean divides by N whatever the labels."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    N, K = x.shape
    valid = (y >= 0) & (y < K)
    ys = np.where(valid, y, 0)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    xy = x[np.arange(N), ys]
    rows = ((1.0 - eps) * (lse - xy) + eps * (lse - x.mean(1))) * valid
    target = np.full((N, K), eps / K)
    target[np.arange(N), ys] += 1.0 - eps
    d = (e / s - target) / N * valid[:, None]
    return rows.sum() / N, rows, d, hits(x, y), float((~valid).any())


def hits(logits, labels):
    """[N][2] int32 {top-1, top-5}: a hit at k = fewer than k logits of the row are STRICTLY greater than the label's logit (no sort; a tie with
    the label's logit never costs the hit); a label outside [0, K) never hits"""
    x = np.asarray(logits)
    y = np.asarray(labels, dtype=np.int64)
    N, K = x.shape
    valid = (y >= 0) & (y < K)
    xy = x[np.arange(N), np.where(valid, y, 0)]
    above = (x > xy[:, None]).sum(1)
    return np.stack([(above < 1) & valid, (above < 5) & valid], 1).astype(np.int32)


def xent_case(N, K, shift, seed=0):
    """fp32 logits [N][K] and labels [N]; row r is of kind KINDS[(r + shift) % 6]:
      normal     5 * standard normal, a random label
      equal      every logit the same value (all tied)
      big        magnitude 88 with both signs (exp(88) is finite in fp32, a sum of two of them is not: needs the max subtraction)
      label_max  5 * normal, the label on the maximum
      label_min  5 * normal, the label on the minimum
      ties       2 * normal rounded to integers (many exact ties), a random label"""
    rng = np.random.Generator(np.random.PCG64([seed, N, K, shift]))
    x = np.empty((N, K), dtype=np.float32)
    y = np.empty((N,), dtype=np.int64)
    for r in range(N):
        kind = KINDS[(r + shift) % len(KINDS)]
        row = (5.0 * rng.standard_normal(K)).astype(np.float32)
        lab = int(rng.integers(0, K))
        if kind == "equal":
            row[:] = np.float32(rng.uniform(-3, 3))
        elif kind == "big":
            sign = np.where(rng.integers(0, 2, K) > 0, 1.0, -1.0)
            if K > 1:
                sign[0], sign[1] = 1.0, -1.0
            row = (88.0 * sign + 0.25 * rng.standard_normal(K)).astype(np.float32)
        elif kind == "label_max":
            lab = int(row.argmax())
        elif kind == "label_min":
            lab = int(row.argmin())
        elif kind == "ties":
            row = np.round(2.0 * rng.standard_normal(K)).astype(np.float32)
        x[r], y[r] = row, lab
    return x, y


def xent_cases():
    """every (N, K, eps, shift, logits, labels) of the loss tests"""
    for N, K in XENT_SHAPES:
        for eps in XENT_EPS:
            for shift in range(len(KINDS)):
                x, y = xent_case(N, K, shift)
                yield N, K, eps, shift, x, y


def loss_err(got, ref):
    """error of a mean loss relative to max(|ref|, 1)"""
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def torch_fp32_error():
    """(max loss_err, max |dlogits error|) of stock torch's fp32 CPU F.cross_entropy + autograd against xent() over xent_cases()"""
    import torch
    import torch.nn.functional as F
    worst_l = worst_d = 0.0
    for N, K, eps, shift, x, y in xent_cases():
        t = torch.from_numpy(x).clone().requires_grad_(True)
        loss = F.cross_entropy(t, torch.from_numpy(y), label_smoothing=eps)
        loss.backward()
        ref_l, _, ref_d, _, _ = xent(x, y, eps)
        worst_l = max(worst_l, loss_err(loss.item(), ref_l))
        worst_d = max(worst_d, float(np.abs(t.grad.numpy().astype(np.float64) - ref_d).max()))
    return worst_l, worst_d


# ---- the learning check: 8 synthetic images of 4 classes at 64 x 64, plain SGD, the whole set as one batch -------------------------------------------
LEARN_STEPS, LEARN_LR = 20, 1e-3


def synth_classifier(num_classes, fc_tag=2001):
    """YOLOv1Classifier with the deterministic weights of tests/golden/synth.py on its trunk (bound 1.45 sqrt(3 / fan_in): activations stay O(1)
    through the 20 LeakyReLU layers, so a wrong layer shows in the logits instead of vanishing) and sqrt(3 / 1024) on the Linear layer"""
    import torch
    import torch.nn as nn
    import synth
    from yolo import YOLOv1Classifier
    m = YOLOv1Classifier(num_classes)
    with torch.no_grad():
        for idx, mod in enumerate(m.features):
            if isinstance(mod, nn.Conv2d):
                fan = mod.in_channels * mod.kernel_size[0] ** 2
                mod.weight.copy_(torch.from_numpy(synth.synth_uniform(tuple(mod.weight.shape), 2 * idx, 1.45 * (3.0 / fan) ** 0.5)))
                mod.bias.copy_(torch.from_numpy(synth.synth_uniform(tuple(mod.bias.shape), 2 * idx + 1, 0.1)))
        m.fc.weight.copy_(torch.from_numpy(synth.synth_uniform(tuple(m.fc.weight.shape), fc_tag, (3.0 / 1024) ** 0.5)))
        m.fc.bias.copy_(torch.from_numpy(synth.synth_uniform(tuple(m.fc.bias.shape), fc_tag + 1, 0.1)))
    return m


def learning_loop(device, steps=LEARN_STEPS, lr=LEARN_LR):
    """the loss of every step of: zero_grad, forward, SoftmaxCrossEntropy, backward, SGD(lr, no momentum, no clipping) -- torch.optim.SGD on the
    CPU (the stock modules), yolo.optim.SGD on a device (the HIP path)"""
    import torch
    from yolo import SoftmaxCrossEntropy
    from yolo.dataset import SyntheticClassificationDataset
    ds = SyntheticClassificationDataset(8, 4, 64, seed=0)
    x = torch.stack([ds[i][0] for i in range(8)]).to(device)
    y = torch.tensor([ds[i][1] for i in range(8)]).to(device)
    m = synth_classifier(4).to(device).train()
    if torch.device(device).type == "cuda":
        from yolo.optim import SGD
        opt = SGD(m.parameters(), lr=lr)
    else:
        opt = torch.optim.SGD(m.parameters(), lr=lr)
    crit = SoftmaxCrossEntropy()
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss, parts = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(parts)
    return [p["total"] for p in losses]


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "yolo-v1_amd"), os.path.join(root, "tests", "golden")]
    ls = learning_loop("cpu")
    print(f"learning check on the stock CPU path: first loss {ls[0]:.4f}, loss of step {len(ls)} {ls[-1]:.4f}")
    wl, wd = torch_fp32_error()
    print(f"torch fp32 CPU cross_entropy vs fp64: loss (relative to max(|ref|, 1)) {wl:.3e}, dlogits (absolute) {wd:.3e}")
    print(f"4x: {4 * wl:.3e}, {4 * wd:.3e}")
