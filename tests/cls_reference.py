"""Float64 restatements for the classification path: MONAI 1.5.1's sigmoid focal loss (FocalLoss(to_onehot_y=True), mean reduction) with the
closed-form gradient the kernel evaluates, and the binary metrics of torchmetrics' binary task with the grouped rank sum the stats kernel evaluates.
tests/test_classification_host.py checks them against closed forms, autograd and sklearn; tests/test_classification_gpu.py checks the kernels against them."""
import numpy as np
import torch
import torch.nn.functional as F


def focal_elements(x, labels, gamma, alpha=None):
    """MONAI's arithmetic, element-wise [N, C]: bce = x - x·t - logsigmoid(x); loss = exp(γ·logsigmoid(-x·(2t-1)))·bce (× t·α + (1-t)(1-α))."""
    x = x.double()
    t = F.one_hot(labels.long(), x.shape[1]).double()
    bce = x - x * t - F.logsigmoid(x)
    loss = torch.exp(gamma * F.logsigmoid(-x * (t * 2.0 - 1.0))) * bce
    if alpha is not None:
        loss = (t * alpha + (1.0 - t) * (1.0 - alpha)) * loss
    return loss


def focal_loss(x, labels, gamma, alpha=None):
    return focal_elements(x, labels, gamma, alpha).mean()


def focal_grad(x, labels, gamma, alpha=None):
    """The kernel's closed form of d mean / d x: with z = t ? -x : x, d/dz = σ(z)^γ·(γ·σ(-z)·softplus(z) + σ(z)), times the sign of dz/dx."""
    x = x.double()
    t = F.one_hot(labels.long(), x.shape[1]).double()
    s = 1.0 - 2.0 * t
    z = s * x
    g = torch.exp(gamma * F.logsigmoid(z)) * (gamma * torch.sigmoid(-z) * F.softplus(z) + torch.sigmoid(z)) * s
    if alpha is not None:
        g = g * (t * alpha + (1.0 - t) * (1.0 - alpha))
    return g / x.numel()


def binary_stats(p1, labels):
    """(TP, FP, TN, FN, AUROC) in float64 by the stats kernel's algorithm: counts at p1 > 0.5; over p1 sorted ascending with P(k) = positives below
    position k, AUROC = Σ_neg (2·Npos - P(a) - P(b+1)) / (2·Npos·Nneg) where [a, b] is the negative's tie group; 0.0 when a class is absent."""
    p1 = np.asarray(p1, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64)
    pred = p1 > np.float32(0.5)
    tp, fp = int(np.sum(pred & (y == 1))), int(np.sum(pred & (y == 0)))
    tn, fn = int(np.sum(~pred & (y == 0))), int(np.sum(~pred & (y == 1)))
    npos, nneg = tp + fn, fp + tn
    if npos == 0 or nneg == 0:
        return float(tp), float(fp), float(tn), float(fn), 0.0
    order = np.argsort(p1, kind="stable")
    s, ys = p1[order], y[order]
    P = np.concatenate([[0], np.cumsum(ys)])                  # P[k] = positives before sorted position k
    n = len(s)
    start = np.r_[True, s[1:] != s[:-1]]
    end = np.r_[s[1:] != s[:-1], True]
    a = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    b = np.minimum.accumulate(np.where(end, np.arange(n), n)[::-1])[::-1]
    neg = ys == 0
    total = int(np.sum(2 * npos - P[a[neg]] - P[b[neg] + 1]))
    return float(tp), float(fp), float(tn), float(fn), total / (2.0 * npos * nneg)
