"""Float64 numpy restatements of the two zero-shot kernels (csrc/zero_shot.hip), shared by tests/test_zero_shot_gpu.py and tests/test_zero_shot_host.py."""
import numpy as np


def score(img, prompts, class_off):
    """logits[i, c] = mean over class c's prompts of 100 · <img_i / ||img_i||, prm_t / ||prm_t||>, all in float64 (no eps: a zero row is NaN)."""
    f = np.asarray(img, np.float64)
    t = np.asarray(prompts, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = f / np.linalg.norm(f, axis=1, keepdims=True)
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
    s = 100.0 * f @ t.T
    return np.stack([s[:, class_off[c]:class_off[c + 1]].mean(axis=1) for c in range(len(class_off) - 1)], axis=1)


def softmax(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    return e / e.sum(axis=1, keepdims=True)


def logit_bound(E):
    """Worst-case fp32 rounding of two normalisations (a norm of E terms and a division each) and an E-term dot product of unit vectors, times 100."""
    return 100.0 * (2 * E + 16) * 2.0 ** -24


def roc_curve(p1, labels):
    """(fpr, tpr, thr) as torchmetrics ROC(task="binary", thresholds=None): point 0 is (0, 0, 1.0), then one point per distinct score, descending, with the
    cumulative counts of negatives / positives scoring >= it over the class totals (an absent class: an all-zero axis).  fpr, tpr float64, thr float32."""
    p = np.asarray(p1, np.float32)
    y = np.asarray(labels, np.int64)
    order = np.argsort(-p.astype(np.float64), kind="stable")
    ps, ys = p[order], y[order]
    ends = np.r_[np.nonzero(ps[1:] != ps[:-1])[0], len(ps) - 1]
    tps = np.cumsum(ys)[ends]
    fps = ends + 1 - tps
    npos, nneg = int(ys.sum()), int(len(ys) - ys.sum())
    tpr = tps.astype(np.float64) / np.float64(npos) if npos else np.zeros(len(ends))
    fpr = fps.astype(np.float64) / np.float64(nneg) if nneg else np.zeros(len(ends))
    return np.r_[0.0, fpr], np.r_[0.0, tpr], np.r_[np.float32(1.0), ps[ends]].astype(np.float32)


def roc_inputs(N, tied, seed):
    """Scores of a split: drawn from 7 distinct values (heavy ties) or all distinct, with labels of both classes wherever N allows."""
    rng = np.random.default_rng(seed)
    if tied:
        p = rng.choice(np.linspace(0.05, 0.95, 7).astype(np.float32), N)
    else:
        p = rng.permutation(N).astype(np.float32) / np.float32(N + 1)
    y = rng.integers(0, 2, N)
    if N >= 2:
        y[0], y[1] = 0, 1
    return p.astype(np.float32), y.astype(np.int64)
